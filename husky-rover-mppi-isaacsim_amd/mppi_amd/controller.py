"""Drop-in replacement of thesis_master/warp_implementation/MPPI_isaac.py (Surface, Robot, MPPI_Controller).

Same constructors, methods and attributes as the reference class surface used by
``MPPI_Controller.run`` (MPPI_isaac.py:755-806) and by the Isaac robot loop
(visual_terrain_stack_full_terrain.py:449-576); the step runs in the HIP engine
(libmppi_hip.so) through the C-ABI in include/mppi.h.  Warp arrays become
:class:`EngineArray` objects with the methods callers use (``.numpy()``,
``.assign()``, ``.zero_()``).

There is no CPU fallback: ``warp_setup()`` raises if the HIP library or a GPU
is missing.
"""
from __future__ import annotations

import os

import numpy as np
import yaml

from . import _lib, scene
from . import sampling as _sampling
from .batch import campaign_tasks, episode_scenes, to_mppi_state

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_CONFIG = os.path.join(_HERE, "config.yaml")


def _load_config(config):
    """YAML path or mapping -> dict (MPPI_isaac.py:383-384, :406-407 use yaml.safe_load)."""
    if isinstance(config, dict):
        return config
    with open(config, "r") as f:
        return yaml.safe_load(f)


class EngineArray:
    """Host-side stand-in for a wp.array of the reference controller.

    ``numpy()`` returns a copy of the current values (fetched from the engine
    when needed); ``assign(values)`` uploads; ``zero_()`` zeroes.
    """

    def __init__(self, getter, setter=None, name=""):
        self._get = getter
        self._set = setter
        self.name = name

    def numpy(self):
        return np.array(self._get(), copy=True)

    def assign(self, values):
        if self._set is None:
            raise AttributeError(f"{self.name} is read-only")
        self._set(np.asarray(values))

    def zero_(self):
        self.assign(np.zeros_like(self.numpy()))

    def __array__(self, dtype=None, copy=None):
        a = self.numpy()
        return a.astype(dtype) if dtype is not None else a

    def __len__(self):
        return len(self._get())

    @property
    def shape(self):
        return np.shape(self._get())

    def __repr__(self):
        return f"EngineArray({self.name}, shape={self.shape})"


# =====================================================================  Surface
class Surface:
    """Scene container (MPPI_isaac.py:259-378): DEM Z, costmap and their grid geometry."""

    def __init__(self, which_map, filename, which_costmap, costmap_file, grid_size, half_width, origin,
                 bumps, radius_robot, obstacles=[]):
        self.grid_size = grid_size
        self.r_robot = radius_robot
        self.half_width = half_width
        self.resolution = 2 * self.half_width / self.grid_size            # :265
        x = np.linspace(-self.half_width, self.half_width, grid_size)
        self.X, self.Y = np.meshgrid(x, x)
        self.costmap_size = int(self.grid_size / 8)                       # :271
        self.costmap_resolution = 2 * self.half_width / self.costmap_size  # :272
        xc = np.linspace(-self.half_width, self.half_width, self.costmap_size)
        self.X_costmap, self.Y_costmap = np.meshgrid(xc, xc)
        self.Z = np.zeros_like(self.X)
        self.costmap = None
        self.obstacles = obstacles
        if which_map == "manual":
            self.X, self.Y, self.Z = self.create_surface(bumps)
        if which_map == "imported":
            self.X, self.Y, self.Z = self.import_surface(filename, 1000, 2500, bumps)
        if which_costmap == "manual":
            self.costmap = self.create_obstacles_costmap(obstacles, origin)
        if which_map == "imported" or which_costmap == "imported":
            self.costmap = self.import_obstacles_costmap(costmap_file)

    @classmethod
    def from_arrays(cls, Z, costmap, half_width, radius_robot=1.2):
        """Scene from in-memory arrays (DEM grid_size x grid_size, costmap size x size)."""
        s = cls.__new__(cls)
        Z = np.asarray(Z)
        s.grid_size = Z.shape[1]
        s.r_robot = radius_robot
        s.half_width = half_width
        s.resolution = 2 * half_width / s.grid_size
        s.Z = Z
        s.costmap = np.asarray(costmap)
        s.costmap_size = s.costmap.shape[1]
        s.costmap_resolution = 2 * half_width / s.costmap_size
        s.obstacles = []
        x = np.linspace(-half_width, half_width, s.grid_size)
        s.X, s.Y = np.meshgrid(x, x)
        xc = np.linspace(-half_width, half_width, s.costmap_size)
        s.X_costmap, s.Y_costmap = np.meshgrid(xc, xc)
        return s

    def import_surface(self, filename, start_index, end_index, bumps):
        """MPPI_isaac.py:299-305 (np.load; pickles are never loaded)."""
        x = np.linspace(-self.half_width, self.half_width, end_index - start_index)
        X, Y = np.meshgrid(x, x)
        Z = np.load(filename, allow_pickle=False)
        return X, Y, Z

    # where create_surface computes the crater field: "host" = the reference's numpy loop (default),
    # "device" = the separable float64 sum on the GPU (csrc/mppi_dem_build.hip; at most one float32
    # ulp from the host path on about one cell in 10^5)
    dem_builder = "host"

    def create_surface(self, bumps):
        """MPPI_isaac.py:307-356 (crater field)."""
        if self.dem_builder == "device":
            from . import _lib
            b = getattr(self, "_dem_builder", None)
            if b is None:
                b = self._dem_builder = _lib.DemBuilder(self.device)
            Z = b.build(bumps, self.grid_size, self.half_width).astype(np.float64)
        elif self.dem_builder == "host":
            Z = scene.crater_dem(self.grid_size, self.half_width, bumps).astype(np.float64)
        else:
            raise ValueError(f"Surface.dem_builder must be 'host' or 'device', got {self.dem_builder!r}")
        x = np.linspace(-self.half_width, self.half_width, self.grid_size)
        X, Y = np.meshgrid(x, x)
        return X, Y, Z

    def import_obstacles_costmap(self, costmap_file):
        return np.load(costmap_file, allow_pickle=False)

    # device the HIP costmap builder runs on (the reference's Warp arrays live on "cuda" = device 0)
    device = 0
    # distance metric of the costmap builder: "chamfer" = cv2.distanceTransform(DIST_L2, 5) (reference)
    costmap_metric = "chamfer"
    # steep terrain as no-go cells of the costmap: None (the reference: rocks only),
    # or a scene.Hazard / dict that MPPI_Controller.rebuild_costmap and rock-list costmap slots apply
    hazard = None

    def create_obstacles_costmap(self, obstacles, origin):
        """MPPI_isaac.py:361-378 on the GPU (csrc/mppi_costmap.hip): disc raster, cv2.distanceTransform
        (DIST_L2, 5) as OpenCV's published 5x5 chamfer, min-max normalise, (1 - d)**20; returns the
        ndarray (``costmap_metric = "exact"`` selects the exact EDT instead)."""
        from . import _lib
        b = getattr(self, "_builder", None)
        if b is None:
            b = self._builder = _lib.CostmapBuilder(self.device)
        self.obstacles = obstacles
        return b.build(obstacles, origin, self.costmap_size, self.half_width, self.r_robot, power=20,
                       metric=self.costmap_metric)


_SURFACE = object()   # rebuild_costmap(hazard=): "whatever the surface says"


# =====================================================================  Robot
class Robot:
    """MPPI_isaac.py:381-400."""

    def __init__(self, x, y, heading_vector, config_file):
        config = _load_config(config_file)
        self.x = [x]
        self.y = [y]
        self.z = [0]
        self.lin_vel = []
        self.ang_vel = []
        self.heading_vector = np.array(heading_vector) / np.linalg.norm(heading_vector)
        self.radius = config["frame_work"]["robot_radius"]
        self.left_wheel_speed = 0.0
        self.right_wheel_speed = 0.0

    def update_position(self, new_x, new_y, new_z, new_heading):
        self.x.append(new_x)
        self.y.append(new_y)
        self.z.append(new_z)
        self.heading_vector = new_heading


# =====================================================================  MPPI_Controller
class MPPI_Controller:
    """MPPI_isaac.py:402-806 on the MI355X engine.

    Extra (optional) config section ``engine:`` — ``seed`` (Philox key, default
    42 as default_rng(42) at :409), ``device`` (HIP device, default 0),
    ``max_loops`` (run(), default 3500 as :763), ``async_tail``, ``resident`` (the resident
    step server: true / 1 for back-to-back calls (default), 2 always, false / 0 never;
    mppi_set_option "resident"; env MPPI_RESIDENT wins when set),
    ``resident_idle_us`` (how long an idle server stays resident, 200: DESIGN.md §3.5),
    ``slope`` / ``w_orientation`` (the critic set) and ``sampling: {antithetic:, nominal:, beta:}``
    (the sampling plan; ``set_sampling``).
    """

    def __init__(self, surface, robot, config_path, goal_x, goal_y, goal_orientation):
        config = _load_config(config_path)
        self.config = config
        self.robot = robot
        self.surface = surface
        self.goal_x = goal_x
        self.goal_y = goal_y
        self.goal_orientation = goal_orientation
        self.loop = 0
        c, vel, inp = config["controller"], config["velocities"], config["inputs"]
        self.number_of_iterations = c["number_of_iterations"]
        self.dt = c["dt"]
        self.number_of_trajectories = c["number_of_trajectories"]
        self.initial_linear_velocity = vel["initial_linear_velocity"]
        self.std_dev_u1 = inp["std_dev_u1"]
        self.min_u1 = inp["min_u1"]
        self.max_u1 = inp["max_u1"]
        self.std_dev_u2 = inp["std_dev_u2"]
        self.min_u2 = inp["min_u2"]
        self.max_u2 = inp["max_u2"]
        self.initial_angular_velocity = vel["initial_angular_velocity"]
        self.v_min_linear = vel["min_linear_velocity"]
        self.v_max_linear = vel["max_linear_velocity"]
        self.v_min_angular = vel["min_angular_velocity"]
        self.v_max_angular = vel["max_angular_velocity"]
        self.temperature = config["cost_evaluation"]["temperature"]
        self.horizon = self.dt * self.v_max_linear * self.number_of_iterations   # :440
        eng = config.get("engine", {}) or {}
        self.seed = int(eng.get("seed", 42))
        self.device = int(eng.get("device", 0))
        self.max_loops = int(eng.get("max_loops", 3500))
        # deferred optimal rollout: MPPI_step returns with the controls and row 0 of the
        # *_sim arrays; the other rows are fetched on first access (bitwise identical)
        self.async_tail = bool(eng.get("async_tail", True))
        # the resident step server and its idle limit (mppi_set_option); the environment's
        # MPPI_RESIDENT, when set, takes precedence over the config (profiling runs turn it off)
        self.resident = None if os.environ.get("MPPI_RESIDENT") is not None or "resident" not in eng \
            else int(eng["resident"])  # (true / false, or 0 / 1 / 2: mppi_set_option "resident")
        self.resident_idle_us = eng.get("resident_idle_us")
        # the critic set (Engine.set_critics): the slope critic's mode and the orientation weight
        self.critics = dict(slope=eng.get("slope", "wheels"), w_orientation=float(eng.get("w_orientation", 0.0)))
        # the sampling plan (Engine.set_sampling): engine: {sampling: {antithetic:, nominal:, beta:}}
        self.sampling = _sampling.make_plan(**dict(eng.get("sampling") or {}))
        self.step_index = 0          # Philox step counter (replaces rng.integers at :517)
        self.engine = None
        self._out = None

    # ------------------------------------------------------------ setup
    def _params(self):
        return _lib.make_params(
            self.number_of_trajectories, self.number_of_iterations, dt=self.dt,
            robot_radius=self.robot.radius, min_u1=self.min_u1, max_u1=self.max_u1,
            min_u2=self.min_u2, max_u2=self.max_u2, v_min_linear=self.v_min_linear,
            v_max_linear=self.v_max_linear, v_min_angular=self.v_min_angular,
            v_max_angular=self.v_max_angular, temperature=self.temperature, horizon=self.horizon,
            seed=self.seed)

    def warp_setup(self):
        """MPPI_isaac.py:442-487: allocate the engine and upload DEM + costmap."""
        if self.engine is not None:
            self.engine.close()
        self.engine = _lib.Engine(self._params(), self.device)
        self.engine.set_async_tail(self.async_tail)
        if self.resident is not None:
            self.engine.set_option("resident", self.resident)
        if self.resident_idle_us is not None:
            self.engine.set_option("resident_idle_us", int(self.resident_idle_us))
        self._tail_fresh = True
        if self.critics != dict(slope="wheels", w_orientation=0.0):
            self.engine.set_critics(**self.critics)
        if not _sampling.is_default(self.sampling):
            self.engine.set_sampling(**self.sampling)
        self._upload_dem(self.surface.Z)
        self._upload_costmap(self.surface.costmap)
        H, K = self.number_of_iterations, self.number_of_trajectories
        z3 = np.zeros((H, 3), np.float32)
        self._out = dict(u1_opt=np.zeros(H, np.float32), u2_opt=np.zeros(H, np.float32),
                         lin_vel=np.full(H, self.initial_linear_velocity, np.float32),
                         ang_vel=np.full(H, self.initial_angular_velocity, np.float32),
                         traj_sim=z3, heading_sim=z3.copy(), left_wheel_sim=z3.copy(),
                         right_wheel_sim=z3.copy())
        self._dump = None
        self._cost_terms = None
        o = self._out
        self.optimal_u1_wp = EngineArray(lambda: self.engine.get_nominal()[0],
                                         lambda v: self._set_nominal(v, None), "optimal_u1_wp")
        self.optimal_u2_wp = EngineArray(lambda: self.engine.get_nominal()[1],
                                         lambda v: self._set_nominal(None, v), "optimal_u2_wp")
        self.optimal_lin_vel_wp = EngineArray(lambda: self._out["lin_vel"], name="optimal_lin_vel_wp")
        self.optimal_ang_vel_wp = EngineArray(lambda: self._out["ang_vel"], name="optimal_ang_vel_wp")
        self.trajectories_sim = EngineArray(lambda: self._sim("traj_sim"), name="trajectories_sim")
        self.heading_vectors_sim = EngineArray(lambda: self._sim("heading_sim"), name="heading_vectors_sim")
        self.left_wheel_pos_sim = EngineArray(lambda: self._sim("left_wheel_sim"), name="left_wheel_pos_sim")
        self.right_wheel_pos_sim = EngineArray(lambda: self._sim("right_wheel_sim"), name="right_wheel_pos_sim")
        self.costs_wp = EngineArray(self._costs, name="costs_wp")
        self.weights_wp = EngineArray(self._weights, name="weights_wp")
        # the four unweighted critic values of every rollout of the last step ([K, 4] in
        # _lib.COST_TERMS order) and its waypoints in collision ([K])
        self.cost_terms_wp = EngineArray(lambda: self._terms()[0], name="cost_terms_wp")
        self.collisions_wp = EngineArray(lambda: self._terms()[1], name="collisions_wp")
        self.costmap_wp = EngineArray(lambda: np.asarray(self.surface.costmap, np.float32).ravel(),
                                      self._assign_costmap, "costmap_wp")
        for name, key, shape3 in (("trajectories", "traj", True), ("heading_vectors", "hv", True),
                                  ("left_wheel_pos", "lw", True), ("right_wheel_pos", "rw", True),
                                  ("linear_velocities", "v", False), ("angular_velocities", "w", False),
                                  ("u1", "u1", False), ("u2", "u2", False)):
            setattr(self, name, EngineArray(self._dumped(key, K * H, shape3), name=name))
        self.previous_heading_vector = np.asarray(self.robot.heading_vector, np.float32)
        del o

    # ------------------------------------------------------------ device-array plumbing
    def _upload_dem(self, Z):
        """Z_wp binding (visual_terrain_stack_full_terrain.py:567: ``controller_3d.Z_wp = DEM_warp``).

        Device arrays are bound zero copy: anything exposing ``__cuda_array_interface__`` (a Warp
        array such as the terrain manager's ``dem_wp``, geometry_clipmaps.py:300/332), a CUDA
        ``torch.Tensor``, or a ``__dlpack__`` producer on the GPU.  They must be float32 and
        C-contiguous (refused otherwise: a silent copy would stop following the caller's buffer),
        1-D of n*n cells (the reference's flat dem_wp) or 2-D (rows, cols).  Host arrays (ndarray,
        ``.numpy()``/``__array__`` objects) are uploaded.  After an in-place write of a bound
        device DEM call :meth:`dem_updated` (or bind it again).
        """
        hw = self.surface.half_width
        if isinstance(Z, scene.CraterField):   # built in the engine's own DEM buffer, no upload
            self.engine.build_dem(Z, self.surface.grid_size, hw, base=Z.base, copy_out=False)
            return
        dev = _device_dem(Z)
        if dev is not None:
            ptr, rows, cols, keep = dev
            self.engine.set_dem_device(ptr, rows, cols, hw, keepalive=keep)
            return
        if hasattr(Z, "numpy") and not isinstance(Z, np.ndarray):
            Z = Z.numpy()
        Z = np.asarray(Z, np.float32)
        if Z.ndim == 1:
            n = int(round(np.sqrt(Z.size)))
            Z = Z.reshape(n, n)
        self.engine.set_dem(Z, hw)

    def dem_updated(self):
        """The bound device DEM was written in place (geometry_clipmaps.py:293 ``dem_wp.assign``):
        rebuild the per-cell normal table the rollout reads (the reference's kernels read the live
        heights at every step)."""
        self.engine.dem_updated()

    def _upload_costmap(self, cm):
        cm = np.asarray(cm, np.float32)
        if cm.ndim == 1:
            n = int(round(np.sqrt(cm.size)))
            cm = cm.reshape(n, n)
        self.engine.set_costmap(cm, self.surface.half_width, self.surface.costmap_resolution)

    def _fill_dem_slot(self, batch, slot, Z):
        """One entry of run_batch's `dems` into the batch's DEM slot: an array (uploaded), or a
        scene.CraterField, built on the device on the engine's grid."""
        if isinstance(Z, scene.CraterField):
            batch.build_dem(slot, Z, self.surface.half_width, base=Z.base)
            return
        Z = np.asarray(Z, np.float32)
        batch.set_dem(slot, Z.reshape(self.engine.dem_shape) if Z.ndim == 1 else Z)

    def _fill_costmap_slot(self, batch, slot, cm):
        """One entry of run_batch's `costmaps` into the batch's costmap slot: an array, or a rock list
        built on the device with the surface's robot radius and costmap metric.  A dict entry
        {"obstacles": ..., "origin": ..., "hazard": ..., "dem": k} adds the steep cells of DEM slot k
        (-1 or absent: the engine's DEM) by the hazard rule (absent: the surface's `hazard`); the DEM
        slots are filled first, so a crater field and its matching map never leave the device."""
        shape = self.engine.costmap_shape
        if _is_costmap_array(cm, shape):
            batch.set_costmap(slot, np.asarray(cm, np.float32).reshape(shape))
            return
        hazard, dem = getattr(self.surface, "hazard", None), -1
        if isinstance(cm, dict):
            rocks, origin = cm["obstacles"], cm.get("origin", (0.0, 0.0))
            hazard, dem = cm.get("hazard", hazard), int(cm.get("dem", -1))
        else:
            rocks, origin = cm, (0.0, 0.0)
        batch.build_costmap_hazard(slot, rocks, origin, self.surface.r_robot, hazard, dem, 20,
                                   metric=getattr(self.surface, "costmap_metric", "chamfer"))

    def _assign_costmap(self, flat):
        self.surface.costmap = np.asarray(flat, np.float32).reshape(
            self.surface.costmap_size, self.surface.costmap_size)
        self._upload_costmap(self.surface.costmap)

    def rebuild_costmap(self, obstacles, origin, hazard=_SURFACE):
        """surface.costmap = surface.create_obstacles_costmap(rocks, origin) + costmap_wp.assign(...)
        (visual_terrain_stack_full_terrain.py:561-563) in one device pass: the map is built in the
        engine's own costmap buffer (no upload) and copied back once for surface.costmap.
        hazard (default: surface.hazard; None: rocks only): the steep cells of the bound DEM, as it
        is on the device now, join the rocks.  A DEM written later (dem_updated,
        a new terrain block) does not change the map: call this again."""
        if self.engine is None:
            raise RuntimeError("call warp_setup() first")
        s = self.surface
        s.obstacles = obstacles
        if hazard is _SURFACE:
            hazard = getattr(s, "hazard", None)
        s.costmap = self.engine.build_costmap(obstacles, origin, s.costmap_size, s.half_width, s.r_robot, 20,
                                              metric=getattr(s, "costmap_metric", "chamfer"), hazard=hazard)
        return s.costmap

    @property
    def Z_wp(self):
        return EngineArray(lambda: np.asarray(self.surface.Z, np.float32).ravel(), self._upload_dem, "Z_wp")

    @Z_wp.setter
    def Z_wp(self, value):
        """controller.Z_wp = DEM_warp (visual_terrain_stack_full_terrain.py:567)."""
        self._upload_dem(value)

    @property
    def goal(self):
        return (self.goal_x, self.goal_y)

    @goal.setter
    def goal(self, value):
        self.goal_x, self.goal_y = float(value[0]), float(value[1])

    def _set_nominal(self, u1, u2):
        c1, c2 = self.engine.get_nominal()
        self.engine.set_nominal(c1 if u1 is None else u1, c2 if u2 is None else u2)

    def _sim(self, key):
        """Optimal-rollout arrays; waits for the deferred rollout on first access after a step."""
        if not self._tail_fresh:
            self._out = self.engine.outputs()
            self._tail_fresh = True
        return self._out[key]

    def _costs(self):
        return self.engine.costs()

    def _weights(self):
        """exp(-(c - min)/T) of the last step (critics_warp.py:338-347), for inspection."""
        c = self.engine.costs().astype(np.float64)
        return np.exp(-(c - c.min()) / self.temperature).astype(np.float32)

    def _terms(self):
        """(terms [K, 4], collisions [K]) of the last step, fetched once per step."""
        if self._cost_terms is None:
            self._cost_terms = self.engine.cost_terms()
        return self._cost_terms

    def set_critics(self, slope="wheels", w_orientation=0.0):
        """The critic set of the following steps (Engine.set_critics): slope "wheels" | "body", and the
        path-orientation critic's weight (0: off).  Kept across warp_setup()."""
        _lib.make_critics(slope, w_orientation)     # (ValueError before anything changes)
        self.critics = dict(slope=slope, w_orientation=float(w_orientation))
        if self.engine is not None:
            self.engine.set_critics(**self.critics)
            self._cost_terms = None

    def set_sampling(self, antithetic=False, nominal=False, beta=0.0):
        """The sampling plan of the following steps (Engine.set_sampling, mppi_amd.sampling): antithetic
        pairs, the noise-free nominal rollout as trajectory 0, AR(1) noise of coefficient beta."""
        self.sampling = _sampling.make_plan(antithetic, nominal, beta)     # (ValueError before anything changes)
        if self.engine is not None:
            self.engine.set_sampling(**self.sampling)

    def score_paths(self, traj, lin_vel, left_wheel=None, right_wheel=None, lengths=None, state=None):
        """The critics on caller-supplied paths (Engine.score_paths): logged runs
        (evaluate_trajectory.py) or any candidate plan, with this controller's costmap, weights and
        horizon; state defaults to the pose and goal of the last reset / step."""
        if self.engine is None:
            raise RuntimeError("call warp_setup() first")
        return self.engine.score_paths(traj, lin_vel, left_wheel, right_wheel, lengths, state)

    def optimal_cost(self):
        """Cost of the chosen plan (MPPI_isaac.py:726-752): the last step's optimal rollout
        (trajectories_sim, the wheel paths, optimal_lin_vel_wp) scored from the current robot pose.
        Waits for a deferred optimal rollout.  Returns (cost, terms [4])."""
        if self.engine is None:
            raise RuntimeError("call warp_setup() first")
        traj = self._sim("traj_sim")   # (first: it refreshes every *_sim array)
        r = self.engine.score_paths(traj[None], self._out["lin_vel"][None], self._out["left_wheel_sim"][None],
                                    self._out["right_wheel_sim"][None], state=self._state())
        return float(r["cost"][0]), r["terms"][0].copy()

    def _dumped(self, key, n, vec3):
        def get():
            if self._dump is None:
                self._dump = self.engine.dump()
            a = self._dump[key]
            return a.reshape(n, 3) if vec3 else a.reshape(n)
        return get

    # ------------------------------------------------------------ the step
    def _state(self):
        return _lib.make_state(self.robot.x[-1], self.robot.y[-1], self.robot.heading_vector,
                               self.robot.left_wheel_speed, self.robot.right_wheel_speed,
                               self.goal_x, self.goal_y, self.std_dev_u1, self.std_dev_u2)

    def reset(self, controller_or_sim):
        """MPPI_isaac.py:489-503.  "controller": re-read the robot pose; "sim": zero the nominal sequence."""
        if self.engine is None:
            raise RuntimeError("call warp_setup() first")
        self.previous_heading_vector = np.asarray(
            self.robot.heading_vector / np.linalg.norm(self.robot.heading_vector), np.float32)
        if controller_or_sim == "controller":
            self.engine.set_state(self._state())
        else:
            H = self.number_of_iterations
            self.engine.set_nominal(np.zeros(H, np.float32), np.zeros(H, np.float32))

    def MPPI_step(self, proj):
        """MPPI_isaac.py:505-720: one sample/rollout/cost/update step; outputs land in host memory."""
        if self.engine is None:
            raise RuntimeError("call warp_setup() first")
        self.engine.set_state(self._state())
        self._out = self.engine.step(proj, self.step_index)
        self._tail_fresh = not self.async_tail
        self._dump = None
        self._cost_terms = None
        self.step_index += 1

    # aliases requested by the drop-in contract
    def step(self, proj="3d"):
        """reset("controller") + MPPI_step(proj); returns (v0, omega0)."""
        self.reset("controller")
        self.MPPI_step(proj)
        return self.get_action()

    def get_action(self):
        """First optimal (linear, angular) velocity, as the Isaac loop reads it (:471-472)."""
        return float(self._out["lin_vel"][0]), float(self._out["ang_vel"][0])

    def run(self, proj):
        """Standalone closed loop (MPPI_isaac.py:755-806)."""
        self.warp_setup()
        while ((abs(self.robot.x[-1] - self.goal_x) > 0.5 or abs(self.robot.y[-1] - self.goal_y) > 0.5)
               and self.loop < self.max_loops):
            self.reset("controller")
            self.MPPI_step(proj=proj)
            # row 0 of the optimal rollout is returned with the step itself
            traj = self._out["traj_sim"]
            hv = self._out["heading_sim"]
            self.robot.update_position(traj[0][0], traj[0][1], traj[0][2], hv[0])
            lin_vel = self.optimal_lin_vel_wp.numpy()[0]
            ang_vel = self.optimal_ang_vel_wp.numpy()[0]
            self.std_dev_u1 = np.maximum(0.4, 0.4 - ang_vel * ang_vel)
            self.std_dev_u2 = np.maximum(0.4, 0.4 + ang_vel * ang_vel)
            self.robot.lin_vel.append(lin_vel)
            self.robot.ang_vel.append(ang_vel)
            self.robot.left_wheel_speed = lin_vel - ang_vel * self.robot.radius / 2
            self.robot.right_wheel_speed = lin_vel + ang_vel * self.robot.radius / 2
            self.loop += 1
        print("Number of loops:", self.loop)

    def _open_batch(self, E, states, seeds, variants, episode_variant, dems, costmaps, episode_dem, episode_costmap,
                    episode_trajectories):
        """The set-up run_batch and batch_stepper share: the per-episode arguments checked, then a
        _lib.Batch of E episodes with its variant table and scene slots filled and every episode set
        (states(): one MppiState per episode, asked for once the engine is up).  The caller closes it."""
        seeds = [self.seed + e for e in range(E)] if seeds is None else [int(s) for s in seeds]
        if len(seeds) != E:
            raise ValueError(f"{E} episodes but {len(seeds)} seeds")
        ev = [-1] * E if episode_variant is None else [-1 if v is None else int(v) for v in episode_variant]
        if len(ev) != E:
            raise ValueError(f"{E} episodes but {len(ev)} variant indices")
        if any(v >= 0 for v in ev) and not variants:
            raise ValueError("episode_variant names rows of `variants`, which is empty")
        ed, ec, ek = episode_scenes(E, self.number_of_trajectories, dems, costmaps, episode_dem, episode_costmap,
                                    episode_trajectories)
        if self.engine is None:
            self.warp_setup()
        states = states()
        batch = _lib.Batch(self.engine, E)
        try:
            if variants:
                batch.set_variants(variants)
            for slot, Z in enumerate(dems or []):
                self._fill_dem_slot(batch, slot, Z)
            for slot, cm in enumerate(costmaps or []):
                self._fill_costmap_slot(batch, slot, cm)
            for e in range(E):
                batch.set_episode(e, states[e], seeds[e], ev[e], ed[e], ec[e], ek[e])
        except Exception:
            batch.close()
            raise
        return batch

    def batch_stepper(self, episodes, seeds=None, variants=None, episode_variant=None, dems=None, costmaps=None,
                      episode_dem=None, episode_costmap=None, episode_trajectories=None, track=None, wheel_log=False):
        """E controllers for E rovers of an external, vectorised simulator (mppi_batch_step_device,
        DESIGN.md §3.7): the Isaac loop (visual_terrain_stack_full_terrain.py:466-515) with the poses
        kept in device tensors.  episodes: the E initial states (state dicts of mppi_amd.batch, or
        MppiState); every step replaces them with the states it is given.  seeds, variants,
        episode_variant, dems, costmaps, episode_dem, episode_costmap, episode_trajectories: as
        run_batch.

        Returns a BatchStepper: .step(states, mask=None, reset=None, seeds=None, proj="3d") ->
        (cmd [E, 2], plan [E, 4H + 12]) device tensors (Batch.step_device; the same two tensors at
        every step, so read them in stream order), .batch (the _lib.Batch) and .close().

        track: None, or the arguments of _lib.Batch.set_tracking as a dict (max_steps, and optionally
        yardstick, runs_per_episode, keep_log, goal_tol, slope, metrics): a tracked stepper, whose runs are
        logged, tested against goal and step cap, scored and ended on the device.  .step then takes z= and
        done= and returns (cmd, plan, done); .runs() reads the results once the campaign is over.
        slope="wheels" scores the slope term over the wheel contacts the ingest forms from each pose,
        metrics=True adds compute_path_metrics per run; wheel_log=True keeps the contacts beside the log
        (.batch.wheel_log(e)); it needs `track` with keep_log, and is refused without `track`.
        """
        if wheel_log and track is None:
            raise ValueError("wheel_log=True needs track=...: the plain device step keeps no log")
        states = [s if isinstance(s, _lib.MppiState) else to_mppi_state(s) for s in episodes]
        batch = self._open_batch(len(states), lambda: states, seeds, variants, episode_variant, dems, costmaps, episode_dem,
                                 episode_costmap, episode_trajectories)
        if track is not None:
            try:
                if wheel_log:
                    batch.set_wheel_log()
                batch.set_tracking(**dict(track))
            except Exception:
                batch.close()
                raise
        return BatchStepper(batch)

    def run_batch(self, starts, headings, goals, seeds=None, proj="3d", max_loops=None, policy=None,
                  variants=None, episode_variant=None, score=None, dems=None, costmaps=None, episode_dem=None,
                  episode_costmap=None, episode_trajectories=None, slope="body", metrics=False, wheel_log=False):
        """run() for many episodes at once on this controller's surface and parameters (mppi_batch_*,
        DESIGN.md §3.7): episode e starts at starts[e] = (x, y) with heading headings[e] (normalised
        as Robot does), wheels at rest and the controller's std_dev_u1 / std_dev_u2, and drives to
        goals[e] = (x, y); the loop's state feedback runs on the GPU, no host work between steps.

        seeds: Philox key per episode (default the controller's seed + e); max_loops: the step cap
        (default the controller's); policy: dict(sigma_base, sigma_div, goal_tol[, check_every])
        (default run()'s).  The robot and the controller's own loop state are not touched.

        variants: the batch's variant table, a list of _lib.MppiBatchVariant or dicts
        (_lib.make_variant's arguments: weights, collision_threshold / _penalty, temperature, the two
        filters, sigma_base / sigma_div, proj); episode_variant[e]: the row episode e runs with
        (-1 or None: the controller's parameters, `proj` and `policy`).  A weight sweep or the paired
        2D / 3D runs of evaluate_trajectory.py are then one batch.  score: True (the controller's
        weights) or a yardstick (variant or dict): every executed path is scored on the device with
        that one cost function (mppi_batch_score), each on its own episode's costmap.

        dems: DEMs of the surface's shape, or scene.CraterField values, built on the device on the
        surface's grid (mppi_batch_build_dem: a Monte-Carlo over crater fields uploads no terrain); costmaps: costmaps of the surface's costmap shape (2-D, or
        flat as costmap_wp) or rock lists, built on the device as Surface.create_obstacles_costmap
        builds them ([[x, y, r], ...] about the origin (0, 0), or dict(obstacles=..., origin=(x, y)));
        they fill the batch's scene slots in list order.  episode_dem[e] / episode_costmap[e]: the
        slot episode e runs on (-1 or None: the controller's own surface); episode_trajectories[e]:
        its number of rollouts per step, in [1, number_of_trajectories] (0 or None: all of them).  A
        Monte-Carlo over rock fields, the "rocks removed" comparison and the K = 1000 / 500 / 350
        series are then one batch.

        Returns one dict per episode: x, y, z, lin_vel, ang_vel (the lists Robot accumulates: x, y, z
        begin with the start pose and z = 0), loops, reached; with `score` the pair (that list,
        dict(cost [E], terms [E, 4], collisions [E], rows [E])).

        slope="wheels" (with `score`): the slope term is the controller's own wheel form, over the wheel
        contacts of every executed step (they exist under both projections, so one wheel yardstick serves
        a 2D-vs-3D comparison); metrics=True: the scores also hold `metrics` [E, 4], compute_path_metrics
        of every path (mppi_amd.batch.METRICS_FIELDS).  wheel_log=True (implied by slope="wheels", which
        scores the kept contacts after the run): every episode's dict also holds `wheels` [loops, 6], the
        contacts lx, ly, lz, rx, ry, rz of each step.  slope / metrics without `score` are refused.
        """
        if (slope != "body" or metrics) and (score is None or score is False):
            raise ValueError("slope / metrics belong to `score`: give score=True or a yardstick")
        wheel_log = bool(wheel_log) or slope == "wheels"
        starts = np.asarray(starts, np.float64).reshape(-1, 2)
        E = starts.shape[0]
        headings = np.asarray(headings, np.float64).reshape(E, 3)
        goals = np.asarray(goals, np.float64).reshape(E, 2)
        pol = _lib.make_policy(**(policy or {}))
        batch = self._open_batch(
            E, lambda: [_lib.make_state(starts[e, 0], starts[e, 1], headings[e], 0.0, 0.0, goals[e, 0], goals[e, 1],
                                        self.std_dev_u1, self.std_dev_u2) for e in range(E)],
            seeds, variants, episode_variant, dems, costmaps, episode_dem, episode_costmap, episode_trajectories)
        try:
            if wheel_log:
                batch.set_wheel_log()
            batch.run(self.max_loops if max_loops is None else int(max_loops), proj, pol)
            out = []
            for e in range(E):
                info = batch.episode(e)
                rows = batch.log(e, 0, info["steps_last_run"])
                out.append(dict(x=[starts[e, 0]] + list(rows[:, 0]), y=[starts[e, 1]] + list(rows[:, 1]),
                                z=[0] + list(rows[:, 2]), lin_vel=list(rows[:, 6]), ang_vel=list(rows[:, 7]),
                                loops=info["steps_last_run"], reached=info["reached"]))
                if wheel_log:
                    out[-1]["wheels"] = batch.wheel_log(e, 0, info["steps_last_run"])
            if score is None or score is False:
                return out
            return out, batch.score(None if score is True else score, slope=slope, metrics=metrics)
        finally:
            batch.close()

    def run_campaign(self, starts, headings, goals, seeds=None, lanes=64, max_loops=None, proj="3d", policy=None,
                     variants=None, task_variant=None, score=None, dems=None, costmaps=None, task_dem=None,
                     task_costmap=None, task_trajectories=None, log=True, slope="body", metrics=False,
                     wheel_log=False):
        """run_batch for N tasks on `lanes` episodes (mppi_batch_set_tasks / _run_tasks):
        the lane whose task ends (goal reached, or its step cap) takes the next task of the list on the
        GPU in the same step, so a campaign of runs of very different lengths keeps every lane busy
        and costs no host work between its runs.  Every task's trail is the one run_batch gives the
        same start, goal, seed, variant, scene and trajectory count as an episode.

        starts / headings / goals / seeds / proj / policy / variants / dems / costmaps / score: as
        run_batch, per task.  max_loops: one step cap for every task (default the controller's) or
        one per task.  task_variant / task_dem / task_costmap / task_trajectories: run_batch's
        episode_* arguments, per task.  lanes: the episodes the campaign runs on (at most the tasks).

        With `score` the lanes score their tasks as they run (mppi_batch_set_tasks_scored): the scores
        are those of the log scorer, bit for bit, with each task's `length` (mppi_amd.batch.path_length
        of its log) beside them.  log=False (needs `score`): no log arena is allocated, so a campaign's
        size is not bounded by the sum of its step caps; the per-task dicts then hold `loops`,
        `reached` and the final `x`, `y` only.

        slope="wheels" / metrics=True (with `score`): the online score's slope term in the wheel form, and
        `metrics` [N, 4] beside the scores (campaign_summary then reports their per-variant means); both
        work with log=False, and slope="wheels" does not turn the wheel log on here: the lanes extend the
        chain by the contacts as they run.  wheel_log=True (needs log): each task's dict also holds `wheels`
        [loops, 6].  slope / metrics without `score` are refused.

        Returns what run_batch returns, one dict per task (with `score` the pair; mppi_amd.batch
        campaign_results / campaign_summary turn the pair into the per-variant table).
        """
        scored = not (score is None or score is False)
        if (slope != "body" or metrics) and not scored:
            raise ValueError("slope / metrics belong to `score`: give score=True or a yardstick")
        if not log and not scored:
            raise ValueError("log=False needs score=True or a yardstick: without a log nothing else is kept of a run")
        starts = np.asarray(starts, np.float64).reshape(-1, 2)
        N = starts.shape[0]
        headings = np.asarray(headings, np.float64).reshape(N, 3)
        goals = np.asarray(goals, np.float64).reshape(N, 2)
        seeds = [self.seed + i for i in range(N)] if seeds is None else [int(s) for s in seeds]
        if len(seeds) != N:
            raise ValueError(f"{N} tasks but {len(seeds)} seeds")
        tv, td, tc, tk, caps = campaign_tasks(N, self.number_of_trajectories,
                                              self.max_loops if max_loops is None else max_loops, variants, dems,
                                              costmaps, task_variant, task_dem, task_costmap, task_trajectories)
        if int(lanes) < 1:
            raise ValueError("lanes must be >= 1")
        if self.engine is None:
            self.warp_setup()
        pol = _lib.make_policy(**(policy or {}))
        batch = _lib.Batch(self.engine, min(int(lanes), N))
        try:
            if variants:
                batch.set_variants(variants)
            for slot, Z in enumerate(dems or []):
                self._fill_dem_slot(batch, slot, Z)
            for slot, cm in enumerate(costmaps or []):
                self._fill_costmap_slot(batch, slot, cm)
            if wheel_log:
                if not log:
                    raise ValueError("wheel_log=True needs log=True: the contacts are kept beside the log rows")
                batch.set_wheel_log()
            batch.set_tasks([_lib.make_task(_lib.make_state(starts[i, 0], starts[i, 1], headings[i], 0.0, 0.0,
                                                            goals[i, 0], goals[i, 1], self.std_dev_u1,
                                                            self.std_dev_u2),
                                            seeds[i], caps[i], tv[i], td[i], tc[i], tk[i]) for i in range(N)],
                            scored=score if scored else None, keep_log=bool(log), slope=slope, metrics=bool(metrics))
            done = 0
            while done < N:     # every task ends within its cap, so the campaign ends
                done, _ = batch.run_tasks(max(caps), proj, pol)
            out = []
            for i in range(N):
                info = batch.task(i)
                if not log:
                    out.append(dict(x=info["state"].x, y=info["state"].y, loops=info["steps"],
                                    reached=info["reached"]))
                    continue
                rows = batch.task_log(i, 0, info["steps"])
                out.append(dict(x=[starts[i, 0]] + list(rows[:, 0]), y=[starts[i, 1]] + list(rows[:, 1]),
                                z=[0] + list(rows[:, 2]), lin_vel=list(rows[:, 6]), ang_vel=list(rows[:, 7]),
                                loops=info["steps"], reached=info["reached"]))
                if wheel_log:
                    out[-1]["wheels"] = batch.task_wheel_log(i, 0, info["steps"])
            if not scored:
                return out
            return out, batch.task_scores()
        finally:
            batch.close()


class BatchStepper:
    """What MPPI_Controller.batch_stepper returns: a filled _lib.Batch stepped from device tensors.
    cmd and plan are allocated once, at the first step, and reused."""

    def __init__(self, batch):
        self.batch = batch
        self.cmd = None
        self.plan = None
        self.done = None

    def step(self, states, mask=None, reset=None, seeds=None, proj="3d", z=None, done=None):
        """Batch.step_device with the stepper's own cmd / plan tensors; never synchronises.  A tracked
        stepper (batch_stepper(track=...)) passes z and done through (done: the stepper's own tensor
        when not given) and returns (cmd, plan, done)."""
        if not getattr(self.batch, "tracking", None):
            self.cmd, self.plan = self.batch.step_device(states, mask, reset, seeds, self.cmd, self.plan, proj, z, done)
            return self.cmd, self.plan
        self.cmd, self.plan, self.done = self.batch.step_device(states, mask, reset, seeds, self.cmd, self.plan, proj, z,
                                                                self.done if done is None else done)
        return self.cmd, self.plan, self.done

    def runs(self, e=None):
        """Batch.runs: the result rows of the tracked runs (synchronises)."""
        return self.batch.runs(e)

    def close(self):
        self.batch.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _is_costmap_array(cm, shape):
    """A costmap given as an array (2-D of `shape`, or flat) rather than as a rock list."""
    if isinstance(cm, dict):
        return False
    a = np.asarray(cm)
    return a.shape == tuple(shape) or (a.ndim == 1 and a.size == shape[0] * shape[1])


def _grid_shape(shape):
    """(rows, cols) of a DEM buffer: 2-D as given, 1-D of n*n cells as n x n."""
    if len(shape) == 2:
        return int(shape[0]), int(shape[1])
    if len(shape) == 1:
        n = int(round(np.sqrt(shape[0])))
        if n * n != shape[0]:
            raise ValueError(f"1-D DEM of {shape[0]} cells is not square")
        return n, n
    raise ValueError(f"DEM must be 1-D (n*n) or 2-D, got shape {tuple(shape)}")


def _device_dem(Z):
    """(device pointer, rows, cols, keepalive) for a GPU-resident float32 C-contiguous DEM, None for a
    host array; raises for a device array that would need a copy."""
    dev = _lib.device_array(Z, "device DEM")   # (the rules Batch.step_device applies to its arrays)
    if dev is None:
        return None
    ptr, shape, keep, _ = dev
    rows, cols = _grid_shape(shape)
    return ptr, rows, cols, keep
