"""ctypes binding of libmppi_hip.so (include/mppi.h).

The product path has no fallback: if the HIP library is missing or no GPU is
visible, every entry point raises.  Build it with ``python -c "import
__graft_entry__ as g; g.build()"`` (or ``make -C husky-rover-mppi-isaacsim_amd/csrc``).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MPPI_LIB_PATH: an alternative build of the same library (diagnostic A/B builds)
LIB_PATH = os.environ.get("MPPI_LIB_PATH") or os.path.join(_HERE, "libmppi_hip.so")

MPPI_OK = 0
PROJ = {"2d": 2, "3d": 3, 2: 2, 3: 3}


class MppiParams(C.Structure):
    _fields_ = [
        ("num_trajectories", C.c_int64),
        ("k_offset", C.c_int64),
        ("num_iterations", C.c_int32),
        ("reserved0", C.c_int32),
        ("dt", C.c_float),
        ("robot_radius", C.c_float),
        ("min_u1", C.c_float), ("max_u1", C.c_float),
        ("min_u2", C.c_float), ("max_u2", C.c_float),
        ("v_min_linear", C.c_float), ("v_max_linear", C.c_float),
        ("v_min_angular", C.c_float), ("v_max_angular", C.c_float),
        ("temperature", C.c_float),
        ("filter_k", C.c_float), ("filter_a", C.c_float),
        ("opt_filter_k", C.c_float), ("opt_filter_a", C.c_float),
        ("wheel_offset", C.c_float),
        ("w_path", C.c_float), ("w_slope", C.c_float), ("w_speed", C.c_float),
        ("w_obstacle", C.c_float),
        ("collision_threshold", C.c_float), ("collision_penalty", C.c_float),
        ("horizon", C.c_float),
        ("seed", C.c_uint64),
    ]


class MppiState(C.Structure):
    _fields_ = [
        ("x", C.c_float), ("y", C.c_float),
        ("heading", C.c_float * 3),
        ("left_wheel_speed", C.c_float), ("right_wheel_speed", C.c_float),
        ("goal_x", C.c_float), ("goal_y", C.c_float),
        ("std_dev_u1", C.c_float), ("std_dev_u2", C.c_float),
    ]


_FP = C.POINTER(C.c_float)
_DP = C.POINTER(C.c_double)


class MppiOutputs(C.Structure):
    _fields_ = [(n, _FP) for n in ("u1_opt", "u2_opt", "lin_vel", "ang_vel", "traj_sim",
                                   "heading_sim", "left_wheel_sim", "right_wheel_sim")]


class MppiPathScores(C.Structure):
    """mppi_path_scores: host output pointers of mppi_score_paths (any may be NULL)."""
    _fields_ = [("cost", _FP), ("terms", _FP), ("collisions", C.POINTER(C.c_int32))]


class MppiLoopPolicy(C.Structure):
    """mppi_loop_policy: the closed loop's sigma schedule and goal test (mppi_batch_run)."""
    _fields_ = [("sigma_base", C.c_float), ("sigma_div", C.c_float), ("goal_tol", C.c_float),
                ("check_every", C.c_int32)]


VARIANT_FIELDS = ("w_path", "w_slope", "w_speed", "w_obstacle", "collision_threshold", "collision_penalty",
                  "temperature", "filter_k", "filter_a", "opt_filter_k", "opt_filter_a", "sigma_base", "sigma_div")


class MppiBatchVariant(C.Structure):
    """mppi_batch_variant: the parameters one episode of a batch may override (56 bytes)."""
    _fields_ = [(n, C.c_float) for n in VARIANT_FIELDS] + [("proj", C.c_int32)]


class MppiBatchTask(C.Structure):
    """mppi_batch_task: one task of a batch's task list (88 bytes)."""
    _fields_ = [("start", MppiState), ("seed", C.c_uint64), ("variant", C.c_int32), ("dem_slot", C.c_int32),
                ("costmap_slot", C.c_int32), ("num_trajectories", C.c_int64), ("max_steps", C.c_int32)]


class MppiBatchIo(C.Structure):
    """mppi_batch_io: the device pointers of one mppi_batch_step_device call (any but states may be NULL)."""
    _fields_ = [(n, C.c_void_p) for n in ("states", "mask", "reset", "seeds", "cmd", "plan")]


class MppiCritics(C.Structure):
    """mppi_critics: the critic set of a context or of a variant row (8 bytes)."""
    _fields_ = [("slope_mode", C.c_int32), ("w_orientation", C.c_float)]


class MppiHazard(C.Structure):
    """mppi_hazard (include/mppi.h): the steep-terrain part of a hazard costmap."""
    _fields_ = [("max_slope_deg", C.c_float), ("inflate", C.c_float), ("min_cells", C.c_int32),
                ("reserved", C.c_int32)]


class MppiSampling(C.Structure):
    """mppi_sampling: the sampling plan of a context or of a variant row (12 bytes)."""
    _fields_ = [("antithetic", C.c_int32), ("nominal", C.c_int32), ("beta", C.c_float)]


COST_TERMS = ("path", "slope", "speed", "obstacle")   # mppi_cost_term order (include/mppi.h)
COST_TERMS5 = COST_TERMS + ("orientation",)           # mppi_get_cost_terms5
SLOPE_MODES = {"wheels": 0, "body": 1}                # mppi_slope_mode


# name -> (restype, argtypes); must match include/mppi.h (tests/test_lib_symbols.py checks both ways)
_PROTOS = {
    "mppi_abi_version": (C.c_int, []),
    "mppi_last_error": (C.c_char_p, []),
    "mppi_create": (C.c_int, [C.POINTER(MppiParams), C.c_int32, C.POINTER(C.c_void_p)]),
    "mppi_destroy": (None, [C.c_void_p]),
    "mppi_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mppi_set_dem": (C.c_int, [C.c_void_p, _FP, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float]),
    "mppi_dem_updated": (C.c_int, [C.c_void_p]),
    "mppi_set_dem_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float,
                                      C.c_float, C.c_float]),
    "mppi_set_costmap": (C.c_int, [C.c_void_p, _FP, C.c_int32, C.c_float, C.c_float]),
    "mppi_set_state": (C.c_int, [C.c_void_p, C.POINTER(MppiState)]),
    "mppi_set_nominal": (C.c_int, [C.c_void_p, _FP, _FP]),
    "mppi_get_nominal": (C.c_int, [C.c_void_p, _FP, _FP]),
    "mppi_step": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint64, C.POINTER(MppiOutputs)]),
    "mppi_step_injected": (C.c_int, [C.c_void_p, C.c_int32, _FP, _FP, C.POINTER(MppiOutputs)]),
    "mppi_set_async_tail": (C.c_int, [C.c_void_p, C.c_int32]),
    "mppi_get_outputs": (C.c_int, [C.c_void_p, C.POINTER(MppiOutputs)]),
    "mppi_record_len": (C.c_int64, [C.c_void_p]),
    "mppi_step_partial": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p]),
    "mppi_step_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(MppiOutputs)]),
    "mppi_get_costs": (C.c_int, [C.c_void_p, _FP, C.c_int64]),
    "mppi_dump_rollouts": (C.c_int, [C.c_void_p] + [_FP] * 8),
    "mppi_score_paths": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_int32), _FP, _FP, _FP, _FP,
                                   C.POINTER(MppiState), C.POINTER(MppiPathScores)]),
    "mppi_get_cost_terms": (C.c_int, [C.c_void_p, _FP, C.POINTER(C.c_int32)]),
    "mppi_get_cost_terms5": (C.c_int, [C.c_void_p, _FP, C.POINTER(C.c_int32)]),
    "mppi_set_critics": (C.c_int, [C.c_void_p, C.POINTER(MppiCritics)]),
    "mppi_get_critics": (C.c_int, [C.c_void_p, C.POINTER(MppiCritics)]),
    "mppi_batch_set_variant_critics": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(MppiCritics)]),
    "mppi_set_sampling": (C.c_int, [C.c_void_p, C.POINTER(MppiSampling)]),
    "mppi_get_sampling": (C.c_int, [C.c_void_p, C.POINTER(MppiSampling)]),
    "mppi_batch_set_variant_sampling": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(MppiSampling)]),
    "mppi_get_score_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "mppi_set_timing": (C.c_int, [C.c_void_p, C.c_int32]),
    "mppi_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
    "mppi_get_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                  C.POINTER(C.c_int64)]),
    "mppi_get_tail_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "mppi_get_launch_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int32]),
    "mppi_get_chain_clock": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int32]),
    "mppi_get_server_time": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.POINTER(C.c_int64)]),
    "mppi_bilinear_query": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "mppi_selftest": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.POINTER(C.c_int64)]),
    "mppi_bilinear_tiles": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "mppi_bin_queries": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "mppi_bilinear_tiled": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mppi_sync": (C.c_int, [C.c_void_p]),
    "mppi_debug_hold": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "mppi_build_costmap": (C.c_int, [C.c_void_p, _DP, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                     C.c_double, C.c_double, C.c_int32, _FP, C.c_int32]),
    "mppi_costmap_builder_create": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    "mppi_costmap_builder_destroy": (None, [C.c_void_p]),
    "mppi_costmap_builder_build": (C.c_int, [C.c_void_p, _DP, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                             C.c_double, C.c_double, C.c_int32, _FP, C.c_void_p, C.c_int32]),
    "mppi_costmap_builder_last_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "mppi_build_costmap_hazard": (C.c_int, [C.c_void_p, _DP, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                            C.c_double, C.c_double, C.c_int32, C.POINTER(MppiHazard), _FP,
                                            C.POINTER(C.c_uint8), C.c_int32]),
    "mppi_costmap_builder_build_hazard": (C.c_int, [C.c_void_p, _DP, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                                    C.c_double, C.c_double, C.c_int32, C.c_void_p, C.c_int32,
                                                    C.c_int32, C.c_float, C.c_float, C.c_float,
                                                    C.POINTER(MppiHazard), _FP, C.c_void_p, C.POINTER(C.c_uint8),
                                                    C.c_int32]),
    "mppi_costmap_builder_hazard_count_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "mppi_dem_builder_create": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    "mppi_dem_builder_destroy": (None, [C.c_void_p]),
    "mppi_dem_builder_build": (C.c_int, [C.c_void_p, _DP, C.c_int32, C.c_int32, C.c_double, _FP, _FP, C.c_void_p,
                                         C.c_int32]),
    "mppi_dem_builder_last_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "mppi_dem_builder_product": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, _FP,
                                           C.c_void_p, C.c_int32]),
    "mppi_build_dem": (C.c_int, [C.c_void_p, _DP, C.c_int32, C.c_int32, C.c_double, _FP, _FP, C.c_int32]),
    "mppi_batch_build_dem": (C.c_int, [C.c_void_p, C.c_int32, _DP, C.c_int32, C.c_double, _FP, _FP, C.c_int32]),
    "mppi_group_create": (C.c_int, [C.POINTER(MppiParams), C.c_int32, C.POINTER(C.c_int32),
                                    C.POINTER(C.c_void_p)]),
    "mppi_group_destroy": (None, [C.c_void_p]),
    "mppi_group_size": (C.c_int, [C.c_void_p]),
    "mppi_group_context": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "mppi_group_shard": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mppi_group_step": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint64, C.POINTER(MppiOutputs)]),
    "mppi_group_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int32]),
    "mppi_group_selftest": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "mppi_batch_create": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "mppi_batch_destroy": (None, [C.c_void_p]),
    "mppi_batch_set_episode": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(MppiState), C.c_uint64]),
    "mppi_batch_run": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(MppiLoopPolicy)]),
    "mppi_batch_get_episode": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(MppiState), C.POINTER(C.c_int64),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32), _FP, _FP]),
    "mppi_batch_step_device": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(MppiBatchIo)]),
    "mppi_batch_set_tracking": (C.c_int, [C.c_void_p, C.POINTER(MppiBatchVariant), C.c_float, C.c_int32, C.c_int32,
                                          C.c_int32]),
    "mppi_batch_step_tracked": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(MppiBatchIo), C.c_void_p, C.c_void_p]),
    "mppi_batch_get_runs": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(MppiState),
                                      C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                      C.POINTER(MppiPathScores), C.POINTER(C.c_int32), _DP]),
    "mppi_batch_get_run_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "mppi_batch_get_log": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _FP]),
    "mppi_batch_get_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "mppi_batch_variant_default": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(MppiLoopPolicy),
                                             C.POINTER(MppiBatchVariant)]),
    "mppi_batch_set_variants": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(MppiBatchVariant)]),
    "mppi_batch_set_episode_variant": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "mppi_batch_set_dem": (C.c_int, [C.c_void_p, C.c_int32, _FP]),
    "mppi_batch_set_costmap": (C.c_int, [C.c_void_p, C.c_int32, _FP]),
    "mppi_batch_build_costmap": (C.c_int, [C.c_void_p, C.c_int32, _DP, C.c_int32, C.c_double, C.c_double,
                                           C.c_double, C.c_int32, C.c_int32, _FP]),
    "mppi_batch_build_costmap_hazard": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _DP, C.c_int32, C.c_double,
                                                  C.c_double, C.c_double, C.c_int32, C.c_int32,
                                                  C.POINTER(MppiHazard), _FP, C.POINTER(C.c_uint8)]),
    "mppi_batch_set_episode_scene": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "mppi_batch_set_episode_trajectories": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64]),
    "mppi_batch_score": (C.c_int, [C.c_void_p, C.POINTER(MppiBatchVariant), C.POINTER(MppiState),
                                   C.POINTER(MppiPathScores), C.POINTER(C.c_int32)]),
    "mppi_batch_set_tasks": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(MppiBatchTask)]),
    "mppi_batch_run_tasks": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(MppiLoopPolicy),
                                       C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "mppi_batch_get_task": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(MppiState), C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mppi_batch_get_task_log": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _FP]),
    "mppi_batch_score_tasks": (C.c_int, [C.c_void_p, C.POINTER(MppiBatchVariant), C.POINTER(MppiState),
                                         C.POINTER(MppiPathScores), C.POINTER(C.c_int32)]),
    "mppi_batch_set_tasks_scored": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(MppiBatchTask),
                                              C.POINTER(MppiBatchVariant), C.c_int32]),
    "mppi_batch_get_task_scores": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(MppiPathScores),
                                             C.POINTER(C.c_int32), _DP]),
    "mppi_batch_set_wheel_log": (C.c_int, [C.c_void_p, C.c_int32]),
    "mppi_batch_get_wheel_log": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _FP]),
    "mppi_batch_get_task_wheel_log": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _FP]),
    "mppi_batch_score_ex": (C.c_int, [C.c_void_p, C.POINTER(MppiBatchVariant), C.POINTER(MppiState), C.c_int32,
                                      C.POINTER(MppiPathScores), C.POINTER(C.c_int32), _DP]),
    "mppi_batch_score_tasks_ex": (C.c_int, [C.c_void_p, C.POINTER(MppiBatchVariant), C.POINTER(MppiState), C.c_int32,
                                            C.POINTER(MppiPathScores), C.POINTER(C.c_int32), _DP]),
    "mppi_batch_set_score_options": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "mppi_batch_get_task_metrics": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _DP]),
    "mppi_batch_get_run_metrics": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _DP]),
    "mppi_detmath_atan2": (C.c_int, [C.c_void_p, C.c_int64, _DP, _DP, _DP, _DP]),
    "mppi_rollout_python25d": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, _DP, _DP, _DP, _DP, _DP, C.c_double,
                                         C.c_double, C.c_double, C.c_double, _DP, C.POINTER(C.c_int32)]),
}

_lib = None


def load_library(path: str = LIB_PATH):
    """Load libmppi_hip.so and declare its prototypes (raises if it is missing)."""
    global _lib
    if _lib is not None and path == LIB_PATH:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError(
            f"HIP engine library not found at {path}; build it with "
            "`make -C husky-rover-mppi-isaacsim_amd/csrc` (no CPU fallback exists)")
    # PyTorch-ROCm bundles its own libamdhip64.so.7.  Load it first so that the
    # engine's NEEDED libamdhip64.so.7 resolves to the same runtime: a second
    # HIP/HSA runtime in the process would make torch.cuda fail to initialise
    # ("No HIP GPUs are available") once the engine has claimed the device.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.mppi_abi_version() != 1:
        raise RuntimeError("libmppi_hip.so ABI mismatch")
    if path == LIB_PATH:
        _lib = lib
    return lib


def _fp(a):
    return a.ctypes.data_as(_FP)


_DTYPE_NAMES = {"f4": "float32", "i4": "int32", "u8": "uint64", "i8": "int64"}


def device_array(a, what, codes=("f4",)):
    """(device pointer, shape, keepalive, device index or None) of a GPU-resident array, taken zero
    copy; None for anything that is not one (a host array).

    Accepted: an object exposing ``__cuda_array_interface__`` (a Warp array), a CUDA
    ``torch.Tensor``, or a ``__dlpack__`` producer on the GPU (viewed as a tensor, no copy).  The
    element type must be one of `codes` (array-interface codes: "f4", "i4", "u8", "i8") and the array
    C-contiguous: ValueError otherwise, naming `what` (a silent copy would stop following the
    caller's buffer).  The device index is known for tensors only.
    """
    want = " or ".join(_DTYPE_NAMES[c] for c in codes)
    cai = getattr(a, "__cuda_array_interface__", None)
    if cai is not None:
        shape = tuple(int(n) for n in cai["shape"])
        ts = cai.get("typestr")
        if not isinstance(ts, str) or ts.lstrip("<=|") not in codes:
            raise ValueError(f"{what} must be {want}, got typestr {ts!r}")
        item = int(ts.lstrip("<=|")[1:])
        strides = cai.get("strides")
        if strides is not None and tuple(strides) != tuple(
                item * int(np.prod(shape[i + 1:])) for i in range(len(shape))):
            raise ValueError(f"{what} must be C-contiguous, got strides {strides}")
        return int(cai["data"][0]), shape, a, None
    try:
        import torch
    except ImportError:
        return None
    if not isinstance(a, torch.Tensor) and hasattr(a, "__dlpack__"):
        dev = a.__dlpack_device__()[0] if hasattr(a, "__dlpack_device__") else None
        if dev in (2, 10):  # kDLCUDA, kDLROCM: a device producer, viewed as a tensor (no copy)
            a = torch.from_dlpack(a)
    if isinstance(a, torch.Tensor) and a.is_cuda:
        ok = [getattr(torch, _DTYPE_NAMES[c]) for c in codes if hasattr(torch, _DTYPE_NAMES[c])]
        if a.dtype not in ok:
            raise ValueError(f"{what} must be {want}, got {a.dtype}")
        if not a.is_contiguous():
            raise ValueError(f"{what} must be contiguous (pass a contiguous buffer: a copy would not "
                             "follow the caller's updates)")
        return a.data_ptr(), tuple(int(n) for n in a.shape), a, a.device.index
    return None


def _obstacles(obstacles):
    """Obstacle list [(x_global, y_global, r_obs), ...] -> contiguous float64 [n, 3] (n may be 0)."""
    a = np.ascontiguousarray(np.asarray(obstacles, dtype=np.float64).reshape(-1, 3))
    return a, a.ctypes.data_as(_DP)


COSTMAP_METRICS = {"chamfer": 0, "exact": 1, "chamfer_raster": 2}   # mppi_costmap_metric (include/mppi.h)


def _metric(m):
    if m not in COSTMAP_METRICS:
        raise ValueError(f"costmap metric must be one of {sorted(COSTMAP_METRICS)}, got {m!r}")
    return COSTMAP_METRICS[m]


def make_hazard(hazard, r_robot):
    """A hazard given as a dict or a scene.Hazard (max_slope_deg, inflate=None, min_cells=1) -> MppiHazard,
    or None for None.  inflate None: r_robot + 0.1, the margin the reference gives its rocks."""
    if hazard is None:
        return None
    if isinstance(hazard, MppiHazard):
        return hazard
    if isinstance(hazard, dict):
        unknown = set(hazard) - {"max_slope_deg", "inflate", "min_cells"}
        if unknown or "max_slope_deg" not in hazard:
            raise ValueError(f"hazard: expected max_slope_deg and optionally inflate, min_cells; got {sorted(hazard)}")
        get = hazard.get
    else:
        get = lambda k, d=None: getattr(hazard, k, d)   # noqa: E731
    inflate = get("inflate", None)
    return MppiHazard(float(get("max_slope_deg")), float(r_robot) + 0.1 if inflate is None else float(inflate),
                      int(get("min_cells", 1)), 0)


def _mask(size, want):
    m = np.empty((int(size), int(size)), np.uint8) if want else None
    return m, (None if m is None else m.ctypes.data_as(C.POINTER(C.c_uint8)))


class CostmapBuilder:
    """Surface.create_obstacles_costmap (MPPI_isaac.py:361-378) on the GPU, no controller context needed.

    build(...) returns the size x size float32 costmap as an ndarray (the reference returns one);
    with out_device=<pointer> the map is written to caller-owned device memory instead.
    With hazard= and dem=(z_device, rows, cols, x_min, y_min, resolution) the steep cells of those
    device-resident heights join the rocks; return_mask adds the uint8 mask
    (bit 0 H0, bit 1 H1, bit 2 rock disc) as a second result.
    """

    def __init__(self, device: int = 0):
        self.lib = load_library()
        self.device = int(device)
        h = C.c_void_p()
        _check(self.lib, self.lib.mppi_costmap_builder_create(self.device, C.byref(h)),
               "mppi_costmap_builder_create")
        self.h = h

    def build(self, obstacles, origin, size, half_width, r_robot, power=20, out_device=None, metric="chamfer",
              dem=None, hazard=None, return_mask=False):
        """metric "chamfer": the reference's cv2.distanceTransform(DIST_L2, 5); "exact": exact EDT."""
        obs, optr = _obstacles(obstacles)
        out = None if out_device is not None else np.empty((size, size), np.float32)
        hz = make_hazard(hazard, r_robot)
        if hz is None:
            if return_mask:
                raise ValueError("return_mask needs a hazard")
            _check(self.lib, self.lib.mppi_costmap_builder_build(
                self.h, optr, obs.shape[0], int(size), float(half_width), float(origin[0]), float(origin[1]),
                float(r_robot), int(power), None if out is None else _fp(out),
                None if out_device is None else C.c_void_p(int(out_device)), _metric(metric)),
                "mppi_costmap_builder_build")
            return out
        if dem is None:
            raise ValueError("hazard: dem=(z_device, rows, cols, x_min, y_min, resolution) is needed")
        z, rows, cols, x_min, y_min, res = dem
        mask, mptr = _mask(size, return_mask)
        _check(self.lib, self.lib.mppi_costmap_builder_build_hazard(
            self.h, optr, obs.shape[0], int(size), float(half_width), float(origin[0]), float(origin[1]),
            float(r_robot), int(power), C.c_void_p(int(z) or None), int(rows), int(cols), float(x_min), float(y_min),
            float(res), C.byref(hz), None if out is None else _fp(out),
            None if out_device is None else C.c_void_p(int(out_device)), mptr, _metric(metric)),
            "mppi_costmap_builder_build_hazard")
        return (out, mask) if return_mask else out

    def hazard_count_ms(self):
        """Device time of the steep-cell count kernel alone in the last hazard build."""
        ms = C.c_double()
        _check(self.lib, self.lib.mppi_costmap_builder_hazard_count_ms(self.h, C.byref(ms)),
               "mppi_costmap_builder_hazard_count_ms")
        return ms.value

    def last_ms(self):
        ms = C.c_double()
        _check(self.lib, self.lib.mppi_costmap_builder_last_ms(self.h, C.byref(ms)), "mppi_costmap_builder_last_ms")
        return ms.value

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.mppi_costmap_builder_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


DEM_VARIANTS = {"mfma": 0, "valu": 1}   # mppi_dem_variant (include/mppi.h)


def _dem_variant(v):
    if v not in DEM_VARIANTS:
        raise ValueError(f"DEM variant must be one of {sorted(DEM_VARIANTS)}, got {v!r}")
    return DEM_VARIANTS[v]


def _craters(bumps):
    """Crater list -> contiguous float64 [n, 4] rows (cx, cy, height, width) (n may be 0).  Accepted: the
    reference's own shape [((cx, cy), height, width), ...] (MPPI_isaac.py:318) or an (n, 4) array."""
    from .scene import crater_rows
    a = crater_rows(bumps)
    return a, a.ctypes.data_as(_DP)


def _dem_base(base, grid_size):
    if base is None:
        return None
    base = np.ascontiguousarray(base, dtype=np.float32)
    if base.shape != (grid_size, grid_size):
        raise ValueError(f"base: shape {base.shape}, the DEM's is {(grid_size, grid_size)}")
    return base


class DemBuilder:
    """Surface.create_surface (MPPI_isaac.py:307-356) on the GPU as a separable float64 sum (DESIGN.md
    §3.6), no controller context needed.

    build(...) returns the grid_size x grid_size float32 heights as an ndarray; with out_device=<pointer>
    they are written to caller-owned device memory instead.
    """

    def __init__(self, device: int = 0):
        self.lib = load_library()
        self.device = int(device)
        h = C.c_void_p()
        _check(self.lib, self.lib.mppi_dem_builder_create(self.device, C.byref(h)), "mppi_dem_builder_create")
        self.h = h

    def build(self, bumps, grid_size, half_width, base=None, out_device=None, variant="mfma"):
        """variant "mfma": the product on the matrix cores; "valu": on the vector ALU (same result up to
        the order of the sum)."""
        cr, cptr = _craters(bumps)
        grid_size = int(grid_size)
        base = _dem_base(base, grid_size)
        out = None if out_device is not None else np.empty((grid_size, grid_size), np.float32)
        _check(self.lib, self.lib.mppi_dem_builder_build(
            self.h, cptr, cr.shape[0], grid_size, float(half_width), None if base is None else _fp(base),
            None if out is None else _fp(out), None if out_device is None else C.c_void_p(int(out_device)),
            _dem_variant(variant)), "mppi_dem_builder_build")
        return out

    def product(self, r_device, c_device, terms, grid_size, out_device=None, variant="mfma"):
        """Test hook (mppi_dem_builder_product): the product kernel on caller-supplied device factor
        tables, both [terms][grid_size] float64, terms a multiple of 4."""
        grid_size = int(grid_size)
        out = None if out_device is not None else np.empty((grid_size, grid_size), np.float32)
        _check(self.lib, self.lib.mppi_dem_builder_product(
            self.h, C.c_void_p(int(r_device)), C.c_void_p(int(c_device)), int(terms), grid_size,
            None if out is None else _fp(out), None if out_device is None else C.c_void_p(int(out_device)),
            _dem_variant(variant)), "mppi_dem_builder_product")
        return out

    def last_ms(self):
        ms = C.c_double()
        _check(self.lib, self.lib.mppi_dem_builder_last_ms(self.h, C.byref(ms)), "mppi_dem_builder_last_ms")
        return ms.value

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.mppi_dem_builder_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _check(lib, rc, what):
    if rc != MPPI_OK:
        msg = lib.mppi_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed ({rc}): {msg}")


def make_params(K, H, k_offset=0, **kw):
    """Fill mppi_params; float fields are rounded to float32 by ctypes."""
    p = MppiParams()
    p.num_trajectories = int(K)
    p.k_offset = int(k_offset)
    p.num_iterations = int(H)
    defaults = dict(dt=0.045, robot_radius=1.2, min_u1=-1.0, max_u1=1.0, min_u2=-1.0, max_u2=1.0,
                    v_min_linear=0.0, v_max_linear=2.0, v_min_angular=-1.0, v_max_angular=1.0,
                    temperature=0.3, filter_k=3.5, filter_a=0.96, opt_filter_k=3.0, opt_filter_a=0.92,
                    wheel_offset=0.2, w_path=100.5, w_slope=50.5, w_speed=0.5, w_obstacle=25.0,
                    collision_threshold=0.99, collision_penalty=100000.0, horizon=None, seed=42)
    defaults.update({k: v for k, v in kw.items() if v is not None or k != "horizon"})
    if defaults["horizon"] is None:
        defaults["horizon"] = float(defaults["dt"]) * float(defaults["v_max_linear"]) * int(H)
    for k, v in defaults.items():
        if k == "seed":
            p.seed = int(v) & 0xFFFFFFFFFFFFFFFF
        else:
            setattr(p, k, float(v))
    return p


def make_state(x, y, heading=(1.0, 0.0, 0.0), left_wheel_speed=0.0, right_wheel_speed=0.0,
               goal_x=0.0, goal_y=0.0, std_dev_u1=0.25, std_dev_u2=0.25):
    """Fill mppi_state; the heading is normalised in float64 first (MPPI_isaac.py:493)."""
    s = MppiState()
    s.x, s.y = float(x), float(y)
    h = np.asarray(heading, dtype=np.float64)
    h = (h / np.linalg.norm(h)).astype(np.float32)
    for i in range(3):
        s.heading[i] = float(h[i])
    s.left_wheel_speed = float(left_wheel_speed)
    s.right_wheel_speed = float(right_wheel_speed)
    s.goal_x, s.goal_y = float(goal_x), float(goal_y)
    s.std_dev_u1, s.std_dev_u2 = float(std_dev_u1), float(std_dev_u2)
    return s


def check_paths(traj, lin_vel, left_wheel=None, right_wheel=None, lengths=None):
    """Validate and normalise the arrays of Engine.score_paths (no library call).

    traj [n, L, 3], lin_vel [n, L], optional left_wheel / right_wheel [n, L, 3] (both or neither),
    optional lengths [n] of integers in [1, L].  Returns (n, L, traj, lin_vel, left_wheel,
    right_wheel, lengths) as C-contiguous float32 / int32 arrays (None where not given); raises
    ValueError on anything the library would refuse.
    """
    traj = np.ascontiguousarray(traj, dtype=np.float32)
    if traj.ndim != 3 or traj.shape[2] != 3:
        raise ValueError(f"traj must have shape [n, L, 3], got {traj.shape}")
    n, L = int(traj.shape[0]), int(traj.shape[1])
    if L < 1:
        raise ValueError("paths need at least one waypoint")
    if n * L >= 2 ** 31:
        raise ValueError("n * L must be below 2^31")
    lin_vel = np.ascontiguousarray(lin_vel, dtype=np.float32)
    if lin_vel.shape != (n, L):
        raise ValueError(f"lin_vel must have shape {(n, L)}, got {lin_vel.shape}")
    if (left_wheel is None) != (right_wheel is None):
        raise ValueError("give both wheel arrays or neither")
    if left_wheel is not None:
        left_wheel = np.ascontiguousarray(left_wheel, dtype=np.float32)
        right_wheel = np.ascontiguousarray(right_wheel, dtype=np.float32)
        for name, a in (("left_wheel", left_wheel), ("right_wheel", right_wheel)):
            if a.shape != (n, L, 3):
                raise ValueError(f"{name} must have shape {(n, L, 3)}, got {a.shape}")
    if lengths is not None:
        raw = np.asarray(lengths)
        if raw.shape != (n,):
            raise ValueError(f"lengths must have shape {(n,)}, got {raw.shape}")
        if raw.dtype.kind not in "iu":
            raise ValueError("lengths must be integers")
        if n and (raw.min() < 1 or raw.max() > L):
            raise ValueError(f"lengths must lie in [1, {L}]")
        lengths = np.ascontiguousarray(raw, dtype=np.int32)
    return n, L, traj, lin_vel, left_wheel, right_wheel, lengths


def step_word(step):
    """The Philox step of a step call as an integer in [0, 2^64) (include/mppi.h mppi_step; DESIGN.md §4
    D14: the counter is a full 64-bit word and the step after 2^64 - 1 is 0).  ValueError outside: ctypes
    would reduce it modulo 2^64 without a word, and a caller's -1 would run as step 2^64 - 1."""
    step = int(step)
    if not 0 <= step <= 0xFFFFFFFFFFFFFFFF:
        raise ValueError(f"step must lie in [0, 2^64), got {step}")
    return step


class Engine:
    """One device context of the HIP MPPI engine (thin, allocation-free per step)."""

    OUT_NAMES = ("u1_opt", "u2_opt", "lin_vel", "ang_vel", "traj_sim", "heading_sim",
                 "left_wheel_sim", "right_wheel_sim")

    def __init__(self, params: MppiParams, device: int = 0, _ctx=None):
        self.lib = load_library()
        self.params = params
        self.H = int(params.num_iterations)
        self.K = int(params.num_trajectories)
        self.device = int(device)
        self._owned = _ctx is None
        if _ctx is None:
            ctx = C.c_void_p()
            _check(self.lib, self.lib.mppi_create(C.byref(params), self.device, C.byref(ctx)), "mppi_create")
        else:
            ctx = _ctx   # a group member: the group destroys it
        self.ctx = ctx
        H = self.H
        self._buf = {n: np.zeros(3 * H if n.endswith("_sim") else H, np.float32) for n in self.OUT_NAMES}
        self._out = MppiOutputs(*[_fp(self._buf[n]) for n in self.OUT_NAMES])
        self._outref = C.byref(self._out)
        self._step_fn = self.lib.mppi_step   # the per-step call, bound once (it sits on the step's host path)
        self._keep = []
        self.async_tail = False
        self.dem_shape = None       # (rows, cols) of the bound DEM and (size, size) of the costmap:
        self.costmap_shape = None   # the shape a Batch's scene slots must have

    # ------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "ctx", None) and self.ctx.value:
            if getattr(self, "_owned", True):
                self.lib.mppi_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _c(self, rc, what):
        _check(self.lib, rc, what)

    # ------------------------------------------------------------ scene / state
    def set_stream(self, stream_handle):
        self._c(self.lib.mppi_set_stream(self.ctx, C.c_void_p(stream_handle or None)), "mppi_set_stream")

    def set_dem(self, Z, half_width=None, resolution=None, x_min=None, y_min=None):
        Z = np.ascontiguousarray(Z, dtype=np.float32)
        rows, cols = Z.shape
        if resolution is None:
            resolution = 2.0 * half_width / cols
        if x_min is None:
            x_min = -half_width
        if y_min is None:
            y_min = -half_width
        self._c(self.lib.mppi_set_dem(self.ctx, _fp(Z), rows, cols, x_min, y_min, resolution), "mppi_set_dem")
        self.dem_shape = (rows, cols)

    def set_dem_device(self, ptr, rows, cols, half_width, resolution=None, keepalive=None):
        if resolution is None:
            resolution = 2.0 * half_width / cols
        self._c(self.lib.mppi_set_dem_device(self.ctx, C.c_void_p(int(ptr)), rows, cols, -half_width,
                                             -half_width, resolution), "mppi_set_dem_device")
        self.dem_shape = (int(rows), int(cols))
        self._keep = [keepalive]

    def dem_updated(self):
        """The bound device DEM was written in place: rebuild the per-cell normal table."""
        self._c(self.lib.mppi_dem_updated(self.ctx), "mppi_dem_updated")

    def set_costmap(self, cm, half_width, resolution=None):
        cm = np.ascontiguousarray(cm, dtype=np.float32)
        size = cm.shape[1]
        if resolution is None:
            resolution = 2.0 * half_width / size
        self._c(self.lib.mppi_set_costmap(self.ctx, _fp(cm), size, half_width, resolution), "mppi_set_costmap")
        self.costmap_shape = (size, size)

    def build_costmap(self, obstacles, origin, size, half_width, r_robot, power=20, copy_out=True,
                      metric="chamfer", hazard=None, return_mask=False):
        """Surface.create_obstacles_costmap + costmap_wp.assign in one device pass
        (visual_terrain_stack_full_terrain.py:561-563); returns the map if copy_out.
        hazard (a dict or scene.Hazard): the steep cells of the bound DEM, read in place, join the
        rocks; return_mask: (map, uint8 mask with bit 0 H0, bit 1 H1, bit 2 rock disc)."""
        obs, optr = _obstacles(obstacles)
        out = np.empty((size, size), np.float32) if copy_out else None
        hz = make_hazard(hazard, r_robot)
        if hz is None:
            if return_mask:
                raise ValueError("return_mask needs a hazard")
            self._c(self.lib.mppi_build_costmap(self.ctx, optr, obs.shape[0], int(size), float(half_width),
                                                float(origin[0]), float(origin[1]), float(r_robot), int(power),
                                                None if out is None else _fp(out), _metric(metric)),
                    "mppi_build_costmap")
            self.costmap_shape = (int(size), int(size))
            return out
        mask, mptr = _mask(size, return_mask)
        self._c(self.lib.mppi_build_costmap_hazard(self.ctx, optr, obs.shape[0], int(size), float(half_width),
                                                   float(origin[0]), float(origin[1]), float(r_robot), int(power),
                                                   C.byref(hz), None if out is None else _fp(out), mptr,
                                                   _metric(metric)), "mppi_build_costmap_hazard")
        self.costmap_shape = (int(size), int(size))
        return (out, mask) if return_mask else out

    def build_dem(self, bumps, grid_size, half_width, base=None, copy_out=True, variant="mfma"):
        """Surface.create_surface + set_dem in one device pass (mppi_build_dem): the crater field is
        built in the engine's own DEM buffer with the geometry set_dem(Z, half_width) gives; returns
        the heights if copy_out."""
        cr, cptr = _craters(bumps)
        grid_size = int(grid_size)
        base = _dem_base(base, grid_size)
        out = np.empty((grid_size, grid_size), np.float32) if copy_out else None
        self._c(self.lib.mppi_build_dem(self.ctx, cptr, cr.shape[0], grid_size, float(half_width),
                                        None if base is None else _fp(base), None if out is None else _fp(out),
                                        _dem_variant(variant)), "mppi_build_dem")
        self.dem_shape = (grid_size, grid_size)
        self._keep = []
        return out

    def rollout_python25d(self, x0, y0, heading, lin_vel, ang_vel, dt, half_width, resolution, bound=20.0):
        """debug.generate_trajectory_25D (debug.py:312-364) for K trajectories on this context's DEM, float64.

        Returns (traj [K, H, 3], valid [K] bool); valid is False where the reference returns None."""
        v = np.ascontiguousarray(lin_vel, np.float64)
        w = np.ascontiguousarray(ang_vel, np.float64)
        K, H = v.shape
        assert w.shape == (K, H)
        x0 = np.ascontiguousarray(np.broadcast_to(np.asarray(x0, np.float64), (K,)))
        y0 = np.ascontiguousarray(np.broadcast_to(np.asarray(y0, np.float64), (K,)))
        hd = np.ascontiguousarray(np.broadcast_to(np.asarray(heading, np.float64).reshape(-1, 3), (K, 3)))
        traj = np.zeros((K, H, 3), np.float64)
        valid = np.zeros(K, np.int32)
        dp = lambda a: a.ctypes.data_as(_DP)  # noqa: E731
        self._c(self.lib.mppi_rollout_python25d(self.ctx, K, H, dp(x0), dp(y0), dp(hd), dp(v), dp(w), float(dt),
                                                float(half_width), float(resolution), float(bound), dp(traj),
                                                valid.ctypes.data_as(C.POINTER(C.c_int32))),
                "mppi_rollout_python25d")
        return traj, valid.astype(bool)

    def set_state(self, state: MppiState):
        self._c(self.lib.mppi_set_state(self.ctx, C.byref(state)), "mppi_set_state")

    def set_nominal(self, u1, u2):
        u1 = np.ascontiguousarray(u1, dtype=np.float32)
        u2 = np.ascontiguousarray(u2, dtype=np.float32)
        assert u1.size == self.H and u2.size == self.H
        self._c(self.lib.mppi_set_nominal(self.ctx, _fp(u1), _fp(u2)), "mppi_set_nominal")

    def get_nominal(self):
        u1 = np.zeros(self.H, np.float32)
        u2 = np.zeros(self.H, np.float32)
        self._c(self.lib.mppi_get_nominal(self.ctx, _fp(u1), _fp(u2)), "mppi_get_nominal")
        return u1, u2

    def _outputs(self):
        H = self.H
        b = self._buf
        return dict(u1_opt=b["u1_opt"].copy(), u2_opt=b["u2_opt"].copy(), lin_vel=b["lin_vel"].copy(),
                    ang_vel=b["ang_vel"].copy(), traj_sim=b["traj_sim"].reshape(H, 3).copy(),
                    heading_sim=b["heading_sim"].reshape(H, 3).copy(),
                    left_wheel_sim=b["left_wheel_sim"].reshape(H, 3).copy(),
                    right_wheel_sim=b["right_wheel_sim"].reshape(H, 3).copy())

    def step(self, proj="3d", step=0, copy=True):
        rc = self._step_fn(self.ctx, PROJ[proj], step_word(step), self._outref)
        if rc != MPPI_OK:
            self._c(rc, "mppi_step")
        return self._outputs() if copy else None

    def step_injected(self, u1, u2, proj="3d"):
        u1 = np.ascontiguousarray(u1, dtype=np.float32).reshape(-1)
        u2 = np.ascontiguousarray(u2, dtype=np.float32).reshape(-1)
        assert u1.size == self.K * self.H and u2.size == self.K * self.H
        self._c(self.lib.mppi_step_injected(self.ctx, PROJ[proj], _fp(u1), _fp(u2), C.byref(self._out)),
                "mppi_step_injected")
        return self._outputs()

    def set_async_tail(self, on=True):
        """Deferred optimal rollout: step() returns the controls + row 0 of the *_sim arrays;
        outputs() waits for the rest (bitwise identical)."""
        self._c(self.lib.mppi_set_async_tail(self.ctx, 1 if on else 0), "mppi_set_async_tail")
        self.async_tail = bool(on)

    def outputs(self):
        """All outputs of the last step (waits for a deferred optimal rollout)."""
        self._c(self.lib.mppi_get_outputs(self.ctx, C.byref(self._out)), "mppi_get_outputs")
        return self._outputs()

    def record_len(self):
        return int(self.lib.mppi_record_len(self.ctx))

    def step_partial(self, record_ptr, proj="3d", step=0):
        self._c(self.lib.mppi_step_partial(self.ctx, PROJ[proj], step_word(step), C.c_void_p(int(record_ptr))),
                "mppi_step_partial")

    def step_finish(self, records_ptr, n, copy=True):
        self._c(self.lib.mppi_step_finish(self.ctx, C.c_void_p(int(records_ptr)), int(n), C.byref(self._out)),
                "mppi_step_finish")
        return self._outputs() if copy else None

    # ------------------------------------------------------------ introspection
    def costs(self):
        c = np.zeros(self.K, np.float32)
        self._c(self.lib.mppi_get_costs(self.ctx, _fp(c), self.K), "mppi_get_costs")
        return c

    def dump(self):
        K, H = self.K, self.H
        arrs = dict(traj=np.zeros((K, H, 3), np.float32), hv=np.zeros((K, H, 3), np.float32),
                    lw=np.zeros((K, H, 3), np.float32), rw=np.zeros((K, H, 3), np.float32),
                    v=np.zeros((K, H), np.float32), w=np.zeros((K, H), np.float32),
                    u1=np.zeros((K, H), np.float32), u2=np.zeros((K, H), np.float32))
        self._c(self.lib.mppi_dump_rollouts(self.ctx, *[_fp(arrs[n]) for n in
                                                        ("traj", "hv", "lw", "rw", "v", "w", "u1", "u2")]),
                "mppi_dump_rollouts")
        return arrs

    def score_paths(self, traj, lin_vel, left_wheel=None, right_wheel=None, lengths=None, state=None):
        """mppi_score_paths: the critics on caller-supplied paths, traj [n, L, 3], lin_vel [n, L].

        Without wheel arrays the slope critic runs on the body path; lengths [n] gives ragged paths
        (rows past a path's length are not read); state (MppiState) is the position and goal the
        critics measure from, default the engine's current state.  Returns dict(cost [n],
        terms [n, 4] in COST_TERMS order, collisions [n])."""
        n, L, traj, lin_vel, left_wheel, right_wheel, lengths = check_paths(traj, lin_vel, left_wheel,
                                                                           right_wheel, lengths)
        out = dict(cost=np.zeros(n, np.float32), terms=np.zeros((n, 4), np.float32),
                   collisions=np.zeros(n, np.int32))
        i32 = C.POINTER(C.c_int32)
        sc = MppiPathScores(_fp(out["cost"]), _fp(out["terms"]), out["collisions"].ctypes.data_as(i32))
        self._c(self.lib.mppi_score_paths(
            self.ctx, n, L, None if lengths is None else lengths.ctypes.data_as(i32), _fp(traj),
            None if left_wheel is None else _fp(left_wheel), None if right_wheel is None else _fp(right_wheel),
            _fp(lin_vel), None if state is None else C.byref(state), C.byref(sc)), "mppi_score_paths")
        return out

    def cost_terms(self):
        """mppi_get_cost_terms: (terms [K, 4] in COST_TERMS order, collisions [K]) of the last step's rollouts."""
        terms = np.zeros((self.K, 4), np.float32)
        col = np.zeros(self.K, np.int32)
        self._c(self.lib.mppi_get_cost_terms(self.ctx, _fp(terms), col.ctypes.data_as(C.POINTER(C.c_int32))),
                "mppi_get_cost_terms")
        return terms, col

    def cost_terms5(self):
        """mppi_get_cost_terms5: (terms [K, 5] in COST_TERMS5 order, collisions [K]) of the last step's
        rollouts; recombined in the critic set's order they are the bits of costs() for any set."""
        terms = np.zeros((self.K, 5), np.float32)
        col = np.zeros(self.K, np.int32)
        self._c(self.lib.mppi_get_cost_terms5(self.ctx, _fp(terms), col.ctypes.data_as(C.POINTER(C.c_int32))),
                "mppi_get_cost_terms5")
        return terms, col

    def set_critics(self, slope="wheels", w_orientation=0.0):
        """mppi_set_critics: the slope critic on the wheel contacts ("wheels", the default) or on the
        body path ("body", the only slope information of the 2D projection), and the weight of the
        path-orientation critic (0: off).  Applies from the next step."""
        k = make_critics(slope, w_orientation)
        self._c(self.lib.mppi_set_critics(self.ctx, C.byref(k)), "mppi_set_critics")

    def critics(self):
        """mppi_get_critics: dict(slope="wheels" | "body", w_orientation)."""
        k = MppiCritics()
        self._c(self.lib.mppi_get_critics(self.ctx, C.byref(k)), "mppi_get_critics")
        return critics_as_dict(k)

    def set_sampling(self, antithetic=False, nominal=False, beta=0.0):
        """mppi_set_sampling: how the K control sequences are drawn from the next step on (mppi_amd.sampling):
        antithetic pairs, a noise-free rollout of the shifted nominal as trajectory 0, AR(1) noise of
        coefficient beta in [0, 1).  The default changes no bit."""
        k = make_sampling(antithetic, nominal, beta, k_offset=int(self.params.k_offset))
        self._c(self.lib.mppi_set_sampling(self.ctx, C.byref(k)), "mppi_set_sampling")

    def get_sampling(self):
        """mppi_get_sampling: dict(antithetic, nominal, beta)."""
        k = MppiSampling()
        self._c(self.lib.mppi_get_sampling(self.ctx, C.byref(k)), "mppi_get_sampling")
        return dict(antithetic=bool(k.antithetic), nominal=bool(k.nominal), beta=float(k.beta))

    def detmath_atan2(self, y, x):
        """mppi_detmath_atan2: (dm_atan2(y, x) as the device computes it, the device library's atan2(y, x)),
        float64 arrays of y's shape (y and x broadcast)."""
        y, x = np.broadcast_arrays(np.asarray(y, np.float64), np.asarray(x, np.float64))
        y, x = np.ascontiguousarray(y), np.ascontiguousarray(x)
        dm, dev = np.empty(y.shape, np.float64), np.empty(y.shape, np.float64)
        self._c(self.lib.mppi_detmath_atan2(self.ctx, y.size, y.ctypes.data_as(_DP), x.ctypes.data_as(_DP),
                                            dm.ctypes.data_as(_DP), dev.ctypes.data_as(_DP)), "mppi_detmath_atan2")
        return dm, dev

    def score_ms(self):
        """HIP-event time (ms) of the last scoring kernel (score_paths / cost_terms)."""
        ms = C.c_double()
        self._c(self.lib.mppi_get_score_ms(self.ctx, C.byref(ms)), "mppi_get_score_ms")
        return ms.value

    def set_option(self, name, value):
        """mppi_set_option (include/mppi.h): per-context tuning / test hooks by name."""
        self._c(self.lib.mppi_set_option(self.ctx, name.encode(), int(value)), "mppi_set_option")

    def set_timing(self, on=True):
        """on: False / True (rollout, finish and tail events) or 2 (rollout and finish only)."""
        mode = on if isinstance(on, int) and not isinstance(on, bool) else (1 if on else 0)
        self._c(self.lib.mppi_set_timing(self.ctx, mode), "mppi_set_timing")

    def timing(self):
        r = C.c_double()
        f = C.c_double()
        n = C.c_int64()
        self._c(self.lib.mppi_get_timing(self.ctx, C.byref(r), C.byref(f), C.byref(n)), "mppi_get_timing")
        return r.value, f.value, n.value

    def tail_timing(self):
        t = C.c_double()
        n = C.c_int64()
        self._c(self.lib.mppi_get_tail_timing(self.ctx, C.byref(t), C.byref(n)), "mppi_get_tail_timing")
        return t.value, n.value

    def launch_info(self):
        info = (C.c_int64 * 19)()
        self._c(self.lib.mppi_get_launch_info(self.ctx, info, 19), "mppi_get_launch_info")
        keys = ("reserved", "block", "blocks", "window_cols", "window_rows", "lds_bytes", "finish_kind",
                "finish_records", "finish_ncol", "finish_groups", "ucache_steps", "resident",
                "server_launches", "server_steps", "server_failed_steps", "server_relaunches",
                "server_fallbacks", "cadence_steps", "verified_reciprocals")
        return dict(zip(keys, [int(v) for v in info]))

    def server_time(self):
        """mppi_get_server_time: (rollout us summed, step us summed, steps) on the resident server."""
        r, st, n = C.c_double(0), C.c_double(0), C.c_int64(0)
        self._c(self.lib.mppi_get_server_time(self.ctx, C.byref(r), C.byref(st), C.byref(n)), "mppi_get_server_time")
        return r.value, st.value, n.value

    def chain_clock(self):
        """mppi_get_chain_clock: shader MHz, cycles per chain step, chain us and cycles of the last rollout."""
        v = (C.c_double * 10)()
        self._c(self.lib.mppi_get_chain_clock(self.ctx, v, 10), "mppi_get_chain_clock")
        return dict(zip(("shader_mhz", "cycles_per_step", "chain_us", "chain_cycles", "start_to_chain_us",
                         "chain_to_roles_done_us", "leaf_us", "wg_start_spread_us", "wg_end_spread_us",
                         "wg_span_us"), [float(x) for x in v]))

    def selftest(self, what, n=1 << 24, seed=1):
        bad = C.c_int64()
        self._c(self.lib.mppi_selftest(self.ctx, int(what), int(n), int(seed), C.byref(bad)), "mppi_selftest")
        return bad.value

    def bilinear_tiles(self):
        n = C.c_int32()
        self._c(self.lib.mppi_bilinear_tiles(self.ctx, C.byref(n)), "mppi_bilinear_tiles")
        return n.value

    def bin_queries(self, x_ptr, y_ptr, n, xs_ptr, ys_ptr, perm_ptr, off_ptr):
        self._c(self.lib.mppi_bin_queries(self.ctx, C.c_void_p(int(x_ptr)), C.c_void_p(int(y_ptr)), int(n),
                                          C.c_void_p(int(xs_ptr)), C.c_void_p(int(ys_ptr)),
                                          C.c_void_p(int(perm_ptr)), C.c_void_p(int(off_ptr))), "mppi_bin_queries")

    def bilinear_tiled(self, xs_ptr, ys_ptr, off_ptr, h_ptr):
        """Asynchronous on the engine stream (sync() waits)."""
        self._c(self.lib.mppi_bilinear_tiled(self.ctx, C.c_void_p(int(xs_ptr)), C.c_void_p(int(ys_ptr)),
                                             C.c_void_p(int(off_ptr)), C.c_void_p(int(h_ptr))),
                "mppi_bilinear_tiled")

    def sync(self):
        self._c(self.lib.mppi_sync(self.ctx), "mppi_sync")

    def bilinear_query(self, x_ptr, y_ptr, h_ptr, n):
        self._c(self.lib.mppi_bilinear_query(self.ctx, C.c_void_p(int(x_ptr)), C.c_void_p(int(y_ptr)),
                                             C.c_void_p(int(h_ptr)), int(n)), "mppi_bilinear_query")


def make_policy(sigma_base=0.4, sigma_div=1.0, goal_tol=0.5, check_every=0):
    """Fill mppi_loop_policy (defaults: run()'s policy; check_every 0 = the library's 16)."""
    return MppiLoopPolicy(float(sigma_base), float(sigma_div), float(goal_tol), int(check_every))


def make_critics(slope="wheels", w_orientation=0.0):
    """Fill mppi_critics; ValueError names the field (the checks of mppi_set_critics that need no context)."""
    if isinstance(slope, str):
        if slope not in SLOPE_MODES:
            raise ValueError(f"slope must be one of {sorted(SLOPE_MODES)}, got {slope!r}")
        mode = SLOPE_MODES[slope]
    else:
        mode = int(slope)
        if mode not in SLOPE_MODES.values():
            raise ValueError(f"slope mode must be 0 (wheels) or 1 (body), got {mode}")
    w = float(w_orientation)
    if not (np.isfinite(w) and abs(w) <= float(np.finfo(np.float32).max)):
        raise ValueError(f"w_orientation must be a finite float32, got {w_orientation!r}")
    return MppiCritics(mode, w)


def make_sampling(antithetic=False, nominal=False, beta=0.0, k_offset=None):
    """Fill mppi_sampling; ValueError names the field (the checks of mppi_set_sampling; the one on
    k_offset where the caller gives it)."""
    from .sampling import make_plan
    p = make_plan(antithetic, nominal, beta, k_offset)
    return MppiSampling(int(p["antithetic"]), int(p["nominal"]), p["beta"])


def critics_as_dict(k: MppiCritics):
    return dict(slope={v: n for n, v in SLOPE_MODES.items()}[int(k.slope_mode)], w_orientation=float(k.w_orientation))


def make_variant(proj="3d", **fields):
    """Fill mppi_batch_variant: the defaults of make_params and run()'s sigma schedule, overridden by
    `fields` (VARIANT_FIELDS); float fields are rounded to float32 by ctypes.  A dict (as
    Batch.variant_default returns or mppi_amd.batch.variant_params takes) passes as **dict."""
    unknown = set(fields) - set(VARIANT_FIELDS)
    if unknown:
        raise ValueError(f"not fields of mppi_batch_variant: {sorted(unknown)}")
    p = make_params(1, 1)
    v = MppiBatchVariant()
    for n in VARIANT_FIELDS:
        default = {"sigma_base": 0.4, "sigma_div": 1.0}.get(n)
        setattr(v, n, float(fields.get(n, getattr(p, n) if default is None else default)))
    v.proj = PROJ[proj]
    return v


def variant_as_dict(v: MppiBatchVariant):
    """The dict of a MppiBatchVariant (what mppi_amd.batch.variant_params takes)."""
    d = {n: np.float32(getattr(v, n)) for n in VARIANT_FIELDS}
    d["proj"] = int(v.proj)
    return d


def _as_variant(v):
    return v if isinstance(v, MppiBatchVariant) else make_variant(**dict(v))


def make_task(start, seed, max_steps, variant=-1, dem=-1, costmap=-1, trajectories=0):
    """Fill mppi_batch_task: what Batch.set_episode takes (start: MppiState, the heading used as
    given), plus the step cap."""
    t = MppiBatchTask()
    t.start = start
    t.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    t.variant, t.dem_slot, t.costmap_slot = int(variant), int(dem), int(costmap)
    t.num_trajectories, t.max_steps = int(trajectories), int(max_steps)
    return t


class Batch:
    """mppi_batch (include/mppi.h): E closed-loop episodes over one Engine's scene and parameters,
    advanced on the GPU with no host work between steps.  Keeps a reference to its Engine, so the
    context cannot be freed first."""

    def __init__(self, engine: "Engine", episodes: int):
        self.engine = engine
        self.lib = engine.lib
        self.E = int(episodes)
        self.H = engine.H
        h = C.c_void_p()
        _check(self.lib, self.lib.mppi_batch_create(engine.ctx, self.E, C.byref(h)), "mppi_batch_create")
        self.h = h
        self.tracking = None    # set_tracking's arguments while tracking is set
        self.list_metrics = False    # the standing task list was set scored with metrics=True
        self._opts = ("body", False)    # mppi_batch_set_score_options as last set (the library's default)

    def set_wheel_log(self, on=True):
        """mppi_batch_set_wheel_log: runs, task lists and tracking set from here on keep each log row's wheel
        contacts (lx, ly, lz, rx, ry, rz) in an array beside the log: wheel_log() / task_wheel_log() read
        them, score(slope="wheels") scores them.  Refused while a campaign is unfinished or tracking is set."""
        _check(self.lib, self.lib.mppi_batch_set_wheel_log(self.h, 1 if on else 0), "mppi_batch_set_wheel_log")

    def _score_options(self, slope, metrics):
        """The options the next scored list or tracking takes; the library is told only when they change
        (it refuses the change under tracking or an unfinished campaign: the caller ends those first)."""
        if slope not in SLOPE_MODES:
            raise ValueError(f"slope must be one of {sorted(SLOPE_MODES)}, got {slope!r}")
        want = (slope, bool(metrics))
        if want == getattr(self, "_opts", ("body", False)):
            return
        _check(self.lib, self.lib.mppi_batch_set_score_options(self.h, SLOPE_MODES[slope], 1 if metrics else 0),
               "mppi_batch_set_score_options")
        self._opts = want

    def wheel_log(self, e, first=0, count=None):
        """Rows [count, 6] of the most recent run's wheel log: lx, ly, lz, rx, ry, rz beside log row n."""
        if count is None:
            count = self.episode(e)["steps_last_run"] - int(first)
        rows = np.zeros((max(int(count), 0), 6), np.float32)
        _check(self.lib, self.lib.mppi_batch_get_wheel_log(self.h, int(e), int(first), int(count), _fp(rows)),
               "mppi_batch_get_wheel_log")
        return rows

    def task_wheel_log(self, i, first=0, count=None):
        """Rows [count, 6] of task i's wheel log: lx, ly, lz, rx, ry, rz beside the task's log row n."""
        if count is None:
            count = self.task(i)["steps"] - int(first)
        rows = np.zeros((max(int(count), 0), 6), np.float32)
        _check(self.lib, self.lib.mppi_batch_get_task_wheel_log(self.h, int(i), int(first), int(count), _fp(rows)),
               "mppi_batch_get_task_wheel_log")
        return rows

    def set_episode(self, e, state: MppiState, seed, variant=-1, dem=-1, costmap=-1, trajectories=0):
        """Episode e starts at `state` with Philox key `seed` and runs with row `variant` of the table
        of set_variants (-1: the engine's params and run()'s proj / policy), on DEM slot `dem` and
        costmap slot `costmap` (-1: the engine's) with `trajectories` rollouts per step (0: the engine's K)."""
        _check(self.lib, self.lib.mppi_batch_set_episode(self.h, int(e), C.byref(state),
                                                         int(seed) & 0xFFFFFFFFFFFFFFFF),
               "mppi_batch_set_episode")
        _check(self.lib, self.lib.mppi_batch_set_episode_variant(self.h, int(e), int(variant)),
               "mppi_batch_set_episode_variant")
        _check(self.lib, self.lib.mppi_batch_set_episode_scene(self.h, int(e), int(dem), int(costmap)),
               "mppi_batch_set_episode_scene")
        _check(self.lib, self.lib.mppi_batch_set_episode_trajectories(self.h, int(e), int(trajectories)),
               "mppi_batch_set_episode_trajectories")

    def _slot_array(self, a, shape, what):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float32)
        if shape is None:
            raise RuntimeError(f"{what} slot: the engine has no {what} yet (a slot takes its geometry)")
        if a.shape != shape:
            raise ValueError(f"{what} slot: shape {a.shape}, the engine's is {shape}")
        return a

    def set_dem(self, slot, Z):
        """DEM slot `slot` holds a copy of Z (the shape and placement of the engine's DEM) and its normal
        table; None frees the slot."""
        Z = self._slot_array(Z, self.engine.dem_shape, "DEM")
        _check(self.lib, self.lib.mppi_batch_set_dem(self.h, int(slot), None if Z is None else _fp(Z)),
               "mppi_batch_set_dem")

    def build_dem(self, slot, bumps, half_width, base=None, copy_out=False, variant="mfma"):
        """Engine.build_dem with the grid of the engine's DEM (square, centred, of this half_width), into
        DEM slot `slot`; returns the heights if copy_out."""
        cr, cptr = _craters(bumps)
        shape = self.engine.dem_shape
        if shape is None:
            raise RuntimeError("DEM slot: the engine has no DEM yet (a slot takes its geometry)")
        base = self._slot_array(base, shape, "DEM")
        out = np.empty(shape, np.float32) if copy_out else None
        _check(self.lib, self.lib.mppi_batch_build_dem(
            self.h, int(slot), cptr, cr.shape[0], float(half_width), None if base is None else _fp(base),
            None if out is None else _fp(out), _dem_variant(variant)), "mppi_batch_build_dem")
        return out

    def set_costmap(self, slot, cm):
        """Costmap slot `slot` holds a copy of cm (the shape of the engine's costmap); None frees the slot."""
        cm = self._slot_array(cm, self.engine.costmap_shape, "costmap")
        _check(self.lib, self.lib.mppi_batch_set_costmap(self.h, int(slot), None if cm is None else _fp(cm)),
               "mppi_batch_set_costmap")

    def build_costmap(self, slot, obstacles, origin, r_robot, power=20, metric="chamfer", copy_out=False):
        """Engine.build_costmap with the size and half_width of the engine's costmap, into costmap slot
        `slot`; returns the map if copy_out."""
        obs, optr = _obstacles(obstacles)
        if self.engine.costmap_shape is None:
            raise RuntimeError("costmap slot: the engine has no costmap yet (a slot takes its geometry)")
        out = np.empty(self.engine.costmap_shape, np.float32) if copy_out else None
        _check(self.lib, self.lib.mppi_batch_build_costmap(
            self.h, int(slot), optr, obs.shape[0], float(origin[0]), float(origin[1]), float(r_robot), int(power),
            _metric(metric), None if out is None else _fp(out)), "mppi_batch_build_costmap")
        return out

    def build_costmap_hazard(self, slot, obstacles, origin, r_robot, hazard, dem=-1, power=20, metric="chamfer",
                             copy_out=False, return_mask=False):
        """build_costmap with the steep cells of DEM slot `dem` (-1: the engine's DEM), read on the device,
        joining the rocks (hazard: a dict or scene.Hazard, None: build_costmap).  Returns
        the map if copy_out (else None); with return_mask (map or None, uint8 mask: bit 0 H0, bit 1 H1,
        bit 2 rock disc).  (build_costmap keeps its parameter list; this is its hazard form.)"""
        hz = make_hazard(hazard, r_robot)
        if hz is None:
            if return_mask:
                raise ValueError("return_mask needs a hazard")
            return self.build_costmap(slot, obstacles, origin, r_robot, power, metric, copy_out)
        obs, optr = _obstacles(obstacles)
        if self.engine.costmap_shape is None:
            raise RuntimeError("costmap slot: the engine has no costmap yet (a slot takes its geometry)")
        out = np.empty(self.engine.costmap_shape, np.float32) if copy_out else None
        mask, mptr = _mask(self.engine.costmap_shape[0], return_mask)
        _check(self.lib, self.lib.mppi_batch_build_costmap_hazard(
            self.h, int(slot), int(dem), optr, obs.shape[0], float(origin[0]), float(origin[1]), float(r_robot),
            int(power), _metric(metric), C.byref(hz), None if out is None else _fp(out), mptr),
            "mppi_batch_build_costmap_hazard")
        return (out, mask) if return_mask else out

    def set_variants(self, variants):
        """The batch's variant table: a list of MppiBatchVariant or dicts (make_variant's arguments);
        an empty list clears it."""
        from .batch import split_sampling, split_variant
        plans = [(v, None) if isinstance(v, MppiBatchVariant) else split_sampling(v) for v in variants]
        variants = [v for v, _ in plans]
        split = [(v, None) if isinstance(v, MppiBatchVariant) else split_variant(v) for v in variants]
        rows = [_as_variant(v) for v, _ in split]
        arr = (MppiBatchVariant * max(len(rows), 1))(*rows)
        _check(self.lib, self.lib.mppi_batch_set_variants(self.h, len(rows), arr), "mppi_batch_set_variants")
        # dicts with "slope" / "w_orientation" keys fill the critic rows; a row without them runs with
        # the engine's set as it is now
        crit = [k for _, k in split]
        self.set_variant_critics([self.engine.critics() if k is None else k for k in crit]
                                 if any(k is not None for k in crit) else [])

        # and with "antithetic" / "nominal" / "noise_beta" keys the sampling rows, by the same rule
        samp = [k for _, k in plans]
        self.set_variant_sampling([self.engine.get_sampling() if k is None else k for k in samp]
                                  if any(k is not None for k in samp) else [])

    def set_variant_sampling(self, rows):
        """mppi_batch_set_variant_sampling: variant row i runs with the sampling plan rows[i] (MppiSampling
        or dict(antithetic=, nominal=, beta=)); variants past the list, and episodes or tasks without a
        variant, run with the engine's plan.  An empty list clears the rows."""
        rows = [k if isinstance(k, MppiSampling) else make_sampling(**dict(k)) for k in rows]
        arr = (MppiSampling * max(len(rows), 1))(*rows)
        _check(self.lib, self.lib.mppi_batch_set_variant_sampling(self.h, len(rows), arr),
               "mppi_batch_set_variant_sampling")

    def set_variant_critics(self, rows):
        """mppi_batch_set_variant_critics: variant row i runs with critic set rows[i] (MppiCritics or
        dict(slope=, w_orientation=)); variants past the list, and episodes or tasks without a variant,
        run with the engine's set.  An empty list clears the rows."""
        rows = [k if isinstance(k, MppiCritics) else make_critics(**dict(k)) for k in rows]
        arr = (MppiCritics * max(len(rows), 1))(*rows)
        _check(self.lib, self.lib.mppi_batch_set_variant_critics(self.h, len(rows), arr),
               "mppi_batch_set_variant_critics")

    def variant_default(self, proj="3d", policy=None):
        """The variant that changes nothing: the engine's params with `proj` and the policy's sigma schedule."""
        pol = policy if policy is not None else make_policy()
        v = MppiBatchVariant()
        _check(self.lib, self.lib.mppi_batch_variant_default(self.h, PROJ[proj], C.byref(pol), C.byref(v)),
               "mppi_batch_variant_default")
        return v

    def score(self, yardstick=None, origins=None, slope="body", metrics=False):
        """mppi_batch_score: every episode's executed path (the log of its most recent run) scored on
        the device with one cost function.  yardstick: MppiBatchVariant or dict whose weights,
        collision_threshold and collision_penalty are used (default the engine's params); origins: E
        MppiState (x, y, goal_x, goal_y are read; default each episode's position when its most recent
        run began and its goal).  Returns dict(cost [E], terms [E, 4] in COST_TERMS order,
        collisions [E], rows [E]).

        slope="wheels" (mppi_batch_score_ex): the slope term over the wheel log's two contact paths, what
        Engine.score_paths gives in the wheels mode for the log's waypoints and those contacts; needs
        set_wheel_log() before the run.  metrics=True: also `metrics` [E, 4] float64 in
        mppi_amd.batch.METRICS_FIELDS order (compute_path_metrics of each path)."""
        if slope not in SLOPE_MODES:
            raise ValueError(f"slope must be one of {sorted(SLOPE_MODES)}, got {slope!r}")
        E = self.E
        out = dict(cost=np.zeros(E, np.float32), terms=np.zeros((E, 4), np.float32),
                   collisions=np.zeros(E, np.int32), rows=np.zeros(E, np.int32))
        i32 = C.POINTER(C.c_int32)
        sc = MppiPathScores(_fp(out["cost"]), _fp(out["terms"]), out["collisions"].ctypes.data_as(i32))
        y = None if yardstick is None else C.byref(_as_variant(yardstick))
        o = None
        if origins is not None:
            origins = list(origins)
            if len(origins) != E:
                raise ValueError(f"{E} episodes but {len(origins)} origins")
            o = (MppiState * E)(*origins)
        if slope == "body" and not metrics:
            _check(self.lib, self.lib.mppi_batch_score(self.h, y, o, C.byref(sc), out["rows"].ctypes.data_as(i32)),
                   "mppi_batch_score")
            return out
        if metrics:
            out["metrics"] = np.zeros((E, 4), np.float64)
        _check(self.lib, self.lib.mppi_batch_score_ex(
            self.h, y, o, SLOPE_MODES[slope], C.byref(sc), out["rows"].ctypes.data_as(i32),
            out["metrics"].ctypes.data_as(_DP) if metrics else None), "mppi_batch_score_ex")
        return out

    def run(self, n_steps, proj="3d", policy=None):
        """Advance every active episode by up to n_steps steps (policy: MppiLoopPolicy, default run()'s)."""
        pol = policy if policy is not None else make_policy()
        _check(self.lib, self.lib.mppi_batch_run(self.h, PROJ[proj], int(n_steps), C.byref(pol)), "mppi_batch_run")

    def _io_array(self, a, name, codes, shape):
        """The device pointer of one array of step_device, checked: a device array (device_array's
        rules) of the given element type and shape on the engine's device."""
        dev = device_array(a, name, codes)
        if dev is None:
            raise TypeError(f"{name} must be a device array (a CUDA torch.Tensor, or an object exposing "
                            f"__cuda_array_interface__ or __dlpack__ on the GPU), got {type(a).__name__}")
        ptr, shp, _, index = dev
        if shp != shape:
            raise ValueError(f"{name} must have shape {shape}, got {shp}")
        if index is not None and index != self.engine.device:
            raise ValueError(f"{name} is on device {index}, the engine's is {self.engine.device}")
        return ptr

    def set_tracking(self, yardstick=None, max_steps=None, runs_per_episode=1, keep_log=True, goal_tol=0.5,
                     slope="body", metrics=False):
        """mppi_batch_set_tracking: from here on step_device tracks a run per set episode on the device:
        it logs each ingested state beside the command before it, tests the goal (goal_tol) and the
        step cap max_steps, scores the run with `yardstick` (MppiBatchVariant or dict whose weights,
        collision_threshold and collision_penalty are used; default the engine's params) and writes
        its result into one of the episode's runs_per_episode result rows; an ended episode idles
        until its next reset.  keep_log=False: no log row is written (log() then has no rows).
        Setting it again starts every run and count over.  runs() / run_counts() read the results.

        slope="wheels": the run's slope term is the wheel form, over the contacts the ingest forms from each
        ingested pose and the episode's DEM; metrics=True: runs() also returns `metrics` [R, 4] float64
        (mppi_amd.batch.path_metrics of the run's rows).  With set_wheel_log() on and keep_log the contacts
        are kept too (wheel_log())."""
        if slope not in SLOPE_MODES:
            raise ValueError(f"slope must be one of {sorted(SLOPE_MODES)}, got {slope!r}")
        if max_steps is None:
            raise ValueError("set_tracking needs max_steps, the step cap of a run (clear_tracking() turns tracking off)")
        max_steps, runs_per_episode = int(max_steps), int(runs_per_episode)
        if max_steps < 1:
            raise ValueError(f"max_steps must be >= 1, got {max_steps} (clear_tracking() turns tracking off)")
        if runs_per_episode < 1:
            raise ValueError(f"runs_per_episode must be >= 1, got {runs_per_episode}")
        if not float(goal_tol) >= 0:
            raise ValueError(f"goal_tol must be >= 0, got {goal_tol!r}")
        y = None if yardstick is None else C.byref(_as_variant(yardstick))
        if getattr(self, "tracking", None) and (slope, bool(metrics)) != getattr(self, "_opts", ("body", False)):
            self.clear_tracking()    # (the library refuses new options under tracking; setting it again starts over anyway)
        self._score_options(slope, metrics)
        _check(self.lib, self.lib.mppi_batch_set_tracking(self.h, y, float(goal_tol), max_steps, runs_per_episode,
                                                          1 if keep_log else 0), "mppi_batch_set_tracking")
        self.tracking = dict(max_steps=max_steps, runs_per_episode=runs_per_episode, keep_log=bool(keep_log))
        if slope != "body" or metrics:
            self.tracking.update(slope=slope, metrics=bool(metrics))

    def clear_tracking(self):
        """Turn tracking off and free its tables: step_device is the plain device step again."""
        _check(self.lib, self.lib.mppi_batch_set_tracking(self.h, None, 0.0, 0, 0, 0), "mppi_batch_set_tracking")
        self.tracking = None

    def run_counts(self):
        """mppi_batch_get_run_counts: int32 [E], the runs each episode has ended since tracking was set
        (a count above runs_per_episode: results were dropped)."""
        if not getattr(self, "tracking", None):
            raise RuntimeError("run_counts: tracking is not set (set_tracking)")
        counts = np.zeros(self.E, np.int32)
        _check(self.lib, self.lib.mppi_batch_get_run_counts(self.h, counts.ctypes.data_as(C.POINTER(C.c_int32))),
               "mppi_batch_get_run_counts")
        return counts

    def runs(self, e=None):
        """mppi_batch_get_runs: the result rows of tracked runs.  e: an episode -> dict of arrays over its
        runs_per_episode rows: run (the ordinal), state [R, 11] (mppi_state order, at the ending
        ingest), steps, reached, status (0: no run has ended into the row, 1: reached, 2: the cap,
        3: abandoned), cost, terms [R, 4], collisions, rows, length (float64), and metrics [R, 4] (float64,
        mppi_amd.batch.METRICS_FIELDS) when tracking was set with metrics=True.  e=None: every
        episode's rows stacked, with an `episode` column (mppi_amd.batch.campaign_summary takes it)."""
        tr = getattr(self, "tracking", None)
        if not tr:
            raise RuntimeError("runs: tracking is not set (set_tracking)")
        R = tr["runs_per_episode"]
        if e is None:
            per = [self.runs(i) for i in range(self.E)]
            out = {k: np.concatenate([p[k] for p in per]) for k in per[0]}
            out["episode"] = np.repeat(np.arange(self.E, dtype=np.int32), R)
            return out
        e = int(e)
        if not 0 <= e < self.E:
            raise ValueError(f"episode {e} outside [0, {self.E})")
        i32 = C.POINTER(C.c_int32)
        st = (MppiState * R)()
        out = dict(run=np.arange(R, dtype=np.int32), steps=np.zeros(R, np.int32), reached=np.zeros(R, np.int32),
                   status=np.zeros(R, np.int32), cost=np.zeros(R, np.float32), terms=np.zeros((R, 4), np.float32),
                   collisions=np.zeros(R, np.int32), rows=np.zeros(R, np.int32), length=np.zeros(R, np.float64))
        sc = MppiPathScores(_fp(out["cost"]), _fp(out["terms"]), out["collisions"].ctypes.data_as(i32))
        _check(self.lib, self.lib.mppi_batch_get_runs(
            self.h, e, 0, R, st, out["steps"].ctypes.data_as(i32), out["reached"].ctypes.data_as(i32),
            out["status"].ctypes.data_as(i32), C.byref(sc), out["rows"].ctypes.data_as(i32),
            out["length"].ctypes.data_as(_DP)), "mppi_batch_get_runs")
        out["state"] = np.frombuffer(bytes(st), dtype=np.float32).reshape(R, 11).copy()
        if tr.get("metrics"):
            out["metrics"] = np.zeros((R, 4), np.float64)
            _check(self.lib, self.lib.mppi_batch_get_run_metrics(self.h, e, 0, R, out["metrics"].ctypes.data_as(_DP)),
                   "mppi_batch_get_run_metrics")
        return out

    def step_device(self, states, mask=None, reset=None, seeds=None, cmd=None, plan=None, proj="3d", z=None,
                    done=None):
        """mppi_batch_step_device: one step of every set episode from states held on the device, for a
        plant that is not the controller's own model.  Enqueues on the engine's stream and returns;
        it never synchronises, so the arrays are read and written in stream order and must stay
        alive until the step has run.

        states: float32 [E, 11] in mppi_state field order (mppi_amd.batch.pack_states), the heading
        used as given; mask, reset: int32 [E] or None (episode e steps iff mask[e] != 0; reset[e] != 0
        restarts it first: zero nominal sequence, step index 0); seeds: uint64 or int64 [E] or None,
        the new Philox key where reset[e] != 0; cmd: float32 [E, 2] (v, w); plan: float32
        [E, 4H + 12] (u1_opt, u2_opt, lin_vel, ang_vel [H] each, then row 0 of traj_sim, heading_sim,
        left_wheel_sim, right_wheel_sim).  Every array is a device array taken zero copy (a CUDA
        torch.Tensor, __cuda_array_interface__, a DLPack producer), contiguous, on the engine's
        device.  cmd / plan not given are allocated as torch tensors (uninitialised: the rows of an
        episode that does not step are not written).  Returns (cmd, plan).

        With tracking set (set_tracking) the call is mppi_batch_step_tracked: z: float32 [E] or None,
        the plant's pose height of each rover (None: the episode's DEM at its x, y), the z of the
        run's row; done: int32 [E], written at every step: 0 running (or never set), 1 reached, 2 the step
        cap; allocated as a torch tensor when not given.  Returns (cmd, plan, done).  Without
        tracking z and done are refused.
        """
        E, H = self.E, self.H
        io = MppiBatchIo()
        io.states = self._io_array(states, "states", ("f4",), (E, 11))
        if mask is not None:
            io.mask = self._io_array(mask, "mask", ("i4",), (E,))
        if reset is not None:
            io.reset = self._io_array(reset, "reset", ("i4",), (E,))
        if seeds is not None:
            io.seeds = self._io_array(seeds, "seeds", ("u8", "i8"), (E,))
        if proj not in PROJ:
            raise ValueError(f"proj must be one of {sorted(map(str, PROJ))}, got {proj!r}")
        tracked = bool(getattr(self, "tracking", None))
        if not tracked and (z is not None or done is not None):
            raise ValueError("z and done belong to tracked steps: call set_tracking first")
        z_ptr = None if z is None else self._io_array(z, "z", ("f4",), (E,))
        if cmd is None or plan is None or (tracked and done is None):
            import torch
            device = torch.device("cuda", self.engine.device)
            if cmd is None:
                cmd = torch.empty((E, 2), dtype=torch.float32, device=device)
            if plan is None:
                plan = torch.empty((E, 4 * H + 12), dtype=torch.float32, device=device)
            if tracked and done is None:
                done = torch.empty((E,), dtype=torch.int32, device=device)   # (every entry is written)
        io.cmd = self._io_array(cmd, "cmd", ("f4",), (E, 2))
        io.plan = self._io_array(plan, "plan", ("f4",), (E, 4 * H + 12))
        if not tracked:
            _check(self.lib, self.lib.mppi_batch_step_device(self.h, PROJ[proj], C.byref(io)), "mppi_batch_step_device")
            return cmd, plan
        done_ptr = self._io_array(done, "done", ("i4",), (E,))
        _check(self.lib, self.lib.mppi_batch_step_tracked(self.h, PROJ[proj], C.byref(io), z_ptr, done_ptr),
               "mppi_batch_step_tracked")
        return cmd, plan, done

    def episode(self, e):
        """dict(state (MppiState), steps_total, steps_last_run, reached, u1, u2 (the next nominal sequence))."""
        st = MppiState()
        total, last, reached = C.c_int64(), C.c_int32(), C.c_int32()
        u1 = np.zeros(self.H, np.float32)
        u2 = np.zeros(self.H, np.float32)
        _check(self.lib, self.lib.mppi_batch_get_episode(self.h, int(e), C.byref(st), C.byref(total), C.byref(last),
                                                         C.byref(reached), _fp(u1), _fp(u2)),
               "mppi_batch_get_episode")
        return dict(state=st, steps_total=total.value, steps_last_run=last.value, reached=bool(reached.value),
                    u1=u1, u2=u2)

    def log(self, e, first=0, count=None):
        """Rows [count, 8] of the most recent run: x, y, z, the normalised heading, v, w per step."""
        if count is None:
            count = self.episode(e)["steps_last_run"] - int(first)
        rows = np.zeros((max(int(count), 0), 8), np.float32)
        _check(self.lib, self.lib.mppi_batch_get_log(self.h, int(e), int(first), int(count), _fp(rows)),
               "mppi_batch_get_log")
        return rows

    # ---- the task queue: N tasks on the E episodes as lanes (mppi_batch_set_tasks / _run_tasks) ----
    def set_tasks(self, tasks, scored=None, keep_log=True, slope="body", metrics=False):
        """The batch's task list: MppiBatchTask (make_task) or dicts of make_task's arguments; an empty
        list clears it.  The results are reset.

        scored: None (a plain list), or the yardstick every task is scored with as it runs
        (mppi_batch_set_tasks_scored): True for the engine's params, or a MppiBatchVariant / dict whose
        weights, collision_threshold and collision_penalty are used; task_scores() then reads the
        scores.  keep_log=False (scored lists only): no log arena is allocated, so task_log and
        score_tasks raise and the sum of the step caps has no limit.

        slope="wheels" (scored lists): the slope term of the online score in its wheel form (the contacts
        of every executed step; no log needed); metrics=True (scored lists): a `metrics` row per task
        (compute_path_metrics; task_scores() returns it).  Both are refused for a plain list, which scores
        nothing as it runs.  scored=dict(yardstick=None | variant, slope=, metrics=) says the same in one
        argument: a dict with the key `yardstick`, `slope` or `metrics` holds exactly those keys (a
        yardstick's own fields go under `yardstick`), and then the two keywords must be left alone."""
        if isinstance(scored, dict) and (set(scored) & {"slope", "metrics", "yardstick"}):
            # the one-argument form: exactly these keys, never mixed with a yardstick's fields
            extra = set(scored) - {"slope", "metrics", "yardstick"}
            if extra:
                raise ValueError(f"scored=dict(yardstick=, slope=, metrics=) takes no other key, got {sorted(extra)}: "
                                 "a yardstick's fields go under `yardstick`")
            if slope != "body" or metrics:
                raise ValueError("give slope / metrics either as keywords or inside scored=dict(...), not both")
            slope, metrics = scored.get("slope", "body"), scored.get("metrics", False)
            scored = True if scored.get("yardstick") is None else scored["yardstick"]
        if slope not in SLOPE_MODES:
            raise ValueError(f"slope must be one of {sorted(SLOPE_MODES)}, got {slope!r}")
        if (slope != "body" or metrics) and (scored is None or scored is False):
            raise ValueError("slope / metrics belong to a scored list (scored=True or a yardstick): a plain list "
                             "scores nothing as it runs (score_tasks(slope=, metrics=) scores its log afterwards)")
        opts = dict(slope=slope, metrics=bool(metrics))
        rows = [t if isinstance(t, MppiBatchTask) else make_task(**dict(t)) for t in tasks]
        arr = (MppiBatchTask * max(len(rows), 1))(*rows)
        if (opts["slope"], opts["metrics"]) != getattr(self, "_opts", ("body", False)) and scored is not None and scored is not False:
            # (the library refuses new options while a campaign is unfinished: the old list goes first)
            _check(self.lib, self.lib.mppi_batch_set_tasks(self.h, 0, arr), "mppi_batch_set_tasks")
            self._score_options(opts["slope"], opts["metrics"])
        self.list_metrics = False
        if scored is None or scored is False:
            if not keep_log:
                raise ValueError("keep_log=False needs a scored list (scored=True or a yardstick): "
                                 "without a log nothing of a plain list's runs could be scored")
            _check(self.lib, self.lib.mppi_batch_set_tasks(self.h, len(rows), arr), "mppi_batch_set_tasks")
        else:
            y = None if scored is True else C.byref(_as_variant(scored))
            _check(self.lib, self.lib.mppi_batch_set_tasks_scored(self.h, len(rows), arr, y, 1 if keep_log else 0),
                   "mppi_batch_set_tasks_scored")
            self.list_metrics = getattr(self, "_opts", ("body", False))[1] and len(rows) > 0
        self.n_tasks = len(rows)

    def task_scores(self, first=0, count=None):
        """mppi_batch_get_task_scores: the scores the lanes computed as they ran tasks
        [first, first + count) of a scored list (count None: to the end of the list).  Returns
        dict(cost [n], terms [n, 4] in COST_TERMS order, collisions [n], rows [n], length [n] float64);
        a task that has not ended, or took no step, has zeros."""
        N = int(getattr(self, "n_tasks", 0))
        first = int(first)
        n = N - first if count is None else int(count)
        if first < 0 or n < 0 or first + n > N:
            raise ValueError(f"tasks [{first}, {first + n}) outside the list of {N} tasks")
        out = dict(cost=np.zeros(n, np.float32), terms=np.zeros((n, 4), np.float32),
                   collisions=np.zeros(n, np.int32), rows=np.zeros(n, np.int32), length=np.zeros(n, np.float64))
        i32 = C.POINTER(C.c_int32)
        sc = MppiPathScores(_fp(out["cost"]), _fp(out["terms"]), out["collisions"].ctypes.data_as(i32))
        _check(self.lib, self.lib.mppi_batch_get_task_scores(self.h, first, n, C.byref(sc),
                                                             out["rows"].ctypes.data_as(i32),
                                                             out["length"].ctypes.data_as(_DP)),
               "mppi_batch_get_task_scores")
        if getattr(self, "list_metrics", False):
            out["metrics"] = np.zeros((n, 4), np.float64)
            _check(self.lib, self.lib.mppi_batch_get_task_metrics(self.h, first, n, out["metrics"].ctypes.data_as(_DP)),
                   "mppi_batch_get_task_metrics")
        return out

    def run_tasks(self, n_steps, proj="3d", policy=None):
        """Advance the campaign by up to n_steps batch steps (it stops when every task has ended; a
        further call goes on).  Returns (tasks ended so far, batch steps of this call)."""
        pol = policy if policy is not None else make_policy()
        done, steps = C.c_int32(), C.c_int64()
        _check(self.lib, self.lib.mppi_batch_run_tasks(self.h, PROJ[proj], int(n_steps), C.byref(pol), C.byref(done),
                                                       C.byref(steps)), "mppi_batch_run_tasks")
        return done.value, steps.value

    def task(self, i):
        """dict(state (MppiState), steps, reached, started: 0 not yet claimed, 1 running, 2 ended)."""
        st = MppiState()
        steps, reached, started = C.c_int32(), C.c_int32(), C.c_int32()
        _check(self.lib, self.lib.mppi_batch_get_task(self.h, int(i), C.byref(st), C.byref(steps), C.byref(reached),
                                                      C.byref(started)), "mppi_batch_get_task")
        return dict(state=st, steps=steps.value, reached=bool(reached.value), started=started.value)

    def task_log(self, i, first=0, count=None):
        """Rows [count, 8] of task i: x, y, z, the normalised heading, v, w per step."""
        if count is None:
            count = self.task(i)["steps"] - int(first)
        rows = np.zeros((max(int(count), 0), 8), np.float32)
        _check(self.lib, self.lib.mppi_batch_get_task_log(self.h, int(i), int(first), int(count), _fp(rows)),
               "mppi_batch_get_task_log")
        return rows

    def score_tasks(self, yardstick=None, origins=None, slope="body", metrics=False):
        """mppi_batch_score_tasks: score() over the N task logs, each on its task's costmap; origins: N
        MppiState (default each task's start and goal).  Returns dict(cost [N], terms [N, 4],
        collisions [N], rows [N]); slope, metrics: as score() (mppi_batch_score_tasks_ex)."""
        if slope not in SLOPE_MODES:
            raise ValueError(f"slope must be one of {sorted(SLOPE_MODES)}, got {slope!r}")
        N = int(getattr(self, "n_tasks", 0))
        out = dict(cost=np.zeros(N, np.float32), terms=np.zeros((N, 4), np.float32),
                   collisions=np.zeros(N, np.int32), rows=np.zeros(N, np.int32))
        i32 = C.POINTER(C.c_int32)
        sc = MppiPathScores(_fp(out["cost"]), _fp(out["terms"]), out["collisions"].ctypes.data_as(i32))
        y = None if yardstick is None else C.byref(_as_variant(yardstick))
        o = None
        if origins is not None:
            origins = list(origins)
            if len(origins) != N:
                raise ValueError(f"{N} tasks but {len(origins)} origins")
            o = (MppiState * max(N, 1))(*origins)
        if slope == "body" and not metrics:
            _check(self.lib, self.lib.mppi_batch_score_tasks(self.h, y, o, C.byref(sc),
                                                             out["rows"].ctypes.data_as(i32)),
                   "mppi_batch_score_tasks")
            return out
        if metrics:
            out["metrics"] = np.zeros((N, 4), np.float64)
        _check(self.lib, self.lib.mppi_batch_score_tasks_ex(
            self.h, y, o, SLOPE_MODES[slope], C.byref(sc), out["rows"].ctypes.data_as(i32),
            out["metrics"].ctypes.data_as(_DP) if metrics else None), "mppi_batch_score_tasks_ex")
        return out

    def last_ms(self):
        ms = C.c_double()
        _check(self.lib, self.lib.mppi_batch_get_ms(self.h, C.byref(ms)), "mppi_batch_get_ms")
        return ms.value

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            if self.engine.ctx and self.engine.ctx.value:   # (a closed engine took its stream along)
                self.lib.mppi_batch_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def debug_hold(device, stream_handle, groups, lds_bytes, microseconds):
    """mppi_debug_hold (test hook): `groups` workgroups holding lds_bytes of LDS each for `microseconds`
    on the given stream (another stream's kernels occupying CUs when a step is posted)."""
    lib = load_library()
    _check(lib, lib.mppi_debug_hold(int(device), C.c_void_p(stream_handle or None), int(groups), int(lds_bytes),
                                    int(microseconds)), "mppi_debug_hold")


class Group:
    """mppi_group (include/mppi.h): one controller over n GPUs from one process.

    Member i is an Engine over the contiguous shard mppi_group_shard(i) of the K trajectories;
    setters broadcast to every member; step() runs every member's rollout (each member's launches
    enqueued by its own thread), all-gathers the records (RCCL between distinct devices, device
    copies when members share one) and returns the outputs.  When every member's shard is a
    power-of-two number of 256-trajectory leaves the member roots are subtrees of the one-context
    tree and the step is bitwise equal to one context over all K; other splits (e.g. 3 members,
    ragged K) run the same float64 combine with a different pairing.
    """

    def __init__(self, params: MppiParams, devices):
        self.lib = load_library()
        self.params = params
        self.H = int(params.num_iterations)
        self.K = int(params.num_trajectories)
        devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        _check(self.lib, self.lib.mppi_group_create(C.byref(params), len(devices), devs, C.byref(h)),
               "mppi_group_create")
        self.h = h
        self.members = []
        for i, d in enumerate(devices):
            ctx = C.c_void_p()
            _check(self.lib, self.lib.mppi_group_context(h, i, C.byref(ctx)), "mppi_group_context")
            b, n = self.shard(i)
            p = MppiParams.from_buffer_copy(params)
            p.num_trajectories = n if n > 0 else 256
            p.k_offset = int(params.k_offset) + b
            self.members.append(Engine(p, d, _ctx=ctx))

    def shard(self, i):
        b, n = C.c_int64(), C.c_int64()
        _check(self.lib, self.lib.mppi_group_shard(self.h, int(i), C.byref(b), C.byref(n)), "mppi_group_shard")
        return b.value, n.value

    def __len__(self):
        return len(self.members)

    def info(self):
        """mppi_group_info: members, distinct devices, RCCL in use, RCCL ranks, member threads, their spin
        (us) and the granted CPUs."""
        v = (C.c_int64 * 7)()
        _check(self.lib, self.lib.mppi_group_info(self.h, v, 7), "mppi_group_info")
        return dict(zip(("members", "devices", "rccl", "rccl_ranks", "threaded", "spin_us", "granted_cpus"),
                        [int(x) for x in v]))

    def _each(self, name, *a, **kw):
        for m in self.members:
            getattr(m, name)(*a, **kw)

    def set_dem(self, *a, **kw):
        self._each("set_dem", *a, **kw)

    def set_costmap(self, *a, **kw):
        self._each("set_costmap", *a, **kw)

    def set_state(self, state: MppiState):
        self._each("set_state", state)

    def set_nominal(self, u1, u2):
        self._each("set_nominal", u1, u2)

    def set_critics(self, slope="wheels", w_orientation=0.0):
        """The critic set of every member (Engine.set_critics)."""
        self._each("set_critics", slope, w_orientation)

    def set_sampling(self, antithetic=False, nominal=False, beta=0.0):
        """The sampling plan of every member (Engine.set_sampling); the members' k_offset are even
        (shards are whole leaves), so a pair never straddles two members."""
        self._each("set_sampling", antithetic, nominal, beta)

    def set_async_tail(self, on=True):
        """Deferred optimal rollout on every member (Engine.set_async_tail)."""
        self._each("set_async_tail", on)

    def step(self, proj="3d", step=0, copy=True):
        m0 = self.members[0]
        _check(self.lib, self.lib.mppi_group_step(self.h, PROJ[proj], step_word(step), C.byref(m0._out)),
               "mppi_group_step")
        return m0._outputs() if copy else None

    def outputs(self):
        """All outputs of the last step (every member's deferred optimal rollout waited for)."""
        for m in self.members[1:]:
            m.outputs()
        return self.members[0].outputs()

    def costs(self):
        """Every trajectory's cost in global order (the members' shards concatenated)."""
        return np.concatenate([m.costs()[:self.shard(i)[1]] for i, m in enumerate(self.members)])

    def cost_terms(self):
        """Every trajectory's critic terms [K, 4] and collision count [K] in global order."""
        parts = [m.cost_terms() for m in self.members]
        counts = [self.shard(i)[1] for i in range(len(self.members))]
        return (np.concatenate([t[:c] for (t, _), c in zip(parts, counts)]),
                np.concatenate([k[:c] for (_, k), c in zip(parts, counts)]))

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            for m in self.members:
                m.close()
            self.lib.mppi_group_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
