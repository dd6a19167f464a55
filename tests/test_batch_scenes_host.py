"""CPU: the host side of per-episode scenes and trajectory counts of the batched episodes
(include/mppi.h mppi_batch_set_dem, mppi_batch_set_costmap, mppi_batch_build_costmap,
mppi_batch_set_episode_scene, mppi_batch_set_episode_trajectories).  No device is
touched."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from mppi_amd import _lib
from mppi_amd import batch as MB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mppi.h")
KERNELS_H = os.path.join(ROOT, "husky-rover-mppi-isaacsim_amd", "csrc", "mppi_kernels.h")
NEW = ("mppi_batch_set_dem", "mppi_batch_set_costmap", "mppi_batch_build_costmap", "mppi_batch_set_episode_scene",
       "mppi_batch_set_episode_trajectories")


def test_header_exports_and_prototypes_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"^[A-Za-z_][\w\s\*]*?\b(mppi_\w+)\s*\(", text, flags=re.M))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW:
        assert name in declared and name in exported and name in _lib._PROTOS, name
    assert set(_lib._PROTOS) == declared


def test_prototypes_have_the_declared_arity():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        assert len(args.split(",")) == len(_lib._PROTOS[name][1]), name
    assert _lib._PROTOS["mppi_batch_set_episode_trajectories"][1][2] is C.c_int64


def test_slot_limits_are_the_kernels():
    text = open(KERNELS_H).read()
    assert int(re.search(r"kBatchMaxDems = (\d+)", text).group(1)) == MB.MAX_DEM_SLOTS == 256
    assert int(re.search(r"kBatchMaxCostmaps = (\d+)", text).group(1)) == MB.MAX_COSTMAP_SLOTS == 1024
    # the episode table's record did not grow: the scene record is a parallel array
    assert re.search(r"static_assert\(sizeof\(BatchEpisode\) == 96", text)
    assert re.search(r"static_assert\(sizeof\(BatchScene\) == 16", text)


def test_new_entry_points_refuse_a_null_batch():
    lib = _lib.load_library()
    z = np.zeros(4, np.float32)
    obs = np.zeros(3, np.float64)
    calls = {
        "mppi_batch_set_dem": lambda: lib.mppi_batch_set_dem(None, 0, _lib._fp(z)),
        "mppi_batch_set_costmap": lambda: lib.mppi_batch_set_costmap(None, 0, _lib._fp(z)),
        "mppi_batch_build_costmap": lambda: lib.mppi_batch_build_costmap(None, 0, obs.ctypes.data_as(_lib._DP), 1, 0.0, 0.0,
                                                                         0.3, 20, 0, None),
        "mppi_batch_set_episode_scene": lambda: lib.mppi_batch_set_episode_scene(None, 0, -1, -1),
        "mppi_batch_set_episode_trajectories": lambda: lib.mppi_batch_set_episode_trajectories(None, 0, 0),
    }
    assert set(calls) == set(NEW)
    for name, call in calls.items():
        assert call() == -1, name
        assert b"null batch" in lib.mppi_last_error(), name


def test_python_signatures():
    sig = inspect.signature(_lib.Batch.set_episode).parameters
    assert [(n, sig[n].default) for n in ("variant", "dem", "costmap", "trajectories")] == \
        [("variant", -1), ("dem", -1), ("costmap", -1), ("trajectories", 0)]
    sig = inspect.signature(_lib.Batch.build_costmap).parameters
    assert list(sig)[1:] == ["slot", "obstacles", "origin", "r_robot", "power", "metric", "copy_out"]
    assert (sig["power"].default, sig["metric"].default, sig["copy_out"].default) == (20, "chamfer", False)
    assert list(inspect.signature(_lib.Batch.set_dem).parameters)[1:] == ["slot", "Z"]
    assert list(inspect.signature(_lib.Batch.set_costmap).parameters)[1:] == ["slot", "cm"]
    from mppi_amd import controller
    sig = inspect.signature(controller.MPPI_Controller.run_batch).parameters
    for n in ("dems", "costmaps", "episode_dem", "episode_costmap", "episode_trajectories"):
        assert sig[n].default is None, n


def test_episode_scenes_defaults_and_passthrough():
    assert MB.episode_scenes(3, 512) == ([-1] * 3, [-1] * 3, [0] * 3)
    ed, ec, ek = MB.episode_scenes(3, 512, dems=["a", "b"], costmaps=["c"], episode_dem=[1, None, 0],
                                   episode_costmap=[-1, 0, None], episode_trajectories=[300, None, 512])
    assert (ed, ec, ek) == ([1, -1, 0], [-1, 0, -1], [300, 0, 512])
    # tables without indices, and K_e alone, are fine
    assert MB.episode_scenes(2, 512, dems=["a"])[0] == [-1, -1]
    assert MB.episode_scenes(2, 512, episode_trajectories=[1, 0])[2] == [1, 0]


@pytest.mark.parametrize("kw, word", [
    (dict(episode_dem=[0, 0]), "episode_dem"),                                  # length
    (dict(episode_costmap=[0] * 4), "episode_costmap"),
    (dict(episode_trajectories=[1]), "episode_trajectories"),
    (dict(episode_dem=[0, -1, -1]), "dems"),                                    # index without a table
    (dict(episode_costmap=[-1, -1, 2]), "costmaps"),
    (dict(dems=["a"], episode_dem=[0, 1, -1]), "episode_dem[1]"),               # outside the table
    (dict(costmaps=["a", "b"], episode_costmap=[2, 0, 0]), "episode_costmap[0]"),
    (dict(dems=["a"], episode_dem=[-2, 0, 0]), "episode_dem[0]"),
    (dict(episode_trajectories=[513, 0, 0]), "episode_trajectories[0]"),        # K_e outside [1, K]
    (dict(episode_trajectories=[0, -5, 0]), "episode_trajectories[1]"),
    (dict(dems=["z"] * 257), "dems"),                                           # more slots than the batch has
    (dict(costmaps=["c"] * 1025), "costmaps"),
])
def test_episode_scenes_refuses(kw, word):
    with pytest.raises(ValueError) as err:
        MB.episode_scenes(3, 512, **kw)
    assert word in str(err.value)


def test_run_batch_checks_before_touching_the_engine():
    """run_batch validates the scene arguments before it creates the engine (no device here)."""
    from mppi_amd import controller
    ctl = controller.MPPI_Controller.__new__(controller.MPPI_Controller)
    ctl.seed = 1
    ctl.number_of_trajectories = 512
    ctl.engine = None
    ctl.warp_setup = lambda: pytest.fail("the engine was set up before the arguments were checked")
    starts, heads, goals = [(0.0, 0.0)] * 2, [(1.0, 0.0, 0.0)] * 2, [(1.0, 1.0)] * 2
    for kw in (dict(episode_dem=[0, -1]), dict(episode_costmap=[0]), dict(episode_trajectories=[0, 600]),
               dict(dems=[np.zeros((4, 4))], episode_dem=[1, 0])):
        with pytest.raises(ValueError):
            ctl.run_batch(starts, heads, goals, **kw)
