"""CPU: the host side of the tracked device steps (mppi_batch_set_tracking / _step_tracked / _get_runs,
DESIGN.md §3.7).

The prototypes and the ctypes mirrors, the null-argument refusals of the entry points, the argument
checks of Batch.set_tracking, Batch.step_device(z=, done=) and Batch.runs, which all happen before any
library call, and campaign_summary on the stacked rows of tracked runs.  No GPU.
"""
import ctypes

import numpy as np
import pytest

F32 = np.float32
NEW = ("mppi_batch_set_tracking", "mppi_batch_step_tracked", "mppi_batch_get_runs", "mppi_batch_get_run_counts")


def test_prototypes_and_struct_sizes():
    from mppi_amd import _lib
    for name in NEW:
        assert name in _lib._PROTOS, name
        assert _lib._PROTOS[name][0] is ctypes.c_int
    assert len(_lib._PROTOS["mppi_batch_set_tracking"][1]) == 6
    assert _lib._PROTOS["mppi_batch_set_tracking"][1][2] is ctypes.c_float
    assert len(_lib._PROTOS["mppi_batch_step_tracked"][1]) == 5
    assert len(_lib._PROTOS["mppi_batch_get_runs"][1]) == 11
    # the io block of the plain step did not grow: z and done are arguments of the tracked entry
    assert ctypes.sizeof(_lib.MppiBatchIo) == 48
    assert [n for n, _ in _lib.MppiBatchIo._fields_] == ["states", "mask", "reset", "seeds", "cmd", "plan"]
    assert ctypes.sizeof(_lib.MppiBatchVariant) == 56 and ctypes.sizeof(_lib.MppiState) == 44


def test_null_batch_is_refused_with_a_message():
    from mppi_amd import _lib
    lib = _lib.load_library()
    io = _lib.MppiBatchIo()
    counts = (ctypes.c_int32 * 2)()
    for rc in (lib.mppi_batch_set_tracking(None, None, 0.5, 10, 1, 1),
               lib.mppi_batch_step_tracked(None, 3, ctypes.byref(io), None, None),
               lib.mppi_batch_get_runs(None, 0, 0, 1, None, None, None, None, None, None, None),
               lib.mppi_batch_get_run_counts(None, counts)):
        assert rc != 0
        assert b"null" in lib.mppi_last_error()


class _Cai:
    """A device array as a Warp array shows itself: __cuda_array_interface__ only (no memory behind it)."""

    def __init__(self, shape, typestr="<f4", strides=None):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(0x7f0000000000, False),
                                             version=3, strides=strides)


class _Refusing:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the arguments were checked")


def _stub_batch(E=3, H=20, tracking=None):
    """A Batch that was never created: any library call fails the test."""
    from mppi_amd import _lib
    b = _lib.Batch.__new__(_lib.Batch)
    b.E, b.H, b.lib, b.h = E, H, _Refusing(), ctypes.c_void_p()
    b.engine = type("Eng", (), dict(device=0, ctx=None))()
    if tracking:
        b.tracking = dict(tracking)
    return b


TRACK = dict(max_steps=10, runs_per_episode=2, keep_log=True)


def test_set_tracking_checks_its_arguments_before_any_library_call():
    b = _stub_batch()
    with pytest.raises(ValueError, match="needs max_steps"):
        b.set_tracking()
    with pytest.raises(ValueError, match="max_steps must be >= 1"):
        b.set_tracking(max_steps=0)
    with pytest.raises(ValueError, match="runs_per_episode must be >= 1"):
        b.set_tracking(max_steps=5, runs_per_episode=0)
    with pytest.raises(ValueError, match="goal_tol must be >= 0"):
        b.set_tracking(max_steps=5, goal_tol=-1.0)
    with pytest.raises(ValueError, match="goal_tol must be >= 0"):
        b.set_tracking(max_steps=5, goal_tol=float("nan"))
    with pytest.raises(ValueError, match="not fields of mppi_batch_variant"):
        b.set_tracking(dict(w_pathh=1.0), max_steps=5)
    assert not getattr(b, "tracking", None)


def test_set_and_clear_tracking_reach_the_library():
    from mppi_amd import _lib
    b = _stub_batch()
    seen = []

    class Lib:
        def mppi_batch_set_tracking(self, h, y, tol, max_steps, runs, keep):
            w = None if y is None else ctypes.cast(y, ctypes.POINTER(_lib.MppiBatchVariant)).contents.w_path
            seen.append((w, tol, max_steps, runs, keep))
            return 0
    b.lib = Lib()
    b.set_tracking(max_steps=40)
    assert b.tracking == dict(max_steps=40, runs_per_episode=1, keep_log=True)
    b.set_tracking(dict(w_path=2.0), max_steps=7, runs_per_episode=3, keep_log=False, goal_tol=0.25)
    assert b.tracking == dict(max_steps=7, runs_per_episode=3, keep_log=False)
    b.clear_tracking()
    assert b.tracking is None
    assert seen == [(None, 0.5, 40, 1, 1), (2.0, 0.25, 7, 3, 0), (None, 0.0, 0, 0, 0)]


def test_z_and_done_are_refused_without_tracking():
    b = _stub_batch()
    E, H = b.E, b.H
    good = dict(states=_Cai((E, 11)), cmd=_Cai((E, 2)), plan=_Cai((E, 4 * H + 12)))
    with pytest.raises(ValueError, match="set_tracking first"):
        b.step_device(z=_Cai((E,)), **good)
    with pytest.raises(ValueError, match="set_tracking first"):
        b.step_device(done=_Cai((E,), "<i4"), **good)
    with pytest.raises(RuntimeError, match="tracking is not set"):
        b.runs()
    with pytest.raises(RuntimeError, match="tracking is not set"):
        b.run_counts()


def test_tracked_step_checks_z_and_done_before_any_library_call():
    b = _stub_batch(tracking=TRACK)
    E, H = b.E, b.H
    good = dict(states=_Cai((E, 11)), cmd=_Cai((E, 2)), plan=_Cai((E, 4 * H + 12)), done=_Cai((E,), "<i4"))
    with pytest.raises(ValueError, match="z must be float32"):
        b.step_device(z=_Cai((E,), "<f8"), **good)
    with pytest.raises(ValueError, match=r"z must have shape \(3,\)"):
        b.step_device(z=_Cai((E, 1)), **good)
    with pytest.raises(TypeError, match="z must be a device array"):
        b.step_device(z=np.zeros(E, F32), **good)
    with pytest.raises(ValueError, match="z must be C-contiguous"):
        b.step_device(z=_Cai((E,), strides=(8,)), **good)
    with pytest.raises(ValueError, match="done must be int32"):
        b.step_device(**{**good, "done": _Cai((E,), "<f4")})
    with pytest.raises(ValueError, match=r"done must have shape \(3,\)"):
        b.step_device(**{**good, "done": _Cai((E + 1,), "<i4")})
    with pytest.raises(TypeError, match="done must be a device array"):
        b.step_device(**{**good, "done": np.zeros(E, np.int32)})
    # the other arrays' checks stand in tracked mode
    with pytest.raises(ValueError, match="states must be float32"):
        b.step_device(**{**good, "states": _Cai((E, 11), "<f8")})
    with pytest.raises(ValueError, match=r"episode 3 outside \[0, 3\)"):
        b.runs(3)


def test_good_arguments_reach_the_tracked_entry_once():
    from mppi_amd import _lib
    b = _stub_batch(tracking=TRACK)
    E, H = b.E, b.H
    seen = []

    class Lib:
        def mppi_batch_step_tracked(self, h, proj, io, z, done):
            got = ctypes.cast(io, ctypes.POINTER(_lib.MppiBatchIo)).contents
            seen.append((proj, got.states, got.mask, got.reset, got.seeds, got.cmd, got.plan, z, done))
            return 0
    b.lib = Lib()
    cmd, plan, done = _Cai((E, 2)), _Cai((E, 4 * H + 12)), _Cai((E,), "<i4")
    out = b.step_device(_Cai((E, 11)), reset=_Cai((E,), "<i4"), cmd=cmd, plan=plan, proj="2d", z=_Cai((E,)), done=done)
    assert out == (cmd, plan, done)
    out = b.step_device(_Cai((E, 11)), cmd=cmd, plan=plan, done=done)
    assert out == (cmd, plan, done)
    p = 0x7f0000000000
    assert seen == [(2, p, None, p, None, p, p, p, p), (3, p, None, None, None, p, p, None, p)]


def test_runs_reads_every_row_of_an_episode():
    """runs(e) asks for the episode's runs_per_episode rows in one call and unpacks the states."""
    from mppi_amd import _lib
    b = _stub_batch(tracking=TRACK)
    calls = []

    class Lib:
        def mppi_batch_get_runs(self, h, e, first, count, states, steps, reached, status, out, rows, length):
            calls.append((e, first, count))
            for i in range(count):
                states[i].x, states[i].goal_y = 10.0 * e + i, -1.0
                steps[i], reached[i], status[i], rows[i], length[i] = 3 + i, i, 1 + i, 3 + i, 0.5 * (i + 1)
            sc = ctypes.cast(out, ctypes.POINTER(_lib.MppiPathScores)).contents
            sc.cost[0], sc.terms[5], sc.collisions[1] = 7.0, 2.5, 4
            return 0
    b.lib = Lib()
    r = b.runs(1)
    assert calls == [(1, 0, 2)]
    assert r["state"].shape == (2, 11) and r["state"][:, 0].tolist() == [10.0, 11.0] and (r["state"][:, 8] == -1).all()
    assert r["steps"].tolist() == [3, 4] and r["status"].tolist() == [1, 2] and r["run"].tolist() == [0, 1]
    assert r["cost"][0] == 7.0 and r["terms"][1, 1] == 2.5 and r["collisions"][1] == 4
    assert r["length"].dtype == np.float64 and r["length"].tolist() == [0.5, 1.0]
    stacked = b.runs()
    assert stacked["episode"].tolist() == [0, 0, 1, 1, 2, 2] and stacked["state"].shape == (6, 11)
    assert stacked["terms"].shape == (6, 4) and stacked["run"].tolist() == [0, 1] * 3


def _stacked():
    """Three episodes, two result rows each: episode 0 ran twice, episode 1 once (its second row is
    empty), episode 2 ended one run and abandoned one."""
    n = 6
    runs = dict(episode=np.repeat(np.arange(3, dtype=np.int32), 2), run=np.tile(np.arange(2, dtype=np.int32), 3),
                status=np.array([1, 2, 1, 0, 2, 3], np.int32), reached=np.array([1, 0, 1, 0, 0, 0], np.int32),
                steps=np.array([4, 10, 6, 0, 10, 3], np.int32), cost=np.arange(1, n + 1, dtype=F32),
                terms=np.arange(4 * n, dtype=F32).reshape(n, 4), collisions=np.array([0, 2, 0, 0, 1, 5], np.int32),
                rows=np.array([4, 10, 6, 0, 10, 3], np.int32), length=np.linspace(1.0, 2.0, n))
    return runs


def test_campaign_summary_on_stacked_runs():
    from mppi_amd.batch import campaign_summary, tracked_results
    runs = _stacked()
    table = campaign_summary(runs, by=["2d", "3d", "2d"])
    assert list(table) == ["2d", "3d"]
    assert table["2d"]["count"] == 3 and table["2d"]["reached"] == 1 and table["2d"]["collided"] == 2
    assert table["3d"]["count"] == 1 and table["3d"]["reached"] == 1 and table["3d"]["collided"] == 0
    assert table["2d"]["mean"]["cost"] == pytest.approx(np.mean([1.0, 2.0, 5.0]))
    assert table["2d"]["mean"]["path"] == pytest.approx(np.mean([0.0, 4.0, 16.0]))
    assert table["3d"]["mean"]["length"] == pytest.approx(runs["length"][2])
    # the same table as the per-task form gives the same rows
    rows, keys = tracked_results(runs, ["2d", "3d", "2d"])
    assert [r["episode"] for r in rows] == [0, 0, 1, 2] and keys == ["2d", "2d", "3d", "2d"]
    assert campaign_summary(rows, keys) == table
    # one group; the abandoned run on request
    assert campaign_summary(runs)[None]["count"] == 4
    rows, keys = tracked_results(runs, abandoned=True)
    assert len(rows) == 5 and rows[-1]["status"] == 3 and keys == [None] * 5
    with pytest.raises(ValueError, match="3 episodes but 2 group keys"):
        campaign_summary(runs, by=["a", "b"])
