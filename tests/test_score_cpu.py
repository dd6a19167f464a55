"""Host side of path scoring: _lib.check_paths and the null-context refusals of the C-ABI (no GPU)."""
import ctypes as C

import numpy as np
import pytest

from mppi_amd import _lib


def _paths(n=3, L=5):
    rng = np.random.default_rng(0)
    return rng.standard_normal((n, L, 3)), rng.random((n, L))


def test_check_paths_accepts_and_normalises():
    traj, v = _paths()
    n, L, t, vv, lw, rw, ln = _lib.check_paths(traj.tolist(), v.astype(np.float64))
    assert (n, L) == (3, 5) and lw is None and rw is None and ln is None
    assert t.dtype == np.float32 and t.flags.c_contiguous and t.shape == (3, 5, 3)
    assert vv.dtype == np.float32 and vv.flags.c_contiguous and vv.shape == (3, 5)
    np.testing.assert_array_equal(t, traj.astype(np.float32))
    # non-contiguous wheel arrays and a list of lengths come back contiguous float32 / int32
    wheels = np.asfortranarray(traj)
    n, L, t, vv, lw, rw, ln = _lib.check_paths(traj, v, wheels, wheels[::1], lengths=[1, 5, 3])
    assert lw.flags.c_contiguous and rw.flags.c_contiguous and lw.dtype == np.float32
    assert ln.dtype == np.int32 and ln.tolist() == [1, 5, 3]
    # no path at all is valid input
    assert _lib.check_paths(np.zeros((0, 4, 3)), np.zeros((0, 4)))[:2] == (0, 4)


@pytest.mark.parametrize("bad", [
    dict(traj=np.zeros((3, 5))),                        # wrong rank
    dict(traj=np.zeros((3, 5, 2))),                     # not x, y, z
    dict(traj=np.zeros((3, 0, 3)), lin_vel=np.zeros((3, 0))),   # no waypoint
    dict(lin_vel=np.zeros((3, 4))),                     # lin_vel of another length
    dict(lin_vel=np.zeros((3, 5, 1))),
    dict(left_wheel=np.zeros((3, 5, 3))),               # one wheel array without the other
    dict(right_wheel=np.zeros((3, 5, 3))),
    dict(left_wheel=np.zeros((3, 5, 3)), right_wheel=np.zeros((3, 4, 3))),
    dict(lengths=[1, 2]),                               # wrong size
    dict(lengths=[[1, 2, 3]]),
    dict(lengths=[0, 2, 3]),                            # out of range
    dict(lengths=[1, 2, 6]),
    dict(lengths=[1.0, 2.0, 3.0]),                      # not integers
])
def test_check_paths_rejects(bad):
    traj, v = _paths()
    kw = dict(traj=traj, lin_vel=v)
    kw.update(bad)
    with pytest.raises(ValueError):
        _lib.check_paths(**kw)


def test_null_context_is_refused_without_a_device():
    lib = _lib.load_library()
    traj = np.zeros((1, 2, 3), np.float32)
    v = np.zeros((1, 2), np.float32)
    out = _lib.MppiPathScores()
    terms = np.zeros(4, np.float32)
    ms = C.c_double()
    calls = (
        lambda: lib.mppi_score_paths(None, 1, 2, None, _lib._fp(traj), None, None, _lib._fp(v), None, C.byref(out)),
        lambda: lib.mppi_get_cost_terms(None, _lib._fp(terms), None),
        lambda: lib.mppi_get_score_ms(None, C.byref(ms)),
    )
    for call in calls:
        assert call() == -1   # MPPI_EINVAL
        assert "null" in lib.mppi_last_error().decode()
