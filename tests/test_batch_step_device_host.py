"""CPU: the host side of the batch's device-resident step (mppi_batch_step_device).

The state packing, the ctypes mirror of mppi_batch_io, the null-argument refusal of the entry point
and the argument checks of Batch.step_device, which all happen before any library call.  No GPU.
"""
import ctypes

import numpy as np
import pytest

F32 = np.float32


def test_pack_states_round_trip_and_field_order():
    """pack_states writes mppi_state's fields in the struct's own order; unpack_states inverts it."""
    from mppi_amd import _lib
    from mppi_amd.batch import STATE_WIDTH, pack_states, state_dict, to_mppi_state, unpack_states
    rng = np.random.default_rng(5)
    states = [state_dict(*rng.normal(size=2), rng.normal(size=3), *rng.normal(size=6)) for _ in range(4)]
    rows = pack_states(states)
    assert rows.dtype == F32 and rows.shape == (4, 11) and STATE_WIDTH == 11
    assert ctypes.sizeof(_lib.MppiState) == 11 * 4
    for s, row in zip(states, rows):
        raw = np.frombuffer(bytes(to_mppi_state(s)), dtype=F32)    # the struct as the C side reads it
        assert np.array_equal(raw.view(np.uint32), row.view(np.uint32))
    order = [n for n, _ in _lib.MppiState._fields_]
    assert order == ["x", "y", "heading", "left_wheel_speed", "right_wheel_speed", "goal_x", "goal_y", "std_dev_u1",
                     "std_dev_u2"]
    marked = pack_states([state_dict(1, 2, (3, 4, 5), 6, 7, 8, 9, 10, 11)])
    assert marked.tolist() == [[1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]]
    back = unpack_states(rows)
    assert np.array_equal(pack_states(back).view(np.uint32), rows.view(np.uint32))
    for s, t in zip(states, back):
        assert set(s) == set(t)
    assert pack_states([]).shape == (0, 11)
    with pytest.raises(ValueError, match="shape"):
        unpack_states(np.zeros((3, 10), F32))


def test_batch_io_mirror_is_six_pointers():
    from mppi_amd import _lib
    assert ctypes.sizeof(_lib.MppiBatchIo) == 6 * ctypes.sizeof(ctypes.c_void_p)
    assert [n for n, _ in _lib.MppiBatchIo._fields_] == ["states", "mask", "reset", "seeds", "cmd", "plan"]
    assert "mppi_batch_step_device" in _lib._PROTOS


def test_null_batch_is_refused_with_a_message():
    from mppi_amd import _lib
    lib = _lib.load_library()
    io = _lib.MppiBatchIo()
    assert lib.mppi_batch_step_device(None, 3, ctypes.byref(io)) != 0
    assert b"null" in lib.mppi_last_error()
    assert lib.mppi_batch_step_device(None, 3, None) != 0
    assert b"null" in lib.mppi_last_error()


class _Cai:
    """A device array as a Warp array shows itself: __cuda_array_interface__ only (no memory behind it)."""

    def __init__(self, shape, typestr="<f4", strides=None):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(0x7f0000000000, False),
                                             version=3, strides=strides)


class _Refusing:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the arguments were checked")


def _stub_batch(E=3, H=20):
    """A Batch that was never created: any library call fails the test."""
    from mppi_amd import _lib
    b = _lib.Batch.__new__(_lib.Batch)
    b.E, b.H, b.lib, b.h = E, H, _Refusing(), ctypes.c_void_p()
    b.engine = type("Eng", (), dict(device=0, ctx=None))()
    return b


def test_step_device_checks_its_arguments_before_any_library_call():
    b = _stub_batch()
    E, H = b.E, b.H
    good = dict(states=_Cai((E, 11)), cmd=_Cai((E, 2)), plan=_Cai((E, 4 * H + 12)))
    # a wrong dtype
    with pytest.raises(ValueError, match="states must be float32"):
        b.step_device(**{**good, "states": _Cai((E, 11), "<f8")})
    with pytest.raises(ValueError, match="mask must be int32"):
        b.step_device(mask=_Cai((E,), "<f4"), **good)
    with pytest.raises(ValueError, match="reset must be int32"):
        b.step_device(reset=_Cai((E,), "<i8"), **good)
    with pytest.raises(ValueError, match="seeds must be uint64 or int64"):
        b.step_device(seeds=_Cai((E,), "<i4"), **good)
    with pytest.raises(ValueError, match="plan must be float32"):
        b.step_device(**{**good, "plan": _Cai((E, 4 * H + 12), "<f2")})
    # a wrong shape
    with pytest.raises(ValueError, match=r"states must have shape \(3, 11\)"):
        b.step_device(**{**good, "states": _Cai((E, 10))})
    with pytest.raises(ValueError, match=r"states must have shape"):
        b.step_device(**{**good, "states": _Cai((E * 11,))})
    with pytest.raises(ValueError, match=r"mask must have shape \(3,\)"):
        b.step_device(mask=_Cai((E + 1,), "<i4"), **good)
    with pytest.raises(ValueError, match=r"cmd must have shape \(3, 2\)"):
        b.step_device(**{**good, "cmd": _Cai((E, 3))})
    with pytest.raises(ValueError, match=r"plan must have shape \(3, 92\)"):
        b.step_device(**{**good, "plan": _Cai((E, 4 * H))})
    # a host array
    with pytest.raises(TypeError, match="states must be a device array"):
        b.step_device(**{**good, "states": np.zeros((E, 11), F32)})
    with pytest.raises(TypeError, match="mask must be a device array"):
        b.step_device(mask=[1, 1, 1], **good)
    with pytest.raises(TypeError, match="cmd must be a device array"):
        b.step_device(**{**good, "cmd": np.zeros((E, 2), F32)})
    # not contiguous
    with pytest.raises(ValueError, match="states must be C-contiguous"):
        b.step_device(**{**good, "states": _Cai((E, 11), strides=(88, 4))})
    with pytest.raises(ValueError, match="proj"):
        b.step_device(proj="4d", **good)


def test_step_device_refuses_host_and_strided_tensors():
    """The same checks on torch tensors: a CPU tensor is a host array; the stub fails any library call."""
    torch = pytest.importorskip("torch")
    b = _stub_batch()
    E, H = b.E, b.H
    good = dict(cmd=_Cai((E, 2)), plan=_Cai((E, 4 * H + 12)))
    with pytest.raises(TypeError, match="states must be a device array"):
        b.step_device(torch.zeros((E, 11)), **good)
    with pytest.raises(TypeError, match="seeds must be a device array"):
        b.step_device(_Cai((E, 11)), seeds=torch.zeros(E, dtype=torch.int64), **good)


def test_good_arguments_reach_the_library_once():
    """With every argument in order the one library call is mppi_batch_step_device, with the pointers given."""
    from mppi_amd import _lib
    b = _stub_batch()
    E, H = b.E, b.H
    seen = []

    class Lib:
        def mppi_batch_step_device(self, h, proj, io):
            got = ctypes.cast(io, ctypes.POINTER(_lib.MppiBatchIo)).contents
            seen.append((proj, got.states, got.mask, got.reset, got.seeds, got.cmd, got.plan))
            return 0
    b.lib = Lib()
    cmd, plan = _Cai((E, 2)), _Cai((E, 4 * H + 12))
    out = b.step_device(_Cai((E, 11)), mask=_Cai((E,), "<i4"), seeds=_Cai((E,), "<u8"), cmd=cmd, plan=plan, proj="2d")
    assert out == (cmd, plan)
    p = 0x7f0000000000
    assert seen == [(2, p, p, None, p, p, p)]
