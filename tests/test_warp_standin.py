"""CPU: the Warp stand-in alone (oracle/warp_standin.py).  The reference-run fixture
tests/golden/ref_warp_steps.npz is only as good as these properties: strict float32 in source order,
truncating ints, checked indices, annotation-driven arguments, ordered atomics, recorded noise."""
import math

import numpy as np
import pytest

from oracle import dmath
from oracle import warp_standin as W

F32 = np.float32


@pytest.fixture()
def wp():
    return W.create("project")


def test_every_operation_rounds_to_float32(wp):
    @wp.kernel
    def k(x: wp.array(dtype=float), y: wp.array(dtype=float), out: wp.array(dtype=float)):
        t = wp.tid()
        out[t] = x[t] * 0.1 + y[t]

    rng = np.random.default_rng(0)
    x = rng.uniform(-100, 100, 257).astype(F32)
    y = rng.uniform(-1, 1, 257).astype(F32)
    out = wp.zeros(257, dtype=float)
    wp.launch(k, dim=257, inputs=[wp.array(x, dtype=float), wp.array(y, dtype=float), out])
    want = (x * F32(0.1)).astype(F32) + y                      # F32(F32(x * F32(0.1)) + y)
    got = out.numpy()
    assert got.dtype == F32 and np.array_equal(got, want)
    fused = (x.astype(np.float64) * np.float64(F32(0.1)) + y).astype(F32)      # one rounding: an fma
    double = (x.astype(np.float64) * 0.1 + y).astype(F32)                      # the literal as a double
    assert (got != fused).any() and (got != double).any(), "the case cannot tell the roundings apart"


def test_scalar_types(wp):
    assert [wp.int(F32(v)) for v in (-0.9, -1.0, -1.5, -2.999, 0.9, 2.999, -0.0)] == [0, -1, -1, -2, 0, 2, 0]
    assert all(type(wp.int(F32(v))) is int for v in (-1.5, 1.5))
    assert -wp.int(F32(-3.7)) == 3                              # the row index form: -int(f), not int(-f) of a floor
    for f in (wp.float, wp.float32):
        r = f(0.1)
        assert type(r) is F32 and r == F32(0.1) and float(r) != 0.1
        assert type(f(7)) is F32
    assert wp.uint32(-1) == 0xFFFFFFFF and wp.uint32(2 ** 32 + 5) == 5
    assert type(wp.trunc(F32(-2.5))) is F32 and wp.trunc(F32(-2.5)) == -2.0
    assert wp.clamp(5.0, -1.0, 1.0) == 1.0 and wp.clamp(-5.0, -1.0, 1.0) == -1.0 and wp.clamp(0.25, -1, 1) == 0.25


def test_indices_never_wrap(wp):
    a = wp.zeros(5, dtype=float)
    v = wp.zeros(5, dtype=wp.vec3f)
    for arr in (a, v):
        for bad in (5, -1, 2 ** 31):
            with pytest.raises(IndexError):
                arr[bad]
        with pytest.raises(IndexError):
            arr[-1] = arr[0]
        with pytest.raises(TypeError):
            arr[F32(1.0)]
    with pytest.raises(IndexError):
        v[0][3]

    @wp.kernel
    def reads_past(a: wp.array(dtype=float), n: int):
        a[wp.tid()] = a[wp.tid() + n]

    with pytest.raises(IndexError):
        wp.launch(reads_past, dim=5, inputs=[a, 1])
    with pytest.raises(IndexError):
        wp.launch(reads_past, dim=5, inputs=[a, -1])


def test_arguments_follow_the_annotations(wp):
    seen = {}

    @wp.kernel
    def k(f: float, n: int, g: wp.float32, v: wp.vec2f, a: wp.array(dtype=wp.vec3f), as_float: float):
        seen.update(f=f, n=n, g=g, v=v, a=a, as_float=as_float)

    arr = wp.zeros(2, dtype=wp.vec3f)
    wp.launch(k, dim=1, inputs=[0.1, np.int64(7), np.float64(1.0) / 3.0, wp.vec2f(0.1, 2), arr, 3])
    assert type(seen["f"]) is F32 and seen["f"] == F32(0.1)
    assert type(seen["n"]) is int and seen["n"] == 7
    assert type(seen["g"]) is F32 and seen["g"] == F32(1.0 / 3.0)
    assert type(seen["as_float"]) is F32 and seen["as_float"] == 3.0       # an int for a float parameter
    assert type(seen["v"][0]) is F32 and seen["v"][0] == F32(0.1)
    assert seen["a"] is arr
    with pytest.raises(TypeError):
        wp.launch(k, dim=1, inputs=[0.1, 7.5, 1.0, wp.vec2f(0, 0), arr, 3])     # 7.5 is no int
    with pytest.raises(TypeError):
        wp.launch(k, dim=1, inputs=[0.1, 7, 1.0, wp.vec2f(0, 0), wp.zeros(2, dtype=float), 3])
    with pytest.raises(TypeError):
        wp.launch(k, dim=1, inputs=[0.1, 7, 1.0, wp.vec2f(0, 0), arr])

    @wp.func
    def f(x: float, i: int) -> float:
        return x, i

    x, i = f(0.1, np.int32(3))
    assert type(x) is F32 and type(i) is int


def test_threads_run_in_ascending_order_and_atomics_follow(wp):
    order = []

    @wp.kernel
    def k(w: wp.array(dtype=float), s: wp.array(dtype=float), m: wp.array(dtype=float)):
        t = wp.tid()
        order.append(t)
        wp.atomic_add(s, 0, w[t])
        wp.atomic_min(m, 0, w[t])

    w = np.array([1.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24], F32)
    sums = []
    for perm in ([0, 1, 2, 3, 4], [1, 2, 3, 4, 0]):
        s = wp.array([0.0], dtype=float)
        m = wp.array([np.inf], dtype=float)
        order.clear()
        wp.launch(k, dim=5, inputs=[wp.array(w[perm], dtype=float), s, m])
        assert order == [0, 1, 2, 3, 4]
        want = F32(0.0)
        for x in w[perm]:
            want = want + x
        assert s.numpy()[0] == want and m.numpy()[0] == F32(2.0 ** -24)
        sums.append(s.numpy()[0])
    # the sum depends on the launch order: 1 + four halves of an ulp stays 1 when they arrive one at
    # a time after the 1, and is 1 + 2^-22 when they are summed first
    assert sums == [F32(1.0), F32(1.0) + F32(2.0 ** -22)]
    assert wp.array(w, dtype=float).numpy().dtype == F32


def test_dot_is_left_to_right_and_cross_rounds_each_product(wp):
    a = wp.vec3f(1.0, 2.0 ** -12, 2.0 ** -12)
    b = wp.vec3f(1.0, 2.0 ** -12, 2.0 ** -12)
    # (1 + 2^-24) + 2^-24 = 1 in float32 left to right; 1 + (2^-24 + 2^-24) = 1 + 2^-23
    assert wp.dot(a, b) == F32(1.0)
    assert F32(1.0) + (F32(2.0 ** -24) + F32(2.0 ** -24)) != F32(1.0)
    rng = np.random.default_rng(1)
    for _ in range(50):
        p, q = rng.normal(size=3).astype(F32), rng.normal(size=3).astype(F32)
        d = wp.dot(wp.vec3f(p), wp.vec3f(q))
        assert type(d) is F32 and d == (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]
        c = wp.cross(wp.vec3f(p), wp.vec3f(q))
        assert [c[0], c[1], c[2]] == [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]
        d2 = wp.dot(wp.vec2f(p[:2]), wp.vec2f(q[:2]))
        assert d2 == p[0] * q[0] + p[1] * q[1]


def test_small_types_stay_float32_and_copy(wp):
    v = wp.vec3f(0.1, 0.2, 0.3)
    s = F32(1.0) / F32(3.0)
    for r in (v * s, s * v, v / s, v + v, v - v, -v, 0.2 * v, v * 0.2):
        assert isinstance(r, wp.vec3f) and all(type(x) is F32 for x in r)
    assert (s * v)[1] == s * F32(0.2) and (v / s)[2] == F32(0.3) / s and (0.2 * v)[0] == F32(0.2) * F32(0.1)
    arr = wp.zeros(2, dtype=wp.vec3f)
    got = arr[0]
    got[0] = 5.0
    assert arr.numpy()[0, 0] == 0.0                            # a read is a copy
    arr[1] = v
    assert np.array_equal(arr.numpy()[1], np.array([0.1, 0.2, 0.3], F32))
    q = wp.zeros(1, dtype=wp.mat22f)
    m = q[0]
    m[0, 1] = 0.1
    q[0] = m
    assert q.numpy()[0, 0, 1] == F32(0.1) and type(q[0][0, 1]) is F32
    with pytest.raises(TypeError):
        v + wp.vec2f(1, 2)
    host = wp.array([wp.vec2f(1.5, -2.5)] * 3, dtype=wp.vec2f)
    assert host.numpy().shape == (3, 2) and host[2][1] == -2.5
    z = wp.array(np.arange(4, dtype=np.float64) * 0.1, dtype=wp.float32)
    z2 = wp.zeros(4, dtype=float)
    z2.assign(z)
    assert np.array_equal(z2.numpy(), (np.arange(4) * 0.1).astype(F32))
    z2.zero_()
    assert not z2.numpy().any()


def test_randn_reads_the_table_and_records_the_states(wp):
    table = np.arange(100, dtype=F32) * F32(0.5)
    wp.randn_table = table

    @wp.kernel
    def k(seed: int, out: wp.array(dtype=float)):
        t = wp.tid()
        out[t] = wp.randn(wp.uint32(seed + t)) + wp.randn(wp.uint32(seed + t + 10))

    out = wp.zeros(4, dtype=float)
    wp.launch(k, dim=4, inputs=[np.int64(20), out])
    assert wp.randn_states == [20, 30, 21, 31, 22, 32, 23, 33]
    assert np.array_equal(out.numpy(), table[20:24] + table[30:34])
    with pytest.raises(IndexError):
        wp.randn(100)


def test_math_tables():
    proj, libm = W.create("project"), W.create("libm")
    xs = np.linspace(-3.0, 3.0, 41).astype(F32)
    for x in xs:
        s, c = dmath.dm_sincosf(x)
        assert proj.sin(x) == s and proj.cos(x) == c and proj.exp(x) == dmath.dm_expf(x)
        assert libm.sin(x) == F32(math.sin(float(x))) and libm.cos(x) == F32(math.cos(float(x)))
        assert libm.exp(x) == F32(math.exp(float(x))) and libm.atan(x) == F32(math.atan(float(x)))
        for wp_ in (proj, libm):
            assert all(type(f(x)) is F32 for f in (wp_.sin, wp_.cos, wp_.exp, wp_.abs))
            assert type(wp_.sqrt(x * x)) is F32 and wp_.sqrt(x * x) == np.sqrt(x * x)
    assert proj.pow(F32(3.7), 1.0) == F32(3.7) and libm.pow(F32(3.7), 1.0) == F32(3.7)
    assert libm.pow(F32(2.0), 0.5) == F32(math.sqrt(2.0))
    with pytest.raises(NotImplementedError):
        proj.pow(F32(2.0), 2.0)
    with pytest.raises(NotImplementedError):
        proj.atan(F32(1.0))
    with pytest.raises(ValueError):
        W.create("cuda")


def test_launch_is_not_reentrant_and_tid_needs_one(wp):
    with pytest.raises(RuntimeError):
        wp.tid()
    with pytest.raises(TypeError):
        wp.launch(lambda: None, dim=1, inputs=[])
