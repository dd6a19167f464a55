"""CPU: sampling plans (include/mppi.h mppi_sampling) without a GPU.

  native   tests/native/sampling_plan_check.cpp runs the device functions of mppi_detmath.h
           (plan_source, plan_ar1, plan_apply) on the host with the library's float flags, and its
           sequences equal mppi_amd.sampling.apply_plan on the oracle's base normals, bit for bit
  mirror   the numpy statement itself: unit variance and lag-1 correlation beta of the AR(1) form,
           exact pair sums, the all +0 nominal row
  parsing  variant dicts, the YAML section, the refusals that need no context
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from mppi_amd import batch as MB
from mppi_amd import sampling as S
from oracle import dmath

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "husky-rover-mppi-isaacsim_amd", "csrc")
F32 = np.float32


def _compiler():
    for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++") or ""):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no clang++")
    exe = str(tmp_path_factory.mktemp("native") / "sampling_plan_check")
    flags = ["-O2", "-std=c++17", "-ffp-contract=off", f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}",
             "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include"]
    cmd = [cxx, *flags, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only",
           os.path.join(HERE, "native", "sampling_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("beta", [0.0, 0.5, 0.96875])
@pytest.mark.parametrize("H", [5, 20])
def test_native_plan_equals_numpy_statement(plan_check, H, beta):
    rng = np.random.default_rng(1000 * H + int(beta * 64))
    ks = np.array([0, 1, 2, 3, 255, 256, 257, 299, 1023, (1 << 33) + 1, (1 << 33) + 2] +
                  rng.integers(0, 1 << 40, 40).tolist(), np.int64)
    for anti in (0, 1):
        for nominal in (0, 1):
            seed, step = int(rng.integers(0, 1 << 62)), int(rng.integers(0, 1 << 20))     # random blocks
            plan = dict(antithetic=bool(anti), nominal=bool(nominal), beta=beta)
            out = subprocess.run([plan_check, str(seed), str(step), str(H), repr(beta), str(anti), str(nominal),
                                  *[str(int(k)) for k in ks]], capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, out.stderr[-2000:]
            got = np.array([[int(w, 16) for w in line.split()[1:]] for line in out.stdout.splitlines()], np.uint32)
            assert got.shape == (ks.size, 2 * H)
            src, sign, zero = S.plan_sources(ks, plan)
            z1, z2 = dmath.noise(seed, step, src, H)
            e1, e2 = S.apply_plan(z1, z2, ks, plan)
            want = np.concatenate([e1, e2], axis=1).view(np.uint32)
            assert np.array_equal(got, want), (plan, np.argwhere(got != want)[:5])
            if nominal:
                assert not got[0].any()                                  # k = 0: +0.0 everywhere
            if anti:
                assert np.array_equal(src[:4], [0, 0, 2, 2]) and np.array_equal(sign[:4], [1, -1, 1, -1])


def test_plan_sources():
    k = np.arange(6)
    src, sign, zero = S.plan_sources(k, dict(antithetic=True, nominal=True, beta=0.0))
    assert src.tolist() == [0, 0, 2, 2, 4, 4]
    assert sign.tolist() == [1, -1, 1, -1, 1, -1] and sign.dtype == F32
    assert zero.tolist() == [True, False, False, False, False, False]
    src, sign, zero = S.plan_sources(k + 256, dict(antithetic=False, nominal=True, beta=0.3))
    assert src.tolist() == (k + 256).tolist() and (sign == 1).all() and not zero.any()


def test_mirror_statistics_and_exact_pairs():
    """beta = 0.7 over 2e5 draws: variance within 3 % of 1, lag-1 correlation within 0.02 of beta (the
    stationary AR(1) from e[0] = z[0] has both exactly; the sampling error of either at n = 2e5 is
    below 0.5 %)."""
    n, H = 10000, 21                      # 2e5 lag-1 pairs, 2.1e5 draws
    k = np.arange(n, dtype=np.int64)
    plan = dict(antithetic=False, nominal=False, beta=0.7)
    z1, z2 = dmath.noise(3, 5, k, H)
    e1, e2 = S.apply_plan(z1, z2, k, plan)
    for e in (e1, e2):
        e = e.astype(np.float64)
        var = e.var()
        rho = np.mean(e[:, 1:] * e[:, :-1]) / var
        print(f"variance {var:.5f} lag-1 correlation {rho:.5f}")
        assert abs(var - 1.0) <= 0.03
        assert abs(rho - 0.7) <= 0.02
    both = dict(antithetic=True, nominal=True, beta=0.7)
    src, _, _ = S.plan_sources(k, both)
    z1, z2 = dmath.noise(3, 5, src, H)
    a1, a2 = S.apply_plan(z1, z2, k, both)
    for a in (a1, a2):
        assert a.dtype == F32
        assert not a[0].view(np.uint32).any()                            # the nominal row: all +0.0
        s = a[2::2] + a[3::2]
        assert not s.view(np.uint32).any()                               # a pair sums to exactly +0
        # k = 1 reflects k = 0's un-zeroed (correlated) draw
        assert np.array_equal(a[1].view(np.uint32), (-S.correlate(z1 if a is a1 else z2, 0.7)[0]).view(np.uint32))
    # beta = 0 changes no bit of the base normals
    d1, d2 = S.apply_plan(z1, z2, k, dict(antithetic=False, nominal=False, beta=0.0))
    assert np.array_equal(d1.view(np.uint32), z1.view(np.uint32))


def test_variant_dicts_with_and_without_the_keys():
    base = MB.variant_dict("3d")
    v, plan = MB.split_sampling(base)
    assert plan is None and v == base
    v, plan = MB.split_sampling(dict(base, antithetic=True))
    assert plan == dict(antithetic=True, nominal=False, beta=0.0) and v == base
    v, plan = MB.split_sampling(dict(base, nominal=1, noise_beta=0.7, slope="body"))
    assert plan == dict(antithetic=False, nominal=True, beta=float(F32(0.7)))
    assert v == dict(base, slope="body")                                # the critic keys are the next split's
    v2, crit = MB.split_variant(v)
    assert crit["slope"] == "body" and v2 == base
    MB.variant_params({}, v2)                                            # and what is left is a full variant
    for bad in (1.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="beta"):
            MB.split_sampling(dict(base, noise_beta=bad))
    with pytest.raises(ValueError, match="antithetic"):
        MB.split_sampling(dict(base, antithetic=2))
    with pytest.raises(ValueError, match="nominal"):
        MB.split_sampling(dict(base, nominal=-1))


def test_make_sampling_refusals():
    from mppi_amd import _lib
    k = _lib.make_sampling(True, False, 0.5)
    assert (k.antithetic, k.nominal, k.beta) == (1, 0, 0.5)
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="beta"):
            _lib.make_sampling(beta=bad)
    with pytest.raises(ValueError, match="antithetic"):
        _lib.make_sampling(antithetic=3)
    # the k_offset rule at the Python layer, where the caller knows it
    with pytest.raises(ValueError, match="antithetic.*k_offset"):
        S.make_plan(antithetic=True, k_offset=1)
    with pytest.raises(ValueError, match="antithetic.*k_offset"):
        _lib.make_sampling(antithetic=True, k_offset=257)          # what Engine.set_sampling calls
    assert S.make_plan(antithetic=True, k_offset=256)["antithetic"] is True
    assert S.make_plan(antithetic=False, k_offset=1)["antithetic"] is False


def test_yaml_section(tmp_path):
    import yaml
    from mppi_amd import controller as MC
    surface = MC.Surface.from_arrays(np.zeros((32, 32), F32), np.zeros((4, 4), F32), 1.6)
    robot = MC.Robot(0.0, 0.0, [1.0, 0.0, 0.0], MC.DEFAULT_CONFIG)

    def make(text):
        with open(MC.DEFAULT_CONFIG) as f:
            cfg = yaml.safe_load(f)
        cfg["engine"].update(yaml.safe_load(text) or {})
        return MC.MPPI_Controller(surface, robot, cfg, 5.0, 1.0, 0.0)

    assert make("").sampling == S.DEFAULT_PLAN
    got = make("sampling: {antithetic: true, beta: 0.7}").sampling
    assert got == dict(antithetic=True, nominal=False, beta=float(F32(0.7)))
    assert make("sampling: {nominal: true}").sampling == dict(antithetic=False, nominal=True, beta=0.0)
    for bad in ("1.0", "-0.1", ".nan"):
        with pytest.raises(ValueError, match="beta"):
            make(f"sampling: {{beta: {bad}}}")
    ctl = make("")
    ctl.set_sampling(nominal=True, beta=0.5)               # (no engine yet: kept for warp_setup)
    assert ctl.sampling == dict(antithetic=False, nominal=True, beta=0.5)
    with pytest.raises(ValueError, match="beta"):
        ctl.set_sampling(beta=1.0)
