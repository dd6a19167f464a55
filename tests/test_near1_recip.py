"""CPU: the rollout chain's reciprocal for near-unit norms (mppi_detmath.h recip_near1) is the IEEE one.

Compiles tests/native/near1_recip_check.cpp for the host with the library's float flags
(-ffp-contract=off), so the function checked is the one the kernels run, and sweeps
  * every squared norm that gives a divisor b with |bits(b) - bits(1)| <= 1024 (the guard, kNear1 = 2047
    ulps of the squared norm, admits a subset): b == sqrtf(n), y == 1.0f / b;
  * for every such b, every significand a in [1, 2) with both signs, and +-0: the chain's quotient
    (recip_div: q0 = a y, e = fma(b, q0, -a), q = fma(-e, y, q0)) == a / b.  Exponents of a scale exactly.
The four divisors just outside the range are reported, not judged: the guard is what excludes them from
the helper (a lane beyond it redoes its step with the IEEE operators), whatever the helper would give.
"""
import os
import re
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "husky-rover-mppi-isaacsim_amd", "csrc")


def _compiler():
    for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++") or ""):
        if c and os.path.exists(c):
            return c
    return None


def _has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return any(re.match(r"flags\s*:.*\bfma\b", ln) for ln in f)
    except OSError:
        return False


def test_near1_reciprocal_and_quotients_exhaustive(tmp_path):
    cxx = _compiler()
    assert cxx is not None, "no clang++ (the compiler that builds the library)"
    exe = str(tmp_path / "near1_recip_check")
    fma = _has_fma()
    flags = ["-O2", "-std=c++17", "-ffp-contract=off", "-pthread", f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}",
             "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include"] + (["-mfma"] if fma else [])
    cmd = [cxx, *flags, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only",
           os.path.join(HERE, "native", "near1_recip_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # the full sweep is ~20 CPU-seconds with hardware fma (3 s on 8 threads); through libm's fmaf only the
    # divisors within 128 ulps and every 8th beyond
    threads = max(1, min(8, len(os.sched_getaffinity(0))))
    out = subprocess.run([exe, "full" if fma else "quick", str(threads)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-3000:]
    assert "divisors -1024 .. 1024 ulps: 0 sqrt mismatches, 0 reciprocal mismatches" in out.stdout
    assert re.search(r"both signs, \+-0\): 0 quotient mismatches", out.stdout)
    assert "near1 reciprocal: 0 mismatches" in out.stdout
    # the four divisors just outside: excluded by the guard, reported whatever they give
    assert len(re.findall(r"outside: divisor -?\d+ ulps \(norm -?\d+ ulps, guard excludes it\)", out.stdout)) == 4
