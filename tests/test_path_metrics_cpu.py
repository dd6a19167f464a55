"""CPU: the path metrics of executed paths (mppi_amd.batch.path_metrics, dm_atan2).

  * path_metrics against tests/golden/path_metrics.npz: the reference's own compute_path_metrics
    (MPPI_isaac.py:231-256) called on the same float32 waypoints (tests/golden/make_path_metrics_golden.py).
    Tolerance, derived: every term of every sum is non-negative, each is within a few ulp of the
    reference's (one sqrt, one arctangent within a few ulp, one product), and a path of 3500 rows has at
    most 175 terms, so the sums differ by at most a few hundred ulp relative, far inside 1e-13 on the two
    angle sums; length20 and distance_up are the same IEEE operations up to the order inside the norm:
    4 ulp.  Measured: angle sums 4.4e-16 relative, length20 and distance_up 0 ulp.
  * dm_atan2 against numpy.arctan2 on a dense grid with the axes, (0, 0), the diagonal (t = 1) and tiny
    and huge ratios.  Nothing derives an ulp bound for the construction, so the bound is the maximum
    measured on this grid, 6 ulp, plus 1.
  * the online segment state machine and the whole-path form of csrc/mppi_path_metrics.h, walked on the
    host by tests/native/path_metrics_check.cpp for every length 0 .. 70, and the header's dm_atan2
    against this module's on the same points, bit for bit (printed as hex by the program).
"""
import os
import shutil
import subprocess

import numpy as np

from mppi_amd.batch import METRICS_FIELDS, dm_atan2, path_metrics

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "husky-rover-mppi-isaacsim_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden", "path_metrics.npz")
ATAN2_ULP = 6 + 1       # the measured maximum on _grid(), plus 1


def _ulps(got, want):
    want = np.asarray(want, np.float64)
    return np.abs(np.asarray(got, np.float64) - want) / np.spacing(np.maximum(np.abs(want), np.finfo(np.float64).tiny))


def test_path_metrics_match_the_reference_fixture():
    d = np.load(GOLDEN)
    n = int(d["cases"])
    lengths = sorted(len(d[f"path_{k}"]) for k in range(n))
    for L in (0, 1, 21, 22, 23, 41, 42, 43, 61, 62, 3500):
        assert L in lengths
    worst_rel, worst_ulp = 0.0, 0.0
    both = 0
    for k in range(n):
        p, want = d[f"path_{k}"], d[f"metrics_{k}"]
        assert p.dtype == np.float32 and want.dtype == np.float64
        got = path_metrics(p)
        assert got.shape == (4,) and got.dtype == np.float64
        if len(p) < 22:
            assert not got.any() and not want.any()
        for j in (1, 2):    # the angle sums
            rel = abs(got[j] - want[j]) / max(abs(want[j]), 1e-300)
            worst_rel = max(worst_rel, rel)
            assert rel <= 1e-13, (str(d["names"][k]), METRICS_FIELDS[j], got[j], want[j])
        for j in (0, 3):    # length20, distance_up
            u = float(_ulps(got[j], want[j]))
            worst_ulp = max(worst_ulp, u)
            assert u <= 4, (str(d["names"][k]), METRICS_FIELDS[j], got[j], want[j])
        both += want[1] > 0 and want[2] > 0
    print("angle sums: max relative difference", worst_rel, "; length20 / distance_up: max ulp", worst_ulp)
    assert both >= 3        # paths that climb and descend within one run
    names = [str(s) for s in d["names"]]
    z = d[f"path_{names.index('zero_segment')}"]
    assert np.array_equal(z[0], z[21])                          # a zero-length segment
    lv = d[f"path_{names.index('level_segment')}"]
    assert lv[0, 2] == lv[21, 2] and not np.array_equal(lv[0], lv[21])     # a level one


def test_path_metrics_takes_log_rows():
    """[L, 8] log rows give what their first three columns give; fewer than 22 rows give zeros."""
    rng = np.random.RandomState(3)
    rows = rng.normal(size=(50, 8)).astype(np.float32)
    assert np.array_equal(path_metrics(rows), path_metrics(rows[:, :3]))
    assert path_metrics(rows)[0] > 0
    assert not path_metrics(rows[:21]).any()
    assert not path_metrics(np.zeros((0, 8), np.float32)).any()


def _grid():
    pos = np.concatenate([np.logspace(-300, 300, 301), np.linspace(0, 1, 501)[1:], np.linspace(1, 50, 197),
                          [1e-310, 5e-324, 1.7e308]])
    return np.unique(np.concatenate([[0.0], pos, -pos]))


def test_dm_atan2_against_numpy():
    v = _grid()
    y, x = np.meshgrid(v, v)
    got, want = dm_atan2(y, x), np.arctan2(y, x)
    assert got.dtype == np.float64
    zero = want == 0
    assert np.all(got[zero] == 0)
    u = _ulps(got[~zero], want[~zero])
    i = int(np.argmax(u))
    print("dm_atan2:", y.size, "points, max", u.max(), "ulp at y, x =", y[~zero][i], x[~zero][i])
    assert u.max() <= ATAN2_ULP
    # the axes, the origin and the diagonal
    assert dm_atan2(0.0, 0.0) == 0.0 and dm_atan2(0.0, 1.0) == 0.0
    assert dm_atan2(0.0, -1.0) == np.pi and dm_atan2(1.0, 0.0) == np.pi / 2 and dm_atan2(-1.0, 0.0) == -np.pi / 2
    assert abs(dm_atan2(1.0, 1.0) - np.pi / 4) <= ATAN2_ULP * np.spacing(np.pi / 4)
    assert dm_atan2(-3.0, 2.0) == -dm_atan2(3.0, 2.0)
    assert isinstance(dm_atan2(1.0, 2.0), np.float64)


def _compiler():
    for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++") or ""):
        if c and os.path.exists(c):
            return c
    return None


def test_online_state_machine_and_header_arctangent(tmp_path):
    """tests/native/path_metrics_check.cpp, built for the host with the library's float flags and the host
    sanitizers: the online form fed one row at a time equals the whole-path form for every length 0 .. 70,
    and the header's dm_atan2 and path_metrics_rows give the bits of this module's on the points and the
    path the program prints."""
    cxx = _compiler()
    assert cxx is not None, "no clang++ (the compiler that builds the library)"
    exe = str(tmp_path / "path_metrics_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", f"-I{CSRC}", os.path.join(HERE, "native", "path_metrics_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert "path metrics ok" in out.stdout
    pts, path, metrics = [], [], None
    for ln in out.stdout.splitlines():
        w = ln.split()
        if w and w[0] == "atan2":
            pts.append([float.fromhex(t) for t in w[1:4]])
        elif w and w[0] == "row":
            path.append([float.fromhex(t) for t in w[1:4]])
        elif w and w[0] == "metrics":
            metrics = np.array([float.fromhex(t) for t in w[1:5]])
    pts = np.array(pts)
    assert len(pts) >= 1000
    mine = dm_atan2(pts[:, 0], pts[:, 1])
    assert np.array_equal(mine.view(np.uint64), pts[:, 2].copy().view(np.uint64)), \
        int((mine != pts[:, 2]).sum())
    path = np.array(path, np.float32)
    assert len(path) == 70 and metrics is not None
    assert np.array_equal(path_metrics(path).view(np.uint64), metrics.view(np.uint64)), (path_metrics(path), metrics)
