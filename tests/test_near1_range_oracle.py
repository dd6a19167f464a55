"""CPU: the three re-normalisations of unit vectors in the rollout see norms within a few ulps of 1.

The chain replaces the reciprocal of those norms by a closed form that is exact within 1024 ulps of 1
(mppi_detmath.h recip_near1, guarded at 2047 ulps of the squared norm; a lane beyond redoes its step
with the IEEE operators, so no result depends on the bound).  This test measures the norms where the
numpy restatement takes them, by wrapping oracle.mppi_ref.update_orientation / update_position (their
dot3(h, h) and dot3(r, r) are the squared norms of the three sites):
  tangent     update_orientation, the second normalisation of the tangent
  rotated     update_orientation, the Rodrigues rotation's result
  heading     update_position, the heading before the position update
on the C3 scene at K = 2048, H = 100 from two poses.  Every norm must lie within 64 ulps of 1 (measured:
3), a sixteenth of the range the closed form is verified for, so the guard does not fire on this terrain.
"""
import numpy as np

import helpers as hp
from oracle import mppi_ref as R

ONE = 0x3F800000
CAP = 64


def _ulps_from_one(b):
    return np.abs(np.asarray(b, np.float32).view(np.int32).astype(np.int64) - ONE)


def test_unit_vector_norms_stay_within_64_ulps_of_one(monkeypatch):
    Z, hw, cm = hp.c3_scene()
    sc = hp.oracle_scene(Z, hw, cm)
    site = []  # the wrapped function being run, innermost last
    seen = {"tangent": [], "rotated": [], "heading": []}
    count = {"update_orientation": 0, "update_position": 0}
    dot3, upd_o, upd_p = R.dot3, R.update_orientation, R.update_position

    def dot3_rec(a, b):
        n = dot3(a, b)
        if site and a is b:  # a squared norm inside one of the wrapped functions
            if site[-1] == "update_position":
                seen["heading"].append(n)
            else:  # update_orientation: dot3(h, h) first, then dot3(r, r)
                count["norms_in_call"] += 1
                seen["tangent" if count["norms_in_call"] == 1 else "rotated"].append(n)
        return n

    def wrap(fn, name):
        def inner(*a, **k):
            site.append(name)
            count[name] += 1
            count["norms_in_call"] = 0
            try:
                return fn(*a, **k)
            finally:
                site.pop()
        return inner

    monkeypatch.setattr(R, "dot3", dot3_rec)
    monkeypatch.setattr(R, "update_orientation", wrap(upd_o, "update_orientation"))
    monkeypatch.setattr(R, "update_position", wrap(upd_p, "update_position"))
    K, H = 2048, 100
    for x, y, heading in ((hp.START[0], hp.START[1], (1.0, 0.0, 0.0)), (10.0, 20.0, (0.6, -0.8, 0.0))):
        st = hp.oracle_state(x=x, y=y, heading=heading)
        R.mppi_step(R.Params(K=K, H=H), sc, st, np.zeros(H, np.float32), np.zeros(H, np.float32), 0)
    assert count["update_orientation"] > 0 and count["update_position"] > 0
    for name, sq in seen.items():
        assert sq, f"no norm recorded at site {name}"
        n2 = np.concatenate([np.ravel(np.asarray(v, np.float32)) for v in sq])
        assert n2.size >= 2 * K * H, f"{name}: {n2.size} norms"
        d = _ulps_from_one(np.sqrt(n2))
        d2 = _ulps_from_one(n2)
        print(f"{name}: {n2.size} norms, max |ulps from 1| {int(d.max())} (squared norm {int(d2.max())}), "
              f"{100.0 * np.mean(d == 0):.1f} % exactly 1")
        assert int(d.max()) <= CAP, f"{name}: a norm {int(d.max())} ulps from 1"
