"""CPU: the host side of a scored task list: the Python-side argument checks of
Batch.set_tasks / task_scores and MPPI_Controller.run_campaign, mppi_amd.batch.campaign_summary on
hand-made results, and path_length (the numpy restatement of `length`) on short paths.  No GPU and no
library call.
"""
import numpy as np
import pytest

from mppi_amd import _lib, batch


# ---- argument checks ----
class _NoLib:
    """Stands where the library would be called: the checks below must refuse before any call."""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def _fake_batch(n_tasks):
    b = object.__new__(_lib.Batch)
    b.lib, b.h, b.n_tasks = _NoLib(), None, n_tasks
    return b


def test_keep_log_false_needs_a_scored_list():
    b = _fake_batch(0)
    st = _lib.make_state(0.0, 0.0, (1.0, 0.0, 0.0), 0.0, 0.0, 5.0, 5.0)
    for scored in (None, False):
        with pytest.raises(ValueError, match="keep_log=False needs a scored list"):
            b.set_tasks([_lib.make_task(st, 1, 3)], scored=scored, keep_log=False)
    with pytest.raises(ValueError, match="not fields of mppi_batch_variant"):
        b.set_tasks([_lib.make_task(st, 1, 3)], scored=dict(w_bogus=1.0))


@pytest.mark.parametrize("first, count", [(-1, 1), (0, 5), (3, 2), (5, 0), (0, -1)])
def test_task_scores_range(first, count):
    with pytest.raises(ValueError, match="outside the list of 4 tasks"):
        _fake_batch(4).task_scores(first, count)


def test_prototypes():
    import ctypes as C
    res, args = _lib._PROTOS["mppi_batch_set_tasks_scored"]
    assert res is C.c_int and len(args) == 5 and args[4] is C.c_int32
    res, args = _lib._PROTOS["mppi_batch_get_task_scores"]
    assert res is C.c_int and len(args) == 6 and args[5] is _lib._DP


def test_run_campaign_log_false_needs_score():
    from mppi_amd import controller
    ctl = object.__new__(controller.MPPI_Controller)
    for score in (None, False):
        with pytest.raises(ValueError, match="log=False needs score"):
            ctl.run_campaign([(0.0, 0.0)], [(1.0, 0.0, 0.0)], [(5.0, 5.0)], score=score, log=False)


# ---- campaign_summary ----
def _result(reached, cost, terms, collisions, length):
    return dict(reached=reached, cost=np.float32(cost), terms=np.asarray(terms, np.float32),
                collisions=np.int32(collisions), length=np.float64(length), loops=3)


def test_campaign_summary():
    rs = [_result(True, 10.0, (1, 2, 3, 4), 0, 2.0), _result(False, 30.0, (3, 2, 5, 8), 2, 6.0),
          _result(True, 7.0, (0.5, 0.25, 0, 1), 0, 1.5), _result(True, 20.0, (2, 2, 4, 0), 1, 4.0)]
    t = batch.campaign_summary(rs, by=[0, 0, 1, 0])
    assert list(t) == [0, 1]
    a = t[0]
    assert (a["count"], a["reached"], a["collided"]) == (3, 2, 2)
    assert a["mean"] == dict(cost=20.0, path=2.0, slope=2.0, speed=4.0, obstacle=4.0, length=4.0)
    # the population's standard deviation: of (10, 30, 20) it is sqrt(200 / 3)
    assert a["std"]["cost"] == pytest.approx(np.sqrt(200.0 / 3.0), rel=1e-15)
    assert a["std"]["slope"] == 0.0 and a["std"]["length"] == pytest.approx(np.sqrt(8.0 / 3.0), rel=1e-15)
    b = t[1]
    assert (b["count"], b["reached"], b["collided"]) == (1, 1, 0)
    assert b["mean"] == dict(cost=7.0, path=0.5, slope=0.25, speed=0.0, obstacle=1.0, length=1.5)
    assert all(v == 0.0 for v in b["std"].values())
    # one group without keys, string keys in order of first appearance
    one = batch.campaign_summary(rs)
    assert list(one) == [None] and one[None]["count"] == 4 and one[None]["mean"]["cost"] == 16.75
    assert list(batch.campaign_summary(rs, by=["b", "a", "b", "a"])) == ["b", "a"]
    assert batch.campaign_summary([]) == {}
    with pytest.raises(ValueError, match="4 results but 3 group keys"):
        batch.campaign_summary(rs, by=[0, 1, 2])


def test_campaign_results():
    tasks = [dict(loops=2, reached=False), dict(loops=0, reached=True)]
    scores = dict(cost=np.array([5.0, 0.0], np.float32), terms=np.array([[1, 2, 3, 4], [0, 0, 0, 0]], np.float32),
                  collisions=np.array([1, 0], np.int32), rows=np.array([2, 0], np.int32),
                  length=np.array([0.0, 0.0]))
    rs = batch.campaign_results(tasks, scores)
    assert rs[0]["cost"] == 5.0 and rs[0]["loops"] == 2 and list(rs[0]["terms"]) == [1, 2, 3, 4]
    t = batch.campaign_summary(rs)[None]
    assert (t["count"], t["reached"], t["collided"]) == (2, 1, 1) and t["mean"]["cost"] == 2.5


# ---- path_length ----
def _rows(n):
    """n waypoints whose float32 coordinates have no short float64 differences."""
    rng = np.random.default_rng(11)
    rows = np.zeros((n, 8), np.float32)
    rows[:, :3] = np.cumsum(rng.normal(0.0, 0.37, (n, 3)), 0).astype(np.float32)
    return rows


def _length_by_hand(rows):
    """The issue's statement, index by index."""
    total = np.float64(0.0)
    sampled = list(range(0, len(rows), 5))
    for a, b in zip(sampled[:-1], sampled[1:]):
        dx = np.float64(rows[b, 0]) - np.float64(rows[a, 0])
        dy = np.float64(rows[b, 1]) - np.float64(rows[a, 1])
        dz = np.float64(rows[b, 2]) - np.float64(rows[a, 2])
        total = total + np.sqrt((dx * dx + dy * dy) + dz * dz)
    return total


@pytest.mark.parametrize("n, segments", [(0, 0), (1, 0), (5, 0), (6, 1), (11, 2)])
def test_path_length(n, segments):
    rows = _rows(n)
    got = batch.path_length(rows)
    assert isinstance(got, np.float64)
    assert got.view(np.uint64) == _length_by_hand(rows).view(np.uint64)
    assert (got > 0) == (segments > 0)
    if segments == 0:
        assert got == 0.0


def test_path_length_values():
    rows = np.zeros((11, 3), np.float32)
    rows[5] = (3.0, 4.0, 12.0)          # 13 from the origin
    rows[10] = (3.0, 4.0, 10.0)         # 2 further
    rows[[1, 2, 3, 4, 6, 7, 8, 9]] = 99.0       # the rows in between are not read
    assert batch.path_length(rows) == 15.0
    assert batch.path_length(rows[:10]) == 13.0
    assert batch.path_length(rows[:5]) == 0.0
    # the differences are taken in float64 of the float32 coordinates, not in float32
    a = np.array([[0.1, 0.0, 0.0]] + [[0.0] * 3] * 4 + [[16777216.0, 0.0, 0.0]], np.float32)
    assert batch.path_length(a) == np.float64(np.float32(16777216.0)) - np.float64(np.float32(0.1))
