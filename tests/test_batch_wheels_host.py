"""CPU: the host bookkeeping of the wheel log, the wheel slope mode and the path metrics (mppi_amd._lib.Batch,
mppi_amd.batch), on a stub library that records the calls: nothing here needs a GPU.

  * a Batch that is not asked for any of the options calls none of the new entry points: the library is
    told about the score options only when they change, so existing callers launch what they launched;
  * scored=dict(slope=, metrics=) and set_tracking(slope=, metrics=) reach mppi_batch_set_score_options
    before the list or tracking is set, an unfinished list or standing tracking is ended first (the
    library refuses the options under either), and the refusals the library gives come back as errors;
  * score / score_tasks pick the _ex siblings only for the wheel form or the metrics;
  * task_scores() and runs() fetch the metrics rows only when the list or tracking was set with them;
  * campaign_summary / campaign_results / tracked_results carry the four metrics when they are present.
"""
import ctypes

import numpy as np
import pytest

E, H = 2, 20


class _Lib:
    """Records (name, scalar arguments); every call succeeds unless its name is in `refuse`."""

    def __init__(self, refuse=()):
        self.calls = []
        self.refuse = set(refuse)

    def mppi_last_error(self):
        return b"refused: a campaign is unfinished"

    def __getattr__(self, name):
        if not name.startswith("mppi_"):
            raise AttributeError(name)

        def call(*a):
            self.calls.append((name,) + tuple(x for x in a[1:] if isinstance(x, (int, float))))
            return -3 if name in self.refuse else 0
        return call

    def names(self):
        return [c[0] for c in self.calls]


def _batch(lib=None):
    from mppi_amd import _lib
    b = _lib.Batch.__new__(_lib.Batch)
    b.E, b.H, b.lib, b.h = E, H, lib or _Lib(), ctypes.c_void_p()
    b.engine = type("Eng", (), dict(device=0, ctx=None))()
    return b


def _task():
    from mppi_amd import _lib
    return _lib.make_task(_lib.make_state(0.0, 0.0, goal_x=5.0, goal_y=5.0), 1, 10)


NEW = {"mppi_batch_set_wheel_log", "mppi_batch_get_wheel_log", "mppi_batch_get_task_wheel_log", "mppi_batch_score_ex",
       "mppi_batch_score_tasks_ex", "mppi_batch_set_score_options", "mppi_batch_get_task_metrics",
       "mppi_batch_get_run_metrics"}


def test_new_entry_points_are_declared():
    from mppi_amd import _lib
    assert NEW <= set(_lib._PROTOS)


def test_defaults_call_no_new_entry_point():
    b = _batch()
    b.set_tasks([_task()])
    b.set_tasks([_task()], scored=True, keep_log=False)
    b.set_tasks([_task()], scored=dict(w_path=2.0))          # a yardstick dict, as before
    b.task_scores()
    b.score()
    b.score_tasks()
    b.set_tracking(max_steps=5)
    b.set_tracking(dict(w_path=2.0), max_steps=7)
    b.runs(0)
    b.clear_tracking()
    assert not NEW & set(b.lib.names()), b.lib.names()
    assert "metrics" not in b.task_scores() and b.lib.names().count("mppi_batch_set_tasks_scored") == 2


def test_scored_options_reach_the_library_before_the_list():
    b = _batch()
    b.set_tasks([_task()], scored=dict(slope="wheels", metrics=True), keep_log=False)
    names = b.lib.names()
    # the standing list is cleared first (the library refuses new options while a campaign is unfinished)
    assert names == ["mppi_batch_set_tasks", "mppi_batch_set_score_options", "mppi_batch_set_tasks_scored"]
    assert b.lib.calls[0] == ("mppi_batch_set_tasks", 0)
    assert b.lib.calls[1] == ("mppi_batch_set_score_options", 0, 1)      # MPPI_SLOPE_WHEELS = 0, metrics on
    out = b.task_scores()
    assert out["metrics"].shape == (1, 4) and out["metrics"].dtype == np.float64
    assert b.lib.names()[-1] == "mppi_batch_get_task_metrics"
    # the same options again: the library is not told twice
    b.set_tasks([_task()], scored=dict(slope="wheels", metrics=True, yardstick=dict(w_path=2.0)))
    assert b.lib.names().count("mppi_batch_set_score_options") == 1
    # back to the defaults: told once more, and the scores have no metrics
    b.set_tasks([_task()], scored=True)
    assert b.lib.calls[-2] == ("mppi_batch_set_score_options", 1, 0)     # MPPI_SLOPE_BODY = 1
    assert "metrics" not in b.task_scores()
    with pytest.raises(ValueError, match="slope must be one of"):
        b.set_tasks([_task()], scored=dict(slope="wheel"))
    # a plain list takes no score options
    n = len(b.lib.calls)
    b.set_tasks([_task()])
    assert [c[0] for c in b.lib.calls[n:]] == ["mppi_batch_set_tasks"]


def test_set_tasks_keywords_and_the_one_argument_form():
    b = _batch()
    b.set_tasks([_task()], scored=dict(w_path=2.0), slope="wheels", metrics=True, keep_log=False)
    assert b.lib.names() == ["mppi_batch_set_tasks", "mppi_batch_set_score_options", "mppi_batch_set_tasks_scored"]
    assert b.lib.calls[1] == ("mppi_batch_set_score_options", 0, 1) and b.list_metrics
    n = len(b.lib.calls)
    b.set_tasks([_task()], scored=True, slope="wheels", metrics=True)           # the same options: not told again
    assert [c[0] for c in b.lib.calls[n:]] == ["mppi_batch_set_tasks_scored"]
    n = len(b.lib.calls)
    with pytest.raises(ValueError, match="belong to a scored list"):
        b.set_tasks([_task()], slope="wheels")
    with pytest.raises(ValueError, match="belong to a scored list"):
        b.set_tasks([_task()], scored=False, metrics=True)
    with pytest.raises(ValueError, match="takes no other key"):
        b.set_tasks([_task()], scored=dict(slope="wheels", w_path=2.0))           # no mix with a yardstick's fields
    with pytest.raises(ValueError, match="not both"):
        b.set_tasks([_task()], scored=dict(slope="wheels"), metrics=True)
    with pytest.raises(ValueError, match="slope must be one of"):
        b.set_tasks([_task()], scored=True, slope="wheel")
    assert len(b.lib.calls) == n                                                  # refused before any library call


def test_tracking_options_and_their_refusal():
    b = _batch()
    b.set_tracking(max_steps=9, slope="wheels", metrics=True)
    assert b.lib.names() == ["mppi_batch_set_score_options", "mppi_batch_set_tracking"]
    assert b.tracking == dict(max_steps=9, runs_per_episode=1, keep_log=True, slope="wheels", metrics=True)
    r = b.runs(0)
    assert r["metrics"].shape == (1, 4) and b.lib.names()[-1] == "mppi_batch_get_run_metrics"
    assert b.runs()["metrics"].shape == (E, 4)
    # other options under tracking: tracking is cleared first, then set again
    n = len(b.lib.calls)
    b.set_tracking(max_steps=9)
    assert [c[0] for c in b.lib.calls[n:]] == ["mppi_batch_set_tracking", "mppi_batch_set_score_options",
                                               "mppi_batch_set_tracking"]
    assert b.lib.calls[n][1:] == (0.0, 0, 0, 0)
    assert "metrics" not in b.runs(0)
    with pytest.raises(ValueError, match="slope must be one of"):
        b.set_tracking(max_steps=9, slope="both")
    # what the library refuses (an unfinished campaign, say) is an error, and the options stay as they were
    b = _batch(_Lib(refuse={"mppi_batch_set_score_options", "mppi_batch_set_wheel_log"}))
    with pytest.raises(RuntimeError, match="campaign is unfinished"):
        b.set_tracking(max_steps=9, metrics=True)
    assert not getattr(b, "tracking", None) and getattr(b, "_opts", ("body", False)) == ("body", False)
    with pytest.raises(RuntimeError, match="campaign is unfinished"):
        b.set_wheel_log()


def test_score_siblings_are_picked_by_the_options():
    b = _batch()
    b.n_tasks = 3
    assert set(b.score()) == {"cost", "terms", "collisions", "rows"}
    assert b.score(slope="wheels")["cost"].shape == (E,)
    assert b.score(metrics=True)["metrics"].shape == (E, 4)
    assert b.score_tasks(slope="wheels", metrics=True)["metrics"].shape == (3, 4)
    b.score_tasks()
    assert b.lib.names() == ["mppi_batch_score", "mppi_batch_score_ex", "mppi_batch_score_ex",
                             "mppi_batch_score_tasks_ex", "mppi_batch_score_tasks"]
    assert b.lib.calls[1] == ("mppi_batch_score_ex", 0) and b.lib.calls[2] == ("mppi_batch_score_ex", 1)
    with pytest.raises(ValueError, match="slope must be one of"):
        b.score(slope="wheel")
    with pytest.raises(ValueError, match="slope must be one of"):
        b.score_tasks(slope=0)


def test_campaign_summary_adds_the_metrics_when_present():
    from mppi_amd.batch import METRICS_FIELDS, SUMMARY_FIELDS, campaign_results, campaign_summary, tracked_results
    tasks = [dict(reached=True, loops=30), dict(reached=False, loops=45), dict(reached=True, loops=25)]
    scores = dict(cost=np.array([1.0, 3.0, 5.0], np.float32), terms=np.arange(12, dtype=np.float32).reshape(3, 4),
                  collisions=np.array([0, 2, 0], np.int32), length=np.array([1.0, 2.0, 4.0]))
    plain = campaign_summary(campaign_results(tasks, scores), by=["a", "b", "a"])
    assert set(plain["a"]["mean"]) == set(SUMMARY_FIELDS)
    scores["metrics"] = np.array([[2.0, 10.0, 0.0, 0.5], [3.0, 0.0, 7.0, 0.0], [4.0, 30.0, 2.0, 1.5]])
    res = campaign_results(tasks, scores)
    assert np.array_equal(res[2]["metrics"], scores["metrics"][2])
    out = campaign_summary(res, by=["a", "b", "a"])
    assert set(out["a"]["mean"]) == set(SUMMARY_FIELDS) | set(METRICS_FIELDS) == set(out["a"]["std"])
    assert out["a"]["mean"]["length20"] == 3.0 and out["a"]["mean"]["angle_up"] == 20.0
    assert out["a"]["mean"]["angle_down"] == 1.0 and out["a"]["mean"]["distance_up"] == 1.0
    assert out["a"]["std"]["angle_up"] == 10.0 and out["b"]["mean"]["angle_down"] == 7.0
    for f in SUMMARY_FIELDS:
        assert out["a"]["mean"][f] == plain["a"]["mean"][f]
    # one result without metrics in a group: that group has no metrics columns
    res[0] = {k: v for k, v in res[0].items() if k != "metrics"}
    mixed = campaign_summary(res, by=["a", "b", "a"])
    assert set(mixed["a"]["mean"]) == set(SUMMARY_FIELDS) and "angle_up" in mixed["b"]["mean"]
    # the stacked rows of tracked runs
    runs = dict(episode=np.array([0, 0, 1]), run=np.array([0, 1, 0]), status=np.array([1, 0, 2]),
                reached=np.array([1, 0, 0]), steps=np.array([30, 0, 45]), cost=scores["cost"], terms=scores["terms"],
                collisions=scores["collisions"], length=scores["length"], metrics=scores["metrics"])
    rows, keys = tracked_results(runs, by=["x", "y"])
    assert [r["episode"] for r in rows] == [0, 1] and keys == ["x", "y"]
    assert np.array_equal(rows[1]["metrics"], scores["metrics"][2])
    assert campaign_summary(runs, by=["x", "y"])["y"]["mean"]["length20"] == 4.0
    del runs["metrics"]
    assert "metrics" not in tracked_results(runs)[0][0]
