"""CPU: the host side of a batch's task queue (mppi_amd.batch campaign_tasks / campaign_makespan).

No GPU and no library: argument checking of MPPI_Controller.run_campaign's per-task arguments, and
the claim rule's step count against a lane-by-lane simulation.
"""
import numpy as np
import pytest

from mppi_amd.batch import campaign_makespan, campaign_tasks


def _simulate(lengths, lanes):
    """Every lane explicitly, one batch step at a time: a lane whose task ends takes the next task
    of the list, skipping tasks of length 0, in the same step."""
    todo = list(lengths)
    left = [0] * lanes

    def claim(lane):
        left[lane] = 0
        while todo:
            n = todo.pop(0)
            if n > 0:
                left[lane] = n
                return

    for lane in range(lanes):
        claim(lane)
    steps = 0
    while any(left):
        steps += 1
        for lane in range(lanes):
            if left[lane]:
                left[lane] -= 1
                if left[lane] == 0:
                    claim(lane)
    return steps


def test_makespan_of_the_issue():
    assert campaign_makespan([3, 9, 2, 2, 4], 2) == 11
    assert campaign_makespan([0, 3, 0, 0, 2, 0], 2) == 3
    assert campaign_makespan([], 4) == 0
    assert campaign_makespan([0, 0, 0], 1) == 0
    assert campaign_makespan([5], 64) == 5                 # lanes > tasks
    assert campaign_makespan([1, 2, 3], 1) == 6
    assert campaign_makespan(np.array([4, 4, 4, 4]), 4) == 4


def test_makespan_against_a_simulation():
    rng = np.random.RandomState(3)
    for _ in range(400):
        n = rng.randint(0, 14)
        lengths = [0 if rng.rand() < 0.3 else int(rng.randint(1, 10)) for _ in range(n)]
        lanes = int(rng.randint(1, 8))                     # often more lanes than tasks
        assert campaign_makespan(lengths, lanes) == _simulate(lengths, lanes), (lengths, lanes)


def test_makespan_bounds():
    """Greedy list scheduling: at least the longest task and the mean load, at most their sum."""
    rng = np.random.RandomState(4)
    for _ in range(100):
        lengths = [int(v) for v in rng.randint(0, 50, size=rng.randint(1, 40))]
        lanes = int(rng.randint(1, 9))
        m = campaign_makespan(lengths, lanes)
        assert m >= max(lengths) and m * lanes >= sum(lengths)
        assert m <= -(-sum(lengths) // lanes) + max(lengths)


def test_makespan_refusals():
    with pytest.raises(ValueError, match="lanes"):
        campaign_makespan([1, 2], 0)
    with pytest.raises(ValueError, match="lengths"):
        campaign_makespan([1, -2], 2)


def test_campaign_tasks_fills_in():
    tv, td, tc, tk, caps = campaign_tasks(3, 512, 40)
    assert (tv, td, tc, tk, caps) == ([-1] * 3, [-1] * 3, [-1] * 3, [0] * 3, [40] * 3)
    tv, td, tc, tk, caps = campaign_tasks(3, 512, [2, 6, 13], variants=[{}, {}], dems=[0], costmaps=[0, 1],
                                          task_variant=[1, None, -1], task_dem=[0, -1, None],
                                          task_costmap=[None, 1, 0], task_trajectories=[None, 300, 512])
    assert tv == [1, -1, -1] and td == [0, -1, -1] and tc == [-1, 1, 0] and tk == [0, 300, 512]
    assert caps == [2, 6, 13]
    assert campaign_tasks(2, 8, np.int64(5))[4] == [5, 5]


@pytest.mark.parametrize("kw, words", [
    (dict(max_loops=0), ("max_loops[0]", ">= 1")),
    (dict(max_loops=[3, 0, 2]), ("max_loops[1]",)),
    (dict(max_loops=[3, 2]), ("3 tasks", "max_loops")),
    (dict(task_variant=[0, -1, -1]), ("task_variant", "variants", "empty")),
    (dict(variants=[{}], task_variant=[0, 1, -1]), ("task_variant[1]", "1 rows")),
    (dict(variants=[{}], task_variant=[0, -2, -1]), ("task_variant[1]",)),
    (dict(variants=[{}], task_variant=[0, 0]), ("3 tasks", "task_variant")),
    (dict(task_dem=[0, -1, -1]), ("task_dem", "dems", "empty")),
    (dict(dems=[0], task_dem=[0, 1, -1]), ("task_dem[1]",)),
    (dict(dems=[0], task_dem=[0, -1]), ("3 tasks", "task_dem")),
    (dict(costmaps=[0, 1], task_costmap=[2, 0, 0]), ("task_costmap[0]",)),
    (dict(task_trajectories=[0, 513, 1]), ("task_trajectories[1]", "512")),
    (dict(task_trajectories=[0, -1, 1]), ("task_trajectories[1]",)),
    (dict(task_trajectories=[0, 1]), ("3 tasks", "task_trajectories")),
    (dict(dems=[0] * 257), ("dems", "256")),
    (dict(costmaps=[0] * 1025), ("costmaps", "1024")),
])
def test_campaign_tasks_refusals(kw, words):
    kw = dict(kw)
    max_loops = kw.pop("max_loops", 40)
    with pytest.raises(ValueError) as err:
        campaign_tasks(3, 512, max_loops, **kw)
    for w in words:
        assert w in str(err.value), (w, str(err.value))


def test_campaign_needs_a_task():
    with pytest.raises(ValueError, match="at least one task"):
        campaign_tasks(0, 512, 40)
