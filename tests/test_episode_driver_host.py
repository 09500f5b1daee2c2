"""The five batched-episode entry points (``BatchedPOMCP.run_episodes`` /
``run_episode_queue`` / ``run_planner_queue``, ``BatchedINTMCP.run_episodes`` /
``run_episode_queue``) against a recording stub engine, without a GPU and
without the library: the exact sequence of engine calls with their arguments,
the rows' keys in order and their values, the ``write_row`` / ``on_step``
counts and every guard's exception.  The planners are made with ``__new__``
and given only the attributes the entry points read, so the file characterises
the drivers whatever lies between them and the engine."""
import math
import time
import types

import numpy as np
import psutil
import pytest

from posggym_baselines_amd import _native as N
from posggym_baselines_amd.planning.episodes import EPISODE_RESULT_HEADS
from posggym_baselines_amd.planning.intmcp import BatchedINTMCP
from posggym_baselines_amd.planning.policies import FixedDistributionPolicy
from posggym_baselines_amd.planning.pomcp import BatchedPOMCP

SLOTS, ENTRIES, MAX_STEPS, ACTIONS, SIMS = 4, 6, 3, 3, 7
DISCOUNT = 0.9
POW = [DISCOUNT ** t for t in range(MAX_STEPS)]
TIMING = ((2.0, 6.0, 1.0), 4)      # (update, search, step kernel) ms, steps
RSS_MIB = 512.0
PROBS = [[0.2, 0.3, 0.5], [0.0, 0.25, 0.75]]
IDS = ["slow", "keen"]
BASE_KEYS = EPISODE_RESULT_HEADS + ["env_seed"]


def results(n):
    """``n`` canned ``pomcp_episode_result``s; record 1 never reached the
    planner's statistics (``searched_steps`` 0)."""
    r = np.zeros(n, dtype=N.EPISODE_RESULT_DTYPE)
    for i in range(n):
        r[i]["env_seed"] = 100 + i
        r[i]["len"] = 1 + i % MAX_STEPS
        r[i]["searched_steps"] = 0 if i == 1 else 1 + i % MAX_STEPS
        r[i]["ret"] = 0.1 * (i + 1)
        r[i]["discounted_return"] = 0.07 * (i + 1)
        r[i]["search_depth_sum"] = 10 + 3 * i
        r[i]["num_sims_sum"] = SIMS * (1 + i % MAX_STEPS)
        r[i]["min_value_sum"] = -1.0 - i / 3
        r[i]["max_value_sum"] = 2.0 + i / 7
    return r


def accs(n):
    """``n`` canned belief-accuracy records; record 2 has no recorded step."""
    a = np.zeros(n, dtype=N.EPISODE_BELIEF_ACC_DTYPE)
    for i in range(n):
        a[i]["count"] = 0 if i == 2 else 1 + i % MAX_STEPS
        a[i]["state_sum"] = 0.1 + i / 3
        a[i]["policy_sum"] = 0.2 + i / 7
        a[i]["action_sum"] = 0.3 + i / 11
    return a


ACC_STEPS = (np.arange(SLOTS * MAX_STEPS * 3, dtype=np.float64) / 13).reshape(SLOTS, MAX_STEPS, 3)
POP_INDEX = [1, 0, 0, 1, 1, 0]


class StubEngine:
    """Records every ``episodes_*`` call; ``live`` scripts ``episodes_step``."""

    def __init__(self, live, max_episode_steps=MAX_STEPS, state_belief_only=True):
        self.model = types.SimpleNamespace(
            spec=types.SimpleNamespace(max_episode_steps=max_episode_steps))
        self.config = types.SimpleNamespace(discount=DISCOUNT, state_belief_only=state_belief_only)
        self.A = ACTIONS
        self.live = list(live)
        self.calls = []

    def _rec(self, name, *args, **kw):
        self.calls.append((name, args, kw))

    def episodes_set_population(self, *args, **kw):
        self._rec("set_population", *args, **kw)

    def episodes_track_belief_acc(self, *args, **kw):
        self._rec("track_belief_acc", *args, **kw)

    def episodes_begin(self, *args, **kw):
        self._rec("begin", *args, **kw)

    def episodes_queue_begin(self, *args, **kw):
        self._rec("queue_begin", *args, **kw)

    def episodes_group_queue_begin(self, *args, **kw):
        self._rec("group_queue_begin", *args, **kw)

    def episodes_step(self, *args, **kw):
        self._rec("step", *args, **kw)
        return self.live.pop(0)

    def episodes_results(self):
        self._rec("results")
        return results(SLOTS)

    def episodes_queue_rows(self):
        self._rec("queue_rows")
        q = np.zeros(ENTRIES, dtype=N.EPISODE_QUEUE_ROW_DTYPE)
        q["res"] = results(ENTRIES)
        q["slot"] = [0, 1, 2, 3, 2, 0]
        q["slot_order"] = [0, 0, 0, 0, 1, 1]
        q["policy_index"] = POP_INDEX
        q["acc"] = accs(ENTRIES)
        return q

    def episodes_timing(self):
        self._rec("timing")
        return TIMING

    def episodes_pop_states(self):
        self._rec("pop_states")
        p = np.zeros(SLOTS, dtype=N.EPISODE_POP_STATE_DTYPE)
        p["policy_index"] = POP_INDEX[:SLOTS]
        return p

    def episodes_belief_acc(self):
        self._rec("belief_acc")
        return accs(SLOTS)

    def episodes_belief_acc_steps(self, *args, **kw):
        self._rec("belief_acc_steps", *args, **kw)
        return ACC_STEPS.copy()


@pytest.fixture(autouse=True)
def clock(monkeypatch):
    """``time.time()`` counts the engine calls made so far, so a row's ``time``
    is the number of engine calls its clock spans; the RSS is a constant."""
    engines = []
    monkeypatch.setattr(time, "time", lambda: float(sum(len(e.calls) for e in engines)))
    monkeypatch.setattr(psutil, "Process", lambda: types.SimpleNamespace(
        memory_info=lambda: types.SimpleNamespace(rss=int(RSS_MIB * 1024**2))))
    return engines


def pomcp(clock, live, planned=(MAX_STEPS, True), other_policy_ids=None, trees=SLOTS, **kw):
    p = BatchedPOMCP.__new__(BatchedPOMCP)
    p.engine = StubEngine(live, **kw)
    p.num_trees, p.num_sims, p._planned = trees, SIMS, planned
    p.other_policy_ids = other_policy_ids
    clock.append(p.engine)
    return p


def intmcp(clock, live, planned=MAX_STEPS, **kw):
    p = BatchedINTMCP.__new__(BatchedINTMCP)
    p.engine = StubEngine(live, **kw)
    p.num_pairs, p.num_sims, p._planned_searches = SLOTS, SIMS, planned
    clock.append(p.engine)
    return p


def population():
    model = types.SimpleNamespace(action_spaces={"1": types.SimpleNamespace(n=ACTIONS)})
    return [FixedDistributionPolicy(model, "1", i, p) for i, p in zip(IDS, PROBS)]


class Hooks:
    def __init__(self):
        self.rows, self.steps = [], []

    def write_row(self, row):
        self.rows.append(row)

    def on_step(self, t, planner):
        self.steps.append((t, planner))


def base_row(num, r, elapsed):
    """The reference columns of one record, written out by hand."""
    n = int(r["searched_steps"])
    (upd, search, _), steps = TIMING
    nan = math.nan
    return {
        "num": num, "len": int(r["len"]), "return": float(r["ret"]),
        "discounted_return": float(r["discounted_return"]), "time": float(elapsed),
        "search_time": search / 1e3 / steps if n else nan,
        "update_time": upd / 1e3 / steps if n else nan,
        "reinvigoration_time": 0.0 if n else nan, "evaluation_time": 0.0 if n else nan,
        "policy_calls": 0.0 if n else nan, "inference_time": 0.0 if n else nan,
        "search_depth": int(r["search_depth_sum"]) / n if n else nan,
        "num_sims": int(r["num_sims_sum"]) / n if n else nan,
        "mem_usage": RSS_MIB if n else nan,
        "min_value": float(r["min_value_sum"]) / n if n else nan,
        "max_value": float(r["max_value_sum"]) / n if n else nan,
        "env_seed": int(r["env_seed"]),
    }


def same(a, b):
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return type(a) is type(b) and a == b


def assert_rows(rows, want):
    assert len(rows) == len(want)
    for got, exp in zip(rows, want):
        assert list(got) == list(exp)
        for k in exp:
            assert same(got[k], exp[k]), (k, got[k], exp[k])


def names(engine):
    return [c[0] for c in engine.calls]


def call(engine, name):
    (c,) = [c for c in engine.calls if c[0] == name]
    return c[1], c[2]


STEP = ("step", (SIMS,), {})


# ------------------------------------------------------- BatchedPOMCP.run_episodes
def test_pomcp_run_episodes_plain(clock):
    p, h = pomcp(clock, [3, 1, 0]), Hooks()
    rows = p.run_episodes(write_row=h.write_row, on_step=h.on_step)
    assert p.engine.calls == [
        ("set_population", (None, None), {}),
        ("track_belief_acc", (False, False), {}),
        ("begin", ([0, 1, 2, 3], POW, MAX_STEPS, "agent_done"),
         {"track_states": False, "group": 1}),
        STEP, STEP, STEP, ("results", (), {}), ("timing", (), {})]
    assert_rows(rows, [base_row(b, r, 8) for b, r in enumerate(results(SLOTS))])
    assert [list(r) for r in rows] == [BASE_KEYS] * SLOTS
    assert h.rows == rows and h.steps == [(0, p), (1, p), (2, p)]


def test_pomcp_run_episodes_stops_when_nothing_is_live_or_at_max_steps(clock):
    p = pomcp(clock, [0])
    p.run_episodes([9, 8, 7, 6], until="all_done", belief_states=True)
    assert names(p.engine) == ["set_population", "track_belief_acc", "begin", "step", "results",
                               "timing"]
    assert call(p.engine, "begin") == (([9, 8, 7, 6], POW, MAX_STEPS, "all_done"),
                                       {"track_states": True, "group": 1})
    p = pomcp(clock, [4, 4, 4, 4])
    p.run_episodes()
    assert names(p.engine).count("step") == MAX_STEPS


def test_pomcp_run_episodes_population_and_per_step_accuracy(clock):
    p, h = pomcp(clock, [2, 0], other_policy_ids=["keen", "other"]), Hooks()
    rows = p.run_episodes(other_agents=population(), belief_acc=True, track_per_step=True,
                          write_row=h.write_row, on_step=h.on_step)
    assert p.engine.calls == [
        ("set_population", (PROBS, [-1, 0]), {}),
        ("track_belief_acc", (True, True), {}),
        ("begin", ([0, 1, 2, 3], POW, MAX_STEPS, "agent_done"),
         {"track_states": False, "group": 1}),
        STEP, STEP, ("results", (), {}), ("timing", (), {}), ("pop_states", (), {}),
        ("belief_acc", (), {}), ("belief_acc_steps", (MAX_STEPS,), {})]
    acc = accs(SLOTS)
    want = []
    for b, r in enumerate(results(SLOTS)):
        row = base_row(b, r, 7)
        row["other_policy_id"] = IDS[POP_INDEX[b]]
        n = int(acc[b]["count"])
        for k in ("policy", "action", "state", "history"):
            mean = 0.0 if k == "history" else float(acc[b][k + "_sum"]) / max(n, 1)
            row[f"belief_{k}_acc"] = mean if n else math.nan
            for t in range(MAX_STEPS):
                v = 0.0 if k == "history" else \
                    float(ACC_STEPS[b, t, ("state", "policy", "action").index(k)])
                row[f"belief_{k}_acc_{t}"] = v if t < n else math.nan
        want.append(row)
    assert_rows(rows, want)
    assert math.isnan(rows[2]["belief_state_acc"]) and math.isnan(rows[0]["belief_state_acc_1"])
    assert rows[3]["belief_policy_acc_0"] == ACC_STEPS[3, 0, 1]
    assert h.rows == rows and len(h.steps) == 2


def test_pomcp_run_episodes_named_accuracy_means(clock):
    p = pomcp(clock, [0], state_belief_only=False)
    rows = p.run_episodes(belief_acc=["state", "action"])
    assert names(p.engine) == ["set_population", "track_belief_acc", "begin", "step", "results",
                               "timing", "belief_acc"]
    assert call(p.engine, "track_belief_acc") == ((True, False), {})
    acc = accs(SLOTS)
    assert [list(r) for r in rows] == [BASE_KEYS + ["belief_state_acc", "belief_action_acc"]] * 4
    for b in (0, 1, 3):
        assert rows[b]["belief_state_acc"] == float(acc[b]["state_sum"]) / int(acc[b]["count"])
        assert rows[b]["belief_action_acc"] == float(acc[b]["action_sum"]) / int(acc[b]["count"])
    assert math.isnan(rows[2]["belief_state_acc"]) and math.isnan(rows[2]["belief_action_acc"])


def test_pomcp_run_episodes_root_parallel(clock):
    p, h = pomcp(clock, [1, 0], trees=8), Hooks()
    rows = p.run_episodes([5, 6, 7, 8], root_parallel=2, other_agents=population(),
                          write_row=h.write_row)
    assert p.engine.calls == [
        ("set_population", (PROBS, [-1, -1]), {}),
        ("track_belief_acc", (False, False), {}),
        ("begin", ([5, 6, 7, 8], POW, MAX_STEPS, "agent_done"),
         {"track_states": False, "group": 2}),
        STEP, STEP, ("results", (), {}), ("timing", (), {}), ("pop_states", (), {})]
    want = [dict(base_row(b, r, 7), other_policy_id=IDS[POP_INDEX[b]])
            for b, r in enumerate(results(SLOTS))]
    assert_rows(rows, want)
    assert h.rows == rows


def test_pomcp_run_episodes_guards(clock):
    def raises(exc, match, planner=None, **kw):
        p = planner or pomcp(clock, [0])
        with pytest.raises(exc, match=match):
            p.run_episodes(**kw)
        assert p.engine.calls == []

    raises(ValueError, "until", until="sometime")
    raises(ValueError, "divide", root_parallel=3)
    raises(ValueError, "divide", root_parallel=0)
    raises(ValueError, "root_parallel", root_parallel=2, belief_states=True)
    raises(ValueError, "root_parallel", root_parallel=2, belief_acc=True)
    raises(ValueError, "env_seeds", env_seeds=[1, 2, 3])
    raises(ValueError, "env_seeds has 4 entries for 2 planners of 2 replica trees",
           env_seeds=[1, 2, 3, 4], root_parallel=2)
    raises(ValueError, "max_episode_steps", planner=pomcp(clock, [0], max_episode_steps=None))
    raises(ValueError, "searches=3, reroot=True", planner=pomcp(clock, [0], planned=(3, False)))
    raises(ValueError, r"sized with searches=2, reroot=True\)",
           planner=pomcp(clock, [0], planned=(2, True)))
    raises(ValueError, "re-roots up to 3 times per tree",
           planner=pomcp(clock, [0], planned=(2, True)))
    raises(ValueError, "unknown belief stat", belief_acc=["state", "shape"])
    raises(NotImplementedError, "belief history", belief_acc=True,
           planner=pomcp(clock, [0], state_belief_only=False))
    raises(ValueError, "track_per_step", track_per_step=True)
    raises(ValueError, "1 to 8", other_agents=[])
    raises(ValueError, "duplicate", other_agents=population() + population())
    raises(NotImplementedError, "fixed-distribution", other_agents=[object()])
    # the caller's own capacities are not second-guessed
    p = pomcp(clock, [0], planned=None)
    assert len(p.run_episodes()) == SLOTS


# -------------------------------------------------- BatchedPOMCP.run_episode_queue
def queue_want(elapsed, pop=False, acc_stats=()):
    acc, want = accs(ENTRIES), []
    slot, order = [0, 1, 2, 3, 2, 0], [0, 0, 0, 0, 1, 1]
    for i, r in enumerate(results(ENTRIES)):
        row = base_row(i, r, elapsed)
        row.update(slot=slot[i], slot_order=order[i])
        if pop:
            row["other_policy_id"] = IDS[POP_INDEX[i]]
        n = int(acc[i]["count"])
        for k in acc_stats:
            mean = 0.0 if k == "history" else float(acc[i][k + "_sum"]) / max(n, 1)
            row[f"belief_{k}_acc"] = mean if n else math.nan
        want.append(row)
    return want


def test_pomcp_run_episode_queue(clock):
    p, h = pomcp(clock, [4, 4, 3, 2, 0], other_policy_ids=["slow"]), Hooks()
    seeds = [11, 12, 13, 14, 15, 16]
    rows = p.run_episode_queue(seeds, other_agents=population(), belief_acc=True,
                               belief_states=True, write_row=h.write_row, on_step=h.on_step)
    assert p.engine.calls == [
        ("set_population", (PROBS, [0, -1]), {}),
        ("track_belief_acc", (True, False), {}),
        ("queue_begin", (seeds, POW, MAX_STEPS, "agent_done"), {"track_states": True}),
        STEP, STEP, STEP, STEP, STEP, ("queue_rows", (), {}), ("timing", (), {})]
    assert_rows(rows, queue_want(10, pop=True, acc_stats=("policy", "action", "state", "history")))
    assert math.isnan(rows[2]["belief_policy_acc"]) and rows[0]["belief_history_acc"] == 0.0
    assert h.rows == rows and h.steps == [(t, p) for t in range(5)]


def test_pomcp_run_episode_queue_plain(clock):
    p = pomcp(clock, [0])
    rows = p.run_episode_queue(np.arange(ENTRIES), until="all_done")
    assert p.engine.calls == [
        ("set_population", (None, None), {}),
        ("track_belief_acc", (False, False), {}),
        ("queue_begin", (list(range(ENTRIES)), POW, MAX_STEPS, "all_done"),
         {"track_states": False}),
        STEP, ("queue_rows", (), {}), ("timing", (), {})]
    assert all(type(s) is int for s in call(p.engine, "queue_begin")[0][0])
    assert_rows(rows, queue_want(6))
    assert [list(r) for r in rows] == [BASE_KEYS + ["slot", "slot_order"]] * ENTRIES


def test_pomcp_run_episode_queue_guards(clock):
    seeds = list(range(ENTRIES))

    def raises(exc, match, planner=None, env_seeds=seeds, **kw):
        p = planner or pomcp(clock, [0])
        with pytest.raises(exc, match=match):
            p.run_episode_queue(env_seeds, **kw)
        assert p.engine.calls == []

    raises(ValueError, "until", until="never")
    raises(ValueError, "root_parallel", root_parallel=2)
    raises(ValueError, "at least 4", env_seeds=[1, 2, 3])
    raises(ValueError, "max_episode_steps", planner=pomcp(clock, [0], max_episode_steps=0))
    raises(ValueError, "searches=3, reroot=True", planner=pomcp(clock, [0], planned=(5, False)))
    raises(ValueError, "re-roots up to 3 times per episode",
           planner=pomcp(clock, [0], planned=(1, True)))
    raises(ValueError, "unknown belief stat", belief_acc=["nothing"])
    raises(ValueError, "1 to 8", other_agents=population() * 5)
    # the queue that never drains
    p = pomcp(clock, [1] * (ENTRIES * MAX_STEPS))
    with pytest.raises(RuntimeError, match="run_episode_queue: 1 slots still playing after 18 steps"):
        p.run_episode_queue(seeds)
    assert names(p.engine)[-1] == "step" and names(p.engine).count("step") == ENTRIES * MAX_STEPS


# -------------------------------------------------- BatchedPOMCP.run_planner_queue
def test_pomcp_run_planner_queue(clock):
    p, h = pomcp(clock, [4, 2, 0], trees=12, other_policy_ids=["keen"]), Hooks()
    seeds = [21, 22, 23, 24, 25, 26]
    rows = p.run_planner_queue(seeds, root_parallel=3, other_agents=population(),
                               write_row=h.write_row, on_step=h.on_step)
    assert p.engine.calls == [
        ("set_population", (PROBS, [-1, 0]), {}),
        ("track_belief_acc", (False, False), {}),
        ("group_queue_begin", (seeds, POW, MAX_STEPS, "agent_done", 3), {}),
        STEP, STEP, STEP, ("queue_rows", (), {}), ("timing", (), {})]
    assert_rows(rows, queue_want(8, pop=True))
    assert h.rows == rows and h.steps == [(0, p), (1, p), (2, p)]


def test_pomcp_run_planner_queue_guards(clock):
    seeds = list(range(ENTRIES))

    def raises(exc, match, planner=None, env_seeds=seeds, root_parallel=2, **kw):
        p = planner or pomcp(clock, [0])
        with pytest.raises(exc, match=match):
            p.run_planner_queue(env_seeds, root_parallel=root_parallel, **kw)
        assert p.engine.calls == []

    raises(ValueError, "until", until="")
    raises(ValueError, "root_parallel", root_parallel=1)
    raises(ValueError, "divide", root_parallel=3)
    raises(ValueError, "at least 2", env_seeds=[1])
    raises(ValueError, "max_episode_steps", planner=pomcp(clock, [0], max_episode_steps=None))
    raises(ValueError, "searches=3, reroot=True", planner=pomcp(clock, [0], planned=(2, True)))
    raises(ValueError, "re-roots up to 3 times per episode",
           planner=pomcp(clock, [0], planned=(2, True)))
    raises(ValueError, "1 to 8", other_agents=[])
    p = pomcp(clock, [2] * (ENTRIES * MAX_STEPS))
    with pytest.raises(RuntimeError,
                       match="run_planner_queue: 2 planners still playing after 18 steps"):
        p.run_planner_queue(seeds, root_parallel=2)


# ------------------------------------------------------ BatchedINTMCP.run_episodes
def test_intmcp_run_episodes(clock):
    p, h = intmcp(clock, [2, 0]), Hooks()
    rows = p.run_episodes(other_agents=population(), write_row=h.write_row, on_step=h.on_step)
    assert p.engine.calls == [
        ("set_population", (PROBS,), {}),
        ("begin", ([0, 1, 2, 3], POW, MAX_STEPS, "agent_done"), {}),
        STEP, STEP, ("results", (), {}), ("timing", (), {}), ("pop_states", (), {})]
    assert_rows(rows, [dict(base_row(b, r, 6), other_policy_id=IDS[POP_INDEX[b]])
                       for b, r in enumerate(results(SLOTS))])
    assert h.rows == rows and h.steps == [(0, p), (1, p)]


def test_intmcp_run_episodes_max_steps(clock):
    p = intmcp(clock, [4, 4, 4], planned=2)
    rows = p.run_episodes([4, 3, 2, 1], until="all_done", max_steps=2)
    assert p.engine.calls == [
        ("set_population", (None,), {}),
        ("begin", ([4, 3, 2, 1], POW[:2], 2, "all_done"), {}),
        STEP, STEP, ("results", (), {}), ("timing", (), {})]
    assert_rows(rows, [base_row(b, r, 6) for b, r in enumerate(results(SLOTS))])


def test_intmcp_run_episodes_guards(clock):
    def raises(exc, match, planner=None, **kw):
        p = planner or intmcp(clock, [0])
        with pytest.raises(exc, match=match):
            p.run_episodes(**kw)
        assert p.engine.calls == []

    raises(ValueError, "env_seeds", env_seeds=[1])
    raises(ValueError, "until", until="later")
    raises(ValueError, "run_episodes needs the model's spec.max_episode_steps",
           planner=intmcp(clock, [0], max_episode_steps=None))
    raises(ValueError, "max_steps", max_steps=0)
    raises(ValueError, "max_steps", max_steps=MAX_STEPS + 1)
    raises(ValueError, r"searches=3\)", planner=intmcp(clock, [0], planned=2))
    raises(ValueError, r"sized with searches=2\)", planner=intmcp(clock, [0], planned=2))
    raises(ValueError, "1 to 8", other_agents=[])
    p = intmcp(clock, [0], planned=None)
    assert len(p.run_episodes()) == SLOTS


# ------------------------------------------------- BatchedINTMCP.run_episode_queue
def test_intmcp_run_episode_queue(clock):
    p, h = intmcp(clock, [4, 3, 3, 0]), Hooks()
    seeds = [31, 32, 33, 34, 35, 36]
    rows = p.run_episode_queue(seeds, other_agents=population(), write_row=h.write_row,
                               on_step=h.on_step)
    assert p.engine.calls == [
        ("set_population", (PROBS,), {}),
        ("queue_begin", (seeds, POW, MAX_STEPS, "agent_done"), {}),
        STEP, STEP, STEP, STEP, ("queue_rows", (), {}), ("results", (), {}), ("timing", (), {})]
    assert_rows(rows, queue_want(9, pop=True))
    assert h.rows == rows and len(h.steps) == 4
    p = intmcp(clock, [0])
    assert_rows(p.run_episode_queue(seeds, max_steps=1), queue_want(6))
    assert call(p.engine, "queue_begin") == ((seeds, POW[:1], 1, "agent_done"), {})


def test_intmcp_run_episode_queue_guards(clock):
    seeds = list(range(ENTRIES))

    def raises(exc, match, planner=None, env_seeds=seeds, **kw):
        p = planner or intmcp(clock, [0])
        with pytest.raises(exc, match=match):
            p.run_episode_queue(env_seeds, **kw)
        assert p.engine.calls == []

    raises(ValueError, "at least 4", env_seeds=[1, 2])
    raises(ValueError, "until", until="x")
    raises(ValueError, "run_episode_queue needs the model's spec.max_episode_steps",
           planner=intmcp(clock, [0], max_episode_steps=None))
    raises(ValueError, "max_steps", max_steps=9)
    raises(ValueError, "searches=3", planner=intmcp(clock, [0], planned=1))
    raises(ValueError, "1 to 8", other_agents=population() * 5)
    p = intmcp(clock, [3] * (ENTRIES * MAX_STEPS))
    with pytest.raises(RuntimeError, match="run_episode_queue: 3 slots still playing after 18 steps"):
        p.run_episode_queue(seeds)
    assert names(p.engine)[-1] == "step"
