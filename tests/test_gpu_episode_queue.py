"""BatchedPOMCP.run_episode_queue: N >= num_trees episodes on the batch's slots,
a finished tree refilled on the device from a queue of environment seeds
(pomcp_episodes_queue_begin; k_queue_rank / k_queue_refill / k_log_drop,
csrc/pomcp_episode_queue.hip).  k_log_drop alone against a numpy filter of the
logs read back; whole queues against the assignment rule restated in Python
and, slot by slot, against the SERIAL harness (run_planning_episodes over the
slot's seed sequence on one planner keyed like the slot), bit for bit, on every
search kernel mode."""
import functools

import numpy as np
import pytest

from gpu_util import product_config, product_model
from oracle.episode import fhex
from test_gpu_episode_population import (EGO, OTHER, PE_POP, PE_S, PE_STEPS, TEST_CFG,
                                         pe_population, potmmcp_setup, swap_engine)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["lane", "lane_eager", "wave", "wave_tree", "wave_plain"])
def search_kernel(request, monkeypatch):
    """The search kernel modes of tests/test_gpu_batched_episodes.py."""
    kind, _, mode = request.param.partition("_")
    monkeypatch.setenv("POMCP_SEARCH_KERNEL", kind)
    if kind == "lane":
        monkeypatch.setenv("POMCP_DEFER_CUTOFF", "0" if mode == "eager" else "1")
    elif mode:
        monkeypatch.setenv("POMCP_STEP_TREE", "1" if mode == "tree" else "0")
    return kind


S = 32
ID_BITS = 26          # csrc/pomcp_device.h kIdBits
DROP_PASS = 2048      # csrc/pomcp_episode_queue.hip kDropThreads * kDropRecs
PLANNER_COLUMNS = ("search_depth", "num_sims", "min_value", "max_value")


# ------------------------------------------------------------ k_log_drop alone
def searched_batch(potmmcp):
    """70 Driving-v1 trees (two search waves, the second with 6 trees) after an
    initial update and one search."""
    from posggym_baselines_amd.planning import BatchedPOMCP
    if potmmcp:
        from posggym_baselines_amd.planning.potmmcp import type_policy_tables
        data, model, others, meta, mix, cfg, pop = potmmcp_setup()
        bp = BatchedPOMCP(model, EGO, cfg, 70, data["num_sims"], searches=2, reroot=True,
                          type_policies=type_policy_tables(model, EGO, meta, mix),
                          other_policy_ids=list(mix.policies))
    else:
        bp = BatchedPOMCP(product_model("Driving-v1"), EGO, product_config(TEST_CFG, S), 70, S,
                          searches=2, reroot=True)
    bp.init_synthetic(1000)
    bp.search()
    return bp


def mask_of(lanes):
    return sum(1 << l for l in lanes)


def filtered(log, mask):
    ids = log[0]
    keep = ((np.uint64(mask) >> (ids >> np.uint32(ID_BITS)).astype(np.uint64)) & np.uint64(1)) == 0
    return [a[keep] if a is not None else None for a in log]


def assert_logs_equal(got, exp, where):
    for g, e in zip(got, exp):
        assert (g is None) == (e is None), where
        if g is not None:
            assert g.tobytes() == e.tobytes(), where


@pytest.mark.parametrize("potmmcp", [False, True], ids=["plain", "potmmcp_aux"])
def test_log_drop_equals_a_numpy_filter_of_the_log(potmmcp):
    bp = searched_batch(potmmcp)
    before = [bp.engine.debug_wave_log(w) for w in range(2)]
    assert (before[0][3] is not None) == potmmcp
    lanes = [np.unique(b[0] >> np.uint32(ID_BITS)).tolist() for b in before]
    print("log records per wave:", [len(b[0]) for b in before], "lanes of wave 1:", lanes[1])
    # the test's own conditions: wave 0's log takes more than one pass of the
    # kernel, every tree of both waves has records
    assert len(before[0][0]) > DROP_PASS
    assert lanes[0] == list(range(64)) and lanes[1] == list(range(6))
    masks = [mask_of([0, 5, 63]), mask_of([1])]
    bp.engine.debug_log_drop(masks)
    for w in range(2):
        got = bp.engine.debug_wave_log(w)
        exp = filtered(before[w], masks[w])
        assert 0 < len(exp[0]) < len(before[w][0])
        assert_logs_equal(got, exp, w)
    bp.close()
    if potmmcp:
        return
    # a fresh engine: zero masks leave the logs bit-identical, full masks empty them
    bp = searched_batch(False)
    fresh = [bp.engine.debug_wave_log(w) for w in range(2)]
    for w in range(2):    # (the same searches: the same logs)
        assert_logs_equal(fresh[w], before[w], w)
    bp.engine.debug_log_drop([0, 0])
    for w in range(2):
        assert_logs_equal(bp.engine.debug_wave_log(w), before[w], w)
    bp.engine.debug_log_drop([2**64 - 1, 2**64 - 1])
    for w in range(2):
        assert len(bp.engine.debug_wave_log(w)[0]) == 0
    bp.close()


# ------------------------------------------------------------------ whole queues
class QueueRecorder:
    """on_step callback of run_episode_queue: per queue entry the (ego action,
    other action, reward bits) of every step, attributed through
    episode_queue_slots(); an episode's last step comes from
    episode_queue_finished() (its slot's record is the next episode's by then).
    Per step, the slots refilled and the slots left mid-episode."""

    def __init__(self, B, N):
        self.cur = np.arange(B, dtype=np.int32)
        self.steps = [[] for _ in range(N)]
        self.refilled, self.mid, self.retired_at = [], [], {}

    def __call__(self, t, bp):
        fin_q, fin = bp.episode_queue_finished()
        st = bp.episode_states()
        now = bp.episode_queue_slots()
        for b in np.nonzero(self.cur >= 0)[0]:
            q = int(self.cur[b])
            src = st
            if fin_q[b] >= 0:
                assert int(fin_q[b]) == q and int(fin["finished"][b]) == 1
                src = fin
            else:
                assert int(now[b]) == q and int(st["finished"][b]) == 0
            assert int(src["res"]["len"][b]) == len(self.steps[q]) + 1
            self.steps[q].append((int(src["last_action"][b]), int(src["last_other_action"][b]),
                                  fhex(src["last_reward"][b])))
        ended = (self.cur >= 0) & (fin_q >= 0)
        self.refilled.append(set(np.nonzero(ended & (now >= 0))[0].tolist()))
        for b in np.nonzero(ended & (now < 0))[0]:
            self.retired_at[int(b)] = t
        self.mid.append(set(np.nonzero((self.cur >= 0) & ~ended & (st["res"]["len"] > 0))[0].tolist()))
        self.cur = now.copy()


def restated_schedule(B, lens):
    """The assignment rule replayed on the episodes' lengths: per queue entry
    (slot, ordinal within the slot)."""
    N = len(lens)
    out = [None] * N
    cur, left, order = list(range(B)), [lens[b] for b in range(B)], [0] * B
    for b in range(B):
        out[b] = (b, 0)
    nxt = B
    while any(q >= 0 for q in cur):
        for b in range(B):
            if cur[b] >= 0:
                left[b] -= 1
        for b in range(B):
            if cur[b] >= 0 and left[b] == 0:
                if nxt < N:
                    order[b] += 1
                    cur[b], left[b] = nxt, lens[nxt]
                    out[nxt] = (b, order[b])
                    nxt += 1
                else:
                    cur[b] = -1
    return out


@functools.lru_cache(maxsize=None)
def serial_slot(env, slot, seeds, until, with_pop, ego=EGO, num_sims=S):
    """The serial harness over one slot's seed sequence, on one planner keyed
    like the slot; computed once for all modes (the search kernels are
    bit-identical, tests/test_gpu_parity.py).  Returns (rows, per-episode steps,
    per-episode lists of the planner statistics of the steps that reached
    PlanningStatTracker).  ego / num_sims: the planning agent and its simulations
    per search (tests/test_gpu_child_map.py plays the other agent)."""
    from posggym_baselines_amd.planning import (POMCP, BeliefStatTracker, EpisodeEnvView,
                                                RandomSearchPolicy, run_planning_episodes)
    model = product_model(env)
    other = next(i for i in model.possible_agents if i != ego)
    cfg = product_config(TEST_CFG, num_sims)
    planner = POMCP(model, ego, cfg, RandomSearchPolicy(model, ego))
    swap_engine(planner, model, cfg, num_sims, slot, ego=ego)
    env_model = product_model(env)
    tracker = pop = None
    if with_pop:
        pop = pe_population(model)
        tracker = BeliefStatTracker(planner, EpisodeEnvView(env_model, ego), track_per_step=True,
                                    stats_to_track=["state"])
    steps, tracked = [], []

    def on_step(t, obs, a, ts):
        if t == 0:
            steps.append([])
            tracked.append(None)
        steps[-1].append((a[ego], a[other], fhex(ts.rewards[ego])))
        # (the tracker's own lists so far: the last copy is the whole episode's)
        tracked[-1] = {k: list(planner.stat_tracker._current_stats[k]) for k in PLANNER_COLUMNS}

    rows = run_planning_episodes(planner, env_model, len(seeds), ego, env_seeds=list(seeds),
                                 until=until, belief_tracker=tracker, other_agents=pop,
                                 on_step=on_step)
    planner._engine.close()
    return rows, steps, tracked


def sequential_mean(values):
    """The batch's planner columns: the sequential FP64 sum of the steps that
    reached the statistics / their count (NaN for none)."""
    vals = [float(v) for v in values if not np.isnan(v)]
    total = 0.0
    for v in vals:
        total = total + v
    return total / len(vals) if vals else float("nan")


def check_slot(rows, rec, slot, env, seeds, until, with_pop=False, **planner):
    """Every episode of one slot against the serial harness (planner: serial_slot's
    ego / num_sims)."""
    mine = sorted((r for r in rows if r["slot"] == slot), key=lambda r: r["slot_order"])
    assert [r["slot_order"] for r in mine] == list(range(len(mine)))
    srows, ssteps, stracked = serial_slot(env, slot, tuple(seeds[r["num"]] for r in mine), until,
                                          with_pop, **planner)
    assert len(srows) == len(mine)
    for r, sr, ss, sk in zip(mine, srows, ssteps, stracked):
        where = (slot, r["slot_order"], r["num"])
        assert r["env_seed"] == seeds[r["num"]], where
        assert rec.steps[r["num"]] == ss, where
        assert r["len"] == sr["len"] == len(ss), where
        assert fhex(r["return"]) == fhex(sr["return"]), where
        assert fhex(r["discounted_return"]) == fhex(sr["discounted_return"]), where
        for k in PLANNER_COLUMNS:
            assert fhex(float(r[k])) == fhex(sequential_mean(sk[k])), (where, k)
        if with_pop:
            assert r["other_policy_id"] == sr["other_policy_id"], where
            total = 0.0
            for t in range(sr["len"]):
                total = total + sr[f"belief_state_acc_{t}"]
            assert fhex(r["belief_state_acc"]) == fhex(total / sr["len"]), where
    return mine


def test_driving_queue_equals_the_rule_and_the_serial_harness():
    """B = 70 slots (two search waves, the second with 6 trees), N = 200
    entries, until all_done, uniform other agents."""
    from posggym_baselines_amd.planning import BatchedPOMCP
    from posggym_baselines_amd.planning.episodes import EPISODE_RESULT_HEADS
    B, N, first, max_steps = 70, 200, 3000, 50
    seeds = list(range(first, first + N))
    bp = BatchedPOMCP(product_model("Driving-v1"), EGO, product_config(TEST_CFG, S), B, S,
                      searches=max_steps, reroot=True)
    rec = QueueRecorder(B, N)
    rows = bp.run_episode_queue(seeds, until="all_done", on_step=rec)
    bp.close()
    assert len(rows) == N
    assert all(list(r) == EPISODE_RESULT_HEADS + ["env_seed", "slot", "slot_order"] for r in rows)
    assert [r["num"] for r in rows] == list(range(N))
    assert [r["env_seed"] for r in rows] == seeds
    lens = [r["len"] for r in rows]
    assert all(1 <= n <= max_steps for n in lens)
    assert [len(s) for s in rec.steps] == lens
    # --- the whole schedule is the rule's, replayed on the lengths
    assert [(r["slot"], r["slot_order"]) for r in rows] == restated_schedule(B, lens)
    assert sorted(rec.retired_at) == list(range(B))      # every slot retired in the end
    # --- slots against the serial harness: chosen after the run, from both waves
    played = np.bincount([r["slot"] for r in rows], minlength=B)
    most = int(np.argmax(played))
    wave1 = 64 + int(np.argmax(played[64:]))
    chosen = []
    for b in (most, wave1, 0, 5, 63, 65):
        if b not in chosen:
            chosen.append(b)
    assert len(chosen) <= 8 and any(b < 64 for b in chosen) and any(b >= 64 for b in chosen)
    for b in chosen:
        mine = check_slot(rows, rec, b, "Driving-v1", seeds, "all_done")
        assert len(mine) == played[b]
    # --- the conditions that keep the test from passing vacuously
    assert played[most] >= 3
    for wave in (range(0, 64), range(64, 70)):
        w = set(wave)
        assert any(r & w and m & w for r, m in zip(rec.refilled, rec.mid)), wave
    assert any(b in m and r & (set(range(64)) if b < 64 else set(range(64, 70)))
               for b in chosen for r, m in zip(rec.refilled, rec.mid))


def test_pursuit_evasion_queue_with_a_population_and_the_state_accuracy():
    """B = 24, N = 60, until agent_done, the 2-policy population of
    tests/test_gpu_episode_population.py, belief_acc=["state"]."""
    from posggym_baselines_amd.planning import BatchedPOMCP
    B, N, first = 24, 60, 2000
    assert S == PE_S
    seeds = list(range(first, first + N))
    model = product_model("PursuitEvasion-v1")
    bp = BatchedPOMCP(model, EGO, product_config(TEST_CFG, S), B, S, searches=PE_STEPS, reroot=True)
    rec = QueueRecorder(B, N)
    rows = bp.run_episode_queue(seeds, until="agent_done", other_agents=pe_population(model),
                                belief_acc=["state"], on_step=rec)
    bp.close()
    lens = [r["len"] for r in rows]
    assert len(rows) == N and all(n >= 1 for n in lens)
    assert [(r["slot"], r["slot_order"]) for r in rows] == restated_schedule(B, lens)
    assert {r["other_policy_id"] for r in rows} == {p for p, _ in PE_POP}
    assert all("belief_state_acc" in r and "belief_state_acc_0" not in r for r in rows)
    played = np.bincount([r["slot"] for r in rows], minlength=B)
    most = int(np.argmax(played))
    chosen = [most] + [b for b in (0, 11, 23) if b != most]
    assert len(chosen) <= 4 and played[most] >= 3
    seen = set()
    for b in chosen:
        for r in check_slot(rows, rec, b, "PursuitEvasion-v1", seeds, "agent_done", with_pop=True):
            seen.add(r["other_policy_id"])
    assert len(seen) == 2                                 # both policies were compared
    assert any(r["belief_state_acc"] > 0.0 for r in rows)
    assert any(r["slot"] in chosen and r["slot_order"] > 0 and r["belief_state_acc"] > 0.0
               for r in rows)


def test_guards_coexistence_and_retired_slots():
    from posggym_baselines_amd._native import PomcpError
    from posggym_baselines_amd.planning import BatchedPOMCP
    B, N, max_steps = 8, 20, 50
    qseeds = list(range(3100, 3100 + N))
    eseeds = list(range(3300, 3300 + B))

    def engine(**kw):
        kw = {"searches": max_steps, "reroot": True, **kw}
        return BatchedPOMCP(product_model("Driving-v1"), EGO, product_config(TEST_CFG, S), B, S, **kw)

    # --- guards, before anything is launched
    bp = engine()
    with pytest.raises(ValueError, match="at least 8"):
        bp.run_episode_queue(qseeds[:B - 1])
    with pytest.raises(ValueError, match="until"):
        bp.run_episode_queue(qseeds, until="never")
    with pytest.raises(ValueError, match="unknown belief stat"):
        bp.run_episode_queue(qseeds, belief_acc=["states"])
    with pytest.raises(ValueError, match="1 to 8"):
        bp.run_episode_queue(qseeds, other_agents=[])
    with pytest.raises(TypeError):
        bp.run_episode_queue(qseeds, track_per_step=True)
    with pytest.raises(PomcpError):   # nothing was launched: no batch of episodes exists
        bp.episode_states()
    with pytest.raises(PomcpError):
        bp.episode_queue_slots()
    small = engine(searches=1, reroot=False)
    with pytest.raises(ValueError, match="searches=50, reroot=True"):
        small.run_episode_queue(qseeds)
    small.close()

    # --- a retired slot keeps the root statistics of its last real search
    rec = QueueRecorder(B, N)
    kept, changed = {}, []

    def on_step(t, bp_):
        rec(t, bp_)
        stats = bp_.engine.root_stats()
        for b, t0 in rec.retired_at.items():
            now = bytes(stats[b])
            if t0 == t:
                kept[b] = now
            elif now != kept[b]:
                changed.append((b, t))

    rows = bp.run_episode_queue(qseeds, until="all_done", on_step=on_step)
    assert len(kept) == B and not changed
    early = [b for b, t0 in rec.retired_at.items() if t0 < len(rec.mid) - 1]
    assert early                      # some slot stayed retired through later steps
    # --- queue mode is left cleanly and the planners' streams continue
    rows1 = rows
    after1 = bp.run_episodes(eseeds, until="all_done")
    with pytest.raises(PomcpError):   # run_episodes ended queue mode
        bp.episode_queue_slots()
    bp.close()
    other = engine()
    rows2 = other.run_episode_queue(qseeds, until="all_done")
    after2 = other.run_episodes(eseeds, until="all_done")
    other.close()
    fresh = engine()
    after_fresh = fresh.run_episodes(eseeds, until="all_done")
    fresh.close()
    timing = {"time", "search_time", "update_time", "mem_usage"}

    def same(a, b):
        return all(fhex(float(x[k])) == fhex(float(y[k])) for x, y in zip(a, b) for k in x
                   if k not in timing)

    assert same(rows1, rows2) and same(after1, after2)
    assert len(after1) == B and [r["num"] for r in after1] == list(range(B))
    assert not same(after1, after_fresh)     # the streams went on from the queue's episodes
    # the serial harness says the same: slot b's queue episodes, then the batch's episode b
    for b in (0, B - 1):
        mine = sorted((r for r in rows1 if r["slot"] == b), key=lambda r: r["slot_order"])
        srows, _, stracked = serial_slot(
            "Driving-v1", b, tuple(r["env_seed"] for r in mine) + (eseeds[b],), "all_done", False)
        for r, sr, sk in zip(mine + [after1[b]], srows, stracked):
            assert r["len"] == sr["len"] and fhex(r["return"]) == fhex(sr["return"]), b
            for k in PLANNER_COLUMNS:
                assert fhex(float(r[k])) == fhex(sequential_mean(sk[k])), (b, k)
