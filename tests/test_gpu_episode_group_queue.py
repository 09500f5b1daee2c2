"""BatchedPOMCP.run_planner_queue: N >= G episodes on the G root-parallel
planners of a batch of G * K trees, a finished GROUP refilled on the device from
a queue of environment seeds (pomcp_episodes_group_queue_begin; k_queue_rank
over the groups, k_group_queue_refill / k_group_queue_trees,
csrc/pomcp_episode_group_queue.hip, then k_log_drop).  Whole queues against the
assignment rule replayed on the returned lengths, every group's first episode
against the oracle (OracleRootParallel) and, group by group, against the SERIAL
harness: run_planning_episodes over the group's seed sequence on one
POMCP(root_parallel=K) keyed like the group, bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

from gpu_util import product_config, product_model
from oracle.episode import fhex
from root_parallel_util import TEST_CFG, TIMING, last_real, oracle_groups, return_bits
from test_gpu_episode_groups import ALL_MODES, PE_POP, batch, set_mode
from test_gpu_episode_queue import restated_schedule

pytestmark = pytest.mark.gpu

PLANNER_COLUMNS = ("search_depth", "num_sims", "min_value", "max_value")


class GroupQueueRecorder:
    """on_step callback of run_planner_queue: per queue entry the (ego action,
    other action, reward bits) of every step, attributed through
    episode_queue_slots(); an episode's last step comes from
    episode_queue_finished() (its group's record is the next episode's by then)
    and its kept merged record from episode_queue_finished_merged().  Per step
    the groups refilled and the groups left mid-episode; per retired group the
    step it retired at and whether its record or kept merged record changed
    afterwards."""

    def __init__(self, G, N):
        self.G = G
        self.cur = np.arange(G, dtype=np.int32)
        self.steps = [[] for _ in range(N)]
        self.fin_merged = [None] * N
        self.refilled, self.mid, self.retired_at = [], [], {}
        self.parked, self.changed = {}, []

    def __call__(self, t, bp):
        G = self.G
        fin_q, fin = bp.episode_queue_finished()
        st = bp.episode_states()
        now = bp.episode_queue_slots()
        fm = bp.episode_queue_finished_merged()
        merged = bp.episode_merged_roots()
        assert len(fin_q) == len(fin) == len(st) == len(now) == len(fm) == len(merged) == G
        for g in np.nonzero(self.cur >= 0)[0]:
            q = int(self.cur[g])
            src = st
            if fin_q[g] >= 0:
                assert int(fin_q[g]) == q and int(fin["finished"][g]) == 1
                src = fin
                self.fin_merged[q] = bytes(fm[g])
            else:
                assert int(now[g]) == q and int(st["finished"][g]) == 0
                assert bytes(fm[g]) == bytes(len(bytes(fm[g])))   # zeros: none ended here
            assert int(src["res"]["len"][g]) == len(self.steps[q]) + 1
            self.steps[q].append((int(src["last_action"][g]), int(src["last_other_action"][g]),
                                  fhex(src["last_reward"][g])))
        ended = (self.cur >= 0) & (fin_q >= 0)
        self.refilled.append(set(np.nonzero(ended & (now >= 0))[0].tolist()))
        for g in np.nonzero(ended & (now < 0))[0]:
            self.retired_at[int(g)] = t
        self.mid.append(set(np.nonzero((self.cur >= 0) & ~ended & (st["res"]["len"] > 0))[0].tolist()))
        # a refilled group starts from nothing: no step played, no merged record kept
        for g in self.refilled[-1]:
            assert int(st["res"]["len"][g]) == 0 and int(st["finished"][g]) == 0, (t, g)
            assert bytes(merged[g]) == bytes(len(bytes(merged[g]))), (t, g)
        # a retired group keeps its record and its kept merged record
        for g, t0 in self.retired_at.items():
            snap = (st[g].tobytes(), bytes(merged[g]))
            if t0 == t:
                assert snap[1] == self.fin_merged[int(self.cur[g])], g
                self.parked[g] = snap
            elif snap != self.parked[g]:
                self.changed.append((g, t))
        self.cur = now.copy()


@functools.lru_cache(maxsize=None)
def serial_group_seq(env, ego, K, S, g, seeds, until, pop=None):
    """Group g through the serial harness over its whole seed sequence: the
    planner of tests/test_gpu_episode_groups.py serial_group -- a POMCP with
    root_parallel=K and K * S simulations whose replicas are keyed (seed, g*K +
    k) -- reset between the episodes by run_planning_episodes.  Computed once for
    all search kernel modes (they are bit-identical, tests/test_gpu_parity.py).
    Returns (rows, per-episode steps, per-episode step statistics of the steps
    that reached the planner's statistics)."""
    from posggym_baselines_amd.planning import POMCP, RandomSearchPolicy, run_planning_episodes
    from posggym_baselines_amd.planning.engine import PomcpEngine
    from posggym_baselines_amd.planning.policies import FixedDistributionPolicy
    model = product_model(env)
    cfg = product_config(dict(TEST_CFG), K * S)
    cfg.root_parallel = K
    planner = POMCP(model, ego, cfg, RandomSearchPolicy(model, ego))
    planner._engine.close()
    planner._engine = PomcpEngine(model, ego, cfg, num_trees=K, num_sims=S, tree_key_base=g * K,
                                  type_policies=planner.type_policies)
    other = "1" if ego == "0" else "0"
    population = None if pop is None else \
        [FixedDistributionPolicy(model, other, pid, list(p)) for pid, p in pop]
    steps, stats = [], []

    def on_step(t, obs, a, ts):
        if t == 0:
            steps.append([])
            stats.append([])
        steps[-1].append((a[ego], a[other], fhex(ts.rewards[ego])))
        s = planner.step_statistics
        if not np.isnan(s["num_sims"]):
            stats[-1].append({k: s[k] for k in PLANNER_COLUMNS})

    rows = run_planning_episodes(planner, product_model(env), len(seeds), ego,
                                 env_seeds=list(seeds), until=until, other_agents=population,
                                 on_step=on_step)
    planner.close()
    return rows, steps, stats


def check_group(rows, rec, g, env, ego, K, S, seeds, until, pop=None):
    """Every episode of one group against the serial harness: the steps, the
    length, the returns, the drawn policy and the planner columns as sequential
    FP64 sum / n over the serial planner's step statistics."""
    mine = sorted((r for r in rows if r["slot"] == g), key=lambda r: r["slot_order"])
    assert [r["slot_order"] for r in mine] == list(range(len(mine)))
    srows, ssteps, sstats = serial_group_seq(env, ego, K, S, g,
                                             tuple(seeds[r["num"]] for r in mine), until, pop)
    assert len(srows) == len(mine)
    for r, sr, ss, stats in zip(mine, srows, ssteps, sstats):
        where = (g, r["slot_order"], r["num"])
        assert r["env_seed"] == seeds[r["num"]], where
        assert rec.steps[r["num"]] == ss, where
        assert r["len"] == sr["len"] == len(ss), where
        assert fhex(r["return"]) == fhex(sr["return"]), where
        assert fhex(r["discounted_return"]) == fhex(sr["discounted_return"]), where
        assert r.get("other_policy_id") == sr.get("other_policy_id"), where
        n = len(stats)
        assert n > 0, where
        for k in PLANNER_COLUMNS:
            s = 0 if k in ("search_depth", "num_sims") else 0.0
            for st in stats:
                s = s + st[k]
            assert fhex(float(r[k])) == fhex(s / n), (where, k)
    return mine


def check_rows_and_schedule(rows, rec, G, seeds):
    """N rows in queue order whose (slot, slot_order) are the assignment rule's,
    replayed on the returned lengths."""
    from posggym_baselines_amd.planning.episodes import EPISODE_RESULT_HEADS
    N = len(seeds)
    assert len(rows) == N
    assert all(list(r)[:len(EPISODE_RESULT_HEADS) + 3] ==
               EPISODE_RESULT_HEADS + ["env_seed", "slot", "slot_order"] for r in rows)
    assert [r["num"] for r in rows] == list(range(N))
    assert [r["env_seed"] for r in rows] == seeds
    lens = [r["len"] for r in rows]
    assert all(n >= 1 for n in lens) and [len(s) for s in rec.steps] == lens
    assert [(r["slot"], r["slot_order"]) for r in rows] == restated_schedule(G, lens)
    assert sorted(rec.retired_at) == list(range(G))      # every group retired in the end
    assert not rec.changed


def groups_of_wave(w, K, G):
    """The groups with a tree in search wave w (trees [64 w, 64 w + 64))."""
    return {b // K for b in range(64 * w, 64 * w + 64) if b < G * K}


# ---------------------------------------------------------------- Driving, K = 3
DRIVING3 = ("Driving-v1", "0", 3, 24, 8, 3000, 50)
DRIVING3_N = 60


@pytest.mark.parametrize("mode", ALL_MODES)
def test_driving_queue_of_groups_of_three(mode, monkeypatch):
    """72 trees = 24 planners of 3 replicas, 8 simulations per replica, 60 env
    seeds from 3000, until all_done (the oracle's episodes): group 21 owns trees
    63..65, one in search wave 0 and two in wave 1, so its refill sets bits in
    two drop masks while groups 0..20 and 22, 23 share those waves' logs."""
    set_mode(monkeypatch, mode)
    env, ego, K, G, S, first, max_steps = DRIVING3
    N, until = DRIVING3_N, "all_done"
    seeds = list(range(first, first + N))
    groups = oracle_groups(env, ego, K, G, S, first, max_steps)
    bp = batch(env, ego, K, G, S, max_steps)
    A = bp.engine.A
    rec = GroupQueueRecorder(G, N)
    rows = bp.run_planner_queue(seeds, root_parallel=K, until=until, on_step=rec)
    bp.close()
    check_rows_and_schedule(rows, rec, G, seeds)
    # --- every group's first episode is the oracle's
    e = int(ego)
    for g, (trace, records) in enumerate(groups):
        steps, row = trace["steps"], rows[g]
        assert (row["slot"], row["slot_order"], row["len"]) == (g, 0, len(steps)), g
        assert [s[0] for s in rec.steps[g]] == [s["actions"][e] for s in steps], g
        assert [s[1] for s in rec.steps[g]] == [s["actions"][1 - e] for s in steps], g
        assert [s[2] for s in rec.steps[g]] == [s["reward"] for s in steps], g
        assert (fhex(row["return"]), fhex(row["discounted_return"])) == \
            return_bits(steps, TEST_CFG["discount"]), g
        from posggym_baselines_amd import _native as Nat
        m = Nat.PomcpMergedRoot.from_buffer_copy(rec.fin_merged[g])
        last = last_real(records)
        action, visits, totals = last["merged"]
        assert (int(m.action), int(m.num_trees), int(m.error)) == (action, K, 0), g
        assert [float(v) for v in m.visits[:A]] == [float(v) for v in visits], g
        assert [fhex(v) for v in m.totals[:A]] == [fhex(v) for v in totals], g
        assert int(m.search_depth) == last["search_depth"], g
        assert (fhex(m.min_value), fhex(m.max_value)) == \
            (fhex(last["min_value"]), fhex(last["max_value"])), g
    # --- whole groups against the serial harness: group 21, a neighbour of it in
    # each of its two search waves, the group that played most and group 0
    w0, w1 = groups_of_wave(0, K, G), groups_of_wave(1, K, G)
    assert 21 in w0 and 21 in w1 and 20 in w0 and 20 not in w1 and 22 in w1 and 22 not in w0
    played = np.bincount([r["slot"] for r in rows], minlength=G)
    most = int(np.argmax(played))
    chosen = [21, 20, 22]
    for g in (most, 0, 23, 5):
        if g not in chosen and len(chosen) < 5:
            chosen.append(g)
    assert len(chosen) == 5
    for g in chosen:
        assert len(check_group(rows, rec, g, env, ego, K, S, seeds, until)) == played[g]
    # --- the conditions that keep the test from passing vacuously
    assert any(21 in r and m & (w0 - {21}) and m & (w1 - {21})
               for r, m in zip(rec.refilled, rec.mid))
    assert any(len(r) >= 2 for r in rec.refilled)
    assert played[most] >= 3
    total = len(rec.mid)
    assert any(t0 < total - 1 for t0 in rec.retired_at.values())   # retired while others play on


# --------------------------------------------------------------- Driving, K = 70
@pytest.mark.parametrize("mode", ["lane", "wave"])
def test_driving_queue_of_groups_of_seventy(mode, monkeypatch):
    """140 trees = 2 planners of 70 replicas, 4 simulations per replica, 5 env
    seeds from 4100: group 0 is all of search wave 0 and bits 0..5 of wave 1,
    group 1 the rest of wave 1 and wave 2."""
    set_mode(monkeypatch, mode)
    env, ego, K, G, S, first, max_steps = "Driving-v1", "0", 70, 2, 4, 4100, 50
    N, until = 5, "all_done"
    seeds = list(range(first, first + N))
    bp = batch(env, ego, K, G, S, max_steps)
    rec = GroupQueueRecorder(G, N)
    rows = bp.run_planner_queue(seeds, root_parallel=K, until=until, on_step=rec)
    bp.close()
    check_rows_and_schedule(rows, rec, G, seeds)
    for g in range(G):
        check_group(rows, rec, g, env, ego, K, S, seeds, until)
    # a refilled group covers a whole search wave and part of the shared wave 1
    # while the other group is mid-episode in that wave
    assert groups_of_wave(0, K, G) == {0} and groups_of_wave(1, K, G) == {0, 1} and \
        groups_of_wave(2, K, G) == {1}
    assert any(len(r) == 1 and m == {1 - next(iter(r))} for r, m in zip(rec.refilled, rec.mid))


# ------------------------------------------------------ PursuitEvasion, ego "1"
def test_pursuit_evasion_queue_of_groups_against_a_population():
    """30 trees = 6 planners of 5 replicas, ego "1", 15 env seeds from 5000, the
    two-policy population of tests/test_gpu_episode_groups.py drawn per group
    and entry."""
    from posggym_baselines_amd.planning.episodes import PopulationAgents
    from posggym_baselines_amd.planning.policies import FixedDistributionPolicy
    env, ego, K, G, S, first, max_steps = "PursuitEvasion-v1", "1", 5, 6, 8, 5000, 100
    N, until = 15, "agent_done"
    seeds = list(range(first, first + N))
    model = product_model(env)
    pop = [FixedDistributionPolicy(model, "0", pid, list(p)) for pid, p in PE_POP]
    bp = batch(env, ego, K, G, S, max_steps)
    rec = GroupQueueRecorder(G, N)
    rows = bp.run_planner_queue(seeds, root_parallel=K, until=until, other_agents=pop, on_step=rec)
    bp.close()
    check_rows_and_schedule(rows, rec, G, seeds)
    drawn = []
    for s in seeds:
        agents = PopulationAgents(model, s, pop)
        agents.reset()
        drawn.append(agents.policy_id)
    assert [r["other_policy_id"] for r in rows] == drawn
    assert set(drawn) == {pid for pid, _ in PE_POP}
    played = np.bincount([r["slot"] for r in rows], minlength=G)
    most = int(np.argmax(played))
    assert played[most] >= 2
    chosen = [most, 0 if most != 0 else G - 1]
    seen = set()
    for g in chosen:
        for r in check_group(rows, rec, g, env, ego, K, S, seeds, until, PE_POP):
            seen.add(r["other_policy_id"])
    assert len(seen) == 2                                 # both policies were compared
    assert any(r["slot"] in chosen and r["slot_order"] > 0 for r in rows)


# ----------------------------------------------------------------------- guards
def same_rows(a, b):
    return len(a) == len(b) and all(
        list(x) == list(y) and
        all(x[k] == y[k] if isinstance(x[k], str) else fhex(float(x[k])) == fhex(float(y[k]))
            for k in x if k not in TIMING)
        for x, y in zip(a, b))


def test_guards_refuse_before_any_launch_and_the_engine_plays_on():
    from posggym_baselines_amd import _native as N
    from posggym_baselines_amd._native import PomcpError
    env, S, max_steps = "Driving-v1", 8, 50
    qseeds = list(range(3100, 3108))

    def engine(**kw):
        return batch(env, "0", 1, 6, S, max_steps, **kw)

    bp = engine()

    def nothing_launched():
        with pytest.raises(PomcpError):   # no batch of episodes exists
            bp.episode_states()
        with pytest.raises(PomcpError):
            bp.episode_queue_slots()
        with pytest.raises(PomcpError):
            bp.episode_queue_finished_merged()

    with pytest.raises(ValueError, match="root_parallel"):
        bp.run_planner_queue(qseeds, root_parallel=1)
    with pytest.raises(ValueError, match="root_parallel"):
        bp.run_planner_queue(qseeds, root_parallel=0)
    with pytest.raises(ValueError, match="divide"):
        bp.run_planner_queue(qseeds, root_parallel=4)
    with pytest.raises(ValueError, match="at least 3"):
        bp.run_planner_queue(qseeds[:2], root_parallel=2)
    with pytest.raises(ValueError, match="until"):
        bp.run_planner_queue(qseeds, root_parallel=2, until="never")
    with pytest.raises(TypeError):
        bp.run_planner_queue(qseeds)
    with pytest.raises(ValueError, match="root_parallel"):   # the old entry point still refuses
        bp.run_episode_queue(range(12), root_parallel=2)
    from posggym_baselines_amd.planning import BatchedPOMCP
    small = BatchedPOMCP(product_model(env), "0", product_config(TEST_CFG, S), 6, S, searches=1,
                         reroot=False)
    with pytest.raises(ValueError, match="searches=50, reroot=True"):
        small.run_planner_queue(qseeds, root_parallel=2)
    small.close()
    nothing_launched()
    # --- the C ABI's own refusals
    lib, ctx = bp.engine._lib, bp.engine._ctx
    seeds = (C.c_uint64 * 8)(*qseeds)
    pw = (C.c_double * max_steps)(*[TEST_CFG["discount"] ** t for t in range(max_steps)])
    begin = lib.pomcp_episodes_group_queue_begin
    assert begin(ctx, 1, seeds, 8, pw, max_steps, N.UNTIL_ALL_DONE) == N.POMCP_E_INVALID
    assert begin(ctx, 4, seeds, 8, pw, max_steps, N.UNTIL_ALL_DONE) == N.POMCP_E_INVALID
    assert begin(ctx, 2, seeds, 2, pw, max_steps, N.UNTIL_ALL_DONE) == N.POMCP_E_INVALID
    assert begin(ctx, 2, None, 8, pw, max_steps, N.UNTIL_ALL_DONE) == N.POMCP_E_INVALID
    assert lib.pomcp_episodes_track_states(ctx, 1) == 0
    assert begin(ctx, 2, seeds, 8, pw, max_steps, N.UNTIL_ALL_DONE) == N.POMCP_E_UNSUPPORTED
    assert lib.pomcp_episodes_track_states(ctx, 0) == 0
    assert lib.pomcp_episodes_track_belief_acc(ctx, 1, 0) == 0
    assert begin(ctx, 2, seeds, 8, pw, max_steps, N.UNTIL_ALL_DONE) == N.POMCP_E_UNSUPPORTED
    assert lib.pomcp_episodes_track_belief_acc(ctx, 0, 0) == 0
    live = C.c_int32()
    assert lib.pomcp_episodes_step(ctx, S, C.byref(live)) == N.POMCP_E_STATE
    nothing_launched()
    # the group size is the call's own: a stored group neither helps nor is changed
    assert lib.pomcp_episodes_set_group(ctx, 3) == 0
    assert lib.pomcp_episodes_queue_begin(ctx, seeds, 8, pw, max_steps, N.UNTIL_ALL_DONE) == \
        N.POMCP_E_UNSUPPORTED
    nothing_launched()
    assert lib.pomcp_episodes_set_group(ctx, 1) == 0
    # --- the same engine plays a queue of groups, an ungrouped queue, a batch of groups
    rows_q = bp.run_planner_queue(qseeds, root_parallel=2, until="all_done")
    assert len(bp.episode_queue_slots()) == 3 and len(bp.episode_merged_roots()) == 3
    assert len(bp.episode_queue_finished_merged()) == 3
    rows_u = bp.run_episode_queue(qseeds, until="all_done")
    assert len(bp.episode_queue_slots()) == 6
    with pytest.raises(PomcpError):   # the ungrouped queue ended the mode
        bp.episode_queue_finished_merged()
    rows_g = bp.run_episodes(qseeds[:3], until="all_done", root_parallel=2)
    with pytest.raises(PomcpError):   # run_episodes ended queue mode
        bp.episode_queue_slots()
    bp.close()
    # the same calls on a fresh engine: the same rows (the streams went on alike)
    other = engine()
    assert same_rows(rows_q, other.run_planner_queue(qseeds, root_parallel=2, until="all_done"))
    assert same_rows(rows_u, other.run_episode_queue(qseeds, until="all_done"))
    assert same_rows(rows_g, other.run_episodes(qseeds[:3], until="all_done", root_parallel=2))
    other.close()
    # and each alone on a fresh engine: the first equals, the later ones started
    # from streams the earlier calls had advanced
    fresh = engine()
    rows_u0 = fresh.run_episode_queue(qseeds, until="all_done")
    fresh.close()
    fresh = engine()
    rows_g0 = fresh.run_episodes(qseeds[:3], until="all_done", root_parallel=2)
    fresh.close()
    assert not same_rows(rows_u, rows_u0) and not same_rows(rows_g, rows_g0)
    assert [r["num"] for r in rows_q] == list(range(8)) and {r["slot"] for r in rows_q} == {0, 1, 2}
    assert [r["num"] for r in rows_g] == [0, 1, 2]


# ------------------------------------------- the overflow map's generation wrap
EPOCH_MASK = 16383     # csrc/pomcp_device.h kEpochMask
WRAP = dict(env="PursuitEvasion-v1", ego="1", K=5, G=6, S=8, N=15, first=5000, max_steps=100,
            until="agent_done", twin_gen=5000)


class MapWatch:
    """GroupQueueRecorder plus the map scans (gpu_util.map_scan: live, stale,
    generation) of a group's K trees right after a refill of interest -- the
    trees are empty then, before the new episode's first update.  watch: {group:
    the refill (1, 2, ...) to scan}; None: every group's first two."""

    def __init__(self, G, N, K, watch=None):
        self.rec = GroupQueueRecorder(G, N)
        self.K, self.watch = K, watch
        self.refills = [0] * G
        self.scans = {}

    def __call__(self, t, bp):
        from gpu_util import map_scan
        self.rec(t, bp)
        for g in sorted(self.rec.refilled[-1]):
            self.refills[g] += 1
            k = self.refills[g]
            if (k <= 2) if self.watch is None else (self.watch.get(g) == k):
                self.scans[(g, k)] = map_scan(bp.engine, range(g * self.K, (g + 1) * self.K))


def wrap_run(generations, watch):
    """The queue with the obs-child map under load (one inline slot, as
    tests/test_gpu_child_map.py) from the given starting generations."""
    from gpu_util import set_map_generation
    from posggym_baselines_amd import _native as N
    w = WRAP
    seeds = list(range(w["first"], w["first"] + w["N"]))
    bp = batch(w["env"], w["ego"], w["K"], w["G"], w["S"], w["max_steps"])
    assert N.load().pomcp_debug_set_inline_slots(bp.engine._ctx, 1) == 0
    set_map_generation(bp.engine, generations)
    watcher = MapWatch(w["G"], w["N"], w["K"], watch)
    rows = bp.run_planner_queue(seeds, root_parallel=w["K"], until=w["until"], on_step=watcher)
    bp.close()
    check_rows_and_schedule(rows, watcher.rec, w["G"], seeds)
    return rows, watcher


@functools.lru_cache(maxsize=None)
def wrap_twin():
    """The queue played from a generation far from the wrap, once for all search
    kernels (they are bit-identical): the schedule and the per-tree generation
    counts the wrapping run's starting generations are derived from."""
    return wrap_run(WRAP["twin_gen"], None)


@pytest.mark.parametrize("mode", ["lane", "wave"])
def test_a_refilled_groups_trees_wrap_their_map_generation(mode, monkeypatch):
    """30 trees = 6 planners of 5 replicas, 15 seeds.  Every tree of the watched
    groups starts at 16,384 minus the generations the twin run counted for it up
    to the watched refill (the reset of the begin, its re-roots, the refills), so
    that refill wraps all K of the group's maps: two groups refilled in the same
    batch step at their first refill (k_group_queue_trees clears ten maps of one
    wave in turn while other groups of the wave are mid-episode), one group at
    its second refill.  The rows and per-step records equal the twin's, and a
    wrapped tree's map reads (0, 0, 1) right after the refill where the twin's
    holds stale entries."""
    set_mode(monkeypatch, mode)
    K, G, gen0 = WRAP["K"], WRAP["G"], WRAP["twin_gen"]
    trows, tw = wrap_twin()
    # two groups whose first refills fall into one batch step, with a group mid-episode
    first_refill = {}
    for t, r in enumerate(tw.rec.refilled):
        for g in r:
            first_refill.setdefault(g, t)
    step = next(t for t in sorted(set(first_refill.values()))
                if sum(1 for s in first_refill.values() if s == t) >= 2 and tw.rec.mid[t])
    together = sorted(g for g, s in first_refill.items() if s == step)[:2]
    second = next(g for g in range(G) if g not in together and (g, 2) in tw.scans)
    watch = {together[0]: 1, together[1]: 1, second: 2}
    gens = [gen0 + b for b in range(G * K)]
    for g, k in watch.items():
        for j, (_, _, gen) in enumerate(tw.scans[(g, k)]):
            assert gen0 < gen < EPOCH_MASK                # (the twin never wrapped)
            gens[g * K + j] = EPOCH_MASK + 1 - (gen - gen0)
    print("watched refills:", watch, "at step", step, "generations:",
          {g: gens[g * K:(g + 1) * K] for g in watch})
    rows, w = wrap_run(gens, watch)
    assert len(rows) == len(trows)
    for r, tr in zip(rows, trows):
        assert list(r) == list(tr)
        for k in r:
            if k not in TIMING:
                assert fhex(float(r[k])) == fhex(float(tr[k])), (r["num"], k)
    assert w.rec.steps == tw.rec.steps and w.rec.fin_merged == tw.rec.fin_merged
    print("scans after the watched refills:", w.scans, "the twin's:",
          {k: tw.scans[k] for k in w.scans})
    assert sorted(w.scans) == sorted(watch.items())
    for key, scans in w.scans.items():
        assert scans == [(0, 0, 1)] * K, key
        assert all(s[0] == 0 for s in tw.scans[key]) and sum(s[1] for s in tw.scans[key]) > 0, key
    assert set(together) <= w.rec.refilled[step] and w.rec.mid[step]
