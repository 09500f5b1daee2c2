"""IntmcpEngine.reset_pairs and BatchedINTMCP.run_episode_queue: some pairs of a
live batch reset on the device (k_im_clear_pairs / k_im_reset_pairs,
csrc/intmcp_episode_queue.hip) and N >= num_pairs episodes played on the batch's
slots, a finished pair reset and refilled from a device-resident queue
(intmcp_episodes_queue_begin; k_queue_rank / k_im_queue_list / k_im_clear_pairs /
k_im_queue_refill).  The reset alone against the arena scan and the untouched
neighbours' bytes; reset-then-replay against the whole-context reset of a
one-pair engine; whole queues against the assignment rule restated in Python
and, slot by slot, the SERIAL harness (run_planning_episodes over the slot's
seed sequence on one INTMCP keyed like the slot) and the oracle.  Bit for bit."""
import functools

import numpy as np
import pytest

from gpu_util import intmcp_state_record, product_config, product_model
from oracle.episode import fhex
from oracle.run import oracle_intmcp_episode
from test_gpu_episode_queue import QueueRecorder, sequential_mean
from test_gpu_intmcp import TEST_CFG
from test_gpu_intmcp_episodes import POP, agent_done_length, check_pair, population

pytestmark = pytest.mark.gpu

S = 8   # simulations per level
EGO, OTHER = "0", "1"
PLANNER_COLUMNS = ("search_depth", "num_sims", "min_value", "max_value")
TIMING = {"time", "search_time", "update_time", "mem_usage"}
# test_reset_pairs_alone: the smallest of 32, 64, 128, 256 simulations per level at
# which a reset pair holds an occupied obs-child map slot after two searches
# (the observed counts are in the comment at the assertion)
RESET_S = 32


def batch(env, B, searches, nesting_level=1, num_sims=S):
    from posggym_baselines_amd.planning import BatchedINTMCP
    return BatchedINTMCP(product_model(env), EGO, product_config(TEST_CFG, num_sims), B, num_sims,
                         searches=searches, nesting_level=nesting_level)


def trees_of(eng):
    return eng.nesting_level + 1 if eng.nesting_level >= 2 else 2


def pair_bytes(eng, b):
    """Everything the getters read of one pair, as bytes."""
    out = []
    for k in range(trees_of(eng)):
        out += [eng.nodes(b, k).tobytes(), eng.stats(b, k).tobytes()]
    out.append(eng.root_belief(b).tobytes())
    out += [a.tobytes() for a in eng.support(b)]
    for k in range(1, eng.nesting_level):
        out += [a.tobytes() for a in eng.mid_support(b, k)]
    return out


# ------------------------------------------------------------ reset_pairs alone
@pytest.mark.timeout(300)
@pytest.mark.parametrize("nesting", [1, 2])
def test_reset_pairs_alone(nesting):
    """70 Driving pairs (two waves, the second 6 pairs wide: its slabs are 6
    nodes wide), an initial update and two searches, then pairs 0, 5, 63 (wave
    0) and 65 (the partial wave) are reset."""
    B, picked = 70, [0, 5, 63, 65]
    bp = batch("Driving-v1", B, 3, nesting, RESET_S)
    eng = bp.engine
    nt = trees_of(eng)
    just_reset = [bytes(s) for s in eng.root_stats()]
    assert len(set(just_reset)) == 1          # (a reset pair's statistics name no pair)
    bp.init_synthetic(1000)
    bp.search()
    bp.search()
    before = [pair_bytes(eng, b) for b in range(B)]
    counts = eng.tree_counts().copy()
    scans = {(b, k): eng.debug_arena_scan(b, k) for b in picked for k in range(nt)}
    print("nesting", nesting, "scan before (blocks, top, map slots):", scans)
    for (b, k), (used, top, slots) in scans.items():
        assert used == top == counts[b, k, 0] > 1, (b, k)
    # the test's own condition: the clear has map slots to empty.  Chosen: 32
    # simulations per level, the smallest of 32, 64, 128, 256; observed on an
    # MI355X: 32 occupied slots in the four pairs at nesting level 1 (7 to 9 per
    # pair, all in tree 1), 63 at nesting level 2 (trees 1 and 2) -- and the same
    # counts at 64, 128 and 256 (the slots are the initial update's children)
    assert any(s[2] > 0 for s in scans.values())
    eng.reset_pairs(picked)
    after_counts = eng.tree_counts()
    stats = eng.root_stats()
    for b in picked:
        for k in range(nt):
            assert eng.debug_arena_scan(b, k) == (1, 1, 0), (b, k)      # node 0 alone
            assert tuple(after_counts[b, k]) == (1, 0, 0), (b, k)
        assert (after_counts[b, nt:] == 0).all()
        assert bytes(stats[b]) == just_reset[b], b
        assert len(eng.root_belief(b)) == 0 and len(eng.support(b)[0]) == 0
    for b in range(B):
        if b not in picked:
            assert pair_bytes(eng, b) == before[b], b
            assert (after_counts[b] == counts[b]).all(), b
    # the guards of the call
    from posggym_baselines_amd._native import POMCP_E_INVALID, PomcpError
    for bad in ([B], [-1], [3, 3]):
        with pytest.raises(PomcpError) as e:
            eng.reset_pairs(bad)
        assert e.value.code == POMCP_E_INVALID
    eng.reset_pairs([])
    bp.close()


# ----------------------------------------------------------- reset, then replay
@pytest.mark.timeout(300)
def test_reset_then_replay_equals_the_whole_context_reset():
    """Pairs 5, 63, 65 of a 70-pair engine: update, search, reset_pairs, update,
    search == a one-pair engine keyed like the pair through update, search,
    reset(), update, search (actions and step records).  Pairs 6 and 64, not
    reset and skipped by the second update, equal the same pairs of an engine
    that searched twice."""
    from posggym_baselines_amd import _native as N
    from posggym_baselines_amd.planning.intmcp import IntmcpEngine
    B, picked, others = 70, [5, 63, 65], [6, 64]
    model, cfg = product_model("Driving-v1"), product_config(TEST_CFG, S)
    first = np.full(B, -1, dtype=np.int32)
    bp = batch("Driving-v1", B, 3)
    eng = bp.engine
    keys = eng.synthetic_obs(1000)
    eng.update(first, keys)
    a1 = eng.search(S)
    rec1 = {b: intmcp_state_record(eng, b, True, a1[b]) for b in picked}
    eng.reset_pairs(picked)
    second = np.full(B, N.INTMCP_SKIP, dtype=np.int32)
    second[picked] = -1
    eng.update(second, keys)
    a2 = eng.search(S)
    rec2 = {b: intmcp_state_record(eng, b, True, a2[b]) for b in picked + others}
    for b in picked:
        one = IntmcpEngine(model, EGO, cfg, num_pairs=1, num_sims=S, searches=3, tree_key_base=b)
        one.update([-1], [keys[b]])
        s1 = one.search(S)
        assert int(s1[0]) == int(a1[b]) and intmcp_state_record(one, 0, True, s1[0]) == rec1[b], b
        one.reset()
        one.update([-1], [keys[b]])
        s2 = one.search(S)
        assert int(s2[0]) == int(a2[b]) and intmcp_state_record(one, 0, True, s2[0]) == rec2[b], b
        assert rec2[b] != rec1[b], b       # (the streams went on: another search)
        one.close()
    bp.close()
    plain = batch("Driving-v1", B, 3)
    plain.engine.update(first, keys)
    plain.engine.search(S)
    p2 = plain.engine.search(S)
    for b in others:
        assert int(p2[b]) == int(a2[b]), b
        assert intmcp_state_record(plain.engine, b, True, p2[b]) == rec2[b], b
    plain.close()


# ------------------------------------------------------------------ whole queues
def restated_schedule(B, lens):
    """The assignment rule replayed on the episodes' lengths: per queue entry
    (slot, ordinal within the slot), and the slots refilled at each step."""
    n = len(lens)
    out = [None] * n
    cur, left, order = list(range(B)), [lens[b] for b in range(B)], [0] * B
    for b in range(B):
        out[b] = (b, 0)
    nxt, refills = B, []
    while any(q >= 0 for q in cur):
        now = set()
        for b in range(B):
            if cur[b] >= 0:
                left[b] -= 1
        for b in range(B):
            if cur[b] >= 0 and left[b] == 0:
                if nxt < n:
                    order[b] += 1
                    cur[b], left[b] = nxt, lens[nxt]
                    out[nxt] = (b, order[b])
                    now.add(b)
                    nxt += 1
                else:
                    cur[b] = -1
        refills.append(now)
    return out, refills


@functools.lru_cache(maxsize=None)
def serial_slot(env, slot, seeds, until, with_pop, nesting=1, max_steps=None):
    """The serial harness over one slot's seed sequence on one INTMCP keyed like
    the slot (tests/test_gpu_intmcp_episodes.py serial_episode, for several
    episodes).  Returns (rows, per-episode steps, per-episode planner statistics
    of the steps that reached PlanningStatTracker, the step record of the very
    last step rebuilt from the planner's device state)."""
    from posggym_baselines_amd.planning import INTMCP, run_planning_episodes
    from posggym_baselines_amd.planning.intmcp import IntmcpEngine
    model = product_model(env)
    cfg = product_config(TEST_CFG, S)
    planner = INTMCP.initialize(model, EGO, cfg, nesting, None)
    planner._engine.close()
    planner._engine = IntmcpEngine(model, EGO, cfg, num_pairs=1, num_sims=S, tree_key_base=slot,
                                   nesting_level=nesting)
    env_model = product_model(env)
    if max_steps is not None:
        env_model.spec = env_model.spec._replace(max_episode_steps=max_steps)
    steps, tracked, last = [], [], {}

    def on_step(t, obs, a, ts):
        if t == 0:
            steps.append([])
            tracked.append(None)
            last["searched"] = True
        else:
            last["searched"] = not last["absorbing"]
        last["absorbing"] = planner.root.is_absorbing
        steps[-1].append((a[EGO], a[OTHER], fhex(ts.rewards[EGO])))
        tracked[-1] = {k: list(planner.stat_tracker._current_stats[k]) for k in PLANNER_COLUMNS}

    rows = run_planning_episodes(planner, env_model, len(seeds), EGO, env_seeds=list(seeds),
                                 until=until, other_agents=population(env_model) if with_pop else None,
                                 on_step=on_step)
    final = intmcp_state_record(planner._engine, 0, last["searched"], steps[-1][-1][0])
    planner.close()
    return rows, steps, tracked, final


@functools.lru_cache(maxsize=None)
def oracle_first(env, seed, b, max_steps, nesting=1):
    return oracle_intmcp_episode(TEST_CFG, S, seed, ego=EGO, tree=b, max_steps=max_steps, env=env,
                                 nesting_level=nesting)


def check_slot(rows, rec, slot, env, seeds, until, with_pop=False, nesting=1, max_steps=None):
    """Every episode of one slot against the serial harness; returns the
    slot's rows and the harness's last step record."""
    mine = sorted((r for r in rows if r["slot"] == slot), key=lambda r: r["slot_order"])
    assert [r["slot_order"] for r in mine] == list(range(len(mine)))
    srows, ssteps, stracked, final = serial_slot(env, slot, tuple(seeds[r["num"]] for r in mine),
                                                 until, with_pop, nesting, max_steps)
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
    return mine, final


def check_first_episode(rows, rec, b, env, seed, until, max_steps, nesting=1):
    """Entry b, slot b's first episode, against the oracle planner with tree key b."""
    trace, records = oracle_first(env, seed, b, max_steps, nesting)
    n = len(trace["steps"])
    if until == "agent_done":
        n = agent_done_length(product_model(env), seed, trace["steps"])
    assert (rows[b]["slot"], rows[b]["slot_order"]) == (b, 0)
    check_pair(rows[b], rec.steps[b], b, seed, trace, records, n)


def run_queue(env, B, N, first, searches, until, nesting=1, with_pop=False, max_steps=None):
    model = product_model(env)
    seeds = list(range(first, first + N))
    bp = batch(env, B, searches, nesting)
    rec = QueueRecorder(B, N)
    rows = bp.run_episode_queue(seeds, until=until, max_steps=max_steps, on_step=rec,
                                other_agents=population(model) if with_pop else None)
    assert len(rows) == N and [r["num"] for r in rows] == list(range(N))
    assert [r["env_seed"] for r in rows] == seeds
    lens = [r["len"] for r in rows]
    assert [len(s) for s in rec.steps] == lens and min(lens) >= 1
    schedule, refills = restated_schedule(B, lens)
    assert [(r["slot"], r["slot_order"]) for r in rows] == schedule
    assert rec.refilled == refills
    assert sorted(rec.retired_at) == list(range(B))       # every slot retired in the end
    # the clear's own account: every refill stored its trees' whole maps and at
    # least node 0's block (plus tree 1's first child's), at most the arenas
    caps, nt = bp.engine.capacities, trees_of(bp.engine)
    cleared = bp.engine.debug_queue_cleared_bytes()
    assert (N - B) * (nt * (caps.hash_slots * 16 + 320) + 320) <= cleared
    assert cleared <= (N - B) * nt * (caps.hash_slots * 16 + caps.max_nodes * 320)
    return bp, rec, rows, seeds


@pytest.mark.timeout(600)
@pytest.mark.parametrize("until", ["all_done", "agent_done"])
def test_driving_queue_equals_the_rule_the_serial_harness_and_the_oracle(until):
    """70 slots (two waves, the second with 6 pairs), 200 entries."""
    from posggym_baselines_amd.planning.episodes import EPISODE_RESULT_HEADS
    env, B, N, first, max_steps = "Driving-v1", 70, 200, 3000, 50
    bp, rec, rows, seeds = run_queue(env, B, N, first, max_steps, until)
    bp.close()
    assert all(list(r) == EPISODE_RESULT_HEADS + ["env_seed", "slot", "slot_order"] for r in rows)
    played = np.bincount([r["slot"] for r in rows], minlength=B)
    busy = [b for b in range(B) if played[b] >= 3]
    assert busy                                            # some slot played three episodes
    chosen = sorted(set([0, 63, 64, 69] + busy))
    print(until, "slots checked:", len(chosen), "episodes:", int(played[chosen].sum()))
    for b in chosen:
        mine, _ = check_slot(rows, rec, b, env, seeds, until)
        assert len(mine) == played[b]
        check_first_episode(rows, rec, b, env, seeds[b], until, max_steps)
    # a refill inside a wave whose other pairs are mid-episode, in both waves
    for wave in (set(range(0, 64)), set(range(64, 70))):
        assert any(r & wave and m & wave for r, m in zip(rec.refilled, rec.mid)), wave


@pytest.mark.timeout(600)
def test_pursuit_evasion_queue_against_a_population():
    """24 slots, 60 entries, until agent_done, the two-policy population."""
    env, B, N, first, max_steps = "PursuitEvasion-v1", 24, 60, 2000, 100
    bp, rec, rows, seeds = run_queue(env, B, N, first, max_steps, "agent_done", with_pop=True)
    bp.close()
    assert {r["other_policy_id"] for r in rows} == {p for p, _ in POP}
    played = np.bincount([r["slot"] for r in rows], minlength=B)
    busy = [b for b in range(B) if played[b] >= 3]
    assert busy
    seen = set()
    for b in sorted(set([0, 23] + busy)):
        mine, _ = check_slot(rows, rec, b, env, seeds, "agent_done", with_pop=True)
        seen |= {r["other_policy_id"] for r in mine}
    assert len(seen) == 2                                  # both policies were compared


@pytest.mark.timeout(600)
@pytest.mark.parametrize("nesting", [0, 2])
def test_other_nesting_levels(nesting):
    """16 slots, 40 entries: nesting level 0 (the planner's tree is tree 1) and
    2 (three trees per pair cleared)."""
    env, B, N, first, max_steps = "Driving-v1", 16, 40, 5000, 50
    bp, rec, rows, seeds = run_queue(env, B, N, first, max_steps, "all_done", nesting)
    bp.close()
    played = np.bincount([r["slot"] for r in rows], minlength=B)
    most = int(np.argmax(played))
    assert played[most] >= 2
    for b in sorted({0, 15, most}):
        check_slot(rows, rec, b, env, seeds, "all_done", nesting=nesting)
        check_first_episode(rows, rec, b, env, seeds[b], "all_done", max_steps, nesting)


@pytest.mark.timeout(600)
def test_1030_pairs_two_steps_refill_forty_slots():
    """The lane-per-pair update (more than 1,024 pairs).  max_steps = 2 ends every
    first episode in the batch's second step (of the oracle's 1,030 episodes on
    env seeds 7000.. none ends after one step, tests/test_gpu_intmcp_episodes.py),
    so slots 0..39 take the entries 1030..1069 and the other 990 retire."""
    env, B, N, first, max_steps = "Driving-v1", 1030, 1070, 7000, 2
    lives = []
    seeds = list(range(first, first + N))
    bp = batch(env, B, max_steps)
    step = bp.engine.episodes_step

    def counted(num_sims):
        lives.append(step(num_sims))
        return lives[-1]

    bp.engine.episodes_step = counted
    rec = QueueRecorder(B, N)
    rows = bp.run_episode_queue(seeds, until="all_done", max_steps=max_steps, on_step=rec)
    bp.close()
    lens = [r["len"] for r in rows]
    assert lens[:B] == [2] * B
    schedule, refills = restated_schedule(B, lens)
    assert [(r["slot"], r["slot_order"]) for r in rows] == schedule
    assert rec.refilled == refills and refills[1] == set(range(40))
    assert [(r["slot"], r["slot_order"]) for r in rows[B:]] == [(b, 1) for b in range(40)]
    # the second episodes' lengths, from the serial harness on all forty slots
    second = []
    for b in range(40):
        srows, _, _, _ = serial_slot(env, b, (seeds[b], seeds[B + b]), "all_done", False, 1, max_steps)
        second.append(srows[1]["len"])
    assert lens[B:] == second
    playing_on = sum(n == 2 for n in second)
    assert lives == [B, 40, playing_on] + ([0] if playing_on else [])
    for b in (0, 39, 40, 1029):
        check_slot(rows, rec, b, env, seeds, "all_done", max_steps=max_steps)
        check_first_episode(rows, rec, b, env, seeds[b], "all_done", max_steps)


@pytest.mark.timeout(600)
def test_after_the_call_and_a_replay_on_a_fresh_engine():
    """8 slots, 20 entries.  When the call returns every slot's getters read what
    they read after its last step (the retired slots' pairs are restored), and a
    fresh engine replays the queue."""
    env, B, N, first, max_steps = "Driving-v1", 8, 20, 3100, 50
    bp, rec, rows, seeds = run_queue(env, B, N, first, max_steps, "all_done")
    parked = [bytes(s) for s in bp.engine.root_stats()]
    searched = 0
    for b in range(B):
        mine, final = check_slot(rows, rec, b, env, seeds, "all_done")
        last = rec.steps[mine[-1]["num"]][-1]
        assert intmcp_state_record(bp.engine, b, final["searched"], last[0]) == final, b
        searched += final["searched"]
    assert searched >= 1      # (a last step without a search has only its action to compare)
    # the batch has ended: its results again change nothing
    bp.engine.episodes_results()
    assert [bytes(s) for s in bp.engine.root_stats()] == parked
    bp.close()
    other, rec2, rows2, _ = run_queue(env, B, N, first, max_steps, "all_done")
    other.close()
    assert rec2.steps == rec.steps
    for r, r2 in zip(rows, rows2):
        assert all(fhex(float(r[k])) == fhex(float(r2[k])) for k in r if k not in TIMING)


@pytest.mark.timeout(120)
def test_guards_raise_before_any_launch():
    from posggym_baselines_amd._native import POMCP_E_STATE, PomcpError
    bp = batch("Driving-v1", 4, 1)
    with pytest.raises(ValueError, match="searches=50"):
        bp.run_episode_queue(range(8))
    with pytest.raises(PomcpError):   # nothing was launched: no batch of episodes exists
        bp.episode_states()
    bp.close()
    bp = batch("Driving-v1", 4, 50)
    with pytest.raises(ValueError, match="at least 4"):
        bp.run_episode_queue([1, 2, 3])
    with pytest.raises(ValueError, match="until"):
        bp.run_episode_queue(range(8), until="never")
    with pytest.raises(ValueError, match="max_steps"):
        bp.run_episode_queue(range(8), max_steps=51)
    with pytest.raises(ValueError, match="max_steps"):
        bp.run_episode_queue(range(8), max_steps=0)
    with pytest.raises(ValueError, match="1 to 8"):
        bp.run_episode_queue(range(8), other_agents=[])
    with pytest.raises(TypeError):
        bp.run_episode_queue(range(8), belief_acc=["state"])
    with pytest.raises(PomcpError):
        bp.episode_states()
    with pytest.raises(PomcpError):
        bp.episode_queue_slots()
    # reset_pairs is refused while a batch of episodes is active
    gamma = bp.engine.config.discount
    bp.engine.episodes_queue_begin(list(range(8)), [gamma ** t for t in range(50)], 50, "all_done")
    with pytest.raises(PomcpError) as e:
        bp.engine.reset_pairs([0])
    assert e.value.code == POMCP_E_STATE
    bp.close()
