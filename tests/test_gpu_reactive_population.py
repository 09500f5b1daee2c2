"""Batched episodes against a population with state-reactive members (the
Driving-v1 shortest-path agents; k_episode_step / k_group_episode_step and the
queue forms through csrc/episode_step.h with pomcp_policy_kinds): every entry
point that shares the episode step against the SERIAL harness
(run_planning_episodes with other_agents= on one planner keyed like the tree,
slot or group), bit for bit."""
import functools

import pytest

from gpu_util import product_config, product_model
from oracle.episode import fhex
from root_parallel_util import TEST_CFG
from test_gpu_episode_group_queue import GroupQueueRecorder
from test_gpu_episode_groups import Recorder as GroupRecorder
from test_gpu_episode_population import Recorder, check_tree, potmmcp_setup, serial_row, swap_engine
from test_gpu_episode_queue import QueueRecorder, restated_schedule

pytestmark = pytest.mark.gpu

ENV, EGO, OTHER, MAX_STEPS = "Driving-v1", "0", "1", 50
FIVE = [f"Driving-v1/A{g}Shortestpath-v0" for g in (0, 40, 60, 80, 100)]
FIXED = ("o_left", [0.1, 0.05, 0.5, 0.3, 0.05])


def five(model, other=OTHER):
    from posggym_baselines_amd.planning.policies import ShortestPathPolicy
    return [ShortestPathPolicy.from_id(model, other, pid) for pid in FIVE]


def mixed(model, other=OTHER):
    """The reactive population of the small cases: A100, A0 and a fixed one."""
    from posggym_baselines_amd.planning.policies import FixedDistributionPolicy, ShortestPathPolicy
    return [ShortestPathPolicy.from_id(model, other, FIVE[4]),
            ShortestPathPolicy.from_id(model, other, FIVE[0]),
            FixedDistributionPolicy(model, other, *FIXED)]


@functools.lru_cache(maxsize=None)
def serial(K, S, key_base, seeds, until, pop_name, ego=EGO):
    """The serial harness over `seeds` on one plain planner of K replicas keyed
    (seed, key_base + k); returns (rows, per-episode steps)."""
    from posggym_baselines_amd.planning import POMCP, RandomSearchPolicy, run_planning_episodes
    from posggym_baselines_amd.planning.engine import PomcpEngine
    model = product_model(ENV)
    other = "1" if ego == "0" else "0"
    cfg = product_config(dict(TEST_CFG), K * S)
    cfg.root_parallel = K
    planner = POMCP(model, ego, cfg, RandomSearchPolicy(model, ego))
    planner._engine.close()
    planner._engine = PomcpEngine(model, ego, cfg, num_trees=K, num_sims=S, tree_key_base=key_base,
                                  type_policies=planner.type_policies)
    pop = {"five": five, "mixed": mixed}[pop_name](model, other)
    steps = []

    def on_step(t, obs, a, ts):
        if t == 0:
            steps.append([])
        steps[-1].append((a[ego], a[other], fhex(ts.rewards[ego])))

    rows = run_planning_episodes(planner, product_model(ENV), len(seeds), ego,
                                 env_seeds=list(seeds), until=until, other_agents=pop,
                                 on_step=on_step)
    planner.close()
    return rows, steps


def same_episode(row, steps, srow, ssteps, where):
    assert row["other_policy_id"] == srow["other_policy_id"], where
    assert steps == ssteps, where
    assert row["len"] == srow["len"] == len(ssteps), where
    assert fhex(row["return"]) == fhex(srow["return"]), where
    assert fhex(row["discounted_return"]) == fhex(srow["discounted_return"]), where


def reactive_actions_follow_the_state(bp_model, pop, row, steps, seed, ego=EGO):
    """The recorded episode replayed on the host model: a reactive member's
    action at every step is the Python rule's on the state before the step."""
    other = "1" if ego == "0" else "0"
    pol = next(p for p in pop if p.policy_id == row["other_policy_id"])
    bp_model.seed(seed)
    state = bp_model.sample_initial_state()
    for a_ego, a_oth, _ in steps:
        assert a_oth == pol.action_from_state(state)
        state = bp_model.step(state, {ego: a_ego, other: a_oth}).state


# ----------------------------------------- plain POMCP against the five agents
def test_plain_batch_against_the_five_shortest_path_agents():
    """64 trees of the plain planner, one episode each against the population
    of the reference's Driving experiments, until the planning agent is done."""
    from posggym_baselines_amd.planning import BatchedPOMCP
    B, S, first, until = 64, 16, 3000, "agent_done"
    model = product_model(ENV)
    pop = five(model)
    bp = BatchedPOMCP(model, EGO, product_config(TEST_CFG, S), B, S, searches=MAX_STEPS, reroot=True)
    rec = Recorder(B, acc=False)
    rows = bp.run_episodes(range(first, first + B), until=until, other_agents=pop, on_step=rec)
    pops = bp.engine.episodes_pop_states()
    bp.close()
    assert (pops["mixture_index"] == -1).all()
    assert {int(k) for k in pops["policy_index"]} == {0, 1, 2, 3, 4}
    host = product_model(ENV)
    for b in range(B):
        srows, ssteps = serial(1, S, b, (first + b,), until, "five")
        same_episode(rows[b], rec.steps[b], srows[0], ssteps[0], b)
        assert rows[b]["other_policy_id"] == FIVE[int(pops["policy_index"][b])]
        reactive_actions_follow_the_state(host, pop, rows[b], rec.steps[b], first + b)
    lens = [r["len"] for r in rows]
    assert min(lens) < max(lens)
    others = {s[1] for b in range(B) for s in rec.steps[b]}
    assert {0, 1, 3, 4} <= others        # it accelerates, turns both ways and coasts
    # a cautious agent braked for the planner's vehicle at least once
    assert any(s[1] == 2 for b in range(B) for s in rec.steps[b])


# ------------------------------ a type-based planner, belief accuracy on device
DRV_B = 70
DRV_SUBSET = [0, 1, 2, 3, 4, 5, 64, 65, 66, 67, 68, 69]
STATS = ["policy", "state"]


def modelled_and_reactive(model, mix):
    """The planner's own (fixed) policies and two shortest-path agents it does
    not model."""
    from posggym_baselines_amd.planning.policies import ShortestPathPolicy
    return [ShortestPathPolicy.from_id(model, OTHER, FIVE[4])] + list(mix.policies.values()) + \
        [ShortestPathPolicy.from_id(model, OTHER, FIVE[0])]


@functools.lru_cache(maxsize=None)
def potmmcp_serial():
    from posggym_baselines_amd.planning import POTMMCP
    data, model, others, meta, mix, cfg, _ = potmmcp_setup()
    out = {}
    for b in DRV_SUBSET:
        planner = POTMMCP(model, EGO, cfg, others, meta)
        swap_engine(planner, model, cfg, data["num_sims"], b)
        out[b] = serial_row(planner, ENV, 3000 + b, modelled_and_reactive(model, mix), STATS,
                            "all_done")
        planner._engine.close()
    return out


def test_type_based_batch_with_unmodelled_reactive_members_and_belief_accuracy():
    """70 trees (two search waves, one partial) of the POTMMCP planner of
    tests/test_gpu_episode_population.py: its mixture holds fixed policies, the
    population adds two reactive agents it does not model, whose policy
    accuracy is exactly 0.0."""
    from posggym_baselines_amd.planning import BatchedPOMCP
    from posggym_baselines_amd.planning.potmmcp import type_policy_tables
    data, model, others, meta, mix, cfg, _ = potmmcp_setup()
    pop = modelled_and_reactive(model, mix)
    B, S = DRV_B, data["num_sims"]
    bp = BatchedPOMCP(model, EGO, cfg, B, S, searches=MAX_STEPS, reroot=True,
                      type_policies=type_policy_tables(model, EGO, meta, mix),
                      other_policy_ids=list(mix.policies))
    rec = Recorder(B)
    rows = bp.run_episodes(range(3000, 3000 + B), until="all_done", belief_acc=STATS,
                           track_per_step=True, other_agents=pop, on_step=rec)
    pops = bp.engine.episodes_pop_states()
    assert not bp.episode_belief_acc()["error"].any()
    bp.close()
    serial_rows = potmmcp_serial()
    n = len(pop)
    assert {int(pops["policy_index"][b]) for b in DRV_SUBSET} >= {0, n - 1}
    assert any(0 < int(pops["policy_index"][b]) < n - 1 for b in DRV_SUBSET)
    for b in DRV_SUBSET:
        srow, ssteps = serial_rows[b]
        check_tree(rows[b], rec.steps[b], srow, ssteps, STATS, MAX_STEPS, b)
    lens = [r["len"] for r in rows]
    assert min(lens) < max(lens)
    vals = [rows[b][f"belief_policy_acc_{t}"] for b in range(B) for t in range(lens[b])]
    assert any(0.0 < v < 1.0 for v in vals)
    strangers = [b for b in range(B) if int(pops["policy_index"][b]) in (0, n - 1)]
    assert strangers and all(int(pops["mixture_index"][b]) == -1 for b in strangers)
    for b in strangers:
        assert rows[b]["other_policy_id"] in (FIVE[4], FIVE[0])
        assert rows[b]["belief_policy_acc"] == 0.0
        assert all(rows[b][f"belief_policy_acc_{t}"] == 0.0 for t in range(lens[b]))
    assert any(rows[b]["belief_state_acc"] > 0.0 for b in strangers)


# ------------------------------------------- the shared step's other callers
def test_episode_queue_against_the_reactive_population():
    """8 slots, 24 seeds."""
    from posggym_baselines_amd.planning import BatchedPOMCP
    B, N, S, first, until = 8, 24, 16, 3100, "all_done"
    seeds = list(range(first, first + N))
    model = product_model(ENV)
    bp = BatchedPOMCP(model, EGO, product_config(TEST_CFG, S), B, S, searches=MAX_STEPS, reroot=True)
    rec = QueueRecorder(B, N)
    rows = bp.run_episode_queue(seeds, until=until, other_agents=mixed(model), on_step=rec)
    bp.close()
    lens = [r["len"] for r in rows]
    assert len(rows) == N and [len(s) for s in rec.steps] == lens
    assert [(r["slot"], r["slot_order"]) for r in rows] == restated_schedule(B, lens)
    assert {r["other_policy_id"] for r in rows} == {FIVE[4], FIVE[0], FIXED[0]}
    for b in range(B):
        mine = sorted((r for r in rows if r["slot"] == b), key=lambda r: r["slot_order"])
        srows, ssteps = serial(1, S, b, tuple(seeds[r["num"]] for r in mine), until, "mixed")
        for r, sr, ss in zip(mine, srows, ssteps):
            same_episode(r, rec.steps[r["num"]], sr, ss, (b, r["num"]))
    assert any(r["slot_order"] > 0 and r["other_policy_id"] != FIXED[0] for r in rows)


def test_root_parallel_groups_against_the_reactive_population():
    """12 trees = 4 planners of 3 replicas."""
    from posggym_baselines_amd.planning import BatchedPOMCP
    K, G, S, first, until = 3, 4, 8, 3200, "all_done"
    model = product_model(ENV)
    bp = BatchedPOMCP(model, EGO, product_config(TEST_CFG, S), G * K, S, searches=MAX_STEPS,
                      reroot=True)
    rec = GroupRecorder(G)
    rows = bp.run_episodes(range(first, first + G), until=until, other_agents=mixed(model),
                           on_step=rec, root_parallel=K)
    bp.close()
    for g in range(G):
        srows, ssteps = serial(K, S, g * K, (first + g,), until, "mixed")
        same_episode(rows[g], rec.steps[g], srows[0], ssteps[0], g)
    assert any(r["other_policy_id"] != FIXED[0] for r in rows)


def test_planner_queue_against_the_reactive_population():
    """12 trees = 4 planners of 3 replicas, 10 seeds, the other agent planning."""
    from posggym_baselines_amd.planning import BatchedPOMCP
    K, G, N, S, first, until, ego = 3, 4, 10, 8, 3300, "agent_done", "1"
    seeds = list(range(first, first + N))
    model = product_model(ENV)
    bp = BatchedPOMCP(model, ego, product_config(TEST_CFG, S), G * K, S, searches=MAX_STEPS,
                      reroot=True)
    rec = GroupQueueRecorder(G, N)
    rows = bp.run_planner_queue(seeds, root_parallel=K, until=until,
                                other_agents=mixed(model, "0"), on_step=rec)
    bp.close()
    lens = [r["len"] for r in rows]
    assert len(rows) == N and [len(s) for s in rec.steps] == lens
    assert [(r["slot"], r["slot_order"]) for r in rows] == restated_schedule(G, lens)
    for g in range(G):
        mine = sorted((r for r in rows if r["slot"] == g), key=lambda r: r["slot_order"])
        srows, ssteps = serial(K, S, g * K, tuple(seeds[r["num"]] for r in mine), until, "mixed",
                               ego=ego)
        for r, sr, ss in zip(mine, srows, ssteps):
            same_episode(r, rec.steps[r["num"]], sr, ss, (g, r["num"]))
    assert any(r["other_policy_id"] != FIXED[0] for r in rows)
    assert any(r["slot_order"] > 0 for r in rows)


# -------------------------------------------------------------------- guards
def test_guards_raise_before_any_launch_and_fixed_populations_play_on():
    from posggym_baselines_amd._native import PomcpError
    from posggym_baselines_amd.planning import BatchedINTMCP, BatchedPOMCP
    from posggym_baselines_amd.planning.policies import FixedDistributionPolicy
    S = 8
    drv, pe = product_model(ENV), product_model("PursuitEvasion-v1")
    bp = BatchedPOMCP(pe, EGO, product_config(TEST_CFG, S), 4, S, searches=100, reroot=True)
    with pytest.raises(NotImplementedError, match="PursuitEvasion"):
        bp.run_episodes(other_agents=mixed(drv))
    with pytest.raises(PomcpError):       # nothing was launched: no batch of episodes exists
        bp.episode_states()
    # the C ABI refuses the kind as well, and wants a population first
    SP = 1
    bp.engine.episodes_set_population([[0.25] * 4])
    with pytest.raises(PomcpError, match="UNSUPPORTED"):
        bp.engine.episodes_set_population_kinds([(SP, 1, 3)])
    bp.engine.episodes_set_population(None)
    with pytest.raises(PomcpError, match="STATE"):
        bp.engine.episodes_set_population_kinds([(SP, 1, 3)])
    bp.close()
    bp = BatchedPOMCP(drv, EGO, product_config(TEST_CFG, S), 4, S, searches=MAX_STEPS, reroot=True)
    bp.engine.episodes_set_population([[0.2] * 5])
    for bad in ((2, 0, 3), (SP, 16, 3), (SP, 1, 4), (SP, -1, 3)):
        with pytest.raises(PomcpError, match="INVALID"):
            bp.engine.episodes_set_population_kinds([bad])
    with pytest.raises(ValueError, match="planning agent"):
        bp.run_episodes(other_agents=mixed(drv, EGO))
    # kinds last one population: the next one is all fixed again, and its
    # members draw from their distributions as PopulationAgents does
    from posggym_baselines_amd.planning import PopulationAgents
    seeds = list(range(3400, 3404))
    rows_r = bp.run_episodes(seeds, other_agents=mixed(drv))
    assert {r["other_policy_id"] for r in rows_r} <= {FIVE[4], FIVE[0], FIXED[0]}
    fixed = [FixedDistributionPolicy(drv, OTHER, pid, FIXED[1]) for pid in ("a", "b", "c")]
    rec = Recorder(4, acc=False)
    rows_f = bp.run_episodes(seeds, other_agents=fixed, on_step=rec)
    bp.close()
    for b, seed in enumerate(seeds):
        agents = PopulationAgents(drv, seed, fixed)
        agents.reset()
        assert rows_f[b]["other_policy_id"] == agents.policy_id
        assert [s[1] for s in rec.steps[b]] == [agents.act(OTHER) for _ in rec.steps[b]], b
    # I-NTMCP plays against fixed populations only
    im = BatchedINTMCP(drv, EGO, product_config(TEST_CFG, S), 2, S, searches=MAX_STEPS,
                       nesting_level=1)
    with pytest.raises(NotImplementedError, match="I-NTMCP"):
        im.run_episodes(other_agents=mixed(drv))
    with pytest.raises(NotImplementedError, match="I-NTMCP"):
        im.run_episode_queue(range(4), other_agents=mixed(drv))
    im.close()
