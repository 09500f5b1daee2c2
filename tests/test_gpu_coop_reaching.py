"""CooperativeReaching-v0 on the GPU (k_search<EnvCoopReaching, ...> and every
kernel the environment reaches through the dispatch): the reference goldens of
tests/golden/coop_reaching record for record in both lane modes, the device
step against the host twin, size-independent properties of a large batch, and
the batched episode entry points against the serial harness with the
heuristic agents as the population, bit for bit."""
import ctypes as C
import functools
import math
import sys

import numpy as np
import pytest

from golden_util import GOLDEN, load
from gpu_util import product_config, stats_record
from oracle.episode import ENV_TREE_BASE, fhex
from oracle.rng import Streams
from test_gpu_episode_group_queue import GroupQueueRecorder
from test_gpu_episode_groups import Recorder as GroupRecorder
from test_gpu_episode_population import Recorder, check_tree, swap_engine
from test_gpu_episode_queue import QueueRecorder, restated_schedule
from test_gpu_potmmcp import _record

sys.path.insert(0, GOLDEN)
from coop_reaching_model import CooperativeReachingModel as PyModel, run_episode  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = ["pomcp_ucb", "pomcp_pucb_ego1_od1", "pomcp_deep", "ipomcp_pucb_mix", "ipomcp_reinv",
         "potmmcp_ucb_ego1_od2", "mcts_fixed_other"]
H = [f"CooperativeReaching-v0/H{k}-v0" for k in range(1, 6)]
EGO, OTHER, MAX_STEPS = "0", "1", 50
TEST_CFG = dict(discount=0.95, search_time_limit=0.1, c=math.sqrt(2), truncated=False,
                action_selection="ucb", pucb_exploration_fraction=0.25, known_bounds=None,
                step_limit=None, epsilon=0.92, seed=0, state_belief_only=True)


def product(size=5, obs_distance=None):
    from posggym_baselines_amd.envs import CooperativeReachingModel
    return CooperativeReachingModel(size=size, obs_distance=obs_distance)


def other_policy(model, other, pid, row):
    from posggym_baselines_amd.planning.policies import FixedDistributionPolicy, GoalHeuristicPolicy
    if row is None:
        return GoalHeuristicPolicy.from_id(model, other, pid)
    return FixedDistributionPolicy(model, other, pid, row)


def make_planner(data, cfg, model):
    """The drop-in planner of a golden case, built from the build's policies."""
    from posggym_baselines_amd.planning import (IPOMCP, MCTS, POMCP, POTMMCP,
                                                OtherAgentMixturePolicy, POTMMCPMetaPolicy,
                                                RandomSearchPolicy)
    from posggym_baselines_amd.planning.policies import FixedDistributionPolicy
    ego, spec = data["ego"], data["spec"]
    other = [i for i in model.possible_agents if i != ego][0]
    config = product_config(cfg, data["num_sims"])
    search = RandomSearchPolicy(model, ego)
    if data["planner"] == "POMCP":
        return POMCP(model, ego, config, search)
    if data["planner"] == "POTMMCP":
        ego_pols = {k: FixedDistributionPolicy(model, ego, k, v) for k, v in spec["ego"].items()}
        mix = OtherAgentMixturePolicy(model, other, {
            k: other_policy(model, other, k, v) for k, v in spec["other"].items()})
        return POTMMCP(model, ego, config, {other: mix},
                       POTMMCPMetaPolicy(model, ego, ego_pols, spec["meta"]))
    o = spec["other"]
    if o["kind"] == "fixed":
        return MCTS(model, ego, config, {other: FixedDistributionPolicy(model, other, "fixed",
                                                                        o["probs"])}, search)
    mix = OtherAgentMixturePolicy(model, other, {
        k: other_policy(model, other, k, v) for k, v in o["policies"].items()})
    return IPOMCP(model, ego, config, {other: mix}, search)


# -------------------------------------------------------------- golden replay
@pytest.mark.parametrize("mode", ["lane", "lane_eager"])
@pytest.mark.parametrize("case", CASES)
def test_reference_goldens_replay_bit_for_bit(case, mode, monkeypatch):
    monkeypatch.setenv("POMCP_SEARCH_KERNEL", "lane")
    monkeypatch.setenv("POMCP_DEFER_CUTOFF", "0" if mode == "lane_eager" else "1")
    data = load("coop_reaching/" + case)
    ego = data["ego"]
    for ep in data["episodes"]:
        model = product(data["size"], data["obs_distance"])
        planner = make_planner(data, ep["config"], model)
        typed = planner.type_policies is not None
        assert typed == (data["planner"] != "POMCP")
        if data["spec"] is not None and data["spec"]["other"].get("kind") != "fixed":
            assert planner._engine.other_reactive
        planner.reset()
        A = model.action_spaces[ego].n
        records = []

        def step(obs):
            searched = not planner.root.is_absorbing
            a = planner.step(model.obs_key(obs))
            n = planner.step_statistics["num_sims"] if searched else 0
            if not searched:
                records.append({"searched": False, "action": int(a)})
            elif typed:
                records.append(_record(planner, planner._engine, 0, A, a, n))
            else:
                rec = stats_record(planner._engine.root_stats()[0], A, True, a,
                                   planner.root_belief())
                rec["num_sims"] = int(n)
                records.append(rec)
            return a

        env = PyModel(Streams(ep["env_seed"], ENV_TREE_BASE), data["size"], data["obs_distance"])
        trace = run_episode(env, step, ego, data["other_agent"], data["max_steps"])
        trace["env_seed"] = ep["env_seed"]
        planner.close()
        assert len(records) == len(ep["records"]), case
        for t, (got, exp) in enumerate(zip(records, ep["records"])):
            assert got == exp, f"{case} env_seed {ep['env_seed']} step {t}"
        assert trace == ep["trace"]


def test_six_first_step_trees_in_one_launch():
    """Six planners in one engine (tree keys 0..5) searched by one launch: each
    tree's first step equals the reference POTMMCP under that key."""
    from posggym_baselines_amd.planning.engine import PomcpEngine
    from posggym_baselines_amd.planning.potmmcp import type_policy_tables
    data = load("coop_reaching/potmmcp_ucb_ego1_od2")
    ego, ep = data["ego"], data["episodes"][0]
    model = product(data["size"], data["obs_distance"])
    from posggym_baselines_amd.planning import OtherAgentMixturePolicy, POTMMCPMetaPolicy
    from posggym_baselines_amd.planning.policies import FixedDistributionPolicy
    spec, other = data["spec"], "0"
    ego_pols = {k: FixedDistributionPolicy(model, ego, k, v) for k, v in spec["ego"].items()}
    mix = OtherAgentMixturePolicy(model, other, {
        k: other_policy(model, other, k, v) for k, v in spec["other"].items()})
    meta = POTMMCPMetaPolicy(model, ego, ego_pols, spec["meta"])
    B, S = len(data["trees"]), data["num_sims"]
    eng = PomcpEngine(model, ego, product_config(ep["config"], S), num_trees=B, num_sims=S,
                      searches=4, type_policies=type_policy_tables(model, ego, meta, mix))
    eng.reset()
    env = PyModel(Streams(ep["env_seed"], ENV_TREE_BASE), data["size"], data["obs_distance"])
    key = env.pack_obs(env.sample_initial_obs(env.sample_initial_state())[ego])
    assert key == data["trees"][0]["trace"]["steps"][0]["obs"]
    eng.update(np.full(B, -1, dtype=np.int32), np.full(B, key, dtype=np.uint64))
    eng.search(S)
    A = model.action_spaces[ego].n
    for k, tr in enumerate(data["trees"]):
        got = _record(None, eng, k, A, eng.root_stats()[k].action, S)
        assert got == tr["records"][0], f"tree {k}"
    eng.close()


# ------------------------------------------------------------- kernel choice
def test_wave_kernel_is_unsupported_and_small_batches_run_the_lane_kernel():
    from posggym_baselines_amd import _native as N
    from posggym_baselines_amd.planning import BatchedPOMCP
    bp = BatchedPOMCP(product(), EGO, product_config(TEST_CFG, 16), 4, 16)
    lib, ctx = bp.engine._lib, bp.engine._ctx
    assert lib.pomcp_search_kernel_used(ctx) == N.SEARCH_LANE      # (4 trees: the wave's range)
    assert lib.pomcp_set_search_kernel(ctx, N.SEARCH_WAVE) == N.POMCP_E_UNSUPPORTED
    assert b"CooperativeReaching" in lib.pomcp_last_error(ctx)
    assert lib.pomcp_set_search_kernel(ctx, N.SEARCH_LANE) == 0
    assert lib.pomcp_set_search_kernel(ctx, N.SEARCH_AUTO) == 0
    bp.init_synthetic(7)
    bp.search()
    assert all(s.error == 0 and s.num_sims == 16 for s in bp.engine.root_stats())
    bp.close()


# ------------------------------------------------------------- env self-test
_PU32 = C.POINTER(C.c_uint32)


@pytest.mark.parametrize("size,obs_distance", [(5, None), (8, 1), (3, 0)])
def test_device_step_equals_the_host_twin(size, obs_distance):
    """k_env_selftest<EnvCoopReaching> on the states of 64 seeded random
    trajectories x every joint action, for both egos."""
    from posggym_baselines_amd import _native as N
    from posggym_baselines_amd.planning import BatchedPOMCP
    model = product(size, obs_distance)
    rng = np.random.default_rng(size)
    states = []
    for seed in range(64):
        model.seed(seed)
        s = model.sample_initial_state()
        for _ in range(MAX_STEPS):
            states.append(s)
            ts = model.step(s, {"0": int(rng.integers(5)), "1": int(rng.integers(5))})
            if ts.all_done:
                states.append(ts.state)      # a terminal state steps like any other
                break
            s = ts.state
    states = sorted(set(states))
    cases = np.array([(s0, s1, a0, a1, 0) for (s0, s1) in states for a0 in range(5)
                      for a1 in range(5)], dtype=np.uint32)
    assert len(cases) > 5000
    for ego in ("0", "1"):
        bp = BatchedPOMCP(model, ego, product_config(TEST_CFG, 16), 4, 16)
        out = np.zeros((len(cases), 8), dtype=np.uint32)
        rc = N.load().pomcp_debug_env_step(bp.engine._ctx, cases.ctypes.data_as(_PU32), len(cases),
                                           out.ctypes.data_as(_PU32))
        bp.close()
        assert rc == 0
        ref = np.zeros_like(out)
        oth = "1" if ego == "0" else "0"
        for i, (s0, s1, ae, ao, _) in enumerate(cases.tolist()):
            ts = model.step((s0, s1), {ego: ae, oth: ao})
            r = int(np.float64(ts.rewards[ego]).view(np.uint64))
            key = model.obs_key(ts.observations[ego])
            ref[i] = (ts.state[0], ts.state[1], r & 0xFFFFFFFF, r >> 32,
                      int(ts.terminations[ego]), key & 0xFFFFFFFF, key >> 32, 0)
        bad = np.flatnonzero((out != ref).any(axis=1))
        assert len(bad) == 0, (ego, len(bad), [(cases[i].tolist(), out[i].tolist(), ref[i].tolist())
                                               for i in bad[:5]])
        assert ref[:, 4].any() and (ref[:, 2:4] != 0).any()      # terminal steps and rewards


# --------------------------------------------------- size-independent properties
@pytest.mark.parametrize("mode", ["lane", "lane_eager"])
def test_many_trees_properties_over_two_steps(mode, monkeypatch):
    """2,048 trees x 64 simulations under partial observation, a search, a
    re-root and a second search: visit conservation, Welford totals, action =
    argmax value, and a restore that reproduces the first search bit for bit."""
    from posggym_baselines_amd.planning import BatchedPOMCP
    monkeypatch.setenv("POMCP_DEFER_CUTOFF", "0" if mode == "lane_eager" else "1")
    B, S = 2048, 64
    bp = BatchedPOMCP(product(5, 1), EGO, product_config(TEST_CFG, S), B, S, searches=3,
                      reroot=True)
    bp.init_synthetic(5000)

    def check(stats, actions, trees, first):
        for b in trees:
            st = stats[b]
            v = np.array(st.child_visits[:5])
            assert st.error == 0 and st.num_sims == S
            if first:
                assert st.root_visits == S and v.sum() == S
            else:                    # the kept subtree's visits stay
                assert st.root_visits >= S and S - 1 <= v.sum() <= st.root_visits
            vals = np.array(st.child_values[:5])
            tot = np.array(st.child_totals[:5])
            assert np.allclose(vals[v > 0], tot[v > 0] / v[v > 0], rtol=1e-9, atol=1e-12)
            assert vals[actions[b]] == vals.max()

    key = lambda stats: [(s.action, tuple(s.child_visits), tuple(s.child_values)) for s in stats]
    actions = bp.search()
    check(bp.engine.root_stats(), actions, range(B), True)
    first = key(bp.engine.root_stats())
    assert len({f[0] for f in first}) > 1
    obs = bp.engine.synthetic_step(5000, actions)
    absorbing = bp.engine.update(actions, obs)
    live = np.flatnonzero(~absorbing)
    assert len(live) > B // 2
    actions2 = bp.search()
    check(bp.engine.root_stats(), actions2, live, False)
    bp.restore()
    bp.search()
    assert key(bp.engine.root_stats()) == first
    bp.close()


# ------------------------------------------------------ batched against serial
B, S, FIRST = 16, 32, 4000
FIXED = ("o_left", [0.1, 0.05, 0.1, 0.7, 0.05])


def population(model, other=OTHER):
    """The five heuristic agents beside one fixed distribution."""
    return [other_policy(model, other, pid, None) for pid in H] + \
        [other_policy(model, other, *FIXED)]


@functools.lru_cache(maxsize=None)
def serial(K, key_base, seeds, until, ego=EGO):
    """The serial harness over `seeds` on one plain planner of K replicas keyed
    (seed, key_base + k); returns (rows, per-episode steps)."""
    from posggym_baselines_amd.planning import POMCP, RandomSearchPolicy, run_planning_episodes
    from posggym_baselines_amd.planning.engine import PomcpEngine
    model = product()
    other = "1" if ego == "0" else "0"
    cfg = product_config(dict(TEST_CFG), K * S)
    cfg.root_parallel = K
    planner = POMCP(model, ego, cfg, RandomSearchPolicy(model, ego))
    planner._engine.close()
    planner._engine = PomcpEngine(model, ego, cfg, num_trees=K, num_sims=S, tree_key_base=key_base,
                                  type_policies=planner.type_policies)
    steps = []

    def on_step(t, obs, a, ts):
        if t == 0:
            steps.append([])
        steps[-1].append((a[ego], a[other], fhex(ts.rewards[ego])))

    rows = run_planning_episodes(planner, product(), len(seeds), ego, env_seeds=list(seeds),
                                 until=until, other_agents=population(model, other),
                                 on_step=on_step)
    planner.close()
    return rows, steps


def same_episode(row, steps, srow, ssteps, where):
    assert row["other_policy_id"] == srow["other_policy_id"], where
    assert steps == ssteps, where
    assert row["len"] == srow["len"] == len(ssteps), where
    assert fhex(row["return"]) == fhex(srow["return"]), where
    assert fhex(row["discounted_return"]) == fhex(srow["discounted_return"]), where


@pytest.mark.parametrize("until", ["all_done", "agent_done"])
def test_run_episodes_equals_the_serial_harness(until):
    from posggym_baselines_amd.planning import BatchedPOMCP
    model = product()
    pop = population(model)
    bp = BatchedPOMCP(model, EGO, product_config(TEST_CFG, S), B, S, searches=MAX_STEPS, reroot=True)
    rec = Recorder(B, acc=False)
    rows = bp.run_episodes(range(FIRST, FIRST + B), until=until, other_agents=pop, on_step=rec)
    pops = bp.engine.episodes_pop_states()
    bp.close()
    host = product()
    for b in range(B):
        srows, ssteps = serial(1, b, (FIRST + b,), until)
        same_episode(rows[b], rec.steps[b], srows[0], ssteps[0], b)
        k = int(pops["policy_index"][b])
        assert rows[b]["other_policy_id"] == (H + [FIXED[0]])[k]
        if k < 5:        # a heuristic's action is the Python rule's on the state before the step
            host.seed(FIRST + b)
            state = host.sample_initial_state()
            for a_ego, a_oth, _ in rec.steps[b]:
                assert a_oth == pop[k].action_from_state(state)
                state = host.step(state, {EGO: a_ego, OTHER: a_oth}).state
    assert len({int(k) for k in pops["policy_index"]}) >= 4
    lens = [r["len"] for r in rows]
    assert min(lens) < max(lens)
    assert {float(r["return"]) for r in rows} <= {0.0, 0.75, 1.0}
    assert any(r["return"] > 0.0 for r in rows)


def test_episode_queue_equals_the_serial_harness():
    """8 slots, 24 episodes."""
    from posggym_baselines_amd.planning import BatchedPOMCP
    slots, N, first, until = 8, 24, 4100, "all_done"
    seeds = list(range(first, first + N))
    model = product()
    bp = BatchedPOMCP(model, EGO, product_config(TEST_CFG, S), slots, S, searches=MAX_STEPS,
                      reroot=True)
    rec = QueueRecorder(slots, N)
    rows = bp.run_episode_queue(seeds, until=until, other_agents=population(model), on_step=rec)
    bp.close()
    lens = [r["len"] for r in rows]
    assert len(rows) == N and [len(s) for s in rec.steps] == lens
    assert [(r["slot"], r["slot_order"]) for r in rows] == restated_schedule(slots, lens)
    for b in range(slots):
        mine = sorted((r for r in rows if r["slot"] == b), key=lambda r: r["slot_order"])
        srows, ssteps = serial(1, b, tuple(seeds[r["num"]] for r in mine), until)
        for r, sr, ss in zip(mine, srows, ssteps):
            same_episode(r, rec.steps[r["num"]], sr, ss, (b, r["num"]))
    assert any(r["slot_order"] > 0 and r["other_policy_id"] != FIXED[0] for r in rows)


def test_root_parallel_planners_equal_the_serial_harness():
    """16 trees = 4 planners of 4 replicas."""
    from posggym_baselines_amd.planning import BatchedPOMCP
    K, G, first, until = 4, 4, 4200, "all_done"
    model = product()
    bp = BatchedPOMCP(model, EGO, product_config(TEST_CFG, S), G * K, S, searches=MAX_STEPS,
                      reroot=True)
    rec = GroupRecorder(G)
    rows = bp.run_episodes(range(first, first + G), until=until, other_agents=population(model),
                           on_step=rec, root_parallel=K)
    bp.close()
    for g in range(G):
        srows, ssteps = serial(K, g * K, (first + g,), until)
        same_episode(rows[g], rec.steps[g], srows[0], ssteps[0], g)


def test_planner_queue_equals_the_serial_harness():
    """12 trees = 3 planners of 4 replicas, 9 episodes, agent '1' planning."""
    from posggym_baselines_amd.planning import BatchedPOMCP
    K, G, N, first, until, ego = 4, 3, 9, 4300, "agent_done", "1"
    seeds = list(range(first, first + N))
    model = product()
    bp = BatchedPOMCP(model, ego, product_config(TEST_CFG, S), G * K, S, searches=MAX_STEPS,
                      reroot=True)
    rec = GroupQueueRecorder(G, N)
    rows = bp.run_planner_queue(seeds, root_parallel=K, until=until,
                                other_agents=population(model, "0"), on_step=rec)
    bp.close()
    lens = [r["len"] for r in rows]
    assert len(rows) == N and [len(s) for s in rec.steps] == lens
    assert [(r["slot"], r["slot_order"]) for r in rows] == restated_schedule(G, lens)
    for g in range(G):
        mine = sorted((r for r in rows if r["slot"] == g), key=lambda r: r["slot_order"])
        srows, ssteps = serial(K, g * K, tuple(seeds[r["num"]] for r in mine), until, ego=ego)
        for r, sr, ss in zip(mine, srows, ssteps):
            same_episode(r, rec.steps[r["num"]], sr, ss, (g, r["num"]))
    assert any(r["slot_order"] > 0 for r in rows)


# ----------------------------- a type-based engine, belief accuracy on the device
STATS = ["state", "policy"]
IPOMCP_CFG = dict(TEST_CFG, action_selection="pucb", state_belief_only=False)


def typed_setup():
    """IPOMCP modelling {H1, H2, H3} under partial observation; the population
    adds H5 and a fixed policy it does not model."""
    from posggym_baselines_amd.planning import OtherAgentMixturePolicy, RandomSearchPolicy
    model = product(5, 1)
    mix = OtherAgentMixturePolicy(model, OTHER, {
        pid: other_policy(model, OTHER, pid, None) for pid in H[:3]})
    pop = list(mix.policies.values()) + [other_policy(model, OTHER, H[4], None),
                                         other_policy(model, OTHER, *FIXED)]
    return model, mix, RandomSearchPolicy(model, EGO), product_config(IPOMCP_CFG, S), pop


def test_belief_accuracy_on_the_device_equals_the_serial_tracker():
    from posggym_baselines_amd.planning import (IPOMCP, BatchedPOMCP, BeliefStatTracker,
                                                EpisodeEnvView, run_planning_episodes)
    from posggym_baselines_amd.planning.ipomcp import base_type_tables
    model, mix, search, cfg, pop = typed_setup()
    first = 4400
    bp = BatchedPOMCP(model, EGO, cfg, B, S, searches=MAX_STEPS, reroot=True,
                      type_policies=base_type_tables(model, EGO, cfg, {OTHER: mix}, search),
                      other_policy_ids=list(mix.policies))
    rec = Recorder(B)
    rows = bp.run_episodes(range(first, first + B), until="all_done", belief_acc=STATS,
                           track_per_step=True, other_agents=pop, on_step=rec)
    pops = bp.engine.episodes_pop_states()
    assert not bp.episode_belief_acc()["error"].any()
    with pytest.raises(NotImplementedError, match="per-particle"):
        bp.run_episodes(range(first, first + B), belief_acc=["policy", "action"])
    bp.close()
    for b in range(B):
        planner = IPOMCP(model, EGO, cfg, {OTHER: mix}, search)
        swap_engine(planner, model, cfg, S, b)
        env_model = product(5, 1)
        tracker = BeliefStatTracker(planner, EpisodeEnvView(env_model, EGO), track_per_step=True,
                                    stats_to_track=STATS)
        ssteps = []
        srows = run_planning_episodes(
            planner, env_model, 1, EGO, env_seeds=[first + b], until="all_done",
            belief_tracker=tracker, other_agents=pop,
            on_step=lambda t, obs, a, ts: ssteps.append((a[EGO], a[OTHER], fhex(ts.rewards[EGO]))))
        planner._engine.close()
        check_tree(rows[b], rec.steps[b], srows[0], ssteps, STATS, MAX_STEPS, b)
    lens = [r["len"] for r in rows]
    assert min(lens) < max(lens)
    modelled = [b for b in range(B) if int(pops["mixture_index"][b]) >= 0]
    strangers = [b for b in range(B) if int(pops["mixture_index"][b]) < 0]
    assert modelled and strangers
    # under full knowledge of the type the belief is the policy: it is found
    assert any(rows[b][f"belief_policy_acc_{lens[b] - 1}"] == 1.0 for b in modelled)
    vals = [rows[b][f"belief_policy_acc_{t}"] for b in modelled for t in range(lens[b])]
    assert any(0.0 < v < 1.0 for v in vals)
    for b in strangers:
        assert rows[b]["belief_policy_acc"] == 0.0
    assert any(0.0 < rows[b]["belief_state_acc"] for b in range(B))

