"""State-reactive policies modelled inside the search (k_search<TM = 1>'s
other-agent draw at the tree levels and in the rollout, k_update's rejection
reinvigoration, pomcp_set_type_policy_kinds): every reference golden of
tests/golden/reactive (the real reference IPOMCP / POTMMCP with
ShortestPathPolicy members in the mixture) record for record and trace for
trace, the batched type-based engine with belief accuracy against the serial
harness, and the guards."""
import functools

import pytest

from golden_util import load
from gpu_util import product_config, product_model
from oracle.episode import run_episode
from test_gpu_episode_population import Recorder, check_tree, serial_row, swap_engine
from test_gpu_potmmcp import _record

pytestmark = pytest.mark.gpu

EGO, OTHER = "0", "1"
CASES = ["ipomcp_pucb", "ipomcp_deep_ego1", "ipomcp_reinv", "potmmcp"]
A0, A100 = "Driving-v1/A0Shortestpath-v0", "Driving-v1/A100Shortestpath-v0"
FIXED = ("o_left", [0.1, 0.05, 0.5, 0.3, 0.05])


def other_policy(model, other, pid, row):
    from posggym_baselines_amd.planning.policies import FixedDistributionPolicy, ShortestPathPolicy
    if row is None:
        return ShortestPathPolicy.from_id(model, other, pid)
    return FixedDistributionPolicy(model, other, pid, row)


def make_planner(data, cfg, model):
    from posggym_baselines_amd.planning import (IPOMCP, POTMMCP, OtherAgentMixturePolicy,
                                                POTMMCPMetaPolicy, RandomSearchPolicy)
    from posggym_baselines_amd.planning.policies import FixedDistributionPolicy
    ego, spec = data["ego"], data["spec"]
    other = [i for i in model.possible_agents if i != ego][0]
    config = product_config(cfg, data["num_sims"])
    if data["planner"] == "POTMMCP":
        ego_pols = {k: FixedDistributionPolicy(model, ego, k, v) for k, v in spec["ego"].items()}
        mix = OtherAgentMixturePolicy(model, other, {
            k: other_policy(model, other, k, v) for k, v in spec["other"].items()})
        return POTMMCP(model, ego, config, {other: mix},
                       POTMMCPMetaPolicy(model, ego, ego_pols, spec["meta"]))
    mix = OtherAgentMixturePolicy(model, other, {
        k: other_policy(model, other, k, v) for k, v in spec["other"]["policies"].items()})
    return IPOMCP(model, ego, config, {other: mix}, RandomSearchPolicy(model, ego))


@pytest.mark.parametrize("case", CASES)
def test_reactive_mixtures_match_the_reference_goldens(case):
    data = load("reactive/" + case)
    ego = data["ego"]
    for ep in data["episodes"]:
        model = product_model(data["env"])
        planner = make_planner(data, ep["config"], model)
        assert planner.type_policies is not None and planner._engine.other_reactive
        planner.reset()
        A = model.action_spaces[ego].n
        records = []

        def step(obs):
            searched = not planner.root.is_absorbing
            a = planner.step(obs)
            if not searched:
                records.append({"searched": False, "action": int(a)})
            else:
                records.append(_record(planner, planner._engine, 0, A, a,
                                       planner.step_statistics["num_sims"]))
            return a

        trace = run_episode(step, ep["env_seed"], ego=ego, max_steps=data["max_steps"],
                            env=data["env"])
        planner.close()
        assert len(records) == len(ep["records"]), case
        for t, (got, exp) in enumerate(zip(records, ep["records"])):
            assert got == exp, f"{case} env_seed {ep['env_seed']} step {t}"
        assert trace == ep["trace"]


# ------------------------------------------------- batched, type-based engine
B, S, FIRST, MAX_STEPS = 70, 64, 3000, 50
SUBSET = [0, 1, 2, 3, 4, 5, 64, 65, 66, 67, 68, 69]     # both search waves
STATS = ["policy", "state"]
IPOMCP_CFG = dict(discount=0.95, search_time_limit=0.1, c=2.0 ** 0.5, truncated=False,
                  action_selection="pucb", pucb_exploration_fraction=0.25, known_bounds=None,
                  step_limit=None, epsilon=0.92, seed=0, state_belief_only=False)


def setup():
    """IPOMCP modelling {A100, A0}; the population adds a fixed policy it does
    not model."""
    from posggym_baselines_amd.planning import OtherAgentMixturePolicy, RandomSearchPolicy
    model = product_model("Driving-v1")
    mix = OtherAgentMixturePolicy(model, OTHER, {
        pid: other_policy(model, OTHER, pid, None) for pid in (A100, A0)})
    pop = list(mix.policies.values()) + [other_policy(model, OTHER, *FIXED)]
    return model, mix, RandomSearchPolicy(model, EGO), product_config(IPOMCP_CFG, S), pop


@functools.lru_cache(maxsize=None)
def serial_subset():
    from posggym_baselines_amd.planning import IPOMCP
    model, mix, search, cfg, pop = setup()
    out = {}
    for b in SUBSET:
        planner = IPOMCP(model, EGO, cfg, {OTHER: mix}, search)
        swap_engine(planner, model, cfg, S, b)
        out[b] = serial_row(planner, "Driving-v1", FIRST + b, pop, STATS, "all_done")
        planner._engine.close()
    return out


def test_batched_episodes_with_modelled_reactive_policies_and_belief_accuracy():
    from posggym_baselines_amd.planning import BatchedPOMCP
    from posggym_baselines_amd.planning.ipomcp import base_type_tables
    model, mix, search, cfg, pop = setup()
    bp = BatchedPOMCP(model, EGO, cfg, B, S, searches=MAX_STEPS, reroot=True,
                      type_policies=base_type_tables(model, EGO, cfg, {OTHER: mix}, search),
                      other_policy_ids=list(mix.policies))
    rec = Recorder(B)
    rows = bp.run_episodes(range(FIRST, FIRST + B), until="all_done", belief_acc=STATS,
                           track_per_step=True, other_agents=pop, on_step=rec)
    pops = bp.engine.episodes_pop_states()
    assert not bp.episode_belief_acc()["error"].any()
    # 'action' accuracy would need a per-particle evaluation: refused before a launch
    with pytest.raises(NotImplementedError, match="per-particle"):
        bp.run_episodes(range(FIRST, FIRST + B), belief_acc=["policy", "action"])
    with pytest.raises(NotImplementedError, match="per-particle"):
        bp.run_episodes(range(FIRST, FIRST + B), belief_acc=["action"])
    bp.close()
    serial = serial_subset()
    assert {int(pops["policy_index"][b]) for b in SUBSET} == {0, 1, 2}
    for b in SUBSET:
        srow, ssteps = serial[b]
        check_tree(rows[b], rec.steps[b], srow, ssteps, STATS, MAX_STEPS, b)
    lens = [r["len"] for r in rows]
    assert min(lens) < max(lens)                           # episodes of different lengths
    vals = [rows[b][f"belief_policy_acc_{t}"] for b in range(B) for t in range(lens[b])]
    assert any(0.0 < v < 1.0 for v in vals)
    strangers = [b for b in range(B) if int(pops["policy_index"][b]) == 2]
    assert strangers and all(int(pops["mixture_index"][b]) == -1 for b in strangers)
    for b in strangers:                                    # the unmodelled member's column
        assert rows[b]["other_policy_id"] == FIXED[0] and rows[b]["belief_policy_acc"] == 0.0
        assert all(rows[b][f"belief_policy_acc_{t}"] == 0.0 for t in range(lens[b]))


def test_guards_and_the_kinds_entry_point():
    from posggym_baselines_amd import _native as N
    from posggym_baselines_amd._native import PomcpError
    from posggym_baselines_amd.planning import (IPOMCP, BeliefStatTracker, EpisodeEnvView, POMCP,
                                                RandomSearchPolicy)
    import ctypes as C
    model, mix, search, cfg, pop = setup()
    planner = IPOMCP(model, EGO, cfg, {OTHER: mix}, search)
    with pytest.raises(NotImplementedError, match="per-particle"):
        BeliefStatTracker(planner, EpisodeEnvView(model, EGO), stats_to_track=["policy", "action"])
    BeliefStatTracker(planner, EpisodeEnvView(model, EGO), stats_to_track=["policy", "state"])
    planner.reset()
    with pytest.raises(NotImplementedError, match="per-particle"):
        planner.belief_stats(other_actions={OTHER: 0}, stats=["action"])
    # the entry point: after pomcp_set_type_policies, Driving only, checked parameters
    lib, ctx = planner._engine._lib, planner._engine._ctx
    SP = N.POLICY_DRIVING_SHORTEST_PATH

    def kinds(kind, p0, p1):
        rec = N.PomcpPolicyKinds()
        rec.kind[1], rec.param0[1], rec.param1[1] = kind, p0, p1
        return C.byref(rec)

    assert lib.pomcp_set_type_policy_kinds(ctx, kinds(SP, 3, 2)) == 0
    assert lib.pomcp_set_type_policy_kinds(ctx, None) == 0
    for bad in ((2, 0, 3), (SP, 16, 3), (SP, 1, 4), (SP, -1, 3)):
        assert lib.pomcp_set_type_policy_kinds(ctx, kinds(*bad)) == N.POMCP_E_INVALID
    planner.close()
    plain = POMCP(model, EGO, product_config(dict(IPOMCP_CFG, state_belief_only=True), 8),
                  RandomSearchPolicy(model, EGO))
    assert lib.pomcp_set_type_policy_kinds(plain._engine._ctx, kinds(SP, 1, 3)) == N.POMCP_E_STATE
    plain.close()
    pe = product_model("PursuitEvasion-v1")
    from posggym_baselines_amd.planning import OtherAgentMixturePolicy
    from posggym_baselines_amd.planning.policies import FixedDistributionPolicy
    pe_mix = OtherAgentMixturePolicy(pe, OTHER, {
        k: FixedDistributionPolicy(pe, OTHER, k, [0.25] * 4) for k in ("a", "b")})
    pe_planner = IPOMCP(pe, EGO, cfg, {OTHER: pe_mix}, RandomSearchPolicy(pe, EGO))
    assert lib.pomcp_set_type_policy_kinds(pe_planner._engine._ctx, kinds(SP, 1, 3)) == \
        N.POMCP_E_UNSUPPORTED
    assert lib.pomcp_set_type_policy_kinds(pe_planner._engine._ctx, kinds(0, 0, 0)) == 0
    pe_planner.close()
    with pytest.raises(PomcpError):
        planner.belief_stats(state=(1, 2))      # (closed: nothing runs on it)
