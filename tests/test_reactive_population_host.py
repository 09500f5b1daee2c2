"""Episodes against a population with state-reactive members, on the host: the
episode step of csrc/episode_step.h with pomcp_policy_kinds through its host
twin (pomcp_host_episode_step_pop_kinds) against ``oracle/driving.py`` and the
Python policy, step by step; ``PopulationAgents`` and the serial harness with
such members; a population of fixed distributions byte for byte what it was;
and the guards, each raised before anything is launched."""
import ctypes as C
import types

import pytest

from oracle.driving import DrivingModel as OracleDriving
from oracle.episode import ENV_TREE_BASE, fhex
from oracle.rng import Streams
from posggym_baselines_amd import _native as N
from posggym_baselines_amd.envs import DrivingModel, PursuitEvasionModel
from posggym_baselines_amd.planning.policies import (FixedDistributionPolicy, ShortestPathPolicy,
                                                     cumulative)
from test_episode_population_host import (CASES, DISCOUNT, PROBS, c_population, replay,
                                          restated_index, scripted_ego, word)

EGO, OTHER = "0", "1"
A0, A80, A100 = (f"Driving-v1/A{g}Shortestpath-v0" for g in (0, 80, 100))
FIXED = ("never0", PROBS["Driving-v1"][1])
SEEDS, MAX_STEPS = CASES["Driving-v1"]


def population(model, other=OTHER):
    """Two reactive members around a fixed one."""
    return [ShortestPathPolicy.from_id(model, other, A100),
            FixedDistributionPolicy(model, other, *FIXED),
            ShortestPathPolicy.from_id(model, other, A0)]


def c_records(pop):
    """The population as the C ABI takes it (planning/episodes.py's route)."""
    from posggym_baselines_amd.planning.episodes import check_population, population_kinds
    planner = types.SimpleNamespace(engine=types.SimpleNamespace(model=pop[0].model))
    rec = N.PomcpEpisodePopulation()
    rec.num_policies = len(pop)
    for k, pi in enumerate(check_population(pop, 5)):
        for a, p in enumerate(pi):
            rec.pi[k][a] = p
    for k in range(N.POMCP_MAX_TYPE_POLICIES):
        rec.mixture_index[k] = -1
    kinds = N.PomcpPolicyKinds()
    for k, (kind, p0, p1) in enumerate(population_kinds(planner, pop)):
        kinds.kind[k], kinds.param0[k], kinds.param1[k] = kind, p0, p1
    return rec, kinds


@pytest.mark.parametrize("until", [N.UNTIL_ALL_DONE, N.UNTIL_AGENT_DONE])
@pytest.mark.parametrize("ego", [0, 1])
def test_kinds_twin_replays_the_oracle_environment_and_the_python_policy(ego, until):
    lib = N.load()
    model = DrivingModel()
    grid = model.pomcp_grid()
    other = str(1 - ego)
    pow_table = (C.c_double * MAX_STEPS)(*[DISCOUNT ** t for t in range(MAX_STEPS)])
    seen, lengths, braked = set(), [], 0
    for seed in SEEDS:
        oracle = OracleDriving(Streams(seed, ENV_TREE_BASE))
        pop = population(oracle, other)
        rec, kinds = c_records(pop)
        state = oracle.sample_initial_state()
        st, ps, key = N.PomcpEpisodeState(), N.PomcpEpisodePopState(), C.c_uint64()
        assert lib.pomcp_host_episode_reset_pop(N.ENV_DRIVING, C.byref(grid), ego, seed,
                                                C.byref(rec), C.byref(st), C.byref(ps),
                                                C.byref(key)) == 0
        k = restated_index(seed, 3)
        assert ps.policy_index == k
        seen.add(k)
        cum, total = cumulative(FIXED[1])
        for t in range(MAX_STEPS + 1):
            a_ego = scripted_ego(seed, t, 5)
            i = N.PomcpEpisodeStepIn(root_absorbing=0, action=a_ego, search_depth=2, num_sims=8,
                                     min_value=-1.0, max_value=1.0)
            o = N.PomcpEpisodeStepOut()
            assert lib.pomcp_host_episode_step_pop_kinds(
                N.ENV_DRIVING, C.byref(grid), ego, C.byref(i), pow_table, MAX_STEPS, until,
                C.byref(rec), C.byref(kinds), C.byref(ps), C.byref(st), C.byref(o)) == 0
            if not o.stepped:
                break
            if k == 1:
                import bisect
                x = word(seed, 40 + int(other), t) * 2.0 ** -32 * total
                a_oth = bisect.bisect_right(cum, x, 0, 4)
            else:
                a_oth = pop[k].action_from_state(state)    # from the state before the step
                braked += a_oth == 2
            where = (ego, seed, t)
            assert (o.ego_action, o.other_action) == (a_ego, a_oth), where
            ts = oracle.step(state, {str(ego): a_ego, other: a_oth})
            state = ts.state
            assert fhex(o.reward) == fhex(ts.rewards[str(ego)]), where
            assert o.obs_key == oracle.pack_obs(ts.observations[str(ego)]), where
            assert (st.v0, st.v1) == oracle.pack_words(state), where
            # the stream's word is taken whatever the member's kind
            assert st.policy_ctr == t + 1 and st.last_other_action == a_oth
            done = bool(ts.all_done) if until == N.UNTIL_ALL_DONE else \
                bool(ts.terminations[str(ego)] or ts.all_done)
            assert st.finished == int(done or t + 1 >= MAX_STEPS), where
        assert st.finished == 1 and st.res.error == 0
        lengths.append(st.res.len)
    assert seen == {0, 1, 2} and min(lengths) < max(lengths)
    assert braked > 0       # the cautious member met the ego's vehicle


@pytest.mark.parametrize("until", [N.UNTIL_ALL_DONE, N.UNTIL_AGENT_DONE])
def test_a_fixed_population_is_what_it_was_byte_for_byte(until):
    """kinds = NULL and kinds all POMCP_POLICY_FIXED (parameters ignored)
    against the existing population twin."""
    lib = N.load()
    model = DrivingModel()
    grid = model.pomcp_grid()
    pop = c_population("Driving-v1")
    fixed = N.PomcpPolicyKinds()
    for k in range(N.POMCP_MAX_TYPE_POLICIES):
        fixed.param0[k], fixed.param1[k] = 3, 2
    pow_table = (C.c_double * MAX_STEPS)(*[DISCOUNT ** t for t in range(MAX_STEPS)])
    for seed in list(SEEDS)[:8]:
        ref, ref_ps, ref_outs = replay("Driving-v1", seed, pop, until)
        for kinds in (None, C.byref(fixed)):
            st, ps, key = N.PomcpEpisodeState(), N.PomcpEpisodePopState(), C.c_uint64()
            assert lib.pomcp_host_episode_reset_pop(N.ENV_DRIVING, C.byref(grid), 0, seed,
                                                    C.byref(pop), C.byref(st), C.byref(ps),
                                                    C.byref(key)) == 0
            outs = []
            for t in range(MAX_STEPS + 1):
                i = N.PomcpEpisodeStepIn(root_absorbing=0, action=scripted_ego(seed, t, 5),
                                         search_depth=2, num_sims=8, min_value=-1.0, max_value=1.0)
                o = N.PomcpEpisodeStepOut()
                assert lib.pomcp_host_episode_step_pop_kinds(
                    N.ENV_DRIVING, C.byref(grid), 0, C.byref(i), pow_table, MAX_STEPS, until,
                    C.byref(pop), kinds, C.byref(ps), C.byref(st), C.byref(o)) == 0
                if not o.stepped:
                    break
                outs.append((o.ego_action, o.other_action, fhex(o.reward), o.obs_key))
            assert outs == ref_outs and bytes(st) == bytes(ref) and bytes(ps) == bytes(ref_ps)


def test_kinds_are_checked():
    lib = N.load()
    drv, pe = DrivingModel(), PursuitEvasionModel()
    pow_table = (C.c_double * 4)(1.0, 0.5, 0.25, 0.125)
    i = N.PomcpEpisodeStepIn(action=0)
    o = N.PomcpEpisodeStepOut()

    def step(env_id, grid, env, kinds, pop=True):
        rec = c_population(env)
        st, ps, key = N.PomcpEpisodeState(), N.PomcpEpisodePopState(), C.c_uint64()
        assert lib.pomcp_host_episode_reset_pop(env_id, C.byref(grid), 0, 7, C.byref(rec),
                                                C.byref(st), C.byref(ps), C.byref(key)) == 0
        return lib.pomcp_host_episode_step_pop_kinds(
            env_id, C.byref(grid), 0, C.byref(i), pow_table, 4, N.UNTIL_ALL_DONE,
            C.byref(rec) if pop else None, C.byref(kinds), C.byref(ps), C.byref(st), C.byref(o))

    def kinds(kind, p0, p1, k=2):
        rec = N.PomcpPolicyKinds()
        rec.kind[k], rec.param0[k], rec.param1[k] = kind, p0, p1
        return rec

    SP = N.POLICY_DRIVING_SHORTEST_PATH
    dg, pg = drv.pomcp_grid(), pe.pomcp_pe_grid()
    assert step(N.ENV_DRIVING, dg, "Driving-v1", kinds(SP, 3, 2)) == 0
    assert step(N.ENV_DRIVING, dg, "Driving-v1", kinds(SP, 0, 3)) == 0
    for bad in ((2, 0, 3), (-1, 0, 3), (SP, -1, 3), (SP, 16, 3), (SP, 1, 4), (SP, 1, -1)):
        assert step(N.ENV_DRIVING, dg, "Driving-v1", kinds(*bad)) == N.POMCP_E_INVALID, bad
    # entries past the population's three policies are not read
    assert step(N.ENV_DRIVING, dg, "Driving-v1", kinds(9, -5, 77, k=3)) == 0
    # PursuitEvasion has no reactive kinds; all-fixed kinds are accepted there
    assert step(N.ENV_PURSUIT_EVASION, pg, "PursuitEvasion-v1", kinds(SP, 1, 3)) == \
        N.POMCP_E_UNSUPPORTED
    assert step(N.ENV_PURSUIT_EVASION, pg, "PursuitEvasion-v1", kinds(0, 0, 0)) == 0
    # kinds without a population
    assert step(N.ENV_DRIVING, dg, "Driving-v1", kinds(SP, 1, 3), pop=False) == N.POMCP_E_INVALID


# ------------------------------------------------------------------- Python
def test_population_agents_play_reactive_members_from_the_state():
    from posggym_baselines_amd.planning import PopulationAgents
    from posggym_baselines_amd.planning.episodes import UniformRandomAgents
    model = DrivingModel()
    pop = population(model)
    seen = set()
    for seed in SEEDS:
        agents = PopulationAgents(model, seed, pop)
        agents.reset()
        k = restated_index(seed, 3)
        assert (agents.policy_index, agents.policy_id) == (k, pop[k].policy_id)
        seen.add(k)
        model.seed(seed)
        state = model.sample_initial_state()
        uniform = UniformRandomAgents(model, seed)
        uniform.reset()
        for t in range(6):
            a = agents.act(OTHER, state)
            assert agents._ctr[OTHER] == t + 1      # one word of the stream per action
            if k != 1:
                assert a == pop[k].action_from_state(state)
            state = model.step(state, {EGO: scripted_ego(seed, t, 5), OTHER: a}).state
            uniform.act(OTHER, state)               # (the state is accepted and ignored)
        if k != 1:
            with pytest.raises(ValueError, match="acts on the state"):
                agents.act(OTHER)
            with pytest.raises(ValueError, match="agent"):
                agents.act(EGO, state)
    assert seen == {0, 1, 2}


def stub_planner(model, ego=EGO):
    return types.SimpleNamespace(engine=types.SimpleNamespace(
        model=model, A=5, ego=model.possible_agents.index(ego)))


def test_python_guards_raise_before_any_launch():
    from posggym_baselines_amd.planning import (IPOMCP, POTMMCP, MCTSConfig,
                                                OtherAgentMixturePolicy, POTMMCPMetaPolicy)
    from posggym_baselines_amd.planning.episodes import (check_population, episode_population,
                                                         population_kinds)
    from posggym_baselines_amd.planning.search_policy import SearchPolicyWrapper
    drv, pe = DrivingModel(), PursuitEvasionModel()
    pop = population(drv)
    K = N.POLICY_DRIVING_SHORTEST_PATH
    assert population_kinds(stub_planner(drv), pop) == [(K, 0, 3), (N.POLICY_FIXED, 0, 0), (K, 3, 2)]
    # a fixed population makes no kinds call at all
    assert population_kinds(stub_planner(drv), [pop[1]]) is None
    assert population_kinds(stub_planner(drv), None) is None
    ids, probs, mix = episode_population(stub_planner(drv), pop, [A0, "x"])
    assert ids == [A100, "never0", A0] and mix == [-1, -1, 0]
    assert probs[0] == probs[2] == [0.2] * 5 and probs[1] == FIXED[1]
    # a reactive policy on PursuitEvasion, or on a PursuitEvasion planner
    with pytest.raises(NotImplementedError, match="Driving-v1"):
        ShortestPathPolicy(pe, OTHER, "x", 0.5)
    with pytest.raises(NotImplementedError, match="PursuitEvasion"):
        population_kinds(stub_planner(pe), pop)
    # built for the planning agent
    with pytest.raises(ValueError, match="planning agent"):
        population_kinds(stub_planner(drv, ego=OTHER), pop)
    with pytest.raises(ValueError, match="duplicate"):
        check_population(pop + [pop[0]])
    # inside the search a reactive policy is a member of the other agent's
    # mixture: not the search policy, not a meta-policy's ego policy, not alone
    # (all refused while the tables are built, before an engine exists)
    from posggym_baselines_amd.planning.ipomcp import base_type_tables
    from posggym_baselines_amd.planning.potmmcp import type_policy_tables
    cfg = MCTSConfig(discount=0.95, search_time_limit=0.1, c=1.0, truncated=False,
                     action_selection="pucb", pucb_exploration_fraction=0.25, known_bounds=None,
                     step_limit=None, epsilon=0.01, seed=0, state_belief_only=False, num_sims=8)
    mixture = OtherAgentMixturePolicy(drv, OTHER, {p.policy_id: p for p in pop})
    uniform = SearchPolicyWrapper(FixedDistributionPolicy.uniform(drv, EGO))
    tp = base_type_tables(drv, EGO, cfg, {OTHER: mixture}, uniform)
    assert tp.other_kinds == [(K, 0, 3), (N.POLICY_FIXED, 0, 0), (K, 3, 2)]
    assert list(tp.other_pi[0])[:5] == [0.2] * 5           # the placeholder row
    fixed_mix = OtherAgentMixturePolicy(drv, OTHER, {"never0": pop[1]})
    assert base_type_tables(drv, EGO, cfg, {OTHER: fixed_mix}, uniform).other_kinds is None
    with pytest.raises(NotImplementedError, match="other agent only"):
        IPOMCP(drv, EGO, cfg, {OTHER: fixed_mix},
               SearchPolicyWrapper(ShortestPathPolicy.from_id(drv, EGO, A80)))
    import dataclasses
    sbo = dataclasses.replace(cfg, state_belief_only=True)
    with pytest.raises(NotImplementedError, match="OtherAgentMixturePolicy"):
        base_type_tables(drv, EGO, sbo, {OTHER: pop[0]}, uniform)
    with pytest.raises(NotImplementedError, match="PursuitEvasion"):
        base_type_tables(pe, EGO, cfg, {OTHER: OtherAgentMixturePolicy(
            pe, OTHER, {p.policy_id: p for p in pop})}, SearchPolicyWrapper(
                FixedDistributionPolicy.uniform(pe, EGO)))
    ego_pols = {"u": FixedDistributionPolicy.uniform(drv, EGO, "u")}
    meta = POTMMCPMetaPolicy(drv, EGO, ego_pols, {p.policy_id: {"u": 1.0} for p in pop})
    assert type_policy_tables(drv, EGO, meta, mixture).other_kinds == tp.other_kinds
    bad_meta = POTMMCPMetaPolicy(drv, EGO, {"sp": ShortestPathPolicy.from_id(drv, EGO, A80)},
                                 {p.policy_id: {"sp": 1.0} for p in pop})
    with pytest.raises(NotImplementedError, match="other agent only"):
        POTMMCP(drv, EGO, cfg, {OTHER: mixture}, bad_meta)
    # 'action' accuracy with a reactive policy in the planner's mixture
    from posggym_baselines_amd.planning import BeliefStatTracker, EpisodeEnvView
    stub = types.SimpleNamespace(config=cfg, other_agent_policies={OTHER: mixture}, model=drv,
                                 agent_id=EGO)
    with pytest.raises(NotImplementedError, match="per-particle"):
        BeliefStatTracker(stub, EpisodeEnvView(drv, EGO), stats_to_track=["action"])
    BeliefStatTracker(stub, EpisodeEnvView(drv, EGO), stats_to_track=["policy", "state"])
    stub_fixed = types.SimpleNamespace(config=cfg, other_agent_policies={OTHER: fixed_mix},
                                       model=drv, agent_id=EGO)
    BeliefStatTracker(stub_fixed, EpisodeEnvView(drv, EGO), stats_to_track=["action"])
