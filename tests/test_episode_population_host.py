"""Episodes against a policy population, on the host: ``PopulationAgents``
(planning/episodes.py) against a pure-Python restatement of its draws, the
population overloads of csrc/episode_step.h through their host twins
(pomcp_host_episode_reset_pop / pomcp_host_episode_step_pop) against the
oracle's environment models, and the accuracy arithmetic of
k_episode_belief_acc (pomcp_host_belief_acc, csrc/belief_stats.h bel_accuracy)
against ``POMCP.belief_stats`` on hand-made counts, bit for bit."""
import bisect
import ctypes as C
import types

import numpy as np
import pytest

from oracle.envs import make_model
from oracle.episode import ENV_TREE_BASE, fhex
from oracle.rng import Streams
from posggym_baselines_amd import _native as N
from posggym_baselines_amd.envs import DrivingModel, PursuitEvasionModel
from posggym_baselines_amd.planning.policies import FixedDistributionPolicy, cumulative

S_ENV_POLICY_BASE = 40
S_ENV_POPULATION = 44     # csrc/philox.h; used by no stream of oracle/rng.py
EGO, OTHER = "0", "1"
DISCOUNT = 0.95
CASES = {
    "Driving-v1": (range(3000, 3024), 50),
    "PursuitEvasion-v1": (range(2000, 2024), 100),
}
# unequal, non-dyadic probabilities; the second policy never plays action 0
PROBS = {
    "Driving-v1": [[0.1, 0.2, 0.3, 0.15, 0.25], [0.0, 0.37, 0.21, 0.3, 0.12],
                   [0.05, 0.07, 0.6, 0.17, 0.11]],
    "PursuitEvasion-v1": [[0.1, 0.2, 0.3, 0.4], [0.0, 0.37, 0.21, 0.42], [0.05, 0.07, 0.6, 0.28]],
}
IDS = ["slow", "never0", "keen"]


def env_handle(env):
    if env == "Driving-v1":
        m = DrivingModel()
        return N.ENV_DRIVING, m.pomcp_grid(), m
    m = PursuitEvasionModel()
    return N.ENV_PURSUIT_EVASION, m.pomcp_pe_grid(), m


def population(env, model):
    return [FixedDistributionPolicy(model, OTHER, pid, p) for pid, p in zip(IDS, PROBS[env])]


def c_population(env, mixture_index=(0, -1, 1)):
    pop = N.PomcpEpisodePopulation()
    pop.num_policies = len(PROBS[env])
    for k, pi in enumerate(PROBS[env]):
        for a, p in enumerate(pi):
            pop.pi[k][a] = p
    for k in range(N.POMCP_MAX_TYPE_POLICIES):
        pop.mixture_index[k] = mixture_index[k] if k < len(mixture_index) else -1
    return pop


def word(seed, stream, j):
    w = (C.c_uint32 * 1)()
    assert N.load().pomcp_philox_words(seed, ENV_TREE_BASE, stream, j, 1, w) == 0
    return int(w[0])


def restated_index(seed, n):
    return (word(seed, S_ENV_POPULATION, 0) * n) >> 32


def restated_action(seed, probs, j):
    cum, total = cumulative(probs)
    x = word(seed, S_ENV_POLICY_BASE + int(OTHER), j) * 2.0 ** -32 * total
    return bisect.bisect_right(cum, x, 0, len(cum) - 1)


@pytest.mark.parametrize("env", list(CASES))
def test_population_agents_equal_the_restatement(env):
    from posggym_baselines_amd.planning import PopulationAgents
    from posggym_baselines_amd.planning.episodes import UniformRandomAgents
    seeds, max_steps = CASES[env]
    _, _, model = env_handle(env)
    pop = population(env, model)
    seen, differs = set(), 0
    for seed in seeds:
        agents = PopulationAgents(model, seed, pop)
        agents.reset()
        k = restated_index(seed, len(pop))
        assert (agents.policy_index, agents.policy_id) == (k, IDS[k]), seed
        seen.add(k)
        uniform = UniformRandomAgents(model, seed)
        uniform.reset()
        got = [agents.act(OTHER) for _ in range(max_steps)]
        assert got == [restated_action(seed, PROBS[env][k], j) for j in range(max_steps)], seed
        if k == 1:
            assert 0 not in got
        differs += got != [uniform.act(OTHER) for _ in range(max_steps)]
        # a reset starts the same episode again
        agents.reset()
        assert agents.policy_index == k and agents.act(OTHER) == got[0]
    assert seen == {0, 1, 2}          # the seeds reach every policy
    assert differs == len(seeds)      # and none of them plays the uniform agent's actions


def test_population_is_checked():
    from posggym_baselines_amd.planning import PopulationAgents
    model = DrivingModel()
    pop = population("Driving-v1", model)
    with pytest.raises(ValueError, match="duplicate"):
        PopulationAgents(model, 1, pop + [pop[0]])
    with pytest.raises(ValueError, match="1 to 8"):
        PopulationAgents(model, 1, [])
    many = [FixedDistributionPolicy(model, OTHER, f"p{k}", PROBS["Driving-v1"][0])
            for k in range(9)]
    with pytest.raises(ValueError, match="1 to 8"):
        PopulationAgents(model, 1, many)
    with pytest.raises(NotImplementedError):
        PopulationAgents(model, 1, [object()])


def scripted_ego(seed, t, n):
    return (seed + 3 * t + t * t) % n


def replay(env, seed, pop, until):
    """One episode through the population twins with a scripted ego, checked
    step by step against the oracle's environment model; returns the record,
    the population record and the per-step outputs."""
    lib = N.load()
    env_id, grid, model = env_handle(env)
    max_steps = CASES[env][1]
    ego = int(EGO)
    A = model.action_spaces[EGO].n
    pow_table = (C.c_double * max_steps)(*[DISCOUNT ** t for t in range(max_steps)])
    oracle = make_model(env, Streams(seed, ENV_TREE_BASE))
    state = oracle.sample_initial_state()
    obs = oracle.sample_initial_obs(state)
    st, ps, key = N.PomcpEpisodeState(), N.PomcpEpisodePopState(), C.c_uint64()
    ppop = C.byref(pop) if pop is not None else None
    assert lib.pomcp_host_episode_reset_pop(env_id, C.byref(grid), ego, seed, ppop, C.byref(st),
                                            C.byref(ps), C.byref(key)) == 0
    assert key.value == oracle.pack_obs(obs[EGO])
    if pop is None:
        assert (ps.policy_index, ps.mixture_index) == (-1, -1)
    else:
        k = restated_index(seed, pop.num_policies)
        assert (ps.policy_index, ps.mixture_index) == (k, pop.mixture_index[k])
    outs = []
    ret = disc = 0.0
    for t in range(max_steps + 1):
        a_ego = scripted_ego(seed, t, A)
        i = N.PomcpEpisodeStepIn(root_absorbing=0, action=a_ego, search_depth=2, num_sims=8,
                                 min_value=-1.0, max_value=1.0)
        o = N.PomcpEpisodeStepOut()
        assert lib.pomcp_host_episode_step_pop(env_id, C.byref(grid), ego, C.byref(i), pow_table,
                                               max_steps, until, ppop, C.byref(ps), C.byref(st),
                                               C.byref(o)) == 0
        if not o.stepped:
            break
        if pop is None:
            a_oth = (word(seed, S_ENV_POLICY_BASE + int(OTHER), t) * A) >> 32
        else:
            a_oth = restated_action(seed, list(pop.pi[ps.policy_index])[:A], t)
        where = (env, seed, t)
        assert (o.ego_action, o.other_action) == (a_ego, a_oth), where
        ts = oracle.step(state, {EGO: a_ego, OTHER: a_oth})
        state, obs = ts.state, ts.observations
        assert fhex(o.reward) == fhex(ts.rewards[EGO]), where
        assert o.obs_key == oracle.pack_obs(obs[EGO]), where
        ret += ts.rewards[EGO]
        disc += DISCOUNT ** t * ts.rewards[EGO]
        done = bool(ts.all_done) if until == N.UNTIL_ALL_DONE else \
            bool(ts.terminations[EGO] or ts.all_done)
        truncated = t + 1 >= max_steps
        assert (st.res.len, st.finished, st.res.truncated) == \
            (t + 1, int(done or truncated), int(truncated)), where
        assert (st.res.all_done, st.res.ego_terminated) == \
            (int(bool(ts.all_done)), int(bool(ts.terminations[EGO]))), where
        assert st.last_other_action == a_oth and st.policy_ctr == t + 1
        outs.append((o.ego_action, o.other_action, fhex(o.reward), o.obs_key))
    assert st.finished == 1 and st.res.error == 0 and st.res.len == len(outs)
    assert (fhex(st.res.ret), fhex(st.res.discounted_return)) == (fhex(ret), fhex(disc))
    return st, ps, outs


@pytest.mark.parametrize("until", [N.UNTIL_ALL_DONE, N.UNTIL_AGENT_DONE])
@pytest.mark.parametrize("env", list(CASES))
def test_population_twins_replay_the_oracle_environment(env, until):
    seeds, max_steps = CASES[env]
    pop = c_population(env)
    lengths, seen = [], set()
    for seed in seeds:
        st, ps, outs = replay(env, seed, pop, until)
        lengths.append(st.res.len)
        seen.add(ps.policy_index)
        if ps.policy_index == 1:
            assert all(o[1] != 0 for o in outs)
    assert seen == {0, 1, 2}
    assert min(lengths) < max(lengths)


@pytest.mark.parametrize("env", list(CASES))
def test_null_population_equals_the_existing_twins(env):
    lib = N.load()
    env_id, grid, model = env_handle(env)
    seeds, max_steps = CASES[env]
    ego = int(EGO)
    A = model.action_spaces[EGO].n
    pow_table = (C.c_double * max_steps)(*[DISCOUNT ** t for t in range(max_steps)])
    for seed in list(seeds)[:8]:
        st, _, outs = replay(env, seed, None, N.UNTIL_ALL_DONE)
        ref, key = N.PomcpEpisodeState(), C.c_uint64()
        assert lib.pomcp_host_episode_reset(env_id, C.byref(grid), ego, seed, C.byref(ref),
                                            C.byref(key)) == 0
        ref_outs = []
        for t in range(max_steps + 1):
            i = N.PomcpEpisodeStepIn(root_absorbing=0, action=scripted_ego(seed, t, A),
                                     search_depth=2, num_sims=8, min_value=-1.0, max_value=1.0)
            o = N.PomcpEpisodeStepOut()
            assert lib.pomcp_host_episode_step(env_id, C.byref(grid), ego, C.byref(i), pow_table,
                                               max_steps, N.UNTIL_ALL_DONE, C.byref(ref),
                                               C.byref(o)) == 0
            if not o.stepped:
                break
            ref_outs.append((o.ego_action, o.other_action, fhex(o.reward), o.obs_key))
        assert outs == ref_outs and bytes(st) == bytes(ref), (env, seed)
    # a null population needs no record; a population needs one
    st, key = N.PomcpEpisodeState(), C.c_uint64()
    assert lib.pomcp_host_episode_reset_pop(env_id, C.byref(grid), ego, 5, None, C.byref(st), None,
                                            C.byref(key)) == 0
    pop = c_population(env)
    assert lib.pomcp_host_episode_reset_pop(env_id, C.byref(grid), ego, 5, C.byref(pop),
                                            C.byref(st), None, C.byref(key)) == N.POMCP_E_INVALID
    pop.num_policies = 9
    ps = N.PomcpEpisodePopState()
    assert lib.pomcp_host_episode_reset_pop(env_id, C.byref(grid), ego, 5, C.byref(pop),
                                            C.byref(st), C.byref(ps), C.byref(key)) == \
        N.POMCP_E_INVALID
    pop = c_population(env)
    pop.pi[1][1] = -0.5
    assert lib.pomcp_host_episode_reset_pop(env_id, C.byref(grid), ego, 5, C.byref(pop),
                                            C.byref(st), C.byref(ps), C.byref(key)) == \
        N.POMCP_E_INVALID


# ------------------------------------------------------ the accuracy arithmetic
OTHER_PI = [[0.1, 0.2, 0.3, 0.15, 0.25], [0.0, 0.37, 0.21, 0.3, 0.12], [0.05, 0.07, 0.6, 0.17, 0.11],
            [0.2, 0.2, 0.2, 0.2, 0.2]]


def tracker_arithmetic(n, matches, hist, true_id, action):
    """``POMCP.belief_stats`` itself (planning/pomcp.py) on a stub planner whose
    engine returns these counts: the arithmetic the kernel restates."""
    from posggym_baselines_amd.planning import POMCP, OtherAgentMixturePolicy
    model = DrivingModel()
    ids = [f"pi{j}" for j in range(len(hist))]
    mix = OtherAgentMixturePolicy(model, OTHER, {
        pid: FixedDistributionPolicy(model, OTHER, pid, OTHER_PI[j]) for j, pid in enumerate(ids)})
    counts = np.zeros(1, dtype=N.BELIEF_COUNTS_DTYPE)
    counts["belief_size"], counts["state_matches"] = n, matches
    counts["policy_hist"][0, :len(hist)] = hist
    stub = types.SimpleNamespace(
        config=types.SimpleNamespace(state_belief_only=False), BELIEF_STATS=POMCP.BELIEF_STATS,
        model=model, agent_id=EGO, other_agent_policies={OTHER: mix},
        _engine=types.SimpleNamespace(belief_counts=lambda q: counts))
    out = POMCP.belief_stats(stub, state=(1, 2), other_policy_ids={OTHER: true_id},
                             other_actions={OTHER: action})
    return [out["state"], out["policy"], out["action"]]


ACC_CASES = [
    # n, matches, hist, true policy's mixture index (-1: not modelled), action
    (0, 0, [0, 0, 0], 1, 2),                 # an empty belief
    (7, 3, [2, 0, 5], 0, 2),                 # a histogram with a zero, n no power of two
    (7, 3, [2, 0, 5], 1, 0),                 # the true policy has no particle
    (7, 0, [2, 0, 5], -1, 4),                # the planner does not model the true policy
    (1000, 333, [333, 334, 333], 2, 1),
    (193, 64, [64, 65, 64], 1, 0),           # a zero-probability action in one bin
    (4099, 4099, [1, 4097, 1, 0], 3, 3),
    (97, 11, [97], 0, 3),                    # one policy
]


@pytest.mark.parametrize("n,matches,hist,mix,action", ACC_CASES)
def test_host_belief_acc_is_the_trackers_arithmetic(n, matches, hist, mix, action):
    lib = N.load()
    c = N.PomcpBeliefCounts(belief_size=n, state_matches=matches)
    for j, h in enumerate(hist):
        c.policy_hist[j] = h
    pi = ((C.c_double * N.POMCP_MAX_ACTIONS) * N.POMCP_MAX_TYPE_POLICIES)()
    for j in range(len(hist)):
        for a, p in enumerate(OTHER_PI[j]):
            pi[j][a] = p
    out = (C.c_double * 3)()
    flat = C.cast(pi, C.POINTER(C.c_double))
    assert lib.pomcp_host_belief_acc(C.byref(c), mix, action, flat, len(hist), out) == 0
    true_id = f"pi{mix}" if mix >= 0 else "a_stranger"
    exp = tracker_arithmetic(n, matches, hist, true_id, action)
    assert [float(x).hex() for x in out] == [float(x).hex() for x in exp]
    if n:
        assert out[0] == matches / n
        if mix < 0:
            assert out[1] == 0.0
    else:
        assert list(out) == [0.0, 0.0, 0.0]
    # particles without a policy (a plain context): the state accuracy alone
    assert lib.pomcp_host_belief_acc(C.byref(c), mix, action, None, 0, out) == 0
    assert list(out) == [matches / n if n else 0.0, 0.0, 0.0]
    assert lib.pomcp_host_belief_acc(C.byref(c), mix, action, None, 2, out) == N.POMCP_E_INVALID
    assert lib.pomcp_host_belief_acc(None, mix, action, flat, 1, out) == N.POMCP_E_INVALID


def test_new_structs_have_the_c_sizes(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    structs = {"pomcp_episode_population": N.PomcpEpisodePopulation,
               "pomcp_episode_pop_state": N.PomcpEpisodePopState,
               "pomcp_episode_belief_acc": N.PomcpEpisodeBeliefAcc,
               # the existing records keep their layout (ABI 7)
               "pomcp_episode_state": N.PomcpEpisodeState,
               "pomcp_episode_result": N.PomcpEpisodeResult}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "pomcp.h"', "int main(void){"]
    for st, cls in structs.items():
        lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
        for f, *_ in cls._fields_:
            lines.append(f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));')
    lines.append("return 0;}")
    (tmp_path / "probe.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"),
                    str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.run(
        [str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split("\n")
        if line)
    for st, cls in structs.items():
        assert int(out[st]) == C.sizeof(cls), st
        for f, *_ in cls._fields_:
            assert int(out[f"{st}.{f}"]) == getattr(cls, f).offset, f"{st}.{f}"
    assert C.sizeof(N.PomcpEpisodeState) == 120 and C.sizeof(N.PomcpEpisodeResult) == 80
    assert C.sizeof(N.PomcpEpisodePopState) == np.dtype(N.EPISODE_POP_STATE_DTYPE).itemsize == 8
    assert C.sizeof(N.PomcpEpisodeBeliefAcc) == np.dtype(N.EPISODE_BELIEF_ACC_DTYPE).itemsize == 32
    assert N.load().pomcp_abi_version() == 7
