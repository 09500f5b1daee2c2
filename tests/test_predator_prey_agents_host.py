"""The PredatorPrey-v0 heuristic agents H1 .. H3 on the host: the rule of
csrc/predator_prey_policy.h through its host twins against the Python policy
(planning/policies.py ``PreyHeuristicPolicy``) -- the distribution as exact
doubles and the action each word of the stream draws --, the
observation-driven form against the state-driven one, hand-built states,
episode statistics through the episode step twin, the header under the
sanitizers and the guards."""
import bisect
import ctypes as C
import itertools
import os
import random
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

from oracle.episode import ENV_TREE_BASE, fhex
from oracle.rng import Streams
from posggym_baselines_amd import _native as N
from posggym_baselines_amd.envs import (CooperativeReachingModel, DrivingModel, PredatorPreyModel,
                                        PursuitEvasionModel)
from posggym_baselines_amd.planning.policies import (PREDATOR_PREY_POLICY_IDS,
                                                     FixedDistributionPolicy,
                                                     GoalHeuristicPolicy, PreyHeuristicPolicy,
                                                     cumulative, is_reactive, policy_kinds)
from test_episode_population_host import DISCOUNT, restated_index, scripted_ego, word

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from predator_prey_model import PredatorPreyModel as PyModel  # noqa: E402

H = list(PREDATOR_PREY_POLICY_IDS)
H1, H2, H3 = H
MAX_STEPS = 50
WORDS = 16
S_ENV_POLICY_BASE = 40
PU32, P32, PD = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_double)


def product(grid="10x10", num_prey=3, prey_strength=2, obs_dim=2):
    return PredatorPreyModel(grid=grid, num_prey=num_prey, prey_strength=prey_strength,
                             obs_dim=obs_dim)


def pymodel(grid="10x10", num_prey=3, prey_strength=2, obs_dim=2, seed=0):
    return PyModel(Streams(seed, ENV_TREE_BASE), grid, num_prey, prey_strength, obs_dim)


def state(p0, p1, *prey):
    return (p0, p1, tuple(prey) + (None,) * (3 - len(prey)))


def twin_pi(prod, words, agent, rule):
    """pomcp_host_pp_policy_pi on [(w0, w1)]: an [n][5] array of doubles."""
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, 2)
    w0, w1 = np.ascontiguousarray(w[:, 0]), np.ascontiguousarray(w[:, 1])
    out = np.zeros((len(w), 5), dtype=np.float64)
    rc = N.load().pomcp_host_pp_policy_pi(
        C.byref(prod.pomcp_pp_grid()), len(w), w0.ctypes.data_as(PU32), w1.ctypes.data_as(PU32),
        agent, rule, out.ctypes.data_as(PD))
    assert rc == 0, rc
    return out


def twin_actions(prod, words, agent, rule, draws):
    """pomcp_host_pp_policy_actions: state k with the word draws[k]."""
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, 2)
    w0, w1 = np.ascontiguousarray(w[:, 0]), np.ascontiguousarray(w[:, 1])
    d = np.ascontiguousarray(draws, dtype=np.uint32)
    out = np.zeros(len(w), dtype=np.int32)
    rc = N.load().pomcp_host_pp_policy_actions(
        C.byref(prod.pomcp_pp_grid()), len(w), w0.ctypes.data_as(PU32), w1.ctypes.data_as(PU32),
        agent, rule, d.ctypes.data_as(PU32), out.ctypes.data_as(P32))
    assert rc == 0, rc
    return out


def python_action(pi, w):
    """rng.choices(range(5), weights=pi) on the word ``w`` of the stream."""
    cum, total = cumulative(pi)
    return bisect.bisect_right(cum, w * 2.0 ** -32 * total, 0, len(cum) - 1)


def check_states(prod, py, states, seed):
    """every rule x agent on ``states``: the twin's pi is the Python policy's bit
    for bit (from the tuple state and from the words), and WORDS words per state
    draw the Python action.  Returns the supports seen per rule."""
    rng = random.Random(seed)
    words = [py.pack_words(s) for s in states]
    # words that land on and next to the cumulative weights' steps, and random ones
    edges = [0, 1, (1 << 30) - 1, 1 << 30, (1 << 31) - 1, 1 << 31, 1431655765, 1431655766,
             2863311530, 2863311531, 3 << 30, (1 << 32) - 1]
    seen = {}
    for rule, pid in enumerate(H):
        for agent in (0, 1):
            pol = PreyHeuristicPolicy.from_id(prod, str(agent), pid)
            pyp = PreyHeuristicPolicy.from_id(py, str(agent), pid)
            got = twin_pi(prod, words, agent, rule)
            want = []
            for k, s in enumerate(states):
                pi = pyp.pi_from_state(s)
                want.append(pi)
                assert [fhex(p) for p in got[k]] == [fhex(p) for p in pi], (pid, agent, s)
                seen.setdefault(rule, set()).add(tuple(p > 0.0 for p in pi))
            # (the product model's states are the packed words)
            for k in rng.sample(range(len(states)), min(200, len(states))):
                assert pol.pi_from_state(words[k]) == want[k], (pid, agent, states[k])
            draws = [edges[(k + i) % len(edges)] if i < 4 else rng.getrandbits(32)
                     for k in range(len(states)) for i in range(WORDS)]
            acts = twin_actions(prod, [w for w in words for _ in range(WORDS)], agent, rule, draws)
            for k in range(len(states)):
                for i in range(WORDS):
                    j = k * WORDS + i
                    assert acts[j] == python_action(want[k], draws[j]), \
                        (pid, agent, states[k], draws[j])
    return seen


def sampled_states(py, n, seed):
    """seeded states, with caught prey among them: distinct cells for the
    predators and the live prey"""
    rng = random.Random(seed)
    S = py.size
    cells = [(x, y) for y in range(S) for x in range(S)]
    out = []
    for _ in range(n):
        live = [k for k in range(py.num_prey) if rng.random() < 0.8]
        pick = rng.sample(cells, 2 + len(live))
        prey = [None] * 3
        for k, c in zip(live, pick[2:]):
            prey[k] = c
        out.append((pick[0], pick[1], tuple(prey)))
    return out


# ------------------------------------------------------------------ rule twin
def test_rule_twin_equals_the_python_policy_exhaustively_on_5x5_with_one_prey():
    prod, py = product("5x5", 1, 1, 1), pymodel("5x5", 1, 1, 1)
    cells = [(x, y) for y in range(5) for x in range(5)]
    states = [state(a, b, q) for a, b in itertools.permutations(cells, 2)
              for q in [None] + [c for c in cells if c not in (a, b)]]
    assert len(states) == 25 * 24 * 24
    seen = check_states(prod, py, states, 1)
    # every support size: DO_NOTHING alone, and 1 to 4 moves
    for rule in range(3):
        assert {sum(s[1:]) for s in seen[rule]} == {0, 1, 2, 3, 4}, rule
        assert any(s[0] for s in seen[rule])


@pytest.mark.parametrize("args", [("5x5", 2, 1, 1), ("10x10", 3, 2, 2), ("5x5", 3, 2, 2),
                                  ("10x10", 2, 1, 1)])
def test_rule_twin_equals_the_python_policy_on_sampled_states(args):
    prod, py = product(*args), pymodel(*args)
    n = 20000 if args in (("5x5", 2, 1, 1), ("10x10", 3, 2, 2)) else 2000
    states = sampled_states(py, n, 17)
    assert any(s[2].count(None) == 3 for s in states) and any(None not in s[2][:args[1]]
                                                              for s in states)
    seen = check_states(prod, py, states, 2)
    for rule in range(3):
        assert {sum(s[1:]) for s in seen[rule]} >= {1, 2, 3, 4}, rule


def test_observation_driven_form_equals_the_state_form_under_overrides():
    """300 seeded episodes per rule in which a quarter of the agent's played
    actions are random ones: the policy that saw only its observations gives the
    state form's distribution at every decision."""
    for rule, pid in enumerate(H):
        decisions = overridden = targets = 0
        for seed in range(300):
            rng = random.Random(1000 * rule + seed)
            args = (("5x5", 2, 1, 1), ("10x10", 3, 2, 2), ("5x5", 3, 2, 2), ("10x10", 1, 1, 1))[seed % 4]
            model = pymodel(*args, seed=seed)
            i = seed % 2
            me, mate = str(i), str(1 - i)
            pol = PreyHeuristicPolicy.from_id(model, me, pid, rng=rng)
            helper = PreyHeuristicPolicy(model, mate, "mate", (rule + 1) % 3)
            s = model.sample_initial_state()
            obs = model.sample_initial_obs(s)
            ps = pol.get_next_state(None, obs[me], pol.get_initial_state())
            for t in range(MAX_STEPS):
                pi = pol.get_pi(ps).probs
                want = pol.pi_from_state(s)
                assert [pi[a] for a in range(5)] == want, (pid, seed, t, s)
                assert pol.pi_from_state(model.pack_words(s)) == want
                assert pol.pi_from_obs(model.pack_obs(obs[me])) == want      # (from the key)
                decisions += 1
                targets += sum(p > 0.0 for p in want[1:]) in (1, 2)
                a = pol.sample_action(ps)
                assert want[a] > 0.0
                if rng.random() < 0.25:
                    a = rng.randrange(5)
                    overridden += 1
                a_mate = python_action(helper.pi_from_state(s), rng.getrandbits(32))
                ts = model.step(s, {me: a, mate: a_mate})
                s, obs = ts.state, ts.observations
                ps = pol.get_next_state(a, obs[me], ps)
                if ts.all_done:
                    break
        assert decisions > 5000 and overridden > 1000 and targets > 1000, (pid, decisions)


# ------------------------------------------------------------- known answers
# (5x5, obs_dim 1 unless said; actions DO_NOTHING, UP, DOWN, LEFT, RIGHT)
def pi_of(*moves):
    return [1.0 / len(moves) if a in moves else 0.0 for a in range(5)]


KNOWN = [
    # name, model args, state, agent, {rule: the moves pi is uniform over}
    # explore: nothing in sight, the corner leaves two moves
    ("explore in the corner", ("5x5", 1, 1, 1), state((0, 0), (4, 4), (2, 2)), 0,
     {0: (2, 4), 1: (2, 4), 2: (2, 4)}),
    ("explore in the open", ("5x5", 1, 1, 1), state((2, 2), (4, 4), (0, 0)), 0,
     {0: (1, 2, 3, 4), 1: (1, 2, 3, 4), 2: (1, 2, 3, 4)}),
    # the corner with the mate adjacent and nothing else in sight: H1 and H3
    # head for the mate, whose cell is not free -- nothing brings them closer;
    # H2 is close enough and explores over the one free move
    ("corner, mate adjacent", ("5x5", 1, 1, 1), state((0, 0), (1, 0), (3, 3)), 0,
     {0: (0,), 1: (2,), 2: (0,)}),
    # the mate diagonal: two moves bring the agent closer
    ("mate diagonal", ("5x5", 1, 1, 1), state((1, 1), (2, 2), (4, 0)), 0,
     {0: (2, 4), 1: (2, 4), 2: (2, 4)}),
    # a prey diagonal to the agent: two candidates at 0.5 each
    ("prey diagonal", ("5x5", 1, 1, 1), state((2, 2), (0, 4), (3, 1)), 0,
     {0: (1, 4), 1: (1, 4), 2: (1, 4)}),
    # prey right, mate two cells below (obs_dim 2): H1 hunts, H2 closes up first,
    # H3 hunts the one prey
    ("prey or mate", ("5x5", 1, 1, 2), state((2, 1), (2, 3), (4, 1)), 0,
     {0: (4,), 1: (2,), 2: (4,)}),
    # two prey in sight, the near one left (distance 1 would be adjacent: 2 here),
    # the far one right-down next to the mate: H3 takes the mate's prey
    ("the mate's prey", ("5x5", 2, 2, 2), state((2, 2), (4, 3), (0, 2), (4, 4)), 0,
     {0: (3,), 1: (2, 4), 2: (2, 4)}),
    # a tie between two prey at distance 2: the window's row-major order, the
    # smaller dy first (UP), not the lower prey index; H2 closes up on the mate
    # in the window's corner, H3 takes the prey next to the mate
    ("window order, dy", ("5x5", 2, 1, 2), state((2, 2), (4, 4), (2, 4), (2, 0)), 0,
     {0: (1,), 1: (2, 4), 2: (2,)}),
    # ... and the smaller dx in one row (LEFT)
    ("window order, dx", ("5x5", 2, 1, 2), state((2, 2), (2, 0), (4, 2), (0, 2)), 0,
     {0: (3,), 1: (1,), 2: (3,)}),
    # a chase blocked by a second prey: the target straight ahead, another prey
    # on the only cell that brings the agent closer
    ("blocked by a prey", ("5x5", 2, 2, 2), state((0, 2), (4, 0), (2, 2), (1, 2)), 0,
     {0: (0,), 1: (0,), 2: (0,)}),
    # ... blocked by the mate
    ("blocked by the mate", ("5x5", 1, 2, 2), state((0, 2), (1, 2), (2, 2)), 0,
     {0: (0,), 1: (0,), 2: (0,)}),
    # the other agent's view of a state, and a caught prey is not a target
    ("agent 1, caught prey", ("5x5", 2, 1, 1), state((4, 4), (1, 1), None, (1, 0)), 1,
     {0: (0,), 1: (0,), 2: (0,)}),
    ("agent 1 hunts", ("5x5", 2, 1, 1), state((4, 4), (1, 1), None, (2, 0)), 1,
     {0: (1, 4), 1: (1, 4), 2: (1, 4)}),
    # a prey out of the window is not seen although it is near by Manhattan... (obs_dim 1)
    ("prey two cells away, obs_dim 1", ("10x10", 1, 1, 1), state((5, 5), (0, 0), (7, 5)), 0,
     {0: (1, 2, 3, 4), 1: (1, 2, 3, 4), 2: (1, 2, 3, 4)}),
    # ... and a diagonal one at Manhattan distance 4 is (obs_dim 2)
    ("prey in the window's corner", ("10x10", 1, 1, 2), state((5, 5), (0, 0), (7, 7)), 0,
     {0: (2, 4), 1: (2, 4), 2: (2, 4)}),
]


@pytest.mark.parametrize("case", KNOWN, ids=[c[0] for c in KNOWN])
def test_known_answers(case):
    _, args, s, agent, answers = case
    prod, py = product(*args), pymodel(*args)
    w = py.pack_words(s)
    for rule, moves in answers.items():
        want = pi_of(*moves)
        pol = PreyHeuristicPolicy(py, str(agent), "h", rule)
        assert pol.pi_from_state(s) == want, rule
        assert pol.pi_from_obs(py._obs(s, agent)) == want, rule
        assert twin_pi(prod, [w], agent, rule)[0].tolist() == want, rule
        # the word picks among the support in action order
        acts = twin_actions(prod, [w, w], agent, rule, [0, (1 << 32) - 1])
        assert (acts[0], acts[1]) == (moves[0], moves[-1]), rule


def test_the_corner_case_the_adjacent_mate_blocks():
    """'corner, mate adjacent' above: the free moves of the agent on (0, 0) with
    the mate on (1, 0) are DOWN alone"""
    py = pymodel("5x5", 1, 1, 1)
    s = state((0, 0), (1, 0), (3, 3))
    for rule, want in ((0, pi_of(0)), (1, pi_of(2)), (2, pi_of(0))):
        assert PreyHeuristicPolicy(py, "0", "h", rule).pi_from_state(s) == want


# ---------------------------------------------------------- episode step twin
FIXED = ("never0", [0.0, 0.4, 0.1, 0.3, 0.2])
S_EGO_WORDS = 47          # the scripted ego's own words (a stream nothing else reads)


def c_records(pop):
    rec = N.PomcpEpisodePopulation()
    rec.num_policies = len(pop)
    for k, pol in enumerate(pop):
        pi = pol.probs if isinstance(pol, FixedDistributionPolicy) else [0.2] * 5
        for a, p in enumerate(pi):
            rec.pi[k][a] = p
    for k in range(N.POMCP_MAX_TYPE_POLICIES):
        rec.mixture_index[k] = -1
    kinds = N.PomcpPolicyKinds()
    for k, (kind, p0, p1) in enumerate(policy_kinds(pop[0].model, pop)):
        kinds.kind[k], kinds.param0[k], kinds.param1[k] = kind, p0, p1
    return rec, kinds


# prey caught over the seeds 0 .. 199 with both predators by the same rule, from
# the Python statement alone (python_statistic below): [H1, H2, H3]
CAUGHT_5X5 = [397, 400, 397]        # 5x5, 2 prey, strength 1, obs_dim 1
CAUGHT_10X10 = [12, 21, 12]         # 10x10, 3 prey, strength 2, obs_dim 2


def python_statistic(args, rule, ego=0):
    """Both predators by ``rule`` in the Python model: the ego's word is word t of
    stream S_EGO_WORDS, the other's word t of its environment-policy stream."""
    total = 0
    for seed in range(200):
        py = pymodel(*args, seed=seed)
        pols = [PreyHeuristicPolicy(py, str(i), "h", rule) for i in range(2)]
        s = py.sample_initial_state()
        for t in range(MAX_STEPS):
            a = {}
            for i in range(2):
                stream = S_EGO_WORDS if i == ego else S_ENV_POLICY_BASE + i
                a[str(i)] = python_action(pols[i].pi_from_state(s), word(seed, stream, t))
            ts = py.step(s, a)
            total += sum(q is None for q in ts.state[2]) - sum(q is None for q in s[2])
            s = ts.state
            if ts.all_done:
                break
    return total


@pytest.mark.parametrize("args,known", [(("5x5", 2, 1, 1), CAUGHT_5X5),
                                        (("10x10", 3, 2, 2), CAUGHT_10X10)])
def test_known_episode_statistics_through_the_episode_twin(args, known):
    lib = N.load()
    prod, ego = product(*args), 0
    grid = prod.pomcp_pp_grid()
    pow_table = (C.c_double * MAX_STEPS)(*[DISCOUNT ** t for t in range(MAX_STEPS)])
    reward = prod.capture_reward
    for rule in range(3):
        pop = [PreyHeuristicPolicy(prod, "1", "h", rule)]
        rec, kinds = c_records(pop)
        me = PreyHeuristicPolicy(prod, "0", "me", rule)
        caught = 0
        for seed in range(200):
            st, ps, key = N.PomcpEpisodeState(), N.PomcpEpisodePopState(), C.c_uint64()
            assert lib.pomcp_host_episode_reset_pop(N.ENV_PREDATOR_PREY, C.byref(grid), ego, seed,
                                                    C.byref(rec), C.byref(st), C.byref(ps),
                                                    C.byref(key)) == 0
            for t in range(MAX_STEPS + 1):
                a_ego = python_action(me.pi_from_state((st.v0, st.v1)), word(seed, S_EGO_WORDS, t))
                i = N.PomcpEpisodeStepIn(root_absorbing=0, action=a_ego, search_depth=1, num_sims=1)
                o = N.PomcpEpisodeStepOut()
                assert lib.pomcp_host_episode_step_pop_kinds(
                    N.ENV_PREDATOR_PREY, C.byref(grid), ego, C.byref(i), pow_table, MAX_STEPS,
                    N.UNTIL_ALL_DONE, C.byref(rec), C.byref(kinds), C.byref(ps), C.byref(st),
                    C.byref(o)) == 0
                if not o.stepped:
                    break
                caught += round(o.reward / reward)
            assert st.finished == 1 and st.res.error == 0
        assert caught == known[rule], (rule, caught)
    # the committed integers are the Python statement's
    assert python_statistic(args, 1) == known[1]


def test_committed_statistics_are_the_python_statements():
    assert [python_statistic(("5x5", 2, 1, 1), r) for r in range(3)] == CAUGHT_5X5
    assert [python_statistic(("10x10", 3, 2, 2), r) for r in (0, 2)] == \
        [CAUGHT_10X10[0], CAUGHT_10X10[2]]


@pytest.mark.parametrize("until", [N.UNTIL_ALL_DONE, N.UNTIL_AGENT_DONE])
@pytest.mark.parametrize("ego", [0, 1])
def test_mixed_population_twin_replays_the_python_episode_harness(ego, until):
    """{H1, fixed, H3} through the host episode twins against PopulationAgents (the
    other agent of run_planning_episodes) on the product model: actions and
    counters seed for seed, and the Python model's step beside them."""
    from posggym_baselines_amd.planning import PopulationAgents
    lib = N.load()
    args = ("5x5", 2, 1, 1)
    prod = product(*args)
    grid = prod.pomcp_pp_grid()
    other = str(1 - ego)
    ENV = N.ENV_PREDATOR_PREY
    pow_table = (C.c_double * MAX_STEPS)(*[DISCOUNT ** t for t in range(MAX_STEPS)])
    pop = [PreyHeuristicPolicy.from_id(prod, other, H1), FixedDistributionPolicy(prod, other, *FIXED),
           PreyHeuristicPolicy.from_id(prod, other, H3)]
    rec, kinds = c_records(pop)
    assert [kinds.kind[k] for k in range(3)] == [N.POLICY_PP_HEURISTIC, 0, N.POLICY_PP_HEURISTIC]
    assert [kinds.param0[k] for k in range(3)] == [0, 0, 2]
    seen, lengths, differ = set(), [], 0
    for seed in range(90):
        py = pymodel(*args, seed=seed)
        s = py.sample_initial_state()
        agents = PopulationAgents(prod, seed, pop)
        agents.reset()
        st, ps, key = N.PomcpEpisodeState(), N.PomcpEpisodePopState(), C.c_uint64()
        assert lib.pomcp_host_episode_reset_pop(ENV, C.byref(grid), ego, seed, C.byref(rec),
                                                C.byref(st), C.byref(ps), C.byref(key)) == 0
        assert (st.v0, st.v1) == py.pack_words(s)
        k = restated_index(seed, 3)
        assert ps.policy_index == agents.policy_index == k
        seen.add(k)
        first = st.model_ctr
        for t in range(MAX_STEPS + 1):
            a_ego = scripted_ego(seed, t, 5)
            i = N.PomcpEpisodeStepIn(root_absorbing=0, action=a_ego, search_depth=2, num_sims=8,
                                     min_value=0.0, max_value=1.0)
            o = N.PomcpEpisodeStepOut()
            before = (st.v0, st.v1)
            assert lib.pomcp_host_episode_step_pop_kinds(
                ENV, C.byref(grid), ego, C.byref(i), pow_table, MAX_STEPS, until, C.byref(rec),
                C.byref(kinds), C.byref(ps), C.byref(st), C.byref(o)) == 0
            if not o.stepped:
                break
            a_oth = agents.act(other, before)            # from the state before the step
            where = (ego, seed, t)
            assert (o.ego_action, o.other_action) == (a_ego, a_oth), where
            if k != 1:      # the word decides among the rule's moves
                pi = pop[k].pi_from_state(before)
                assert a_oth == python_action(pi, word(seed, S_ENV_POLICY_BASE + int(other), t))
                differ += sum(p > 0.0 for p in pi) > 1
            ts = py.step(s, {str(ego): a_ego, other: a_oth})
            s = ts.state
            assert fhex(o.reward) == fhex(ts.rewards[str(ego)]), where
            assert (st.v0, st.v1) == py.pack_words(s), where
            assert st.policy_ctr == agents._ctr[other] == t + 1      # one word per action
            assert st.model_ctr == first + t + 1                     # one model draw per step
            assert st.finished == int(bool(ts.all_done) or t + 1 >= MAX_STEPS), where
        assert st.finished == 1 and st.res.error == 0
        lengths.append(st.res.len)
    assert seen == {0, 1, 2} and min(lengths) < max(lengths) and differ > 100


# ------------------------------------------------------------------ the codes
def test_kind_codes_of_the_host_entry_points():
    lib = N.load()
    pow_table = (C.c_double * MAX_STEPS)(*[DISCOUNT ** t for t in range(MAX_STEPS)])
    rec = N.PomcpEpisodePopulation()
    rec.num_policies = 1
    for a in range(5):
        rec.pi[0][a] = 0.2 if a < 4 else 0.0

    def step(env, grid, kind, p0, p1):
        st, ps, key = N.PomcpEpisodeState(), N.PomcpEpisodePopState(), C.c_uint64()
        assert lib.pomcp_host_episode_reset_pop(env, C.byref(grid), 0, 1, C.byref(rec), C.byref(st),
                                                C.byref(ps), C.byref(key)) == 0
        kinds = N.PomcpPolicyKinds()
        kinds.kind[0], kinds.param0[0], kinds.param1[0] = kind, p0, p1
        i = N.PomcpEpisodeStepIn(root_absorbing=0, action=0, search_depth=1, num_sims=1)
        o = N.PomcpEpisodeStepOut()
        return lib.pomcp_host_episode_step_pop_kinds(
            env, C.byref(grid), 0, C.byref(i), pow_table, MAX_STEPS, N.UNTIL_ALL_DONE, C.byref(rec),
            C.byref(kinds), C.byref(ps), C.byref(st), C.byref(o))

    K = N.POLICY_PP_HEURISTIC
    assert K == 5
    pp = product("5x5", 1, 1, 1).pomcp_pp_grid()
    for rule in range(3):
        assert step(N.ENV_PREDATOR_PREY, pp, K, rule, 0) == 0
    envs = [(N.ENV_DRIVING, DrivingModel().pomcp_grid()),
            (N.ENV_COOPERATIVE_REACHING, CooperativeReachingModel(size=5).pomcp_cr_grid()),
            (N.ENV_PURSUIT_EVASION, PursuitEvasionModel().pomcp_pe_grid())]
    for env, grid in envs:
        assert step(env, grid, K, 0, 0) == N.POMCP_E_UNSUPPORTED, env
    for bad in ((K, -1, 0), (K, 3, 0), (K, 0, 1), (K, 0, -1), (4, 0, 0), (2, 0, 0), (6, 0, 0)):
        assert step(N.ENV_PREDATOR_PREY, pp, *bad) == N.POMCP_E_INVALID, bad
        for env, grid in envs:
            assert step(env, grid, *bad) == N.POMCP_E_INVALID, (env, bad)
    # the other environments' kinds stay unsupported here
    assert step(N.ENV_PREDATOR_PREY, pp, N.POLICY_CR_GOAL, 0, 0) == N.POMCP_E_UNSUPPORTED
    assert step(N.ENV_PREDATOR_PREY, pp, N.POLICY_DRIVING_SHORTEST_PATH, 3, 2) == \
        N.POMCP_E_UNSUPPORTED
    # the rule twins
    w, d = (C.c_uint32 * 1)(0 | (12 << 7) | (6 << 21)), (C.c_uint32 * 1)(24)
    words, pi, act = (C.c_uint32 * 1)(7), (C.c_double * 5)(), (C.c_int32 * 1)()
    g = C.byref(pp)
    assert lib.pomcp_host_pp_policy_pi(g, 1, w, d, 0, 0, pi) == 0
    assert lib.pomcp_host_pp_policy_pi(g, 0, None, None, 0, 0, None) == 0
    assert lib.pomcp_host_pp_policy_actions(g, 1, w, d, 1, 2, words, act) == 0
    assert lib.pomcp_host_pp_policy_actions(g, 0, None, None, 0, 0, None, None) == 0
    for rule in (-1, 3):
        assert lib.pomcp_host_pp_policy_pi(g, 1, w, d, 0, rule, pi) == N.POMCP_E_INVALID
        assert lib.pomcp_host_pp_policy_actions(g, 1, w, d, 0, rule, words, act) == N.POMCP_E_INVALID
    for agent in (-1, 2):
        assert lib.pomcp_host_pp_policy_pi(g, 1, w, d, agent, 0, pi) == N.POMCP_E_INVALID
        assert lib.pomcp_host_pp_policy_actions(g, 1, w, d, agent, 0, words, act) == \
            N.POMCP_E_INVALID
    assert lib.pomcp_host_pp_policy_pi(None, 1, w, d, 0, 0, pi) == N.POMCP_E_INVALID
    assert lib.pomcp_host_pp_policy_pi(g, -1, w, d, 0, 0, pi) == N.POMCP_E_INVALID
    assert lib.pomcp_host_pp_policy_pi(g, 1, None, d, 0, 0, pi) == N.POMCP_E_INVALID
    assert lib.pomcp_host_pp_policy_pi(g, 1, w, None, 0, 0, pi) == N.POMCP_E_INVALID
    assert lib.pomcp_host_pp_policy_pi(g, 1, w, d, 0, 0, None) == N.POMCP_E_INVALID
    assert lib.pomcp_host_pp_policy_actions(None, 1, w, d, 0, 0, words, act) == N.POMCP_E_INVALID
    assert lib.pomcp_host_pp_policy_actions(g, -1, w, d, 0, 0, words, act) == N.POMCP_E_INVALID
    assert lib.pomcp_host_pp_policy_actions(g, 1, w, d, 0, 0, None, act) == N.POMCP_E_INVALID
    assert lib.pomcp_host_pp_policy_actions(g, 1, w, d, 0, 0, words, None) == N.POMCP_E_INVALID
    bad = N.PomcpPpGrid.from_buffer_copy(bytes(pp))
    bad.size = 8
    assert lib.pomcp_host_pp_policy_pi(C.byref(bad), 1, w, d, 0, 0, pi) == N.POMCP_E_INVALID


def test_enum_value_in_the_header(tmp_path):
    (tmp_path / "probe.c").write_text(
        '#include <stdio.h>\n#include "pomcp.h"\nint main(void){printf("%d %d %d\\n", '
        'POMCP_POLICY_PP_HEURISTIC, POMCP_ABI_VERSION, (int)sizeof(pomcp_policy_kinds));return 0;}')
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"),
                    str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")], check=True)
    out = subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout
    assert out.split() == [str(N.POLICY_PP_HEURISTIC), "7", str(C.sizeof(N.PomcpPolicyKinds))]
    assert N.load().pomcp_abi_version() == 7


# ------------------------------------------------- the header under sanitizers
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_policy_header_is_clean_under_the_sanitizers(tmp_path):
    """tests/native/pp_policy_sanitize.cpp walks the exhaustive 5x5 one-prey set and
    a sampled 10x10 three-prey set through the rule, its cumulative weights and
    the draw, and the host twins' refusals, compiled with ASan + UBSan and run as
    a program."""
    exe = tmp_path / "pp_policy_sanitize"
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas",
         "-I" + os.path.join(ROOT, "include"),
         os.path.join(ROOT, "tests", "native", "pp_policy_sanitize.cpp"), "-o", str(exe)],
        check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    states, sampled, checksum = (int(x) for x in r.stdout.split())
    assert states == 25 * 24 * 24 and sampled == 20000 and checksum > 0


# --------------------------------------------------------------------- guards
def stub_planner(model, ego="0"):
    return types.SimpleNamespace(engine=types.SimpleNamespace(
        model=model, A=5, ego=model.possible_agents.index(ego)))


def test_python_policy_and_its_refusals():
    from posggym_baselines_amd.planning import (IPOMCP, POTMMCP, BatchedINTMCP, MCTSConfig,
                                                OtherAgentMixturePolicy, POTMMCPMetaPolicy)
    from posggym_baselines_amd.planning.episodes import (check_population, episode_population,
                                                         population_kinds)
    from posggym_baselines_amd.planning.ipomcp import base_type_tables
    from posggym_baselines_amd.planning.policies import ego_policy_kinds
    from posggym_baselines_amd.planning.potmmcp import type_policy_tables
    from posggym_baselines_amd.planning.search_policy import SearchPolicyWrapper
    EGO, OTHER = "0", "1"
    pp, drv, cr = product("5x5", 2, 1, 1), DrivingModel(), CooperativeReachingModel(size=5)
    K = N.POLICY_PP_HEURISTIC
    assert PREDATOR_PREY_POLICY_IDS == {"PredatorPrey-v0/H1-v0": 0, "PredatorPrey-v0/H2-v0": 1,
                                        "PredatorPrey-v0/H3-v0": 2}
    pols = [PreyHeuristicPolicy.from_id(pp, OTHER, pid) for pid in H]
    assert [p.kind_params() for p in pols] == [(K, 0, 0), (K, 1, 0), (K, 2, 0)]
    assert all(is_reactive(p) for p in pols)
    with pytest.raises(KeyError):
        PreyHeuristicPolicy.from_id(pp, OTHER, "PredatorPrey-v0/H4-v0")
    for bad in (-1, 3, 1.5, True):
        with pytest.raises(ValueError):
            PreyHeuristicPolicy(pp, OTHER, "h", bad)
    with pytest.raises(NotImplementedError, match="PredatorPrey-v0"):
        PreyHeuristicPolicy.from_id(drv, OTHER, H1)
    with pytest.raises(NotImplementedError, match="PredatorPrey-v0"):
        PreyHeuristicPolicy.from_id(cr, OTHER, H1)
    with pytest.raises(NotImplementedError, match="CooperativeReaching-v0"):
        GoalHeuristicPolicy.from_id(pp, OTHER, "CooperativeReaching-v0/H1-v0")
    with pytest.raises(NotImplementedError):
        pols[0].get_value({})
    # the posggym interface: the state is the last observation
    s = pp.sample_initial_state()
    obs = pp.sample_initial_obs(s)[OTHER]
    ps = pols[0].get_next_state(None, obs, pols[0].get_initial_state())
    assert ps == {"obs": obs}
    pi = pols[0].get_pi(ps).probs
    assert list(pi) == [0, 1, 2, 3, 4] and [pi[a] for a in range(5)] == pols[0].pi_from_state(s)
    pols[0].rng = random.Random(3)
    assert pi[pols[0].sample_action(ps)] > 0.0
    # kinds of a population and of a mixture
    fixed = FixedDistributionPolicy(pp, OTHER, *FIXED)
    pop = [pols[0], fixed, pols[2]]
    want = [(K, 0, 0), (N.POLICY_FIXED, 0, 0), (K, 2, 0)]
    assert policy_kinds(pp, pop) == want
    assert population_kinds(stub_planner(pp), pop) == want
    assert check_population(pop) == [[0.2] * 5, FIXED[1], [0.2] * 5]
    ids, probs, mix = episode_population(stub_planner(pp), pop, [H3, "x"])
    assert ids == [H1, "never0", H3] and mix == [-1, -1, 0]
    with pytest.raises(NotImplementedError, match="acts in"):
        policy_kinds(drv, pop)
    with pytest.raises(NotImplementedError, match="Driving"):
        population_kinds(stub_planner(drv), pop)
    with pytest.raises(ValueError, match="planning agent"):
        population_kinds(stub_planner(pp, ego=OTHER), pop)
    cfg = MCTSConfig(discount=0.95, search_time_limit=0.1, c=1.0, truncated=False,
                     action_selection="pucb", pucb_exploration_fraction=0.25, known_bounds=None,
                     step_limit=None, epsilon=0.01, seed=0, state_belief_only=False, num_sims=8)
    mixture = OtherAgentMixturePolicy(pp, OTHER, {p.policy_id: p for p in pop})
    uniform = SearchPolicyWrapper(FixedDistributionPolicy.uniform(pp, EGO))
    tp = base_type_tables(pp, EGO, cfg, {OTHER: mixture}, uniform)
    assert tp.other_kinds == want
    assert list(tp.other_pi[0])[:5] == [0.2] * 5               # the placeholder row
    ego_pols = {"u": FixedDistributionPolicy.uniform(pp, EGO, "u")}
    meta = POTMMCPMetaPolicy(pp, EGO, ego_pols, {p.policy_id: {"u": 1.0} for p in pop})
    assert type_policy_tables(pp, EGO, meta, mixture).other_kinds == want
    # refused: as the ego's search policy or a meta-policy's member ...
    mine = PreyHeuristicPolicy.from_id(pp, EGO, H1)
    with pytest.raises(NotImplementedError, match="other agent only"):
        ego_policy_kinds(pp, EGO, [mine], "the search policy")
    fixed_mix = OtherAgentMixturePolicy(pp, OTHER, {"never0": fixed})
    with pytest.raises(NotImplementedError, match="other agent only"):
        IPOMCP(pp, EGO, cfg, {OTHER: fixed_mix}, SearchPolicyWrapper(mine))
    bad_meta = POTMMCPMetaPolicy(pp, EGO, {"h": mine}, {p.policy_id: {"h": 1.0} for p in pop})
    with pytest.raises(NotImplementedError, match="other agent only"):
        POTMMCP(pp, EGO, cfg, {OTHER: mixture}, bad_meta)
    # ... alone outside a mixture ...
    import dataclasses
    sbo = dataclasses.replace(cfg, state_belief_only=True)
    with pytest.raises(NotImplementedError, match="OtherAgentMixturePolicy"):
        base_type_tables(pp, EGO, sbo, {OTHER: pols[0]}, uniform)
    # ... belief 'action' accuracy with a reactive mixture ...
    from posggym_baselines_amd.planning import BeliefStatTracker, EpisodeEnvView
    stub = types.SimpleNamespace(config=cfg, other_agent_policies={OTHER: mixture}, model=pp,
                                 agent_id=EGO)
    with pytest.raises(NotImplementedError, match="per-particle"):
        BeliefStatTracker(stub, EpisodeEnvView(pp, EGO), stats_to_track=["action"])
    BeliefStatTracker(stub, EpisodeEnvView(pp, EGO), stats_to_track=["policy", "state"])
    # ... and I-NTMCP on this environment
    with pytest.raises(NotImplementedError, match="PredatorPrey-v0"):
        BatchedINTMCP(pp, EGO, cfg, 2, 8)


def test_population_agents_draw_with_the_word():
    from posggym_baselines_amd.planning import PopulationAgents
    pp = product("5x5", 2, 1, 1)
    pop = [PreyHeuristicPolicy.from_id(pp, "1", pid) for pid in H]
    seen = set()
    for seed in range(30):
        agents = PopulationAgents(pp, seed, pop)
        agents.reset()
        k = restated_index(seed, 3)
        assert agents.policy_index == k
        seen.add(k)
        pp.seed(seed)
        s = pp.sample_initial_state()
        for t in range(8):
            a = agents.act("1", s)
            assert agents._ctr["1"] == t + 1
            assert a == python_action(pop[k].pi_from_state(s), word(seed, S_ENV_POLICY_BASE + 1, t))
            s = pp.step(s, {"0": scripted_ego(seed, t, 5), "1": a}).state
        with pytest.raises(ValueError, match="acts on the state"):
            agents.act("1")
        with pytest.raises(ValueError, match="agent"):
            agents.act("0", s)
    assert seen == {0, 1, 2}
