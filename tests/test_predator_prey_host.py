"""PredatorPrey-v0 on the host: the model of csrc/predator_prey.h through its
host twins against the Python restatement (tests/golden/predator_prey_model.py),
hand-built states, the episode step twin with ``env_id = 4`` against the Python
episode loop, the header under the sanitizers and the guards."""
import ctypes as C
import itertools
import os
import random
import shutil
import subprocess
import sys

import pytest

from oracle.episode import ENV_TREE_BASE, fhex
from oracle.rng import S_MODEL, Streams
from posggym_baselines_amd import _native as N
from posggym_baselines_amd.envs import PredatorPreyModel, engine_model
from test_episode_population_host import DISCOUNT, scripted_ego, word

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from predator_prey_model import PredatorPreyModel as PyModel  # noqa: E402
from predator_prey_model import capture_reward  # noqa: E402

MAX_STEPS = 50
# every accepted combination: grid x num_prey x prey_strength x obs_dim
COMBOS = list(itertools.product(("5x5", "10x10"), (1, 2, 3), (1, 2), (1, 2)))
THIRD = capture_reward(3)


def product(grid="10x10", num_prey=3, prey_strength=2, obs_dim=2):
    return PredatorPreyModel(grid=grid, num_prey=num_prey, prey_strength=prey_strength,
                             obs_dim=obs_dim)


def twin_step(prod, words, actions, j):
    """pomcp_debug_pp_step_draw: (next words, reward, terminated, obs keys, rules, blocked)."""
    st = (C.c_uint32 * 2)(*words)
    act = (C.c_int32 * 2)(*actions)
    nxt, rew, term = (C.c_uint32 * 2)(), (C.c_double * 2)(), (C.c_int32 * 2)()
    keys, rules, blocked = (C.c_uint64 * 2)(), (C.c_int32 * 3)(), (C.c_int32 * 2)()
    rc = N.load().pomcp_debug_pp_step_draw(C.byref(prod.pomcp_pp_grid()), st, act, j, nxt, rew, term,
                                     keys, rules, blocked)
    assert rc == 0, rc
    assert rew[0] == rew[1] and term[0] == term[1]
    return (nxt[0], nxt[1]), rew[0], bool(term[0]), (keys[0], keys[1]), list(rules), list(blocked)


# ------------------------------------------------------------------ model twin
@pytest.mark.parametrize("grid,num_prey,strength,obs_dim", COMBOS)
def test_host_twin_equals_the_python_model_on_random_trajectories(grid, num_prey, strength,
                                                                  obs_dim):
    prod = product(grid, num_prey, strength, obs_dim)
    bytes_seen = [set() for _ in range(num_prey)]
    steps = ended = 0
    for seed in range(5000):
        if steps >= 3000 and all(len(b) == 256 for b in bytes_seen):
            break
        rng = random.Random(seed)
        py = PyModel(Streams(seed, ENV_TREE_BASE), grid, num_prey, strength, obs_dim)
        prod.seed(seed)
        s = py.sample_initial_state()
        w = prod.sample_initial_state()
        assert w == py.pack_words(s), seed
        assert py.unpack_words(w) == s
        assert prod.sample_initial_obs(w) == py.sample_initial_obs(s)
        for t in range(MAX_STEPS):
            acts = {"0": rng.randrange(5), "1": rng.randrange(5)}
            j = (word(seed, S_MODEL, py.streams.counters()[S_MODEL]) << 25) >> 32
            for k in range(num_prey):
                if s[2][k] is not None:
                    bytes_seen[k].add((j >> (8 * k)) & 255)
            ts, tw = py.step(s, acts), prod.step(w, acts)
            where = (seed, t)
            assert tw.state == py.pack_words(ts.state), where
            assert tw.observations == ts.observations, where
            assert {k: fhex(v) for k, v in tw.rewards.items()} == \
                {k: fhex(v) for k, v in ts.rewards.items()}, where
            assert tw.terminations == ts.terminations and tw.all_done == ts.all_done, where
            assert tw.truncations == {"0": False, "1": False}
            s, w = ts.state, tw.state
            steps += 1
            if ts.all_done:
                ended += 1
                break
    assert steps >= 3000
    assert all(len(b) == 256 for b in bytes_seen), [len(b) for b in bytes_seen]
    if strength == 1 and grid == "5x5":
        assert ended > 0


def toward(p, q):
    """the action that takes a predator on ``p`` closer to the cell ``q``"""
    dx, dy = q[0] - p[0], q[1] - p[1]
    if abs(dx) >= abs(dy) and dx != 0:
        return 3 if dx < 0 else 4
    return 0 if dy == 0 else (1 if dy < 0 else 2)


@pytest.mark.parametrize("grid,num_prey,strength,obs_dim", COMBOS)
def test_step_draw_twin_equals_the_python_model_with_its_facts(grid, num_prey, strength, obs_dim):
    """the twin with the draw given: the rule that decided every prey's move and
    the blocked predators are the Python model's"""
    prod = product(grid, num_prey, strength, obs_dim)
    rng = random.Random(7)
    py = PyModel(Streams(1, ENV_TREE_BASE), grid, num_prey, strength, obs_dim)
    rules_seen, blocked_seen = set(), set()
    for ep in range(60):
        s = py.sample_initial_state()
        for t in range(40):
            # (half of the moves head for a live prey, so that predators meet prey
            # on the 10x10 grid too)
            q = next(c for c in s[2] if c is not None)
            acts = tuple(toward(s[i], q) if rng.random() < 0.5 else rng.randrange(5)
                         for i in range(2))
            j = rng.randrange(1 << 25)
            facts = {"rules": [0, 0, 0], "blocked_order": [0, 0], "captures": 0}
            nxt, n = py.step_draw(s, acts, j, facts)
            got, r, term, keys, rules, blocked = twin_step(prod, py.pack_words(s), acts, j)
            assert got == py.pack_words(nxt), (ep, t)
            assert fhex(r) == fhex(n * py.reward)
            assert term == all(q is None for q in nxt[2])
            assert keys == tuple(py.pack_obs(py._obs(nxt, i)) for i in range(2))
            live = [k for k in range(3) if s[2][k] is not None]
            assert [rules[k] for k in range(3) if k not in live] == [-1] * (3 - len(live))
            for rule in range(3):
                assert sum(rules[k] == rule for k in live) == facts["rules"][rule]
            assert sum(blocked) == sum(facts["blocked_order"])
            assert facts["blocked_order"][1 - (j >> 24)] == 0
            rules_seen.update(rules[k] for k in live)
            blocked_seen.update((j >> 24, i) for i in range(2) if blocked[i])
            s = nxt
            if term:
                break
    # (at strength 1 a prey is caught in the step a predator comes beside it, so
    # with obs_dim 1 no prey starts a step seeing one -- but for the 5x5 grid's
    # initial states, where a prey may start beside a predator's start cell)
    fled = not (strength == 1 and obs_dim == 1 and grid == "10x10")
    assert ({0, 2} if fled else {2}) <= rules_seen and len(blocked_seen) == 4
    if num_prey > 1:
        assert rules_seen == ({0, 1, 2} if fled else {1, 2})


@pytest.mark.parametrize("grid,num_prey,strength,obs_dim", COMBOS)
def test_sample_agent_initial_state_agrees_on_initial_observations(grid, num_prey, strength,
                                                                   obs_dim):
    lib = N.load()
    prod = product(grid, num_prey, strength, obs_dim)
    g = prod.pomcp_pp_grid()
    for seed in range(80):
        py = PyModel(Streams(seed, ENV_TREE_BASE), grid, num_prey, strength, obs_dim)
        s = py.sample_initial_state()
        for agent in ("0", "1"):
            obs = py.sample_initial_obs(s)[agent]
            ctr = C.c_uint32(py.streams.counters()[S_MODEL])
            out = (C.c_uint32 * 2)()
            assert lib.pomcp_pp_sample_agent_initial_state(
                C.byref(g), int(agent), py.pack_obs(obs), seed, ENV_TREE_BASE, C.byref(ctr),
                out) == 0
            got = py.sample_agent_initial_state(agent, obs)
            assert (out[0], out[1]) == py.pack_words(got), (seed, agent)
            assert ctr.value == py.streams.counters()[S_MODEL]
            assert got[int(agent)] == s[int(agent)]     # the start cell from the walls alone
    # inconsistent: walls no start cell has (a lone wall cell); bits beyond the window
    out, ctr = (C.c_uint32 * 2)(), C.c_uint32(0)
    n = (2 * obs_dim + 1) ** 2 - 1
    for bad in (1 << (2 * (n // 2)), 1 << (2 * n)):
        assert lib.pomcp_pp_sample_agent_initial_state(C.byref(g), 0, bad, 0, 0, C.byref(ctr),
                                                       out) == N.POMCP_E_INVALID
    with pytest.raises(ValueError):
        py.sample_agent_initial_state("0", prod.obs_from_key(1 << (2 * (n // 2))))


# ---------------------------------------------------------- hand-built states
def state(p0, p1, *prey):
    return (p0, p1, tuple(prey) + (None,) * (3 - len(prey)))


def both(py, prod, s, acts, j):
    """the step on both sides; returns (next state, reward, terminated, blocked)"""
    nxt, n = py.step_draw(s, acts, j, {"rules": [0, 0, 0], "blocked_order": [0, 0], "captures": 0})
    got, r, term, _, _, blocked = twin_step(prod, py.pack_words(s), acts, j)
    assert got == py.pack_words(nxt)
    assert fhex(r) == fhex(n * py.reward)
    return nxt, r, term, blocked


def models(grid, num_prey, strength, obs_dim=2):
    return (PyModel(Streams(0, 0), grid, num_prey, strength, obs_dim),
            product(grid, num_prey, strength, obs_dim))


def test_capture_takes_two_predators_at_strength_two_and_one_at_strength_one():
    # no predator within obs_dim = 1 of the prey, so tie byte 0 has it stay in its corner
    s = state((0, 2), (2, 0), (0, 0))
    py, prod = models("5x5", 1, 2, 1)
    nxt, r, term, _ = both(py, prod, s, (UP := 1, LEFT := 3), 0)
    assert nxt == state((0, 1), (1, 0), None) and r == 1.0 and term
    nxt, r, term, _ = both(py, prod, s, (UP, 0), 0)           # one predator beside it: none
    assert nxt[2][0] is not None and r == 0.0 and not term
    py, prod = models("5x5", 1, 1, 1)
    nxt, r, term, _ = both(py, prod, s, (UP, 0), 0)           # strength 1: caught
    assert nxt == state((0, 1), (2, 0), None) and r == 1.0 and term


def test_two_prey_caught_in_one_step_pay_two_thirds():
    py, prod = models("10x10", 3, 1, 1)
    # prey in two corners, each with a predator two cells away; the third far off
    s = state((0, 2), (9, 2), (0, 0), (9, 0), (5, 9))
    nxt, r, term, _ = both(py, prod, s, (1, 1), 0)
    assert nxt[2][0] is None and nxt[2][1] is None and nxt[2][2] is not None
    assert fhex(r) == fhex(2 * THIRD) == fhex(0.6666666865348816) and not term
    assert py.pack_words(nxt)[0] >> 21 == 3


def test_predator_blocked_by_a_prey_the_other_predator_and_the_edge_in_both_orders():
    py, prod = models("10x10", 1, 2, 1)
    for order in (0, 1):
        j = order << 24
        # the edge
        nxt, _, _, blocked = both(py, prod, state((0, 0), (9, 9), (5, 5)), (3, 4), j)
        assert nxt[:2] == ((0, 0), (9, 9)) and blocked == [1, 1]
        # a prey that stays: cornered between the predators, it has no other candidate
        nxt, _, _, blocked = both(py, prod, state((1, 0), (0, 1), (0, 0)), (3, 0), j)
        assert nxt[0] == (1, 0) and blocked == [1, 0]
    # the other predator's current cell: predator 0 moves onto the cell predator 1
    # leaves -- free when predator 1 went first, taken when predator 0 goes first
    s = state((3, 3), (4, 3), (8, 8))
    nxt, _, _, blocked = both(py, prod, s, (4, 4), 0)
    assert nxt[:2] == ((3, 3), (5, 3)) and blocked == [1, 0]
    nxt, _, _, blocked = both(py, prod, s, (4, 4), 1 << 24)
    assert nxt[:2] == ((4, 3), (5, 3)) and blocked == [0, 0]
    s = state((4, 3), (3, 3), (8, 8))
    nxt, _, _, blocked = both(py, prod, s, (4, 4), 1 << 24)
    assert nxt[:2] == ((5, 3), (3, 3)) and blocked == [0, 1]


def test_a_cornered_prey_has_the_single_candidate_stay():
    py, prod = models("5x5", 1, 2, 1)
    s = state((1, 0), (0, 1), (0, 0))
    for byte in (0, 127, 255):
        nxt, n = py.step_draw(s, (0, 0), byte, {"rules": [0, 0, 0], "blocked_order": [0, 0],
                                                "captures": 0})
        # (it stayed, and with two predators beside it was caught there)
        assert nxt == state((1, 0), (0, 1), None) and n == 1
        assert twin_step(prod, py.pack_words(s), (0, 0), byte)[0] == py.pack_words(nxt)
    # uncaught: strength 2 with one predator beside it and the other blocking diagonally
    py, prod = models("5x5", 2, 2, 1)
    s = state((1, 0), (4, 4), (0, 0), (0, 1))
    for byte in (0, 255):
        nxt, _, _, _ = both(py, prod, s, (0, 0), byte)
        assert nxt[2][0] == (0, 0)


@pytest.mark.parametrize("num_prey", [1, 2, 3])
def test_done_is_the_caught_mask_of_the_words_alone(num_prey):
    py, prod = models("10x10", num_prey, 1)
    spots = ((3, 3), (5, 5), (7, 7))
    for mask in range(1 << num_prey):
        prey = [None if (mask >> k) & 1 else spots[k] for k in range(num_prey)]
        s = state((0, 0), (9, 9), *prey)
        w = py.pack_words(s)
        assert (w[0] >> 21) & 7 == mask | (7 & ~((1 << num_prey) - 1))
        if mask == (1 << num_prey) - 1:
            continue        # (a terminal state is not stepped)
        _, _, term, _, _, _ = twin_step(prod, w, (0, 0), 0)
        assert not term
    # stepping a state in which the last prey is caught terminates; the flag is bit 21..23 == 7
    s = state((0, 2), (2, 0), (0, 0))
    py, prod = models("5x5", 1, 1, 1)
    got, _, term, _, _, _ = twin_step(prod, py.pack_words(s), (1, 0), 0)
    assert term and (got[0] >> 21) & 7 == 7


def test_host_twins_refuse_words_that_are_no_state():
    py, prod = models("5x5", 2, 1)
    good = py.pack_words(state((0, 0), (4, 4), (2, 2), (2, 3)))
    twin_step(prod, good, (0, 0), 0)
    st_bad = [
        (good[0] | (1 << 24), good[1]),               # bits beyond the fields
        (good[0], good[1] | (5 << 7)),                # the absent prey has a cell
        ((good[0] & ~127) | 25, good[1]),             # predator 0 off the grid
        ((good[0] & ~127) | 24, good[1]),             # both predators on one cell
        (good[0] & ~(4 << 21), good[1]),              # the absent prey not in the mask
    ]
    lib = N.load()
    for w in st_bad:
        st, keys = (C.c_uint32 * 2)(*w), (C.c_uint64 * 2)()
        assert lib.pomcp_pp_obs(C.byref(prod.pomcp_pp_grid()), st, keys) == N.POMCP_E_INVALID, w
    act = (C.c_int32 * 2)(0, 5)
    st = (C.c_uint32 * 2)(*good)
    nxt, rew, term, keys = (C.c_uint32 * 2)(), (C.c_double * 2)(), (C.c_int32 * 2)(), \
        (C.c_uint64 * 2)()
    g = C.byref(prod.pomcp_pp_grid())
    assert lib.pomcp_debug_pp_step_draw(g, st, act, 0, nxt, rew, term, keys, None, None) == \
        N.POMCP_E_INVALID
    act = (C.c_int32 * 2)(0, 0)
    assert lib.pomcp_debug_pp_step_draw(g, st, act, 1 << 25, nxt, rew, term, keys, None, None) == \
        N.POMCP_E_INVALID


# ---------------------------------------------------------- episode step twin
@pytest.mark.parametrize("until", [N.UNTIL_ALL_DONE, N.UNTIL_AGENT_DONE])
@pytest.mark.parametrize("ego", [0, 1])
def test_episode_twin_replays_the_python_episode_loop(ego, until):
    lib = N.load()
    args = ("5x5", 2, 1, 1)         # (captures, early ends and full-length episodes)
    prod = product(*args)
    grid = prod.pomcp_pp_grid()
    other = str(1 - ego)
    ENV = N.ENV_PREDATOR_PREY
    pow_table = (C.c_double * MAX_STEPS)(*[DISCOUNT ** t for t in range(MAX_STEPS)])
    lengths, returns = [], set()
    for seed in range(60):
        py = PyModel(Streams(seed, ENV_TREE_BASE), *args)
        s = py.sample_initial_state()
        st, key = N.PomcpEpisodeState(), C.c_uint64()
        assert lib.pomcp_host_episode_reset(ENV, C.byref(grid), ego, seed, C.byref(st),
                                            C.byref(key)) == 0
        assert key.value == py.pack_obs(py.sample_initial_obs(s)[str(ego)])
        assert (st.v0, st.v1) == py.pack_words(s)
        first = py.streams.counters()[S_MODEL]
        for t in range(MAX_STEPS + 1):
            a_ego = scripted_ego(seed, t, 5)
            i = N.PomcpEpisodeStepIn(root_absorbing=0, action=a_ego, search_depth=2, num_sims=8,
                                     min_value=0.0, max_value=1.0)
            o = N.PomcpEpisodeStepOut()
            assert lib.pomcp_host_episode_step(ENV, C.byref(grid), ego, C.byref(i), pow_table,
                                               MAX_STEPS, until, C.byref(st), C.byref(o)) == 0
            if not o.stepped:
                break
            a_oth = (word(seed, 40 + int(other), t) * 5) >> 32
            where = (ego, seed, t)
            assert (o.ego_action, o.other_action) == (a_ego, a_oth), where
            ts = py.step(s, {str(ego): a_ego, other: a_oth})
            s = ts.state
            assert fhex(o.reward) == fhex(ts.rewards[str(ego)]), where
            assert o.obs_key == py.pack_obs(ts.observations[str(ego)]), where
            assert (st.v0, st.v1) == py.pack_words(s), where
            assert st.model_ctr == first + t + 1                 # one model draw per step
            assert st.finished == int(bool(ts.all_done) or t + 1 >= MAX_STEPS), where
        assert st.finished == 1 and st.res.error == 0
        lengths.append(st.res.len)
        returns.add(st.res.ret)
    assert min(lengths) < max(lengths) == MAX_STEPS
    assert {0.5, 1.0} <= returns <= {0.0, 0.5, 1.0}


# ------------------------------------------------- the header under sanitizers
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_model_header_is_clean_under_the_sanitizers(tmp_path):
    """tests/native/predator_prey_sanitize.cpp drives predator_prey.h over the
    hand-built states above and a random walk on every accepted description,
    and the host twins pomcp_pp_* of host_api.cpp (one translation unit with
    it) over episodes of their own and their refusals, compiled with ASan +
    UBSan and run as a program."""
    exe = tmp_path / "predator_prey_sanitize"
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas",
         "-I" + os.path.join(ROOT, "include"),
         os.path.join(ROOT, "tests", "native", "predator_prey_sanitize.cpp"), "-o", str(exe)],
        check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    steps, captures, checksum = (int(x) for x in r.stdout.split())
    assert steps == 24 * 200 * 50 and captures > 0 and checksum > 0


# --------------------------------------------------------------------- guards
class _Spec:
    def __init__(self, id, **kwargs):
        self.id, self.kwargs = id, kwargs


class _Model:
    possible_agents = ("0", "1")

    def __init__(self, id, **kwargs):
        self.spec = _Spec(id, **kwargs)


def test_engine_model_takes_the_registration_and_refuses_other_kwargs():
    m = engine_model(_Model("PredatorPrey-v0"))
    assert isinstance(m, PredatorPreyModel)
    assert (m.grid, m.size, m.num_predators, m.num_prey, m.cooperative, m.prey_strength,
            m.obs_dim) == ("10x10", 10, 2, 3, True, 2, 2)
    assert m.spec.max_episode_steps == 50 and m.action_spaces["0"].n == 5
    assert fhex(m.capture_reward) == fhex(0.3333333432674408)
    # the reference's env_kwargs.yaml
    m = engine_model(_Model("PredatorPrey-v0", grid="10x10", num_predators=2, num_prey=3,
                            cooperative=True, prey_strength=2, obs_dim=2))
    assert (m.size, m.num_prey, m.prey_strength, m.obs_dim) == (10, 3, 2, 2)
    m = engine_model(_Model("PredatorPrey-v0", grid="5x5", num_prey=1, prey_strength=1, obs_dim=1,
                            render_mode=None))
    assert (m.size, m.num_prey, m.prey_strength, m.obs_dim) == (5, 1, 1, 1)
    for bad in (dict(grid="15x15"), dict(grid="5x5Blocks"), dict(grid="10x10Blocks"),
                dict(grid=10), dict(num_predators=3), dict(num_predators=4), dict(num_prey=0),
                dict(num_prey=4), dict(num_prey=1.5), dict(cooperative=False),
                dict(prey_strength=0), dict(prey_strength=3), dict(obs_dim=0), dict(obs_dim=3),
                dict(obs_dim=(3, 1, 1)), dict(size=5), dict(num_agents=2)):
        with pytest.raises(NotImplementedError):
            engine_model(_Model("PredatorPrey-v0", **bad))


def test_reactive_kinds_are_refused_on_the_environment():
    lib = N.load()
    prod = product("5x5", 1, 1, 1)
    rec = N.PomcpEpisodePopulation()
    rec.num_policies = 1
    for a in range(5):
        rec.pi[0][a] = 0.2
    pow_table = (C.c_double * MAX_STEPS)(*[DISCOUNT ** t for t in range(MAX_STEPS)])
    grid = prod.pomcp_pp_grid()

    def step(kind, p0, p1):
        st, ps, key = N.PomcpEpisodeState(), N.PomcpEpisodePopState(), C.c_uint64()
        assert lib.pomcp_host_episode_reset_pop(N.ENV_PREDATOR_PREY, C.byref(grid), 0, 1,
                                                C.byref(rec), C.byref(st), C.byref(ps),
                                                C.byref(key)) == 0
        kinds = N.PomcpPolicyKinds()
        kinds.kind[0], kinds.param0[0], kinds.param1[0] = kind, p0, p1
        i = N.PomcpEpisodeStepIn(root_absorbing=0, action=0, search_depth=1, num_sims=1)
        o = N.PomcpEpisodeStepOut()
        return lib.pomcp_host_episode_step_pop_kinds(
            N.ENV_PREDATOR_PREY, C.byref(grid), 0, C.byref(i), pow_table, MAX_STEPS,
            N.UNTIL_ALL_DONE, C.byref(rec), C.byref(kinds), C.byref(ps), C.byref(st), C.byref(o))

    assert step(N.POLICY_FIXED, 0, 0) == 0
    assert step(N.POLICY_CR_GOAL, 0, 0) == N.POMCP_E_UNSUPPORTED
    assert step(N.POLICY_DRIVING_SHORTEST_PATH, 3, 2) == N.POMCP_E_UNSUPPORTED


def test_intmcp_refuses_the_environment_by_name():
    from posggym_baselines_amd.planning import INTMCP, BatchedINTMCP, MCTSConfig
    cfg = MCTSConfig(discount=0.95, c=1.4, truncated=False, search_time_limit=0.1,
                     action_selection="ucb", num_sims=8)
    with pytest.raises(NotImplementedError, match="PredatorPrey-v0"):
        INTMCP(product(), "0", cfg, 1)
    with pytest.raises(NotImplementedError, match="PredatorPrey-v0"):
        INTMCP.initialize(_Model("PredatorPrey-v0"), "0", cfg, nesting_level=1)
    with pytest.raises(NotImplementedError, match="PredatorPrey-v0"):
        BatchedINTMCP(product(), "0", cfg, 2, 8)


def test_pomcp_create_refuses_the_environment_without_its_description():
    """(validation comes before any device is opened)"""
    lib = N.load()
    c = N.PomcpConfig()
    c.abi_version = N.POMCP_ABI_VERSION
    c.env_id = N.ENV_PREDATOR_PREY
    c.num_agents, c.num_actions = 2, 5
    ctx = C.c_void_p()
    assert lib.pomcp_create(C.byref(c), 0, None, C.byref(ctx)) == N.POMCP_E_UNSUPPORTED
    assert not ctx.value
    g = product().pomcp_pp_grid()
    void = lambda d: C.cast(C.byref(d), C.c_void_p)
    assert lib.pomcp_create_env(C.byref(c), void(g), C.sizeof(g) - 8, 0, None,
                                C.byref(ctx)) == N.POMCP_E_INVALID
    # (the other additive description's size is not this environment's)
    assert lib.pomcp_create_env(C.byref(c), void(g), C.sizeof(N.PomcpCrGrid), 0, None,
                                C.byref(ctx)) == N.POMCP_E_INVALID
    assert lib.pomcp_create_env(C.byref(c), None, C.sizeof(g), 0, None,
                                C.byref(ctx)) == N.POMCP_E_INVALID
    for field, value in (("size", 8), ("num_prey", 4), ("num_prey", 0), ("prey_strength", 3),
                         ("obs_dim", 0), ("obs_dim", 3), ("capture_reward", 1.0 / 3.0)):
        bad = N.PomcpPpGrid.from_buffer_copy(bytes(g))
        setattr(bad, field, value)
        assert lib.pomcp_create_env(C.byref(c), void(bad), C.sizeof(bad), 0, None,
                                    C.byref(ctx)) == N.POMCP_E_INVALID, field
    bad = N.PomcpPpGrid.from_buffer_copy(bytes(g))
    bad.start[1][0] = 4                                 # not the edge cell at x = S / 2
    assert lib.pomcp_create_env(C.byref(c), void(bad), C.sizeof(bad), 0, None,
                                C.byref(ctx)) == N.POMCP_E_INVALID
    assert not ctx.value


def test_abi_and_struct_sizes(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "pomcp.h"', "int main(void){",
             'printf("config %zu\\n", sizeof(pomcp_config));',
             'printf("pp %zu\\n", sizeof(pomcp_pp_grid));']
    for f, *_ in N.PomcpPpGrid._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(pomcp_pp_grid, {f}));')
    lines.append('printf("ids %d %d\\n", POMCP_ENV_PREDATOR_PREY, POMCP_ABI_VERSION); return 0;}')
    (tmp_path / "probe.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"),
                    str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")], check=True)
    out = subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True,
                         text=True).stdout.split("\n")
    vals = dict(line.split(" ", 1) for line in out if line)
    assert int(vals["config"]) == C.sizeof(N.PomcpConfig) == 3880
    assert int(vals["pp"]) == C.sizeof(N.PomcpPpGrid) == 40
    for f, *_ in N.PomcpPpGrid._fields_:
        assert int(vals[f]) == getattr(N.PomcpPpGrid, f).offset
    assert vals["ids"] == f"{N.ENV_PREDATOR_PREY} 7" == "4 7"
    assert N.load().pomcp_abi_version() == 7
