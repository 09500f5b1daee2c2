"""k_update's rejection reinvigoration (pomcp_kernels.hip; mcts.py:651-700,
belief.py:145-194) on every path it can take, device against the CPU oracle,
bit for bit.

Each directed case loads a caller-supplied parent belief into a fresh tree
(``pomcp_set_root_belief``; the oracle holds the same list), searches 64
simulations, updates with an observation the test chooses -- *real* (stepped
from the belief's first particle) or *impossible* (from an unrelated
environment state, so no particle produces it) -- searches, updates once more
with a real observation and searches again.  After each update the new root
belief is compared row by row ((t, v0, v1), insertion order: a failure names
the first wrong slot) and after each search the full record: the later
searches see a wrong stream counter or a stale LDS page of the three streams
the sampler advances, the rows see everything else.

Before anything runs on the device every case asserts, from the oracle's
recorder (``OraclePOMCP.reinvigorations``: need, tries, accepted,
rejected_total, parent_size), that its reinvigoration is of the path class it
is meant to pin -- so a case cannot quietly come to test nothing.  The path
classes and the k_update branches they take:

* tries: 64 per pass, the last pass partial when ``limit`` is no multiple of
  64 (``valid``), ``limit = factor * need`` need not be an integer;
* accepted particles to [n, n + need), rejected ones to [n + need, n + 2 need)
  capped at ``need`` (``nrej``), then ``fill = min(need - got, nrej)`` rejected
  particles copied over the gap 64 per pass;
* ``need <= 0`` and an absorbing child: no sampling, no draw;
* ``n + 2 need`` beyond the belief region: POMCP_E_ARENA for that tree alone.
"""
import functools
import math
import os
import random

import numpy as np
import pytest

from gpu_util import product_config, product_model, stats_record
from oracle.envs import make_model
from oracle.episode import ENV_TREE_BASE, run_episode
from oracle.rng import S_ENV_POLICY_BASE, Streams
from oracle.run import make_oracle, oracle_record

pytestmark = pytest.mark.gpu

S = 64   # simulations per search
DRIVING, PE = "Driving-v1", "PursuitEvasion-v1"
BASE_CFG = dict(discount=0.95, c=math.sqrt(2), truncated=False, action_selection="ucb",
                pucb_exploration_fraction=0.25, known_bounds=None, step_limit=None, epsilon=0.92,
                seed=0, state_belief_only=True)


@pytest.fixture(autouse=True, params=["lane", "wave"])
def search_kernel(request, monkeypatch):
    """Both search kernels feed the update (their particle logs, their RNG
    pages): every test runs after k_search and after k_search_lds."""
    monkeypatch.setenv("POMCP_SEARCH_KERNEL", request.param)
    return request.param


# ------------------------------------------------------------------ oracle side
def case_cfg(stl, factor, prop=1.0 / 16, seed=0):
    return dict(BASE_CFG, search_time_limit=stl, extra_particles_prop=prop,
                reinvigoration_sample_limit_factor=factor, seed=seed)


def n_target_of(cfg):
    """config.py:47-48: ceil(100 * search_time_limit) + ceil(prop * num_particles)."""
    num = math.ceil(100 * cfg["search_time_limit"])
    return num + math.ceil(num * cfg["extra_particles_prop"])


@functools.lru_cache(maxsize=None)
def donor_particles(env, ego, env_seed):
    """A few hundred (state, t = 1) particles: a donor oracle's initial belief."""
    d = make_oracle(case_cfg(3.0, 4.0), 8, ego=ego, tree=9, env=env)
    run_episode(lambda obs: (d.update(None, obs), 0)[1], env_seed, ego=ego, max_steps=1, env=env)
    return tuple(d.belief[d.root])


def parent_belief(env, ego, length, donors=(55,), rng_seed=1):
    """`length` particles drawn (seeded) from the donors' initial beliefs; more
    than one donor mixes particles of different initial observations."""
    pool = [q for s in donors for q in donor_particles(env, ego, s)]
    rng = random.Random(rng_seed)
    return [pool[rng.randrange(len(pool))] for _ in range(length)]


@functools.lru_cache(maxsize=None)
def late_belief(env, ego, env_seed):
    """The last non-absorbing root belief of a short oracle episode: particles
    one step away from the episode's end."""
    p = make_oracle(case_cfg(0.3, 4.0), 32, ego=ego, tree=3, env=env)
    beliefs = []

    def step(obs):
        a = p.step(obs)
        if not p.on_abs[p.root]:
            beliefs.append(tuple(p.belief[p.root]))
        return a

    run_episode(step, env_seed, ego=ego, max_steps=40, env=env)
    return beliefs[-1]


def impossible_obs(env, ego, env_seed=991, steps=5):
    """The ego's observation `steps` steps into an unrelated episode."""
    es = Streams(env_seed, ENV_TREE_BASE)
    m = make_model(env, es)
    st = m.sample_initial_state()
    for _ in range(steps):
        ts = m.step(st, {i: es.randint(S_ENV_POLICY_BASE + int(i), m.action_spaces[i].n)
                         for i in m.possible_agents})
        st = ts.state
    return ts.observations[ego]


def scenario(env, ego, cfg, parts, obs_kind, tree=0, other_action=0):
    """The oracle's run of the recipe: rows0 (the loaded belief), rec0 (the first
    search) and two steps {action, key, cls, rows, rec}: the update's inputs,
    what the recorder saw, the new root belief and the search after it."""
    p = make_oracle(cfg, S, ego=ego, tree=tree, env=env)
    node = p._new_obs_node(parts[0][1], 0)
    p.belief[node] = list(parts)
    p.root = node
    world = make_model(env, Streams(77, ENV_TREE_BASE))   # its draws are not the planner's
    other = [i for i in p.model.possible_agents if i != ego][0]

    def rows():
        return [(t,) + tuple(p.model.pack_words(st)) for st, t in p.belief[p.root]]

    def record(a):
        p.stats["searched"] = True
        p.stats["belief"] = list(p.belief[p.root])
        return oracle_record(p, True, a)

    out = {"rows0": rows(), "steps": []}
    p.stats = {}
    a = p.get_action()
    out["rec0"] = record(a)
    for k in range(2):
        if k == 0 and obs_kind == "impossible":
            obs = impossible_obs(env, ego)
        elif k == 0 and obs_kind == "terminal":
            # an observation whose child under `a` the search marked absorbing
            an = p.on_block[p.root] * p.A + a
            obs = next(ts.observations[ego] for st, _ in p.belief[p.root] for oa in range(p.A)
                       for ts in [world.step(st, {ego: a, other: oa})]
                       if p.on_abs[p.children.get((an, p.model.pack_obs(ts.observations[ego])), 0)])
        else:
            first = p.belief[p.root][0][0]
            obs = world.step(first, {ego: a, other: other_action}).observations[ego]
        del p.reinvigorations[:]
        p.stats = {}
        p.update(a, obs)
        cls = list(p.reinvigorations)
        a2 = p.get_action()
        out["steps"].append({"action": a, "key": p.model.pack_obs(obs), "cls": cls, "rows": rows(),
                             "absorbing": bool(p.on_abs[p.root]), "rec": record(a2)})
        a = a2
    return out


# name: (env, ego, search_time_limit, extra_particles_prop, factor, n_target, parent rows,
#        donor env seeds, observation, class the oracle's recorder must report)
CASES = {
    # 133 passes, the last partial (8500 = 132 * 64 + 52); nrej capped at need;
    # fill = 2125: 34 fill passes; uniform_int(word, 70001) into rbel
    "zero_accept_large": (DRIVING, "0", 20.0, 1 / 16, 4.0, 2125, 70001, (55,), "impossible",
                          lambda c: c == (2125, 8500, 0, 8500, 70001)),
    "all_accepted_large_parent": (DRIVING, "0", 20.0, 1 / 16, 4.0, 2125, 70001, (55,), "real",
                                  lambda c: c[0] == c[1] == c[2] and c[0] > 64 and c[3] == 0
                                  and c[4] > 65536),
    # need at the wave size, limit = 2.5 * need: 157.5, 160, 162.5
    "need_63": (DRIVING, "0", 0.63, 0.0, 2.5, 63, 3, (55,), "impossible",
                lambda c: c == (63, 158, 0, 158, 3)),
    "need_64": (DRIVING, "0", 0.64, 0.0, 2.5, 64, 3, (55,), "impossible",
                lambda c: c == (64, 160, 0, 160, 3)),
    "need_65": (DRIVING, "0", 0.65, 0.0, 2.5, 65, 3, (55,), "impossible",
                lambda c: c == (65, 163, 0, 163, 3)),
    # factor 1.0: tries == need, some accepted: fill = need - accepted
    "minimum_factor": (PE, "1", 1.0, 1 / 16, 1.0, 107, 200, (55,), "real",
                       lambda c: c[1] == c[0] and 0 < c[2] < c[0] and c[3] == c[0] - c[2]),
    # more rejects than `need` (the cap) and a fill of more than one pass
    "capped_rejects_long_fill": (PE, "0", 3.0, 1 / 16, 4.0, 319, 300, (55, 56, 57), "real",
                                 lambda c: c[2] < c[0] and c[3] > c[0] and c[0] - c[2] > 64),
    # ego "1": the other agent's actions come from stream / page c_act0 / r_act0
    "other_stream_zero_accept": (DRIVING, "1", 1.0, 1 / 16, 2.5, 107, 200, (55,), "impossible",
                                 lambda c: c == (107, 268, 0, 268, 200)),
    "other_stream_partial": (DRIVING, "1", 1.0, 1 / 16, 1.0, 107, 200, (55, 56), "real",
                             lambda c: c[1] == c[0] and 0 < c[2] < c[0]),
    # the child already holds n_target particles: nothing sampled, nothing drawn
    "nothing_to_do": (DRIVING, "0", 0.1, 1 / 16, 4.0, 11, 50, (55,), "real",
                      lambda c: c[0] <= 0 and c[1:4] == (0, 0, 0)),
}


@functools.lru_cache(maxsize=None)
def case_scenario(name):
    env, ego, stl, prop, factor, n_target, length, donors, obs_kind, _ = CASES[name]
    cfg = case_cfg(stl, factor, prop)
    assert n_target_of(cfg) == n_target
    return cfg, scenario(env, ego, cfg, parent_belief(env, ego, length, donors), obs_kind)


def check_class(name, sc):
    """The first update's reinvigoration is of the case's path class; neither
    root turned absorbing (both later searches run)."""
    (cls,) = sc["steps"][0]["cls"]
    assert CASES[name][9](cls), (name, cls)
    assert not sc["steps"][0]["absorbing"] and not sc["steps"][1]["absorbing"], name
    assert sc["steps"][1]["rec"]["num_sims"] == S


# ------------------------------------------------------------------ device side
def assert_rows(got, exp, what):
    got = np.asarray(got, dtype=np.int64).reshape(-1, 3)
    exp = np.asarray(exp, dtype=np.int64).reshape(-1, 3)
    assert len(got) == len(exp), f"{what}: belief_size {len(got)} != {len(exp)}"
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} wrong belief slots, the first at {bad[0]}: "
                           f"{got[bad[0]].tolist()} != {exp[bad[0]].tolist()}")


def make_engine(env, ego, cfg, scens, max_belief=None):
    """One BatchedPOMCP, tree b holding scens[b]'s parent belief."""
    from posggym_baselines_amd.planning import BatchedPOMCP
    from posggym_baselines_amd.planning.engine import plan_capacities
    model = product_model(env)
    config = product_config(cfg, S)
    A = model.action_spaces[ego].n
    caps = plan_capacities(config, model.spec.max_episode_steps, S, 3, reroot=True, num_actions=A)
    if max_belief is None:
        # the parent belief (at most half the region, pomcp_set_root_belief) and
        # the next one with its 2 * need of sampling room
        nt = config.num_particles + config.extra_particles
        longest = max(len(sc["rows0"]) for sc in scens)
        caps.max_belief = max(caps.max_belief, 2 * longest + 4 * nt + 3 * S + 64)
    else:
        caps.max_belief = max_belief
    bp = BatchedPOMCP(model, ego, config, len(scens), S, searches=3, reroot=True, capacities=caps)
    assert bp.engine.search_kernel() == os.environ["POMCP_SEARCH_KERNEL"]
    for b, sc in enumerate(scens):
        bp.engine.set_root_belief(b, sc["rows0"])
    return bp, A


def device_equals_oracle(env, ego, cfg, scens, trees=None):
    """Replay the scenarios on the device, tree b = scens[b] (the oracle ran it
    under tree key b), and compare every belief and record."""
    bp, A = make_engine(env, ego, cfg, scens)
    trees = range(len(scens)) if trees is None else trees
    try:
        def check_search(which, k):
            acts = bp.search()
            stats = bp.engine.root_stats()
            for b in trees:
                exp = scens[b]["rec0"] if k is None else scens[b]["steps"][k]["rec"]
                got = stats_record(stats[b], A, True, acts[b], bp.engine.root_belief(b))
                for field in exp:
                    assert got.get(field) == exp[field], \
                        f"tree {b} {which}: {field}: {got.get(field)} != {exp[field]}"
                assert got == exp, f"tree {b} {which}"

        check_search("first search", None)
        for k in range(2):
            acts = np.array([sc["steps"][k]["action"] for sc in scens], dtype=np.int32)
            keys = np.array([sc["steps"][k]["key"] for sc in scens], dtype=np.uint64)
            absorbing = bp.engine.update(acts, keys)
            for b in trees:
                st = scens[b]["steps"][k]
                assert bool(absorbing[b]) == st["absorbing"], f"tree {b} update {k}"
                assert_rows(bp.engine.root_belief(b), st["rows"], f"tree {b} update {k}")
            check_search(f"search after update {k}", k)
    finally:
        bp.close()


@pytest.mark.parametrize("name", list(CASES))
def test_directed_case(name):
    env, ego = CASES[name][:2]
    cfg, sc = case_scenario(name)
    check_class(name, sc)
    device_equals_oracle(env, ego, cfg, [sc])


@functools.lru_cache(maxsize=None)
def absorbing_scenario(tree=0, stl=1.0, factor=4.0):
    cfg = case_cfg(stl, factor)
    return cfg, scenario(DRIVING, "0", cfg, list(late_belief(DRIVING, "0", 105)), "terminal",
                         tree=tree)


def check_absorbing(cfg, sc):
    """The update moved to a child the search marked absorbing: far fewer
    particles than n_target, yet the sampler is never called."""
    st = sc["steps"][0]
    assert st["absorbing"] and st["cls"] == [] and 0 < len(st["rows"]) < n_target_of(cfg) - 64
    assert st["rec"]["num_sims"] == 0 and sc["steps"][1]["rows"] == st["rows"]


def test_absorbing_child_is_not_reinvigorated():
    cfg, sc = absorbing_scenario()
    check_absorbing(cfg, sc)
    device_equals_oracle(DRIVING, "0", cfg, [sc])


# Seven trees = two 4-tree k_update workgroups, the second partial; one factor
# (2.5: limits that are no integers) and n_target 319, the classes differ by
# belief and observation.  With 64 simulations a child never holds n_target
# >= 65 particles, so "nothing to do" is here the absorbing child.
# (parent rows, donor env seeds, observation, class)
BATCH = [
    (500, (55,), "impossible", lambda c: c[2] == 0 and c[1] == math.ceil(2.5 * c[0]) == c[3]),
    (70, (55,), "real", lambda c: c[0] == c[1] == c[2] > 64),
    None,   # the absorbing child: no call
    (400, (55, 56), "real", lambda c: c[0] == c[2] < c[1] and c[3] > 64),
    (3, (56,), "impossible", lambda c: c[2] == 0 and c[1] == math.ceil(2.5 * c[0]) == c[3]),
    (300, (55, 56, 57, 58), "real", lambda c: 0 < c[2] < c[0] and c[3] > c[0]),
    (5000, (57,), "real", lambda c: c[0] == c[1] == c[2] > 64),
]


@functools.lru_cache(maxsize=None)
def batch_scenarios():
    cfg = case_cfg(3.0, 2.5)
    assert n_target_of(cfg) == 319
    scens = []
    for b, spec in enumerate(BATCH):
        if spec is None:
            scens.append(absorbing_scenario(tree=b, stl=3.0, factor=2.5)[1])
        else:
            length, donors, obs_kind, _ = spec
            scens.append(scenario(DRIVING, "0", cfg, parent_belief(DRIVING, "0", length, donors,
                                                                   rng_seed=10 + b),
                                  obs_kind, tree=b))
    return cfg, scens


def test_batched_trees_of_different_classes():
    """One engine, one update call: neighbouring waves of a workgroup run
    different numbers of tries and fill passes (or none) on their own RNG
    pages; every tree equals its own oracle (tree key b)."""
    cfg, scens = batch_scenarios()
    for b, spec in enumerate(BATCH):
        if spec is None:
            check_absorbing(cfg, scens[b])
        else:
            (cls,) = scens[b]["steps"][0]["cls"]
            assert spec[3](cls), (b, cls)
            assert not scens[b]["steps"][1]["absorbing"]
    passes = {-(-sc["steps"][0]["cls"][0][1] // 64) if sc["steps"][0]["cls"] else 0
              for sc in scens[:4]}
    assert len(passes) == 4, passes   # the first workgroup's four waves all differ
    device_equals_oracle(DRIVING, "0", cfg, scens)


@functools.lru_cache(maxsize=None)
def guard_scenarios():
    cfg = case_cfg(1.0, 4.0)
    assert n_target_of(cfg) == 107
    scens = [scenario(DRIVING, "0", cfg, parent_belief(DRIVING, "0", 150, rng_seed=20),
                      "impossible", tree=0)]
    scens += [scenario(DRIVING, "0", cfg, parent_belief(DRIVING, "0", 20, rng_seed=20 + b), "real",
                       tree=b) for b in range(1, 5)]
    return cfg, scens


def test_sampling_room_guard_reports_arena_for_that_tree_alone():
    """max_belief 330: tree 0 (150 parent rows, no child particle, need 107)
    has room for its parent belief and the child's particles but not for
    n + 2 * need = 214 records next to the parent (330 - 150 = 180): its update
    reports POMCP_E_ARENA, a status.  The other four trees (20 parent rows) of
    the same call re-root, reinvigorate and search equal to their oracles, then
    and after one more update."""
    from posggym_baselines_amd import _native as N
    cfg, scens = guard_scenarios()
    assert scens[0]["steps"][0]["cls"] == [(107, 428, 0, 428, 150)]
    for sc in scens[1:]:
        (cls,) = sc["steps"][0]["cls"]
        n = 107 - cls[0]
        assert cls[0] > 0 and n + 2 * cls[0] <= 330 - 20, cls
        (cls,) = sc["steps"][1]["cls"]
        assert cls[0] > 0 and (107 - cls[0]) + 2 * cls[0] <= 330 - 107, cls
    bp, A = make_engine(DRIVING, "0", cfg, scens, max_belief=330)
    eng, lib, B = bp.engine, bp.engine._lib, len(scens)
    try:
        acts = bp.search()
        stats = eng.root_stats()
        for b in range(B):
            assert stats_record(stats[b], A, True, acts[b], eng.root_belief(b)) == scens[b]["rec0"]
        for k in range(2):
            acts = np.array([sc["steps"][k]["action"] for sc in scens], dtype=np.int32)
            keys = np.array([sc["steps"][k]["key"] for sc in scens], dtype=np.uint64)
            with pytest.raises(N.PomcpError) as raised:   # the engine raises the status
                eng.update(acts, keys)
            assert raised.value.code == N.POMCP_E_ARENA
            assert lib.pomcp_last_error(eng._ctx) == b"update: tree 0: arena capacity exceeded"
            for b in range(1, B):
                assert_rows(eng.root_belief(b), scens[b]["steps"][k]["rows"], f"tree {b} update {k}")
            assert lib.pomcp_search(eng._ctx, S, None) == 0
            rc = lib.pomcp_get_root_stats(eng._ctx, eng._stats)   # tree 0's error is kept
            assert rc == N.POMCP_E_ARENA
            assert lib.pomcp_last_error(eng._ctx) == b"search: tree 0: arena capacity exceeded"
            assert eng._stats[0].action == -1
            for b in range(1, B):
                st = eng._stats[b]
                got = stats_record(st, A, True, st.action, eng.root_belief(b))
                assert got == scens[b]["steps"][k]["rec"], f"tree {b} search after update {k}"
    finally:
        bp.close()
