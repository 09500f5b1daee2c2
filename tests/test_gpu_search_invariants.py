"""k_search's loop invariants as countdowns (csrc/pomcp_search.hip): the
simulations left and the room left in the particle log and in the block arena
are per-wave / per-lane counters tested against a literal, the depth limit of a
depth-specialised kernel is a literal everywhere, and the passes above the last
load their slot line for every lane.  None of it may change a value, so every
case here is the oracle's records bit for bit (as
tests/test_gpu_depth_kernels.py), on the tree-per-lane kernel with the
cut-off records deferred ("lane") and looked up ("lane_eager"), on the
depth-specialised kernels DL = 1, 2, 3 and on the generic kernel forced with
POMCP_SEARCH_DEPTH_SPEC=0, for both environments.

A case is one first search of an episode (the initial update, then the
search) of 70 planners -- two search waves, the second partly empty -- with 64
simulations unless it says otherwise.  The cases sit where a countdown can be
off by one: 1, 2 and 3 simulations and a search split over unequal launches
(the loop bound and the belief prefetch's "a simulation follows"); a particle
log and a block arena that are exactly full, and one record / one block short
for one tree of five (the error, the tree it names and what that tree
appended); root beliefs whose time step makes depth 1 or depth 2 the last step
of some lanes of a wave and not of others (the lanes that skip the child lookup
in a pass above the last, whose slot line is now loaded anyway); and one inline
slot per action node, so that the lookup's mask meets children beyond it.
The oracle's records are computed once per configuration and shared.
"""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BASE_CFG = dict(discount=0.95, search_time_limit=0.1, c=math.sqrt(2), truncated=False,
                action_selection="ucb", pucb_exploration_fraction=0.25, known_bounds=None,
                step_limit=None, epsilon=0.92, seed=0, state_belief_only=True)
SIMS, TREES = 64, 70
ENVS = ("Driving-v1", "PursuitEvasion-v1")
MODES = ("lane", "lane_eager")
# name: (epsilon, POMCP_SEARCH_DEPTH_SPEC, the depth limit, the kernel's DL)
KERNELS = {"dl1": (0.96, None, 1, 1), "dl2": (0.92, None, 2, 2), "dl3": (0.88, None, 3, 3),
           "generic": (0.92, "0", 2, 0)}


def matrix(kerns=tuple(KERNELS), envs=ENVS):
    return pytest.mark.parametrize(
        "env,kern,mode", [(e, k, m) for e in envs for k in kerns for m in MODES])


def choose(monkeypatch, kern, mode, **overrides):
    """Sets the process-wide kernel choice of the case; returns its configuration."""
    eps, spec, _, _ = KERNELS[kern]
    monkeypatch.setenv("POMCP_SEARCH_KERNEL", "lane")
    monkeypatch.setenv("POMCP_DEFER_CUTOFF", "0" if mode == "lane_eager" else "1")
    if spec is None:
        monkeypatch.delenv("POMCP_SEARCH_DEPTH_SPEC", raising=False)
    else:
        monkeypatch.setenv("POMCP_SEARCH_DEPTH_SPEC", spec)
    return dict(BASE_CFG, epsilon=eps, **overrides)


def cfg_key(cfg):
    return tuple(sorted(cfg.items()))


# ------------------------------------------------------------------ the oracle
def count_cutoffs(p):
    """Wraps p._select: counts the levels below the root whose children lie
    beyond the depth / step limits (k_search's n_cutoff: mcts.py:315 for the
    child, tested at its parent's level)."""
    select, n = p._select, [0]

    def counting(node):
        depth = p.on_t[node] - p.on_t[p.root]
        if depth >= 1 and (depth + 1 > p.cfg.depth_limit or p.on_t[node] + 1 > p.step_limit):
            n[0] += 1
        return select(node)

    p._select = counting
    return n


def tree_needs(p):
    """(records appended, blocks in use) of the oracle's tree after one search
    from a fresh root: one record per level stepped (every particle but the
    root's), one block per expanded obs node."""
    levels = sum(len(b) for n, b in enumerate(p.belief) if n != p.root)
    return levels, len(p.an_visits) // p.A


@functools.lru_cache(maxsize=None)
def first_step(key, env, sims, tree, seed):
    """The first planner step of the episode of env seed `seed` on the planner
    keyed `tree`: (record, (levels, blocks) needs, n_cutoff)."""
    from oracle.episode import run_episode
    from oracle.run import make_oracle, oracle_record
    p = make_oracle(dict(key), sims, tree=tree, env=env)
    cut = count_cutoffs(p)
    out = []

    def step(obs):
        p.update(None, obs)
        a = p.get_action()
        p.stats["searched"] = True
        out.append(oracle_record(p, True, a))
        return a

    run_episode(step, seed, max_steps=1, env=env)
    return out[0], tree_needs(p), cut[0]


def first_steps(cfg, env, sims=SIMS, trees=TREES, first_seed=3000):
    """Planner b on env seed first_seed + b: (env seeds, records, needs, n_cutoff)."""
    seeds = tuple(range(first_seed, first_seed + trees))
    steps = [first_step(cfg_key(cfg), env, sims, b, s) for b, s in enumerate(seeds)]
    return seeds, [r for r, _, _ in steps], [n for _, n, _ in steps], [c for _, _, c in steps]


def first_obs_keys(env, seeds):
    """The ego's first observation key of each environment (gpu_util.lockstep's)."""
    from oracle.envs import make_model
    from oracle.episode import ENV_TREE_BASE
    from oracle.rng import Streams
    keys = []
    for s in seeds:
        e = make_model(env, Streams(s, ENV_TREE_BASE))
        keys.append(e.pack_obs(e.sample_initial_obs(e.sample_initial_state())["0"]))
    return np.array(keys, dtype=np.uint64)


# ------------------------------------------------------------------ the engine
class Run:
    """One search of every tree, in `launches` launches (final_sel only in the
    last): .rc / .message of the last pomcp_get_root_stats, .stats (the root
    statistics after the last launch), .records (the oracle's format; a tree
    with an error has None) and .depths (each launch's search_depth per tree)."""

    def __init__(self, cfg, env, kern, launches, *, seeds=None, beliefs=None, capacities=None,
                 inline_slots=None):
        from gpu_util import product_config, product_model, stats_record
        from posggym_baselines_amd import _native as N
        from posggym_baselines_amd.planning import BatchedPOMCP
        model = product_model(env)
        B = len(seeds if seeds is not None else beliefs)
        sims = sum(launches)
        pcfg = product_config(cfg, sims)
        assert pcfg.depth_limit == KERNELS[kern][2], (kern, pcfg.depth_limit)
        bp = BatchedPOMCP(model, "0", pcfg, B, sims, capacities=capacities)
        try:
            eng, lib = bp.engine, N.load()
            assert (eng.search_kernel(), eng.search_depth_spec()) == ("lane", KERNELS[kern][3])
            if inline_slots is not None:
                assert lib.pomcp_debug_set_inline_slots(eng._ctx, int(inline_slots)) == 0
            if beliefs is not None:
                for b, rows in enumerate(beliefs):
                    eng.set_root_belief(b, rows)
            else:
                eng.update(np.full(B, -1, dtype=np.int32), first_obs_keys(env, seeds))
            stats = (N.PomcpRootStats * B)()
            self.depths = []
            for i, n in enumerate(launches):
                if i + 1 < len(launches):
                    assert lib.pomcp_search_continue(eng._ctx, int(n)) == 0
                else:
                    assert lib.pomcp_search(eng._ctx, int(n), None) == 0
                self.rc = lib.pomcp_get_root_stats(eng._ctx, stats)
                assert all(int(st.num_sims) == n for st in stats if st.error == 0), (i, n)
                self.depths.append([int(st.search_depth) for st in stats])
            self.message = lib.pomcp_last_error(eng._ctx) if self.rc != 0 else b""
            self.stats = stats
            self.records = []
            for b in range(B):
                if stats[b].error != 0:
                    self.records.append(None)
                    continue
                rec = stats_record(stats[b], eng.A, True, stats[b].action, eng.root_belief(b))
                # a launch reports its own simulations and depth: the search's are
                # their sum and maximum (POMCP.get_action does the same)
                rec["num_sims"] = sims
                rec["search_depth"] = max(d[b] for d in self.depths)
                self.records.append(rec)
        finally:
            bp.close()


def assert_records(got, exp, seeds, trees=None):
    for b in range(len(exp)) if trees is None else trees:
        assert got[b] == exp[b], f"tree {b} (env seed {seeds[b]})"


# ------------------------------------------------------- a. simulation budgets
@matrix()
@pytest.mark.parametrize("sims", [1, 2, 3])
def test_one_two_and_three_simulations(env, kern, mode, sims, monkeypatch):
    """The loop bound and the belief prefetch ("a simulation follows this one")
    at their ends: the last simulation draws no particle for a next one, so a
    count that is off by one shows in the belief stream's counter -- the next
    search step would differ -- and in the records at once when a simulation is
    lost or added."""
    cfg = choose(monkeypatch, kern, mode)
    seeds, exp, needs, _ = first_steps(cfg, env, sims=sims)
    run = Run(cfg, env, kern, [sims], seeds=seeds)
    assert run.rc == 0, run.message
    assert_records(run.records, exp, seeds)
    assert [int(st.n_levels) for st in run.stats] == [n[0] for n in needs]


@matrix()
def test_search_split_over_unequal_launches(env, kern, mode, monkeypatch):
    """64 simulations as launches of 5, 1, 2 and 56, the final action drawn by
    the last: the records of one 64-simulation search.  Every launch but the
    last ends with a belief lookahead word held and no particle prefetched; the
    next one starts from the stored counters."""
    cfg = choose(monkeypatch, kern, mode)
    seeds, exp, needs, cuts = first_steps(cfg, env)
    launches = [5, 1, 2, SIMS - 8]
    run = Run(cfg, env, kern, launches, seeds=seeds)
    assert run.rc == 0, run.message
    assert_records(run.records, exp, seeds)
    # (a launch's counters are its own: the last launch's levels are below the search's)
    assert all(0 < int(st.n_levels) < n[0] for st, n in zip(run.stats, needs))
    one = Run(cfg, env, kern, [SIMS], seeds=seeds)
    assert_records(one.records, exp, seeds)
    assert [int(st.n_levels) for st in one.stats] == [n[0] for n in needs]
    assert [int(st.n_cutoff) for st in one.stats] == cuts
    assert [int(st.n_deferred) for st in one.stats] == (cuts if mode == "lane" else [0] * TREES)


# ------------------------------------------- b. exactly full log / block arena
FIVE = 5


POOL = 40      # env seeds tried per planner
TIGHT = 2      # the planner that needs the most


@functools.lru_cache(maxsize=None)
def five_planners(key, env, which):
    """Planners 0..4 on env seeds chosen so that planner TIGHT alone needs the
    most records (which = 0) / blocks (which = 1): its seed of the largest need
    among POOL, and for every other planner the first seed of a smaller need
    (where nearly every simulation expands a node -- PursuitEvasion at depth
    limit 3 -- some planners have none and need as much as TIGHT).
    Returns (env seeds, records, needs)."""
    pool = range(3000, 3000 + POOL)
    top, seeds = max((first_step(key, env, SIMS, TIGHT, s)[1][which], -s) for s in pool), []
    for b in range(FIVE):
        seeds.append(-top[1] if b == TIGHT else
                     next((s for s in pool if first_step(key, env, SIMS, b, s)[1][which] < top[0]),
                          pool[0]))
    steps = [first_step(key, env, SIMS, b, s) for b, s in enumerate(seeds)]
    return tuple(seeds), [r for r, _, _ in steps], [n for _, n, _ in steps]


def planned(cfg, env, sims, **fields):
    from gpu_util import product_config, product_model
    from posggym_baselines_amd.planning.engine import plan_capacities
    model = product_model(env)
    pcfg = product_config(cfg, sims)
    caps = plan_capacities(pcfg, pcfg.step_limit or model.spec.max_episode_steps, sims, 1,
                           reroot=False, num_actions=model.action_spaces["0"].n)
    for k, v in fields.items():
        setattr(caps, k, v)
    return caps


@matrix()
@pytest.mark.parametrize("arena", ["log", "blocks"])
def test_exactly_full_arena_and_one_short(env, kern, mode, arena, monkeypatch):
    """The capacity a search needs, taken from a first run (the largest n_log /
    n_blocks of five trees): with exactly that capacity no tree reports an
    error; with one less, the tree that needed it -- and only that one, unless
    all five need the same (five_planners) -- reports POMCP_E_ARENA, having appended (allocated) exactly what there was
    room for, since a level that finds the log full appends nothing and an
    expansion that finds the arena full allocates nothing; the four others'
    records are the oracle's in all three runs."""
    from posggym_baselines_amd import _native as N
    cfg = choose(monkeypatch, kern, mode)
    which = 0 if arena == "log" else 1
    field, used = ("max_particles", "n_log") if arena == "log" else ("max_blocks", "n_blocks")
    seeds, exp, needs = five_planners(cfg_key(cfg), env, which)
    first = Run(cfg, env, kern, [SIMS], seeds=seeds)
    assert first.rc == 0, first.message
    assert_records(first.records, exp, seeds)
    use = [int(getattr(st, used)) for st in first.stats]
    top = max(use)
    # (the oracle's counts are the engine's, up to what a fresh root holds)
    assert len({u - n[which] for u, n in zip(use, needs)}) == 1, (use, needs)
    short_of = [b for b in range(FIVE) if use[b] == top]   # the trees one short below
    assert TIGHT in short_of, use
    if not (env == "PursuitEvasion-v1" and kern == "dl3" and arena == "blocks"):
        assert short_of == [TIGHT], use   # (there: a block per simulation for most seeds)
    print(arena, "use", use, "needs", needs)
    full = Run(cfg, env, kern, [SIMS], seeds=seeds,
               capacities=planned(cfg, env, SIMS, **{field: top}))
    assert full.rc == 0, full.message
    assert_records(full.records, exp, seeds)
    assert [int(getattr(st, used)) for st in full.stats] == use
    short = Run(cfg, env, kern, [SIMS], seeds=seeds,
                capacities=planned(cfg, env, SIMS, **{field: top - 1}))
    assert short.rc == N.POMCP_E_ARENA
    assert f"tree {short_of[0]}: arena capacity exceeded".encode() in short.message, short.message
    errors = [int(st.error) for st in short.stats]
    assert errors == [N.POMCP_E_ARENA if b in short_of else 0 for b in range(FIVE)]
    for b in short_of:
        assert int(getattr(short.stats[b], used)) == top - 1, b
        assert int(short.stats[b].num_sims) < SIMS, b
    assert_records(short.records, exp, seeds, [b for b in range(FIVE) if b not in short_of])


# ------------------------------------------------ c. the step limit inside a wave
STEP_LIMIT = 6
# root time steps, lane by lane: far from the limit; depth 1 is the last step
# (the children of the depth-1 node are beyond it: a skipping lane of pass 1);
# depth 2 the last (pass 2 of DL = 3); the root the last; the root beyond it
ROOT_T = (1, STEP_LIMIT - 1, STEP_LIMIT - 2, STEP_LIMIT, STEP_LIMIT + 1, 2)


@functools.lru_cache(maxsize=None)
def host_beliefs(key, env):
    """Per tree b a root belief at time ROOT_T[b % 6] (another planner's b0
    particles relabelled, insertion order kept) and the oracle's record of a
    search from it: (rows per tree, records, n_cutoff)."""
    from oracle.episode import run_episode
    from oracle.run import make_oracle, oracle_record
    cfg = dict(key)
    beliefs, recs, cuts = [], [], []
    for b in range(TREES):
        t = ROOT_T[b % len(ROOT_T)]
        donor = make_oracle(cfg, 1, tree=1000 + b, env=env)
        run_episode(lambda obs: (donor.update(None, obs), 0)[1], 5000 + b, max_steps=1, env=env)
        parts = [(st, t) for st, _ in donor.belief[donor.root]]
        beliefs.append([(t,) + tuple(donor.model.pack_words(st)) for st, _ in parts])
        p = make_oracle(cfg, SIMS, tree=b, env=env)
        node = p._new_obs_node(t, 0)
        p.belief[node] = list(parts)
        p.root = node
        cut = count_cutoffs(p)
        p.stats = {}
        a = p.get_action()
        p.stats["searched"] = True
        p.stats["belief"] = list(p.belief[p.root])
        recs.append(oracle_record(p, True, a))
        cuts.append(cut[0])
    return beliefs, recs, cuts


@matrix(kerns=("dl2", "dl3", "generic"))
def test_step_limit_reached_by_some_lanes_of_a_wave(env, kern, mode, monkeypatch):
    """step_limit = 6 and root beliefs at t = 1, 5, 4, 6, 7, 2 in turn over the
    lanes: in one wave the depth-1 pass (DL = 2 and 3) and the depth-2 pass
    (DL = 3) hold lanes at their last step -- which skip the child lookup when
    the cut-off records are deferred -- beside lanes that look up, a root whose
    children are cut off and a root beyond the limit (every simulation backs up
    0 at once).  Records and the cut-off counters equal the oracle's."""
    cfg = choose(monkeypatch, kern, mode, step_limit=STEP_LIMIT)
    beliefs, exp, cuts = host_beliefs(cfg_key(cfg), env)
    run = Run(cfg, env, kern, [SIMS], beliefs=beliefs)
    assert run.rc == 0, run.message
    assert_records(run.records, exp, list(range(TREES)))
    assert [int(st.n_cutoff) for st in run.stats] == cuts
    assert [int(st.n_deferred) for st in run.stats] == (cuts if mode == "lane" else [0] * TREES)
    by_t = {t: sum(c for b, c in enumerate(cuts) if ROOT_T[b % len(ROOT_T)] == t) for t in ROOT_T}
    print("cut-off levels by root t:", by_t)
    assert by_t[STEP_LIMIT - 1] > 0 and by_t[STEP_LIMIT] == 0 and by_t[STEP_LIMIT + 1] == 0


# --------------------------------------------------------------- d. fewer slots
@matrix()
def test_one_inline_slot_and_the_overflow_map(env, kern, mode, monkeypatch):
    """One inline obs slot per action node (pomcp_debug_set_inline_slots, as
    tests/test_gpu_child_map.py): every second child of an action node lives in
    the overflow map, so find_slot's mask of the slots in use decides at every
    lookup -- also over the slot lines that the passes above the last now load
    for every lane.  The records are the oracle's and the map was probed."""
    cfg = choose(monkeypatch, kern, mode)
    seeds, exp, _, _ = first_steps(cfg, env)
    run = Run(cfg, env, kern, [SIMS], seeds=seeds, inline_slots=1,
              capacities=planned(cfg, env, SIMS, overflow_slots=256))
    assert run.rc == 0, run.message
    assert_records(run.records, exp, seeds)
    probes = sum(int(st.n_probes) for st in run.stats)
    print("overflow-map probes:", probes)
    assert probes > 0
