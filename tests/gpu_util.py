"""Drive the product (GPU) planner in the oracle's record format."""
import functools
import hashlib
import math
import struct

from oracle.episode import fhex, run_episode


def product_config(cfg_kwargs, num_sims):
    from posggym_baselines_amd.planning import KnownBounds, MCTSConfig
    kw = dict(cfg_kwargs)
    if kw.get("known_bounds") is not None:
        kw["known_bounds"] = KnownBounds(*kw["known_bounds"])
    return MCTSConfig(num_sims=num_sims, **kw)


def rows_digest(rows):
    """(size, sha1 over (t, v0, v1) u32 triples): oracle.episode.belief_digest of
    the packed particle words."""
    h = hashlib.sha1()
    for t, v0, v1 in rows:
        h.update(struct.pack("<III", int(t), int(v0), int(v1)))
    return len(rows), h.hexdigest()


def product_model(env):
    from posggym_baselines_amd.envs import DrivingModel, PursuitEvasionModel
    return PursuitEvasionModel() if env == "PursuitEvasion-v1" else DrivingModel()


def stats_record(st, A, searched, action, rows):
    rec = {"searched": searched, "action": int(action)}
    if not searched:
        return rec
    rec["belief_size"], rec["belief_digest"] = rows_digest(rows)
    rec["num_sims"] = int(st.num_sims)
    if rec["num_sims"] > 0:
        rec["search_depth"] = int(st.search_depth)
        rec["root_visits"] = int(st.root_visits)
        rec["child_visits"] = [int(x) for x in st.child_visits[:A]]
        rec["child_values"] = [fhex(x) for x in st.child_values[:A]]
        rec["child_totals"] = [fhex(x) for x in st.child_totals[:A]]
        rec["min_value"] = fhex(st.min_value)
        rec["max_value"] = fhex(st.max_value)
    return rec


def gpu_episode(cfg_kwargs, num_sims, env_seed, ego="0", max_steps=50, env="Driving-v1",
                planner_cls="POMCP", select_margin=None, exact=None):
    """select_margin: k_search's fast-selection margin (pomcp_debug_set_select_margin);
    exact: a list that receives each search's n_exact_selects."""
    from posggym_baselines_amd.planning import (IPOMCP, POMCP, RandomOtherAgentPolicy,
                                                RandomSearchPolicy)
    model = product_model(env)
    config = product_config(cfg_kwargs, num_sims)
    if planner_cls == "IPOMCP":
        others = {i: RandomOtherAgentPolicy(model, i) for i in model.possible_agents if i != ego}
        planner = IPOMCP(model, ego, config, others, RandomSearchPolicy(model, ego))
    else:
        planner = POMCP(model, ego, config, RandomSearchPolicy(model, ego))
    if select_margin is not None:
        from posggym_baselines_amd import _native as N
        assert N.load().pomcp_debug_set_select_margin(planner._engine._ctx,
                                                      float(select_margin)) == 0
    planner.reset()
    records = []
    A = model.action_spaces[ego].n

    def step(obs):
        searched = not planner.root.is_absorbing
        a = planner.step(obs)
        if not searched:
            records.append({"searched": False, "action": int(a)})
            return a
        rows = planner.root_belief()
        st = planner._engine.root_stats()[0]
        if exact is not None:
            exact.append(int(st.n_exact_selects))
        rec = stats_record(st, A, True, a, rows)
        rec["num_sims"] = int(planner.step_statistics["num_sims"])
        if rec["num_sims"] == 0:
            for k in ("search_depth", "root_visits", "child_visits", "child_values",
                      "child_totals", "min_value", "max_value"):
                rec.pop(k, None)
        records.append(rec)
        return a

    trace = run_episode(step, env_seed, ego=ego, max_steps=max_steps, env=env)
    planner.close()
    return trace, records


def _arena_usage(engine):
    import ctypes as C
    nb, nl = C.c_int32(), C.c_int32()
    assert engine._lib.pomcp_arena_usage(engine._ctx, C.byref(nb), C.byref(nl)) == 0
    return nb.value, nl.value


def batched_episodes(cfg_kwargs, num_sims, env_seeds, steps, capacities=None, usage=None,
                     inline_slots=None, probes=None, spin_limit=None, env="Driving-v1",
                     select_margin=None, counters=None, ego="0", map_generation=None,
                     map_scans=None):
    """Lockstep episodes of len(env_seeds) independent planners in ONE engine
    (tree b = planner b, env seed env_seeds[b]), `steps` real steps each.
    Returns per-tree record lists in the oracle format.  inline_slots: use only
    that many inline obs slots per action node (pomcp_debug_set_inline_slots);
    probes: a list that receives each search's overflow-map probes; spin_limit:
    k_search_lds's polls of a late step-tree hand-off (pomcp_debug_set_spin_limit);
    select_margin: k_search's fast-selection margin (pomcp_debug_set_select_margin);
    counters: a list that receives each search's summed (n_exact_selects,
    n_deferred, n_cutoff); ego: the planning agent (the other acts uniformly
    at random on the env's own stream, oracle/episode.py run_episode);
    map_generation: the overflow map's generation (pomcp_debug_set_map_generation),
    one int or one per tree, set once the engine is built and before the first
    update; map_scans: a list that receives every tree's (live, stale,
    generation) (pomcp_debug_map_scan) after every update."""
    from posggym_baselines_amd.planning import BatchedPOMCP
    model = product_model(env)
    B = len(env_seeds)
    bp = BatchedPOMCP(model, ego, product_config(cfg_kwargs, num_sims), B, num_sims,
                      searches=steps, reroot=True, capacities=capacities)
    if inline_slots is not None:
        from posggym_baselines_amd import _native as N
        assert N.load().pomcp_debug_set_inline_slots(bp.engine._ctx, int(inline_slots)) == 0
    if spin_limit is not None:
        from posggym_baselines_amd import _native as N
        assert N.load().pomcp_debug_set_spin_limit(bp.engine._ctx, int(spin_limit)) == 0
    if select_margin is not None:
        from posggym_baselines_amd import _native as N
        assert N.load().pomcp_debug_set_select_margin(bp.engine._ctx, float(select_margin)) == 0
    records = [[] for _ in range(B)]
    if map_generation is not None:
        set_map_generation(bp.engine, map_generation)
    scan = None if map_scans is None else lambda t: map_scans.append(map_scan(bp.engine))
    for t, stats in lockstep(bp, env, ego, env_seeds, steps, records, usage=usage,
                             after_update=scan):
        if probes is not None:
            probes.append(sum(int(st.n_probes) for st in stats))
        if counters is not None:
            counters.append((sum(int(st.n_exact_selects) for st in stats),
                             sum(int(st.n_deferred) for st in stats),
                             sum(int(st.n_cutoff) for st in stats)))
    bp.close()
    return records


def set_map_generation(engine, gen):
    """pomcp_debug_set_map_generation: one int for every tree, or one per tree."""
    import ctypes as C
    import numpy as np
    from posggym_baselines_amd import _native as N
    g = np.broadcast_to(np.asarray(gen, dtype=np.int32), (engine.num_trees,)).copy()
    rc = N.load().pomcp_debug_set_map_generation(engine._ctx, g.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0, rc


def map_scan(engine, trees=None):
    """pomcp_debug_map_scan of every tree (or `trees`): [(live, stale, generation)]."""
    import ctypes as C
    from posggym_baselines_amd import _native as N
    lib, out, res = N.load(), (C.c_int64 * 3)(), []
    for b in range(engine.num_trees) if trees is None else trees:
        assert lib.pomcp_debug_map_scan(engine._ctx, int(b), out) == 0
        res.append((int(out[0]), int(out[1]), int(out[2])))
    return res


def lockstep(bp, env, ego, env_seeds, steps, records, usage=None, after_update=None):
    """One lockstep episode per tree of `bp` (batched_episodes), a generator:
    appends every step's record to records[b] and yields (t, root statistics)
    after each search, before the environments step; after_update(t) is called
    between a step's update and its search."""
    import numpy as np
    from oracle.envs import make_model
    from oracle.episode import ENV_TREE_BASE
    from oracle.rng import S_ENV_POLICY_BASE, Streams
    A = bp.engine.A
    B = len(env_seeds)
    envs = []
    for s in env_seeds:
        es = Streams(s, ENV_TREE_BASE)
        e = make_model(env, es)
        st = e.sample_initial_state()
        envs.append([es, e, st, e.sample_initial_obs(st)])
    last = np.full(B, -1, dtype=np.int32)
    for t in range(steps):
        keys = np.array([e[1].pack_obs(e[3][ego]) for e in envs], dtype=np.uint64)
        if usage is not None:
            usage.append(("before_update", _arena_usage(bp.engine)))
        bp.engine.update(last, keys)
        if usage is not None:
            usage.append(("after_update", _arena_usage(bp.engine)))
        if after_update is not None:
            after_update(t)
        actions = bp.search()
        stats = bp.engine.root_stats()
        for b in range(B):
            records[b].append(stats_record(stats[b], A, True, actions[b], bp.engine.root_belief(b)))
        yield t, stats
        for b in range(B):
            es, e, st, obs = envs[b]
            acts = {i: int(actions[b]) if i == ego else
                    es.randint(S_ENV_POLICY_BASE + int(i), e.action_spaces[i].n)
                    for i in e.possible_agents}
            ts = e.step(st, acts)
            envs[b][2], envs[b][3] = ts.state, ts.observations
        last = actions.astype(np.int32)


def node_history(nodes, n, A):
    """The (action, obs key) path of node n of a device tree (intmcp_get_nodes'
    records; the None action -> -1): the oracle's OracleINTMCP.history."""
    out = []
    while n != 0:
        a = int(nodes[n]["info"]) & 7
        out.append((-1 if a == A else a, int(nodes[n]["okey"])))
        n = int(nodes[n]["parent"])
    return tuple(reversed(out))


def intmcp_device_tables(eng, pair):
    """The tables of device trees 1 .. max(L, 1) of one pair (the middle trees'
    intmcp_get_middle_support, the level-0 tree's intmcp_get_support) in the
    form of oracle_intmcp_limits_pair's "tables"."""
    L = max(eng.nesting_level, 1)
    out = []
    for k in range(1, L + 1):
        ent, parts = eng.mid_support(pair, k) if k < L else eng.support(pair)
        nk = eng.nodes(pair, k)
        below = eng.nodes(pair, k + 1) if k < L else None
        out.append([(node_history(nk, int(e["node"]), eng.A),
                     [((int(q[0]), int(q[1])),
                       node_history(below, int(q[2]), eng.A) if below is not None else None)
                      for q in parts[int(e["off"]):int(e["off"]) + int(e["size"])]])
                    for e in ent])
    return out


def intmcp_state_record(eng, pair, searched, action):
    """The oracle's I-NTMCP step record (oracle/run.py oracle_intmcp_record)
    rebuilt from the device state of one planner pair."""
    from oracle.intmcp_record import intmcp_record
    from posggym_baselines_amd.planning.intmcp import node_order
    rec = {"searched": searched, "action": int(action)}
    if not searched:
        return rec
    st = eng.root_stats()[pair]
    A = eng.A
    n1 = eng.nodes(pair, 1)
    s1 = eng.stats(pair, 1)
    ent, sparts = eng.support(pair)
    kids = [(int(st.child_action[i]), int(st.child_visits[i]), st.child_values[i],
             st.child_totals[i]) for i in range(st.num_children)]
    if eng.nesting_level == 0:   # the planner's tree (tree 1), its root belief = support entry 0
        t_root = int(n1[int(ent[0]["node"])]["t"])
        parts = [(t_root, (int(q[0]), int(q[1])), ()) for q in eng.root_belief(pair)]
        return intmcp_record(rec, int(st.num_sims), int(st.search_depth), int(st.root_visits),
                             kids, st.min_value, st.max_value, parts, [])
    rows = eng.root_belief(pair)

    def history(nodes, n):
        return node_history(nodes, n, A)

    def node(nodes, stats, n, ent_, parts_):
        """(visits, registered children, particles) of node n, its particles
        from its materialised belief entry"""
        nd = nodes[n]
        nk = [(a, int(stats[int(nd["stats"]) + a]["visits"]),
               float(stats[int(nd["stats"]) + a]["value"]))
              for a in node_order(int(nd["info"])) if a < A]
        hit = [e for e in ent_ if int(e["node"]) == n]
        rows_ = []
        if hit:
            e = hit[0]
            rows_ = parts_[int(e["off"]):int(e["off"]) + int(e["size"])]
        return (int(nd["visits"]), nk, [(int(nd["t"]), (int(q[0]), int(q[1]))) for q in rows_]), rows_

    L = eng.nesting_level

    def table(k):   # tree k's materialised beliefs: a middle tree's, else the level-0 support
        return eng.mid_support(pair, k) if 1 <= k <= L - 1 else (ent, sparts)

    ent1, parts1 = table(1)
    # the root's t: every root particle's other-agent history has that length
    t_root = int(n1[int(rows[0][2])]["t"]) if len(rows) else 0
    parts = [(t_root, (int(r[0]), int(r[1])), history(n1, int(r[2]))) for r in rows]
    nested, seen, mrows = [], [], []
    for r in rows:
        m = int(r[2])
        if m in seen:
            continue
        seen.append(m)
        nd, rows_ = node(n1, s1, m, ent1, parts1)
        nested.append((history(n1, m), nd))
        mrows.append(rows_)
    # the third tree on (nesting level >= 2): the histories carried by the
    # particles of the previous tree's recorded nodes, and those nodes
    chain, up_rows = [], mrows
    for k in range(2, L + 1):
        nk_, sk_ = eng.nodes(pair, k), eng.stats(pair, k)
        ek, pk = table(k)
        seqs, nodes2, seen2, rows2 = [], [], [], []
        for rows_ in up_rows:
            seq = []
            for q in rows_:
                h2 = int(q[2])
                seq.append(history(nk_, h2))
                if h2 not in seen2:
                    seen2.append(h2)
                    nd, r2 = node(nk_, sk_, h2, ek, pk)
                    nodes2.append((history(nk_, h2), nd))
                    rows2.append(r2)
            seqs.append(seq)
        chain.append((seqs, nodes2))
        up_rows = rows2
    return intmcp_record(rec, int(st.num_sims), int(st.search_depth), int(st.root_visits), kids,
                         st.min_value, st.max_value, parts, nested,
                         nested2=chain[0] if chain else None, deeper=chain[1:])


def _softmax_debug(ctx, slack):
    """Widen the I-NTMCP fast softmax bound (intmcp_debug_set_softmax_slack) and
    start counting exact-path draws."""
    from posggym_baselines_amd import _native as N
    assert N.load().intmcp_debug_set_softmax_slack(ctx, float(slack)) == 0


def _exact_draws(ctx):
    import ctypes as C
    from posggym_baselines_amd import _native as N
    n = C.c_uint64()
    assert N.load().intmcp_debug_exact_draws(ctx, C.byref(n)) == 0
    return int(n.value)


def intmcp_search_policies(model, search_probs):
    """{level: {agent: probs}} -> the product's INTMCP.initialize search_policies
    (SearchPolicyWrapper(FixedDistributionPolicy) / RandomSearchPolicy)."""
    if search_probs is None:
        return None
    from posggym_baselines_amd.planning.policies import FixedDistributionPolicy
    from posggym_baselines_amd.planning.search_policy import (RandomSearchPolicy,
                                                               SearchPolicyWrapper)
    return {lv: {i: (RandomSearchPolicy(model, i) if pols.get(i) is None else
                     SearchPolicyWrapper(FixedDistributionPolicy(model, i, "search", pols[i])))
                 for i in model.possible_agents}
            for lv, pols in search_probs.items()}


def gpu_intmcp_episode(cfg_kwargs, num_sims, env_seed, ego="0", max_steps=50, env="Driving-v1",
                       softmax_slack=None, exact=None, nesting_level=1, search_probs=None):
    """softmax_slack: the fast softmax bound's widening (None: the product's);
    the exact-path draws of the episode are appended to `exact` (a list);
    search_probs: {level: {agent: probs}} fixed-distribution search policies."""
    from posggym_baselines_amd.planning import INTMCP
    model = product_model(env)
    planner = INTMCP.initialize(model, ego, product_config(cfg_kwargs, num_sims), nesting_level,
                                intmcp_search_policies(model, search_probs))
    if softmax_slack is not None:
        _softmax_debug(planner._engine._ctx, softmax_slack)
    planner.reset()
    records = []

    def step(obs):
        searched = not planner.root.is_absorbing
        a = planner.step(obs)
        records.append(intmcp_state_record(planner._engine, 0, searched, a))
        return a

    trace = run_episode(step, env_seed, ego=ego, max_steps=max_steps, env=env)
    if exact is not None:
        exact.append(_exact_draws(planner._engine._ctx))
    planner.close()
    return trace, records


def batched_intmcp_episodes(cfg_kwargs, num_sims, env_seeds, steps, env="Driving-v1", ego="0",
                            softmax_slack=None, exact=None, nesting_level=1):
    """Lockstep I-NTMCP episodes of len(env_seeds) planner pairs in ONE engine
    (pair b = tree key b, env seed env_seeds[b]), at most `steps` real steps;
    a pair whose episode ended is skipped (INTMCP_SKIP).  Per-pair record lists
    in the oracle format (oracle/run.py oracle_intmcp_episode)."""
    import numpy as np
    from oracle.envs import make_model
    from oracle.episode import ENV_TREE_BASE
    from oracle.rng import S_ENV_POLICY_BASE, Streams
    from posggym_baselines_amd import _native as N
    from posggym_baselines_amd.planning import BatchedINTMCP
    model = product_model(env)
    B = len(env_seeds)
    bp = BatchedINTMCP(model, ego, product_config(cfg_kwargs, num_sims), B, num_sims,
                       searches=steps, nesting_level=nesting_level)
    if softmax_slack is not None:
        _softmax_debug(bp.engine._ctx, softmax_slack)
    envs = []
    for s in env_seeds:
        es = Streams(s, ENV_TREE_BASE)
        e = make_model(env, es)
        st = e.sample_initial_state()
        envs.append([es, e, st, e.sample_initial_obs(st), False])
    records = [[] for _ in range(B)]
    last = np.full(B, -1, dtype=np.int32)
    absorbing = np.zeros(B, dtype=bool)
    for t in range(steps):
        acts_in = last.copy()
        keys = np.zeros(B, dtype=np.uint64)
        searched = ~absorbing
        for b in range(B):
            if envs[b][4] or absorbing[b]:
                acts_in[b] = N.INTMCP_SKIP
            else:
                keys[b] = envs[b][1].pack_obs(envs[b][3][ego])
        absorbing = bp.engine.update(acts_in, keys)
        actions = bp.search()
        for b in range(B):
            if envs[b][4]:
                continue
            a = int(actions[b]) if searched[b] else int(last[b])
            records[b].append(intmcp_state_record(bp.engine, b, bool(searched[b]), a))
            es, e, st, obs, _ = envs[b]
            ja = {}
            for i in e.possible_agents:
                ja[i] = a if i == ego else es.randint(S_ENV_POLICY_BASE + int(i),
                                                      e.action_spaces[i].n)
            ts = e.step(st, ja)
            envs[b][2], envs[b][3] = ts.state, ts.observations
            envs[b][4] = bool(ts.all_done)
            last[b] = a
    if exact is not None:
        exact.append(_exact_draws(bp.engine._ctx))
    bp.close()
    return records


# ------------------------------------------------- I-NTMCP at its arena limits
# (tests/test_gpu_intmcp_limits.py, tests/test_intmcp_limits_cases.py)
class _Belief(list):
    """A node's belief that counts its appends (a particle entering the node in
    _simulate: the device's particle-log record) into n[0]; extend() -- the
    reinvigoration -- is not an append and logs nothing on the device either."""

    def __init__(self, items, n):
        super().__init__(items)
        self.n = n

    def append(self, x):
        self.n[0] += 1
        super().append(x)


class _Beliefs(list):
    """A tree's beliefs, every one a _Belief on the same counter."""

    def __init__(self, items, n):
        super().__init__(_Belief(b, n) for b in items)
        self.n = n

    def append(self, b):
        super().append(_Belief(b, self.n))

    def __setitem__(self, i, b):
        super().__setitem__(i, _Belief(b, self.n))


def count_appends(planner):
    """Wraps the belief append of a planner's (freshly reset) tree, as
    tests/test_gpu_search_invariants.py count_cutoffs wraps _select; returns the
    one-element counter."""
    n = [0]
    planner.tree.belief = _Beliefs(planner.tree.belief, n)
    return n


def oracle_tree_counts(tree, appended):
    """(n_nodes, n_log, n_stats) the device keeps for this oracle tree: its
    nodes, the particles appended, A statistics per node that holds a
    registered real action (the None action of node 0 has none)."""
    with_stats = sum(1 for order in tree.order if any(a < tree.A for a in order))
    return (len(tree.parent), appended, tree.A * with_stats)


def oracle_map_need(tree, inline=2):
    """Obs-child map entries of a tree: per (node, action) its children beyond
    the inline slots of the action's record."""
    per = {}
    for (n, a, _okey) in tree.children:
        per[(n, a)] = per.get((n, a), 0) + 1
    return sum(max(0, c - inline) for c in per.values())


def oracle_intmcp_limits_pair(cfg_kwargs, num_sims, env, nesting_level, pair, env_seed, steps,
                              last_search=True):
    """Pair `pair`'s lockstep episode on the oracle (oracle/run.py
    oracle_intmcp_episode with tree key `pair`), sampled as IntmcpLockstep
    samples the device: {"records", "calls": the (step, "update" | "search") of
    each sample of a step that searched, "counts": per sample a [trees][nodes,
    log, stats] list in the device's tree order (a nesting-0 planner's tree is
    tree 1, tree 0 an empty root), "levels": per sample None or, for a search,
    the counts after each search level's simulations, "root_sizes": the root
    belief after each update, "support_series": the materialised particles the
    largest table needs at each update, "entry_series": per update, for each
    device tree k = 1 .. max(L, 1), the histories of the distribution handed to
    that tree's planner (the entries of its table), "tables": per update and
    such tree, the table after the update as [(history, [(state words, the
    history the particle carries in the tree below or None)])] in the
    distribution's order, "map_need": the obs-child map entries
    per tree at the end, "map_series" / "map_levels": the same at every sample
    and after each search level}.
    last_search=False: the last step ends after its update (no record)."""
    from oracle.run import make_oracle_intmcp, oracle_intmcp_record
    p = make_oracle_intmcp(cfg_kwargs, num_sims, tree=pair, env=env, nesting_level=nesting_level)
    p.reset()
    by_tree = list(reversed(p.planners))          # device tree k = the level-(L - k) planner
    appended = [count_appends(pl) for pl in by_tree]
    out = {"records": [], "counts": [], "calls": [], "levels": [], "root_sizes": [],
           "map_series": [], "map_levels": []}

    def counts():
        rows = [list(oracle_tree_counts(pl.tree, n[0])) for pl, n in zip(by_tree, appended)]
        return [[1, 0, 0]] + rows if nesting_level == 0 else rows

    def maps():
        need = [oracle_map_need(pl.tree) for pl in by_tree]
        return [0] + need if nesting_level == 0 else need

    top = p.top
    target = p.cfg.num_particles + p.cfg.extra_particles
    out["support_series"] = []

    out["entry_series"], out["tables"] = [], []

    def materialised(pl, k):
        """The particles of pl's materialised beliefs (the device's support, a
        middle tree's table): the initial beliefs as drawn; at a re-root, per
        history its particles so far and room for a reinvigoration's accepted
        and rejected samples (csrc/intmcp.hip im_extract_support's cap).  And
        the entries of device tree k's table: the histories of the distribution
        the planner is handed."""
        first, later = pl._initial_nested_update, pl._nested_update

        def initial(dist):
            entries[k] = list(dist)
            first(dist)
            needs.append(sum(len(pl.tree.belief[n]) for n in dist))

        def update(dist):
            entries[k] = list(dist)
            need = sum(len(pl.tree.belief[n]) + 2 * math.ceil(pr * target) + 2
                       for n, pr in dist.items())
            needs.append(need)
            later(dist)

        pl._initial_nested_update, pl._nested_update = initial, update

    tabled = max(nesting_level, 1)     # device trees 1 .. tabled keep a table
    tabled_planner = {k: by_tree[k] if nesting_level > 0 else by_tree[0] for k in range(1, tabled + 1)}
    for k, pl in tabled_planner.items():
        materialised(pl, k)

    def table(k, nodes):
        """Device tree k's table after the update: per history of the
        distribution, in its order, (the history, its belief's particles as
        (state words, the history each carries in the tree below, if any))."""
        pl = tabled_planner[k]
        low = pl.nested if pl.level > 0 else None
        return [(p.history(pl.tree, n),
                 [(tuple(p.model.pack_words(q[0])),
                   p.history(low.tree, q[1]) if low is not None else None)
                  for q in pl.tree.belief[n]]) for n in nodes]

    nested_sim, levels, map_levels, needs, entries = top._nested_sim, [], [], [], {}

    def by_level(n, level, top_level):     # the counts when a search level's simulations end
        while len(levels) < level:
            levels.append(counts())
            map_levels.append(maps())
        nested_sim(n, level, top_level)

    top._nested_sim = by_level

    class Stop(Exception):
        pass

    def step(obs):
        t = len(out["records"])
        searched = not top.tree.absorbing[top.cur]
        if searched:       # OracleINTMCP.step, sampled between its update and its search
            p.stats = {"searched": True}
            del needs[:]
            entries.clear()
            top.update(top.last_action, obs)
            out["support_series"].append(max(needs))
            out["entry_series"].append([len(entries.get(k, ())) for k in range(1, tabled + 1)])
            out["tables"].append([table(k, entries.get(k, ())) for k in range(1, tabled + 1)])
            out["calls"].append((t, "update"))
            out["counts"].append(counts())
            out["levels"].append(None)
            out["map_series"].append(maps())
            out["map_levels"].append(None)
            out["root_sizes"].append(len(top.tree.belief[top.cur]))
            if t == steps - 1 and not last_search:
                raise Stop
            for pl in p.planners:
                pl.search_depth = 0
            del levels[:], map_levels[:]
            top.last_action = top.get_action(p.cfg.num_sims)
            levels.append(counts())
            map_levels.append(maps())
            out["calls"].append((t, "search"))
            out["counts"].append(levels[-1])
            out["levels"].append(list(levels))
            out["map_series"].append(map_levels[-1])
            out["map_levels"].append(list(map_levels))
        elif t == steps - 1 and not last_search:
            raise Stop
        a = top.last_action
        out["records"].append(oracle_intmcp_record(p, searched, a))
        return a

    try:
        run_episode(step, env_seed, max_steps=steps, env=env)
    except Stop:
        pass
    out["map_need"] = maps()
    return out


class _QuietEngine:
    """An IntmcpEngine whose root_stats() is the array the driver fetched: the
    engine's own raises for the first pair with an error, whichever pair is
    asked for."""

    def __init__(self, engine, stats):
        self._engine, self._stats = engine, stats

    def root_stats(self):
        return self._stats

    def __getattr__(self, name):
        return getattr(self._engine, name)


class IntmcpLockstep:
    """batched_intmcp_episodes' lockstep episode through the C ABI, for an engine
    in which pairs may fail: every call's return code and intmcp_last_error are
    kept, a pair whose error is set is skipped (INTMCP_SKIP) from then on with
    nothing more recorded for it, and the others play to the end.

    .calls: per intmcp_update / intmcp_search, in order, a dict: step, what,
      rc, message, counts (intmcp_get_tree_counts after it, [pairs][trees][nodes,
      log, stats]), errors (every pair's error after it), num_sims (every
      pair's);
    .failed: {pair: index of the call in which its error appeared};
    .records[b]: the oracle-format records of pair b (pairs in `record`; None: all);
    .root_sizes[b]: its root belief after each of its updates;
    .support_series[b] (support=True): after each of its updates, the largest
      off + cap of its materialised beliefs (intmcp_get_support, and every
      middle tree's), and .n_entries[b]: the entries of the table of each tree
      k = 1 .. max(L, 1) (the oracle's "entry_series"; support="entries":
      these alone, from the pairs' headers);
    .failed_entries[b] (support=True): the same counts of a pair that failed in
      an update, read after that call;
    .tables[b] (pairs in `tables`): after each of its updates, those trees'
      tables (intmcp_device_tables; the oracle's "tables");
    .scans (scans=True): intmcp_debug_arena_scan's live map slots at the end,
      [pairs][trees].
    last_search=False: the episode ends after the last step's update."""

    def __init__(self, cfg_kwargs, num_sims, env_seeds, steps, env="Driving-v1", ego="0",
                 nesting_level=1, capacities=None, record=None, last_search=True, support=False,
                 scans=False, tables=()):
        import ctypes as C
        import numpy as np
        from oracle.envs import make_model
        from oracle.episode import ENV_TREE_BASE
        from oracle.rng import S_ENV_POLICY_BASE, Streams
        from posggym_baselines_amd import _native as N
        from posggym_baselines_amd.planning import BatchedINTMCP
        from posggym_baselines_amd.planning.intmcp import MAX_TREES
        B = len(env_seeds)
        bp = BatchedINTMCP(product_model(env), ego, product_config(cfg_kwargs, num_sims), B, num_sims,
                           searches=steps, nesting_level=nesting_level, capacities=capacities)
        try:
            eng, lib = bp.engine, N.load()
            ctx = eng._ctx
            stats = (N.IntmcpRootStats * B)()
            quiet = _QuietEngine(eng, stats)
            trees = eng.nesting_level + 1 if eng.nesting_level >= 2 else 2
            self.capacities = eng.capacities
            self.calls, self.failed = [], {}
            self.records = [[] for _ in range(B)]
            self.root_sizes = [[] for _ in range(B)]
            self.support_series = [[] for _ in range(B)]
            self.n_entries = [[] for _ in range(B)]
            self.tables = {b: [] for b in tables}
            self.failed_entries = {}
            recorded = set(range(B)) if record is None else set(record)
            p32 = C.POINTER(C.c_int32)

            def call(t, what, rc):
                msg = lib.intmcp_last_error(ctx) if rc != 0 else b""
                lib.intmcp_get_root_stats(ctx, stats)      # (its code: the first pair's error again)
                counts = np.zeros((B, MAX_TREES, 3), dtype=np.int32)
                assert lib.intmcp_get_tree_counts(ctx, counts.ctypes.data_as(p32)) == 0
                errors = np.array([st.error for st in stats], dtype=np.int32)
                for b in np.nonzero(errors)[0]:
                    self.failed.setdefault(int(b), len(self.calls))
                self.calls.append(dict(step=t, what=what, rc=int(rc), message=bytes(msg).decode(),
                                       counts=counts[:, :trees], errors=errors,
                                       num_sims=np.array([st.num_sims for st in stats])))

            def tabs_of(b):     # the entries of trees 1 .. max(L, 1)
                return [eng.mid_support(b, k)[0] for k in range(1, eng.nesting_level)] \
                    + [eng.support(b)[0]]

            def entry_counts(b):     # their number alone: nothing but the pair's header is read
                ne, npart, out = C.c_int32(), C.c_int32(), []
                for k in range(1, eng.nesting_level):
                    assert lib.intmcp_get_middle_support(ctx, b, k, None, 0, C.byref(ne), None, 0,
                                                         C.byref(npart)) == 0
                    out.append(int(ne.value))
                assert lib.intmcp_get_support(ctx, b, None, 0, C.byref(ne), None, 0,
                                              C.byref(npart)) == 0
                return out + [int(ne.value)]

            envs = []
            for s in env_seeds:
                es = Streams(s, ENV_TREE_BASE)
                e = make_model(env, es)
                st = e.sample_initial_state()
                envs.append([es, e, st, e.sample_initial_obs(st), False])
            last = np.full(B, -1, dtype=np.int32)
            absorbing = np.zeros(B, dtype=np.int32)
            for t in range(steps):
                acts = last.copy()
                keys = np.zeros(B, dtype=np.uint64)
                searched = absorbing == 0
                for b in range(B):
                    if envs[b][4] or absorbing[b] or b in self.failed:
                        acts[b] = N.INTMCP_SKIP
                    else:
                        keys[b] = envs[b][1].pack_obs(envs[b][3][ego])
                call(t, "update", lib.intmcp_update(ctx, acts.ctypes.data_as(p32),
                                                    keys.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                    absorbing.ctypes.data_as(p32)))
                for b in range(B):
                    if support and self.failed.get(b) == len(self.calls) - 1:
                        self.failed_entries[b] = entry_counts(b)
                    if acts[b] == N.INTMCP_SKIP or b in self.failed:
                        continue
                    self.root_sizes[b].append(int(stats[b].belief_size))
                    if support == "entries":
                        self.n_entries[b].append(entry_counts(b))
                    elif support:
                        tabs = tabs_of(b)
                        self.support_series[b].append(max(int(e["off"]) + int(e["cap"])
                                                          for tab in tabs for e in tab))
                        self.n_entries[b].append([len(tab) for tab in tabs])
                    if b in self.tables:
                        self.tables[b].append(intmcp_device_tables(eng, b))
                if t == steps - 1 and not last_search:
                    break
                actions = np.zeros(B, dtype=np.int32)
                call(t, "search", lib.intmcp_search(ctx, int(num_sims), actions.ctypes.data_as(p32)))
                for b in range(B):
                    if envs[b][4] or b in self.failed:
                        continue
                    a = int(stats[b].action) if searched[b] else int(last[b])
                    if b in recorded:
                        self.records[b].append(intmcp_state_record(quiet, b, bool(searched[b]), a))
                    es, e, st, obs, _ = envs[b]
                    ja = {i: a if i == ego else es.randint(S_ENV_POLICY_BASE + int(i),
                                                           e.action_spaces[i].n)
                          for i in e.possible_agents}
                    ts = e.step(st, ja)
                    envs[b][2], envs[b][3] = ts.state, ts.observations
                    envs[b][4] = bool(ts.all_done)
                    last[b] = a
            self.scans = None
            if scans:
                self.scans = [[eng.debug_arena_scan(b, k)[2] for k in range(trees)] for b in range(B)]
        finally:
            bp.close()

    def searched(self):
        """The pair-steps recorded as searched."""
        return sum(bool(r["searched"]) for recs in self.records for r in recs)


IM_LIMITS_PAIRS, IM_LIMITS_STEPS, IM_LIMITS_FIRST_SEED = 70, 3, 3000
# (environment, nesting level) of sections a and b: k_im_search / k_im_update
# at nesting 0 (the planner's own tree is tree 1) and 1, k_im_searchN<3> /
# k_im_updateN<3> at nesting 2
IM_LIMITS_CASES = (("Driving-v1", 0), ("Driving-v1", 1), ("Driving-v1", 2),
                   ("PursuitEvasion-v1", 1), ("PursuitEvasion-v1", 2))


def im_limits_cfg():
    """BASE_CFG of tests/golden/make_oracle_digests.py (seed 3, the nested
    belief, ucb)."""
    import os
    import sys
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if golden not in sys.path:
        sys.path.insert(0, golden)
    from make_oracle_digests import BASE_CFG
    return dict(BASE_CFG)


@functools.lru_cache(maxsize=None)
def oracle_intmcp_limits(env, nesting_level, num_sims, pairs=None, first_seed=IM_LIMITS_FIRST_SEED,
                         steps=IM_LIMITS_STEPS, last_search=True):
    """oracle_intmcp_limits_pair of pair b on env seed first_seed + b for the
    pairs listed (None: 0 .. IM_LIMITS_PAIRS - 1), computed once: {pair: ...}."""
    cfg = im_limits_cfg()
    return {b: oracle_intmcp_limits_pair(cfg, num_sims, env, nesting_level, b, first_seed + b,
                                         steps, last_search)
            for b in (range(IM_LIMITS_PAIRS) if pairs is None else pairs)}


def oracle_arena_peaks(batch, which):
    """{pair: its largest count of arena `which` (0 nodes, 1 log, 2 stats) over
    its trees and samples}, and the tree that held each pair's peak."""
    peaks, trees = {}, {}
    for b, x in batch.items():
        peaks[b], trees[b] = max((c[k][which], k) for c in x["counts"] for k in range(len(c)))
    return peaks, trees


# The nested history tables at max_root_belief (section f of tests/
# test_gpu_intmcp_limits.py): (environment, nesting level, simulations per
# level, first env seed, the largest table of a tree k >= 2, {pair at it:
# (step of the update that builds it, tree)}) -- pinned on the oracle by
# tests/test_intmcp_limits_cases.py, which records how they were found.
IM_TABLE_CASES = (
    ("PursuitEvasion-v1", 3, 32, 3000, 26, {42: (2, 3)}),
    ("Driving-v1", 2, 32, 16000, 29, {24: (2, 2)}),
    ("PursuitEvasion-v1", 3, 32, 5000, 24, {48: (2, 2)}),
)
IM_ROOT_BELIEF_FLOOR = 22     # intmcp_create's least max_root_belief: 2 x (num_particles + extra_particles)


def nested_table_need(entry_series, root_sizes):
    """entry_series[b] / root_sizes[b]: pair b's table entries per update and
    tree k = 1 .. L ("entry_series", IntmcpLockstep.n_entries) and its root
    belief per update.  Returns (each pair's largest table over the trees k >=
    2, which im_support_nested fills; the largest of them; {pair at it: (the
    first update that builds such a table, the first tree -- the update goes
    top down -- that holds it)}; what max_root_belief needs without those
    tables: the largest root belief, at least intmcp_create's floor).  A pair
    updates at every step until its episode ends, so the update's index is its
    step."""
    nested = [max((max(e[1:]) for e in es), default=0) for es in entry_series]
    top = max(nested)
    tied = {}
    for b, es in enumerate(entry_series):
        if nested[b] == top:
            t = next(t for t, e in enumerate(es) if max(e[1:]) == top)
            tied[b] = (t, 2 + es[t][1:].index(top))
    other = max(IM_ROOT_BELIEF_FLOOR, max(max(r, default=0) for r in root_sizes))
    return nested, top, tied, other
