"""The obs-child overflow map (OvfSlot, csrc/pomcp_device.h) where no other test
takes it: the wrap of its 14-bit generation at all four sites (k_reset,
k_restore, k_compact, k_queue_refill), generations with the key's high bits
set, probe chains that leave the home bucket, and a full map.

Every planner is PursuitEvasion-v1's agent "1" with ONE inline obs slot per
action node (pomcp_debug_set_inline_slots), so most obs children live in the
map.  The yardstick is the oracle, which has no map and no generations: the
records of every search bit for bit, and the map's own contents
(pomcp_debug_map_scan: live / stale slots, the generation) against the number of
entries the oracle's tree needs, sum(max(0, children - 1)) over the action nodes
below its root.

Generations (TreeHdr.epoch) advance by one per reset, restore, re-root and queue
refill -- not on an initial update -- and go from kEpochMask = 16,383 to 1 with
the map cleared.  A fresh BatchedPOMCP is at 2 (pomcp_create resets and so does
the constructor).  Tests that need stale entries plant them first: a PRE_K = 2
step episode (generations 2 and 3) and a reset, which leaves the engine at
generation 4."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from gpu_util import lockstep, map_scan, product_config, product_model, set_map_generation, stats_record
from oracle.episode import fhex, run_episode
from oracle.run import make_oracle, oracle_record

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["lane", "lane_eager", "wave"])
def search_kernel(request, monkeypatch):
    """The search kernels of tests/test_gpu_parity.py: k_search with the cut-off
    children deferred to the re-root ("lane": they enter the map in
    k_compact_log) or looked up during the search ("lane_eager"), and
    k_search_lds ("wave", which never defers)."""
    kind, _, mode = request.param.partition("_")
    monkeypatch.setenv("POMCP_SEARCH_KERNEL", kind)
    if kind == "lane":
        monkeypatch.setenv("POMCP_DEFER_CUTOFF", "0" if mode == "eager" else "1")
    return request.param


ENV, EGO, OTHER = "PursuitEvasion-v1", "1", "0"
EPOCH_MASK = 16383     # csrc/pomcp_device.h kEpochMask
BUCKET = 16            # csrc/pomcp_device.h kBucket
ISLOTS = 1
FRESH = 2              # a new BatchedPOMCP's generation: pomcp_create's reset and its own
PRE_K = 2              # the planting episode's steps
PLANTED = FRESH + PRE_K   # the generation after it and a reset: PRE_K - 1 re-roots, + 1
TWIN_GEN = 5000        # a generation far from the wrap (and from every planted one)
TEST_CFG = dict(discount=0.95, search_time_limit=0.1, c=math.sqrt(2), truncated=False,
                action_selection="ucb", pucb_exploration_fraction=0.25, known_bounds=None,
                step_limit=None, epsilon=0.92, seed=0, state_belief_only=True)


def advance(gen, n):
    """The generation n increments after `gen`: 1..kEpochMask, cyclic."""
    return (gen - 1 + n) % EPOCH_MASK + 1


# ------------------------------------------------------------------ the oracle
def map_need(p, max_depth=None):
    """The map entries the oracle's tree needs below its current root:
    sum(max(0, children - ISLOTS)) over the action nodes of the root's subtree
    (the nodes above the root are gone from the engine's map after a re-root).
    max_depth: without the children deeper than that below the root -- the
    cut-off children, which a deferring search leaves to the next re-root."""
    kids = {}
    for (an, _), c in p.children.items():
        kids.setdefault(an, []).append(c)
    need, stack = 0, [(p.root, 0)]
    while stack:
        n, d = stack.pop()
        b = p.on_block[n]
        if b < 0 or (max_depth is not None and d + 1 > max_depth):
            continue
        for a in range(p.A):
            ch = kids.get(b * p.A + a, [])
            need += max(0, len(ch) - ISLOTS)
            stack.extend((c, d + 1) for c in ch)
    return need


def map_lookups(p, max_depth=None):
    """The map lookups of an episode's FIRST search (the tree was empty before
    it): every arrival at a child that is not its action node's first one, a
    child's visits being its arrivals.  max_depth as map_need's."""
    kids = {}
    for (an, _), c in p.children.items():
        kids.setdefault(an, []).append(c)
    n, stack = 0, [(p.root, 0)]
    while stack:
        node, d = stack.pop()
        b = p.on_block[node]
        if b < 0 or (max_depth is not None and d + 1 > max_depth):
            continue
        for a in range(p.A):
            ch = kids.get(b * p.A + a, [])
            n += sum(p.on_visits[c] for c in ch[ISLOTS:])
            stack.extend((c, d + 1) for c in ch)
    return n


def ovf_hash(an, key):
    """csrc/pomcp_device.h ovf_hash."""
    m = (1 << 64) - 1
    h = key ^ ((an * 0x9E3779B97F4A7C15) & m)
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & m
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & m
    h ^= h >> 33
    return h & 0xFFFFFFFF


def map_model(p, buckets, max_depth=None):
    """The map of an episode's FIRST search restated: the children beyond each
    action node's first enter in the order they were created (the oracle's node
    numbering; its action node index is the engine's), each in the first
    bucket from its home (ovf_hash & bucket_mask, then b + 1 & bucket_mask)
    with a free slot, and every arrival at a child probes the buckets from its
    home to its own.  Returns (the search's probes, entries at home in each
    bucket, entries outside their home bucket).  max_depth as map_need's."""
    kids = {}
    for (an, okey), c in p.children.items():
        kids.setdefault(an, []).append((c, okey))
    entries, stack = [], [(p.root, 0)]
    while stack:
        node, d = stack.pop()
        b = p.on_block[node]
        if b < 0 or (max_depth is not None and d + 1 > max_depth):
            continue
        for a in range(p.A):
            ch = kids.get(b * p.A + a, [])
            entries.extend((c, b * p.A + a, okey) for c, okey in ch[ISLOTS:])
            stack.extend((c, d + 1) for c, _ in ch)
    fill, homes, probes, away = [0] * buckets, [0] * buckets, 0, 0
    for c, an, okey in sorted(entries):
        h = ovf_hash(an, okey) % buckets
        homes[h] += 1
        k = 0
        while fill[(h + k) % buckets] >= BUCKET:
            k += 1
        fill[(h + k) % buckets] += 1
        away += k > 0
        probes += p.on_visits[c] * (k + 1)
    return probes, tuple(homes), away


def oracle_episodes(S, tree, plan):
    """The episodes plan = [(env seed, steps), ...] played in turn on ONE oracle
    planner keyed (seed, tree), reset between them (its streams carry on).  Per
    episode (len, records, needs, lookups); needs[t] = map_need (after the
    update, after the search, after the search without the cut-off children);
    lookups = the first search's (map_lookups, map_model in two buckets) with all
    children and without the cut-off ones."""
    p = make_oracle(TEST_CFG, S, ego=EGO, tree=tree, env=ENV)
    out = []
    for n, (seed, K) in enumerate(plan):
        if n:
            p.reset()
        recs, needs, lookups = [], [], []

        def step(obs):
            if p.on_abs[p.root]:
                recs.append(oracle_record(p, False, p.step(obs)))
                needs.append(None)
                return p.last_action
            p.stats = {"searched": True}       # (OraclePOMCP.step, with the tree read in between)
            p.update(p.last_action, obs)
            after_update = map_need(p)
            p.last_action = p.get_action()
            needs.append((after_update, map_need(p), map_need(p, p.cfg.depth_limit)))
            if not lookups:
                lookups.extend((map_lookups(p, d), map_model(p, 2, d))
                               for d in (None, p.cfg.depth_limit))
            recs.append(oracle_record(p, True, p.last_action))
            return p.last_action

        trace = run_episode(step, seed, ego=EGO, max_steps=K, env=ENV)
        out.append((trace["len"], recs, needs, tuple(lookups)))
    return out


def _played(ep, K):
    n, recs = ep[:2]
    return n >= K and all(r["searched"] and r.get("num_sims") for r in recs)


@functools.lru_cache(maxsize=None)
def planted_planners(S, B, K, first):
    """B planners that play a planting episode of PRE_K steps (env seed s) and a
    main episode of K steps (env seed s + 500), both searched at every step, as
    the tests here and tests/test_gpu_parity.py choose theirs; the planting
    episode puts entries in the map on every search kernel (a need > 0 without
    the cut-off children).  Returns (planting seeds, main seeds, expected
    records of both episodes in a row, the main episode's needs)."""
    pre, seeds, exp, needs = [], [], [], []
    s = first
    while len(seeds) < B:
        e0, e1 = oracle_episodes(S, len(seeds), [(s, PRE_K), (s + 500, K)])
        if _played(e0, PRE_K) and _played(e1, K) and any(n[2] > 0 for n in e0[2]):
            pre.append(s)
            seeds.append(s + 500)
            exp.append(e0[1] + e1[1])
            needs.append(e1[2])
        s += 1
    return pre, seeds, exp, needs


# planner keys (seed 0, tree key) whose first search overflows a home bucket of two
# even without the cut-off children; found by playing keys 0..699 on the oracle
# (every planner's first search starts from PursuitEvasion's one initial
# observation, so its map is a function of the key alone).  Env seed 4400 + key.
LOADED_KEYS = (82, 116, 234, 245)


@functools.lru_cache(maxsize=None)
def loaded_planners(S, K):
    """The planners LOADED_KEYS (no planting episode): their K-step episodes
    never need more than two buckets of entries, and their first search sends
    more than 16 entries to one home bucket of two on every search kernel.
    Returns (keys, seeds, expected records, needs, the first search's (lookups,
    map_model) with all children and without the cut-off ones)."""
    seeds, exp, needs, lookups = [], [], [], []
    for key in LOADED_KEYS:
        (e,) = oracle_episodes(S, key, [(4400 + key, K)])
        assert _played(e, K) and max(n[1] for n in e[2]) <= 2 * BUCKET, key
        assert all(max(model[1]) > BUCKET and model[2] > 0 for _, model in e[3]), (key, e[3])
        seeds.append(4400 + key)
        exp.append(e[1])
        needs.append(e[2])
        lookups.append(e[3])
    return LOADED_KEYS, seeds, exp, needs, lookups


# ------------------------------------------------------------------ the engine
def make_engine(S, B, searches, overflow_slots=None, tree_key_base=0):
    from posggym_baselines_amd import _native as N
    from posggym_baselines_amd.planning import BatchedPOMCP
    from posggym_baselines_amd.planning.engine import plan_capacities
    model = product_model(ENV)
    cfg = product_config(TEST_CFG, S)
    caps = None
    if overflow_slots is not None:
        caps = plan_capacities(cfg, model.spec.max_episode_steps, S, searches, reroot=True,
                               overflow_slots=overflow_slots,
                               num_actions=model.action_spaces[EGO].n)
    bp = BatchedPOMCP(model, EGO, cfg, B, S, searches=searches, reroot=True, capacities=caps,
                      tree_key_base=tree_key_base)
    assert N.load().pomcp_debug_set_inline_slots(bp.engine._ctx, ISLOTS) == 0
    return bp


def plant(bp, pre_seeds, records):
    """The planting episode and a reset; every map then holds stale entries only."""
    for _ in lockstep(bp, ENV, EGO, pre_seeds, PRE_K, records):
        pass
    bp.engine.reset()


def play(bp, seeds, K, records, scans=None, search_scans=None, probes=None, after_update=None):
    """K lockstep steps; scans / search_scans: every tree's map scan after each
    update / search; probes: each search's overflow-map probes, per tree."""
    def hook(t):
        if after_update is not None:
            after_update(t)
        if scans is not None:
            scans.append(map_scan(bp.engine))
    for _, stats in lockstep(bp, ENV, EGO, seeds, K, records, after_update=hook):
        if search_scans is not None:
            search_scans.append(map_scan(bp.engine))
        if probes is not None:
            probes.append([int(st.n_probes) for st in stats])


def searched_need(search_kernel, need):
    """The live entries after a search: all of the oracle's, or (a deferring
    search) those without the cut-off children."""
    return need[2] if search_kernel == "lane" else need[1]


def assert_records(got, exp, seeds):
    for b in range(len(seeds)):
        for t, (g, e) in enumerate(zip(got[b], exp[b])):
            assert g == e, f"tree {b} (env seed {seeds[b]}) record {t}"
        assert len(got[b]) == len(exp[b]), b


# -------------------------------------------------------------- a. k_reset's wrap
def test_reset_at_the_last_generation_clears_the_map():
    """A reset at generation kEpochMask leaves every map empty at generation 1;
    the same reset at generation 5,000 leaves the planted entries (stale) at
    5,001.  Both engines then play K = 3 steps equal to the oracle's second
    episode on one planner."""
    S, K, B = 128, 3, 6
    pre, seeds, exp, needs = planted_planners(S, B, K, 4400)
    for gen in (EPOCH_MASK, TWIN_GEN):
        bp = make_engine(S, B, max(K, PRE_K))
        records = [[] for _ in range(B)]
        plant(bp, pre, records)
        planted = map_scan(bp.engine)
        print("generation", gen, "planted:", planted)
        assert all(live == 0 and stale > 0 and g == PLANTED for live, stale, g in planted)
        set_map_generation(bp.engine, gen)
        bp.engine.reset()
        after = map_scan(bp.engine)
        print("after the reset:", after)
        if gen == EPOCH_MASK:
            assert after == [(0, 0, 1)] * B
        else:
            assert [(live, g) for live, _, g in after] == [(0, TWIN_GEN + 1)] * B
            assert [stale for _, stale, _ in after] == [stale for _, stale, _ in planted]
        scans = []
        play(bp, seeds, K, records, scans=scans)
        bp.close()
        assert_records(records, exp, seeds)
        for t in range(K):   # (an initial update makes no generation; each re-root one)
            assert [g for _, _, g in scans[t]] == [advance(after[0][2], t)] * B
            assert [live for live, _, _ in scans[t]] == [needs[b][t][0] for b in range(B)], t


# ------------------------------------------------------------ b. k_restore's wrap
def test_restore_at_the_last_generation_clears_the_map():
    """Snapshot after the second episode's initial update, one search (entries
    of the planted generation), then a restore at generation kEpochMask: empty
    maps at generation 1 (at 5,000: the entries stay, stale, at 5,001) and the
    next search is the oracle's first step again, as in
    test_rekey_survives_restore."""
    S, B = 128, 6
    pre, seeds, exp, needs = planted_planners(S, B, 3, 4400)
    first = [e[:PRE_K + 1] for e in exp]
    for gen in (EPOCH_MASK, TWIN_GEN):
        bp = make_engine(S, B, PRE_K)
        records = [[] for _ in range(B)]
        plant(bp, pre, records)
        play(bp, seeds, 1, records, after_update=lambda t: bp.engine.snapshot())
        assert_records(records, first, seeds)
        searched = map_scan(bp.engine)
        assert all(stale > 0 and g == PLANTED for _, stale, g in searched)
        set_map_generation(bp.engine, gen)
        bp.restore()
        after = map_scan(bp.engine)
        print("generation", gen, "searched:", searched, "restored:", after)
        if gen == EPOCH_MASK:
            assert after == [(0, 0, 1)] * B
        else:
            assert all(live == 0 and stale > 0 and g == TWIN_GEN + 1 for live, stale, g in after)
        actions = bp.search()
        stats = bp.engine.root_stats()
        for b in range(B):
            got = stats_record(stats[b], bp.engine.A, True, actions[b], bp.engine.root_belief(b))
            assert got == first[b][PRE_K], f"tree {b} (env seed {seeds[b]})"
        bp.close()


# ------------------------------------------------------------ c. k_compact's wrap
def test_reroot_at_the_last_generation_rebuilds_the_map_under_generation_1(search_kernel):
    """70 planners (two search waves sharing logs), K = 5: the second episode
    starts at generation kEpochMask + 1 - 2, since its initial update makes no
    generation and each of its re-roots one, so the SECOND re-root wraps:
    k_compact copies the live entries out, clears the map and re-inserts them
    under generation 1.  After that update every tree has generation 1, no
    stale entry, and as many live entries as the twin engine that plays the
    same episodes from generation 5,000 (which still holds stale ones there)
    -- the number the oracle's tree needs.  All steps bit-exact, the map
    probed in every search."""
    S, K, B = 128, 5, 70
    wrap_at = 2                                # the update (t = 2) that wraps
    start = EPOCH_MASK + 1 - wrap_at           # 16,382
    pre, seeds, exp, needs = planted_planners(S, B, K, 4400)
    runs = {}
    for gen in (start, TWIN_GEN):
        bp = make_engine(S, B, K)
        records = [[] for _ in range(B)]
        plant(bp, pre, records)
        set_map_generation(bp.engine, gen)
        scans, probes = [], []
        play(bp, seeds, K, records, scans=scans, probes=probes)
        bp.close()
        print("generation", gen, "probes:", [sum(n) for n in probes], "tree 0's scans:", [s[0] for s in scans],
              "stale entries after update", wrap_at, ":", sum(s[1] for s in scans[wrap_at]))
        assert_records(records, exp, seeds)
        assert all(sum(n) > 0 for n in probes), probes
        runs[gen] = scans
    wrapped, twin = runs[start], runs[TWIN_GEN]
    assert [g for _, _, g in wrapped[0]] == [start] * B
    assert [g for _, _, g in wrapped[wrap_at - 1]] == [EPOCH_MASK] * B
    for t in range(wrap_at, K):
        assert [g for _, _, g in wrapped[t]] == [1 + t - wrap_at] * B, t
    assert [stale for _, stale, _ in wrapped[wrap_at]] == [0] * B
    assert all(stale > 0 for _, stale, _ in twin[wrap_at])
    for t in range(K):
        assert [g for _, _, g in twin[t]] == [TWIN_GEN + t] * B, t
        live = [live for live, _, _ in wrapped[t]]
        assert live == [live for live, _, _ in twin[t]], t
        assert live == [needs[b][t][0] for b in range(B)], t
    assert sum(live for live, _, _ in wrapped[wrap_at]) > 0   # (there was something to re-insert)


# ------------------------------------------- e. generations with the high bits set
def test_high_generations_are_only_a_tag(search_kernel):
    """The same K = 5 step episodes from generations 1, 8,190 (bit 63 of the
    key is set from 8,192 on: the episode's third re-root) and 16,300 (all the
    key's high bits, no wrap): equal to the oracle, with the oracle's number of
    live entries after every update and every search.  The planting episode
    runs from generation 100 here (set on the empty maps): from the default one
    its entries would carry generations 2 and 3, which the run from 1 reaches."""
    S, K, B = 128, 5, 8
    pre_gen = 100
    pre, seeds, exp, needs = planted_planners(S, B, K, 4400)
    for gen in (1, 8190, 16300):
        bp = make_engine(S, B, K)
        set_map_generation(bp.engine, pre_gen)
        records = [[] for _ in range(B)]
        plant(bp, pre, records)
        planted = map_scan(bp.engine)
        assert all(live == 0 and stale > 0 and g == pre_gen + PRE_K for live, stale, g in planted)
        set_map_generation(bp.engine, gen)
        scans, searches = [], []
        play(bp, seeds, K, records, scans=scans, search_scans=searches)
        bp.close()
        print("generation", gen, "live after the updates:", [[s[0] for s in sc] for sc in scans],
              "after the searches:", [[s[0] for s in sc] for sc in searches])
        assert_records(records, exp, seeds)
        for t in range(K):
            assert [g for _, _, g in scans[t]] == [gen + t] * B
            assert [g for _, _, g in searches[t]] == [gen + t] * B
            assert [live for live, _, _ in scans[t]] == [needs[b][t][0] for b in range(B)], t
            assert [live for live, _, _ in searches[t]] == \
                [searched_need(search_kernel, needs[b][t]) for b in range(B)], t
        assert sum(live for live, _, _ in searches[K - 1]) > 0
    assert 8190 + K - 1 >= 8192 and 16300 + K - 1 <= EPOCH_MASK


# ------------------------------------------------------------- f. a loaded map
LOADED = dict(S=256, K=4)


def test_probe_chains_wrap_round_a_two_bucket_map(search_kernel):
    """overflow_slots = 32 (two buckets of 16, bucket_mask = 1), one engine per
    planner of LOADED_KEYS.  Their first search hashes 17 to 20 entries to
    bucket 1, on every search kernel, so 1 to 4 of them take the
    b = (b + 1) & bucket_mask step -- round to bucket 0 -- when they are
    inserted and at every later arrival.  Checked three ways: the records are
    the oracle's over K = 4 steps (re-roots' rebuilds and inserts included);
    the live entries after every update and search are the oracle's need; and
    the first search's n_probes is the restated map's (map_model) exactly, which
    exceeds the search's map lookups (the oracle's arrivals at children beyond
    an action node's first).
    Load reached after the first search (S = 256): 26, 29, 26 and 29 live
    entries of 32 slots where the search looks the cut-off children up
    ("lane_eager", "wave": load factors 0.81 to 0.91) and 26, 26, 26 and 27
    where it defers them ("lane": 0.81 to 0.84); no episode needs more than 29.
    Not reached at these sizes: a bucket-0 overflow (PursuitEvasion's single
    initial observation gives every first search the same root keys, which
    hash 2:1 to bucket 1) and a chain in the re-root's lookups (ovf_lookup,
    k_compact, k_compact_log), whose subtrees need at most 5 entries here."""
    S, K = LOADED["S"], LOADED["K"]
    keys, seeds, exp, needs, lookups = loaded_planners(S, K)
    v = 1 if search_kernel == "lane" else 0          # (without / with the cut-off children)
    for i, key in enumerate(keys):
        bp = make_engine(S, 1, K, overflow_slots=2 * BUCKET, tree_key_base=key)
        assert bp.engine.capacities.overflow_slots == 2 * BUCKET
        records = [[]]
        scans, searches, probes = [], [], []
        play(bp, [seeds[i]], K, records, scans=scans, search_scans=searches, probes=probes)
        bp.close()
        looked, (model_probes, homes, away) = lookups[i][v]
        print("planner key", key, "needs:", needs[i], "live after the searches:",
              [sc[0][0] for sc in searches], "probes:", [n[0] for n in probes],
              "first search: lookups", looked, "model", (model_probes, homes, away))
        assert_records(records, [exp[i]], [seeds[i]])
        for t in range(K):
            assert scans[t][0][0] == needs[i][t][0], (key, t)
            assert searches[t][0][0] == searched_need(search_kernel, needs[i][t]), (key, t)
        assert BUCKET < searches[0][0][0] <= 2 * BUCKET
        assert probes[0][0] == model_probes > looked, (key, probes[0], model_probes, looked)
        assert all(n[0] > 0 for n in probes), probes


# --------------------------------------------------------------- g. a full map
def test_a_full_map_reports_arena_then_a_new_context_searches(search_kernel):
    """The same planners with overflow_slots = 16: their first search needs more
    entries than the map has, which is POMCP_E_ARENA with the tree named (the
    designed return of ovf_child's exhausted probe loop), and after close() a
    new context with a planned map searches the oracle's first step."""
    from posggym_baselines_amd import _native as N
    S, K = LOADED["S"], LOADED["K"]
    keys, seeds, exp, needs, _ = loaded_planners(S, K)
    assert all(searched_need(search_kernel, n[0]) > BUCKET for n in needs)
    for i, key in enumerate(keys):
        bp = make_engine(S, 1, 1, overflow_slots=BUCKET, tree_key_base=key)
        try:
            assert bp.engine.capacities.overflow_slots == BUCKET
            bp.engine.update(np.full(1, -1, dtype=np.int32), first_obs_keys([seeds[i]]))
            out = np.zeros(1, dtype=np.int32)
            rc = bp.engine._lib.pomcp_search(bp.engine._ctx, S,
                                             out.ctypes.data_as(C.POINTER(C.c_int32)))
            assert rc == N.POMCP_E_ARENA, key
            err = bp.engine._lib.pomcp_last_error(bp.engine._ctx)
            assert b"tree 0: arena capacity exceeded" in err, err
        finally:
            bp.close()
        bp = make_engine(S, 1, 1, tree_key_base=key)
        try:
            assert bp.engine.capacities.overflow_slots > 2 * BUCKET
            records = [[]]
            play(bp, [seeds[i]], 1, records)
            assert_records(records, [exp[i][:1]], [seeds[i]])
        finally:
            bp.close()


def first_obs_keys(seeds):
    """The ego's first observation key of each environment (gpu_util.lockstep's)."""
    from oracle.envs import make_model
    from oracle.episode import ENV_TREE_BASE
    from oracle.rng import Streams
    keys = []
    for s in seeds:
        e = make_model(ENV, Streams(s, ENV_TREE_BASE))
        keys.append(e.pack_obs(e.sample_initial_obs(e.sample_initial_state())[EGO]))
    return np.array(keys, dtype=np.uint64)



# ------------------------------------------------- d. the queue refill's wrap
QUEUE = dict(S=32, B=70, N=240, first=7000, searches=100)
TIMING = {"time", "search_time", "update_time", "mem_usage"}


class QueueWatch:
    """run_episode_queue's on_step: tests/test_gpu_episode_queue.py's
    QueueRecorder, plus every finished entry's searched steps (its re-roots are
    those but the first) and the map scan of a slot right after a refill of
    interest -- its tree is empty then, before the new episode's first update.
    watch: {slot: the refill (1, 2, ...) to scan}; None: every slot's first two."""

    def __init__(self, B, N, watch=None):
        from test_gpu_episode_queue import QueueRecorder
        self.rec = QueueRecorder(B, N)
        self.watch = watch
        self.searched = [None] * N
        self.refills = [0] * B
        self.scans = {}

    def __call__(self, t, bp):
        fin_q, fin = bp.episode_queue_finished()
        for b in np.nonzero(fin_q >= 0)[0]:
            self.searched[int(fin_q[b])] = int(fin["res"]["searched_steps"][b])
        self.rec(t, bp)
        for b in sorted(self.rec.refilled[-1]):
            self.refills[b] += 1
            k = self.refills[b]
            if (k <= 2) if self.watch is None else (self.watch.get(b) == k):
                self.scans[(b, k)] = map_scan(bp.engine, [b])[0]


def queue_run(generations, watch):
    q = QUEUE
    seeds = list(range(q["first"], q["first"] + q["N"]))
    bp = make_engine(q["S"], q["B"], q["searches"])
    if generations is not None:
        set_map_generation(bp.engine, generations)
    w = QueueWatch(q["B"], q["N"], watch)
    rows = bp.run_episode_queue(seeds, until="agent_done", on_step=w)
    final = map_scan(bp.engine)
    bp.close()
    assert all(n is not None for n in w.searched)
    return seeds, rows, w, final


def slot_episodes(rows, b):
    return sorted((r for r in rows if r["slot"] == b), key=lambda r: r["slot_order"])


def increments(rows, w, b, episodes=None):
    """The generations slot b made up to the refill after its first `episodes`
    episodes (None: to the end of the call): the reset of
    pomcp_episodes_queue_begin, a re-root per searched step but the first of
    every episode, and a refill after every episode but the slot's last."""
    mine = slot_episodes(rows, b)
    part = mine if episodes is None else mine[:episodes]
    n = 1 + sum(w.searched[r["num"]] - 1 for r in part)
    return n + (len(mine) - 1 if episodes is None else episodes)


@functools.lru_cache(maxsize=None)
def queue_twin():
    """The queue played from the default generation (no wrap anywhere), once for
    all search kernels (they are bit-identical): the schedule the wrapping run's
    starting generations are derived from, and its twin."""
    seeds, rows, w, final = queue_run(None, None)
    for b in range(QUEUE["B"]):
        assert final[b][2] == advance(FRESH, increments(rows, w, b)), b
    return seeds, rows, w, final


def test_queue_refills_wrap_some_trees_of_a_wave_and_leave_the_others_alone():
    """B = 70 slots, N = 240 seeds, until agent_done: every slot refills at least
    twice.  Starting generations per slot, from the twin run's schedule: two
    slots of the first search wave whose first episodes end in the same batch
    step start at 16,384 - (1 + re-roots of the first episode + 1), so both
    wrap at their first refill and one wave of k_queue_refill clears both maps
    in turn while other trees of the wave are mid-episode; a third starts so
    that its second refill wraps; one slot of the second wave wraps at its
    first refill; every other slot starts at 5,000 + slot and never wraps.
    Rows and per-step records equal the twin's for every entry and the serial
    harness's for the wrapping slots and two others (the parity statement of
    tests/test_gpu_episode_queue.py); a wrapped slot's map reads (0, 0, 1)
    right after its refill, where the twin's still holds stale entries; every
    slot ends at the generation its refills and re-roots add up to."""
    from collections import Counter
    from test_gpu_episode_queue import check_slot
    B, S = QUEUE["B"], QUEUE["S"]
    seeds, trows, tw, tfinal = queue_twin()
    played = Counter(r["slot"] for r in trows)
    assert min(played[b] for b in range(B)) >= 3          # every slot refills at least twice
    first_len = {b: slot_episodes(trows, b)[0]["len"] for b in range(B)}
    common = Counter(first_len[b] for b in range(64)).most_common(1)[0][0]
    together = [b for b in range(64) if first_len[b] == common][:2]
    assert len(together) == 2
    second = next(b for b in range(64) if b not in together)
    other_wave = 66
    watch = {together[0]: 1, together[1]: 1, second: 2, other_wave: 1}
    gens = [TWIN_GEN + b for b in range(B)]
    for b, k in watch.items():
        gens[b] = EPOCH_MASK + 1 - increments(trows, tw, b, episodes=k)
    print("first episodes of", common, "steps:", together, "second refill:", second,
          "second wave:", other_wave, "generations:", {b: gens[b] for b in watch})
    seeds, rows, w, final = queue_run(gens, watch)
    # --- parity: every entry against the twin, the chosen slots against the serial harness
    assert len(rows) == len(trows) == QUEUE["N"]
    for r, tr in zip(rows, trows):
        assert list(r) == list(tr)
        for k in r:
            if k not in TIMING:
                assert fhex(float(r[k])) == fhex(float(tr[k])), (r["num"], k)
    assert w.rec.steps == tw.rec.steps and w.searched == tw.searched
    for b in list(watch) + [0, B - 1]:
        check_slot(rows, w.rec, b, ENV, seeds, "agent_done", ego=EGO, num_sims=S)
    # --- the wraps: an empty map at generation 1 right after the refill
    print("scans after the watched refills:", w.scans, "the twin's:",
          {k: tw.scans[k] for k in w.scans})
    assert sorted(w.scans) == sorted(watch.items())
    for key, scan in w.scans.items():
        assert scan == (0, 0, 1), key
        assert tw.scans[key][0] == 0 and tw.scans[key][1] > 0, key
    # both maps of the first wave cleared by one launch, other trees mid-episode
    t = common - 1
    assert set(together) <= w.rec.refilled[t] and w.rec.mid[t] & set(range(64))
    # --- every slot's generation, from what it did
    for b in range(B):
        assert final[b][2] == advance(gens[b], increments(rows, w, b)), b
        last = slot_episodes(rows, b)[-1]
        if watch.get(b) == played[b] - 1 and w.searched[last["num"]] <= 1:
            assert final[b][1] == 0, b       # wrapped at its last refill, no re-root since
    assert all(advance(gens[b], increments(rows, w, b)) > TWIN_GEN for b in range(B)
               if b not in watch)            # (the other slots never wrapped)
