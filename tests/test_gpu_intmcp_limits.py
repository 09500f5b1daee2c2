"""I-NTMCP (csrc/intmcp.hip) at its capacity checks and its smallest simulation
budgets, bit for bit against oracle/intmcp.py -- what tests/
test_gpu_search_invariants.py is for the POMCP kernels.  Every other I-NTMCP
test runs on plan_intmcp_capacities' worst-case sizes, where no arena fills and
the obs-child map stays under half full; here an arena is cut to exactly what
the workload needs, then to one less, and the pairs that do not fit must say
so -- ImPair::fail(POMCP_E_ARENA) -- without a byte of their neighbours
changing: node Nn of a pair's tree k is node 0 of its tree k + 1, and the 64
pairs of a wave share slabs, so a check that is off by one rewrites another
tree's root and faults nowhere.

The workload (gpu_util.IntmcpLockstep, the lockstep episode of
batched_intmcp_episodes through the C ABI): 70 planner pairs -- two search
workgroups, the second six pairs wide, so its slabs have another stride --
pair b on tree key b and env seed 3000 + b, BASE_CFG of tests/golden/
make_oracle_digests.py, 3 steps: an initial update and two re-roots with
reinvigoration.  The driver keeps every call's return code and message, reads
intmcp_get_tree_counts after every update and search, and skips a pair from
the call in which its error appears while the others play on.  The oracle's
side (gpu_util.oracle_intmcp_limits) is computed once per configuration; the
conditions on the cases are pinned on the oracle alone by tests/
test_intmcp_limits_cases.py.

Which one-short run reaches which fail site (the pair intmcp_last_error names
and the call are the ones predicted from the run at planned capacity; the
search level from the failed pair's num_sims):
  new_node through the pair's own tree ....... max_nodes, Driving nesting 0
      (search, tree 1 = the planner's own; simulate's child_rec)
  new_node through the history extension ..... max_nodes, nesting 1 and 2: the
      last search's top level, whose simulations reach the tree below only by
      simulate's second child_rec
  new_node from an update ..................... max_nodes at 4 simulations per
      level with the episode ending on its third update (reinvig_top's and, at
      nesting 2, reinvig_mid's step -> child)
  the statistics allocation ................... max_stats (expand_known / reg)
  log_add ..................................... max_log (tree 0 at nesting >= 1)
  the map probe (child_rec) ................... hash_slots = 16 (searches of the
      second and third step, either level)
  im_extract_support .......................... max_support_particles at a re-root
  im_extract_root, a wave per pair ............ max_root_belief, 70 pairs
  im_extract_root, a lane per pair ............ max_root_belief, 1,030 pairs
  im_support_nested, the level-0 tree ......... max_root_belief at nesting 2 and 3,
      env seeds chosen so that a nested table is above every root belief
      (section f); a lane per pair: 1,030 pairs at nesting 3
  im_support_nested, a middle tree ............ max_root_belief, nesting 3, tree 2
"""
import functools

import numpy as np
import pytest

from gpu_util import (IM_LIMITS_CASES, IM_LIMITS_FIRST_SEED, IM_LIMITS_PAIRS, IM_LIMITS_STEPS,
                      IM_TABLE_CASES, IntmcpLockstep, im_limits_cfg, nested_table_need,
                      oracle_intmcp_limits)

pytestmark = pytest.mark.gpu

B, STEPS, FIRST = IM_LIMITS_PAIRS, IM_LIMITS_STEPS, IM_LIMITS_FIRST_SEED
E_ARENA = -3                       # POMCP_E_ARENA (include/pomcp.h)
ARENAS = {"max_nodes": 0, "max_log": 1, "max_stats": 2}     # intmcp_get_tree_counts' columns
MAX_TIES = 3


def arena_sims(nesting):
    return 16 if nesting == 2 else 32


def planned(env, nesting, sims, steps=STEPS, **fields):
    """plan_intmcp_capacities for the workload, with `fields` replaced."""
    from gpu_util import product_config, product_model
    from posggym_baselines_amd.planning.intmcp import plan_intmcp_capacities
    model = product_model(env)
    pcfg = product_config(im_limits_cfg(), sims)
    caps = plan_intmcp_capacities(pcfg, pcfg.step_limit or model.spec.max_episode_steps, sims, steps,
                                  model.action_spaces["0"].n, nesting)
    for k, v in fields.items():
        assert hasattr(caps, k), k
        setattr(caps, k, v)
    return caps


def device(env, nesting, sims, pairs=B, first=FIRST, steps=STEPS, **kw):
    return IntmcpLockstep(im_limits_cfg(), sims, range(first, first + pairs), steps, env=env,
                          nesting_level=nesting, **kw)


@functools.lru_cache(maxsize=None)
def unconstrained(env, nesting, sims, last_search=True, support=False, scans=False):
    """The run at planned capacity, shared by the tests that cut it."""
    return device(env, nesting, sims, last_search=last_search, support=support, scans=scans)


def call_index(t, what):
    return 2 * t + (what == "search")


def assert_ok(run):
    for c in run.calls:
        assert c["rc"] == 0 and not c["errors"].any(), (c["step"], c["what"], c["message"])
    assert run.failed == {}


def assert_records(run, exp, pairs=None):
    """Every pair's records are the oracle's; a failed pair's, those of the
    steps before its failure."""
    for b in exp if pairs is None else pairs:
        want = exp[b]["records"]
        if b in run.failed:
            t = run.calls[run.failed[b]]["step"]
            assert len(run.records[b]) == t, (b, t)
            want = want[:t]
        assert len(run.records[b]) == len(want), f"pair {b}: steps"
        for t, (g, e) in enumerate(zip(run.records[b], want)):
            assert g == e, f"pair {b} step {t}"


def assert_counts(run, exp):
    """n_nodes, n_log and n_stats of every pair and tree after every update and
    search of a step the pair played: the oracle's trees."""
    for b, x in exp.items():
        for (t, what), want in zip(x["calls"], x["counts"]):
            got = run.calls[call_index(t, what)]["counts"][b].tolist()
            assert got == want, f"pair {b} step {t} {what}: [tree][nodes, log, stats]"


def searched(exp):
    return sum(bool(r["searched"]) for x in exp.values() for r in x["records"])


# ------------------------------------------------------- a. smallest budgets
@pytest.mark.parametrize("env,nesting", IM_LIMITS_CASES)
@pytest.mark.parametrize("sims", [1, 2, 3])
def test_one_two_and_three_simulations_per_level(env, nesting, sims):
    """The search keeps look-ahead RNG words across levels and launches
    (la_fill, la_pend) and prefetches the next simulation's root particle: with
    1, 2 and 3 simulations per level a word drawn or dropped once too often
    shows in the records of this step or the next.  The arena counters after
    every call are the oracle's trees: n_nodes = len(tree.parent), n_stats = A
    x the nodes that hold a registered real action, n_log = the particles its
    beliefs had appended (nothing is compacted away within three steps: the
    update keeps the records of nodes at t >= the root's - 2).  At nesting 0
    the planner's tree is tree 1 and tree 0 stays an empty root (1, 0, 0)."""
    exp = oracle_intmcp_limits(env, nesting, sims)
    run = device(env, nesting, sims)
    assert_ok(run)
    assert_records(run, exp)
    n = searched(exp)
    print(env, nesting, sims, "searched pair-steps:", n, "of", B * STEPS)
    assert run.searched() == n
    assert_counts(run, exp)


def assert_calls(run, base, predicted):
    """Call by call of a run in which the pairs of `predicted` ({pair: index of
    the call that fails it}) do not fit: each fails in that call and in no
    other; every call before the first failure returns 0, that call and every
    later one POMCP_E_ARENA with intmcp_last_error naming the lowest pair that
    has failed so far; every pair's error is set from its call on and 0
    before; and the counters of the pairs that have not failed are those of
    `base`, the run at planned capacity."""
    assert run.failed == predicted
    assert len(run.calls) == len(base.calls)
    n = len(run.calls[0]["errors"])
    for i, c in enumerate(run.calls):
        down = sorted(b for b, at in predicted.items() if at <= i)
        assert c["errors"].tolist() == [E_ARENA if b in down else 0 for b in range(n)], i
        if not down:
            assert c["rc"] == 0, (i, c["message"])
        else:
            assert c["rc"] == E_ARENA, i
            assert c["message"] == f"{c['what']}: pair {down[0]}: status {E_ARENA}", (i, c["message"])
        ok = [b for b in range(n) if b not in down]
        assert (c["counts"][ok] == base.calls[i]["counts"][ok]).all(), i


# ------------------------------------ b. nodes, log, statistics: full and short
def one_short(env, nesting, sims, field, base, need, crossing, exp, on_full=None, **kw):
    """The capacity `field` at top = the largest need of a pair, then at top -
    1.  need[b]: pair b's; crossing[b]: the call in which its need passed top -
    1 in the run `base` at planned capacity.  Returns the run one short and
    the pairs it fails.  on_full: further checks of the run exactly full."""
    top = max(need)
    short_of = [b for b in range(len(need)) if need[b] == top]
    print(field, "top", top, "pairs", short_of, "calls", [crossing[b] for b in short_of])
    assert 1 <= len(short_of) <= MAX_TIES
    which = ARENAS.get(field)
    checked = exp.keys()

    steps = kw.get("steps", STEPS)
    full = device(env, nesting, sims, pairs=len(need),
                  capacities=planned(env, nesting, sims, steps, **{field: top}), **kw)
    assert_ok(full)
    assert_records(full, exp, checked)
    for c, c1 in zip(full.calls, base.calls):
        assert (c["counts"] == c1["counts"]).all(), (c["step"], c["what"])
    if on_full is not None:
        on_full(full)

    short = device(env, nesting, sims, pairs=len(need),
                   capacities=planned(env, nesting, sims, steps, **{field: top - 1}), **kw)
    assert_calls(short, base, {b: crossing[b] for b in short_of})
    if which is not None:   # a full arena allocates nothing, in any pair
        for i, c in enumerate(short.calls):
            assert int(c["counts"][:, :, which].max()) <= top - 1, i
    assert_records(short, exp, checked)
    return short, short_of


def search_level(short, b, sims, nesting):
    """The search level whose simulation failed in pair b, `sims` per level,
    from its num_sims: k_im_search and the top level of k_im_searchN count the
    failing simulation, k_im_searchN's lower levels leave it out."""
    c = short.calls[short.failed[b]]
    assert c["what"] == "search"
    n = int(c["num_sims"][b])
    if nesting >= 2:
        assert n != nesting * sims
        return n // sims if n < nesting * sims else nesting
    return max(0, (n - 1) // sims)


@pytest.mark.parametrize("env,nesting", IM_LIMITS_CASES)
@pytest.mark.parametrize("field", list(ARENAS))
def test_arena_exactly_full_and_one_short(env, nesting, field):
    """The capacity is per tree, so a pair's need is its largest tree's count,
    over the samples after every update and search; the counters only grow, so
    that is the count at the pair's last call.  With exactly the largest need
    every pair fits; with one less, the pairs that needed it -- no others --
    report POMCP_E_ARENA in the call in which the first run's count passed the
    capacity, their counters never above it, and every other pair's records and
    counters stay the oracle's to the end of the episode.  For these seeds that
    call is the third step's search for every pair at a peak (asserted here and
    on the oracle in tests/test_intmcp_limits_cases.py), so no call follows a
    failure in this section; sections c and d have failures in earlier calls
    and pairs skipped afterwards.  The search level of the failing simulation
    is the one in which the oracle's tree passed the capacity: level 0 in the
    planner's own tree at nesting 0 (simulate's first child_rec); for
    max_nodes at nesting >= 1 the top level, which reaches the tree below only
    through the history extension (simulate's second child_rec)."""
    sims, which = arena_sims(nesting), ARENAS[field]
    exp = oracle_intmcp_limits(env, nesting, sims)
    first = unconstrained(env, nesting, sims)
    assert_ok(first)
    assert_records(first, exp)
    assert_counts(first, exp)
    per_tree = np.stack([c["counts"][:, :, which] for c in first.calls])   # [call][pair][tree]
    need = per_tree.max(axis=(0, 2)).tolist()
    top = max(need)
    crossing = [int(np.argmax(per_tree[:, b].max(axis=1) > top - 1)) for b in range(B)]
    bound = sorted({int(per_tree[-1, b].argmax()) for b in range(B) if need[b] == top})
    print(env, "nesting", nesting, field, "binds in tree", bound)
    short, short_of = one_short(env, nesting, sims, field, first, need, crossing, exp)
    for b in short_of:
        i = short.failed[b]
        # (the counters only grow, so a pair passes the largest need in its
        # last call: no call follows the failure here -- the calls after one,
        # with the failed pair skipped, are sections c and d's)
        assert i == call_index(STEPS - 1, "search"), (b, i)
        t = short.calls[i]["step"]
        levels = exp[b]["levels"][exp[b]["calls"].index((t, "search"))]
        want = next(lv for lv, c in enumerate(levels) if max(row[which] for row in c) > top - 1)
        got = search_level(short, b, sims, nesting)
        print("  pair", b, "step", t, "search level", got, "of", len(levels) - 1)
        assert got == want, b
        if field == "max_nodes" and nesting >= 1:
            assert got == nesting and bound != [0], (got, bound)   # the history extension's new_node


UPDATE_CASES = (("Driving-v1", 1, 4), ("Driving-v1", 2, 4))


@pytest.mark.parametrize("env,nesting,sims", UPDATE_CASES)
def test_node_arena_full_in_an_update(env, nesting, sims):
    """An update allocates nodes where it reinvigorates a belief whose
    particles carry a history: every attempt extends the other agent's history
    in the tree below (reinvig_top and reinvig_mid: step -> child -> new_node).
    A root belief of 32 simulations is never short of particles, so this case
    has 4 per level, and the episode ends on its third update: the largest node
    count (the bottom tree's at nesting 1 and for the one nesting-2 pair at the
    top) is reached by that update, and the run one short fails in
    intmcp_update, which returns POMCP_E_ARENA with "update: pair ..."."""
    exp = oracle_intmcp_limits(env, nesting, sims, last_search=False)
    first = unconstrained(env, nesting, sims, last_search=False)
    assert_ok(first)
    assert_records(first, exp)
    assert_counts(first, exp)
    per_tree = np.stack([c["counts"][:, :, 0] for c in first.calls])
    need = per_tree.max(axis=(0, 2)).tolist()
    crossing = [int(np.argmax(per_tree[:, b].max(axis=1) > max(need) - 1)) for b in range(B)]
    short, short_of = one_short(env, nesting, sims, "max_nodes", first, need, crossing, exp,
                                last_search=False)
    for b in short_of:
        assert short.calls[short.failed[b]]["what"] == "update", b
        assert short.failed[b] == call_index(STEPS - 1, "update")


def test_fresh_context_after_a_run_with_failed_pairs():
    """Nothing of a run in which pairs failed (max_nodes = 200, below what many
    of the pairs need) outlives its context: a new one at planned capacity
    plays the oracle's records."""
    env, nesting, sims = "Driving-v1", 1, 32
    exp = oracle_intmcp_limits(env, nesting, sims)
    short = device(env, nesting, sims, capacities=planned(env, nesting, sims, max_nodes=200))
    assert short.failed and short.calls[-1]["rc"] == E_ARENA
    run = device(env, nesting, sims)
    assert_ok(run)
    assert_records(run, exp)
    assert_counts(run, exp)


# --------------------------------------- c. the obs-child map at its 16 slots
@pytest.mark.parametrize("env,nesting,sims", [("Driving-v1", 1, 64), ("PursuitEvasion-v1", 1, 96)])
def test_obs_child_map_at_its_floor(env, nesting, sims):
    """hash_slots = 16, intmcp_create's least.  A tree's need is its (node,
    action)s' children beyond the two inline slots of the action's record
    (every action's, the None action's included) -- intmcp_debug_arena_scan's
    occupied slots at the end of a run at planned capacity, and the oracle's
    tree.children say the same; child_rec is the map's only writer and only
    intmcp_reset / intmcp_reset_pairs clear it, so nothing leaves within an
    episode.  A pair whose trees all need at most 16 plays the oracle's records
    with probe chains that wrap past slot 15 in a table up to 100 % full; a
    pair with a tree that needs more reports POMCP_E_ARENA from child_rec's
    probe loop, that tree's table holding exactly 16 entries, in the call --
    and, in a search, at the level -- in which the oracle's tree gains its
    17th entry (gpu_util's "map_series" / "map_levels"); the pairs fail in
    different calls from the second step's search on, so the calls after a
    failure, with the failed pairs skipped, are checked one by one
    (assert_calls); both groups' neighbours are untouched."""
    exp = oracle_intmcp_limits(env, nesting, sims)
    first = unconstrained(env, nesting, sims, scans=True)
    assert_ok(first)
    assert_records(first, exp)
    assert first.scans == [exp[b]["map_need"] for b in range(B)]
    need = [max(s) for s in first.scans]
    over = [b for b in range(B) if need[b] > 16]
    high = [b for b in range(B) if 9 <= need[b] <= 16]
    print(env, sims, "pairs over 16:", over, "at 9 to 16:", len(high), "full:", need.count(16))
    assert len(over) >= 3 and len(high) >= 5
    # the call that needs a tree's 17th entry, from the oracle's trees after
    # every update and search, and the search level within it
    predicted, level = {}, {}
    for b in over:
        x = exp[b]
        j = next(j for j, need_j in enumerate(x["map_series"]) if max(need_j) > 16)
        predicted[b] = call_index(*x["calls"][j])
        if x["map_levels"][j] is not None:
            level[b] = next(lv for lv, m in enumerate(x["map_levels"][j]) if max(m) > 16)
    print("  failing calls (pair: call, search level):",
          {b: (predicted[b], level.get(b)) for b in over})
    assert len(set(predicted.values())) > 1 and min(predicted.values()) < len(first.calls) - 1
    run = device(env, nesting, sims, capacities=planned(env, nesting, sims, hash_slots=16), scans=True)
    assert_calls(run, first, predicted)
    for b in over:
        if b in level:
            assert search_level(run, b, sims, nesting) == level[b], b
        else:
            assert run.calls[run.failed[b]]["what"] == "update", b
    for b in range(B):
        if b in over:
            assert [s for s, n in zip(run.scans[b], first.scans[b]) if n > 16] == \
                [16] * sum(n > 16 for n in first.scans[b]), (b, run.scans[b], first.scans[b])
            assert all(s <= 16 for s in run.scans[b]), b
        else:
            assert run.scans[b] == first.scans[b], b
    assert_records(run, exp)


# --------------------------------------- d. support particles and root belief
def series_need(series, n):
    """(need per pair, the update call in which each pair's series first
    reaches the largest need)."""
    need = [max(s) if s else 0 for s in series[:n]]
    top = max(need)
    crossing = [call_index(next((t for t, v in enumerate(s) if v >= top), 0), "update")
                for s in series[:n]]
    return need, crossing


@pytest.mark.parametrize("env,nesting,sims", [("Driving-v1", 1, 32), ("Driving-v1", 2, 16),
                                              ("PursuitEvasion-v1", 0, 32)])
def test_support_particles_exactly_full_and_one_short(env, nesting, sims):
    """max_support_particles holds the materialised beliefs of one table: a
    pair's need is the largest off + cap its support (and, at nesting 2, its
    middle tree's table) shows after an update -- at a re-root, per history its
    logged particles and room for a reinvigoration's accepted and rejected
    samples, which the oracle's beliefs give as well
    (oracle_intmcp_limits_pair).  One short, im_extract_support finds the sum
    of the caps above the capacity and fails the pair before it writes a
    particle (the initial beliefs are checked per particle and need less)."""
    exp = oracle_intmcp_limits(env, nesting, sims)
    first = unconstrained(env, nesting, sims, support=True)
    assert_ok(first)
    assert_records(first, exp)
    assert first.support_series == [exp[b]["support_series"] for b in range(B)]
    need, crossing = series_need(first.support_series, B)
    short, short_of = one_short(env, nesting, sims, "max_support_particles", first, need, crossing,
                                exp, support=True)
    for b in short_of:
        assert short.calls[short.failed[b]]["step"] >= 1, b   # a re-root: im_extract_support


def test_root_belief_exactly_full_and_one_short():
    """max_root_belief (Nr) is tested where a root belief is written: the
    initial belief (n_target particles), the extraction at a re-root
    (im_extract_root: the log records of the new root, E of them) and
    reinvig_top's room for accepted and rejected samples above them (E + 2 x
    (n_target - E) <= 2 x n_target when E < n_target); the entry tables and
    probabilities hold one slot per distinct history of at most that many
    particles.  intmcp_create takes no Nr below 2 x n_target, so a pair's need
    is max(2 x n_target, its largest E), and a root belief above n_target was
    not reinvigorated: its size after the update is E.  64 simulations per
    level make the largest root belief 76, against 2 x n_target = 22.  A wave
    per pair here (it tests n + popc(batch) > Nr per 64 records); the lane per
    pair update is test_1030_pairs_root_belief_exactly_full_and_one_short."""
    env, nesting, sims = "Driving-v1", 1, 64
    exp = oracle_intmcp_limits(env, nesting, sims)
    first = unconstrained(env, nesting, sims, scans=True)
    assert_ok(first)
    assert first.root_sizes == [exp[b]["root_sizes"] for b in range(B)]
    need, crossing = series_need(first.root_sizes, B)
    assert max(need) > 22
    one_short(env, nesting, sims, "max_root_belief", first, need, crossing, exp)


# ------------------------------ e. the lane-per-pair update (over 1,024 pairs)
BIG, BIG_FIRST, BIG_STEPS = 1030, 7000, 2


def big_checked(failing):
    """The pairs compared with the oracle: the search workgroups that hold a
    failing pair and the partial last one."""
    groups = sorted({b // 64 for b in failing})
    return tuple(b for g in groups for b in range(64 * g, 64 * g + 64)) + tuple(range(1024, BIG))


def big_full_and_short(sims, field, series_of, first_seed=BIG_FIRST):
    first = device("Driving-v1", 1, sims, pairs=BIG, first=first_seed, steps=BIG_STEPS, record=())
    assert_ok(first)
    need, crossing = series_of(first)
    top = max(need)
    failing = [b for b in range(BIG) if need[b] == top]
    assert len(failing) <= MAX_TIES
    checked = big_checked(failing)
    exp = oracle_intmcp_limits("Driving-v1", 1, sims, pairs=checked, first_seed=first_seed,
                               steps=BIG_STEPS)
    short, short_of = one_short("Driving-v1", 1, sims, field, first, need, crossing, exp,
                                first=first_seed, steps=BIG_STEPS, record=checked)
    assert short_of == failing
    return first, short


def test_1030_pairs_node_arena_exactly_full_and_one_short():
    """1,030 Driving pairs, nesting 1, 8 simulations per level, 2 steps: the
    update runs a lane per pair.  max_nodes at the largest need and one short;
    the pairs of the failing pairs' workgroups and of the partial last one are
    compared with the oracle, every other pair's errors and counters with the
    run at planned capacity."""
    def nodes(first):
        per_tree = np.stack([c["counts"][:, :, 0] for c in first.calls])
        need = per_tree.max(axis=(0, 2)).tolist()
        crossing = [int(np.argmax(per_tree[:, b].max(axis=1) > max(need) - 1)) for b in range(BIG)]
        return need, crossing
    big_full_and_short(8, "max_nodes", nodes)


BIG_ROOT_SIMS, BIG_ROOT_FIRST = 64, 18000


def test_1030_pairs_root_belief_exactly_full_and_one_short():
    """im_extract_root in the lane-per-pair update, which tests n >= Nr per
    record where the wave-per-pair update tests n + popc(batch) > Nr per 64
    records: both must fail the pairs whose extracted belief is above the
    capacity, and no others.  With 8 simulations per level no root belief
    comes near 2 x n_target = 22, the least intmcp_create takes (a re-rooted
    belief holds at most the simulations that passed through it: 11 after
    every update of such a run), so this case has 64 per level, whose largest
    second-step beliefs are 44, on env seeds 18000 + b, where one of the 1,030
    pairs reaches that."""
    def roots(first):
        return series_need(first.root_sizes, BIG)
    first, short = big_full_and_short(BIG_ROOT_SIMS, "max_root_belief", roots, first_seed=BIG_ROOT_FIRST)
    assert max(max(s) for s in first.root_sizes) > 22
    for b, i in short.failed.items():
        assert short.calls[i]["what"] == "update" and short.calls[i]["step"] == 1, b


# --------------------------- f. the nested history tables at max_root_belief
def table_need(run, n):
    """nested_table_need of a run at planned capacity, and per pair the update
    call in which a table of a tree k >= 2 first reaches the largest."""
    nested, top, tied, other = nested_table_need(run.n_entries[:n], run.root_sizes[:n])
    crossing = [call_index(next((t for t, e in enumerate(es) if max(e[1:]) >= top), 0), "update")
                for es in run.n_entries[:n]]
    return nested, top, tied, other, crossing


def neighbours(tied, n):
    """The pairs before and after the pairs of `tied`: entry Nr of a pair's
    tables and probabilities is entry 0 of the next pair's."""
    return tuple(sorted({c for b in tied for c in (b - 1, b + 1) if 0 <= c < n and c not in tied}))


def assert_tables(run, exp, watch):
    for b in watch:
        assert len(run.tables[b]) == len(exp[b]["tables"]), b
        for t, (got, want) in enumerate(zip(run.tables[b], exp[b]["tables"])):
            assert got == want, f"pair {b} update {t}: [tree][(history, particles)]"


def assert_table_bound(short, base, exp, tied, top, watch):
    """The run one short of the largest nested table: each pair of `tied` ({pair:
    (step, tree k)}) fails in that step's update, the tables of its trees above
    k already this update's and those of tree k and below still the previous
    update's (the caller returned at once: no selector flipped, no count
    advanced), no table above the capacity and no counter above its arena;
    every other pair's table sizes and root beliefs are the planned run's to
    the end; and the tables of the pairs next to a failed one, read back after
    every update -- the failing one and those after it -- are the oracle's:
    histories in order, sizes and particles."""
    caps = short.capacities
    assert caps.max_root_belief == top - 1
    limits = np.array([caps.max_nodes, caps.max_log, caps.max_stats])
    for b, (t, k) in tied.items():
        c = short.calls[short.failed[b]]
        assert (c["what"], c["step"]) == ("update", t), b
        want = base.n_entries[b][t][:k - 1] + base.n_entries[b][t - 1][k - 1:]
        print("  pair", b, "fails at step", t, "tree", k, "tables", short.failed_entries[b])
        assert short.failed_entries[b] == want, b
        assert max(want) <= top - 1
        assert short.n_entries[b] == base.n_entries[b][:t], b
        assert short.root_sizes[b] == base.root_sizes[b][:t], b
        for c in short.calls:
            assert (c["counts"][b] <= limits).all(), (b, c["step"], c["what"])
    for b in range(len(base.n_entries)):
        if b not in tied:
            assert short.n_entries[b] == base.n_entries[b], b
            assert short.root_sizes[b] == base.root_sizes[b], b
    assert_tables(short, exp, watch)


@pytest.mark.parametrize("env,nesting,sims,first,top,tied", IM_TABLE_CASES)
def test_nested_table_exactly_full_and_one_short(env, nesting, sims, first, top, tied):
    """At nesting 2 and 3 an update builds, for every tree k >= 2, the table of
    the distinct histories carried by the particles of tree k - 1's beliefs
    (im_support_nested), one slot of the pair's [2][Nr] tables and [Nr]
    probabilities each -- often more histories than the root belief has
    particles.  The cases (gpu_util.IM_TABLE_CASES, pinned on the oracle by
    tests/test_intmcp_limits_cases.py) are those whose largest such table is
    above every root belief and above intmcp_create's floor, so that
    max_root_belief cut to it is exactly full for that table alone, and one
    less fails the pairs that hold it in im_support_nested: in the middle-tree
    loop of im_update_nestN (tree 2 at nesting 3) or at its tail (the level-0
    tree).  Exactly full, every pair is the oracle's: records, counters, table
    sizes.  One short: assert_calls and assert_table_bound."""
    exp = oracle_intmcp_limits(env, nesting, sims, first_seed=first)
    base = device(env, nesting, sims, first=first, support=True)
    assert_ok(base)
    assert_records(base, exp)
    assert_counts(base, exp)
    assert base.n_entries == [exp[b]["entry_series"] for b in range(B)]
    assert base.root_sizes == [exp[b]["root_sizes"] for b in range(B)]
    assert base.support_series == [exp[b]["support_series"] for b in range(B)]
    nested, got_top, got_tied, other, crossing = table_need(base, B)
    print(env, nesting, sims, first, "nested top", got_top, got_tied, "root beliefs and floor", other)
    assert got_top > other                                   # (a) the table binds, nothing else
    assert (got_top, got_tied) == (top, tied)                # (b) the pairs the oracle names
    watch = neighbours(tied, B)
    assert all(b + 1 in watch for b in tied)

    def full_too(full):
        assert full.capacities.max_root_belief == top
        assert full.n_entries == base.n_entries
        assert_tables(full, exp, watch)

    short, short_of = one_short(env, nesting, sims, "max_root_belief", base, nested, crossing, exp,
                                on_full=full_too, first=first, support=True, tables=watch)
    assert short_of == sorted(tied)
    assert_table_bound(short, base, exp, tied, top, watch)


TABLE_BIG = ("Driving-v1", 3, 26, 7000, 3)


def test_1030_pairs_nested_table_exactly_full_and_one_short():
    """im_support_nested in the lane-per-pair update (k_im_updateN<.., false>:
    more than 1,024 pairs), where a slot past the table is a neighbouring
    lane's.  1,030 Driving pairs, nesting 3, 26 simulations per level, 3 steps
    on env seeds 7000 + b (tests/test_intmcp_limits_cases.py records the scan):
    the need and the tie condition come from the device's own table sizes and
    root beliefs at planned capacity; the oracle is run on the workgroups of
    the failing pairs (their successors among them) and the partial last
    one."""
    env, nesting, sims, first, steps = TABLE_BIG
    base = device(env, nesting, sims, pairs=BIG, first=first, steps=steps, record=(),
                  support="entries")
    assert_ok(base)
    nested, top, tied, other, crossing = table_need(base, BIG)
    print(env, nesting, sims, first, "nested top", top, tied, "root beliefs and floor", other)
    assert top > other                                       # (a)
    assert 1 <= len(tied) <= MAX_TIES                        # (b)
    watch = neighbours(tied, BIG)
    checked = tuple(sorted(set(big_checked(tied)) | set(watch)))
    exp = oracle_intmcp_limits(env, nesting, sims, pairs=checked, first_seed=first, steps=steps)
    for b in checked:
        assert base.n_entries[b] == exp[b]["entry_series"], b
        assert base.root_sizes[b] == exp[b]["root_sizes"], b

    def full_too(full):
        assert full.capacities.max_root_belief == top
        assert full.n_entries == base.n_entries
        assert_tables(full, exp, watch)

    short, short_of = one_short(env, nesting, sims, "max_root_belief", base, nested, crossing, exp,
                                on_full=full_too, first=first, steps=steps, record=checked,
                                support="entries", tables=watch)
    assert short_of == sorted(tied)
    assert_table_bound(short, base, exp, tied, top, watch)
