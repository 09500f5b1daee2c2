"""The case selection of tests/test_gpu_intmcp_limits.py, on the oracle alone:
what that module assumes about its 70-pair workloads before it cuts an arena
to the size one of them needs -- few enough pairs tie at the top that a run one
short fails at most three of them, the 16-slot obs-child map is overrun by some
pairs and filled past half by others, and nearly every pair-step searches (an
episode that ends at once would test nothing)."""
import pytest

from gpu_util import (IM_LIMITS_CASES, IM_LIMITS_PAIRS, IM_LIMITS_STEPS, IM_ROOT_BELIEF_FLOOR,
                      IM_TABLE_CASES, im_limits_cfg, nested_table_need, oracle_arena_peaks,
                      oracle_intmcp_limits, product_config, product_model)

# Not pinned here: the two 1,030-pair cases of section e (Driving, nesting 1, 2
# steps; 8 simulations per level on env seeds 7000 + b for max_nodes, 64 on
# 18000 + b for max_root_belief).  Their oracle takes 7 s and 60 s on all 1,030
# pairs, so the GPU test asserts the tie condition on the device's own counters
# and root belief sizes, which equal the oracle's wherever the oracle is run.
# The seeds were found on the oracle alone: with 64 simulations per level the
# second step's root belief cannot exceed 44 particles, and of the first seeds
# 7000, 12000, 14000, ..., 25000 only 18000 leaves a single pair (645) at 44
# (the others two to seven); at 8 per level on 7000 + b pair 407 alone needs 61
# nodes.
#
# The nested history tables (gpu_util.IM_TABLE_CASES, section f): a table of a
# tree k >= 2 binds max_root_belief only where the batch's largest one is above
# both intmcp_create's floor of 22 and the batch's largest root belief, and the
# root beliefs grow faster with the simulations than the tables do.  Found on
# the oracle alone, 70 pairs x 3 steps on env seeds first + b, written as
# largest nested table / largest root belief:
#   * first seed 3000: Driving nesting 2 at 16 / 24 / 32 / 64 / 128 simulations
#     per level 15/11, 18/19, 22/27, 51/76, 111/187; Driving nesting 3 at 16 /
#     24 14/12, 18/19; PursuitEvasion nesting 2 at 16 / 24 / 32 / 48 / 64 12/11,
#     16/17, 17/26, 28/40, 35/60; nesting 3 at 16 13/12 -- none binds;
#     PursuitEvasion nesting 3 at 32 does: 26/25, pair 42 alone, in tree 3 (the
#     level-0 tree: im_update_nestN's tail) at the third update, a re-root.
#   * nesting 2: first seeds 3000 .. 6000 at 24, 28, 32, 36, 40 and 48 per level
#     on both environments leave the root belief 1 to 14 ahead, closest on
#     Driving at 28 to 32.  Driving at 28, 30 and 32 on the first seeds 7000,
#     8000, ..., 60000 (162 workloads): only 32 per level on 16000 + b binds,
#     29/28, pair 24 alone, tree 2 (the level-0 tree again), third update.
#   * the middle-tree call site (tree 2 of a nesting-3 planner): first seeds
#     4000, 5000, ..., 15000 of PursuitEvasion nesting 3 at 24 and 32 and
#     Driving nesting 3 at 24 and 32: only PursuitEvasion at 32 on 5000 + b
#     binds, 24/23, pair 48 alone, tree 2, third update.
# Every binding table is built by a re-root (the third update); the initial
# update's tables are far smaller (11 particles per belief).
# Not pinned here, as above: the 1,030-pair case, 3 steps.  Of PursuitEvasion
# and Driving nesting 3 at 26, 28 and 30 per level on the first seeds 7000,
# 18000, 30000 and 42000 (24 workloads, the oracle a minute each on one core),
# and PursuitEvasion nesting 3 at 16, 24 and 32, Driving nesting 3 at 24 and
# nesting 2 at 32 on 7000 (32 also on 18000), only Driving nesting 3 at 26 per
# level on 7000 + b binds: 23/22, pair 952 alone, tree 3.
PAIR_STEPS = IM_LIMITS_PAIRS * IM_LIMITS_STEPS
MAX_TIES = 3          # pairs that may fail in a run one short
MAP_FLOOR = 16        # intmcp_create's smallest hash_slots
MAP_CASES = (("Driving-v1", 1, 64), ("PursuitEvasion-v1", 1, 96))
SUPPORT_CASES = (("Driving-v1", 1, 32), ("Driving-v1", 2, 16), ("PursuitEvasion-v1", 0, 32))
ROOT_CASE = ("Driving-v1", 1, 64)
UPDATE_CASES = (("Driving-v1", 1, 4), ("Driving-v1", 2, 4))


def arena_sims(nesting):
    return 16 if nesting == 2 else 32


def searched(batch):
    return sum(bool(r["searched"]) for x in batch.values() for r in x["records"])


def ties(needs):
    top = max(needs)
    return top, sorted(b for b, n in enumerate(needs) if n == top)


@pytest.mark.parametrize("env,nesting", IM_LIMITS_CASES)
def test_at_most_three_pairs_share_an_arena_peak(env, nesting):
    """Section b: per arena, the pairs whose largest count (over their trees
    and the samples after every update and search) is the batch's."""
    batch = oracle_intmcp_limits(env, nesting, arena_sims(nesting))
    assert searched(batch) >= 150
    for which, name in enumerate(("nodes", "log", "stats")):
        peaks, trees = oracle_arena_peaks(batch, which)
        top, tied = ties([peaks[b] for b in range(IM_LIMITS_PAIRS)])
        print(env, nesting, name, "top", top, "pairs", tied, "tree", [trees[b] for b in tied])
        assert 1 <= len(tied) <= MAX_TIES
        # the call and search level in which a tied pair reaches the peak: what
        # the GPU module's docstring says of the fail site each run reaches
        for b in tied:
            x = batch[b]
            j = next(j for j, c in enumerate(x["counts"]) if max(r[which] for r in c) == top)
            assert x["calls"][j] == (IM_LIMITS_STEPS - 1, "search"), (name, b)
            level = next(lv for lv, c in enumerate(x["levels"][j])
                         if max(r[which] for r in c) == top)
            if nesting == 0:
                assert level == 0 and trees[b] == 1      # the planner's own tree
            elif name == "nodes":
                assert level == nesting and trees[b] > 0   # the history extension


@pytest.mark.parametrize("env,nesting,sims", UPDATE_CASES)
def test_at_most_three_pairs_share_the_node_peak_of_an_update(env, nesting, sims):
    """Section b, the episode that ends on its third update: that update
    reaches the largest node count."""
    batch = oracle_intmcp_limits(env, nesting, sims, last_search=False)
    assert sum(len(x["root_sizes"]) for x in batch.values()) >= 150   # pair-steps updated
    peaks, _ = oracle_arena_peaks(batch, 0)
    top, tied = ties([peaks[b] for b in range(IM_LIMITS_PAIRS)])
    assert 1 <= len(tied) <= MAX_TIES
    for b in tied:
        x = batch[b]
        first = next(j for j, c in enumerate(x["counts"]) if max(r[0] for r in c) == top)
        assert x["calls"][first] == (IM_LIMITS_STEPS - 1, "update")


@pytest.mark.parametrize("env,nesting", IM_LIMITS_CASES)
@pytest.mark.parametrize("sims", [1, 2, 3])
def test_smallest_budgets_search(env, nesting, sims):
    """Section a: 1, 2 and 3 simulations per level still search."""
    batch = oracle_intmcp_limits(env, nesting, sims)
    assert 150 <= searched(batch) <= PAIR_STEPS


@pytest.mark.parametrize("env,nesting,sims", MAP_CASES)
def test_map_floor_fails_some_pairs_and_fills_for_others(env, nesting, sims):
    """Section c: a pair's need is its largest tree's children beyond two
    inline slots per (node, action)."""
    batch = oracle_intmcp_limits(env, nesting, sims)
    assert searched(batch) >= 150
    need = [max(batch[b]["map_need"]) for b in range(IM_LIMITS_PAIRS)]
    over = [b for b, n in enumerate(need) if n > MAP_FLOOR]
    high = [b for b, n in enumerate(need) if 9 <= n <= MAP_FLOOR]
    print(env, sims, "over", len(over), "9 to 16", len(high))
    assert len(over) >= 3 and len(high) >= 5
    # the pairs over the floor pass it in different calls, some before the last:
    # calls follow a failure, with the failed pairs skipped
    calls = {batch[b]["calls"][next(j for j, m in enumerate(batch[b]["map_series"])
                                    if max(m) > MAP_FLOOR)] for b in over}
    assert len(calls) > 1 and min(calls) < (IM_LIMITS_STEPS - 1, "search")


@pytest.mark.parametrize("env,nesting,sims", SUPPORT_CASES)
def test_at_most_three_pairs_share_the_support_peak(env, nesting, sims):
    """Section d: the materialised particles of the largest table."""
    batch = oracle_intmcp_limits(env, nesting, sims)
    assert searched(batch) >= 150
    top, tied = ties([max(batch[b]["support_series"]) for b in range(IM_LIMITS_PAIRS)])
    print(env, nesting, "support top", top, "pairs", tied)
    assert len(tied) <= MAX_TIES


def test_at_most_three_pairs_share_the_root_belief_peak():
    """Section d: the largest root belief is above 2 x (num_particles +
    extra_particles) = 22, the least intmcp_create takes, so the bound binds."""
    env, nesting, sims = ROOT_CASE
    batch = oracle_intmcp_limits(env, nesting, sims)
    top, tied = ties([max(batch[b]["root_sizes"]) for b in range(IM_LIMITS_PAIRS)])
    print("root belief top", top, "pairs", tied)
    assert top > 22 and len(tied) <= MAX_TIES


@pytest.mark.parametrize("env,nesting,sims,first,top,tied", IM_TABLE_CASES)
def test_a_nested_table_binds_the_root_belief_capacity(env, nesting, sims, first, top, tied):
    """Section f: (a) the batch's largest table of a tree k >= 2 -- the ones
    im_support_nested fills -- is above both intmcp_create's floor and the
    largest root belief, so max_root_belief cut to it, less one, fails a pair
    in im_support_nested and nowhere else; (b) at most three pairs hold it; (c)
    the pairs search.  Which update builds it and in which tree is pinned,
    and the pair after each such pair (whose table the GPU test reads back)
    plays that step.  plan_intmcp_capacities leaves room for it."""
    batch = oracle_intmcp_limits(env, nesting, sims, first_seed=first)
    pairs = range(IM_LIMITS_PAIRS)
    nested, got_top, got_tied, other = nested_table_need(
        [batch[b]["entry_series"] for b in pairs], [batch[b]["root_sizes"] for b in pairs])
    print(env, nesting, sims, first, "nested top", got_top, "at (step, tree)", got_tied,
          "root beliefs and floor", other)
    assert got_top > other >= IM_ROOT_BELIEF_FLOOR                     # (a)
    assert 1 <= len(got_tied) <= MAX_TIES                              # (b)
    assert searched(batch) >= 150                                      # (c)
    assert (got_top, got_tied) == (top, tied)
    # a table of tree 1 holds at most one history per root particle
    assert all(e[0] <= r for b in pairs
               for e, r in zip(batch[b]["entry_series"], batch[b]["root_sizes"]))
    for b, (t, k) in tied.items():
        assert t >= 1, "a re-root (the initial tables are the oracle's first update)"
        assert b + 1 < IM_LIMITS_PAIRS and b + 1 not in tied
        assert len(batch[b + 1]["tables"]) > t, "the next pair updates in that step"
        assert [len(tab) for tab in batch[b + 1]["tables"][t]] == batch[b + 1]["entry_series"][t]
    from posggym_baselines_amd.planning.intmcp import plan_intmcp_capacities
    model, pcfg = product_model(env), product_config(im_limits_cfg(), sims)
    caps = plan_intmcp_capacities(pcfg, pcfg.step_limit or model.spec.max_episode_steps, sims,
                                  IM_LIMITS_STEPS, model.action_spaces["0"].n, nesting)
    assert caps.max_root_belief >= top


def test_nested_table_cases_reach_both_call_sites():
    """im_update_nestN calls im_support_nested in its middle-tree loop (tree k
    < L of a nesting-L planner, L = 3) and for the level-0 tree (k = L): the
    cases fail a pair at each, and one is a nesting-2 workload."""
    sites = {("middle" if k < nesting else "level-0")
             for _, nesting, _, _, _, tied in IM_TABLE_CASES for _, k in tied.values()}
    assert sites == {"middle", "level-0"}
    assert 2 in {nesting for _, nesting, *_ in IM_TABLE_CASES}
