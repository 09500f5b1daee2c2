"""The case selection of tests/test_gpu_intmcp_limits.py, on the oracle alone:
what that module assumes about its 70-pair workloads before it cuts an arena
to the size one of them needs -- few enough pairs tie at the top that a run one
short fails at most three of them, the 16-slot obs-child map is overrun by some
pairs and filled past half by others, and nearly every pair-step searches (an
episode that ends at once would test nothing)."""
import pytest

from gpu_util import (IM_LIMITS_CASES, IM_LIMITS_PAIRS, IM_LIMITS_STEPS, oracle_arena_peaks,
                      oracle_intmcp_limits)

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
