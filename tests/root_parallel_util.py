"""Oracle episodes of root-parallel planners, shared by the host and the GPU
tests of ``run_episodes(root_parallel=K)``: planner g of a batch is
``OracleRootParallel`` over K oracle planners keyed (seed, g*K + k), driven by
``oracle.episode.run_episode`` at environment seed ``first_seed + g``.  Computed
once per session and never changed by a test."""
import functools
import math

from oracle.episode import fhex, run_episode
from oracle.root_parallel import OracleRootParallel
from oracle.run import make_oracle

# the configuration of tests/test_gpu_batched_episodes.py (TEST_CFG)
TEST_CFG = dict(discount=0.95, search_time_limit=0.1, c=math.sqrt(2), truncated=False,
                action_selection="ucb", pucb_exploration_fraction=0.25, known_bounds=None,
                step_limit=None, epsilon=0.92, seed=0, state_belief_only=True)
TIMING = {"time", "search_time", "update_time", "mem_usage"}


@functools.lru_cache(maxsize=None)
def oracle_groups(env, ego, K, G, S, first_seed, max_steps):
    """[(trace, records)] per group.  records[t], the planner's side of step t:
    ``searched`` (its root was not absorbing before the step), ``action`` (the
    one played), ``flags`` (every replica's root absorbing after the update),
    and for a searched step ``num_sims`` (K * S, or 0 when the update made every
    replica absorbing), ``search_depth`` (maximum over the replicas that
    searched), ``min_value`` / ``max_value`` (minimum / maximum over the
    replicas' MinMaxStats, which an absorbing replica keeps) and ``merged`` =
    ``oracle.root_parallel.merge_roots``' (action, visits, totals), None when
    nothing was merged."""
    out = []
    for g in range(G):
        ps = [make_oracle(TEST_CFG, S, ego=ego, tree=g * K + k, env=env) for k in range(K)]
        rp = OracleRootParallel(ps, TEST_CFG["action_selection"])
        records = []

        def step(obs, rp=rp, ps=ps, records=records):
            searched = not rp.absorbing()
            a = rp.step(obs)
            rec = {"searched": searched, "action": int(a),
                   "flags": [bool(p.on_abs[p.root]) for p in ps]}
            if searched:
                live = not all(rec["flags"])
                rec.update(
                    num_sims=K * S if live else 0,
                    search_depth=max(p.stats.get("search_depth", 0) for p in ps) if live else 0,
                    min_value=min(p.mm_min for p in ps), max_value=max(p.mm_max for p in ps),
                    merged=None if rp.merged is None else
                    (int(rp.merged[0]), list(rp.merged[1]), list(rp.merged[2])))
            records.append(rec)
            return a

        trace = run_episode(step, first_seed + g, ego=ego, max_steps=max_steps, env=env)
        out.append((trace, records))
    return out


def planner_sums(records):
    """(searched steps, depth sum, simulation sum, min_value sum, max_value sum)
    over the searched steps: integers, and sequential FP64 sums."""
    n = depth = sims = 0
    mn = mx = 0.0
    for r in records:
        if not r["searched"]:
            continue
        n += 1
        depth += r["search_depth"]
        sims += r["num_sims"]
        mn = mn + r["min_value"]
        mx = mx + r["max_value"]
    return n, depth, sims, mn, mx


def shape_facts(groups):
    """What a batch exercises: mixed-absorbing group-steps per group, groups with
    an all-absorbing tail, and the steps each group spends parked."""
    longest = max(t["len"] for t, _ in groups)
    mixed = [sum(1 for r in rec if r["searched"] and any(r["flags"]) and not all(r["flags"]))
             for _, rec in groups]
    tails = [g for g, (_, rec) in enumerate(groups) if not rec[-1]["searched"]]
    parked = [longest - t["len"] for t, _ in groups]
    return mixed, tails, parked


def last_real(records):
    """The record of the group's last real step (searched and merged), or None."""
    real = [r for r in records if r["searched"] and r["merged"] is not None]
    return real[-1] if real else None


def return_bits(steps, gamma):
    ret = disc = 0.0
    for t, s in enumerate(steps):
        r = float.fromhex(s["reward"])
        ret += r
        disc += gamma ** t * r
    return fhex(ret), fhex(disc)
