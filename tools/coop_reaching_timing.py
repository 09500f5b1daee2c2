"""Time the lane-per-tree search on CooperativeReaching-v0 beside Driving-v1, and
a batch step of ``BatchedPOMCP.run_episodes`` against the heuristic agents:

    python tools/coop_reaching_timing.py [--trees 65536] [--sims 65536] [--out FILE]

Search: synthetic roots at the benchmark's configuration (bench.py: plain POMCP,
ucb, depth limit 2, deferred cut-off records, no re-root arenas), one untimed
warm-up search and one timed search per environment in the same process, device
time between two events on the engine's stream.  The two environments do
different work per simulation (other observation fan-out, rollout lengths and
terminations), so the Driving-v1 figure is context, not a target.

Episodes: ``--episode-trees`` x ``--episode-sims`` plain planners, one episode
each against the population {H1 .. H5}, ``until="all_done"``; the batch's wall
time per batch step and the device time of its three kernels' groups
(``pomcp_episodes_timing``).

``--potmmcp`` measures the type-based search with state-reactive EGO policies
instead: POTMMCP on CooperativeReaching-v0 ``size=5`` with the
reference's P0 ``softmax`` meta-policy over the heuristics {H1 .. H5}
(tests/golden/reactive_ego/p0_meta_policy.json) and the mixture {H1 .. H5},
beside the same tables with fixed uniform placeholder ego policies, in the same
process (pucb, ``--potmmcp-trees`` x ``--potmmcp-sims``), and one
``run_episodes`` batch of ``--episode-trees`` x ``--episode-sims`` such
planners against {H1 .. H5}."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "posggym-baselines_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

CFG = dict(discount=0.95, search_time_limit=0.1, c=math.sqrt(2), truncated=False,
           action_selection="ucb", pucb_exploration_fraction=0.25, known_bounds=None,
           step_limit=None, epsilon=0.92, state_belief_only=True)
H = [f"CooperativeReaching-v0/H{k}-v0" for k in range(1, 6)]


def potmmcp_tables(model, reactive):
    """The P0 softmax meta-policy's tables over {H1 .. H5} (``reactive``) or over
    fixed uniform placeholders with the same ids, and the mixture's ids."""
    from posggym_baselines_amd.planning import OtherAgentMixturePolicy, POTMMCPMetaPolicy
    from posggym_baselines_amd.planning.policies import FixedDistributionPolicy, GoalHeuristicPolicy
    from posggym_baselines_amd.planning.potmmcp import type_policy_tables
    with open(os.path.join(ROOT, "tests", "golden", "reactive_ego", "p0_meta_policy.json")) as f:
        rows = json.load(f)["meta_policy"]["softmax"]
    ego = {h: GoalHeuristicPolicy.from_id(model, "0", h) if reactive
           else FixedDistributionPolicy.uniform(model, "0", h) for h in H}
    mix = OtherAgentMixturePolicy(model, "1", {h: GoalHeuristicPolicy.from_id(model, "1", h)
                                               for h in H})
    meta = POTMMCPMetaPolicy(model, "0", ego, rows)
    return type_policy_tables(model, "0", meta, mix), list(mix.policies)


def time_search(model, trees, sims, max_blocks, cfg_over=None, type_policies=None):
    import torch
    from posggym_baselines_amd.planning import BatchedPOMCP, MCTSConfig
    from posggym_baselines_amd.planning.engine import plan_capacities
    cfg = MCTSConfig(seed=0, num_sims=sims, **dict(CFG, **(cfg_over or {})))
    caps = plan_capacities(cfg, model.spec.max_episode_steps, sims, 1, reroot=False,
                           max_blocks=min(max_blocks, sims + 64), overflow_slots=1024)
    stream = torch.cuda.Stream(device=0)
    bp = BatchedPOMCP(model, "0", cfg, trees, sims, capacities=caps, stream=stream.cuda_stream,
                      defer_cutoff=True, device=0, type_policies=type_policies)
    try:
        bp.init_synthetic(1000)
        with torch.cuda.stream(stream):
            bp.search(fetch=False)               # the untimed warm-up
            bp.restore()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            bp.search(fetch=False)
            b.record(stream)
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        st = list(bp.engine.root_stats())        # raises on any per-tree error
        done = sum(s.num_sims for s in st)
        rec = {"trees": trees, "sims": sims, "search_ms": ms,
               "simulations_per_s": done / ms * 1e3,
               "levels_per_sim": sum(s.n_levels for s in st) / done,
               "rollout_steps_per_sim": sum(s.n_rollout_steps for s in st) / done,
               "max_blocks_used": max(s.n_blocks for s in st), "max_blocks": caps.max_blocks}
    finally:
        bp.close()
    return rec


def time_episodes(model, trees, sims, first_seed, cfg_over=None, type_policies=None,
                  other_policy_ids=None):
    from posggym_baselines_amd.planning import BatchedPOMCP, MCTSConfig
    from posggym_baselines_amd.planning.policies import GoalHeuristicPolicy
    cfg = MCTSConfig(seed=0, num_sims=sims, **dict(CFG, **(cfg_over or {})))
    pop = [GoalHeuristicPolicy.from_id(model, "1", pid) for pid in H]
    steps = model.spec.max_episode_steps
    bp = BatchedPOMCP(model, "0", cfg, trees, sims, searches=steps, reroot=True,
                      type_policies=type_policies, other_policy_ids=other_policy_ids)
    try:
        bp.run_episodes(range(first_seed, first_seed + trees), until="all_done",
                        other_agents=pop)       # the untimed warm-up batch
        t0 = time.perf_counter()
        rows = bp.run_episodes(range(first_seed + trees, first_seed + 2 * trees),
                               until="all_done", other_agents=pop)
        wall = time.perf_counter() - t0
        (upd, search, step), n = bp.engine.episodes_timing()
    finally:
        bp.close()
    played = sum(r["len"] for r in rows)
    return {"trees": trees, "sims": sims, "batch_steps": n, "episode_steps": played,
            "wall_ms_per_batch_step": wall * 1e3 / n, "update_ms_per_batch_step": upd / n,
            "search_ms_per_batch_step": search / n, "episode_step_ms_per_batch_step": step / n,
            "mean_return": sum(r["return"] for r in rows) / len(rows)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--trees", type=int, default=65536)
    ap.add_argument("--sims", type=int, default=65536)
    ap.add_argument("--max-blocks", type=int, default=768,
                    help="per-tree block arena (a depth-2 5x5 tree under full observation "
                         "expands up to 1 + 25 + 625 observation nodes)")
    ap.add_argument("--episode-trees", type=int, default=4096)
    ap.add_argument("--episode-sims", type=int, default=256)
    ap.add_argument("--potmmcp", action="store_true",
                    help="the type-based search with reactive ego policies (see above)")
    ap.add_argument("--potmmcp-trees", type=int, default=16384)
    ap.add_argument("--potmmcp-sims", type=int, default=4096)
    ap.add_argument("--out", default="-")
    args = ap.parse_args()
    import torch
    from posggym_baselines_amd.envs import CooperativeReachingModel, DrivingModel
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    rec = {"device": torch.cuda.get_device_name(0), "search": {}}
    if args.potmmcp:
        over = {"action_selection": "pucb", "state_belief_only": False}
        model = CooperativeReachingModel(size=5)
        for name, reactive in (("P0 softmax over H1..H5", True), ("fixed placeholders", False)):
            tp, ids = potmmcp_tables(model, reactive)
            rec["search"][name] = time_search(model, args.potmmcp_trees, args.potmmcp_sims,
                                              args.max_blocks, over, tp)
            print(name, json.dumps(rec["search"][name]), flush=True)
        tp, ids = potmmcp_tables(model, True)
        rec["episodes"] = time_episodes(model, args.episode_trees, args.episode_sims, 3000, over,
                                        tp, ids)
        print("episodes", json.dumps(rec["episodes"]), flush=True)
        if args.out != "-":
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(rec) + "\n")
        return 0
    for name, model in (("CooperativeReaching-v0", CooperativeReachingModel()),
                        ("Driving-v1", DrivingModel())):
        rec["search"][name] = time_search(model, args.trees, args.sims, args.max_blocks)
        print(name, json.dumps(rec["search"][name]), flush=True)
    rec["episodes"] = time_episodes(CooperativeReachingModel(), args.episode_trees,
                                    args.episode_sims, 3000)
    print("episodes", json.dumps(rec["episodes"]), flush=True)
    if args.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
