"""Time the lane-per-tree search on PredatorPrey-v0 beside Driving-v1, and a batch
step of ``BatchedPOMCP.run_episodes``:

    python tools/predator_prey_timing.py [--trees 65536] [--sims 2048] [--out FILE]
    python tools/predator_prey_timing.py --agents [--out FILE]

Search: synthetic roots at the benchmark's configuration (bench.py: plain POMCP,
ucb, depth limit 2, deferred cut-off records, no re-root arenas) on the
reference's kwargs (10x10, 3 prey, strength 2, obs_dim 2), one untimed warm-up
search and one timed search per environment in the same process, device time
between two events on the engine's stream.  The two environments do different
work per simulation (the step itself, observation fan-out, rollout lengths and
terminations), so the Driving-v1 figure is context, not a target; the levels
per simulation and the blocks a tree used are recorded beside it.  Both run the
same roots x simulations with the same arena of ``sims + 64`` blocks a tree,
which no search can outgrow (a simulation expands at most one node): three prey
moving by tie bytes give this environment's depth-2 trees nearly a new
observation node per simulation, so the 65,536 simulations a root the other
environments are timed at would need 50 MB of arena a tree.

Episodes: ``--episode-trees`` x ``--episode-sims`` plain planners, one episode
each against a uniform random other predator, ``until="all_done"``; the batch's
wall time per batch step and the device time of its three kernels' groups
(``pomcp_episodes_timing``).

``--agents`` times the heuristic agents H1 .. H3 instead:
the type-based search (IPOMCP, pucb, a three-member mixture) on
``--episode-trees`` x ``--episode-sims`` with three fixed members and with
{H1, H2, H3}, and one ``run_episodes`` batch of plain planners against the
population {H1, H2, H3}."""
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
REF_KWARGS = dict(grid="10x10", num_predators=2, num_prey=3, cooperative=True, prey_strength=2,
                  obs_dim=2)


def time_search(model, trees, sims, max_blocks):
    import torch
    from posggym_baselines_amd.planning import BatchedPOMCP, MCTSConfig
    from posggym_baselines_amd.planning.engine import plan_capacities
    cfg = MCTSConfig(seed=0, num_sims=sims, **CFG)
    caps = plan_capacities(cfg, model.spec.max_episode_steps, sims, 1, reroot=False,
                           max_blocks=min(max_blocks, sims + 64), overflow_slots=1024)
    stream = torch.cuda.Stream(device=0)
    bp = BatchedPOMCP(model, "0", cfg, trees, sims, capacities=caps, stream=stream.cuda_stream,
                      defer_cutoff=True, device=0)
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
               "mean_blocks_used": sum(s.n_blocks for s in st) / len(st),
               "max_blocks_used": max(s.n_blocks for s in st), "max_blocks": caps.max_blocks}
    finally:
        bp.close()
    return rec


def heuristics(model, other="1"):
    from posggym_baselines_amd.planning.policies import (PREDATOR_PREY_POLICY_IDS,
                                                         PreyHeuristicPolicy)
    return [PreyHeuristicPolicy.from_id(model, other, pid) for pid in PREDATOR_PREY_POLICY_IDS]


def time_type_search(model, trees, sims, reactive):
    """One warmed-up type-based search from the initial belief of one
    observation: a mixture of three fixed rows, or of H1 .. H3."""
    import numpy as np
    import torch
    from posggym_baselines_amd.planning import (MCTSConfig, OtherAgentMixturePolicy,
                                                RandomSearchPolicy)
    from posggym_baselines_amd.planning.engine import PomcpEngine
    from posggym_baselines_amd.planning.ipomcp import base_type_tables
    from posggym_baselines_amd.planning.policies import FixedDistributionPolicy
    cfg = MCTSConfig(seed=0, num_sims=sims, **dict(CFG, action_selection="pucb",
                                                   state_belief_only=False))
    rows = ([0.2] * 5, [0.1, 0.1, 0.1, 0.6, 0.1], [0.3, 0.1, 0.1, 0.4, 0.1])
    members = heuristics(model) if reactive else [
        FixedDistributionPolicy(model, "1", f"o{k}", r) for k, r in enumerate(rows)]
    mix = OtherAgentMixturePolicy(model, "1", {p.policy_id: p for p in members})
    tp = base_type_tables(model, "0", cfg, {"1": mix}, RandomSearchPolicy(model, "0"))
    model.seed(1000)
    key = model.obs_key(model.sample_initial_obs(model.sample_initial_state())["0"])
    out = []
    for _ in range(2):                               # the first engine is the warm-up
        eng = PomcpEngine(model, "0", cfg, num_trees=trees, num_sims=sims, searches=1,
                          type_policies=tp)
        try:
            eng.reset()
            eng.update(np.full(trees, -1, dtype=np.int32), np.full(trees, key, dtype=np.uint64))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.search(sims)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            done = sum(s.num_sims for s in eng.root_stats())
        finally:
            eng.close()
        out.append({"trees": trees, "sims": sims, "reactive": bool(reactive), "search_wall_ms": ms,
                    "simulations_per_s": done / ms * 1e3})
    return out[1]


def time_episodes(model, trees, sims, first_seed, other_agents=None):
    from posggym_baselines_amd.planning import BatchedPOMCP, MCTSConfig
    cfg = MCTSConfig(seed=0, num_sims=sims, **CFG)
    steps = model.spec.max_episode_steps
    bp = BatchedPOMCP(model, "0", cfg, trees, sims, searches=steps, reroot=True)
    try:
        bp.run_episodes(range(first_seed, first_seed + trees), until="all_done",
                        other_agents=other_agents)   # warm-up batch
        t0 = time.perf_counter()
        rows = bp.run_episodes(range(first_seed + trees, first_seed + 2 * trees),
                               until="all_done", other_agents=other_agents)
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
    ap.add_argument("--sims", type=int, default=2048,
                    help="simulations per root; the arena is sims + 64 blocks a tree (see above)")
    ap.add_argument("--episode-trees", type=int, default=4096)
    ap.add_argument("--episode-sims", type=int, default=256)
    ap.add_argument("--agents", action="store_true",
                    help="time the heuristic agents H1 .. H3 instead (see above)")
    ap.add_argument("--out", default="-")
    args = ap.parse_args()
    import torch
    from posggym_baselines_amd.envs import DrivingModel, PredatorPreyModel
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    rec = {"device": torch.cuda.get_device_name(0), "kwargs": REF_KWARGS, "search": {}}
    if args.agents:
        model = PredatorPreyModel(**REF_KWARGS)
        for name, reactive in (("fixed_mixture", False), ("heuristic_mixture", True)):
            rec["search"][name] = time_type_search(model, args.episode_trees, args.episode_sims,
                                                   reactive)
            print(name, json.dumps(rec["search"][name]), flush=True)
        for name, pop in (("episodes_uniform", None), ("episodes_heuristics", heuristics(model))):
            rec[name] = time_episodes(PredatorPreyModel(**REF_KWARGS), args.episode_trees,
                                      args.episode_sims, 3000, pop)
            print(name, json.dumps(rec[name]), flush=True)
        if args.out != "-":
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(rec) + "\n")
        return 0
    for name, model in (("PredatorPrey-v0", PredatorPreyModel(**REF_KWARGS)),
                        ("Driving-v1", DrivingModel())):
        rec["search"][name] = time_search(model, args.trees, args.sims, args.sims + 64)
        print(name, json.dumps(rec["search"][name]), flush=True)
    rec["episodes"] = time_episodes(PredatorPreyModel(**REF_KWARGS), args.episode_trees,
                                    args.episode_sims, 3000)
    print("episodes", json.dumps(rec["episodes"]), flush=True)
    if args.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
