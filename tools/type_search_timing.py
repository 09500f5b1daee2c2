"""Time one type-based search launch (k_search<TM = 1>) on Driving-v1 with an
IPOMCP mixture of fixed distributions and with a mixture of shortest-path
agents {A100, A40, A0}: 4,096 trees x 256 simulations from synthetic roots,
one warmed-up search each, a host clock around the synchronising call.

    python tools/type_search_timing.py [--trees 4096] [--sims 256] [--out FILE]

POMCP_LIB_PATH selects another build of the library (a parent commit's, which
has no reactive kinds: the reactive mixture is then skipped)."""
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
           action_selection="pucb", pucb_exploration_fraction=0.25, known_bounds=None,
           step_limit=None, epsilon=0.92, seed=0, state_belief_only=False)
FIXED = {"o_u": [0.2] * 5, "o_fast": [0.05, 0.7, 0.05, 0.1, 0.1], "o_turn": [0.3, 0.1, 0.1, 0.4, 0.1]}
REACTIVE = [f"Driving-v1/A{g}Shortestpath-v0" for g in (100, 40, 0)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--trees", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=256)
    ap.add_argument("--out", default="-")
    args = ap.parse_args()
    import torch
    from posggym_baselines_amd import _native
    from posggym_baselines_amd.envs import DrivingModel
    from posggym_baselines_amd.planning import (BatchedPOMCP, MCTSConfig, OtherAgentMixturePolicy,
                                                RandomSearchPolicy)
    from posggym_baselines_amd.planning.ipomcp import base_type_tables
    from posggym_baselines_amd.planning.policies import FixedDistributionPolicy, ShortestPathPolicy
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    model = DrivingModel()
    cfg = MCTSConfig(num_sims=args.sims, **CFG)
    mixtures = {"fixed_three": {k: FixedDistributionPolicy(model, "1", k, v)
                                for k, v in FIXED.items()}}
    if hasattr(_native.load(), "pomcp_set_type_policy_kinds"):
        mixtures["shortest_path_three"] = {k: ShortestPathPolicy.from_id(model, "1", k)
                                           for k in REACTIVE}
    rec = {"trees": args.trees, "sims": args.sims, "device": torch.cuda.get_device_name(0)}
    for name, pols in mixtures.items():
        tp = base_type_tables(model, "0", cfg, {"1": OtherAgentMixturePolicy(model, "1", pols)},
                              RandomSearchPolicy(model, "0"))
        bp = BatchedPOMCP(model, "0", cfg, args.trees, args.sims, type_policies=tp)
        try:
            bp.init_synthetic(1000)
            bp.search()                      # the untimed warm-up
            bp.restore()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bp.search()
            ms = (time.perf_counter() - t0) * 1e3
        finally:
            bp.close()
        rec[name] = {"search_ms": ms, "simulations_per_s": args.trees * args.sims / ms * 1e3}
        print(name, json.dumps(rec[name]), flush=True)
    if args.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
