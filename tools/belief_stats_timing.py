"""Time k_belief_stats (pomcp_belief_stats) against the host route it replaces.

On PursuitEvasion-v1, after one update()-inclusive planning step (search, the
environment's answer, re-root + reinvigoration: bench.py's C3 step) at the
largest tree count that fits, this

  * times the kernel alone with events on the context stream
    (pomcp_debug_belief_stats_ms: one untimed launch, then `--reps` launches
    between two events) and the whole pomcp_belief_stats call (upload of the
    query states, kernel, download of the counts, synchronisation);
  * reports the belief bytes the kernel reads per ms, as TB/s and as a fraction
    of the 8 TB/s HBM peak, next to the re-root filter's 3.37 TB/s
    (k_log_filter, profiles/r6f_update_kernels_pmc.json: a comparable
    streaming read);
  * obtains the same counts the way they had to be obtained before the kernel
    existed -- pomcp_get_root_belief per tree, then numpy -- on the first
    `--host-trees` trees, checks that they agree, and compares the time per
    tree.  Exit status 1 if the kernel is not faster per tree.

Usage (one GPU process, under its own time limit):

    timeout -k 10 900 python tools/belief_stats_timing.py --out profiles/belief_stats_timing.json
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "posggym-baselines_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_TBS = 8.0
LOG_FILTER_TBS = 3.37   # profiles/r6f_update_kernels_pmc.json, k_log_filter
CFG = dict(discount=0.95, search_time_limit=0.1, c=math.sqrt(2), truncated=False,
           action_selection="ucb", pucb_exploration_fraction=0.25, known_bounds=None,
           step_limit=None, epsilon=0.92, state_belief_only=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--trees", type=int, default=65536)
    ap.add_argument("--sims", type=int, default=65536)
    ap.add_argument("--env", default="PursuitEvasion-v1",
                    choices=["Driving-v1", "PursuitEvasion-v1"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-trees", type=int, default=256)
    ap.add_argument("--max-blocks", type=int, default=512)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="-", help="JSON record path ('-': stdout only)")
    args = ap.parse_args()

    import numpy as np
    import torch
    from posggym_baselines_amd import _native as N
    from posggym_baselines_amd.envs import DrivingModel, PursuitEvasionModel
    from posggym_baselines_amd.planning import BatchedPOMCP, MCTSConfig
    from posggym_baselines_amd.planning.engine import plan_capacities

    dev, B, S = args.device, args.trees, args.sims
    cfg = MCTSConfig(seed=0, num_sims=S, **CFG)
    model = PursuitEvasionModel() if args.env == "PursuitEvasion-v1" else DrivingModel()
    A = model.action_spaces["0"].n
    # the arenas of bench.py's update()-inclusive step; halve the batch until it fits
    n_target = cfg.num_particles + cfg.extra_particles
    caps = plan_capacities(cfg, model.spec.max_episode_steps, S, 1, reroot=True,
                           max_blocks=min(args.max_blocks, S + 64), overflow_slots=1024,
                           num_actions=A)
    caps.max_belief = min(caps.max_belief, max(S, 2 * n_target) + n_target + 64)
    free = torch.cuda.mem_get_info(dev)[0]
    while B > 1024 and caps.bytes_per_tree(A, reroot=True) * B > 0.92 * free:
        B //= 2
    bp = BatchedPOMCP(model, "0", cfg, B, S, capacities=caps, device=dev)
    try:
        bp.init_synthetic(1000)
        acts = bp.search(fetch=True)
        bp.engine.update(acts, bp.engine.synthetic_step(1000, acts))
        eng = bp.engine

        # the parent route on the first trees: one device-to-host copy of every
        # particle per tree, then numpy; the query is the tree's own first particle
        H = min(args.host_trees, B)
        q = np.zeros((B, 2), dtype=np.uint32)
        for b in range(H):
            r = eng.root_belief(b)
            if len(r):
                q[b] = r[0, 1:3]
        t0 = time.perf_counter()
        host = []
        for b in range(H):
            r = eng.root_belief(b)
            host.append((len(r), int(np.sum((r[:, 1] == q[b, 0]) & (r[:, 2] == q[b, 1])))))
        host_ms = (time.perf_counter() - t0) * 1e3

        # the kernel: the whole call, then the kernel alone
        counts = eng.belief_counts(q)
        t0 = time.perf_counter()
        for _ in range(args.reps):
            counts = eng.belief_counts(q)
        call_ms = (time.perf_counter() - t0) * 1e3 / args.reps
        ms = C.c_float()
        N.check(eng._lib.pomcp_debug_belief_stats_ms(
            eng._ctx, q.ctypes.data_as(C.POINTER(C.c_uint32)), args.reps, C.byref(ms)),
            eng._ctx, "belief_stats_ms")
        kernel_ms = float(ms.value)
        same = all(host[b] == (int(counts["belief_size"][b]), int(counts["state_matches"][b]))
                   for b in range(H))
        sizes = counts["belief_size"].astype(np.int64)
        nbytes = int(sizes.sum()) * 16
        tbs = nbytes / (kernel_ms * 1e-3) / 1e12 if kernel_ms > 0 else 0.0
        rec = {
            "env": args.env, "trees": B, "sims": S, "reps": args.reps,
            "device": torch.cuda.get_device_name(dev),
            "belief_particles": int(sizes.sum()), "belief_size_min": int(sizes.min()),
            "belief_size_max": int(sizes.max()), "belief_bytes": nbytes,
            "kernel_ms": kernel_ms, "call_ms": call_ms,
            "kernel_bytes_per_ms": nbytes / kernel_ms if kernel_ms > 0 else 0.0,
            "kernel_TBs": tbs, "fraction_of_8TBs": tbs / HBM_PEAK_TBS,
            "vs_k_log_filter_3.37TBs": tbs / LOG_FILTER_TBS,
            "kernel_us_per_tree": kernel_ms * 1e3 / B, "call_us_per_tree": call_ms * 1e3 / B,
            "host_route_trees": H, "host_route_ms": host_ms,
            "host_route_us_per_tree": host_ms * 1e3 / H,
            "host_route_particles": int(sum(h[0] for h in host)),
            "counts_agree": bool(same),
            "kernel_faster_per_tree": bool(call_ms / B < host_ms / H),
        }
    finally:
        bp.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if rec["counts_agree"] and rec["kernel_faster_per_tree"] else 1


if __name__ == "__main__":
    sys.exit(main())
