"""Time BatchedPOMCP.run_episodes against the host-stepped route it replaces.

Driving-v1, full episodes (until every agent is done, truncated at 50 steps),
one episode per tree on the same env seeds both ways:

  * ``run_episodes``: one pomcp_episodes_step call per step (update from the
    device inputs, search, k_episode_step), one integer back;
  * the only route there was before: ``engine.update`` + ``engine.search`` per
    step with every tree's environment stepped on the host through
    ``DrivingModel.step`` (a ctypes call per tree and step) and the other
    agent's action from ``UniformRandomAgents`` -- the loop lives here, not in
    the package.  A tree whose episode ended is no longer stepped on the host;
    its root is absorbing by then, so the update and the search leave it alone.

Reported: wall time per episode step of each route (a host clock around calls
that end in a stream synchronise; the whole batch is warmed up by one untimed
run first), their ratio, and the device time of k_episode_step + the live count
per step from events on the context stream (pomcp_episodes_timing).  The two
routes' rows (length, return bits) must agree: exit status 1 if they do not.

With ``--belief-acc`` it times the belief accuracy columns instead, on the same
configuration: ``run_episodes(belief_acc=True)`` (k_episode_belief_acc after
every step, nothing per tree on the host between steps) against the route it
replaces, ``run_episodes(belief_states=True, on_step=...)`` whose callback
fetches ``episode_belief_counts()`` (48 B per tree and step, every tree's belief
reduced, parked ones too) and does the tracker's arithmetic in numpy.  Reported:
wall time per step of both routes and of a run with no belief tracking, and the
device time of k_episode_belief_acc per step (pomcp_episodes_belief_acc_ms).
The two routes' ``belief_state_acc`` columns must agree bit for bit.  The record
is stored under the key ``"belief_acc"`` of the ``--out`` file's record, beside
the figures already there.

With ``--population`` it times ``run_episodes`` against no population, against
five fixed distributions and against the five shortest-path agents
(``planning/policies.py``), one warmed-up run each on a fresh engine: wall time
per batch step and the device time of the update, the search and the episode
step kernels.  Stored under the key ``"population"``.

With ``--queue`` it times the episode queue: ``run_episode_queue`` over
``--rounds`` x trees seeds (a finished tree refilled on the device) against the
route there was before, that many successive ``run_episodes`` calls over the
same seeds on one engine, each after one untimed warm-up of its own on a fresh
engine.  Reported for both: wall time, batch steps, episode steps per second,
the share of slot-steps that were live (sum(len) / (trees x batch steps)), the
device time of the update and the search per step, and for the queue that of
the rank + refill kernels and of k_log_drop (pomcp_episodes_queue_timing).  The
two routes assign seeds to planners differently, so their rows differ: rates
are compared, not rows.  Stored under the key ``"queue"`` (``--until
agent_done``: ``"queue_agent_done"``).

With ``--intmcp`` it times ``BatchedINTMCP.run_episodes`` (one
intmcp_episodes_step call per step) against the host-stepped loop it replaces:
``engine.update`` (INTMCP_SKIP for a pair whose episode is over or whose root
is absorbing) + ``engine.search`` per step, with every pair's environment
stepped on the host through ``DrivingModel.step`` -- that loop goes on searching
the pairs whose episode is over.  Same pairs and seeds both ways, a fresh engine
per route sized with ``searches = 50``, one untimed warm-up; the rows (length,
return bits) are compared on every pair.  Defaults: 2,048 pairs, 64 simulations
per level, nesting level 1 (18.8 MiB of arenas per pair, 38 GiB in all).
Reported per step: wall time of both routes and the device time of the update,
the search and k_im_episode_step + the live count (intmcp_episodes_timing).
Stored under the key ``"intmcp"``.

With ``--intmcp-queue`` it times ``BatchedINTMCP.run_episode_queue`` over
``--rounds`` x pairs seeds (a finished pair reset and refilled on the device)
against that many successive ``run_episodes`` calls over the same seeds on one
engine, in both ``until`` modes, each route after one untimed warm-up of its own
on a fresh engine; the setup is ``--intmcp``'s.  Reported per mode and route as
for ``--queue``, and for the queue the device time per step of the rank + list +
refill kernels and of the arena clear (intmcp_episodes_queue_timing), the bytes
the clear stored (intmcp_debug_queue_cleared_bytes) and its store bandwidth
against ``HBM_PEAK_BYTES_PER_S``.  Stored under the key ``"intmcp_queue"``.

With ``--root-parallel`` it times ``run_episodes(root_parallel=K)`` (groups of
K replica trees, one episode per planner: the merge and k_group_episode_step on
the device) against the route it replaces on the same engine size: per step
``engine.update`` with per-tree inputs, ``engine.search``,
``engine.merge_roots(K)`` fetched, and ``DrivingModel.step`` per group on the
host.  Defaults: 64 planners x 64 replicas x 64 simulations per replica (4,096
trees).  A fresh engine per route, one untimed warm-up; the rows (length,
return bits) are compared on every planner.  Reported per step: wall time of
both routes and the device time of the update, the search + merge and
k_group_episode_step + the live count.  Stored under the key
``"root_parallel"``.

With ``--root-parallel-queue`` it times ``run_planner_queue`` (the episode
queue of root-parallel planners: a finished GROUP refilled on the device) over
``--rounds`` x planners seeds against that many successive
``run_episodes(root_parallel=K)`` calls over the same seeds on one engine, in
both ``until`` modes, each route after one untimed warm-up of its own on a
fresh engine; the setup is ``--root-parallel``'s.  Reported per mode and route
as for ``--queue``, and for the queue the device time per step of
k_group_queue_refill + k_group_queue_trees (with k_queue_rank) and of
k_log_drop (pomcp_episodes_queue_timing).  The routes hand the later seeds to
different planners, so only the entries both play first in the same group are
compared (length, return bits): exit status 1 if they differ.  Stored under the
key ``"root_parallel_queue"``.

Usage (one GPU process, under its own time limit):

    timeout -k 10 900 python tools/batched_episodes_timing.py \
        --out profiles/batched_episodes_timing.json
    timeout -k 10 900 python tools/batched_episodes_timing.py --belief-acc \
        --out profiles/batched_episodes_timing.json
    timeout -k 10 300 python tools/batched_episodes_timing.py --queue \
        --out profiles/batched_episodes_timing.json
    timeout -k 10 600 python tools/batched_episodes_timing.py --intmcp \
        --out profiles/batched_episodes_timing.json
    timeout -k 10 600 python tools/batched_episodes_timing.py --intmcp-queue \
        --out profiles/batched_episodes_timing.json
    timeout -k 10 300 python tools/batched_episodes_timing.py --root-parallel \
        --out profiles/batched_episodes_timing.json
    timeout -k 10 300 python tools/batched_episodes_timing.py --root-parallel-queue \
        --out profiles/batched_episodes_timing.json
"""
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


def host_route(bp, seeds, num_sims, max_steps):
    """Lockstep episodes with the environments on the host; returns
    (rows [(len, return)], steps run, seconds)."""
    import numpy as np
    from posggym_baselines_amd.envs import DrivingModel
    from posggym_baselines_amd.planning.episodes import UniformRandomAgents
    B = len(seeds)
    eng = bp.engine
    models, others, states = [], [], []
    keys = np.zeros(B, dtype=np.uint64)
    for b, s in enumerate(seeds):
        m = DrivingModel(seed=s)
        o = UniformRandomAgents(m, s)
        o.reset()
        st = m.sample_initial_state()
        keys[b] = m.obs_key(m.sample_initial_obs(st)["0"])
        models.append(m)
        others.append(o)
        states.append(st)
    t0 = time.perf_counter()
    eng.reset()
    last = np.full(B, -1, dtype=np.int32)
    was_absorbing = np.zeros(B, dtype=bool)
    done = np.zeros(B, dtype=bool)
    lens = np.zeros(B, dtype=np.int64)
    rets = [0.0] * B
    steps = 0
    while not done.all() and steps < max_steps:
        absorbing = eng.update(last, keys)
        actions = eng.search(num_sims)
        for b in np.nonzero(~done)[0]:
            m = models[b]
            # planner.step: an absorbing root returns the last action (mcts.py:97-117)
            a = int(last[b]) if was_absorbing[b] else int(actions[b])
            ts = m.step(states[b], {"0": a, "1": others[b].act("1")})
            states[b] = ts.state
            keys[b] = m.obs_key(ts.observations["0"])
            last[b] = a
            rets[b] += ts.rewards["0"]
            lens[b] += 1
            done[b] = ts.all_done or lens[b] >= max_steps
        was_absorbing = absorbing
        steps += 1
    sec = time.perf_counter() - t0
    return [(int(lens[b]), float(rets[b]).hex()) for b in range(B)], steps, sec


def group_host_route(bp, seeds, K, num_sims, max_steps):
    """The route run_episodes(root_parallel=K) replaces, on the same engine
    size: per step ``engine.update`` with per-tree inputs (a group's action and
    observation repeated for its K replicas), ``engine.search``,
    ``engine.merge_roots(K)`` fetched, and every group's environment stepped on
    the host.  Returns (rows [(len, return)], steps run, seconds)."""
    import numpy as np
    from posggym_baselines_amd.envs import DrivingModel
    from posggym_baselines_amd.planning.episodes import UniformRandomAgents
    G = len(seeds)
    eng = bp.engine
    models, others, states = [], [], []
    keys = np.zeros(G, dtype=np.uint64)
    for g, s in enumerate(seeds):
        m = DrivingModel(seed=s)
        o = UniformRandomAgents(m, s)
        o.reset()
        st = m.sample_initial_state()
        keys[g] = m.obs_key(m.sample_initial_obs(st)["0"])
        models.append(m)
        others.append(o)
        states.append(st)
    t0 = time.perf_counter()
    eng.reset()
    last = np.full(G, -1, dtype=np.int32)
    was_absorbing = np.zeros(G, dtype=bool)
    done = np.zeros(G, dtype=bool)
    lens = np.zeros(G, dtype=np.int64)
    rets = [0.0] * G
    steps = 0
    while not done.all() and steps < max_steps:
        # the planner's root is absorbing only when every replica's is
        absorbing = eng.update(np.repeat(last, K), np.repeat(keys, K)).reshape(G, K).all(axis=1)
        eng.search(num_sims, fetch=False)
        merged = eng.merge_roots(K)
        for g in np.nonzero(~done)[0]:
            m = models[g]
            # POMCP.step / get_action with root_parallel = K (planning/pomcp.py)
            a = int(last[g]) if was_absorbing[g] else 0 if absorbing[g] else int(merged[g].action)
            ts = m.step(states[g], {"0": a, "1": others[g].act("1")})
            states[g] = ts.state
            keys[g] = m.obs_key(ts.observations["0"])
            last[g] = a
            rets[g] += ts.rewards["0"]
            lens[g] += 1
            done[g] = ts.all_done or lens[g] >= max_steps
        was_absorbing = absorbing
        steps += 1
    sec = time.perf_counter() - t0
    return [(int(lens[g]), float(rets[g]).hex()) for g in range(G)], steps, sec


def root_parallel_timing(args):
    """The --root-parallel comparison; returns (record, rows agree)."""
    import torch
    from posggym_baselines_amd.envs import DrivingModel
    from posggym_baselines_amd.planning import BatchedPOMCP, MCTSConfig
    K = args.replicas
    G = args.trees if args.trees is not None else 64
    S = args.sims if args.sims is not None else 64
    model = DrivingModel()
    max_steps = model.spec.max_episode_steps
    seeds = list(range(args.first_seed, args.first_seed + G))

    def fresh():
        return BatchedPOMCP(model, "0", MCTSConfig(seed=0, num_sims=S, **CFG), G * K, S,
                            searches=max_steps, reroot=True, device=args.device)

    bp = fresh()
    try:    # warm-up: every kernel and shape of both routes
        bp.run_episodes(seeds, until="all_done", root_parallel=K)
        bp.engine.merge_roots(K)
    finally:
        bp.close()
    bp = fresh()
    try:
        t0 = time.perf_counter()
        rows = bp.run_episodes(seeds, until="all_done", root_parallel=K)
        dev_sec = time.perf_counter() - t0
        (upd_ms, search_ms, step_ms), dev_steps = bp.engine.episodes_timing()
    finally:
        bp.close()
    bp = fresh()
    try:
        host_rows, host_steps, host_sec = group_host_route(bp, seeds, K, S, max_steps)
    finally:
        bp.close()
    agree = [(r["len"], float(r["return"]).hex()) for r in rows] == host_rows
    dev_ms = dev_sec * 1e3 / dev_steps
    host_ms = host_sec * 1e3 / host_steps
    rec = {
        "env": "Driving-v1", "planners": G, "replicas": K, "trees": G * K,
        "sims_per_replica": S, "until": "all_done",
        "device": torch.cuda.get_device_name(args.device),
        "episode_steps_total": int(sum(r["len"] for r in rows)),
        "run_episodes_steps": dev_steps, "run_episodes_s": dev_sec,
        "run_episodes_ms_per_step": dev_ms,
        "update_ms_per_step": upd_ms / dev_steps,
        "search_and_merge_ms_per_step": search_ms / dev_steps,
        "k_group_episode_step_ms_per_step": step_ms / dev_steps,
        "host_route_steps": host_steps, "host_route_s": host_sec,
        "host_route_ms_per_step": host_ms,
        "host_over_run_episodes": host_ms / dev_ms,
        "rows_agree": bool(agree),
    }
    return rec, agree


def root_parallel_queue_timing(args):
    """The --root-parallel-queue comparison, both until modes; returns (record,
    the first episodes of every group agree)."""
    import torch
    from posggym_baselines_amd.envs import DrivingModel
    from posggym_baselines_amd.planning import BatchedPOMCP, MCTSConfig
    K = args.replicas
    G = args.trees if args.trees is not None else 64
    S = args.sims if args.sims is not None else 64
    model = DrivingModel()
    max_steps = model.spec.max_episode_steps
    seeds = list(range(args.first_seed, args.first_seed + args.rounds * G))

    def route(queue, until):
        bp = BatchedPOMCP(model, "0", MCTSConfig(seed=0, num_sims=S, **CFG), G * K, S,
                          searches=max_steps, reroot=True, device=args.device)
        try:
            t0 = time.perf_counter()
            steps, upd, search, q_ms = 0, 0.0, 0.0, (0.0, 0.0)
            if queue:
                rows = bp.run_planner_queue(seeds, root_parallel=K, until=until)
                (upd, search, _), steps = bp.engine.episodes_timing()
                q_ms = bp.engine.episodes_queue_timing()
            else:
                rows = []
                for i in range(0, len(seeds), G):
                    rows += bp.run_episodes(seeds[i:i + G], until=until, root_parallel=K)
                    (u, s, _), n = bp.engine.episodes_timing()
                    steps, upd, search = steps + n, upd + u, search + s
            sec = time.perf_counter() - t0
        finally:
            bp.close()
        played = int(sum(r["len"] for r in rows))
        rec = {
            "episodes": len(rows), "wall_s": sec, "batch_steps": steps,
            "episode_steps_total": played, "episode_steps_per_s": played / sec,
            "live_share_of_group_steps": played / (G * steps),
            "ms_per_batch_step": sec * 1e3 / steps,
            "update_ms_per_step": upd / steps, "search_and_merge_ms_per_step": search / steps,
        }
        if queue:
            rec.update({"rank_refill_trees_ms_per_step": q_ms[0] / steps,
                        "k_log_drop_ms_per_step": q_ms[1] / steps})
        return rec, rows

    out = {"env": "Driving-v1", "planners": G, "replicas": K, "trees": G * K,
           "sims_per_replica": S, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(args.device)}
    agree = True
    for until in ("all_done", "agent_done"):
        route(True, until)      # untimed warm-up of both routes' kernels and shapes
        route(False, until)
        q_rec, q_rows = route(True, until)
        s_rec, s_rows = route(False, until)
        # entry g < G is group g's first episode on both routes, from fresh engines
        firsts = [i for i, r in enumerate(q_rows) if r["slot_order"] == 0 and r["slot"] == i]
        same = len(firsts) == G and all(
            (q_rows[i]["len"], float(q_rows[i]["return"]).hex()) ==
            (s_rows[i]["len"], float(s_rows[i]["return"]).hex()) for i in firsts)
        agree = agree and same
        rec = {"run_planner_queue": q_rec, "successive_run_episodes": s_rec,
               "queue_over_successive_steps_per_s":
                   q_rec["episode_steps_per_s"] / s_rec["episode_steps_per_s"],
               "first_episodes_compared": len(firsts), "first_episodes_agree": bool(same)}
        out[until] = rec
        print(until, json.dumps(rec), flush=True)
    return out, agree


def belief_acc_timing(fresh, seeds, max_steps):
    """(record, agree) of the --belief-acc comparison."""
    import numpy as np

    def timed(**kw):
        bp = fresh()
        try:
            t0 = time.perf_counter()
            rows = bp.run_episodes(seeds, until="all_done", **kw)
            sec = time.perf_counter() - t0
            _, steps = bp.engine.episodes_timing()
            acc_ms = bp.engine.episodes_belief_acc_ms()
        finally:
            bp.close()
        return rows, sec, steps, acc_ms

    vals = []

    def on_step(t, bp):
        c = bp.episode_belief_counts()
        n = c["belief_size"].astype(np.float64)
        m = c["state_matches"].astype(np.float64)
        vals.append(np.where(n > 0, m / np.maximum(n, 1.0), 0.0))

    timed(belief_acc=True)                              # warm-up of both routes' kernels
    timed(belief_states=True, on_step=on_step)
    vals.clear()
    plain_rows, plain_sec, plain_steps, _ = timed()
    dev_rows, dev_sec, dev_steps, acc_ms = timed(belief_acc=True)
    host_rows, host_sec, host_steps, _ = timed(belief_states=True, on_step=on_step)
    t0 = time.perf_counter()
    # the tracker's per-episode mean: a tree's steps are those before its length
    lens = np.array([r["len"] for r in host_rows])
    sums = np.zeros(len(seeds))
    for t, v in enumerate(vals):
        sums = sums + np.where(t < lens, v, 0.0)
    host_acc = sums / lens
    host_sec += time.perf_counter() - t0
    agree = [float(r["belief_state_acc"]).hex() for r in dev_rows] == \
        [float(x).hex() for x in host_acc]
    agree = agree and [r["len"] for r in dev_rows] == [r["len"] for r in host_rows]
    rec = {
        "steps": dev_steps,
        "plain_ms_per_step": plain_sec * 1e3 / plain_steps,
        "belief_acc_ms_per_step": dev_sec * 1e3 / dev_steps,
        "k_episode_belief_acc_ms_per_step": acc_ms / dev_steps,
        "on_step_route_ms_per_step": host_sec * 1e3 / host_steps,
        "on_step_route_over_belief_acc": (host_sec / host_steps) / (dev_sec / dev_steps),
        "mean_belief_state_acc": float(np.mean(host_acc)),
        "columns_agree": bool(agree),
    }
    return rec, agree


def population_timing(fresh, model, seeds):
    """The --population record: run_episodes against no population, five fixed
    distributions and the five shortest-path agents (planning/policies.py), one
    warmed-up run each on a fresh engine: the batch step and the episode step
    kernels' share of it."""
    from posggym_baselines_amd.planning.policies import (SHORTEST_PATH_POLICY_IDS,
                                                         FixedDistributionPolicy,
                                                         ShortestPathPolicy)
    weights = [[1 + (a + k) % 5 for a in range(5)] for k in range(5)]
    pops = {
        "uniform_agent": None,
        "fixed_five": [FixedDistributionPolicy(model, "1", f"fixed{k}", w)
                       for k, w in enumerate(weights)],
        "shortest_path_five": [ShortestPathPolicy.from_id(model, "1", pid)
                               for pid in SHORTEST_PATH_POLICY_IDS],
    }
    out = {}
    for name, pop in pops.items():
        for timed in (False, True):        # (False: the untimed warm-up)
            bp = fresh()
            try:
                t0 = time.perf_counter()
                rows = bp.run_episodes(seeds, until="all_done", other_agents=pop)
                sec = time.perf_counter() - t0
                (upd_ms, search_ms, step_ms), steps = bp.engine.episodes_timing()
            finally:
                bp.close()
        out[name] = {
            "steps": steps, "episode_steps_total": int(sum(r["len"] for r in rows)),
            "run_episodes_ms_per_step": sec * 1e3 / steps,
            "update_ms_per_step": upd_ms / steps, "search_ms_per_step": search_ms / steps,
            "k_episode_step_ms_per_step": step_ms / steps,
            "mean_return": sum(r["return"] for r in rows) / len(rows),
        }
        print(name, json.dumps(out[name]), flush=True)
    return out


def queue_timing(fresh, seeds, B, until):
    """The --queue comparison: N = len(seeds) episodes through run_episode_queue
    and through N / B successive run_episodes calls on one engine."""
    def route(queue):
        bp = fresh()
        try:
            t0 = time.perf_counter()
            steps, upd, search, q_ms = 0, 0.0, 0.0, (0.0, 0.0)
            if queue:
                rows = bp.run_episode_queue(seeds, until=until)
                (upd, search, _), steps = bp.engine.episodes_timing()
                q_ms = bp.engine.episodes_queue_timing()
            else:
                rows = []
                for i in range(0, len(seeds), B):
                    rows += bp.run_episodes(seeds[i:i + B], until=until)
                    (u, s, _), n = bp.engine.episodes_timing()
                    steps, upd, search = steps + n, upd + u, search + s
            sec = time.perf_counter() - t0
        finally:
            bp.close()
        played = int(sum(r["len"] for r in rows))
        return {
            "episodes": len(rows), "wall_s": sec, "batch_steps": steps,
            "episode_steps_total": played, "episode_steps_per_s": played / sec,
            "live_share_of_slot_steps": played / (B * steps),
            "ms_per_batch_step": sec * 1e3 / steps,
            "update_ms_per_step": upd / steps, "search_ms_per_step": search / steps,
            "refill_ms_per_step": q_ms[0] / steps, "k_log_drop_ms_per_step": q_ms[1] / steps,
        }

    route(True)     # untimed warm-up of both routes' kernels and shapes
    route(False)
    rec = {"run_episode_queue": route(True), "successive_run_episodes": route(False)}
    rec["queue_over_successive_steps_per_s"] = (
        rec["run_episode_queue"]["episode_steps_per_s"] /
        rec["successive_run_episodes"]["episode_steps_per_s"])
    return rec


def intmcp_host_route(bp, seeds, num_sims, max_steps):
    """The host-stepped I-NTMCP loop run_episodes replaces; returns
    (rows [(len, return)], steps run, seconds)."""
    import numpy as np
    from posggym_baselines_amd import _native as N
    from posggym_baselines_amd.envs import DrivingModel
    from posggym_baselines_amd.planning.episodes import UniformRandomAgents
    B = len(seeds)
    eng = bp.engine
    models, others, states = [], [], []
    keys = np.zeros(B, dtype=np.uint64)
    for b, s in enumerate(seeds):
        m = DrivingModel(seed=s)
        o = UniformRandomAgents(m, s)
        o.reset()
        st = m.sample_initial_state()
        keys[b] = m.obs_key(m.sample_initial_obs(st)["0"])
        models.append(m)
        others.append(o)
        states.append(st)
    t0 = time.perf_counter()
    eng.reset()
    last = np.full(B, -1, dtype=np.int32)
    absorbing = np.zeros(B, dtype=bool)
    done = np.zeros(B, dtype=bool)
    lens = np.zeros(B, dtype=np.int64)
    rets = [0.0] * B
    steps = 0
    while not done.all() and steps < max_steps:
        acts_in = np.where(done | absorbing, N.INTMCP_SKIP, last).astype(np.int32)
        was_absorbing = absorbing
        absorbing = eng.update(acts_in, keys)
        actions = eng.search(num_sims)
        for b in np.nonzero(~done)[0]:
            m = models[b]
            # planner.step: an absorbing root returns the last action (intmcp.py:114-136)
            a = int(last[b]) if was_absorbing[b] else int(actions[b])
            ts = m.step(states[b], {"0": a, "1": others[b].act("1")})
            states[b] = ts.state
            keys[b] = m.obs_key(ts.observations["0"])
            last[b] = a
            rets[b] += ts.rewards["0"]
            lens[b] += 1
            done[b] = ts.all_done or lens[b] >= max_steps
        steps += 1
    sec = time.perf_counter() - t0
    return [(int(lens[b]), float(rets[b]).hex()) for b in range(B)], steps, sec


def intmcp_timing(args):
    """The --intmcp comparison; returns (record, rows agree)."""
    import torch
    from posggym_baselines_amd.envs import DrivingModel
    from posggym_baselines_amd.planning import BatchedINTMCP, MCTSConfig
    B = args.trees if args.trees is not None else 2048
    S = args.sims if args.sims is not None else 64
    model = DrivingModel()
    max_steps = model.spec.max_episode_steps
    seeds = list(range(args.first_seed, args.first_seed + B))
    cfg = MCTSConfig(seed=0, num_sims=S, **dict(CFG, state_belief_only=False))

    def fresh():
        return BatchedINTMCP(model, "0", cfg, B, S, searches=max_steps, device=args.device,
                             nesting_level=1)

    bp = fresh()
    caps = bp.engine.capacities
    try:
        bp.run_episodes(seeds, until="all_done")   # warm-up: every kernel and shape of both routes
    finally:
        bp.close()
    bp = fresh()
    try:
        t0 = time.perf_counter()
        rows = bp.run_episodes(seeds, until="all_done")
        dev_sec = time.perf_counter() - t0
        (upd_ms, search_ms, step_ms), dev_steps = bp.engine.episodes_timing()
    finally:
        bp.close()
    bp = fresh()
    try:
        host_rows, host_steps, host_sec = intmcp_host_route(bp, seeds, S, max_steps)
    finally:
        bp.close()
    agree = [(r["len"], float(r["return"]).hex()) for r in rows] == host_rows
    dev_ms = dev_sec * 1e3 / dev_steps
    host_ms = host_sec * 1e3 / host_steps
    rec = {
        "env": "Driving-v1", "pairs": B, "sims_per_level": S, "nesting_level": 1,
        "until": "all_done", "searches": max_steps,
        "arena_bytes_per_pair": caps.bytes_per_pair(model.action_spaces["0"].n),
        "device": torch.cuda.get_device_name(args.device),
        "episode_steps_total": int(sum(r["len"] for r in rows)),
        "run_episodes_steps": dev_steps, "run_episodes_s": dev_sec,
        "run_episodes_ms_per_step": dev_ms,
        "update_ms_per_step": upd_ms / dev_steps, "search_ms_per_step": search_ms / dev_steps,
        "k_im_episode_step_ms_per_step": step_ms / dev_steps,
        "host_route_steps": host_steps, "host_route_s": host_sec,
        "host_route_ms_per_step": host_ms,
        "host_over_run_episodes": host_ms / dev_ms,
        "rows_agree": bool(agree),
    }
    return rec, agree


HBM_PEAK_BYTES_PER_S = 8e12   # MI355X


def intmcp_queue_timing(args):
    """The --intmcp-queue comparison, both until modes."""
    import torch
    from posggym_baselines_amd.envs import DrivingModel
    from posggym_baselines_amd.planning import BatchedINTMCP, MCTSConfig
    B = args.trees if args.trees is not None else 2048
    S = args.sims if args.sims is not None else 64
    model = DrivingModel()
    max_steps = model.spec.max_episode_steps
    seeds = list(range(args.first_seed, args.first_seed + args.rounds * B))
    cfg = MCTSConfig(seed=0, num_sims=S, **dict(CFG, state_belief_only=False))
    caps = {}

    def route(queue, until):
        bp = BatchedINTMCP(model, "0", cfg, B, S, searches=max_steps, device=args.device,
                           nesting_level=1)
        caps["bytes"] = bp.engine.capacities.bytes_per_pair(model.action_spaces["0"].n)
        try:
            t0 = time.perf_counter()
            steps, upd, search, q_ms, cleared = 0, 0.0, 0.0, (0.0, 0.0), 0
            if queue:
                rows = bp.run_episode_queue(seeds, until=until)
                (upd, search, _), steps = bp.engine.episodes_timing()
                q_ms = bp.engine.episodes_queue_timing()
                cleared = bp.engine.debug_queue_cleared_bytes()
            else:
                rows = []
                for i in range(0, len(seeds), B):
                    rows += bp.run_episodes(seeds[i:i + B], until=until)
                    (u, s, _), n = bp.engine.episodes_timing()
                    steps, upd, search = steps + n, upd + u, search + s
            sec = time.perf_counter() - t0
        finally:
            bp.close()
        played = int(sum(r["len"] for r in rows))
        rec = {
            "episodes": len(rows), "wall_s": sec, "batch_steps": steps,
            "episode_steps_total": played, "episode_steps_per_s": played / sec,
            "live_share_of_slot_steps": played / (B * steps),
            "ms_per_batch_step": sec * 1e3 / steps,
            "update_ms_per_step": upd / steps, "search_ms_per_step": search / steps,
        }
        if queue:
            rec.update({
                "rank_list_refill_ms_per_step": q_ms[0] / steps,
                "clear_ms_per_step": q_ms[1] / steps, "clear_ms_total": q_ms[1],
                "clear_bytes_stored": cleared,
                "clear_bytes_per_s": cleared / (q_ms[1] * 1e-3) if q_ms[1] > 0 else 0.0,
                "clear_share_of_hbm_peak":
                    cleared / (q_ms[1] * 1e-3) / HBM_PEAK_BYTES_PER_S if q_ms[1] > 0 else 0.0,
            })
        return rec

    out = {"env": "Driving-v1", "pairs": B, "sims_per_level": S, "nesting_level": 1,
           "searches": max_steps, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(args.device)}
    for until in ("all_done", "agent_done"):
        route(True, until)      # untimed warm-up of both routes' kernels and shapes
        route(False, until)
        rec = {"run_episode_queue": route(True, until),
               "successive_run_episodes": route(False, until)}
        rec["queue_over_successive_steps_per_s"] = (
            rec["run_episode_queue"]["episode_steps_per_s"] /
            rec["successive_run_episodes"]["episode_steps_per_s"])
        out[until] = rec
        print(until, json.dumps(rec), flush=True)
    out["arena_bytes_per_pair"] = caps["bytes"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--intmcp-queue", action="store_true",
                    help="time BatchedINTMCP.run_episode_queue over --rounds x pairs seeds against "
                         "that many successive run_episodes calls, both until modes")
    ap.add_argument("--queue", action="store_true",
                    help="time run_episode_queue over --rounds x trees seeds against that many "
                         "successive run_episodes calls")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--until", default="all_done", choices=["all_done", "agent_done"],
                    help="--queue only; agent_done is stored under the key queue_agent_done")
    ap.add_argument("--intmcp", action="store_true",
                    help="time BatchedINTMCP.run_episodes against the host-stepped loop "
                         "(defaults: 2048 pairs, 64 simulations per level)")
    ap.add_argument("--trees", type=int, default=None, help="default 4096 (--intmcp: 2048 pairs)")
    ap.add_argument("--sims", type=int, default=None, help="default 256 (--intmcp: 64 per level)")
    ap.add_argument("--first-seed", type=int, default=3000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="-", help="JSON record path ('-': stdout only)")
    ap.add_argument("--belief-acc", action="store_true",
                    help="time run_episodes(belief_acc=True) against the on_step route")
    ap.add_argument("--population", action="store_true",
                    help="time run_episodes against no population, five fixed distributions and "
                         "the five shortest-path agents")
    ap.add_argument("--root-parallel", action="store_true",
                    help="time run_episodes(root_parallel=--replicas) against update + search + "
                         "merge_roots + a host step per group (defaults: 64 planners, 64 "
                         "simulations per replica; --trees counts planners)")
    ap.add_argument("--replicas", type=int, default=64,
                    help="--root-parallel, --root-parallel-queue: replicas per planner")
    ap.add_argument("--root-parallel-queue", action="store_true",
                    help="time run_planner_queue over --rounds x planners seeds against that many "
                         "successive run_episodes(root_parallel=--replicas) calls, both until "
                         "modes (the --root-parallel setup)")
    args = ap.parse_args()

    import torch
    from posggym_baselines_amd.envs import DrivingModel
    from posggym_baselines_amd.planning import BatchedPOMCP, MCTSConfig

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    if args.root_parallel_queue:
        q_rec, agree = root_parallel_queue_timing(args)
        rec = {}
        if args.out != "-" and os.path.exists(args.out):
            with open(args.out) as f:
                rec = json.loads(f.read())
        rec["root_parallel_queue"] = q_rec
        print(json.dumps(q_rec), flush=True)
        if args.out != "-":
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(rec) + "\n")
        return 0 if agree else 1
    if args.root_parallel:
        rp_rec, agree = root_parallel_timing(args)
        rec = {}
        if args.out != "-" and os.path.exists(args.out):
            with open(args.out) as f:
                rec = json.loads(f.read())
        rec["root_parallel"] = rp_rec
        print(json.dumps(rp_rec), flush=True)
        if args.out != "-":
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(rec) + "\n")
        return 0 if agree else 1
    if args.intmcp_queue:
        q_rec = intmcp_queue_timing(args)
        rec = {}
        if args.out != "-" and os.path.exists(args.out):
            with open(args.out) as f:
                rec = json.loads(f.read())
        rec["intmcp_queue"] = q_rec
        print(json.dumps(q_rec), flush=True)
        if args.out != "-":
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(rec) + "\n")
        return 0
    if args.intmcp:
        im_rec, agree = intmcp_timing(args)
        rec = {}
        if args.out != "-" and os.path.exists(args.out):
            with open(args.out) as f:
                rec = json.loads(f.read())
        rec["intmcp"] = im_rec
        print(json.dumps(im_rec), flush=True)
        if args.out != "-":
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(rec) + "\n")
        return 0 if agree else 1
    B, S, dev = args.trees or 4096, args.sims or 256, args.device
    model = DrivingModel()
    max_steps = model.spec.max_episode_steps
    seeds = list(range(args.first_seed, args.first_seed + B))

    def fresh():
        # a new engine per run: the planners' RNG streams continue from episode to
        # episode on one engine (MCTS.reset does not reseed), and the two routes
        # must play the same episodes to be compared row by row
        return BatchedPOMCP(model, "0", MCTSConfig(seed=0, num_sims=S, **CFG), B, S,
                            searches=max_steps, reroot=True, device=dev)

    if args.queue:
        all_seeds = list(range(args.first_seed, args.first_seed + args.rounds * B))
        q_rec = dict({"env": "Driving-v1", "trees": B, "sims": S, "until": args.until,
                      "device": torch.cuda.get_device_name(dev)},
                     **queue_timing(fresh, all_seeds, B, args.until))
        rec = {}
        if args.out != "-" and os.path.exists(args.out):
            with open(args.out) as f:
                rec = json.loads(f.read())
        rec["queue" if args.until == "all_done" else "queue_" + args.until] = q_rec
        print(json.dumps(q_rec), flush=True)
        if args.out != "-":
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(rec) + "\n")
        return 0

    if args.population:
        pop_rec = dict({"trees": B, "sims": S, "device": torch.cuda.get_device_name(dev)},
                       **population_timing(fresh, model, seeds))
        rec = {}
        if args.out != "-" and os.path.exists(args.out):
            with open(args.out) as f:
                rec = json.loads(f.read())
        rec["population"] = pop_rec
        if args.out != "-":
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(rec) + "\n")
        return 0

    if args.belief_acc:
        acc_rec, agree = belief_acc_timing(fresh, seeds, max_steps)
        acc_rec = dict({"trees": B, "sims": S, "device": torch.cuda.get_device_name(dev)},
                       **acc_rec)
        rec = {}
        if args.out != "-" and os.path.exists(args.out):
            with open(args.out) as f:
                rec = json.loads(f.read())
        rec["belief_acc"] = acc_rec
        print(json.dumps(acc_rec), flush=True)
        if args.out != "-":
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(rec) + "\n")
        return 0 if agree else 1

    bp = fresh()
    try:
        bp.run_episodes(seeds, until="all_done")   # warm-up: every kernel and shape of both routes
    finally:
        bp.close()
    bp = fresh()
    try:
        t0 = time.perf_counter()
        rows = bp.run_episodes(seeds, until="all_done")
        dev_sec = time.perf_counter() - t0
        (upd_ms, search_ms, step_ms), dev_steps = bp.engine.episodes_timing()
    finally:
        bp.close()
    bp = fresh()
    try:
        host_rows, host_steps, host_sec = host_route(bp, seeds, S, max_steps)
    finally:
        bp.close()
    agree = [(r["len"], float(r["return"]).hex()) for r in rows] == host_rows
    dev_ms = dev_sec * 1e3 / dev_steps
    host_ms = host_sec * 1e3 / host_steps
    rec = {
        "env": "Driving-v1", "trees": B, "sims": S, "until": "all_done",
        "device": torch.cuda.get_device_name(dev),
        "episode_steps_total": int(sum(r["len"] for r in rows)),
        "run_episodes_steps": dev_steps, "run_episodes_s": dev_sec,
        "run_episodes_ms_per_step": dev_ms,
        "update_ms_per_step": upd_ms / dev_steps, "search_ms_per_step": search_ms / dev_steps,
        "k_episode_step_ms_per_step": step_ms / dev_steps,
        "host_route_steps": host_steps, "host_route_s": host_sec,
        "host_route_ms_per_step": host_ms,
        "host_over_run_episodes": host_ms / dev_ms,
        "rows_agree": bool(agree),
    }
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if agree else 1


if __name__ == "__main__":
    sys.exit(main())
