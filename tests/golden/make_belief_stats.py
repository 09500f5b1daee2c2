"""Generate tests/golden/belief_stats/belief_stats.json (container-only).

Belief accuracies of the REAL reference ``BeliefStatTracker``
(``posggym_baselines/planning/utils.py:147-339``) on episodes that are already
committed goldens: each case re-runs the first episode of its golden with the
real reference planner (oracle/ref_harness.py: stub-imported, injected RNG,
fake clock; same config, num_sims, planner seed and env seed), asserts that the
step records and the trace equal the committed golden's -- so the beliefs
counted here are the ones the existing GPU parity tests already pin -- and
attaches the reference tracker through a ``SimpleNamespace`` env with
``state``, ``last_obs``, ``last_actions``, ``policies`` and ``spec``.

The episode loop is this script's own: ``oracle.episode.run_episode``'s order
of draws, keeping the true state.  Per step it records the state the tracker
compares with (the one before the most recent action) as ``model.pack_words``
words, the other agent's action, the belief size and the reference's
``get_state_accuracy`` / ``get_other_policy_accuracy`` /
``get_other_action_accuracy`` as ``float.hex()``; per episode ``get_episode()``.
The harness's true other agent is uniform random, so the "true policy id" is a
label: the first key of the case's mixture (stored in the fixture).

Each case asserts a condition that keeps the GPU test from comparing 0.0 with
0.0 everywhere (CASES below).

(The file sits in a directory of its own: make_golden.py's regeneration test
owns the *.json files directly under tests/golden/.)

Usage:  python tests/golden/make_belief_stats.py [out.json]
"""
import json
import math
import os
import sys
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

OUT = os.path.join(HERE, "belief_stats", "belief_stats.json")


def _between(v):
    return 0.0 < v < 1.0


# golden case -> (tracked stats, condition on the per-step (state, policy, action) values)
CASES = {
    "c1_ucb": (["state"], lambda s, p, a: sum(map(_between, s)) >= 1),
    "mcts_fixed_other_pucb": (["state"], lambda s, p, a: sum(map(_between, s)) >= 1),
    "mcts_ipomcp_mix_pucb": (["state", "policy", "action"],
                             lambda s, p, a: sum(_between(x) and _between(y)
                                                 for x, y in zip(p, a)) >= 5),
    "mcts_pe_mix_pucb": (["state", "policy", "action"],
                         lambda s, p, a: sum(map(_between, s)) >= 1 and
                         sum(x == 1.0 for x in p) >= 1),
    # POTMMCP (meta-policy over ego policies, mixture over three other-agent policies)
    "potmmcp_ucb_ego1": (["state", "policy", "action"],
                         lambda s, p, a: sum(_between(x) and _between(y)
                                             for x, y in zip(p, a)) >= 5),
}


def _enc(v):
    v = float(v)
    return "nan" if math.isnan(v) else v.hex()


def run_case(name):
    from oracle.envs import make_model
    from oracle.episode import ENV_TREE_BASE, fhex
    from oracle.ref_harness import (import_reference, make_reference_mcts, make_reference_pomcp,
                                    make_reference_potmmcp, reference_mcts_record,
                                    reference_potmmcp_record, reference_record)
    from oracle.rng import S_ENV_POLICY_BASE, Streams
    with open(os.path.join(HERE, f"{name}.json")) as f:
        data = json.load(f)
    stats, condition = CASES[name]
    ep = data["episodes"][0]
    cfg, env_seed, num_sims = ep["config"], ep["env_seed"], data["num_sims"]
    ego, env_id = data["ego"], data.get("env", "Driving-v1")
    max_steps = data.get("max_steps", 100 if env_id == "PursuitEvasion-v1" else 50)
    spec = data.get("spec")

    import_reference()
    from posggym_baselines.planning.utils import BeliefStatTracker
    streams = Streams(cfg.get("seed") or 0, 0)
    model = make_model(env_id, streams)
    if spec is None:
        planner = make_reference_pomcp(model, ego, cfg, num_sims, streams, "POMCP")
        record = reference_record
    elif "meta" in spec:
        planner = make_reference_potmmcp(model, ego, cfg, num_sims, streams, spec)
        record = reference_potmmcp_record
    else:
        planner = make_reference_mcts(model, ego, cfg, num_sims, streams, spec, data["planner"])

        def record(pl, searched, a):
            return reference_mcts_record(pl, searched, a, spec)
    other = [i for i in model.possible_agents if i != ego][0]
    label = None
    if spec is not None and "meta" in spec:
        label = list(spec["other"])[0]
    elif spec is not None and spec["other"]["kind"] == "mixture":
        label = list(spec["other"]["policies"])[0]

    # oracle.episode.run_episode's loop and order of draws, keeping the state
    env_streams = Streams(env_seed, ENV_TREE_BASE)
    env = make_model(env_id, env_streams)
    state = env.sample_initial_state()
    obs = env.sample_initial_obs(state)
    view = SimpleNamespace(state=state, last_obs={other: obs[other]}, last_actions={other: None},
                           policies={other: SimpleNamespace(policy_id=label)},
                           spec=SimpleNamespace(max_episode_steps=max_steps))
    planner.reset()
    tracker = BeliefStatTracker(planner, view, track_per_step=False, stats_to_track=stats)
    trace = {"env_seed": env_seed, "steps": []}
    records, steps, ret = [], [], 0.0
    for t in range(max_steps):
        searched = not planner.root.is_absorbing
        a_ego = planner.step(obs[ego])
        records.append(record(planner, searched, a_ego))
        actions = {}
        for i in env.possible_agents:
            actions[i] = a_ego if i == ego else env_streams.randint(S_ENV_POLICY_BASE + int(i),
                                                                    env.action_spaces[i].n)
        ts = env.step(state, actions)
        ret += ts.rewards[ego]
        trace["steps"].append({"obs": env.pack_obs(obs[ego]),
                               "actions": [actions[i] for i in env.possible_agents],
                               "reward": fhex(ts.rewards[ego])})
        before = state
        state, obs = ts.state, ts.observations
        view.state, view.last_obs = state, {other: obs[other]}
        view.last_actions = {other: actions[other]}
        assert tracker._current_state == before
        n = planner.root.belief.size()
        vals = {"state": 0.0, "policy": 0.0, "action": 0.0}
        if n > 0:   # (utils.py:227-228)
            vals["state"] = tracker.get_state_accuracy(before)
            vals["policy"] = tracker.get_other_policy_accuracy(view.policies)
            vals["action"] = tracker.get_other_action_accuracy(view.last_actions)
        tracker.step(view)
        for k in stats:
            assert tracker._current_stats[k][-1] == vals[k], (name, t, k)
        steps.append({"state": [int(w) for w in model.pack_words(before)],
                      "other_action": int(actions[other]), "belief_size": int(n),
                      "state_acc": _enc(vals["state"]), "policy_acc": _enc(vals["policy"]),
                      "action_acc": _enc(vals["action"])})
        if ts.all_done:
            break
    trace["return"] = fhex(ret)
    trace["len"] = len(trace["steps"])
    episode = {k: _enc(v) for k, v in tracker.get_episode().items()}
    planner.close()
    if records != ep["records"] or trace != ep["trace"]:
        raise SystemExit(f"{name}: the episode differs from the committed golden")
    dec = [[float.fromhex(s[f"{k}_acc"]) for s in steps] for k in ("state", "policy", "action")]
    if not condition(*dec):
        raise SystemExit(f"{name}: the case's condition fails: take another seed pair")
    return {"case": name, "episode": 0, "env": env_id, "ego": ego, "planner_seed": cfg.get("seed"),
            "env_seed": env_seed, "stats": stats, "policy_label": label, "steps": steps,
            "get_episode": episode}


def main(out=OUT):
    from oracle.ref_harness import reference_available
    if not reference_available():
        raise SystemExit("reference not available (container-only script)")
    data = {"cases": [run_case(name) for name in CASES]}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(data, f, separators=(",", ":"))
    for c in data["cases"]:
        print(c["case"], len(c["steps"]), "steps", c["get_episode"])


if __name__ == "__main__":
    main(*sys.argv[1:2])
