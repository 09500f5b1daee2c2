"""Reference goldens of PredatorPrey-v0 (tests/golden/predator_prey/*.json):

    python tests/golden/make_predator_prey.py [--out=DIR] [case ...]

The real reference planners (``oracle.ref_harness.make_reference_pomcp`` /
``make_reference_mcts`` / ``make_reference_potmmcp``, used as they are) run on
the build's Python restatement of the environment
(``tests/golden/predator_prey_model.py``); the episode loop is
``predator_prey_model.run_episode``, as the harness's own is tied to the two
environments of ``oracle.envs``.  The other predator is uniform random.

Records are ``reference_record`` / ``reference_mcts_record`` /
``reference_potmmcp_record``'s.  Episodes are cut at ``MAX_STEPS`` so that no
file is larger than the largest under ``tests/golden/coop_reaching/``.

Every case asserts what it is there for (``CHECKS``), and across the cases some
step catches a prey, some episode ends with every prey caught before
``MAX_STEPS``, some runs to ``MAX_STEPS``, each of the three rules decided some
prey's move and both values of the order bit blocked a predator (the
environment models' ``facts``); the generator aborts otherwise.
"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "posggym-baselines_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT_DIR = os.path.join(HERE, "predator_prey")

ENV = "PredatorPrey-v0"
TEST_CFG = dict(discount=0.95, search_time_limit=0.1, c=math.sqrt(2), truncated=False,
                action_selection="ucb", pucb_exploration_fraction=0.25, known_bounds=None,
                step_limit=None, epsilon=0.92, seed=0, state_belief_only=True)
FIXED = [0.3, 0.1, 0.1, 0.4, 0.1]
MIX3 = {"kind": "mixture", "policies": {"o_u": [0.2] * 5, "o_left": [0.1, 0.1, 0.1, 0.6, 0.1],
                                        "o_fixed": FIXED}}
MAX_STEPS = 12
TREES = 6
REF = dict(grid="10x10", num_prey=3, prey_strength=2, obs_dim=2)      # env_kwargs.yaml
SMALL = dict(grid="5x5", num_prey=1, prey_strength=1, obs_dim=1)

# name: planner, cfg overrides, spec, num_sims, [(planner seed, env seed)], ego, env kwargs
# (seeds: chosen so that the cases meet the assertions of CHECKS and main)
CASES = {
    # (seeds whose searches find prey: most records hold non-zero values)
    "pomcp_ucb": dict(planner="POMCP", over={}, spec=None, num_sims=128,
                      pairs=[(47, 47), (21, 21)], ego="0", kwargs=REF),
    "pomcp_pucb_ego1": dict(planner="POMCP", over={"action_selection": "pucb"}, spec=None,
                            num_sims=96, pairs=[(3, 3), (4, 4)], ego="1", kwargs=SMALL),
    # rollouts to the step limit and a tree deeper than one Philox block of model
    # words: on the 10x10 grid with obs_dim 1 the predator sees nothing but
    # walls for many steps, so an action has one observation child and with a
    # small c the search follows one line of play
    "pomcp_deep": dict(planner="POMCP", over={"discount": 0.99, "epsilon": 0.01, "c": 0.05},
                       spec=None, num_sims=64, pairs=[(5, 5), (6, 6)], ego="0",
                       kwargs=dict(grid="10x10", num_prey=1, prey_strength=1, obs_dim=1)),
    # depth limits 1 and 3: the DL = 1 and DL = 3 specialisations of k_search
    # (epsilon 0.96 and 0.87 at discount 0.95; every other case but the deep one has 2)
    "pomcp_dl1": dict(planner="POMCP", over={"epsilon": 0.96}, spec=None, num_sims=64,
                      pairs=[(13, 13), (14, 14)], ego="0",
                      kwargs=dict(grid="5x5", num_prey=2, prey_strength=1, obs_dim=2)),
    "pomcp_dl3": dict(planner="POMCP", over={"epsilon": 0.87, "action_selection": "pucb"},
                      spec=None, num_sims=64, pairs=[(15, 15), (16, 16)], ego="1",
                      kwargs=dict(grid="5x5", num_prey=3, prey_strength=2, obs_dim=1)),
    # ~107 particles: every re-root reinvigorates
    "ipomcp_reinv": dict(planner="IPOMCP", over={"action_selection": "pucb",
                                                 "state_belief_only": False,
                                                 "search_time_limit": 1.0},
                         spec={"search": None, "other": MIX3}, num_sims=48,
                         pairs=[(7, 7), (8, 8)], ego="0",
                         kwargs=dict(grid="5x5", num_prey=2, prey_strength=1, obs_dim=1)),
    "potmmcp_ucb": dict(
        planner="POTMMCP", over={"state_belief_only": False},
        spec={"ego": {"u": [0.2] * 5, "left": [0.1, 0.1, 0.1, 0.6, 0.1],
                      "down": [0.1, 0.1, 0.6, 0.1, 0.1]},
              "other": {"o_u": [0.2] * 5, "o_left": [0.1, 0.1, 0.1, 0.6, 0.1], "o_fixed": FIXED},
              "meta": {"o_u": {"u": 0.5, "left": 0.5}, "o_left": {"down": 1.0},
                       "o_fixed": {"u": 0.2, "left": 0.4, "down": 0.4}}},
        num_sims=64, pairs=[(9, 9), (10, 10)], ego="1",
        kwargs=dict(grid="5x5", num_prey=2, prey_strength=2, obs_dim=2)),
    # the one non-mixture type path: a stateless fixed other agent
    "mcts_fixed_other": dict(planner="MCTS", over={},
                             spec={"search": None, "other": {"kind": "fixed", "probs": FIXED}},
                             num_sims=96, pairs=[(11, 11), (12, 12)], ego="0",
                             kwargs=dict(grid="5x5", num_prey=3, prey_strength=1, obs_dim=2)),
}


def run_episode_case(case, cfg, env_seed, facts, tree=0, max_steps=MAX_STEPS):
    from predator_prey_model import PredatorPreyModel, run_episode
    from oracle.episode import ENV_TREE_BASE
    from oracle.ref_harness import (make_reference_mcts, make_reference_pomcp,
                                    make_reference_potmmcp, reference_mcts_record,
                                    reference_potmmcp_record, reference_record)
    from oracle.rng import Streams
    cls, spec, ego, num_sims = case["planner"], case["spec"], case["ego"], case["num_sims"]
    assert num_sims <= 128
    streams = Streams(cfg["seed"], tree)
    model = PredatorPreyModel(streams, **case["kwargs"])
    if cls == "POMCP":
        planner = make_reference_pomcp(model, ego, cfg, num_sims, streams, "POMCP")
    elif cls == "POTMMCP":
        planner = make_reference_potmmcp(model, ego, cfg, num_sims, streams, spec)
    else:
        planner = make_reference_mcts(model, ego, cfg, num_sims, streams, spec, cls)
    planner.reset()
    records = []

    def step(obs):
        searched = not planner.root.is_absorbing
        a = planner.step(obs)
        if cls == "POMCP":
            records.append(reference_record(planner, searched, a))
        elif cls == "POTMMCP":
            records.append(reference_potmmcp_record(planner, searched, a))
        else:
            records.append(reference_mcts_record(planner, searched, a, spec))
        if searched:
            facts["max_depth"] = max(facts["max_depth"],
                                     int(planner.step_statistics["search_depth"]))
            facts["depth_limit"] = int(planner.config.depth_limit)
            facts["min_particles"] = min(facts["min_particles"],
                                         len(planner.root.belief.particles))
        return a

    env = PredatorPreyModel(Streams(env_seed, ENV_TREE_BASE), **case["kwargs"])
    trace = run_episode(env, step, ego, max_steps)
    trace["env_seed"] = env_seed
    planner.close()
    for k in range(3):
        facts["rules"][k] += env.facts["rules"][k]
    for k in range(2):
        facts["blocked_order"][k] += env.facts["blocked_order"][k]
    facts["captures"] += env.facts["captures"]
    return trace, records


# what each case is there for (the deep case: a simulation that goes deeper than
# four steps draws more than the four model words of its Philox block)
CHECKS = {
    "pomcp_deep": lambda f: f["depth_limit"] + 1 > 4 and f["max_depth"] >= 6,
    "pomcp_dl1": lambda f: f["depth_limit"] == 1,
    "pomcp_dl3": lambda f: f["depth_limit"] == 3,
    "ipomcp_reinv": lambda f: f["min_particles"] < 128,
}


def new_facts():
    return {"max_depth": 0, "depth_limit": 0, "min_particles": 1 << 30, "rules": [0, 0, 0],
            "blocked_order": [0, 0], "captures": 0}


def run_case(name):
    case = CASES[name]
    out = {"case": name, "planner": case["planner"], "env": ENV, "kwargs": case["kwargs"],
           "num_sims": case["num_sims"], "ego": case["ego"], "max_steps": MAX_STEPS,
           "spec": case["spec"], "episodes": []}
    facts = new_facts()
    for seed, env_seed in case["pairs"]:
        cfg = dict(TEST_CFG, **case["over"])
        cfg["seed"] = seed
        tr, rr = run_episode_case(case, cfg, env_seed, facts)
        out["episodes"].append({"config": dict(cfg), "env_seed": env_seed, "trace": tr,
                                "records": rr})
    if case["planner"] == "POTMMCP":
        # the first step of trees 0 .. 5 (keys (seed, k)) of the first episode
        seed, env_seed = case["pairs"][0]
        cfg = dict(TEST_CFG, **case["over"])
        cfg["seed"] = seed
        out["trees"] = []
        for k in range(TREES):
            tr, rr = run_episode_case(case, cfg, env_seed, new_facts(), tree=k, max_steps=1)
            out["trees"].append({"tree": k, "trace": tr, "records": rr})
    if name == "pomcp_deep":
        out["search_depth"] = facts["max_depth"]
        out["depth_limit"] = facts["depth_limit"]
    assert CHECKS.get(name, lambda f: True)(facts), (name, facts)
    return out, facts


def dumps(data):
    # (key order kept: a mixture's and a meta-policy's order is part of the case)
    return json.dumps(data, indent=None, separators=(",", ":")) + "\n"


def main(only=None, out_dir=OUT_DIR):
    os.makedirs(out_dir, exist_ok=True)
    limit = max(os.path.getsize(os.path.join(HERE, "coop_reaching", f))
                for f in os.listdir(os.path.join(HERE, "coop_reaching")))
    total = new_facts()
    caught_all_early = ran_out = False
    for name in CASES:
        if only and name not in only:
            continue
        data, facts = run_case(name)
        text = dumps(data)
        assert len(text) <= limit, (name, len(text), limit)
        with open(os.path.join(out_dir, name + ".json"), "w") as f:
            f.write(text)
        for k in range(3):
            total["rules"][k] += facts["rules"][k]
        for k in range(2):
            total["blocked_order"][k] += facts["blocked_order"][k]
        total["captures"] += facts["captures"]
        for e in data["episodes"]:
            tr = e["trace"]
            full = abs(float.fromhex(tr["return"]) - 1.0) < 1e-6
            caught_all_early |= full and tr["len"] < MAX_STEPS
            ran_out |= tr["len"] == MAX_STEPS and not full
        print(name, "written", len(text), facts,
              [(e["trace"]["len"], float.fromhex(e["trace"]["return"])) for e in data["episodes"]])
    if not only:
        assert total["captures"] > 0 and caught_all_early and ran_out, \
            (total, caught_all_early, ran_out)
        assert all(n > 0 for n in total["rules"]) and all(n > 0 for n in total["blocked_order"]), \
            total


if __name__ == "__main__":
    args = sys.argv[1:]
    out = [a[len("--out="):] for a in args if a.startswith("--out=")]
    main([a for a in args if not a.startswith("--out=")], out[0] if out else OUT_DIR)
