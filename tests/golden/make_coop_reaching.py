"""Reference goldens of CooperativeReaching-v0 (tests/golden/coop_reaching/*.json):

    python tests/golden/make_coop_reaching.py [--out=DIR] [case ...]

The real reference planners (``oracle.ref_harness.make_reference_pomcp`` /
``make_reference_mcts`` / ``make_reference_potmmcp``, used as they are) run on
the build's Python restatement of the environment
(``tests/golden/coop_reaching_model.py``); the episode loop is
``coop_reaching_model.run_episode``, as the harness's own is tied to the two
environments of ``oracle.envs``.  A mixture member whose spec row is ``None``
is the heuristic agent its id names: the harness builds a placeholder row for
it and the entry of ``planner.other_agent_policies[other].policies`` is
replaced by a ``GoalHeuristicPolicy`` before ``planner.reset()``
(make_reactive.py does the same for Driving-v1).

Records are ``reference_record`` / ``reference_mcts_record`` /
``reference_potmmcp_record``'s.  A case's ``other_agent`` is the agent the
episodes are played against: ``"random"`` or a heuristic agent's id.

Every case asserts what it is there for (``CHECKS``), and across the cases
some episode returns 1.0, some 0.75, and some runs to the 50-step limit; the
generator aborts otherwise.
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
OUT_DIR = os.path.join(HERE, "coop_reaching")

ENV = "CooperativeReaching-v0"
H1, H2, H3, H4, H5 = (f"{ENV}/H{k}-v0" for k in range(1, 6))
TEST_CFG = dict(discount=0.95, search_time_limit=0.1, c=math.sqrt(2), truncated=False,
                action_selection="ucb", pucb_exploration_fraction=0.25, known_bounds=None,
                step_limit=None, epsilon=0.92, seed=0, state_belief_only=True)
FIXED = [0.3, 0.1, 0.1, 0.4, 0.1]
MIX3 = {"kind": "mixture", "policies": {H1: None, H2: None, "o_fixed": FIXED}}
MAX_STEPS = 50
TREES = 6

# name: planner, cfg overrides, spec, num_sims, [(planner seed, env seed)], ego,
#       size, obs_distance, the agent played against
# (seeds: chosen so that the episodes meet the assertions of CHECKS and main and,
# but for the one that runs to the step limit, are short: the files stay small)
CASES = {
    "pomcp_ucb": dict(planner="POMCP", over={}, spec=None, num_sims=128,
                      pairs=[(54, 54), (34, 34)], ego="0", size=5, obs_distance=None,
                      other_agent="random"),
    # partial observation: beliefs over the other agent's cell
    "pomcp_pucb_ego1_od1": dict(planner="POMCP", over={"action_selection": "pucb"}, spec=None,
                                num_sims=96, pairs=[(16, 16), (9, 9)], ego="1", size=5,
                                obs_distance=1, other_agent=H1),
    # rollouts to the step limit, and a deep tree: the ego sees the other agent
    # on its own cell only, so an action has one observation child until they
    # meet, and with a small c the search follows one line of play
    "pomcp_deep": dict(planner="POMCP", over={"discount": 0.99, "epsilon": 0.01, "c": 0.05},
                       spec=None, num_sims=64, pairs=[(9, 9), (4, 4)], ego="0", size=4,
                       obs_distance=0, other_agent=H1),
    "ipomcp_pucb_mix": dict(planner="IPOMCP", over={"action_selection": "pucb",
                                                    "state_belief_only": False},
                            spec={"search": None, "other": MIX3}, num_sims=96,
                            pairs=[(16, 16), (7, 7)], ego="0", size=5, obs_distance=None,
                            other_agent=H1),
    # ~100 particles: every re-root reinvigorates
    "ipomcp_reinv": dict(planner="IPOMCP", over={"action_selection": "pucb",
                                                 "state_belief_only": False,
                                                 "search_time_limit": 1.0},
                         spec={"search": None, "other": MIX3}, num_sims=48,
                         pairs=[(20, 20), (8, 8)], ego="0", size=5, obs_distance=None,
                         other_agent=H2),
    "potmmcp_ucb_ego1_od2": dict(
        planner="POTMMCP", over={"state_belief_only": False},
        spec={"ego": {"u": [0.2] * 5, "left": [0.1, 0.1, 0.1, 0.6, 0.1],
                      "down": [0.1, 0.1, 0.6, 0.1, 0.1]},
              "other": {H1: None, H2: None, H3: None, H4: None, H5: None},
              "meta": {H1: {"u": 0.5, "left": 0.5}, H2: {"down": 1.0},
                       H3: {"u": 0.2, "left": 0.4, "down": 0.4}, H4: {"left": 0.3, "down": 0.7},
                       H5: {"u": 1.0}}},
        num_sims=64, pairs=[(2, 2), (8, 8)], ego="1", size=5, obs_distance=2,
        other_agent=H5),
    # the one non-mixture type path: a stateless fixed other agent
    "mcts_fixed_other": dict(planner="MCTS", over={},
                             spec={"search": None, "other": {"kind": "fixed", "probs": FIXED}},
                             num_sims=96, pairs=[(40, 40), (34, 34)], ego="0", size=5,
                             obs_distance=None, other_agent="random"),
}


def other_entries(spec):
    return spec["other"]["policies"] if "kind" in spec["other"] else spec["other"]


def placeholder_spec(spec):
    """The spec the reference harness builds fixed policies from: a uniform row
    stands where a heuristic agent will be swapped in."""
    if spec is None or spec["other"].get("kind") in ("fixed", "random"):
        return spec
    rows = {k: ([0.2] * 5 if v is None else v) for k, v in other_entries(spec).items()}
    if "kind" in spec["other"]:
        return dict(spec, other=dict(spec["other"], policies=rows))
    return dict(spec, other=rows)


def is_mixture(spec):
    return spec is not None and spec["other"].get("kind") not in ("fixed", "random")


def run_episode_case(case, cfg, env_seed, facts, tree=0, max_steps=MAX_STEPS):
    from coop_reaching_model import CooperativeReachingModel, run_episode
    from oracle.episode import ENV_TREE_BASE
    from oracle.ref_harness import (make_reference_mcts, make_reference_pomcp,
                                    make_reference_potmmcp, reference_mcts_record,
                                    reference_potmmcp_record, reference_record)
    from oracle.rng import S_ACT_BASE, StreamRandom, Streams
    from posggym_baselines_amd.planning.policies import GoalHeuristicPolicy
    cls, spec, ego, num_sims = case["planner"], case["spec"], case["ego"], case["num_sims"]
    streams = Streams(cfg["seed"], tree)
    model = CooperativeReachingModel(streams, case["size"], case["obs_distance"])
    other = [i for i in model.possible_agents if i != ego][0]
    if cls == "POMCP":
        planner = make_reference_pomcp(model, ego, cfg, num_sims, streams, "POMCP")
    elif cls == "POTMMCP":
        planner = make_reference_potmmcp(model, ego, cfg, num_sims, streams, placeholder_spec(spec))
    else:
        planner = make_reference_mcts(model, ego, cfg, num_sims, streams, placeholder_spec(spec), cls)
    reactive = {}
    if is_mixture(spec):
        pols = planner.other_agent_policies[other].policies
        for pid, row in other_entries(spec).items():
            if row is None:
                pols[pid] = reactive[pid] = GoalHeuristicPolicy.from_id(
                    model, other, pid, rng=StreamRandom(streams, S_ACT_BASE + int(other)))
        assert list(pols) == list(other_entries(spec))      # the mixture's order is the spec's
        # accepted rejection samples that carry a reactive policy
        sampler = planner._reinvigorator
        inner = sampler._rejection_sample

        def rejection_sample(agent_id, action, obs, **kw):
            out = inner(agent_id, action, obs, **kw)
            facts["reinv_accepted_reactive"] += sum(
                1 for p in out if model._obs(p.state, int(agent_id)) == obs
                and p.policy_state[other]["policy_id"] in reactive)
            return out

        sampler._rejection_sample = rejection_sample
    planner.reset()
    records = []
    prev_ids = [None]

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
            parts = planner.root.belief.particles
            facts["max_belief_states"] = max(facts["max_belief_states"],
                                             len({p.state for p in parts}))
            facts["max_depth"] = max(facts["max_depth"],
                                     int(planner.step_statistics["search_depth"]))
            if is_mixture(spec):
                ids = {p.policy_state[other]["policy_id"] for p in parts}
                if len(records) >= 4 and len(ids) >= 2:
                    facts["two_policies_at_step_3"] += 1
                if prev_ids[0] is not None and prev_ids[0] - ids:
                    facts["belief_lost_a_policy"] += 1
                prev_ids[0] = ids
        return a

    env = CooperativeReachingModel(Streams(env_seed, ENV_TREE_BASE), case["size"],
                                   case["obs_distance"])
    trace = run_episode(env, step, ego, case["other_agent"], max_steps)
    trace["env_seed"] = env_seed
    planner.close()
    return trace, records


# what each case is there for
CHECKS = {
    "pomcp_pucb_ego1_od1": lambda f: f["max_belief_states"] >= 3,
    "pomcp_deep": lambda f: f["max_depth"] >= 20,
    "ipomcp_pucb_mix": lambda f: f["two_policies_at_step_3"] > 0 and f["belief_lost_a_policy"] > 0,
    "ipomcp_reinv": lambda f: f["reinv_accepted_reactive"] >= 100,
}


def run_case(name):
    case = CASES[name]
    out = {"case": name, "planner": case["planner"], "env": ENV, "size": case["size"],
           "obs_distance": case["obs_distance"], "num_sims": case["num_sims"], "ego": case["ego"],
           "max_steps": MAX_STEPS, "other_agent": case["other_agent"], "spec": case["spec"],
           "episodes": []}
    facts = {"max_belief_states": 0, "max_depth": 0, "two_policies_at_step_3": 0,
             "belief_lost_a_policy": 0, "reinv_accepted_reactive": 0}
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
            tr, rr = run_episode_case(case, cfg, env_seed, dict(facts), tree=k, max_steps=1)
            out["trees"].append({"tree": k, "trace": tr, "records": rr})
    assert CHECKS.get(name, lambda f: True)(facts), (name, facts)
    return out, facts


def dumps(data):
    # (key order kept: a mixture's and a meta-policy's order is part of the case)
    return json.dumps(data, indent=None, separators=(",", ":")) + "\n"


def main(only=None, out_dir=OUT_DIR):
    os.makedirs(out_dir, exist_ok=True)
    returns, lengths = set(), set()
    for name in CASES:
        if only and name not in only:
            continue
        data, facts = run_case(name)
        with open(os.path.join(out_dir, name + ".json"), "w") as f:
            f.write(dumps(data))
        for e in data["episodes"]:
            returns.add(float.fromhex(e["trace"]["return"]))
            lengths.add(e["trace"]["len"])
        print(name, "written", facts,
              [(e["trace"]["len"], float.fromhex(e["trace"]["return"])) for e in data["episodes"]])
    if not only:
        assert 1.0 in returns and 0.75 in returns and MAX_STEPS in lengths, (returns, lengths)


if __name__ == "__main__":
    args = sys.argv[1:]
    out = [a[len("--out="):] for a in args if a.startswith("--out=")]
    main([a for a in args if not a.startswith("--out=")], out[0] if out else OUT_DIR)
