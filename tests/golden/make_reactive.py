"""Reference goldens of the type-based search with state-reactive other-agent
policies (tests/golden/reactive/*.json):

    python tests/golden/make_reactive.py [case ...]

The real reference planners (``oracle.ref_harness.make_reference_mcts`` /
``make_reference_potmmcp``) are built on a spec whose reactive entries are
placeholders, and those entries of ``planner.other_agent_policies[other]
.policies`` are replaced by ``ShortestPathPolicy`` objects before
``planner.reset()``; the reference then tracks their policy states itself
(mcts.py:207-214, 349-351, 436-438).  Records are ``reference_mcts_record`` /
``reference_potmmcp_record``'s, whose belief digest includes each particle's
policy index.  A spec's other-agent policy is a list of probabilities (a fixed
distribution) or ``None`` (the shortest-path agent its id names).

Every case asserts what keeps a table lookup from passing it: particles of at
least two policies survive to step 3, and some reactive policy picks different
actions for two particles of one belief.  ``ipomcp_reinv`` also asserts that a
re-root accepted a rejection sample whose particle carries a reactive policy.

A single reactive other agent outside a mixture (``state_belief_only=True``, as
``mcts_fixed_other_pucb`` has a fixed one) has no case: the reference then
calls ``sample_action({})`` (mcts.py:609-610), and a policy that acts on its
observation has none in ``{}``; the build refuses that arrangement too.
"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "posggym-baselines_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT_DIR = os.path.join(HERE, "reactive")

A0, A40, A60, A80, A100 = (f"Driving-v1/A{g}Shortestpath-v0" for g in (0, 40, 60, 80, 100))
TEST_CFG = dict(discount=0.95, search_time_limit=0.1, c=math.sqrt(2), truncated=False,
                action_selection="ucb", pucb_exploration_fraction=0.25, known_bounds=None,
                step_limit=None, epsilon=0.92, seed=0, state_belief_only=False)
FIXED = [0.3, 0.1, 0.1, 0.4, 0.1]
MAX_STEPS = 12
ENV = "Driving-v1"

# name: (planner, cfg overrides, spec, num_sims, [(planner seed, env seed)], ego)
# (seeds: chosen from 60..99 so that the episodes meet the assertions of run_case)
CASES = {
    # depth_limit 2 (epsilon 0.92)
    "ipomcp_pucb": ("IPOMCP", {"action_selection": "pucb"},
                    {"search": None, "other": {"kind": "mixture", "policies": {
                        A100: None, A0: None, "o_fixed": FIXED}}}, 64, [(60, 60), (61, 61)], "0"),
    # long rollouts: the rollout's other-agent draw
    "ipomcp_deep_ego1": ("IPOMCP", {"discount": 0.95, "epsilon": 0.01},
                         {"search": None, "other": {"kind": "mixture", "policies": {
                             A40: None, A80: None}}}, 32, [(63, 63)], "1"),
    # 107 particles: every re-root reinvigorates
    "ipomcp_reinv": ("IPOMCP", {"action_selection": "pucb", "search_time_limit": 1.0},
                     {"search": None, "other": {"kind": "mixture", "policies": {
                         A100: None, A0: None, "o_fixed": FIXED}}}, 48, [(93, 93), (95, 95)], "0"),
    "potmmcp": ("POTMMCP", {"action_selection": "pucb"},
                {"ego": {"u": [0.2] * 5, "acc": [0.1, 0.5, 0.1, 0.2, 0.1]},
                 "other": {A100: None, A60: None, A0: None},
                 "meta": {A100: {"u": 0.5, "acc": 0.5}, A60: {"acc": 1.0}, A0: {"u": 0.7, "acc": 0.3}}},
                64, [(77, 77)], "0"),
}


def other_entries(spec):
    return spec["other"]["policies"] if "kind" in spec["other"] else spec["other"]


def placeholder_spec(spec):
    """The spec the reference harness builds fixed policies from: a uniform row
    stands where a reactive policy will be swapped in."""
    rows = {k: ([0.2] * 5 if v is None else v) for k, v in other_entries(spec).items()}
    if "kind" in spec["other"]:
        return dict(spec, other=dict(spec["other"], policies=rows))
    return dict(spec, other=rows)


def run_episode_case(cls, cfg, spec, num_sims, env_seed, ego, facts):
    from oracle.envs import make_model
    from oracle.episode import run_episode
    from oracle.ref_harness import (make_reference_mcts, make_reference_potmmcp,
                                    reference_mcts_record, reference_potmmcp_record)
    from oracle.rng import S_ACT_BASE, StreamRandom, Streams
    from posggym_baselines_amd.planning.policies import ShortestPathPolicy
    streams = Streams(cfg["seed"], 0)
    model = make_model(ENV, streams)
    if cls == "POTMMCP":
        planner = make_reference_potmmcp(model, ego, cfg, num_sims, streams, placeholder_spec(spec))
    else:
        planner = make_reference_mcts(model, ego, cfg, num_sims, streams, placeholder_spec(spec),
                                      cls)
    other = [i for i in model.possible_agents if i != ego][0]
    pols = planner.other_agent_policies[other].policies
    reactive = {}
    for pid, row in other_entries(spec).items():
        if row is None:
            pols[pid] = reactive[pid] = ShortestPathPolicy.from_id(
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

    def step(obs):
        searched = not planner.root.is_absorbing
        a = planner.step(obs)
        if cls == "POTMMCP":
            records.append(reference_potmmcp_record(planner, searched, a))
        else:
            records.append(reference_mcts_record(planner, searched, a, spec))
        if searched:
            parts = planner.root.belief.particles
            ids = {p.policy_state[other]["policy_id"] for p in parts}
            if len(records) >= 4 and len(ids) >= 2:
                facts["two_policies_at_step_3"] += 1
            for pid, pol in reactive.items():
                acts = {pol.action(p.policy_state[other]["policy_state"]) for p in parts
                        if p.policy_state[other]["policy_id"] == pid}
                facts["reactive_actions_differ"] += len(acts) >= 2
        return a

    trace = run_episode(step, env_seed, ego=ego, max_steps=MAX_STEPS, env=ENV)
    planner.close()
    return trace, records


def run_case(name):
    cls, over, spec, num_sims, pairs, ego = CASES[name]
    out = {"case": name, "planner": cls, "env": ENV, "num_sims": num_sims, "ego": ego,
           "max_steps": MAX_STEPS, "spec": spec, "episodes": []}
    facts = {"two_policies_at_step_3": 0, "reactive_actions_differ": 0,
             "reinv_accepted_reactive": 0}
    for seed, env_seed in pairs:
        cfg = dict(TEST_CFG, **over)
        cfg["seed"] = seed
        tr, rr = run_episode_case(cls, cfg, spec, num_sims, env_seed, ego, facts)
        out["episodes"].append({"config": dict(cfg), "env_seed": env_seed, "trace": tr,
                                "records": rr})
    assert facts["two_policies_at_step_3"] > 0, (name, facts)
    assert facts["reactive_actions_differ"] > 0, (name, facts)
    if name == "ipomcp_reinv":
        assert facts["reinv_accepted_reactive"] > 0, (name, facts)
    return out, facts


def dumps(data):
    # (key order kept: a mixture's and a meta-policy's order is part of the case)
    return json.dumps(data, indent=None, separators=(",", ":")) + "\n"


def main(only=None, out_dir=OUT_DIR):
    os.makedirs(out_dir, exist_ok=True)
    for name in CASES:
        if only and name not in only:
            continue
        data, facts = run_case(name)
        with open(os.path.join(out_dir, name + ".json"), "w") as f:
            f.write(dumps(data))
        print(name, "written", facts, [e["trace"]["len"] for e in data["episodes"]])


if __name__ == "__main__":
    main(sys.argv[1:])
