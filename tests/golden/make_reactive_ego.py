"""Reference goldens of state-reactive EGO policies on CooperativeReaching-v0
(tests/golden/reactive_ego/*.json):

    python tests/golden/make_reactive_ego.py [--out=DIR] [case ...]

The real reference planners (``oracle.ref_harness.make_reference_potmmcp`` /
``make_reference_mcts``, used as they are) are built over placeholder rows, as
``make_coop_reaching.py`` builds them; before ``planner.reset()`` the entries of
``planner.search_policy.policies`` whose spec row is ``None`` are replaced by
the ``GoalHeuristicPolicy`` their id names (a base planner's search policy by a
``SearchPolicyWrapper`` of it), wired to the ego's action stream.  The records
are in the schema of ``tests/golden/coop_reaching``.

The meta-policies named ``"P0:<name>"`` are read from
``reactive_ego/p0_meta_policy.json``, the reference's
``env_data/CooperativeReaching-v0/meta_policy.yaml`` rows in their key order;
the ego policies are H1 .. H5 in that order (the reference builds its dict
from a set: any order is one it may take).

THE STATE-FORM INVARIANT.  The kernels have no histories: a reactive ego policy
acts there on the simulation's running state.  At every entry of the
reference's ``_simulate`` and ``_rollout``, for every reactive ego policy whose
policy state has a position, the action from the NODE's policy state must equal
``action_from_state(hps.state)``.  The comparisons are counted
(``invariant_checks``); one mismatch aborts the generation.

Every case also asserts what it is there for (``CHECKS``).
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "posggym-baselines_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import make_coop_reaching as mcr  # noqa: E402

OUT_DIR = os.path.join(HERE, "reactive_ego")
ENV = mcr.ENV
H1, H2, H3, H4, H5 = HS = [f"{ENV}/H{k}-v0" for k in range(1, 6)]
TEST_CFG = mcr.TEST_CFG
MAX_STEPS = mcr.MAX_STEPS
TREES = 6
FIXED_EGO = [0.1, 0.3, 0.1, 0.1, 0.4]
FIXED_OTH = mcr.FIXED
ALL_H = {h: None for h in HS}


def p0_meta_policy(name):
    with open(os.path.join(HERE, "reactive_ego", "p0_meta_policy.json")) as f:
        return json.load(f)["meta_policy"][name]


def p0_spec(name):
    return {"ego": dict(ALL_H), "other": dict(ALL_H), "meta": "P0:" + name}


PUCB = {"action_selection": "pucb", "state_belief_only": False}
# name: planner, cfg overrides, spec, num_sims, [(planner seed, env seed)], ego,
#       size, obs_distance, the agent played against
CASES = {
    "potmmcp_p0_softmax": dict(planner="POTMMCP", over=dict(PUCB),   # (depth_limit 2)
                               spec=p0_spec("softmax"), num_sims=96, pairs=[(2, 2), (6, 6)],
                               ego="0", size=5, obs_distance=None, other_agent=H2),
    # long heuristic rollouts: the generic kernel
    "potmmcp_p0_greedy_deep": dict(planner="POTMMCP",
                                   over={"state_belief_only": False, "discount": 0.99,
                                         "epsilon": 0.01},
                                   spec=p0_spec("greedy"), num_sims=64, pairs=[(5, 5), (11, 11)],
                                   ego="0", size=4, obs_distance=None, other_agent=H4),
    # mixed kinds: the moving average leaves {0, 1}
    "potmmcp_mixed": dict(
        planner="POTMMCP", over=dict(PUCB),
        spec={"ego": {H4: None, "e_fixed": FIXED_EGO, H1: None},
              "other": {H1: None, H5: None, "o_fixed": FIXED_OTH},
              "meta": {H1: {H4: 0.5, "e_fixed": 0.25, H1: 0.25},
                       H5: {"e_fixed": 0.4, H1: 0.6},
                       "o_fixed": {H1: 0.2, H4: 0.3, "e_fixed": 0.5}}},
        num_sims=96, pairs=[(5, 5), (8, 8)], ego="1", size=5, obs_distance=1, other_agent=H4,
        trees=True),
    # the third selection rule (min-visit) on the mixed set
    "potmmcp_mixed_uniform": dict(
        planner="POTMMCP", over={"action_selection": "uniform", "state_belief_only": False},
        spec="potmmcp_mixed", num_sims=64, pairs=[(2, 2), (5, 5)], ego="1", size=5,
        obs_distance=1, other_agent=H4),
    # discount 0: depth_limit 0, so every child of a root is created and cut off
    # in the same simulation and the next root is a child that was never
    # expanded (prior code k + 1, no block).  With any deeper limit the reference
    # expands a child in the simulation that creates it.
    "potmmcp_myopic": dict(
        planner="POTMMCP", over=dict(PUCB, discount=0.0),
        spec={"ego": {H2: None, "e_fixed": FIXED_EGO, H3: None},
              "other": {H1: None, H5: None, "o_fixed": FIXED_OTH},
              "meta": {H1: {H2: 0.5, "e_fixed": 0.25, H3: 0.25},
                       H5: {"e_fixed": 0.4, H3: 0.6},
                       "o_fixed": {H3: 0.2, H2: 0.3, "e_fixed": 0.5}}},
        num_sims=32, pairs=[(2, 2), (6, 6)], ego="0", size=4, obs_distance=None, other_agent=H1),
    # 6 simulations per search: roots made by update() without a child
    "potmmcp_starved": dict(planner="POTMMCP", over=dict(PUCB), spec=p0_spec("uniform"),
                            num_sims=6, pairs=[(6, 6), (8, 8)], ego="0", size=5,
                            obs_distance=None, other_agent="random"),
    # the reference's tests/planning/test_pomcp.py:77 pattern
    "pomcp_h3_pucb": dict(planner="POMCP", over={"action_selection": "pucb"},
                          spec={"search": H3, "other": {"kind": "random"}}, num_sims=96,
                          pairs=[(12, 12), (20, 20)], ego="0", size=5, obs_distance=None,
                          other_agent="random"),
    # ~100 particles: every re-root reinvigorates
    "ipomcp_h2_mix": dict(planner="IPOMCP", over=dict(PUCB, search_time_limit=1.0),
                          spec={"search": H2,
                                "other": {"kind": "mixture",
                                          "policies": {H1: None, H5: None, "o_fixed": FIXED_OTH}}},
                          num_sims=48, pairs=[(14, 14), (19, 19)], ego="0", size=5,
                          obs_distance=None, other_agent=H1),
}


for _c in CASES.values():       # (a case that names another's spec shares it)
    if isinstance(_c["spec"], str):
        _c["spec"] = CASES[_c["spec"]]["spec"]


def resolved(spec):
    """The spec with a named meta-policy read from the fixture."""
    if isinstance(spec.get("meta"), str):
        return dict(spec, meta=p0_meta_policy(spec["meta"].split(":", 1)[1]))
    return spec


def placeholder_spec(spec):
    """What the harness builds fixed policies from: a uniform row stands where a
    heuristic will be swapped in, on either side."""
    spec = mcr.placeholder_spec(spec)
    if "ego" in spec:
        return dict(spec, ego={k: ([0.2] * 5 if v is None else v) for k, v in spec["ego"].items()})
    return dict(spec, search=[0.2] * 5)


def run_episode_case(case, cfg, env_seed, facts, tree=0, max_steps=MAX_STEPS):
    from coop_reaching_model import CooperativeReachingModel, run_episode
    from oracle.episode import ENV_TREE_BASE
    from oracle.ref_harness import (make_reference_mcts, make_reference_potmmcp,
                                    reference_mcts_record, reference_potmmcp_record)
    from oracle.rng import S_ACT_BASE, StreamRandom, Streams
    from posggym_baselines_amd.planning.policies import GoalHeuristicPolicy, is_reactive
    cls, spec, ego, num_sims = case["planner"], resolved(case["spec"]), case["ego"], case["num_sims"]
    streams = Streams(cfg["seed"], tree)
    model = CooperativeReachingModel(streams, case["size"], case["obs_distance"])
    other = [i for i in model.possible_agents if i != ego][0]
    heuristic = lambda agent, pid: GoalHeuristicPolicy.from_id(
        model, agent, pid, rng=StreamRandom(streams, S_ACT_BASE + int(agent)))
    typed = cls == "POTMMCP"
    if typed:
        planner = make_reference_potmmcp(model, ego, cfg, num_sims, streams, placeholder_spec(spec))
        pols = planner.search_policy.policies
        for pid, row in spec["ego"].items():
            if row is None:
                pols[pid] = heuristic(ego, pid)
        assert list(pols) == list(spec["ego"])            # the meta-policy's order is the spec's
        ego_pols = dict(pols)
    else:
        planner = make_reference_mcts(model, ego, cfg, num_sims, streams, placeholder_spec(spec), cls)
        import posggym_baselines.planning.search_policy as sp_mod   # (the harness set it up)
        pol = heuristic(ego, spec["search"])
        planner.search_policy = sp_mod.SearchPolicyWrapper(pol)
        ego_pols = {pol.policy_id: pol}
    if mcr.is_mixture(spec):
        mpols = planner.other_agent_policies[other].policies
        for pid, row in mcr.other_entries(spec).items():
            if row is None:
                mpols[pid] = heuristic(other, pid)
        assert list(mpols) == list(mcr.other_entries(spec))

    # ---- the state-form invariant and the facts the case is there for
    def check_state(pid, pstate, hps):
        pol = ego_pols[pid]
        if not is_reactive(pol) or pstate.get("pos") is None:
            return
        facts["invariant_checks"] += 1
        if pol.action(pstate) != pol.action_from_state(hps.state):
            raise SystemExit(f"STATE-FORM INVARIANT BROKEN: {pid} at policy state {pstate}, "
                             f"state {hps.state}")

    def node_states(node):
        return node.search_policy_state if typed else {next(iter(ego_pols)): node.search_policy_state}

    sim, roll = planner._simulate, planner._rollout

    def simulate(hps, obs_node, depth, search_policy):
        for pid, ps in node_states(obs_node).items():
            check_state(pid, ps, hps)
        before = dict(obs_node.action_probs)
        out = sim(hps, obs_node, depth, search_policy)
        if depth > 0 and obs_node.action_probs != before:
            facts["ema_moved_below_root"] += 1
        return out

    def rollout(hps, depth, rollout_policy, rollout_policy_state):
        check_state(rollout_policy.policy_id, rollout_policy_state, hps)
        return roll(hps, depth, rollout_policy, rollout_policy_state)

    planner._simulate, planner._rollout = simulate, rollout
    drawn = set()
    if typed:
        sample = planner.search_policy.sample_policy
        expected = planner.search_policy.get_expected_action_probs
        first = []

        def sample_policy(other_state):
            out = sample(other_state)
            drawn.add(out.policy_id)
            return out

        def get_expected_action_probs(dist, pstate):
            out = expected(dist, pstate)
            if not first:
                first.append(dict(out))
            elif out != first[0]:
                facts["code0_root_at_t>0_differs"] += 1
            return out

        planner.search_policy.sample_policy = sample_policy
        planner.search_policy.get_expected_action_probs = get_expected_action_probs
    update = planner._update

    def _update(action, obs):
        an = planner.root.children[action] if action in planner.root.children else None
        existed = an is not None and an.has_child(obs)
        update(action, obs)
        if existed and not planner.root.is_absorbing and len(planner.root.children) == 0:
            facts["unexpanded_child_became_root"] += 1

    planner._update = _update
    planner.reset()
    records = []

    def step(obs):
        searched = not planner.root.is_absorbing
        drawn.clear()
        a = planner.step(obs)
        if len(drawn) >= 2:
            facts["searches_with_two_ego_policies"] += 1
        if typed:
            records.append(reference_potmmcp_record(planner, searched, a))
        else:
            records.append(reference_mcts_record(planner, searched, a, spec))
        return a

    env = CooperativeReachingModel(Streams(env_seed, ENV_TREE_BASE), case["size"],
                                   case["obs_distance"])
    trace = run_episode(env, step, ego, case["other_agent"], max_steps)
    trace["env_seed"] = env_seed
    planner.close()
    return trace, records


FACTS = ("invariant_checks", "ema_moved_below_root", "code0_root_at_t>0_differs",
         "unexpanded_child_became_root", "searches_with_two_ego_policies")
_typed = lambda f: f["searches_with_two_ego_policies"] > 0 and f["ema_moved_below_root"] > 0
# what each case is there for (every case: invariant_checks > 0)
CHECKS = {
    "potmmcp_p0_softmax": _typed,
    "potmmcp_p0_greedy_deep": lambda f: f["ema_moved_below_root"] > 0,
    "potmmcp_mixed": _typed,
    "potmmcp_myopic": lambda f: f["unexpanded_child_became_root"] > 0,
    "potmmcp_starved": lambda f: f["code0_root_at_t>0_differs"] > 0,
}


def run_case(name):
    case = CASES[name]
    out = {"case": name, "planner": case["planner"], "env": ENV, "size": case["size"],
           "obs_distance": case["obs_distance"], "num_sims": case["num_sims"], "ego": case["ego"],
           "max_steps": MAX_STEPS, "other_agent": case["other_agent"], "spec": case["spec"],
           "episodes": []}
    facts = {k: 0 for k in FACTS}
    for seed, env_seed in case["pairs"]:
        cfg = dict(TEST_CFG, **case["over"])
        cfg["seed"] = seed
        tr, rr = run_episode_case(case, cfg, env_seed, facts)
        out["episodes"].append({"config": dict(cfg), "env_seed": env_seed, "trace": tr,
                                "records": rr})
    if case.get("trees"):
        # the first step of trees 0 .. 5 (keys (seed, k)) of the first episode
        seed, env_seed = case["pairs"][0]
        cfg = dict(TEST_CFG, **case["over"])
        cfg["seed"] = seed
        out["trees"] = []
        for k in range(TREES):
            tr, rr = run_episode_case(case, cfg, env_seed, {k: 0 for k in FACTS}, tree=k,
                                      max_steps=1)
            out["trees"].append({"tree": k, "trace": tr, "records": rr})
    assert facts["invariant_checks"] > 0, (name, facts)
    assert CHECKS.get(name, lambda f: True)(facts), (name, facts)
    out["facts"] = facts
    return out, facts


def main(only=None, out_dir=OUT_DIR):
    os.makedirs(out_dir, exist_ok=True)
    for name in CASES:
        if only and name not in only:
            continue
        data, facts = run_case(name)
        with open(os.path.join(out_dir, name + ".json"), "w") as f:
            f.write(mcr.dumps(data))
        print(name, "written", facts,
              [(e["trace"]["len"], float.fromhex(e["trace"]["return"])) for e in data["episodes"]])


if __name__ == "__main__":
    args = sys.argv[1:]
    out = [a[len("--out="):] for a in args if a.startswith("--out=")]
    main([a for a in args if not a.startswith("--out=")], out[0] if out else OUT_DIR)
