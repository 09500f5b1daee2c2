"""tests/golden/predator_prey_agents/*.json are what
tests/golden/make_predator_prey_agents.py writes: the recorded ``facts`` meet the
conditions the generator asserts, and where the reference planner is present
every case is regenerated (the generator's own assertions run again) and compared
byte for byte."""
import importlib.util
import json
import os

import pytest

from oracle.ref_harness import reference_available

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["ipomcp_pucb", "ipomcp_deep_ego1", "ipomcp_reinv", "potmmcp", "mcts_mix"]
H1, H2, H3 = (f"PredatorPrey-v0/H{k}-v0" for k in (1, 2, 3))


def generator():
    spec = importlib.util.spec_from_file_location(
        "make_predator_prey_agents",
        os.path.join(HERE, "golden", "make_predator_prey_agents.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fixture(case):
    with open(os.path.join(HERE, "golden", "predator_prey_agents", case + ".json")) as f:
        return json.load(f)


def test_the_fixture_set_is_the_generators_and_small():
    gen = generator()
    assert list(gen.CASES) == CASES
    names = sorted(os.listdir(gen.OUT_DIR))
    assert names == sorted(c + ".json" for c in CASES)
    older = os.path.join(HERE, "golden", "predator_prey")
    limit = max(os.path.getsize(os.path.join(older, f)) for f in os.listdir(older))
    for n in names:
        assert os.path.getsize(os.path.join(gen.OUT_DIR, n)) <= limit, n


def test_the_cases_are_the_issues():
    data = {c: fixture(c) for c in CASES}
    mix = lambda c: list(data[c]["spec"]["other"]["policies"].items())
    for c in CASES:
        d = data[c]
        assert d["env"] == "PredatorPrey-v0" and len(d["episodes"]) == 2
        assert d["num_sims"] <= 128 and d["max_steps"] == 12
        assert all(e["trace"]["len"] <= 12 for e in d["episodes"])
        assert all(e["config"]["state_belief_only"] is False for e in d["episodes"])
    d = data["ipomcp_pucb"]
    assert d["planner"] == "IPOMCP" and d["episodes"][0]["config"]["action_selection"] == "pucb"
    assert [k for k, v in mix("ipomcp_pucb")] == [H1, H2, "o_fixed"]
    assert [v is None for k, v in mix("ipomcp_pucb")] == [True, True, False]
    assert d["kwargs"] == dict(grid="5x5", num_prey=2, prey_strength=1, obs_dim=1)
    d = data["ipomcp_deep_ego1"]
    cfg = d["episodes"][0]["config"]
    assert (d["planner"], d["ego"], cfg["action_selection"], cfg["epsilon"]) == \
        ("IPOMCP", "1", "ucb", 0.01)
    assert mix("ipomcp_deep_ego1") == [(H1, None), (H3, None)]
    assert d["kwargs"] == dict(grid="10x10", num_prey=3, prey_strength=2, obs_dim=2)
    d = data["ipomcp_reinv"]
    assert d["spec"] == data["ipomcp_pucb"]["spec"] and d["kwargs"] == data["ipomcp_pucb"]["kwargs"]
    assert d["episodes"][0]["config"]["search_time_limit"] == 1.0
    d = data["potmmcp"]
    assert d["planner"] == "POTMMCP" and list(d["spec"]["other"].items()) == \
        [(H1, None), (H2, None), (H3, None)]
    assert all(isinstance(v, list) for v in d["spec"]["ego"].values())
    assert [t["tree"] for t in d["trees"]] == list(range(6))
    assert all(len(t["records"]) == 1 for t in d["trees"])
    d = data["mcts_mix"]
    assert d["planner"] == "MCTS" and [k for k, v in mix("mcts_mix")] == [H2, H3, "o_fixed"]


def check_facts(case, facts):
    assert facts["pi_checks"] > 0
    assert facts["two_policies_at_step_3"] > 0 and facts["reactive_pis_differ"] > 0
    if case == "ipomcp_reinv":
        # 107 particles of 128: every re-root reinvigorates
        assert facts["min_particles"] < 128 and facts["reinv_accepted_reactive"] > 0


def test_recorded_facts_meet_the_generators_conditions():
    total = {b: 0 for b in ("prey", "mate", "explore", "tie", "blocked")}
    for c in CASES:
        facts = fixture(c)["facts"]
        check_facts(c, facts)
        # every draw was checked against the particle's state
        assert facts["pi_checks"] == facts["prey"] + facts["mate"] + facts["explore"]
        for b in total:
            total[b] += facts[b]
    assert all(n > 0 for n in total.values()), total


def test_records_hold_what_a_table_lookup_cannot():
    """searched records with more than one policy in the belief, and non-zero values"""
    for c in CASES:
        recs = [r for e in fixture(c)["episodes"] for r in e["records"]]
        assert any(r.get("searched", True) for r in recs)
    assert any(float.fromhex(e["trace"]["return"]) > 0.0
               for c in CASES for e in fixture(c)["episodes"])


@pytest.mark.skipif(not reference_available(), reason="the reference planner is not present")
@pytest.mark.parametrize("case", CASES)
def test_fixtures_regenerate_byte_for_byte(case):
    gen = generator()
    data, facts = gen.run_case(case)
    check_facts(case, facts)
    with open(os.path.join(gen.OUT_DIR, case + ".json"), "rb") as f:
        assert f.read() == gen.dumps(data).encode()
