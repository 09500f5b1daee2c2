"""The PredatorPrey-v0 goldens (tests/golden/predator_prey): what the committed
files hold, and -- where the reference is available -- that
tests/golden/make_predator_prey.py reproduces them byte for byte from the real
reference planners."""
import filecmp
import os
import struct
import subprocess
import sys

import pytest

from golden_util import GOLDEN, load
from oracle.ref_harness import reference_available

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["pomcp_ucb", "pomcp_pucb_ego1", "pomcp_deep", "pomcp_dl1", "pomcp_dl3", "ipomcp_reinv",
         "potmmcp_ucb", "mcts_fixed_other"]
DIR = os.path.join(GOLDEN, "predator_prey")


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def test_committed_goldens_hold_the_cases_they_are_there_for():
    data = {c: load("predator_prey/" + c) for c in CASES}
    assert sorted(os.listdir(DIR)) == sorted(c + ".json" for c in CASES)
    largest = max(os.path.getsize(os.path.join(GOLDEN, "coop_reaching", f))
                  for f in os.listdir(os.path.join(GOLDEN, "coop_reaching")))
    caught_all_early = ran_out = caught = False
    for c, d in data.items():
        assert d["env"] == "PredatorPrey-v0" and len(d["episodes"]) == 2, c
        assert d["num_sims"] <= 128 and d["max_steps"] <= 50
        unit = f32(1.0 / d["kwargs"]["num_prey"])
        for ep in d["episodes"]:
            tr = ep["trace"]
            assert len(ep["records"]) == tr["len"] == len(tr["steps"]) <= d["max_steps"]
            assert all(r["num_sims"] == d["num_sims"] for r in ep["records"] if r["searched"])
            # returns on the float32(1 / num_prey) lattice, as in the reference's br_results.csv
            ret, total = float.fromhex(tr["return"]), 0.0
            for s in tr["steps"]:
                r = float.fromhex(s["reward"])
                assert r in [k * unit for k in range(d["kwargs"]["num_prey"] + 1)], (c, r)
                total += r
                caught |= r > 0.0
            assert ret == total and ret in [0.0] + [
                sum([unit] * k) for k in range(1, d["kwargs"]["num_prey"] + 1)], (c, ret)
            full = ret == sum([unit] * d["kwargs"]["num_prey"])
            assert full or tr["len"] == d["max_steps"]        # a shorter episode caught every prey
            caught_all_early |= full and tr["len"] < d["max_steps"]
            ran_out |= tr["len"] == d["max_steps"] and not full
        assert os.path.getsize(os.path.join(DIR, c + ".json")) <= largest
    assert caught and caught_all_early and ran_out
    assert f32(1.0 / 3) == 0.3333333432674408 and 3 * f32(1.0 / 3) == 1.0000000298023224
    p = data["pomcp_ucb"]
    assert (p["planner"], p["ego"]) == ("POMCP", "0")
    assert p["kwargs"] == dict(grid="10x10", num_prey=3, prey_strength=2, obs_dim=2)
    assert p["episodes"][0]["config"]["action_selection"] == "ucb"
    valued = [any(float.fromhex(v) != 0.0 for v in r["child_values"])
              for ep in p["episodes"] for r in ep["records"] if r["searched"]]
    assert sum(valued) >= len(valued) // 2          # FP64 statistics, not only visits
    for c, dl, sel in (("pomcp_dl1", 0.96, "ucb"), ("pomcp_dl3", 0.87, "pucb")):
        cfg = data[c]["episodes"][0]["config"]
        assert (data[c]["planner"], cfg["epsilon"], cfg["action_selection"]) == ("POMCP", dl, sel)
    p = data["pomcp_pucb_ego1"]
    assert (p["planner"], p["ego"]) == ("POMCP", "1")
    assert p["kwargs"] == dict(grid="5x5", num_prey=1, prey_strength=1, obs_dim=1)
    assert p["episodes"][0]["config"]["action_selection"] == "pucb"
    p = data["pomcp_deep"]
    cfg = p["episodes"][0]["config"]
    assert (cfg["discount"], cfg["epsilon"], cfg["action_selection"]) == (0.99, 0.01, "ucb")
    assert p["depth_limit"] + 1 > 4 and p["search_depth"] >= 6
    assert p["search_depth"] == max(r["search_depth"] for ep in p["episodes"]
                                    for r in ep["records"] if r["searched"])
    p = data["ipomcp_reinv"]
    assert p["planner"] == "IPOMCP" and p["kwargs"]["grid"] == "5x5"
    assert list(p["spec"]["other"]["policies"]) == ["o_u", "o_left", "o_fixed"]
    assert p["spec"]["search"] is None
    cfg = p["episodes"][0]["config"]
    assert (cfg["action_selection"], cfg["search_time_limit"]) == ("pucb", 1.0)
    # about 107 particles: every re-root reinvigorates
    sizes = [r["belief_size"] for ep in p["episodes"] for r in ep["records"] if r["searched"]]
    assert len(sizes) >= 10 and all(100 <= s < 128 for s in sizes)
    p = data["potmmcp_ucb"]
    assert p["planner"] == "POTMMCP" and len(p["spec"]["ego"]) == 3
    assert list(p["spec"]["other"]) == list(p["spec"]["meta"]) == ["o_u", "o_left", "o_fixed"]
    assert [t["tree"] for t in p["trees"]] == list(range(6))
    assert len({t["records"][0]["belief_digest"] for t in p["trees"]}) > 1
    p = data["mcts_fixed_other"]
    assert p["planner"] == "MCTS" and p["spec"]["other"]["kind"] == "fixed"
    assert p["episodes"][0]["config"]["state_belief_only"] is True


@pytest.mark.skipif(not reference_available(),
                    reason="the reference exists only in the build container")
def test_make_predator_prey_regenerates_the_committed_fixtures(tmp_path):
    """(a few seconds; the generator aborts when a case misses its own assertions)"""
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_predator_prey.py"),
                        f"--out={tmp_path}"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    names = [c + ".json" for c in CASES]
    _, mismatch, errors = filecmp.cmpfiles(DIR, str(tmp_path), names, shallow=False)
    assert mismatch == [] and errors == []
