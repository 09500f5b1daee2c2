"""The CooperativeReaching-v0 goldens (tests/golden/coop_reaching): what the
committed files hold, and -- where the reference is available -- that
tests/golden/make_coop_reaching.py reproduces them byte for byte from the real
reference planners."""
import filecmp
import os
import subprocess
import sys

import pytest

from golden_util import GOLDEN, load
from oracle.ref_harness import reference_available

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["pomcp_ucb", "pomcp_pucb_ego1_od1", "pomcp_deep", "ipomcp_pucb_mix", "ipomcp_reinv",
         "potmmcp_ucb_ego1_od2", "mcts_fixed_other"]
H = [f"CooperativeReaching-v0/H{k}-v0" for k in range(1, 6)]


def test_committed_goldens_hold_the_cases_they_are_there_for():
    data = {c: load("coop_reaching/" + c) for c in CASES}
    assert sorted(os.listdir(os.path.join(GOLDEN, "coop_reaching"))) == sorted(c + ".json" for c in CASES)
    returns, lengths = set(), set()
    for c, d in data.items():
        assert d["env"] == "CooperativeReaching-v0" and 2 <= len(d["episodes"]) <= 3, c
        assert d["num_sims"] <= 128 and d["max_steps"] == 50
        for ep in d["episodes"]:
            tr = ep["trace"]
            assert len(ep["records"]) == tr["len"] == len(tr["steps"]) <= 50
            returns.add(float.fromhex(tr["return"]))
            lengths.add(tr["len"])
            assert all(r["num_sims"] == d["num_sims"] for r in ep["records"] if r["searched"])
        assert os.path.getsize(os.path.join(GOLDEN, "coop_reaching", c + ".json")) < 1 << 20
    assert returns == {0.0, 0.75, 1.0} and 50 in lengths
    p = data["pomcp_ucb"]
    assert (p["planner"], p["ego"], p["obs_distance"], p["other_agent"]) == ("POMCP", "0", None, "random")
    assert p["episodes"][0]["config"]["action_selection"] == "ucb"
    p = data["pomcp_pucb_ego1_od1"]
    assert (p["planner"], p["ego"], p["obs_distance"]) == ("POMCP", "1", 1)
    assert p["episodes"][0]["config"]["action_selection"] == "pucb"
    p = data["pomcp_deep"]
    cfg = p["episodes"][0]["config"]
    assert (cfg["discount"], cfg["epsilon"], cfg["action_selection"], p["num_sims"]) == \
        (0.99, 0.01, "ucb", 64)
    assert max(r["search_depth"] for ep in p["episodes"] for r in ep["records"]
               if r["searched"]) >= 20
    for c in ("ipomcp_pucb_mix", "ipomcp_reinv"):
        p = data[c]
        assert p["planner"] == "IPOMCP" and p["obs_distance"] is None
        assert list(p["spec"]["other"]["policies"]) == [H[0], H[1], "o_fixed"]
        assert p["spec"]["other"]["policies"][H[0]] is None and p["spec"]["search"] is None
        assert p["episodes"][0]["config"]["action_selection"] == "pucb"
    assert data["ipomcp_reinv"]["num_sims"] == 48
    assert all(r["belief_size"] >= 100 for ep in data["ipomcp_reinv"]["episodes"]
               for r in ep["records"] if r["searched"])
    p = data["potmmcp_ucb_ego1_od2"]
    assert (p["planner"], p["ego"], p["obs_distance"]) == ("POTMMCP", "1", 2)
    assert list(p["spec"]["other"]) == H == list(p["spec"]["meta"]) and len(p["spec"]["ego"]) == 3
    assert [t["tree"] for t in p["trees"]] == list(range(6))
    assert len({t["records"][0]["belief_digest"] for t in p["trees"]}) > 1
    p = data["mcts_fixed_other"]
    assert p["planner"] == "MCTS" and p["spec"]["other"]["kind"] == "fixed"
    assert p["episodes"][0]["config"]["state_belief_only"] is True


@pytest.mark.skipif(not reference_available(),
                    reason="the reference exists only in the build container")
def test_make_coop_reaching_regenerates_the_committed_fixtures(tmp_path):
    """(about ten seconds; the generator aborts when a case misses its own assertions)"""
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_coop_reaching.py"),
                        f"--out={tmp_path}"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    names = [c + ".json" for c in CASES]
    _, mismatch, errors = filecmp.cmpfiles(os.path.join(GOLDEN, "coop_reaching"), str(tmp_path),
                                           names, shallow=False)
    assert mismatch == [] and errors == []
