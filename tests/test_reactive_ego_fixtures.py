"""The reactive-ego goldens (tests/golden/reactive_ego): what the
committed files hold -- the state-form invariant's count and the facts each
case is there for, as the generator recorded them -- and, where the reference
is available, that tests/golden/make_reactive_ego.py reproduces them byte for
byte from the real reference planners."""
import filecmp
import json
import os
import subprocess
import sys

import pytest

from golden_util import GOLDEN, load
from oracle.ref_harness import reference_available

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["potmmcp_p0_softmax", "potmmcp_p0_greedy_deep", "potmmcp_mixed", "potmmcp_mixed_uniform",
         "potmmcp_myopic",
         "potmmcp_starved", "pomcp_h3_pucb", "ipomcp_h2_mix"]
H = [f"CooperativeReaching-v0/H{k}-v0" for k in range(1, 6)]


def test_p0_meta_policy_fixture_keeps_the_rows_and_their_order():
    with open(os.path.join(GOLDEN, "reactive_ego", "p0_meta_policy.json")) as f:
        mp = json.load(f)["meta_policy"]
    assert list(mp) == ["greedy", "softmax", "uniform"]
    for name, rows in mp.items():
        assert list(rows) == H
        for row in rows.values():
            assert list(row) == H and abs(sum(row.values()) - 1.0) < 1e-6
    assert mp["greedy"][H[1]][H[0]] == 1.0 and mp["softmax"][H[0]][H[3]] == 0.3146054830262828


def test_committed_goldens_hold_the_cases_they_are_there_for():
    data = {c: load("reactive_ego/" + c) for c in CASES}
    assert sorted(os.listdir(os.path.join(GOLDEN, "reactive_ego"))) == \
        sorted([c + ".json" for c in CASES] + ["p0_meta_policy.json"])
    for c, d in data.items():
        assert d["env"] == "CooperativeReaching-v0" and len(d["episodes"]) == 2, c
        assert d["num_sims"] <= 128 and d["size"] in (4, 5)
        assert os.path.getsize(os.path.join(GOLDEN, "reactive_ego", c + ".json")) < 32 << 10
        # the CPU proof the kernel's design rests on: every comparison agreed
        # (one mismatch aborts the generator)
        assert d["facts"]["invariant_checks"] > 1000, c
        for ep in d["episodes"]:
            assert len(ep["records"]) == ep["trace"]["len"] <= 50
    f = {c: d["facts"] for c, d in data.items()}
    for c in ("potmmcp_p0_softmax", "potmmcp_mixed"):
        assert f[c]["searches_with_two_ego_policies"] > 0 and f[c]["ema_moved_below_root"] > 0
    assert f["potmmcp_p0_greedy_deep"]["ema_moved_below_root"] > 0
    assert f["potmmcp_starved"]["code0_root_at_t>0_differs"] > 0
    assert f["potmmcp_myopic"]["unexpanded_child_became_root"] > 0
    p = data["potmmcp_p0_softmax"]
    assert p["spec"]["meta"] == "P0:softmax" and list(p["spec"]["ego"]) == H == list(p["spec"]["other"])
    assert p["episodes"][0]["config"]["action_selection"] == "pucb"
    p = data["potmmcp_p0_greedy_deep"]
    cfg = p["episodes"][0]["config"]
    assert (cfg["discount"], cfg["epsilon"], cfg["action_selection"]) == (0.99, 0.01, "ucb")
    assert max(r["search_depth"] for ep in p["episodes"] for r in ep["records"] if r["searched"]) >= 2   # (and rollouts to the end: depth_limit 459)
    p = data["potmmcp_mixed"]
    assert (p["ego"], p["obs_distance"]) == ("1", 1) and [t["tree"] for t in p["trees"]] == list(range(6))
    assert [v is None for v in p["spec"]["ego"].values()] == [True, False, True]
    # a moving average that leaves {0, 1}
    assert any(float.fromhex(x) not in (0.0, 1.0) for ep in p["episodes"] for r in ep["records"]
               if r["searched"] for x in r["prior"])
    assert data["potmmcp_starved"]["num_sims"] == 6
    assert data["potmmcp_myopic"]["episodes"][0]["config"]["discount"] == 0.0
    p = data["pomcp_h3_pucb"]
    assert (p["planner"], p["spec"]["search"]) == ("POMCP", H[2])
    # the base planner's prior: one-hot on the heuristic's action at the root
    assert all(sorted(float.fromhex(x) for x in r["prior"]) == [0.0] * 4 + [1.0]
               for ep in p["episodes"] for r in ep["records"] if r["searched"])
    p = data["ipomcp_h2_mix"]
    assert (p["planner"], p["spec"]["search"]) == ("IPOMCP", H[1])
    sizes = [r["belief_size"] for ep in p["episodes"] for r in ep["records"] if r["searched"]]
    assert min(sizes) == 107 and sizes.count(107) >= len(sizes) - 2      # re-roots reinvigorate


@pytest.mark.skipif(not reference_available(),
                    reason="the reference exists only in the build container")
def test_make_reactive_ego_regenerates_the_committed_fixtures(tmp_path):
    """(a few seconds; the generator aborts when a case misses its own assertions
    or the state-form invariant)"""
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_reactive_ego.py"),
                        f"--out={tmp_path}"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    names = [c + ".json" for c in CASES]
    _, mismatch, errors = filecmp.cmpfiles(os.path.join(GOLDEN, "reactive_ego"), str(tmp_path),
                                           names, shallow=False)
    assert mismatch == [] and errors == []
