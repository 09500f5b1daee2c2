"""tests/golden/reactive/*.json are what tests/golden/make_reactive.py writes:
where the reference planner is present every case is regenerated (the
generator's own assertions run again) and compared byte for byte."""
import importlib.util
import os

import pytest

from oracle.ref_harness import reference_available

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["ipomcp_pucb", "ipomcp_deep_ego1", "ipomcp_reinv", "potmmcp"]


def generator():
    spec = importlib.util.spec_from_file_location(
        "make_reactive", os.path.join(HERE, "golden", "make_reactive.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_fixture_set_is_the_generators_and_small():
    gen = generator()
    assert list(gen.CASES) == CASES
    names = sorted(os.listdir(gen.OUT_DIR))
    assert names == sorted(c + ".json" for c in CASES)
    for n in names:
        assert os.path.getsize(os.path.join(gen.OUT_DIR, n)) < 200 * 1024, n


@pytest.mark.skipif(not reference_available(), reason="the reference planner is not present")
@pytest.mark.parametrize("case", CASES)
def test_fixtures_regenerate_byte_for_byte(case):
    gen = generator()
    data, facts = gen.run_case(case)
    assert facts["two_policies_at_step_3"] > 0 and facts["reactive_actions_differ"] > 0
    if case == "ipomcp_reinv":
        assert facts["reinv_accepted_reactive"] > 0
    with open(os.path.join(gen.OUT_DIR, case + ".json"), "rb") as f:
        assert f.read() == gen.dumps(data).encode()
