"""The reinvigoration goldens (tests/golden/reinv_*.json, make_golden.py CASES)
hold the path classes they were chosen for (no GPU).

The fixtures are the REAL reference planner's records; the oracle replays them
here with its recorder on (``OraclePOMCP.reinvigorations``: need, tries,
accepted, rejected_total, parent_size per call), so a later regeneration with
other seeds cannot quietly lose the paths k_update's parity on these fixtures
(tests/test_gpu_parity.py test_gpu_matches_reference_goldens) is there to pin:
more than one 64-try pass ending at the try limit, more rejected particles
filled in than one 64-lane copy pass holds, and more rejected particles than
the ``need`` kept."""
import math

from golden_util import REINVIGORATION_CASES, case_env, case_max_steps, cfg_kwargs, load
from oracle.episode import run_episode
from oracle.run import make_oracle, oracle_record


def _replay(case):
    """Every (need, tries, accepted, rejected_total, parent_size, limit) of the
    case's episodes; the replayed records equal the fixture's."""
    data = load(case)
    calls = []
    for ep in data["episodes"]:
        kw = cfg_kwargs(ep["config"])
        p = make_oracle(kw, data["num_sims"], ego=data["ego"], env=case_env(data))
        records = []

        def step(obs):
            searched = not p.on_abs[p.root]
            a = p.step(obs)
            records.append(oracle_record(p, searched, a))
            return a

        trace = run_episode(step, ep["env_seed"], ego=data["ego"],
                            max_steps=case_max_steps(case, data), env=case_env(data))
        assert trace == ep["trace"] and records == ep["records"], case
        f = kw["reinvigoration_sample_limit_factor"]
        calls += [c + (f * c[0],) for c in p.reinvigorations]
    return calls


def test_reinvigoration_fixtures_hold_their_path_classes():
    calls = {case: _replay(case) for case in REINVIGORATION_CASES}
    every = [c for v in calls.values() for c in v]
    assert all(len(v) >= 6 for v in calls.values())
    # the try limit hit (the loop ends on tries >= limit, not on need) after
    # more than one 64-try pass; the limit need not be an integer
    hit = [c for c in every if c[2] < c[0] and c[1] > 64]
    assert hit and all(c[1] == math.ceil(c[5]) for c in hit), hit
    assert any(c[5] != int(c[5]) for c in hit)
    # the rejected-fill copy runs more than one 64-lane pass
    assert any(c[0] - c[2] > 64 for c in every)
    # more rejected particles than are kept (the cap at `need`)
    assert any(c[2] < c[0] and c[3] > c[0] for c in every)
    # each case hits its limit at least once, at its own factor
    for case, v in calls.items():
        assert any(c[2] < c[0] for c in v), case
    # and the plain end stays covered next to it: all accepted in more than one pass
    assert any(c[0] == c[2] > 64 for c in every)
