"""Belief accuracy statistics without a GPU: the host twin of k_belief_stats
(``pomcp_host_belief_counts``: the classification the kernel uses,
csrc/belief_stats.h) against numpy, the C ABI's argument checks, the
``BeliefStatTracker`` host logic (``posggym_baselines/planning/utils.py:147-339``)
on a scripted planner, the episode harness's unchanged default rows, and the
reference-generated fixture's regeneration."""
import ctypes as C
import filecmp
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import posggym_baselines_amd.planning as P
from posggym_baselines_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "belief_stats", "belief_stats.json")
QUERY = (0x1234ABCD, 0x00C0FFEE)


def host_counts(records, state, num_other):
    lib = N.load()
    rec = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, 4)
    out = N.PomcpBeliefCounts()
    q = None if state is None else (C.c_uint32 * 2)(*state)
    rc = lib.pomcp_host_belief_counts(rec.ctypes.data_as(C.POINTER(C.c_uint32)), len(rec), q,
                                      num_other, C.byref(out))
    return rc, out


def random_records(rng, n, num_other):
    """n records {t, v0, v1, aux}: exact matches of QUERY (with differing t),
    decoys that match in v0 only and in v1 only, the rest random."""
    rec = rng.integers(0, 2**32, size=(n, 4), dtype=np.uint64).astype(np.uint32)
    kind = rng.integers(0, 4, size=n)
    rec[kind == 0, 1], rec[kind == 0, 2] = QUERY
    rec[kind == 1, 1] = QUERY[0]                     # v0 only
    rec[kind == 1, 2] = QUERY[1] ^ 1
    rec[kind == 2, 1] = QUERY[0] ^ 0x80000000        # v1 only
    rec[kind == 2, 2] = QUERY[1]
    rec[:, 3] = rng.integers(0, max(num_other, 1), size=n)
    return rec


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
@pytest.mark.parametrize("num_other", [0, 3, 8])
def test_host_belief_counts_match_numpy(n, num_other):
    rng = np.random.default_rng(1000 * num_other + n)
    rec = random_records(rng, n, num_other)
    if num_other == 0:
        rec[:, 3] = 0xFFFFFFFF   # a plain belief's aux is not read
    rc, out = host_counts(rec, QUERY, num_other)
    assert rc == N.POMCP_OK and out.error == 0
    assert out.belief_size == n
    assert out.state_matches == int(np.sum((rec[:, 1] == QUERY[0]) & (rec[:, 2] == QUERY[1])))
    if n >= 63:   # the decoys are there, and are not counted
        assert np.sum(rec[:, 1] == QUERY[0]) > out.state_matches
        assert np.sum(rec[:, 2] == QUERY[1]) > out.state_matches
    hist = np.bincount(rec[:, 3], minlength=8)[:8] if num_other else np.zeros(8, dtype=int)
    assert list(out.policy_hist) == [int(h) for h in hist]
    # no query state: -1, everything else unchanged
    rc, out2 = host_counts(rec, None, num_other)
    assert rc == N.POMCP_OK and out2.state_matches == -1
    assert out2.belief_size == n and list(out2.policy_hist) == list(out.policy_hist)


def test_host_belief_counts_rejects_an_out_of_range_policy_index():
    rng = np.random.default_rng(7)
    rec = random_records(rng, 200, 3)
    rec[137, 3] = 3            # == num_other
    rec[11, 3] = 0xFFFFFFFF
    rc, out = host_counts(rec, QUERY, 3)
    assert rc == N.POMCP_E_INVALID and out.error == N.POMCP_E_INVALID
    good = np.delete(rec, [11, 137], axis=0)
    assert list(out.policy_hist) == [int(h) for h in np.bincount(good[:, 3], minlength=8)]
    assert out.belief_size == 200
    # bad arguments
    lib = N.load()
    one = (C.c_uint32 * 4)()
    o = N.PomcpBeliefCounts()
    assert lib.pomcp_host_belief_counts(one, 1, None, 0, None) == N.POMCP_E_INVALID
    assert lib.pomcp_host_belief_counts(None, 1, None, 0, C.byref(o)) == N.POMCP_E_INVALID
    assert lib.pomcp_host_belief_counts(one, -1, None, 0, C.byref(o)) == N.POMCP_E_INVALID
    assert lib.pomcp_host_belief_counts(one, 1, None, 9, C.byref(o)) == N.POMCP_E_INVALID


def test_library_exports_belief_stats_and_checks_null_arguments():
    lib = N.load()
    assert hasattr(lib, "pomcp_belief_stats") and hasattr(lib, "pomcp_host_belief_counts")
    out = N.PomcpBeliefCounts()
    assert lib.pomcp_belief_stats(None, None, C.byref(out)) == N.POMCP_E_INVALID
    assert lib.pomcp_belief_stats(None, None, None) == N.POMCP_E_INVALID
    assert C.sizeof(N.PomcpBeliefCounts) == 48 == np.dtype(N.BELIEF_COUNTS_DTYPE).itemsize
    assert lib.pomcp_abi_version() == 7   # no struct changed layout


# ------------------------------------------------------------------ tracker
class _OtherPi(P.OtherAgentPolicy):
    def sample_initial_state(self):
        return {}

    def get_next_state(self, action, obs, state):
        return {}

    def sample_action(self, state):
        return 0

    def get_pi(self, state):
        return {0: 1.0}


class FakePlanner:
    """A planner whose belief_stats returns scripted values and logs its calls."""

    def __init__(self, script, state_belief_only=True, other=None):
        self.model = SimpleNamespace(possible_agents=["0", "1"])
        self.agent_id = "0"
        self.config = SimpleNamespace(state_belief_only=state_belief_only)
        self.other_agent_policies = {"1": other if other is not None else _OtherPi(self.model, "1")}
        self.script = list(script)
        self.calls = []

    def belief_stats(self, state=None, other_policy_ids=None, other_actions=None, *, stats=None):
        self.calls.append(dict(state=state, other_policy_ids=other_policy_ids,
                               other_actions=other_actions, stats=list(stats)))
        vals = self.script.pop(0)
        return {k: vals[k] for k in stats}


def fake_env(max_steps=4):
    return SimpleNamespace(state=(1, 2), last_obs={"0": "o0", "1": "o1"},
                           last_actions={"1": None},
                           policies={"1": SimpleNamespace(policy_id="pi_true")},
                           spec=SimpleNamespace(max_episode_steps=max_steps))


def test_belief_stat_tracker_is_exported_with_the_reference_keys():
    T = P.BeliefStatTracker
    assert T.TRACKABLE_BELIEF_STATS == ["policy", "action", "state", "history"]
    assert T.get_stat_keys(["state", "policy"], False, None) == ["belief_state_acc",
                                                                 "belief_policy_acc"]
    assert T.get_stat_keys(["action"], True, 3) == ["belief_action_acc", "belief_action_acc_0",
                                                    "belief_action_acc_1", "belief_action_acc_2"]
    with pytest.raises(AssertionError):
        T.get_stat_keys(["bogus"], False, None)


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_belief_stat_tracker_host_logic():
    script = [{"state": 0.5, "policy": 1.0, "action": 0.25, "history": 0.0},
              {"state": 0.0, "policy": 0.5, "action": 0.75, "history": 0.0}]
    pl = FakePlanner(script)
    env = fake_env(max_steps=4)
    tr = P.BeliefStatTracker(pl, env, track_per_step=True)
    assert tr.stats_to_track == ["policy", "action", "state", "history"]
    # an empty episode: NaN everywhere
    ep = tr.get_episode()
    assert sorted(ep) == sorted(P.BeliefStatTracker.get_stat_keys(tr.stats_to_track, True, 4))
    assert all(math.isnan(v) for v in ep.values())
    # step 1: the state compared is the one before the action (at reset)
    env.state, env.last_actions, env.last_obs = (3, 4), {"1": 2}, {"0": "p0", "1": "p1"}
    tr.step(env)
    assert len(pl.calls) == 1          # ONE belief_stats call for all four stats
    assert pl.calls[0]["state"] == (1, 2)
    assert pl.calls[0]["other_policy_ids"] == {"1": "pi_true"}
    assert pl.calls[0]["other_actions"] == {"1": 2}
    assert pl.calls[0]["stats"] == ["policy", "action", "state", "history"]
    env.state, env.last_actions = (5, 6), {"1": 0}
    tr.step(env)
    assert len(pl.calls) == 2 and pl.calls[1]["state"] == (3, 4)
    ep = tr.get_episode()
    assert ep["belief_state_acc"] == 0.25 and ep["belief_policy_acc"] == 0.75
    assert ep["belief_action_acc"] == 0.5 and ep["belief_history_acc"] == 0.0
    assert [ep[f"belief_state_acc_{t}"] for t in range(2)] == [0.5, 0.0]
    assert all(math.isnan(ep[f"belief_{k}_acc_{t}"]) for k in tr.stats_to_track for t in (2, 3))
    # reset_episode before the environment's reset asserts
    with pytest.raises(AssertionError):
        tr.reset_episode()
    env.last_actions, env.state = {"1": None}, (7, 8)
    tr.reset_episode()
    assert tr._num_episodes == 1 and tr._current_state == (7, 8)
    assert all(math.isnan(v) for v in tr.get_episode().values())
    tr.reset()
    assert tr._num_episodes == 0
    # a NaN step makes the episode's mean NaN (utils.py:279)
    pl.script = [{"state": float("nan")}]
    tr2 = P.BeliefStatTracker(pl, env, stats_to_track=["state"])
    tr2.step(env)
    assert math.isnan(tr2.get_episode()["belief_state_acc"])
    assert list(tr2.get_episode()) == ["belief_state_acc"]
    # the single-stat methods
    pl.script = [{"state": 0.125}, {"policy": 0.5}, {"action": 0.75}, {"history": 0.0}]
    assert tr.get_state_accuracy((9, 9)) == 0.125 and pl.calls[-1]["state"] == (9, 9)
    assert tr.get_other_policy_accuracy({"1": SimpleNamespace(policy_id="x")}) == 0.5
    assert pl.calls[-1]["other_policy_ids"] == {"1": "x"}
    assert tr.get_other_action_accuracy({"1": 3}) == 0.75
    assert pl.calls[-1]["other_actions"] == {"1": 3}
    assert tr.get_other_history_accuracy({}) == 0.0


def test_belief_stat_tracker_rejects_what_has_no_parity_target():
    env = fake_env()
    with pytest.raises(NotImplementedError):   # histories are not on the GPU
        P.BeliefStatTracker(FakePlanner([], state_belief_only=False), env)
    P.BeliefStatTracker(FakePlanner([], state_belief_only=False), env,
                        stats_to_track=["state", "policy", "action"])

    class FakeINTMCP(P.INTMCP):
        def __init__(self):
            self.config = SimpleNamespace(state_belief_only=True)

        def __del__(self):
            pass

    with pytest.raises(NotImplementedError):
        P.BeliefStatTracker(FakeINTMCP(), env, stats_to_track=["state"])
    # policy / action need OtherAgentPolicy instances, as in the reference
    with pytest.raises(AssertionError):
        P.BeliefStatTracker(FakePlanner([], other=object()), env, stats_to_track=["policy"])
    P.BeliefStatTracker(FakePlanner([], other=object()), env, stats_to_track=["state"])
    with pytest.raises(AssertionError):
        P.BeliefStatTracker(FakePlanner([]), env, stats_to_track=["bogus"])


# ------------------------------------------------------------------ harness
class _ScriptedPlanner:
    """A planner stand-in for the episode harness: plays action 0."""

    def __init__(self):
        self.config = SimpleNamespace(discount=0.95)
        self.stat_tracker = P.PlanningStatTracker(self)
        self.step_statistics = {}
        self.resets = 0

    def reset(self):
        self.resets += 1
        self.stat_tracker.reset_episode()

    def step(self, obs):
        self.stat_tracker.step()
        return 0


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_episode_harness_default_rows_are_unchanged_and_tracker_columns_join(tmp_path):
    from posggym_baselines_amd.envs import DrivingModel
    from posggym_baselines_amd.planning.episodes import EPISODE_RESULT_HEADS
    model = DrivingModel()
    rows = P.run_planning_episodes(_ScriptedPlanner(), model, 1, "0", env_seeds=[3])
    assert list(rows[0]) == EPISODE_RESULT_HEADS
    # with a tracker: its columns join, the rest of the row is the same
    pl = _ScriptedPlanner()
    fp = FakePlanner([{"state": 0.5}] * 200)
    view = P.EpisodeEnvView(model, "0")
    tr = P.BeliefStatTracker(fp, view, stats_to_track=["state"])
    seen = []
    rows2 = P.run_planning_episodes(pl, model, 1, "0", env_seeds=[3], belief_tracker=tr,
                                    on_step=lambda t, obs, acts, ts: seen.append((acts, ts.state)))
    assert list(rows2[0]) == EPISODE_RESULT_HEADS + ["belief_state_acc"]
    assert rows2[0]["belief_state_acc"] == 0.5
    for k in ("num", "len", "return", "discounted_return"):
        assert rows2[0][k] == rows[0][k]
    assert len(fp.calls) == rows2[0]["len"] == len(seen)
    # the state compared at step t is the one before step t's actions
    assert fp.calls[1]["state"] == seen[0][1]
    assert view.last_actions == {"1": seen[-1][0]["1"]} and view.state == seen[-1][1]
    # the csv writer: today's header by default, extra columns on request
    a, b = tmp_path / "a.csv", tmp_path / "b.csv"
    P.EpisodeResultsWriter(str(a))(rows[0])
    P.EpisodeResultsWriter(str(b), extra_heads=["belief_state_acc"])(rows2[0])
    assert a.read_text().splitlines()[0] == ",".join(EPISODE_RESULT_HEADS)
    assert b.read_text().splitlines()[0] == ",".join(EPISODE_RESULT_HEADS + ["belief_state_acc"])


# ------------------------------------------------------------------ fixture
def test_belief_stats_fixture_holds_the_conditions_the_gpu_test_relies_on():
    import json
    with open(FIXTURE) as f:
        cases = {c["case"]: c for c in json.load(f)["cases"]}
    assert set(cases) >= {"c1_ucb", "mcts_fixed_other_pucb", "mcts_ipomcp_mix_pucb",
                          "mcts_pe_mix_pucb", "potmmcp_ucb_ego1"}

    def col(case, k):
        return [float.fromhex(s[f"{k}_acc"]) for s in cases[case]["steps"]]

    def between(v):
        return 0.0 < v < 1.0

    assert sum(map(between, col("c1_ucb", "state"))) >= 1
    assert sum(map(between, col("mcts_fixed_other_pucb", "state"))) >= 1
    mix = zip(col("mcts_ipomcp_mix_pucb", "policy"), col("mcts_ipomcp_mix_pucb", "action"))
    assert sum(between(p) and between(a) for p, a in mix) >= 5
    assert sum(map(between, col("mcts_pe_mix_pucb", "state"))) >= 1
    assert 1.0 in col("mcts_pe_mix_pucb", "policy")
    pot = zip(col("potmmcp_ucb_ego1", "policy"), col("potmmcp_ucb_ego1", "action"))
    assert sum(between(p) and between(a) for p, a in pot) >= 5
    assert [len(cases[c]["steps"]) for c in ("c1_ucb", "mcts_fixed_other_pucb",
                                             "mcts_ipomcp_mix_pucb", "mcts_pe_mix_pucb")] == \
        [50, 3, 22, 100]


@pytest.mark.skipif(not os.path.isdir("/root/reference/posggym_baselines"),
                    reason="the reference exists only in the build container")
def test_make_belief_stats_regenerates_committed_fixture(tmp_path):
    out = tmp_path / "belief_stats.json"
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_belief_stats.py"), str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert filecmp.cmp(FIXTURE, str(out), shallow=False)
