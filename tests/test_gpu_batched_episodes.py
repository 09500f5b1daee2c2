"""BatchedPOMCP.run_episodes: one episode per tree played on the device
(pomcp_episodes_begin / pomcp_episodes_step, k_episode_reset / k_episode_step)
against the oracle's serial episodes and the reference goldens, bit for bit,
on every search kernel; finished trees parked inside a live batch."""
import csv
import functools
import math

import numpy as np
import pytest

from golden_util import case_env, case_max_steps, cfg_kwargs, load
from gpu_util import product_config, product_model, stats_record
from oracle.episode import fhex
from oracle.run import oracle_episode

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["lane", "lane_eager", "wave", "wave_tree", "wave_plain"])
def search_kernel(request, monkeypatch):
    """Every test runs on every search kernel and mode, as tests/test_gpu_parity.py
    selects them: k_search with cut-off children deferred ("lane") or looked up
    ("lane_eager"), k_search_lds as the engine picks its step-tree producers
    ("wave"), with them forced on ("wave_tree") and off ("wave_plain")."""
    kind, _, mode = request.param.partition("_")
    monkeypatch.setenv("POMCP_SEARCH_KERNEL", kind)
    if kind == "lane":
        monkeypatch.setenv("POMCP_DEFER_CUTOFF", "0" if mode == "eager" else "1")
    elif mode:
        monkeypatch.setenv("POMCP_STEP_TREE", "1" if mode == "tree" else "0")
    return kind


# the configuration of tests/test_gpu_parity.py (TEST_CFG)
TEST_CFG = dict(discount=0.95, search_time_limit=0.1, c=math.sqrt(2), truncated=False,
                action_selection="ucb", pucb_exploration_fraction=0.25, known_bounds=None,
                step_limit=None, epsilon=0.92, seed=0, state_belief_only=True)
S = 32


@functools.lru_cache(maxsize=None)
def oracle_batch(env, first_seed, count, max_steps):
    """Tree b = oracle tree b, env seed first_seed + b; computed once for all modes."""
    return [oracle_episode(TEST_CFG, S, first_seed + b, ego="0", tree=b, max_steps=max_steps,
                           env=env) for b in range(count)]


class Recorder:
    """on_step callback: per tree the (ego action, other action, reward bits) of
    every step it played, from the debug getter."""

    def __init__(self, B):
        self.steps = [[] for _ in range(B)]
        self.lens = np.zeros(B, dtype=np.int64)

    def __call__(self, t, bp):
        st = bp.episode_states()
        for b in np.nonzero(st["res"]["len"] > self.lens)[0]:
            self.steps[b].append((int(st["last_action"][b]), int(st["last_other_action"][b]),
                                  fhex(st["last_reward"][b])))
        self.lens = st["res"]["len"].astype(np.int64)


def expected_planner_columns(records):
    """The row's planner columns from the oracle's records of the steps that
    reach PlanningStatTracker (searched): integer sums / n, sequential FP64
    sums / n.  A searched step without a simulation (the update made the root
    absorbing, mcts.py:270-272) reports depth 0, 0 simulations and the
    MinMaxStats as the last search left them."""
    n = depth = sims = 0
    mn_sum = mx_sum = 0.0
    mn, mx = math.inf, -math.inf
    for r in records:
        if not r["searched"]:
            continue
        if r.get("num_sims", 0) > 0:
            mn, mx = float.fromhex(r["min_value"]), float.fromhex(r["max_value"])
        n += 1
        depth += r.get("search_depth", 0)
        sims += r.get("num_sims", 0)
        mn_sum += mn
        mx_sum += mx
    return n, depth / n, sims / n, mn_sum / n, mx_sum / n


def check_row(row, b, seed, steps, records, gamma):
    assert (row["num"], row["env_seed"], row["len"]) == (b, seed, len(steps))
    ret = disc = 0.0
    for t, s in enumerate(steps):
        r = float.fromhex(s["reward"])
        ret += r
        disc += gamma ** t * r
    assert fhex(row["return"]) == fhex(ret)
    assert fhex(row["discounted_return"]) == fhex(disc)
    n, depth, sims, mn, mx = expected_planner_columns(records[:len(steps)])
    assert (row["search_depth"], row["num_sims"]) == (depth, sims)
    assert (fhex(row["min_value"]), fhex(row["max_value"])) == (fhex(mn), fhex(mx))
    for k in ("reinvigoration_time", "evaluation_time", "policy_calls", "inference_time"):
        assert row[k] == 0.0
    assert row["time"] > 0 and row["search_time"] > 0 and row["update_time"] > 0
    assert row["mem_usage"] > 0
    return n


def test_driving_all_done_equals_oracle_and_parks_finished_trees(tmp_path):
    """70 trees (two search waves and two shared logs, one of them with 6
    trees), env seeds 3000..3069, until all_done: every row and every ego action
    equal the oracle's serial episode; a tree that finished early keeps the
    root statistics of its last search through its neighbours' later steps."""
    from posggym_baselines_amd.planning import BatchedPOMCP
    from posggym_baselines_amd.planning.episodes import EPISODE_RESULT_HEADS, EpisodeResultsWriter
    B, first, max_steps = 70, 3000, 50
    exp = oracle_batch("Driving-v1", first, B, max_steps)
    model = product_model("Driving-v1")
    bp = BatchedPOMCP(model, "0", product_config(TEST_CFG, S), B, S, searches=max_steps, reroot=True)
    rec = Recorder(B)
    writer = EpisodeResultsWriter(str(tmp_path / "episode_results.csv"), extra_heads=["env_seed"])
    rows = bp.run_episodes(range(first, first + B), until="all_done", on_step=rec, write_row=writer)
    assert len(rows) == B and all(set(r) == set(EPISODE_RESULT_HEADS) | {"env_seed"} for r in rows)
    with open(tmp_path / "episode_results.csv") as f:
        lines = list(csv.DictReader(f))
    assert len(lines) == B and [int(r["len"]) for r in lines] == [r["len"] for r in rows]
    res = bp.engine.episodes_results()
    stats = bp.engine.root_stats()
    parked_early = tail_absorbing = 0
    for b, (trace, records) in enumerate(exp):
        steps = trace["steps"]
        n = check_row(rows[b], b, first + b, steps, records, TEST_CFG["discount"])
        assert fhex(rows[b]["return"]) == trace["return"]
        assert int(res[b]["searched_steps"]) == n == sum(r["searched"] for r in records)
        assert [s[0] for s in rec.steps[b]] == [s["actions"][0] for s in steps], b
        assert [s[1] for s in rec.steps[b]] == [s["actions"][1] for s in steps], b
        assert [s[2] for s in rec.steps[b]] == [s["reward"] for s in steps], b
        assert int(res[b]["truncated"]) == (1 if len(steps) == max_steps else 0)
        # parking: the root statistics are those of the tree's last real search
        real = [r for r in records if r["searched"] and r.get("num_sims", 0) > 0]
        last = real[-1]
        if len(real) == len(records):
            # searched to its last step: the root and its belief are that step's
            got = stats_record(stats[b], 5, True, last["action"], bp.engine.root_belief(b))
            assert got == last, b
            parked_early += len(steps) < max_steps - 10
        else:
            # the ego finished first: the root moved on to an absorbing node (its
            # belief is that node's), the statistics kept are the last search's
            got = stats_record(stats[b], 5, True, last["action"], [])
            for k in ("belief_size", "belief_digest"):
                got.pop(k)
            assert got == {k: v for k, v in last.items() if not k.startswith("belief_")}, b
            tail_absorbing += 1
        assert int(stats[b].action) == last["action"]
    # trees parked for tens of steps while their wave's neighbours played on
    assert parked_early >= 1 and tail_absorbing >= 1
    assert max(r["len"] for r in rows) == max_steps
    bp.close()


@pytest.mark.parametrize("until", ["all_done", "agent_done"])
def test_pursuit_evasion_equals_oracle(until):
    """24 PursuitEvasion-v1 trees, env seeds 2000..2023, evader ego.  agent_done
    ends an episode at the first step that terminates the ego, found by
    replaying the oracle trace's joint actions through the product's host
    model; the row is the oracle episode's prefix up to there."""
    from posggym_baselines_amd.planning import BatchedPOMCP
    B, first, max_steps = 24, 2000, 100
    env = "PursuitEvasion-v1"
    exp = oracle_batch(env, first, B, max_steps)
    bp = BatchedPOMCP(product_model(env), "0", product_config(TEST_CFG, S), B, S,
                      searches=max_steps, reroot=True)
    rec = Recorder(B)
    rows = bp.run_episodes(range(first, first + B), until=until, on_step=rec)
    host = product_model(env)
    lens = []
    for b, (trace, records) in enumerate(exp):
        steps = trace["steps"]
        n = len(steps)
        if until == "agent_done":
            host.seed(first + b)
            state = host.sample_initial_state()
            for t, s in enumerate(steps):
                ts = host.step(state, {str(i): a for i, a in enumerate(s["actions"])})
                state = ts.state
                if ts.terminations["0"] or ts.all_done:
                    n = t + 1
                    break
        check_row(rows[b], b, first + b, steps[:n], records, TEST_CFG["discount"])
        assert [s[:2] for s in rec.steps[b]] == [tuple(s["actions"]) for s in steps[:n]], b
        assert [s[2] for s in rec.steps[b]] == [s["reward"] for s in steps[:n]], b
        lens.append(n)
    assert min(lens) < max(lens)   # episodes of different lengths shared the batch
    bp.close()


@pytest.mark.parametrize("case", ["c1_ucb", "pe_evader_ucb"])
def test_reference_goldens_through_one_tree(case):
    """The reference planner's golden episodes through run_episodes on one
    tree: actions of both agents, reward bits, length and return (the batched
    twin of test_episode_harness_replays_reference_episodes)."""
    from posggym_baselines_amd.planning import BatchedPOMCP
    data = load(case)
    env, ego = case_env(data), data["ego"]
    max_steps = case_max_steps(case, data)
    for ep in data["episodes"]:
        steps = ep["trace"]["steps"]
        bp = BatchedPOMCP(product_model(env), ego, product_config(cfg_kwargs(ep["config"]),
                                                                  data["num_sims"]),
                          1, data["num_sims"], searches=max_steps, reroot=True)
        rec = Recorder(1)
        rows = bp.run_episodes([ep["env_seed"]], until="all_done", on_step=rec)
        bp.close()
        e = int(ego)
        assert rows[0]["len"] == ep["trace"]["len"] == len(rec.steps[0])
        assert [(s[0], s[1]) for s in rec.steps[0]] == \
            [(s["actions"][e], s["actions"][1 - e]) for s in steps], case
        assert [s[2] for s in rec.steps[0]] == [s["reward"] for s in steps], case
        assert fhex(rows[0]["return"]) == ep["trace"]["return"]
        assert rows[0]["env_seed"] == ep["env_seed"]


def test_belief_states_on_the_device_equal_the_host_replay():
    """belief_states=True: after each of the first 5 steps, the belief counts
    against the true states the kernels wrote equal the counts against the
    states of a host replay of the same joint actions (the state before the
    step's joint action: the one the root belief is about)."""
    from posggym_baselines_amd.planning import BatchedPOMCP
    B, first, K = 8, 3000, 5
    bp = BatchedPOMCP(product_model("Driving-v1"), "0", product_config(TEST_CFG, S), B, S,
                      searches=50, reroot=True)
    hosts = []
    for b in range(B):
        m = product_model("Driving-v1")
        m.seed(first + b)
        hosts.append([m, m.sample_initial_state()])
    rec = Recorder(B)
    matches = []

    def on_step(t, bp_):
        rec(t, bp_)
        if t >= K:
            return
        assert all(len(s) == t + 1 for s in rec.steps)   # (every episode here lasts > 5 steps)
        before = [h[1] for h in hosts]
        dev = bp_.episode_belief_counts()
        ref = bp_.belief_counts(before)
        assert dev.tobytes() == ref.tobytes(), t
        matches.append(int(dev["state_matches"].sum()))
        assert (dev["belief_size"] > 0).all()
        for b, h in enumerate(hosts):
            a_ego, a_oth, _ = rec.steps[b][t]
            h[1] = h[0].step(h[1], {"0": a_ego, "1": a_oth}).state
        st = bp_.episode_states()
        assert [(int(s["v0"]), int(s["v1"])) for s in st] == [h[1] for h in hosts]

    bp.run_episodes(range(first, first + B), until="all_done", belief_states=True, on_step=on_step)
    assert len(matches) == K and sum(matches) > 0
    bp.close()


def test_run_episodes_refuses_an_engine_sized_for_one_search():
    from posggym_baselines_amd._native import PomcpError
    from posggym_baselines_amd.planning import BatchedPOMCP
    bp = BatchedPOMCP(product_model("Driving-v1"), "0", product_config(TEST_CFG, S), 4, S,
                      searches=1, reroot=False)
    with pytest.raises(ValueError, match="searches=50, reroot=True"):
        bp.run_episodes()
    with pytest.raises(PomcpError):   # nothing was launched: no batch of episodes exists
        bp.episode_states()
    bp.close()
    bp = BatchedPOMCP(product_model("Driving-v1"), "0", product_config(TEST_CFG, S), 4, S,
                      searches=50, reroot=True)
    with pytest.raises(ValueError, match="env_seeds"):
        bp.run_episodes([1, 2, 3])
    with pytest.raises(ValueError, match="until"):
        bp.run_episodes(until="never")
    bp.close()
