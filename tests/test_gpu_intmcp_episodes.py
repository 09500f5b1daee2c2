"""BatchedINTMCP.run_episodes: one episode per planner pair played on the device
(intmcp_episodes_begin / intmcp_episodes_step, k_im_episode_reset /
k_im_episode_step / k_im_episode_unpark) against the oracle's serial I-NTMCP
episodes, the serial harness and the reference goldens, bit for bit; finished
pairs parked inside a live batch and restored when it ends."""
import functools

import numpy as np
import pytest

from golden_util import cfg_kwargs, load
from gpu_util import intmcp_state_record, product_config, product_model
from oracle.episode import fhex
from oracle.run import oracle_intmcp_episode
from test_gpu_batched_episodes import Recorder, check_row
from test_gpu_intmcp import TEST_CFG

pytestmark = pytest.mark.gpu

S = 8   # simulations per level
EGO = "0"


@functools.lru_cache(maxsize=None)
def oracle_batch(env, first_seed, pairs, max_steps, nesting_level=1):
    """{pair b: the oracle planner with tree key b on env seed first_seed + b}."""
    return {b: oracle_intmcp_episode(TEST_CFG, S, first_seed + b, ego=EGO, tree=b,
                                     max_steps=max_steps, env=env, nesting_level=nesting_level)
            for b in pairs}


def engine(env, B, searches, nesting_level=1):
    from posggym_baselines_amd.planning import BatchedINTMCP
    return BatchedINTMCP(product_model(env), EGO, product_config(TEST_CFG, S), B, S,
                         searches=searches, nesting_level=nesting_level)


class StateRecorder(Recorder):
    """Also every pair's whole 120 B record after every step."""

    def __init__(self, B):
        super().__init__(B)
        self.records = []

    def __call__(self, t, bp):
        super().__call__(t, bp)
        self.records.append(bp.episode_states().copy())


def check_pair(row, rec_steps, b, seed, trace, records, n=None):
    """A pair's row and recorded steps against the oracle episode (its first n steps)."""
    steps = trace["steps"][:n]
    searched = check_row(row, b, seed, steps, records, TEST_CFG["discount"])
    assert [s[:2] for s in rec_steps] == [tuple(s["actions"]) for s in steps], b
    assert [s[2] for s in rec_steps] == [s["reward"] for s in steps], b
    return searched


@pytest.mark.timeout(300)
def test_driving_all_done_equals_oracle_parks_and_restores_finished_pairs():
    """70 pairs (two search workgroups, the second with 6 pairs; a partial
    256-lane step workgroup), env seeds 3000..3069, until all_done."""
    from posggym_baselines_amd.planning.episodes import EPISODE_RESULT_HEADS
    B, first, max_steps = 70, 3000, 50
    exp = oracle_batch("Driving-v1", first, tuple(range(B)), max_steps)
    bp = engine("Driving-v1", B, max_steps)
    rec = StateRecorder(B)
    during = {}

    def on_step(t, bp_):
        rec(t, bp_)
        if t == max_steps - 1:   # the last step of the batch: parked pairs read absorbing
            during["stats"] = [(s.root_absorbing, s.action, s.num_sims) for s in bp_.engine.root_stats()]

    rows = bp.run_episodes(range(first, first + B), until="all_done", on_step=on_step)
    assert len(rows) == B and all(list(r) == EPISODE_RESULT_HEADS + ["env_seed"] for r in rows)
    res = bp.engine.episodes_results()
    final = bp.episode_states()
    assert not res["error"].any()
    lens = [r["len"] for r in rows]
    tail = early = 0
    for b in range(B):
        trace, records = exp[b]
        steps = trace["steps"]
        n = check_pair(rows[b], rec.steps[b], b, first + b, trace, records)
        assert fhex(rows[b]["return"]) == trace["return"]
        assert int(res[b]["searched_steps"]) == n == sum(r["searched"] for r in records)
        assert int(res[b]["truncated"]) == (1 if len(steps) == max_steps else 0)
        # the unpark: the device state of the pair is its last step's
        last = records[len(steps) - 1]
        assert intmcp_state_record(bp.engine, b, last["searched"], steps[-1]["actions"][0]) == last, b
        # the park: the pair's record stayed as its last step left it
        assert rec.records[len(steps) - 1][b].tobytes() == final[b].tobytes(), b
        assert all(r[b].tobytes() == final[b].tobytes() for r in rec.records[len(steps):]), b
        if len(steps) < len(rec.records):
            assert during["stats"][b] == (1, 0, 0), b
        tail += not last["searched"]
        early += len(steps) < max_steps - 10 and all(r["searched"] for r in records)
    # the oracle alone: lengths 5..50, 54 pairs with an absorbing tail, 15 parked
    # for more than 10 steps after a searched last step
    assert tail >= 1 and early >= 1 and max(lens) == max_steps and len(set(lens)) > 2
    assert len(rec.records) == max_steps
    # results again: the unpark is idempotent, and the batch has ended
    stats = [(s.root_absorbing, s.action, s.num_sims, s.root_visits) for s in bp.engine.root_stats()]
    assert bp.engine.episodes_results().tobytes() == res.tobytes()
    assert [(s.root_absorbing, s.action, s.num_sims, s.root_visits)
            for s in bp.engine.root_stats()] == stats
    from posggym_baselines_amd._native import PomcpError
    with pytest.raises(PomcpError, match="ended the batch"):
        bp.engine.episodes_step(S)
    bp.close()


PE_B, PE_FIRST, PE_STEPS = 24, 2000, 100


@functools.lru_cache(maxsize=None)
def pe_rows(until):
    """(rows, recorded steps) of the PursuitEvasion batch; shared with the population test."""
    bp = engine("PursuitEvasion-v1", PE_B, PE_STEPS)
    rec = Recorder(PE_B)
    rows = bp.run_episodes(range(PE_FIRST, PE_FIRST + PE_B), until=until, on_step=rec)
    bp.close()
    return rows, rec.steps


def agent_done_length(host, seed, steps):
    """The first step that terminates the ego, by replaying the joint actions
    through the product's host model."""
    host.seed(seed)
    state = host.sample_initial_state()
    for t, s in enumerate(steps):
        ts = host.step(state, {str(i): a for i, a in enumerate(s["actions"])})
        state = ts.state
        if ts.terminations[EGO] or ts.all_done:
            return t + 1
    return len(steps)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("until", ["all_done", "agent_done"])
def test_pursuit_evasion_equals_oracle(until):
    """24 PursuitEvasion-v1 pairs, env seeds 2000..2023, 100 steps; agent_done
    rows are the oracle episode's prefix up to the ego's termination."""
    env = "PursuitEvasion-v1"
    exp = oracle_batch(env, PE_FIRST, tuple(range(PE_B)), PE_STEPS)
    rows, rec_steps = pe_rows(until)
    host = product_model(env)
    lens = []
    for b in range(PE_B):
        trace, records = exp[b]
        n = len(trace["steps"])
        if until == "agent_done":
            n = agent_done_length(host, PE_FIRST + b, trace["steps"])
        check_pair(rows[b], rec_steps[b], b, PE_FIRST + b, trace, records, n)
        lens.append(n)
    assert min(lens) < max(lens)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("nesting,first", [(2, 5000), (0, 5000)])
def test_other_nesting_levels_equal_oracle(nesting, first):
    """8 Driving pairs at nesting level 2 (k_im_updateN / k_im_searchN, three
    trees) and 0 (the planner's root is tree 1's)."""
    B, max_steps = 8, 50
    exp = oracle_batch("Driving-v1", first, tuple(range(B)), max_steps, nesting)
    bp = engine("Driving-v1", B, max_steps, nesting)
    rec = Recorder(B)
    rows = bp.run_episodes(range(first, first + B), until="all_done", on_step=rec)
    for b in range(B):
        trace, records = exp[b]
        check_pair(rows[b], rec.steps[b], b, first + b, trace, records)
        last = records[len(trace["steps"]) - 1]
        assert intmcp_state_record(bp.engine, b, last["searched"],
                                   trace["steps"][-1]["actions"][0]) == last, b
    lens = [r["len"] for r in rows]
    assert min(lens) < max(lens)
    bp.close()


# Of the oracle's 1,030 three-step episodes (tree b, env seed 7000 + b), these two
# end after 2 steps (a crash: reward -1 for both vehicles); every other one is
# truncated at 3.  (From the oracle alone, on all 1,030 pairs: 14 s on a CPU,
# so the test runs it on the pairs below only.)
SHORT_OF_1030 = (65, 817)


@pytest.mark.timeout(300)
def test_1030_pairs_three_steps():
    """The lane-per-pair update (more than 1,024 pairs), five step workgroups,
    17 search workgroups; max_steps below the model's truncates.  Pairs at the
    workgroups' edges and the two whose episode ends early are checked against
    the oracle; the live counts are the oracle's: 1030, 1028, 0."""
    B, first, max_steps = 1030, 7000, 3
    checked = (0, 63, 64, 255, 256, 1023, 1024, 1029) + SHORT_OF_1030
    exp = oracle_batch("Driving-v1", first, checked, max_steps)
    bp = engine("Driving-v1", B, max_steps)
    rec = Recorder(B)
    lives = []
    step = bp.engine.episodes_step

    def counted(num_sims):
        lives.append(step(num_sims))
        return lives[-1]

    bp.engine.episodes_step = counted
    rows = bp.run_episodes(range(first, first + B), until="all_done", max_steps=max_steps,
                           on_step=rec)
    res = bp.engine.episodes_results()
    bp.close()
    assert not res["error"].any()
    for b in checked:
        trace, records = exp[b]
        assert len(trace["steps"]) == (2 if b in SHORT_OF_1030 else 3)
        check_pair(rows[b], rec.steps[b], b, first + b, trace, records)
    full = np.ones(B, dtype=bool)
    full[list(SHORT_OF_1030)] = False
    assert (res["len"][full] == 3).all() and (res["truncated"][full] == 1).all()
    assert (res["len"][~full] == 2).all() and (res["all_done"][~full] == 1).all()
    assert not res["truncated"][~full].any()
    assert lives == [B, B - len(SHORT_OF_1030), 0]


POP = [("p_fw", [0.55, 0.15, 0.2, 0.1]), ("p_turn", [0.0, 0.45, 0.35, 0.2])]
POP_B = 16


def population(model):
    from posggym_baselines_amd.planning.policies import FixedDistributionPolicy
    return [FixedDistributionPolicy(model, "1", pid, p) for pid, p in POP]


def serial_episode(pair, env_seed, until):
    """The serial harness with an INTMCP keyed like the pair: its row and steps."""
    from posggym_baselines_amd.planning import INTMCP, run_planning_episodes
    from posggym_baselines_amd.planning.intmcp import IntmcpEngine
    env = "PursuitEvasion-v1"
    model = product_model(env)
    cfg = product_config(TEST_CFG, S)
    planner = INTMCP.initialize(model, EGO, cfg, 1, None)
    planner._engine.close()
    planner._engine = IntmcpEngine(model, EGO, cfg, num_pairs=1, num_sims=S, tree_key_base=pair,
                                   nesting_level=1)
    steps = []
    env_model = product_model(env)
    rows = run_planning_episodes(
        planner, env_model, 1, EGO, env_seeds=[env_seed], until=until,
        other_agents=population(env_model),
        on_step=lambda t, obs, a, ts: steps.append((a[EGO], a["1"], fhex(ts.rewards[EGO]))))
    planner.close()
    return rows[0], steps


@pytest.mark.timeout(300)
def test_population_equals_the_serial_harness():
    """16 PursuitEvasion pairs against a 2-policy population: four pairs that
    cover both policies equal the serial harness; other_agents=None is the
    uniform agent's batch."""
    env = "PursuitEvasion-v1"
    model = product_model(env)
    bp = engine(env, POP_B, PE_STEPS)
    rec = Recorder(POP_B)
    seeds = range(PE_FIRST, PE_FIRST + POP_B)
    rows = bp.run_episodes(seeds, until="all_done", other_agents=population(model), on_step=rec)
    pops = bp.episode_pop_states()
    ids = [p[0] for p in POP]
    assert [r["other_policy_id"] for r in rows] == [ids[int(k)] for k in pops["policy_index"]]
    assert set(pops["policy_index"].tolist()) == {0, 1} and (pops["mixture_index"] == -1).all()
    picked = [int(np.nonzero(pops["policy_index"] == k)[0][j]) for k in (0, 1) for j in (0, 1)]
    for b in picked:
        srow, ssteps = serial_episode(b, PE_FIRST + b, "all_done")
        assert rows[b]["other_policy_id"] == srow["other_policy_id"], b
        assert rec.steps[b] == ssteps, b
        assert rows[b]["len"] == srow["len"] == len(ssteps), b
        assert fhex(rows[b]["return"]) == fhex(srow["return"]), b
        assert fhex(rows[b]["discounted_return"]) == fhex(srow["discounted_return"]), b
        if rows[b]["other_policy_id"] == "p_turn":
            assert all(s[1] != 0 for s in rec.steps[b])
    # back to the uniform agent on the same engine's successor: the rows of the
    # plain batch (a fresh engine replays the planners' streams)
    bp.close()
    bp = engine(env, POP_B, PE_STEPS)
    rec2 = Recorder(POP_B)
    rows2 = bp.run_episodes(seeds, until="all_done", other_agents=None, on_step=rec2)
    assert (bp.episode_pop_states()["policy_index"] == -1).all()
    bp.close()
    plain, plain_steps = pe_rows("all_done")
    timing = {"time", "search_time", "update_time", "mem_usage"}
    for b in range(POP_B):
        assert "other_policy_id" not in rows2[b]
        assert rec2.steps[b] == plain_steps[b]
        for k in rows2[b]:
            if k not in timing:
                assert fhex(rows2[b][k]) == fhex(plain[b][k]), (b, k)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", ["intmcp_ucb", "intmcp_pe"])
def test_reference_goldens_through_one_pair(case):
    """The reference planner's golden I-NTMCP episodes through run_episodes on
    one pair: both agents' actions, reward bits, length and return."""
    from posggym_baselines_amd.planning import BatchedINTMCP
    data = load(case)
    env, ego, max_steps = data["env"], data["ego"], data["max_steps"]
    e = int(ego)
    for ep in data["episodes"]:
        steps = ep["trace"]["steps"]
        bp = BatchedINTMCP(product_model(env), ego,
                           product_config(cfg_kwargs(ep["config"]), data["num_sims"]), 1,
                           data["num_sims"], searches=max_steps)
        rec = Recorder(1)
        rows = bp.run_episodes([ep["env_seed"]], until="all_done", max_steps=max_steps, on_step=rec)
        bp.close()
        assert rows[0]["len"] == ep["trace"]["len"] == len(rec.steps[0])
        assert [(s[0], s[1]) for s in rec.steps[0]] == \
            [(s["actions"][e], s["actions"][1 - e]) for s in steps], case
        assert [s[2] for s in rec.steps[0]] == [s["reward"] for s in steps], case
        assert fhex(rows[0]["return"]) == ep["trace"]["return"]
        assert rows[0]["env_seed"] == ep["env_seed"]


@pytest.mark.timeout(120)
def test_guards_raise_before_any_launch():
    from posggym_baselines_amd._native import PomcpError
    bp = engine("Driving-v1", 4, 1)
    with pytest.raises(ValueError, match="searches=50"):
        bp.run_episodes()
    with pytest.raises(PomcpError):   # nothing was launched: no batch of episodes exists
        bp.episode_states()
    bp.close()
    bp = engine("Driving-v1", 4, 50)
    with pytest.raises(ValueError, match="until"):
        bp.run_episodes(until="never")
    with pytest.raises(ValueError, match="env_seeds"):
        bp.run_episodes([1, 2, 3])
    with pytest.raises(ValueError, match="max_steps"):
        bp.run_episodes(max_steps=51)
    with pytest.raises(ValueError, match="max_steps"):
        bp.run_episodes(max_steps=0)
    with pytest.raises(PomcpError):
        bp.episode_states()
    bp.close()
