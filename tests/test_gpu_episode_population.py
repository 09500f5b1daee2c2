"""BatchedPOMCP.run_episodes against a policy population, with the belief
accuracy columns accumulated on the device (k_episode_reset / k_episode_step
with a population, k_episode_belief_acc): every tree against the SERIAL harness
(run_planning_episodes with other_agents= and a BeliefStatTracker on a single
planner keyed like the tree), bit for bit, on every search kernel mode."""
import functools
import math

import numpy as np
import pytest

from golden_util import load
from gpu_util import product_config, product_model
from oracle.episode import fhex
from oracle.run import oracle_episode

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["lane", "lane_eager", "wave", "wave_tree", "wave_plain"])
def search_kernel(request, monkeypatch):
    """The search kernel modes of tests/test_gpu_batched_episodes.py."""
    kind, _, mode = request.param.partition("_")
    monkeypatch.setenv("POMCP_SEARCH_KERNEL", kind)
    if kind == "lane":
        monkeypatch.setenv("POMCP_DEFER_CUTOFF", "0" if mode == "eager" else "1")
    elif mode:
        monkeypatch.setenv("POMCP_STEP_TREE", "1" if mode == "tree" else "0")
    return kind


EGO, OTHER = "0", "1"
# the plain planner's configuration (tests/test_gpu_batched_episodes.py TEST_CFG)
TEST_CFG = dict(discount=0.95, search_time_limit=0.1, c=math.sqrt(2), truncated=False,
                action_selection="ucb", pucb_exploration_fraction=0.25, known_bounds=None,
                step_limit=None, epsilon=0.92, seed=0, state_belief_only=True)
STATS3 = ["policy", "action", "state"]


class Recorder:
    """on_step callback of run_episodes: per tree the (ego action, other action,
    reward bits) of every step it played, and the belief accuracy records after
    every step."""

    def __init__(self, B, acc=True):
        self.steps = [[] for _ in range(B)]
        self.lens = np.zeros(B, dtype=np.int64)
        self.acc = [] if acc else None

    def __call__(self, t, bp):
        st = bp.episode_states()
        for b in np.nonzero(st["res"]["len"] > self.lens)[0]:
            self.steps[b].append((int(st["last_action"][b]), int(st["last_other_action"][b]),
                                  fhex(st["last_reward"][b])))
        self.lens = st["res"]["len"].astype(np.int64)
        if self.acc is not None:
            self.acc.append(bp.episode_belief_acc().copy())


def swap_engine(planner, model, cfg, num_sims, tree, ego=EGO):
    """Key a single planner like tree `tree` of a batch: (seed, tree)."""
    from posggym_baselines_amd.planning.engine import PomcpEngine
    planner._engine.close()
    planner._engine = PomcpEngine(model, ego, cfg, num_trees=1, num_sims=num_sims,
                                  tree_key_base=tree, type_policies=planner.type_policies)


def serial_row(planner, env, env_seed, pop, stats, until):
    """One episode of the serial harness: its row and per-step records."""
    from posggym_baselines_amd.planning import (BeliefStatTracker, EpisodeEnvView,
                                                run_planning_episodes)
    env_model = product_model(env)
    tracker = BeliefStatTracker(planner, EpisodeEnvView(env_model, EGO), track_per_step=True,
                                stats_to_track=stats)
    steps = []
    rows = run_planning_episodes(
        planner, env_model, 1, EGO, env_seeds=[env_seed], until=until, belief_tracker=tracker,
        other_agents=pop,
        on_step=lambda t, obs, a, ts: steps.append((a[EGO], a[OTHER], fhex(ts.rewards[EGO]))))
    return rows[0], steps


def check_tree(row, rec_steps, srow, ssteps, stats, max_steps, where):
    """A batch row against the serial harness's: actions, reward bits, returns,
    every per-step accuracy, the means as sequential sums / count."""
    assert row.get("other_policy_id") == srow.get("other_policy_id"), where
    assert rec_steps == ssteps, where
    assert row["len"] == srow["len"] == len(ssteps), where
    assert fhex(row["return"]) == fhex(srow["return"]), where
    assert fhex(row["discounted_return"]) == fhex(srow["discounted_return"]), where
    n = row["len"]
    for k in stats:
        vals = [srow[f"belief_{k}_acc_{t}"] for t in range(n)]
        for t in range(max_steps):
            got = row[f"belief_{k}_acc_{t}"]
            if t < n:
                assert fhex(got) == fhex(vals[t]), (where, k, t)
            else:
                assert np.isnan(got) and np.isnan(srow[f"belief_{k}_acc_{t}"]), (where, k, t)
        s = 0.0
        for v in vals:
            s = s + v
        assert fhex(row[f"belief_{k}_acc"]) == fhex(s / n), (where, k)


# ---------------------------------------------------------------- Driving-v1
DRV_B, DRV_FIRST, DRV_STEPS = 70, 3000, 50
DRV_STRANGER = ("o_left", [0.1, 0.05, 0.5, 0.3, 0.05])
# serial yardstick for these trees: both search waves (0..63, 64..69)
DRV_SUBSET = list(range(10)) + list(range(64, 70))


def potmmcp_setup():
    from test_gpu_potmmcp import _policies
    from posggym_baselines_amd.planning.policies import FixedDistributionPolicy
    data = load("potmmcp_pucb")
    model = product_model("Driving-v1")
    others, meta = _policies(model, EGO, data["spec"])
    mix = others[OTHER]
    cfg = product_config(data["episodes"][0]["config"], data["num_sims"])
    pop = list(mix.policies.values()) + [FixedDistributionPolicy(model, OTHER, *DRV_STRANGER)]
    return data, model, others, meta, mix, cfg, pop


@functools.lru_cache(maxsize=None)
def driving_serial():
    """The serial harness on trees DRV_SUBSET; computed once for all modes (the
    search kernels are bit-identical, tests/test_gpu_parity.py)."""
    from posggym_baselines_amd.planning import POTMMCP
    data, model, others, meta, mix, cfg, pop = potmmcp_setup()
    out = {}
    for b in DRV_SUBSET:
        planner = POTMMCP(model, EGO, cfg, others, meta)
        swap_engine(planner, model, cfg, data["num_sims"], b)
        out[b] = serial_row(planner, "Driving-v1", DRV_FIRST + b, pop, STATS3, "all_done")
        planner._engine.close()
    return out


def test_driving_potmmcp_against_a_population_equals_the_serial_harness():
    from posggym_baselines_amd.planning import BatchedPOMCP, BeliefStatTracker
    from posggym_baselines_amd.planning.episodes import EPISODE_RESULT_HEADS
    from posggym_baselines_amd.planning.potmmcp import type_policy_tables
    data, model, others, meta, mix, cfg, pop = potmmcp_setup()
    B, S = DRV_B, data["num_sims"]
    bp = BatchedPOMCP(model, EGO, cfg, B, S, searches=DRV_STEPS, reroot=True,
                      type_policies=type_policy_tables(model, EGO, meta, mix),
                      other_policy_ids=list(mix.policies))
    rec = Recorder(B)
    sizes = []

    def on_step(t, bp_):
        rec(t, bp_)
        if t < 6:
            sizes.extend(int(n) for n in bp_.episode_belief_counts()["belief_size"])

    rows = bp.run_episodes(range(DRV_FIRST, DRV_FIRST + B), until="all_done", belief_acc=STATS3,
                           track_per_step=True, other_agents=pop, on_step=on_step)
    keys = BeliefStatTracker.get_stat_keys(STATS3, True, DRV_STEPS)
    assert list(rows[0]) == EPISODE_RESULT_HEADS + ["env_seed", "other_policy_id"] + keys
    pops = bp.engine.episodes_pop_states()
    final = bp.episode_belief_acc()
    ids = [p.policy_id for p in pop]
    assert not final["error"].any()
    # --- every subset tree equals the serial harness
    serial = driving_serial()
    assert {int(pops["policy_index"][b]) for b in DRV_SUBSET} == {0, 1, 2}
    for b in DRV_SUBSET:
        srow, ssteps = serial[b]
        assert srow["other_policy_id"] == ids[int(pops["policy_index"][b])]
        check_tree(rows[b], rec.steps[b], srow, ssteps, STATS3, DRV_STEPS, b)
    # --- the conditions that keep the test from passing vacuously
    lens = [r["len"] for r in rows]
    assert min(lens) < max(lens) and max(lens) >= 3       # parked trees; both belief ends read
    per_step = {k: [rows[b][f"belief_{k}_acc_{t}"] for b in range(B) for t in range(lens[b])]
                for k in STATS3}
    assert any(0.0 < v < 1.0 for v in per_step["policy"])
    assert any(v > 0.0 for v in per_step["state"])
    assert any(v > 0.0 for v in per_step["action"])
    strangers = [b for b in range(B) if int(pops["mixture_index"][b]) == -1]
    assert strangers and all(int(pops["policy_index"][b]) == 2 for b in strangers)
    assert any(b in DRV_SUBSET for b in strangers)
    for b in strangers:
        assert rows[b]["other_policy_id"] == DRV_STRANGER[0] and rows[b]["belief_policy_acc"] == 0.0
        assert all(rows[b][f"belief_policy_acc_{t}"] == 0.0 for t in range(lens[b]))
    assert any(n % 64 for n in sizes)
    # --- parked trees: the count is the length, and a tree that finished early
    # kept its record through its neighbours' later steps
    total = len(rec.acc)
    assert total == max(lens)
    assert [int(c) for c in final["count"]] == lens
    early = [b for b in range(B) if lens[b] < total]
    assert early
    for b in early:
        assert rec.acc[lens[b] - 1][b].tobytes() == final[b].tobytes(), b
        assert int(rec.acc[lens[b] - 1]["count"][b]) == lens[b]
    for t in range(total):      # no record runs ahead of its episode
        assert all(int(rec.acc[t]["count"][b]) == min(t + 1, lens[b]) for b in range(B))
    bp.close()


# --------------------------------------------------------- PursuitEvasion-v1
PE_B, PE_FIRST, PE_STEPS, PE_S = 24, 2000, 100, 32
PE_POP = [("p_fw", [0.55, 0.15, 0.2, 0.1]), ("p_turn", [0.0, 0.45, 0.35, 0.2])]
STATS4 = ["policy", "action", "state", "history"]


def pe_population(model):
    from posggym_baselines_amd.planning.policies import FixedDistributionPolicy
    return [FixedDistributionPolicy(model, OTHER, pid, p) for pid, p in PE_POP]


@functools.lru_cache(maxsize=None)
def pe_serial(until):
    from posggym_baselines_amd.planning import POMCP, RandomSearchPolicy
    model = product_model("PursuitEvasion-v1")
    cfg = product_config(TEST_CFG, PE_S)
    out = []
    for b in range(PE_B):
        planner = POMCP(model, EGO, cfg, RandomSearchPolicy(model, EGO))
        swap_engine(planner, model, cfg, PE_S, b)
        out.append(serial_row(planner, "PursuitEvasion-v1", PE_FIRST + b, pe_population(model),
                              STATS4, until))
        planner._engine.close()
    return out


@pytest.mark.parametrize("until", ["all_done", "agent_done"])
def test_pursuit_evasion_plain_planner_against_a_population(until):
    from posggym_baselines_amd.planning import BatchedPOMCP
    model = product_model("PursuitEvasion-v1")
    bp = BatchedPOMCP(model, EGO, product_config(TEST_CFG, PE_S), PE_B, PE_S, searches=PE_STEPS,
                      reroot=True)
    rec = Recorder(PE_B)
    rows = bp.run_episodes(range(PE_FIRST, PE_FIRST + PE_B), until=until, belief_acc=True,
                           track_per_step=True, other_agents=pe_population(model), on_step=rec)
    serial = pe_serial(until)
    final = bp.episode_belief_acc()
    bp.close()
    assert not final["error"].any()
    seen = set()
    for b in range(PE_B):
        srow, ssteps = serial[b]
        check_tree(rows[b], rec.steps[b], srow, ssteps, STATS4, PE_STEPS, (until, b))
        seen.add(rows[b]["other_policy_id"])
        n = rows[b]["len"]
        for k in ("policy", "action", "history"):     # the particles carry no policy
            assert rows[b][f"belief_{k}_acc"] == 0.0
            assert all(rows[b][f"belief_{k}_acc_{t}"] == 0.0 for t in range(n))
        if rows[b]["other_policy_id"] == "p_turn":
            assert all(s[1] != 0 for s in rec.steps[b])
    assert seen == {"p_fw", "p_turn"}
    lens = [r["len"] for r in rows]
    assert min(lens) < max(lens)
    assert [int(c) for c in final["count"]] == lens
    assert any(rows[b]["belief_state_acc"] > 0.0 for b in range(PE_B))


# ------------------------------------------------------------ no population
def test_without_a_population_nothing_changes():
    """run_episodes() with no new keyword against the oracle batch (as
    tests/test_gpu_batched_episodes.py compares it); then other_agents=None with
    belief_acc=True: the same episodes, and every step's state accuracy equal to
    the route it replaces (episode_belief_counts() and host arithmetic)."""
    from posggym_baselines_amd.planning import BatchedPOMCP
    from posggym_baselines_amd.planning.episodes import EPISODE_RESULT_HEADS
    B, first, S, max_steps = 8, 3000, 32, 50
    seeds = range(first, first + B)
    exp = [oracle_episode(TEST_CFG, S, first + b, ego=EGO, tree=b, max_steps=max_steps,
                          env="Driving-v1") for b in range(B)]
    model = product_model("Driving-v1")

    def engine():
        return BatchedPOMCP(model, EGO, product_config(TEST_CFG, S), B, S, searches=max_steps,
                            reroot=True)

    bp = engine()
    rec = Recorder(B, acc=False)
    rows = bp.run_episodes(seeds, until="all_done", on_step=rec)
    assert all(list(r) == EPISODE_RESULT_HEADS + ["env_seed"] for r in rows)
    assert (bp.engine.episodes_pop_states()["policy_index"] == -1).all()
    for b, (trace, _) in enumerate(exp):
        steps = trace["steps"]
        assert rows[b]["len"] == len(steps) and fhex(rows[b]["return"]) == trace["return"]
        assert [list(s[:2]) for s in rec.steps[b]] == [s["actions"] for s in steps], b
        assert [s[2] for s in rec.steps[b]] == [s["reward"] for s in steps], b
    bp.close()

    bp = engine()
    rec2 = Recorder(B)
    host = [[] for _ in range(B)]
    played = np.zeros(B, dtype=np.int64)

    def on_step(t, bp_):
        rec2(t, bp_)
        c = bp_.episode_belief_counts()
        for b in np.nonzero(rec2.lens > played)[0]:
            n = int(c["belief_size"][b])
            host[b].append(int(c["state_matches"][b]) / n if n else 0.0)
        played[:] = rec2.lens

    rows2 = bp.run_episodes(seeds, until="all_done", belief_acc=True, track_per_step=True,
                            on_step=on_step)
    bp.close()
    timing = {"time", "search_time", "update_time", "mem_usage"}
    for b in range(B):
        assert rec2.steps[b] == rec.steps[b]
        assert "other_policy_id" not in rows2[b]
        for k in rows[b]:
            if k not in timing:
                assert fhex(rows2[b][k]) == fhex(rows[b][k]) or rows2[b][k] == rows[b][k], (b, k)
        n = rows2[b]["len"]
        assert [fhex(rows2[b][f"belief_state_acc_{t}"]) for t in range(n)] == \
            [fhex(v) for v in host[b]], b
        s = 0.0
        for v in host[b]:
            s = s + v
        assert fhex(rows2[b]["belief_state_acc"]) == fhex(s / n)
        for k in ("policy", "action", "history"):
            assert rows2[b][f"belief_{k}_acc"] == 0.0
        assert np.isnan(rows2[b][f"belief_state_acc_{max_steps - 1}"]) or n == max_steps
    assert any(rows2[b]["belief_state_acc"] > 0.0 for b in range(B))


# -------------------------------------------------------------------- guards
def test_guards_raise_before_any_launch():
    from posggym_baselines_amd._native import PomcpError
    from posggym_baselines_amd.planning import BatchedPOMCP
    from posggym_baselines_amd.planning.policies import FixedDistributionPolicy
    from posggym_baselines_amd.planning.potmmcp import type_policy_tables
    data, model, others, meta, mix, cfg, pop = potmmcp_setup()
    assert not cfg.state_belief_only
    bp = BatchedPOMCP(model, EGO, cfg, 4, 16, searches=DRV_STEPS, reroot=True,
                      type_policies=type_policy_tables(model, EGO, meta, mix),
                      other_policy_ids=list(mix.policies))
    with pytest.raises(NotImplementedError, match="history"):
        bp.run_episodes(belief_acc=True)
    with pytest.raises(NotImplementedError, match="history"):
        bp.run_episodes(belief_acc=["state", "history"])
    with pytest.raises(ValueError, match="unknown belief stat"):
        bp.run_episodes(belief_acc=["states"])
    with pytest.raises(ValueError, match="track_per_step"):
        bp.run_episodes(track_per_step=True)
    with pytest.raises(ValueError, match="duplicate"):
        bp.run_episodes(other_agents=pop + [pop[0]])
    many = [FixedDistributionPolicy(model, OTHER, f"p{k}", [0.2] * 5) for k in range(9)]
    with pytest.raises(ValueError, match="1 to 8"):
        bp.run_episodes(other_agents=many)
    with pytest.raises(ValueError, match="1 to 8"):
        bp.run_episodes(other_agents=[])
    with pytest.raises(PomcpError):   # nothing was launched: no batch of episodes exists
        bp.episode_states()
    with pytest.raises(PomcpError):
        bp.episode_belief_acc()
    bp.close()
    with pytest.raises(ValueError, match="other_policy_ids"):
        BatchedPOMCP(model, EGO, cfg, 4, 16, searches=DRV_STEPS, reroot=True,
                     other_policy_ids=["o_u"])
