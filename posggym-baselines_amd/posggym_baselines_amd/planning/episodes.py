"""Episode loop of the planning experiments around a GPU planner.

Restates ``run_planning_exp`` (``baseline_exps/exp_utils.py:468-552``) and the
test runner ``run_policies`` (``tests/planning/test_pomcp.py:16-33``) for the
models of this build: reset the environment and the planner, then per step
``planner.step(obs[agent_id])``, the other agents' actions, ``env.step``,
and per episode the reference's result row

    num, len, return, discounted_return, time  + PlanningStatTracker.STAT_KEYS

(``exp_utils.py:325-331, 506-535``).  ``until="agent_done"`` ends an episode
when the planning agent is done (``exp_utils.py:522``), ``"all_done"`` when
every agent is (``test_pomcp.py:28``).  ``env.step`` stops at the model's
``spec.max_episode_steps`` (posggym's TimeLimit).

The non-planning agents are the experiments' uniform random policies
(``UniformOtherAgentFn`` over ``Random-v0``, ``exp_utils.py:481-482``): agent
``i`` draws from Philox stream ``40 + i`` under the key (env seed,
``ENV_TREE_KEY``), the stream the golden episodes were recorded with, so an
episode here replays the reference planner's episode step for step
(``tests/test_gpu_parity.py::test_episode_harness_replays_reference_episodes``).

With ``other_agents=[FixedDistributionPolicy, ...]`` the other agent of every
episode is drawn from that test population instead (``UniformOtherAgentFn``,
``posggym_baselines/utils/agent_env_wrapper.py:8-27``: ``model.rng.choice(ids)``
at every reset; ``PopulationAgents`` below), and the row says which one played
(``other_policy_id``).  A member may be state-reactive (``ShortestPathPolicy``,
Driving-v1's shortest-path agents): it acts on the true state before the joint
action and still takes its word of the agent's stream.

With ``belief_tracker=BeliefStatTracker(planner, EpisodeEnvView(...), ...)`` the
row also carries the tracker's ``belief_*_acc`` columns
(``exp_utils.py:488-534``): the harness keeps the tracker's env view current
(state, last observations, the other agents' last actions), resets the tracker
after the planner and steps it after ``env_model.step``.
"""
import csv
import ctypes as C
import math
import time
from typing import Callable, Dict, List, Optional

import numpy as np
import psutil

from posggym_baselines_amd.planning.utils import PlanningStatTracker

S_ENV_POLICY_BASE = 40   # philox.h S_ENV_POLICY_BASE: true agent i's random policy
S_ENV_POPULATION = 44    # philox.h S_ENV_POPULATION: the episode's policy of the population
EPISODE_RESULT_HEADS = ["num", "len", "return", "discounted_return", "time"] + \
    PlanningStatTracker.STAT_KEYS


def batch_episode_row(num, res, elapsed, search_ms, update_ms, steps, mem):
    """The ``EPISODE_RESULT_HEADS`` + ``env_seed`` row of one tree (or planner
    pair) of a batch played on the device, from its ``pomcp_episode_result``
    ``res`` (``BatchedPOMCP.run_episodes`` documents the columns): the planner
    columns are means over the ``searched_steps`` (integer sum / n, sequential
    FP64 sum / n; NaN without such a step), ``search_time`` / ``update_time``
    the batch's device time per step."""
    n = int(res["searched_steps"])
    row = {k: 0.0 for k in EPISODE_RESULT_HEADS}
    row.update(num=num, len=int(res["len"]), discounted_return=float(res["discounted_return"]),
               time=elapsed, env_seed=int(res["env_seed"]))
    row["return"] = float(res["ret"])
    if n == 0:
        for k in EPISODE_RESULT_HEADS[5:]:
            row[k] = math.nan
    else:
        row.update(search_time=search_ms / 1e3 / steps, update_time=update_ms / 1e3 / steps,
                   search_depth=int(res["search_depth_sum"]) / n,
                   num_sims=int(res["num_sims_sum"]) / n, mem_usage=mem,
                   min_value=float(res["min_value_sum"]) / n,
                   max_value=float(res["max_value_sum"]) / n)
    return row


# ----------------------------------------------------------------------------
# The driver the batched entry points share (BatchedPOMCP.run_episodes /
# run_episode_queue / run_planner_queue, BatchedINTMCP.run_episodes /
# run_episode_queue): each checks the arguments only it has, then
# episode_guards, play_batch and episode_rows.

def check_until(until):
    if until not in ("agent_done", "all_done"):
        raise ValueError(f"until must be 'agent_done' or 'all_done', not {until!r}")


def episode_guards(planner, what, until, max_steps=None):
    """What every entry point checks before anything is launched: ``until``,
    the model's ``spec.max_episode_steps`` (the default and upper limit of
    ``max_steps``) and the planner's own arena sizing
    (``planner._check_sized(what, max_steps)``); returns ``max_steps``."""
    check_until(until)
    spec = getattr(planner.engine.model, "spec", None)
    limit = int(spec.max_episode_steps) if spec is not None and spec.max_episode_steps else 0
    if limit < 1:
        raise ValueError(f"{what} needs the model's spec.max_episode_steps")
    max_steps = limit if max_steps is None else int(max_steps)
    if not 1 <= max_steps <= limit:
        raise ValueError(f"max_steps must be 1 to the model's max_episode_steps ({limit}), "
                         f"not {max_steps}")
    planner._check_sized(what, max_steps)
    return max_steps


def episode_population(planner, other_agents, known_ids=()):
    """``other_agents`` as (the population's ids, its action distributions, each
    policy's index among ``known_ids`` -- the policies the planners model -- or
    -1); three ``None`` without a population."""
    if other_agents is None:
        return None, None, None
    other_agents = list(other_agents)
    probs = check_population(other_agents, planner.engine.A)
    ids = [pol.policy_id for pol in other_agents]
    known = list(known_ids or [])
    return ids, probs, [known.index(i) if i in known else -1 for i in ids]


def population_kinds(planner, other_agents):
    """The population's ``pomcp_policy_kinds`` entries, [(kind, param0, param1)]
    per policy, or ``None`` when every policy is a fixed distribution (or there
    is no population): what ``engine.episodes_set_population_kinds`` takes after
    ``episodes_set_population``.  A reactive policy needs the engine's model to
    be the environment it acts in (``NotImplementedError`` otherwise, before
    anything is launched)."""
    from posggym_baselines_amd.planning.policies import is_reactive, policy_kinds
    if other_agents is None or not any(is_reactive(pol) for pol in other_agents):
        return None
    ego = getattr(planner.engine, "ego", None)     # the planning agent's index
    ego = None if ego is None else planner.engine.model.possible_agents[ego]
    for pol in other_agents:
        if is_reactive(pol) and pol.agent_id == ego:
            raise ValueError(f"{pol.policy_id} is built for agent {ego!r}, the planning agent")
    return policy_kinds(planner.engine.model, other_agents)


def play_batch(planner, what, begin, fetch, slots, max_steps, on_step, entries=None,
               noun="slots"):
    """Begin a batch (``begin(pow_table)``: the population and the engine's
    begin call), step its ``slots`` until none is live and ``fetch()`` its
    records.  A batch plays ``max_steps`` steps at most; a queue of ``entries``
    episodes ``entries * max_steps``, and one that has not drained by then
    raises ``RuntimeError`` (``what``'s ``noun`` still playing).  Returns the
    records and the batch's figures for ``episode_rows``: the wall-clock seconds
    of all of this, the device search and update ms, the steps, the RSS (MiB)."""
    engine = planner.engine
    gamma = engine.config.discount
    pow_table = [gamma ** t for t in range(max_steps)]   # Python's own float ** int
    step_cap = max_steps if entries is None else entries * max_steps
    start = time.time()
    begin(pow_table)
    live, t = slots, 0
    while live > 0 and t < step_cap:
        live = engine.episodes_step(planner.num_sims)
        if on_step is not None:
            on_step(t, planner)
        t += 1
    if entries is not None and live > 0:
        raise RuntimeError(f"{what}: {live} {noun} still playing after {t} steps")
    res = fetch()
    (upd_ms, search_ms, _), steps = engine.episodes_timing()
    elapsed = time.time() - start
    mem = psutil.Process().memory_info().rss / 1024**2
    return res, (elapsed, search_ms, upd_ms, steps, mem)


def belief_acc_columns(acc_stats, acc, acc_steps, max_steps):
    """The ``BeliefStatTracker`` columns of a batch or a queue, every column for
    all episodes at once: [(key, one value per episode)] in the tracker's key
    order, from the device records ``acc`` (``pomcp_episode_belief_acc``) and,
    with ``track_per_step``, the per-step table ``acc_steps`` (else ``None``).
    A mean is NaN for an episode without a recorded step, a step's value NaN
    past the episode's end; sum / count is one IEEE division, as Python's."""
    from posggym_baselines_amd.planning.utils import BeliefStatTracker
    cnt = acc["count"].astype(np.int64)
    played = cnt > 0
    t_idx = np.arange(max_steps)[None, :] < cnt[:, None]
    columns = []
    for key in BeliefStatTracker.get_stat_keys(acc_stats, acc_steps is not None, max_steps):
        k, _, t = key[len("belief_"):].partition("_acc")
        if not t:       # the episode's mean
            v = 0.0 if k == "history" else acc[k + "_sum"] / np.maximum(cnt, 1)
            col = np.where(played, v, np.nan)
        else:           # step t's value ("_<t>")
            t = int(t[1:])
            v = 0.0 if k == "history" else acc_steps[:, t, ("state", "policy", "action").index(k)]
            col = np.where(t_idx[:, t], v, np.nan)
        columns.append((key, col.tolist()))
    return columns


def episode_rows(results, figures, write_row, *, queue=None, pop_ids=None, policy_index=None,
                 acc_columns=()):
    """One ``batch_episode_row`` per record of ``results`` (``num`` = its index)
    with, in this order, ``slot`` / ``slot_order`` of the queue rows ``queue``,
    ``other_policy_id`` = ``pop_ids[policy_index[i]]`` and ``acc_columns``;
    ``write_row`` sees each row."""
    rows = []
    for i in range(len(results)):
        row = batch_episode_row(i, results[i], *figures)
        if queue is not None:
            row.update(slot=int(queue["slot"][i]), slot_order=int(queue["slot_order"][i]))
        if pop_ids is not None:
            row["other_policy_id"] = pop_ids[int(policy_index[i])]
        for key, col in acc_columns:
            row[key] = col[i]
        if write_row is not None:
            write_row(row)
        rows.append(row)
    return rows


class EpisodeEnvView:
    """What ``BeliefStatTracker`` reads of the reference's ``AgentEnvWrapper``
    (``utils.py:224-266``): ``state``, ``last_obs``, ``last_actions`` (the other
    agents', ``None`` after a reset), ``policies[i].policy_id`` and ``spec``.
    ``run_planning_episodes`` keeps it current.  ``policy_ids`` = {other agent:
    the id its true policy goes by} (default: "uniform_random", what the
    harness's other agents play)."""

    def __init__(self, env_model, agent_id: str, policy_ids: Optional[Dict[str, str]] = None):
        from types import SimpleNamespace
        self.spec = env_model.spec
        self.other_agent_ids = [i for i in env_model.possible_agents if i != agent_id]
        ids = policy_ids or {}
        self.policies = {i: SimpleNamespace(policy_id=ids.get(i, "uniform_random"))
                         for i in self.other_agent_ids}
        self.state = None
        self.last_obs = {}
        self.last_actions = {i: None for i in self.other_agent_ids}

    def on_reset(self, state, obs):
        self.state = state
        self.last_obs = dict(obs)
        self.last_actions = {i: None for i in self.other_agent_ids}

    def on_step(self, state, obs, actions):
        self.state = state
        self.last_obs = dict(obs)
        self.last_actions = {i: actions[i] for i in self.other_agent_ids}


class UniformRandomAgents:
    """The true other agents: uniform random actions from their own streams."""

    def __init__(self, model, env_seed: int):
        from posggym_baselines_amd.envs.driving import ENV_TREE_KEY
        self.model = model
        self.env_seed = int(env_seed)
        self.tree = ENV_TREE_KEY
        self._ctr: Dict[str, int] = {}

    def reset(self):
        self._ctr = {i: 0 for i in self.model.possible_agents}

    def act(self, agent_id: str, state=None) -> int:
        from posggym_baselines_amd._native import check, load
        j = self._ctr[agent_id]
        self._ctr[agent_id] = j + 1
        w = (C.c_uint32 * 1)()
        check(load().pomcp_philox_words(self.env_seed, self.tree, S_ENV_POLICY_BASE + int(agent_id),
                                        j, 1, w))
        return (int(w[0]) * self.model.action_spaces[agent_id].n) >> 32


def check_population(population, num_actions: Optional[int] = None):
    """The population's action distributions (``get_pi`` in action order), after
    the checks both episode loops make: 1 to ``POMCP_MAX_TYPE_POLICIES``
    ``FixedDistributionPolicy`` or state-reactive (``ShortestPathPolicy``)
    entries with distinct ``policy_id``s, one probability per action
    (``num_actions``; default: the first policy's).  A reactive policy's row is
    the uniform distribution: a placeholder nothing draws from."""
    from posggym_baselines_amd._native import POMCP_MAX_TYPE_POLICIES
    from posggym_baselines_amd.planning.policies import FixedDistributionPolicy, is_reactive
    population = list(population)
    if not 1 <= len(population) <= POMCP_MAX_TYPE_POLICIES:
        raise ValueError(f"other_agents needs 1 to {POMCP_MAX_TYPE_POLICIES} policies, "
                         f"not {len(population)}")
    for pol in population:
        if not isinstance(pol, FixedDistributionPolicy) and not is_reactive(pol):
            raise NotImplementedError(
                f"policy {getattr(pol, 'policy_id', pol)!r}: the population holds "
                "fixed-distribution and shortest-path policies (planning/policies.py)")
    ids = [pol.policy_id for pol in population]
    if len(set(ids)) != len(ids):
        raise ValueError(f"other_agents has duplicate policy ids: {ids}")
    probs = []
    for pol in population:
        if is_reactive(pol):
            pi = {a: 1.0 / pol.num_actions for a in range(pol.num_actions)}
        else:
            pi = pol.get_pi(pol.get_initial_state()).probs
        if num_actions is None:
            num_actions = len(pi)
        if len(pi) != num_actions:
            raise ValueError(f"{pol.policy_id}: {len(pi)} probabilities for {num_actions} actions")
        probs.append([float(pi.get(a, 0.0)) for a in range(num_actions)])
    return probs


class PopulationAgents:
    """The true other agent drawn per episode from a population of
    ``FixedDistributionPolicy`` (``UniformOtherAgentFn``,
    ``agent_env_wrapper.py:8-27``): ``reset()`` draws the episode's policy index
    as ``uniform_int(word 0 of stream S_ENV_POPULATION, len(population))`` under
    the key (env seed, ``ENV_TREE_KEY``) -- the build's ``model.rng.choice`` --
    and ``act(i)`` turns word ``j`` of agent ``i``'s policy stream (the counter
    ``UniformRandomAgents`` uses) into an action as CPython's ``random.choices``
    does: ``bisect_right(cumulative(probs), word * 2**-32 * total, 0, n - 1)``
    (``tm_choice`` of csrc/pomcp_device.h, ``ep_choice`` of csrc/episode_step.h).
    A state-reactive member (``ShortestPathPolicy``) acts on ``state``, the true
    state before the joint action, which ``act`` must then be given; its word of
    the stream is counted all the same."""

    def __init__(self, model, env_seed: int, population):
        from posggym_baselines_amd.envs.driving import ENV_TREE_KEY
        from posggym_baselines_amd.planning.policies import cumulative
        self.model = model
        self.env_seed = int(env_seed)
        self.tree = ENV_TREE_KEY
        self.population = list(population)
        self._tables = [cumulative(p) for p in check_population(self.population)]
        self._ctr: Dict[str, int] = {}
        self.policy_index = None
        self.policy_id = None

    def _word(self, stream: int, j: int) -> int:
        from posggym_baselines_amd._native import check, load
        w = (C.c_uint32 * 1)()
        check(load().pomcp_philox_words(self.env_seed, self.tree, stream, j, 1, w))
        return int(w[0])

    def reset(self):
        self._ctr = {i: 0 for i in self.model.possible_agents}
        self.policy_index = (self._word(S_ENV_POPULATION, 0) * len(self.population)) >> 32
        self.policy_id = self.population[self.policy_index].policy_id

    def act(self, agent_id: str, state=None) -> int:
        import bisect
        from posggym_baselines_amd.planning.policies import cumulative, is_reactive
        j = self._ctr[agent_id]
        self._ctr[agent_id] = j + 1
        pol = self.population[self.policy_index]
        if is_reactive(pol):
            if state is None:
                raise ValueError(f"{pol.policy_id} acts on the state: act(agent_id, state)")
            if pol.agent_id != agent_id:
                raise ValueError(f"{pol.policy_id} is agent {pol.agent_id!r}'s policy, not "
                                 f"{agent_id!r}'s")
            if not hasattr(pol, "pi_from_state"):
                return pol.action_from_state(state)
            # a stochastic reactive member (PreyHeuristicPolicy): the word draws
            # from the distribution the rule gives in this state
            cum, total = cumulative(pol.pi_from_state(state))
        else:
            cum, total = self._tables[self.policy_index]
        x = self._word(S_ENV_POLICY_BASE + int(agent_id), j) * 2.0 ** -32 * total
        return bisect.bisect_right(cum, x, 0, len(cum) - 1)


def run_planning_episodes(planner, env_model, num_episodes: int, agent_id: str, *,
                          env_seeds: Optional[List[int]] = None, discount: Optional[float] = None,
                          until: str = "agent_done", exp_time_limit: float = math.inf,
                          write_row: Optional[Callable[[Dict], None]] = None,
                          on_step: Optional[Callable] = None,
                          belief_tracker=None, other_agents=None) -> List[Dict]:
    """Play ``num_episodes`` episodes of ``planner`` (agent ``agent_id``) in
    ``env_model`` against uniform random other agents; returns the result rows.

    ``other_agents``: a population (an ordered list of 1 to 8
    ``FixedDistributionPolicy`` or ``ShortestPathPolicy`` with distinct ids) for
    the non-planning agent;
    every episode draws one of them (``PopulationAgents``), the row gains
    ``other_policy_id`` and a ``belief_tracker``'s env view is told the drawn
    policy's id before the tracker is reset.

    ``env_seeds[e]`` seeds episode ``e``'s environment (model stream and the
    other agents' streams; default ``e``).  ``on_step(t, obs, actions, timestep)``
    sees every step.  ``belief_tracker``: a ``BeliefStatTracker`` over an
    ``EpisodeEnvView`` (its ``env``); its episode statistics join the row.
    """
    if until not in ("agent_done", "all_done"):
        raise ValueError(f"until must be 'agent_done' or 'all_done', not {until!r}")
    gamma = planner.config.discount if discount is None else discount
    limit = env_model.spec.max_episode_steps or math.inf
    rows = []
    start = time.time()
    for num in range(num_episodes):
        if time.time() - start >= exp_time_limit:
            break
        seed = num if env_seeds is None else int(env_seeds[num])
        env_model.seed(seed)
        if other_agents is None:
            others = UniformRandomAgents(env_model, seed)
        else:
            others = PopulationAgents(env_model, seed, other_agents)
        others.reset()
        state = env_model.sample_initial_state()
        obs = env_model.sample_initial_obs(state)
        planner.reset()
        if belief_tracker is not None:
            belief_tracker.env.on_reset(state, obs)
            if other_agents is not None:
                for i in belief_tracker.env.other_agent_ids:
                    belief_tracker.env.policies[i].policy_id = others.policy_id
            belief_tracker.reset()
        res = {"num": num, "len": 0, "return": 0.0, "discounted_return": 0.0, "time": 0.0}
        if other_agents is not None:
            res["other_policy_id"] = others.policy_id
        t0 = time.time()
        done = False
        while not done:
            actions = {i: (planner.step(obs[i]) if i == agent_id else None)
                       for i in env_model.possible_agents}
            for i in env_model.possible_agents:
                if i != agent_id:
                    actions[i] = others.act(i, state)
            ts = env_model.step(state, actions)
            if on_step is not None:
                on_step(res["len"], obs, actions, ts)
            reward = ts.rewards[agent_id]
            res["return"] += reward
            res["discounted_return"] += gamma ** res["len"] * reward
            res["len"] += 1
            state, obs = ts.state, ts.observations
            if belief_tracker is not None:
                belief_tracker.env.on_step(state, obs, actions)
                belief_tracker.step(belief_tracker.env)
            truncated = res["len"] >= limit
            if until == "agent_done":
                done = ts.terminations[agent_id] or ts.truncations[agent_id] or ts.all_done
            else:
                done = ts.all_done
            done = done or truncated
        res["time"] = time.time() - t0
        res.update(planner.stat_tracker.get_episode())
        if belief_tracker is not None:
            res.update(belief_tracker.get_episode())
        if write_row is not None:
            write_row(res)
        rows.append(res)
    return rows


class EpisodeResultsWriter:
    """``episode_results.csv`` with the reference's header (``exp_utils.py:363-404``)."""

    def __init__(self, path: str, extra_heads=()):
        """``extra_heads``: further columns after the reference's, e.g.
        ``BeliefStatTracker.get_stat_keys(...)``."""
        self.path = path
        self.heads = EPISODE_RESULT_HEADS + list(extra_heads)
        with open(path, "w", newline="") as f:
            csv.DictWriter(f, fieldnames=self.heads).writeheader()

    def __call__(self, row: Dict):
        with open(self.path, "a", newline="") as f:
            csv.DictWriter(f, fieldnames=self.heads).writerow(row)
