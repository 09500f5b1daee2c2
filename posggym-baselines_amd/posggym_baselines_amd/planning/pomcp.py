"""POMCP drop-in: the reference's ``POMCP`` API (``pomcp.py:9-35`` on top of
``mcts.py:22-739``) with the search, the tree, the particle beliefs and the
generative model on the GPU.

Public surface kept from the reference: ``POMCP(model, agent_id, config,
search_policy)``, ``step(obs)``, ``reset()``, ``update(action, obs)``,
``get_action()``, ``close()``, and the attributes ``model``, ``agent_id``,
``config``, ``other_agent_policies``, ``search_policy``, ``step_statistics``,
``stat_tracker``, ``root``.

``BatchedPOMCP`` runs many independent planners (one tree each) in one kernel
launch; it is what the bench and batch experiments use.

``MCTSConfig.root_parallel = K > 1`` gives ONE planner K replica trees on the
GPU (root parallelisation): replica k is the exact single-tree planner with
RNG key (seed, k), every replica is updated with the played action and the
real observation, searches ceil(num_sims / K) simulations, and the played
action is the device merge of the replicas' root statistics
(``pomcp_merge_roots``: summed visits for PUCB, summed total / summed visits
otherwise).  K = 1 (default) is the reference's planner, bit-exact.

``POMCP(..., process_group=pg)`` spreads the replicas over the ranks of a
``torch.distributed`` group (one process per GPU, backend "nccl" = RCCL):
rank r's replicas take keys (seed, r*K .. r*K+K-1), ``num_sims`` is split over
all world x K replicas (ceil(num_sims / (world K)) each), and before the
decision one all-gather collects every rank's replica records
(``parallel.exchange_roots``); the device merge sums the world x K replicas in
one fixed order, so every rank plays the same action and reports the same
step statistics (simulations and root visits summed over all replicas,
min / max over them).  A failure on any rank (arena, HIP) is agreed on before
each collective and raised on every rank (``parallel.raise_together``), so no
rank waits forever in a collective its peer never reaches.
"""
import dataclasses
import logging
import math
import time
from typing import Optional

import numpy as np
import psutil

from posggym_baselines_amd.envs import engine_model

from posggym_baselines_amd.planning.config import MCTSConfig
from posggym_baselines_amd.planning.engine import PomcpEngine, search_bytes
from posggym_baselines_amd.planning.episodes import (belief_acc_columns, check_until,
                                                     episode_guards, episode_population,
                                                     episode_rows, play_batch, population_kinds)
from posggym_baselines_amd.planning.other_policy import RandomOtherAgentPolicy
from posggym_baselines_amd.planning.policies import mixture_is_reactive
from posggym_baselines_amd.planning.search_policy import RandomSearchPolicy, SearchPolicy
from posggym_baselines_amd.planning.utils import PlanningStatTracker


@dataclasses.dataclass
class RootView:
    """Read-only view of the GPU root node (``ObsNode`` fields the callers use)."""

    t: int = 0
    is_absorbing: bool = False
    visits: int = 0
    child_visits: tuple = ()
    child_values: tuple = ()
    child_totals: tuple = ()
    belief_size: int = 0


class POMCP:
    """Partially Observable Monte-Carlo Planning, GPU-resident tree.

    Other agents are random (``pomcp.py:28-31``).  The search policy is the
    uniform random one (``RandomSearchPolicy``, the reference's POMCP test
    setup, ``tests/planning/test_pomcp.py:36-74``: the plain kernel) or a
    fixed-distribution one (``SearchPolicyWrapper(FixedDistributionPolicy)``:
    node priors and rollouts, planning/ipomcp.py) or, on CooperativeReaching-v0,
    a goal heuristic (``SearchPolicyWrapper(GoalHeuristicPolicy)``, the
    reference's ``test_pomcp.py:77-117`` pattern); history-dependent
    (network) search policies raise ``NotImplementedError``.
    """

    def __init__(self, model, agent_id: str, config: MCTSConfig, search_policy: SearchPolicy,
                 *, num_sims: Optional[int] = None, process_group=None):
        from posggym_baselines_amd.planning.ipomcp import base_type_tables
        if not config.state_belief_only:
            # pomcp.py:32-34 calls config.replace(...), which does not exist on the
            # dataclass (AttributeError in the reference); dataclasses.replace is
            # what it means.  Recorded in DESIGN.md.
            config = dataclasses.replace(config, state_belief_only=True)
        others = {i: RandomOtherAgentPolicy(model, i) for i in model.possible_agents if i != agent_id}
        tables = base_type_tables(model, agent_id, config, others, search_policy)
        self.type_policies = tables
        self._init_planner(model, agent_id, config, search_policy, others, num_sims, process_group,
                           type_policies=tables)

    def _init_planner(self, model, agent_id, config, search_policy, other_agent_policies,
                      num_sims, process_group, type_policies=None):
        self.model = model
        self._emodel = engine_model(model)
        self.agent_id = agent_id
        self.config = config
        self.search_policy = search_policy
        self.other_agent_policies = other_agent_policies
        self.num_agents = len(model.possible_agents)
        self.action_space = list(range(model.action_spaces[agent_id].n))
        self._num_sims = num_sims if num_sims is not None else config.num_sims
        self._K = int(config.root_parallel)
        self._pg = process_group
        self._rank, self._world = 0, 1
        if process_group is not None:
            import torch.distributed as dist
            self._rank = dist.get_rank(process_group)
            self._world = dist.get_world_size(process_group)
        replicas = self._K * self._world
        per = math.ceil(self._num_sims / replicas) if self._num_sims is not None else None
        self._per_replica = per
        self._engine = PomcpEngine(model, agent_id, config, num_trees=self._K,
                                   num_sims=per, tree_key_base=self._rank * self._K,
                                   wall_clock=per is None, type_policies=type_policies)
        # cut-off children are deferred to the re-root (the engine's default):
        # with their bulk materialisation in k_compact_log that is the faster
        # mode for an episode planner too (pomcp_set_defer_cutoff; same results,
        # DESIGN.md §4 "Deferred records")
        self.step_limit = self._engine.step_limit
        self._logger = logging.getLogger()
        self._last_action = None
        self._step_num = 0
        self.root = RootView()
        self.step_statistics = {}
        self._reset_step_statistics()
        self.stat_tracker = PlanningStatTracker(self)

    # ---------------------------------------------------------------- step
    def step(self, obs):
        """``mcts.py:97-117``."""
        assert self.root.t <= self.step_limit
        if self.root.is_absorbing:
            for k in self.step_statistics:
                self.step_statistics[k] = np.nan
            return self._last_action
        self._reset_step_statistics()
        self.update(self._last_action, obs)
        self._last_action = self.get_action()
        self._step_num += 1
        self.step_statistics["mem_usage"] = psutil.Process().memory_info().rss / 1024**2
        self.stat_tracker.step()
        return self._last_action

    def reset(self):
        """``mcts.py:123-138``."""
        self.stat_tracker.reset_episode()
        self._step_num = 0
        self._engine.reset()
        self.root = RootView()
        self._min_value, self._max_value = self._initial_bounds()
        self._reset_step_statistics()
        self._last_action = None

    def _initial_bounds(self):
        kb = self.config.known_bounds
        return (kb[0], kb[1]) if kb else (float("inf"), -float("inf"))

    def _reset_step_statistics(self):
        if not hasattr(self, "_min_value"):
            self._min_value, self._max_value = self._initial_bounds()
        self.step_statistics = {
            "search_time": 0.0, "update_time": 0.0, "reinvigoration_time": 0.0,
            "evaluation_time": 0.0, "policy_calls": 0, "inference_time": 0.0,
            "search_depth": 0, "num_sims": 0, "mem_usage": 0,
            "min_value": self._min_value, "max_value": self._max_value,
            # the build's additions (SURVEY §5 metrics): the search's algorithmic
            # HBM bytes on this rank (engine.search_bytes) and its simulations/s
            "hbm_bytes": 0, "sims_per_s": 0.0,
        }

    # -------------------------------------------------------------- update
    def update(self, action, obs):
        """``mcts.py:159-263``: initial belief at t == 0, else re-root + reinvigorate."""
        if self.root.is_absorbing:
            return
        start = time.time()
        if self.root.t == 0:
            self._last_action = None
            a = -1
        else:
            a = int(action)
        key = self._emodel.obs_key(obs)
        if self._world == 1:
            absorbing = self._engine.update([a], [key])   # broadcast to every replica
            # a replica whose root is absorbing stops searching and merges as zeros;
            # the planner is absorbing once all of them are (oracle/root_parallel.py)
            done = bool(np.all(absorbing))
        else:
            # every rank must stop calling the collectives together: absorbing
            # only when every replica of every rank is, and a failed update on
            # any rank raises on all of them
            from posggym_baselines_amd.planning.parallel import raise_together
            exc, done = None, False
            try:
                done = bool(np.all(self._engine.update([a], [key])))
            except Exception as e:  # noqa: BLE001 -- re-raised after the agreement
                exc = e
            rows = raise_together(exc, [1.0 if done else 0.0], self._pg, self._device())
            done = bool(np.all(rows[:, 1] > 0))
        self.root = dataclasses.replace(self.root, t=self.root.t + 1, is_absorbing=done)
        self.step_statistics["update_time"] = time.time() - start

    # -------------------------------------------------------------- search
    def get_action(self):
        """``mcts.py:269-306`` (fixed ``num_sims``, or chunks until the time limit)."""
        if self.root.is_absorbing:
            return self.action_space[0]
        start = time.time()
        K, world = self._K, self._world
        exc, depth, n_sims = None, 0, 0
        self._hbm = 0
        try:
            depth, n_sims = self._search(start)
        except Exception as e:  # noqa: BLE001 -- raised on every rank below
            if world == 1:
                raise
            exc = e
        A = len(self.action_space)
        if world > 1:
            from posggym_baselines_amd.planning.parallel import exchange_roots, raise_together
            rows = raise_together(exc, [n_sims, depth], self._pg, self._device())
            n_sims, depth = int(rows[:, 1].sum()), int(rows[:, 2].max())
            exchange_roots(self._engine, self._device(), self._pg)
        if K == 1 and world == 1:
            st = self._engine.root_stats()[0]
            action = int(st.action)
            visits, belief_size = st.root_visits, st.belief_size
            cv, cval, ctot = (tuple(st.child_visits[:A]), tuple(st.child_values[:A]),
                              tuple(st.child_totals[:A]))
        else:
            # the merged decision (raises on every rank if any replica failed)
            st = self._engine.merge_roots(K, world=world if world > 1 else 0)[0]
            action = int(st.action)
            visits, belief_size = st.root_visits, None
            cv = tuple(int(v) for v in st.visits[:A])
            ctot = tuple(st.totals[:A])
            cval = tuple(t / v if v > 0 else 0.0 for t, v in zip(ctot, cv))
        search_time = time.time() - start
        if self._hbm is None:   # this rank's replicas' algorithmic bytes (engine.search_bytes)
            self._hbm = search_bytes(self._engine.root_stats(), A, self._engine.type_based)
        self._min_value, self._max_value = st.min_value, st.max_value
        self.root = dataclasses.replace(
            self.root, visits=visits, belief_size=belief_size, child_visits=cv,
            child_values=cval, child_totals=ctot)
        self.step_statistics.update(
            search_time=search_time, search_depth=max(depth, st.search_depth), num_sims=n_sims,
            min_value=st.min_value, max_value=st.max_value, hbm_bytes=self._hbm,
            sims_per_s=n_sims / search_time if search_time > 0 else 0.0)
        return action

    def _device(self):
        return f"cuda:{self.config.device}"

    def _search(self, start):
        """This rank's simulations of one get_action; returns (search depth
        seen by the chunk loop, simulations run by this rank's replicas)."""
        K, depth = self._K, 0
        A = len(self.action_space)
        tb = self._engine.type_based
        if self._num_sims is not None:
            self._engine.search(self._per_replica, fetch=False)
            self._hbm = None   # counted after the decision (errors surface in the merge first)
            return depth, self._per_replica * K
        # the wall-clock loop (mcts.py:285) as launches of growing chunks; the
        # final action choice is drawn once, after the last one.  A chunk is
        # never larger than the arena headroom (PomcpEngine.headroom) nor than
        # what is left of the per-search bound the arenas were sized for
        # (wall_clock_sims: the log(N) table and the kept subtree assume at most
        # that many simulations per search): when either is reached the search
        # ends early (step_statistics "arena_full"), it does not fail.
        done, chunk = 0, 16
        ceiling = self._engine.wall_clock_sims
        room = self._engine.headroom()
        while time.time() - start < self.config.search_time_limit:
            n = min(chunk, room, ceiling - done)
            if n <= 0:
                self.step_statistics["arena_full"] = True
                break
            self._engine.search(n, final=False)
            room = self._engine.headroom()    # synchronises
            depth = max(depth, self._depth())
            self._hbm += search_bytes(self._engine.root_stats(), A, tb)   # this chunk's
            done += n
            chunk = min(chunk * 2, 4096)
        self._engine.search(0, fetch=False)
        return depth, done * K

    def _depth(self):
        if self._K == 1:
            return self._engine.root_stats()[0].search_depth
        return self._engine.merge_roots(self._K)[0].search_depth

    def set_root_belief(self, rows):
        """Search from a caller-supplied belief: after ``reset()``, the root
        becomes an unexpanded node at time t holding ``rows`` ((t, v0, v1) packed
        particles, insertion order; ``pomcp_set_root_belief``) in every replica,
        in place of the initial update's b0 samples (mcts.py:175-227)."""
        rows = np.asarray(rows, dtype=np.uint32).reshape(-1, 3)
        for k in range(self._K):
            self._engine.set_root_belief(k, rows)
        self.root = RootView(t=int(rows[0, 0]), belief_size=len(rows))

    def root_belief(self, replica: int = 0):
        """Root particles as (t, v0, v1) packed u32 rows (of one replica)."""
        return self._engine.root_belief(replica)

    # ------------------------------------------------------- belief accuracy
    BELIEF_STATS = ("state", "policy", "action", "history")

    def belief_stats(self, state=None, other_policy_ids=None, other_actions=None, *, stats=None):
        """The root belief's accuracies (``BeliefStatTracker``, utils.py:292-339)
        from per-tree counts reduced on the GPU (``pomcp_belief_stats``): no
        particle leaves the device.

        ``state``: the engine model's state, a (v0, v1) pair; ``other_policy_ids``
        = {agent: true policy id}; ``other_actions`` = {agent: action just played}.
        ``stats`` names the entries wanted (default: ``state`` / ``policy`` /
        ``action`` for the arguments given, and ``history`` where it is defined).

        * ``state``   matching particles / n (get_state_accuracy, 292-297);
        * ``policy``  particles carrying the true policy id / n (309-324); 0.0
          with ``state_belief_only`` (no policy state in the particles) or when
          the id is not one of the mixture's;
        * ``action``  (sum_j hist[j] * pi_j(a)) / n, pi_j from this planner's
          ``other_agent_policies`` (326-339); 0.0 with ``state_belief_only``;
        * ``history`` 0.0 with ``state_belief_only`` (299-307 skips particles
          without a history); otherwise NotImplementedError: GPU particles carry
          no joint history.
        Every entry is 0.0 for an empty belief (227-228).  With ``root_parallel``
        = K > 1 this rank's K replicas are pooled (summed counts / summed sizes).
        """
        sbo = bool(self.config.state_belief_only)
        if stats is None:
            stats = [k for k, given in (("state", state), ("policy", other_policy_ids),
                                        ("action", other_actions)) if given is not None]
            if sbo:
                stats.append("history")
        for k in stats:
            if k not in self.BELIEF_STATS:
                raise ValueError(f"unknown belief stat {k!r}")
        if "history" in stats and not sbo:
            raise NotImplementedError(
                "belief history accuracy: the GPU particles carry no joint history "
                "(defined here only with state_belief_only, where it is 0.0)")
        if "state" in stats and state is None:
            raise ValueError("belief stat 'state' needs the true state")
        if "policy" in stats and other_policy_ids is None:
            raise ValueError("belief stat 'policy' needs other_policy_ids")
        if "action" in stats and other_actions is None:
            raise ValueError("belief stat 'action' needs other_actions")
        if "action" in stats and not sbo:
            refuse_reactive_action_accuracy(self.other_agent_policies)
        q = None
        if "state" in stats:
            q = [int(state[0]), int(state[1])]
        counts = self._engine.belief_counts(q)
        n = int(counts["belief_size"].sum(dtype=np.int64))
        out = {k: 0.0 for k in stats}
        if n == 0:
            return out
        if "state" in stats:
            out["state"] = int(counts["state_matches"].sum(dtype=np.int64)) / n
        if sbo or not ("policy" in stats or "action" in stats):
            return out
        others = [i for i in self.model.possible_agents if i != self.agent_id]
        other = others[0]   # (the engine plans for two agents: base_type_tables)
        pol = self.other_agent_policies[other]
        mixture = getattr(pol, "policies", None)
        if mixture is not None:
            ids = list(mixture)
            hist = [int(h) for h in counts["policy_hist"].sum(axis=0, dtype=np.int64)[:len(ids)]]
            states = [{"policy_id": pid, "policy_state": mixture[pid].get_initial_state()}
                      for pid in ids]
        else:
            # one stateless other-agent policy (policy state {}: no policy_id)
            ids, hist, states = [None], [n], [pol.sample_initial_state()]
        if "policy" in stats:
            pid = other_policy_ids[other]
            out["policy"] = hist[ids.index(pid)] / n if pid in ids else 0.0
        if "action" in stats:
            a = other_actions[other]
            acc = 0.0
            for j, s in enumerate(states):
                if hist[j]:
                    acc += hist[j] * pol.get_pi(s).get(a, 0.0)
            out["action"] = acc / n
        return out

    def close(self):
        self.search_policy.close()
        for p in self.other_agent_policies.values():
            p.close()
        self._engine.close()

    def __str__(self):
        return "POMCP"


def refuse_reactive_action_accuracy(other_agent_policies):
    """Belief ``action`` accuracy sums a histogram of policies times one action
    distribution each; a state-reactive policy's action depends on each
    particle's state, which would need a per-particle evaluation: not built.
    ``None``: the caller knows the planner models one."""
    if other_agent_policies is None or mixture_is_reactive(other_agent_policies):
        raise NotImplementedError(
            "belief 'action' accuracy with a state-reactive policy among the planner's other-agent "
            "policies needs a per-particle evaluation (track 'policy' and 'state')")


class BatchedPOMCP:
    """``num_trees`` independent POMCP planners searched by one launch.

    Tree ``b`` uses RNG key ``(seed, tree_key_base + b)``; each tree is
    bit-identical to a single ``POMCP`` (and to the oracle) with that key.
    """

    def __init__(self, model, agent_id, config: MCTSConfig, num_trees: int, num_sims: int,
                 *, searches: int = 1, reroot: bool = False, capacities=None, stream=None,
                 tree_key_base: int = 0, device: Optional[int] = None, type_policies=None,
                 defer_cutoff: bool = True, other_policy_ids=None):
        """defer_cutoff: defer cut-off children to the re-root (the default, the
        faster mode with or without an update after every search) or look them
        up during the search (False); same results (``pomcp_set_defer_cutoff``).
        other_policy_ids: the ids of ``type_policies``' other-agent policies in
        their order (``list(OtherAgentMixturePolicy.policies)``); kept so that
        ``run_episodes(other_agents=...)`` can tell which of a population's
        policies the planners model."""
        from posggym_baselines_amd.planning.engine import plan_capacities
        if capacities is None:
            step_limit = config.step_limit or model.spec.max_episode_steps
            capacities = plan_capacities(config, step_limit, num_sims, searches, reroot=reroot,
                                         num_actions=model.action_spaces[agent_id].n)
            self._planned = (int(searches), bool(reroot))
        else:
            self._planned = None   # the caller's own capacities: not second-guessed
        self.num_trees = num_trees
        self.num_sims = num_sims
        self.other_policy_ids = None if other_policy_ids is None else list(other_policy_ids)
        if self.other_policy_ids is not None:
            if type_policies is None or len(self.other_policy_ids) != type_policies.num_other:
                raise ValueError("other_policy_ids names type_policies' other-agent policies, "
                                 "one id each")
        self.engine = PomcpEngine(model, agent_id, config, num_trees=num_trees,
                                  capacities=capacities, stream=stream,
                                  tree_key_base=tree_key_base, device=device,
                                  type_policies=type_policies)
        self.engine.set_defer_cutoff(defer_cutoff)
        self.engine.reset()

    def init_synthetic(self, env_seed_base: int = 1000):
        """Synthetic Driving-v1 roots: per tree an env b0 sample and
        the initial belief update; snapshot so ``restore()`` can re-search them."""
        keys = self.engine.synthetic_obs(env_seed_base)
        self.engine.update(np.full(self.num_trees, -1, dtype=np.int32), keys)
        self.engine.snapshot()
        return keys

    def search(self, fetch=True):
        return self.engine.search(self.num_sims, fetch=fetch)

    def restore(self):
        self.engine.restore()

    def belief_counts(self, states=None):
        """Every tree's belief accuracy counts in one launch
        (``PomcpEngine.belief_counts``): ``states`` is [num_trees][2] (v0, v1)
        query states, or None for the sizes and policy histograms alone."""
        return self.engine.belief_counts(states)

    # ------------------------------------------------------------ episodes
    def run_episodes(self, env_seeds=None, *, until: str = "agent_done",
                     belief_states: bool = False, write_row=None, on_step=None,
                     other_agents=None, belief_acc=False, track_per_step: bool = False,
                     root_parallel: int = 1):
        """Play one episode per tree against uniform random other agents, the
        whole batch in lockstep on the device; returns one result row per tree.

        The batch's ``run_planning_episodes``: tree ``b`` plays the episode the
        serial harness plays with planner key ``(seed, tree_key_base + b)`` and
        environment seed ``env_seeds[b]`` (default ``b``) -- same actions,
        rewards, length and returns, bit for bit.  Every step is one call
        (``pomcp_episodes_step``: update from the device inputs, search,
        ``k_episode_step``) and one integer comes back, the number of trees still
        playing; a finished tree is parked while its neighbours play on.
        ``until``: "agent_done" (the planning agent is done, exp_utils.py:522) or
        "all_done" (every agent is); an episode is truncated at the model's
        ``max_episode_steps``.  As with ``planner.reset()`` in the reference, the
        planners' RNG streams are not reseeded between calls: a second call on
        the same engine continues them (a fresh engine replays the first).

        Row keys: ``EPISODE_RESULT_HEADS`` + ``env_seed``
        (``EpisodeResultsWriter(path, extra_heads=["env_seed"])`` writes them).
        ``num`` is the tree index.  ``time`` is the wall-clock time of this whole
        call and ``search_time`` / ``update_time`` are the batch's device time per
        step (mean over the steps): the BATCH's figures, the same in every row,
        not a tree's share.  ``search_depth`` / ``num_sims`` / ``min_value`` /
        ``max_value`` are the tree's means over the steps that reached the
        planner's statistics (the root was not absorbing before the step, as
        ``PlanningStatTracker`` sees them): integer sum / n, sequential FP64
        sum / n; NaN for a tree without such a step.  ``mem_usage`` is the
        process RSS (MiB); the other planner columns are 0.0.

        ``belief_states``: the kernels also write each tree's true state (the one
        its root belief is about) where ``episode_belief_counts()`` reads it, so
        ``on_step`` can track belief accuracy with no host copy of a state.
        ``write_row(row)`` is called per tree at the end; ``on_step(t, self)``
        after every step (tests: ``episode_states()`` is the debug getter).

        ``other_agents``: a population for the other agent, an ordered list of 1
        to 8 ``FixedDistributionPolicy`` or ``ShortestPathPolicy`` (Driving-v1's
        state-reactive shortest-path agents, ``pomcp_episodes_set_population_kinds``)
        with distinct ids; every tree draws its
        episode's policy from it as ``PopulationAgents`` does for the serial
        harness, on the device (``pomcp_episodes_set_population``), and the row
        gains ``other_policy_id``.  A policy whose id is one of
        ``other_policy_ids`` (the constructor's) is one the planners model.

        ``belief_acc``: the row gains the ``BeliefStatTracker`` columns
        (``get_stat_keys``: ``belief_{k}_acc``, with ``track_per_step`` also
        ``belief_{k}_acc_{t}``, NaN past the episode's end), accumulated on the
        device by ``k_episode_belief_acc`` after every step -- nothing per tree
        comes to the host between steps.  ``True`` tracks ``policy``, ``action``,
        ``state`` and ``history``; a list tracks the named ones (the tracker's
        ``stats_to_track``).  Each mean is the tree's sequential FP64 sum of its
        steps' values / their count (NaN for no step).  ``history`` is 0.0 with
        ``state_belief_only`` and raises ``NotImplementedError`` otherwise, as
        the tracker does; ``policy`` and ``action`` are 0.0 when the particles
        carry no policy (``state_belief_only``), and ``policy`` is 0.0 for a
        true policy the planners do not model (the uniform agent included).

        ``root_parallel`` = K > 1: the batch's ``num_trees = G * K`` trees are G
        root-parallel planners of K replica trees each and every PLANNER plays
        one episode (``pomcp_episodes_set_group``): ``env_seeds`` has G entries
        (default ``g``) and G rows come back, ``num`` = g.  Planner ``g`` owns
        trees ``[gK, (g+1)K)``, replica ``k`` keyed ``(seed, tree_key_base + gK +
        k)``, and the engine's ``num_sims`` is the count PER REPLICA: it plays, bit
        for bit, the episode the serial harness plays with a
        ``POMCP(root_parallel=K, num_sims=K * num_sims)`` whose replicas are keyed
        that way.  Every replica is updated with the merged action
        (``pomcp_merge_roots``' kernel, on the device) and the real observation;
        the planner's root is absorbing only when every replica's is, and a
        replica whose own root is absorbing merges as zeros while its siblings
        play on.  The planner columns of a searched step are the merged maximum
        ``search_depth``, ``num_sims`` = K * num_sims (0 for a step whose update
        made every replica absorbing) and the merged ``min_value`` /
        ``max_value``.  The population (``other_agents``) is drawn per planner,
        ``episode_states()`` returns G records, and ``episode_merged_roots()``
        the merged record of each planner's last real step (the per-replica
        ``root_stats()`` of a finished planner are unspecified).  Not combined
        with ``belief_states`` or ``belief_acc`` (``ValueError``);
        ``run_planner_queue`` is the episode queue of such planners.
        """
        check_until(until)
        K = int(root_parallel)
        if K < 1 or self.num_trees % K:
            raise ValueError(f"root_parallel={root_parallel} does not divide num_trees = "
                             f"{self.num_trees}")
        if K > 1 and (belief_states or self._belief_acc_stats(belief_acc)):
            raise ValueError("root_parallel > 1 plays without belief_states and belief_acc (the "
                             "replicas hold K beliefs about one true state)")
        B = self.num_trees // K   # episodes (and rows): one per planner
        seeds = list(range(B)) if env_seeds is None else [int(s) for s in env_seeds]
        if len(seeds) != B:
            raise ValueError(f"env_seeds has {len(seeds)} entries for {B} " +
                             ("trees" if K == 1 else f"planners of {K} replica trees"))
        max_steps = episode_guards(self, "run_episodes", until)
        acc_stats = self._belief_acc_stats(belief_acc)
        if track_per_step and not acc_stats:
            raise ValueError("track_per_step needs belief_acc")
        kinds = population_kinds(self, other_agents)
        pop_ids, pop_probs, mix = episode_population(self, other_agents, self.other_policy_ids)
        engine = self.engine

        def begin(pow_table):
            engine.episodes_set_population(pop_probs, mix)
            if kinds is not None:
                engine.episodes_set_population_kinds(kinds)
            engine.episodes_track_belief_acc(bool(acc_stats), track_per_step)
            engine.episodes_begin(seeds, pow_table, max_steps, until, track_states=belief_states,
                                  group=K)

        res, figures = play_batch(self, "run_episodes", begin, engine.episodes_results, B,
                                  max_steps, on_step)
        pops = engine.episodes_pop_states() if pop_ids is not None else None
        acc_columns = ()
        if acc_stats:
            acc = engine.episodes_belief_acc()
            acc_steps = engine.episodes_belief_acc_steps(max_steps) if track_per_step else None
            acc_columns = belief_acc_columns(acc_stats, acc, acc_steps, max_steps)
        return episode_rows(res, figures, write_row, pop_ids=pop_ids,
                            policy_index=None if pops is None else pops["policy_index"],
                            acc_columns=acc_columns)

    def run_episode_queue(self, env_seeds, *, until: str = "agent_done", other_agents=None,
                          belief_acc=False, belief_states: bool = False, write_row=None,
                          on_step=None, root_parallel: int = 1):
        """Play ``N = len(env_seeds)`` episodes (``N >= num_trees``) on the batch's
        ``num_trees`` slots; returns ``N`` rows in queue order.

        ``run_episodes`` parks a tree whose episode ends until the slowest one
        of the batch is over; here it takes the next seed of a queue that lives
        on the device (``pomcp_episodes_queue_begin``), so every slot plays until
        ``N`` episodes have been handed out.  The assignment rule: slot ``b``
        starts with entry ``b`` and ``next = num_trees``; at the end of each
        batch step the slots whose episode finished in that step take entries
        ``next, next + 1, ...`` in ascending slot order while entries remain; a
        slot that finds the queue empty is retired (parked as a finished tree
        is, its last real search's root statistics kept).

        Parity: the episodes slot ``b`` plays, in order, are bit for bit the
        episodes ``run_planning_episodes`` plays over their seeds on one planner
        keyed ``(seed, tree_key_base + b)``: the tree is reset between them as
        ``planner.reset()`` resets it and its RNG streams carry on.

        Row keys: ``run_episodes``' plus ``slot`` and ``slot_order`` (the
        episode's ordinal within its slot); ``num`` is the queue index;
        ``time`` / ``search_time`` / ``update_time`` are the whole call's and the
        batch's per-step figures.  ``until``, ``other_agents``, ``belief_acc``
        (the per-episode means; there is no per-step table in queue mode),
        ``belief_states``, ``write_row`` and ``on_step(t, self)`` are
        ``run_episodes``'.  For ``on_step``: ``episode_queue_slots()`` is the
        entry each slot is playing, and ``episode_queue_finished()`` the final
        records of the episodes that ended in the step just played (their
        slots' ``episode_states()`` are the next episodes' by then).
        ``root_parallel``: 1; a queue's slots are single trees (``ValueError``
        for groups of replicas: ``run_planner_queue`` is their queue).
        """
        check_until(until)
        if int(root_parallel) != 1:
            raise ValueError("run_episode_queue has no root_parallel groups: its slots are single "
                             "trees (run_planner_queue(root_parallel=K) is the queue of groups)")
        B = self.num_trees
        seeds = [int(s) for s in env_seeds]
        N = len(seeds)
        if N < B:
            raise ValueError(f"run_episode_queue needs at least {B} env_seeds (one per tree), "
                             f"not {N}")
        max_steps = episode_guards(self, "run_episode_queue", until)
        acc_stats = self._belief_acc_stats(belief_acc)
        kinds = population_kinds(self, other_agents)
        pop_ids, pop_probs, mix = episode_population(self, other_agents, self.other_policy_ids)
        engine = self.engine

        def begin(pow_table):
            engine.episodes_set_population(pop_probs, mix)
            if kinds is not None:
                engine.episodes_set_population_kinds(kinds)
            engine.episodes_track_belief_acc(bool(acc_stats), False)
            engine.episodes_queue_begin(seeds, pow_table, max_steps, until,
                                        track_states=belief_states)

        res, figures = play_batch(self, "run_episode_queue", begin, engine.episodes_queue_rows, B,
                                  max_steps, on_step, entries=N)
        # (the per-episode means; there is no per-step table in queue mode)
        acc_columns = belief_acc_columns(acc_stats, res["acc"], None, max_steps) if acc_stats else ()
        return episode_rows(res["res"], figures, write_row, queue=res, pop_ids=pop_ids,
                            policy_index=res["policy_index"], acc_columns=acc_columns)

    def run_planner_queue(self, env_seeds, *, root_parallel: int, until: str = "agent_done",
                          other_agents=None, write_row=None, on_step=None):
        """Play ``N = len(env_seeds)`` episodes on the batch's ``G = num_trees //
        root_parallel`` root-parallel planners (``N >= G``); returns ``N`` rows in
        queue order.

        ``run_episode_queue`` for the planners of ``run_episodes(root_parallel=
        K)``: the queue's slots are the G groups of K replica trees (group ``g``
        owns trees ``[gK, (g+1)K)``) and the engine's ``num_sims`` is the count
        per replica.  Group ``g`` starts with entry ``g``; at the end of each
        batch step the groups whose episode finished in that step take entries
        ``next, next + 1, ...`` in ascending group order while entries remain,
        and a group that finds the queue empty is retired.  A refilled group is
        reset on the device (``pomcp_episodes_group_queue_begin``): each of its
        K trees as ``planner.reset()`` resets it, the RNG streams carried on,
        its records dropped from the search waves' shared logs.

        Parity: the episodes group ``g`` plays, in order, are bit for bit the
        episodes ``run_planning_episodes`` plays over their seeds on one
        ``POMCP(root_parallel=K, num_sims=K * num_sims)`` whose replicas are
        keyed ``(seed, tree_key_base + gK + k)``.

        Row keys: ``run_episode_queue``'s; ``slot`` is the group, ``slot_order``
        the episode's ordinal within its group, ``num`` the queue index; the
        planner columns are ``run_episodes(root_parallel=K)``'s.  ``until``,
        ``other_agents`` (the policy drawn per group and entry), ``write_row`` and
        ``on_step(t, self)`` are ``run_episode_queue``'s.  For ``on_step``:
        ``episode_queue_slots()`` and ``episode_queue_finished()`` have G
        entries, ``episode_states()`` and ``episode_merged_roots()`` are the
        running episodes', and ``episode_queue_finished_merged()`` is the kept
        merged record of the episodes that ended in the step just played.  Not
        combined with ``belief_states`` or ``belief_acc``.
        """
        check_until(until)
        K = int(root_parallel)
        if K < 2:
            raise ValueError(f"run_planner_queue needs root_parallel >= 2, not {root_parallel} "
                             "(run_episode_queue plays single trees)")
        if self.num_trees % K:
            raise ValueError(f"root_parallel={root_parallel} does not divide num_trees = "
                             f"{self.num_trees}")
        G = self.num_trees // K
        seeds = [int(s) for s in env_seeds]
        N = len(seeds)
        if N < G:
            raise ValueError(f"run_planner_queue needs at least {G} env_seeds (one per planner of "
                             f"{K} replica trees), not {N}")
        max_steps = episode_guards(self, "run_planner_queue", until)
        kinds = population_kinds(self, other_agents)
        pop_ids, pop_probs, mix = episode_population(self, other_agents, self.other_policy_ids)
        engine = self.engine

        def begin(pow_table):
            engine.episodes_set_population(pop_probs, mix)
            if kinds is not None:
                engine.episodes_set_population_kinds(kinds)
            engine.episodes_track_belief_acc(False, False)
            engine.episodes_group_queue_begin(seeds, pow_table, max_steps, until, K)

        res, figures = play_batch(self, "run_planner_queue", begin, engine.episodes_queue_rows, G,
                                  max_steps, on_step, entries=N, noun="planners")
        return episode_rows(res["res"], figures, write_row, queue=res, pop_ids=pop_ids,
                            policy_index=res["policy_index"])

    def episode_queue_slots(self):
        """The queue entry each slot of a running ``run_episode_queue`` (each
        group of a ``run_planner_queue``) is playing (-1: retired).  ``on_step``
        may read it."""
        return self.engine.episodes_queue_slots()

    def episode_queue_finished(self):
        """The episodes that ended in the step just played: per slot (per group
        of a ``run_planner_queue``) the queue entry (-1: none) and the episode's
        final ``pomcp_episode_state``."""
        return self.engine.episodes_queue_finished()

    def episode_queue_finished_merged(self):
        """Per group of a running ``run_planner_queue``, the kept merged record
        (``pomcp_merged_root``, a ``PomcpMergedRoot`` array) of the episode that
        ended in the step just played; zeros for a group where none ended
        (``episode_merged_roots()`` is the next episode's by then)."""
        return self.engine.episodes_queue_finished_merged()

    def _check_sized(self, what, max_steps):
        """``episode_guards``' sizing check: the arenas planned by the constructor
        hold ``max_steps`` searches with a re-root after each."""
        if self._planned is None:
            return
        searches, reroot = self._planned
        if not reroot or searches < max_steps:
            per = "tree" if what == "run_episodes" else "episode"
            raise ValueError(
                f"{what} re-roots up to {max_steps} times per {per}: create the engine with "
                f"BatchedPOMCP(..., searches={max_steps}, reroot=True) (this one was sized with "
                f"searches={searches}, reroot={reroot})")

    def _belief_acc_stats(self, belief_acc):
        """``run_episodes``' ``belief_acc`` as the tracker's ``stats_to_track``
        ([] = off), refused as ``BeliefStatTracker`` refuses it."""
        from posggym_baselines_amd.planning.utils import BeliefStatTracker
        if belief_acc is None or belief_acc is False:
            return []
        if belief_acc is True:
            stats = list(BeliefStatTracker.TRACKABLE_BELIEF_STATS)
        else:
            stats = list(belief_acc)
            for k in stats:
                if k not in BeliefStatTracker.TRACKABLE_BELIEF_STATS:
                    raise ValueError(f"unknown belief stat {k!r}")
        if "history" in stats and not self.engine.config.state_belief_only:
            raise NotImplementedError(
                "belief history accuracy: the GPU particles carry no joint history "
                "(track it only with state_belief_only=True, where it is 0.0)")
        if "action" in stats and getattr(self.engine, "other_reactive", False):
            refuse_reactive_action_accuracy(None)
        return stats

    def episode_belief_acc(self):
        """Every tree's device belief accuracy record (``pomcp_episode_belief_acc``)
        of ``run_episodes(..., belief_acc=...)``: the three sums, the count of
        recorded steps, the error.  ``on_step`` may read it."""
        return self.engine.episodes_belief_acc()

    def episode_states(self):
        """Every tree's device episode record (``pomcp_episode_state``) as a
        structured array: the true state, the stream counters, the last actions,
        the flags and the result so far.  A debug getter.  One record per
        planner of a ``run_episodes(root_parallel=K)`` batch."""
        return self.engine.episodes_states()

    def episode_merged_roots(self):
        """Every planner's kept merged record of a ``run_episodes(root_parallel=K)``
        batch (``pomcp_episodes_merged_roots``, a ``PomcpMergedRoot`` array): the
        ``pomcp_merged_root`` of its last real step -- its root absorbing neither
        before nor after the update, no error -- zeros before the first one.
        What ``root_stats()`` is to a tree of an ungrouped batch: a finished
        planner's replicas are parked and the later searches rewrite their own
        statistics with zeros."""
        return self.engine.episodes_merged_roots()

    def episode_belief_counts(self):
        """``belief_counts`` against the true states ``run_episodes(...,
        belief_states=True)`` keeps on the device."""
        return self.engine.episodes_belief_counts()

    def close(self):
        self.engine.close()


def uct_merge(visits: np.ndarray, totals: np.ndarray) -> np.ndarray:
    """Root-parallel decision from summed (visits, total value) per action:
    argmax of mean value, lowest index on ties."""
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.where(visits > 0, totals / np.maximum(visits, 1), -math.inf)
    return np.argmax(v, axis=-1)
