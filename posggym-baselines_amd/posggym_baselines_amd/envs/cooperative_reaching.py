"""CooperativeReaching-v0 model, product side.

As for the other models, the planner only needs the model's description (grid
size, goals, observation distance) to configure the GPU engine; the dynamics
run on the device (``csrc/cooperative_reaching.h``) and the same header is
exposed on the host through the C ABI (``pomcp_cr_step`` /
``pomcp_cr_sample_initial_state`` / ``pomcp_cr_obs``) for episode loops.

posggym's CooperativeReaching-v0 is not available in this build environment;
the dynamics are the build's documented restatement, parity
with posggym unpinned; the returns {0, 0.75, 1.0} are the ones the reference's
own ``baseline_exps/env_data/CooperativeReaching-v0`` results hold.  Agents
``'0'`` and ``'1'`` on a ``size`` x ``size`` grid with a goal in every corner;
actions DO_NOTHING, UP, DOWN, LEFT, RIGHT; both agents on one goal cell end
the episode with that goal's value for both.

A state is two packed words (csrc/cooperative_reaching.h): position, start cell
and the goal the agent stands on.  An observation is ``((x, y), (ox, oy))``,
the other agent's position ``(size, size)`` beyond ``obs_distance``.
"""
import ctypes as C

import numpy as np

from posggym_baselines_amd.envs.driving import Discrete, JointTimestep, Spec

NUM_ACTIONS = 5
MAX_EPISODE_STEPS = 50
ENV_TREE_KEY = 0x40000000
DO_NOTHING, UP, DOWN, LEFT, RIGHT = range(5)
GOAL_VALUES = (1.0, 1.0, 0.75, 0.75)


def goal_cells(size):
    """The four goals in index order: two of value 1.0 on one diagonal, two of
    value 0.75 on the other."""
    s = int(size) - 1
    return ((0, 0), (s, s), (0, s), (s, 0))


def pack_obs(obs) -> int:
    """((x, y), (ox, oy)) -> 16-bit key (cooperative_reaching.h layout)."""
    (x, y), (ox, oy) = obs
    return int(x) | (int(y) << 4) | (int(ox) << 8) | (int(oy) << 12)


def unpack_obs(key: int):
    key = int(key)
    return ((key & 15, (key >> 4) & 15), ((key >> 8) & 15, (key >> 12) & 15))


class CooperativeReachingModel:
    """CooperativeReaching-v0 (``size``, ``num_goals=4``, ``mode="original"``,
    ``obs_distance``)."""

    env_id = "CooperativeReaching-v0"

    def __init__(self, size=5, num_goals=4, mode="original", obs_distance=None, seed=0):
        if mode != "original":
            raise NotImplementedError(f"CooperativeReaching-v0 mode {mode!r} is not restated "
                                      "(only 'original')")
        if num_goals != 4:
            raise NotImplementedError(f"CooperativeReaching-v0 num_goals={num_goals} is not "
                                      "restated (only 4: the corners)")
        if isinstance(size, bool) or int(size) != size or not 3 <= int(size) <= 8:
            raise NotImplementedError(f"CooperativeReaching-v0 size={size} is not restated (3..8)")
        if obs_distance is not None and (isinstance(obs_distance, bool)
                                         or int(obs_distance) != obs_distance
                                         or not 0 <= int(obs_distance) <= 7):
            raise NotImplementedError(f"CooperativeReaching-v0 obs_distance={obs_distance} is not "
                                      "restated (None or 0..7)")
        self.size = int(size)
        self.num_goals = 4
        self.mode = mode
        self.obs_distance = None if obs_distance is None else int(obs_distance)
        self.goals = goal_cells(self.size)
        self.goal_values = GOAL_VALUES
        self.possible_agents = ("0", "1")
        self.action_spaces = {a: Discrete(NUM_ACTIONS, None if seed is None else seed + i)
                              for i, a in enumerate(self.possible_agents)}
        self.spec = Spec("CooperativeReaching-v0", MAX_EPISODE_STEPS)
        self._grid = None
        self.seed(seed)

    # -- engine description -------------------------------------------------
    def pomcp_cr_grid(self):
        from posggym_baselines_amd._native import PomcpCrGrid
        if self._grid is None:
            g = PomcpCrGrid()
            g.size = self.size
            g.obs_distance = -1 if self.obs_distance is None else self.obs_distance
            g.num_goals = self.num_goals
            for k, (x, y) in enumerate(self.goals):
                g.goal[k][0], g.goal[k][1] = x, y
                g.goal_value[k] = self.goal_values[k]
            self._grid = g
        return self._grid

    def configure_engine(self, cfg):
        """Fill the environment part of a ``pomcp_config`` (the description itself
        goes beside it: ``engine_env_desc``)."""
        from posggym_baselines_amd._native import ENV_COOPERATIVE_REACHING
        cfg.env_id = ENV_COOPERATIVE_REACHING

    def engine_env_desc(self):
        """What ``pomcp_create_env`` takes beside the config."""
        return self.pomcp_cr_grid()

    def obs_key(self, obs) -> int:
        return obs if isinstance(obs, (int, np.integer)) else pack_obs(obs)

    def obs_from_key(self, key: int):
        return unpack_obs(key)

    # -- host environment (same cooperative_reaching.h through the C ABI) ----
    def seed(self, seed=0):
        self._env_seed = 0 if seed is None else int(seed)
        self._model_ctr = C.c_uint32(0)

    def sample_initial_state(self):
        from posggym_baselines_amd._native import check, load
        out = (C.c_uint32 * 2)()
        check(load().pomcp_cr_sample_initial_state(
            C.byref(self.pomcp_cr_grid()), self._env_seed, ENV_TREE_KEY,
            C.byref(self._model_ctr), out))
        return (int(out[0]), int(out[1]))

    def sample_initial_obs(self, state):
        from posggym_baselines_amd._native import check, load
        st = (C.c_uint32 * 2)(*state)
        keys = (C.c_uint64 * 2)()
        check(load().pomcp_cr_obs(C.byref(self.pomcp_cr_grid()), st, keys))
        return {a: self.obs_from_key(keys[i]) for i, a in enumerate(self.possible_agents)}

    def step(self, state, actions):
        from posggym_baselines_amd._native import check, load
        st = (C.c_uint32 * 2)(*state)
        act = (C.c_int32 * 2)(*[int(actions[a]) for a in self.possible_agents])
        nxt = (C.c_uint32 * 2)()
        rew = (C.c_double * 2)()
        term = (C.c_int32 * 2)()
        keys = (C.c_uint64 * 2)()
        check(load().pomcp_cr_step(C.byref(self.pomcp_cr_grid()), st, act, nxt, rew, term, keys))
        agents = self.possible_agents
        terms = {a: bool(term[i]) for i, a in enumerate(agents)}
        return JointTimestep(
            (int(nxt[0]), int(nxt[1])),
            {a: self.obs_from_key(keys[i]) for i, a in enumerate(agents)},
            {a: float(rew[i]) for i, a in enumerate(agents)},
            terms, {a: False for a in agents}, all(terms.values()), {})
