"""CooperativeReaching-v0 generative model -- the build's restatement (pure
Python), with the interface of ``oracle/driving.py`` (``streams``,
``pack_words``) so that the real reference planners run on it
(``oracle.ref_harness.make_reference_pomcp / _mcts / _potmmcp``).

TEST INFRASTRUCTURE.  posggym owns the real CooperativeReaching-v0; its source
is absent, so the dynamics below are the build's documented choices (DESIGN.md
§21), pinned only where the reference's data allows (the returns 0, 0.75, 1.0
of its ``br_results.csv``).  ``csrc/cooperative_reaching.h`` restates this file.

An agent is ``(x, y, start x, start y)``; a state is the two agents.  An
observation is ``((x, y), (ox, oy))``, the other agent's position
``(size, size)`` when ``obs_distance`` is an integer and the Chebyshev distance
exceeds it.
"""
from oracle.driving import Discrete, JointTimestep, Spec
from oracle.rng import S_ACT_BASE, S_MODEL

DO_NOTHING, UP, DOWN, LEFT, RIGHT = range(5)
NUM_ACTIONS = 5
MAX_EPISODE_STEPS = 50
GOAL_VALUES = (1.0, 1.0, 0.75, 0.75)
_DX = (0, 0, 0, -1, 1)
_DY = (0, -1, 1, 0, 0)


def pack_obs(obs) -> int:
    (x, y), (ox, oy) = obs
    return x | (y << 4) | (ox << 8) | (oy << 12)


class CooperativeReachingModel:
    """CooperativeReaching-v0 restatement (2 agents, four corner goals)."""

    env_id = "CooperativeReaching-v0"
    pack_obs = staticmethod(pack_obs)

    def __init__(self, streams, size=5, obs_distance=None):
        assert 3 <= size <= 8
        self.size = size
        self.obs_distance = obs_distance
        s = size - 1
        self.goals = ((0, 0), (s, s), (0, s), (s, 0))
        self.goal_values = GOAL_VALUES
        # the non-goal cells in row-major order
        self.free_cells = [(x, y) for y in range(size) for x in range(size)
                           if (x, y) not in self.goals]
        self.possible_agents = ("0", "1")
        self.num_agents = 2
        self.streams = streams
        self.action_spaces = {str(i): Discrete(NUM_ACTIONS, streams, S_ACT_BASE + i)
                              for i in range(2)}
        self.spec = Spec("CooperativeReaching-v0", MAX_EPISODE_STEPS)

    # -- packed words (csrc/cooperative_reaching.h) ---------------------------
    def pack_agent(self, a) -> int:
        x, y, sx, sy = a
        g = self.goals.index((x, y)) + 1 if (x, y) in self.goals else 0
        return x | (y << 3) | (sx << 6) | (sy << 9) | (g << 12)

    def pack_words(self, state):
        return self.pack_agent(state[0]), self.pack_agent(state[1])

    # -- the model -----------------------------------------------------------
    def _draw_cell(self):
        return self.free_cells[self.streams.randint(S_MODEL, len(self.free_cells))]

    def sample_initial_state(self):
        c0 = self._draw_cell()
        c1 = self._draw_cell()
        return (c0 + c0, c1 + c1)

    def _obs(self, state, i):
        me, other = state[i], state[1 - i]
        hidden = self.obs_distance is not None and \
            max(abs(other[0] - me[0]), abs(other[1] - me[1])) > self.obs_distance
        return ((me[0], me[1]), (self.size, self.size) if hidden else (other[0], other[1]))

    def sample_initial_obs(self, state):
        return {str(i): self._obs(state, i) for i in range(2)}

    def sample_agent_initial_state(self, agent_id, obs):
        """The ego from its observation (start = position); the other agent from
        the observation when it is seen, else drawn like an initial cell and
        rejected until the ego's observation matches (<= 64 tries, then the last
        draw)."""
        i = int(agent_id)
        own, oth = obs
        ego = tuple(own) + tuple(own)
        if tuple(oth) != (self.size, self.size):
            other = tuple(oth) + tuple(oth)
        else:
            other = None
            for _ in range(64):
                c = self._draw_cell()
                other = c + c
                pair = (ego, other) if i == 0 else (other, ego)
                if self._obs(pair, i) == (tuple(own), tuple(oth)):
                    break
        return (ego, other) if i == 0 else (other, ego)

    def _move(self, a, action):
        last = self.size - 1
        x = min(max(a[0] + _DX[action], 0), last)
        y = min(max(a[1] + _DY[action], 0), last)
        return (x, y, a[2], a[3])

    def step(self, state, actions):
        n0 = self._move(state[0], actions["0"])
        n1 = self._move(state[1], actions["1"])
        nxt = (n0, n1)
        r, done = 0.0, False
        if n0[:2] == n1[:2] and n0[:2] in self.goals:
            r, done = self.goal_values[self.goals.index(n0[:2])], True
        obs = {str(i): self._obs(nxt, i) for i in range(2)}
        return JointTimestep(nxt, obs, {"0": r, "1": r}, {"0": done, "1": done},
                             {"0": False, "1": False}, done, {})


def run_episode(env, planner_step, ego="0", other_agent="random", max_steps=MAX_EPISODE_STEPS):
    """One episode on ``env`` (a model on its own streams), in the trace format of
    ``oracle.episode.run_episode``.  ``planner_step(obs) -> action`` plays
    ``ego``; the other agent is uniform random on its environment-policy stream
    (``other_agent="random"``) or the heuristic agent whose registry id
    ``other_agent`` is, acting on the state."""
    from oracle.episode import fhex
    from oracle.rng import S_ENV_POLICY_BASE
    other = [i for i in env.possible_agents if i != ego][0]
    heuristic = None
    if other_agent != "random":
        from posggym_baselines_amd.planning.policies import GoalHeuristicPolicy
        heuristic = GoalHeuristicPolicy.from_id(env, other, other_agent)
    state = env.sample_initial_state()
    obs = env.sample_initial_obs(state)
    steps, ret = [], 0.0
    for _ in range(max_steps):
        a_ego = planner_step(obs[ego])
        if heuristic is not None:
            a_oth = heuristic.action_from_state(state)
        else:
            a_oth = env.streams.randint(S_ENV_POLICY_BASE + int(other), env.action_spaces[other].n)
        actions = {ego: a_ego, other: a_oth}
        ts = env.step(state, actions)
        ret += ts.rewards[ego]
        steps.append({"obs": env.pack_obs(obs[ego]),
                      "actions": [actions[i] for i in env.possible_agents],
                      "reward": fhex(ts.rewards[ego])})
        state, obs = ts.state, ts.observations
        if ts.all_done:
            break
    return {"steps": steps, "return": fhex(ret), "len": len(steps)}
