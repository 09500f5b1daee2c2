"""PredatorPrey-v0 generative model -- the build's restatement (pure Python),
with the interface of ``tests/golden/coop_reaching_model.py`` (``streams``,
``pack_words``) so that the real reference planners run on it
(``oracle.ref_harness.make_reference_pomcp / _mcts / _potmmcp``).

TEST INFRASTRUCTURE.  posggym owns the real PredatorPrey-v0; its source is
absent, so the dynamics below are the build's documented choices (DESIGN.md
§23), pinned only where the reference's data allows (the returns 0, 1/3, 2/3, 1
in multiples of ``float32(1/3)`` and the 50-step limit of its
``br_results.csv``).  ``csrc/predator_prey.h`` restates this file.

A state is ``(predator 0, predator 1, (prey 0, prey 1, prey 2))``, every entity
an ``(x, y)`` and a caught or absent prey ``None``.  An observation is the tuple
of the ``(2 * obs_dim + 1) ** 2 - 1`` cells around the predator, row-major:
0 empty, 1 off the grid, 2 predator, 3 prey; then one entry more: 1 when no
prey is left (the step's terminal flag).
"""
import struct

from oracle.driving import Discrete, JointTimestep, Spec
from oracle.rng import S_ACT_BASE, S_MODEL

DO_NOTHING, UP, DOWN, LEFT, RIGHT = range(5)
NUM_ACTIONS = 5
MAX_EPISODE_STEPS = 50
MAX_PREY = 3
STEP_RANGE = 1 << 25
GRID_SIZES = {"5x5": 5, "10x10": 10}
_DX = (0, 0, 0, -1, 1)
_DY = (0, -1, 1, 0, 0)


def capture_reward(num_prey):
    """(double)(float)(1.0 / num_prey)"""
    return struct.unpack("f", struct.pack("f", 1.0 / num_prey))[0]


def pack_obs(obs) -> int:
    key = 0
    for i, c in enumerate(obs):
        key |= c << (2 * i)
    return key


def _dist(a, b):
    return abs(a[0] - b[0]) + abs(a[1] - b[1])


class PredatorPreyModel:
    """PredatorPrey-v0 restatement (2 predators, 1..3 prey, open grid)."""

    env_id = "PredatorPrey-v0"
    pack_obs = staticmethod(pack_obs)

    def __init__(self, streams, grid="10x10", num_prey=3, prey_strength=2, obs_dim=2):
        assert grid in GRID_SIZES and 1 <= num_prey <= 3 and 1 <= prey_strength <= 2
        assert 1 <= obs_dim <= 2
        self.grid = grid
        self.size = S = GRID_SIZES[grid]
        self.num_prey = num_prey
        self.prey_strength = prey_strength
        self.obs_dim = obs_dim
        self.reward = capture_reward(num_prey)
        l, h = S - 1, S // 2
        # row-major: the corners and the edge cells at x or y = S // 2
        self.start_cells = ((0, 0), (h, 0), (l, 0), (0, h), (l, h), (0, l), (h, l), (l, l))
        if S == 5:      # the centre and its 4-neighbours
            self.block = [(x, y) for y in range(S) for x in range(S)
                          if abs(x - h) + abs(y - h) <= 1]
        else:           # the central (S - 4) x (S - 4) cells
            self.block = [(x, y) for y in range(2, S - 2) for x in range(2, S - 2)]
        self.possible_agents = ("0", "1")
        self.num_agents = 2
        self.streams = streams
        self.action_spaces = {str(i): Discrete(NUM_ACTIONS, streams, S_ACT_BASE + i)
                              for i in range(2)}
        self.spec = Spec("PredatorPrey-v0", MAX_EPISODE_STEPS)
        # what the steps taken so far did (the generator's conditions)
        self.facts = {"rules": [0, 0, 0], "blocked_order": [0, 0], "captures": 0}

    # -- packed words (csrc/predator_prey.h) ----------------------------------
    def _cell(self, p):
        return 0 if p is None else p[1] * self.size + p[0]

    def pack_words(self, state):
        p0, p1, prey = state
        caught = sum(1 << k for k in range(MAX_PREY) if prey[k] is None)
        w0 = self._cell(p0) | (self._cell(prey[0]) << 7) | (self._cell(prey[1]) << 14) | \
            (caught << 21)
        return w0, self._cell(p1) | (self._cell(prey[2]) << 7)

    def unpack_words(self, words):
        w0, w1 = words
        S = self.size
        xy = lambda c: (c % S, c // S)
        caught = (w0 >> 21) & 7
        cells = ((w0 >> 7) & 127, (w0 >> 14) & 127, (w1 >> 7) & 127)
        prey = tuple(None if (caught >> k) & 1 else xy(cells[k]) for k in range(MAX_PREY))
        return (xy(w0 & 127), xy(w1 & 127), prey)

    # -- the model -----------------------------------------------------------
    def _draw(self, n):
        return self.streams.randint(S_MODEL, n)

    def _draw_prey(self):
        prey = []
        for k in range(self.num_prey):
            free = [c for c in self.block if c not in prey]
            prey.append(free[self._draw(len(self.block) - k)])
        return tuple(prey + [None] * (MAX_PREY - self.num_prey))

    def sample_initial_state(self):
        i0 = self._draw(8)
        i1 = self._draw(7)
        i1 += i1 >= i0
        return (self.start_cells[i0], self.start_cells[i1], self._draw_prey())

    def _obs(self, state, i):
        d, S = self.obs_dim, self.size
        me, other = state[i], state[1 - i]
        out = []
        for dy in range(-d, d + 1):
            for dx in range(-d, d + 1):
                if dx == 0 and dy == 0:
                    continue
                c = (me[0] + dx, me[1] + dy)
                if not (0 <= c[0] < S and 0 <= c[1] < S):
                    out.append(1)
                elif c in state[2]:
                    out.append(3)
                elif c == other:
                    out.append(2)
                else:
                    out.append(0)
        out.append(int(all(q is None for q in state[2])))      # no prey left: the terminal flag
        return tuple(out)

    def sample_initial_obs(self, state):
        return {str(i): self._obs(state, i) for i in range(2)}

    def sample_agent_initial_state(self, agent_id, obs):
        """The agent on the start cell whose off-grid pattern is the
        observation's (ValueError: none); the other predator and the prey drawn
        as the initial state draws them and rejected until the whole observation
        matches (<= 64 tries, then the last draw)."""
        i = int(agent_id)
        obs = tuple(obs)
        walls = tuple(c == 1 for c in obs[:-1])
        empty = (None,) * MAX_PREY
        si = None
        for k, c in enumerate(self.start_cells):
            far = (-9, -9)
            if tuple(v == 1 for v in self._obs((c, far, empty), 0)[:-1]) == walls:
                si = k
                break
        if si is None or len(obs) != (2 * self.obs_dim + 1) ** 2 or obs[-1] != 0:
            raise ValueError("observation inconsistent with the model")
        ego = self.start_cells[si]
        state = None
        for _ in range(64):
            k = self._draw(7)
            k += k >= si
            other = self.start_cells[k]
            prey = self._draw_prey()
            state = (ego, other, prey) if i == 0 else (other, ego, prey)
            if self._obs(state, i) == obs:
                break
        return state

    def step_draw(self, state, actions, j, facts=None):
        """The joint step under the model draw ``j`` (``< 2 ** 25``): the next
        state and the number of prey caught."""
        S, d = self.size, self.obs_dim
        pred = [state[0], state[1]]
        prey = list(state[2])
        facts = self.facts if facts is None else facts
        # 1. live prey in index order, each seeing the moves already made
        for k in range(MAX_PREY):
            q = prey[k]
            if q is None:
                continue
            near = [(i, _dist(q, pred[i])) for i in range(2) if _dist(q, pred[i]) <= d]
            others = [prey[i] for i in range(MAX_PREY)
                      if i != k and prey[i] is not None and _dist(q, prey[i]) <= 1]
            if near:
                target, rule = pred[min(near, key=lambda t: (t[1], t[0]))[0]], 0
            elif others:
                target, rule = others[0], 1
            else:
                target, rule = None, 2
            cand = []
            for a in range(5):
                c = (q[0] + _DX[a], q[1] + _DY[a])
                if a == 0 or (0 <= c[0] < S and 0 <= c[1] < S and c not in pred
                              and all(c != prey[i] for i in range(MAX_PREY) if i != k)):
                    cand.append(c)
            if target is not None:
                best = max(_dist(c, target) for c in cand)
                cand = [c for c in cand if _dist(c, target) == best]
            byte = (j >> (8 * k)) & 255
            prey[k] = cand[(byte * len(cand)) >> 8]
            facts["rules"][rule] += 1
        # 2. the predators in the order bit 24 gives
        order = (j >> 24) & 1
        for i in ((1, 0) if order else (0, 1)):
            a = actions[i]
            c = (pred[i][0] + _DX[a], pred[i][1] + _DY[a])
            if 0 <= c[0] < S and 0 <= c[1] < S and c != pred[1 - i] and c not in prey:
                pred[i] = c
            elif a != 0:
                facts["blocked_order"][order] += 1
        # 3. captures
        n = 0
        for k in range(MAX_PREY):
            if prey[k] is not None and \
                    sum(_dist(prey[k], p) == 1 for p in pred) >= self.prey_strength:
                prey[k] = None
                n += 1
        facts["captures"] += n
        return (pred[0], pred[1], tuple(prey)), n

    def step(self, state, actions):
        j = self._draw(STEP_RANGE)
        nxt, n = self.step_draw(state, (actions["0"], actions["1"]), j)
        r = n * self.reward
        done = all(q is None for q in nxt[2])
        obs = {str(i): self._obs(nxt, i) for i in range(2)}
        return JointTimestep(nxt, obs, {"0": r, "1": r}, {"0": done, "1": done},
                             {"0": False, "1": False}, done, {})


def run_episode(env, planner_step, ego="0", max_steps=MAX_EPISODE_STEPS):
    """One episode on ``env`` (a model on its own streams), in the trace format of
    ``oracle.episode.run_episode``.  ``planner_step(obs) -> action`` plays
    ``ego``; the other predator is uniform random on its environment-policy
    stream."""
    from oracle.episode import fhex
    from oracle.rng import S_ENV_POLICY_BASE
    other = [i for i in env.possible_agents if i != ego][0]
    state = env.sample_initial_state()
    obs = env.sample_initial_obs(state)
    steps, ret = [], 0.0
    for _ in range(max_steps):
        a_ego = planner_step(obs[ego])
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
