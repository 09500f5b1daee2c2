"""The environment step on the device, through the device functions k_search
steps its trees with (pomcp_debug_env_step -> k_env_selftest -> Env::step and
Env::obs_key), against the host model (envs.DrivingModel /
PursuitEvasionModel, pinned to the oracle by tests/test_env_model.py): next
states, reward bits, done flag and observation key must be equal for every case.
Driving-v1 gets the cases of the CPU equivalence test (tests/driving_vec_cases.py)
plus 65,536 seeded random pairs, PursuitEvasion-v1 65,536 random pairs.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from driving_vec_cases import driving_cases, pack  # noqa: E402

pytestmark = pytest.mark.gpu

N_RANDOM = 65536
CFG = dict(discount=0.95, search_time_limit=0.1, c=math.sqrt(2), truncated=False,
           action_selection="ucb", pucb_exploration_fraction=0.25, known_bounds=None,
           step_limit=None, epsilon=0.92, seed=0, state_belief_only=True)
_PU32 = C.POINTER(C.c_uint32)


def device_step(model, cases):
    """[N, 8] uint32 rows of pomcp_debug_env_step for the ego '0'."""
    from posggym_baselines_amd import _native as N
    from posggym_baselines_amd.planning import BatchedPOMCP, MCTSConfig
    bp = BatchedPOMCP(model, "0", MCTSConfig(num_sims=16, **CFG), 4, 16)
    try:
        cases = np.ascontiguousarray(cases, dtype=np.uint32)
        out = np.zeros((len(cases), 8), dtype=np.uint32)
        rc = N.load().pomcp_debug_env_step(bp.engine._ctx, cases.ctypes.data_as(_PU32), len(cases),
                                           out.ctypes.data_as(_PU32))
        assert rc == 0, rc
    finally:
        bp.close()
    return out


def host_rows(model, cases, ctr_of_j=None):
    """The same rows from the host model, a step per case."""
    out = np.zeros((len(cases), 8), dtype=np.uint32)
    for i, (s0, s1, a0, a1, j) in enumerate(cases.tolist()):
        if ctr_of_j is not None:
            model._model_ctr.value = ctr_of_j[j]
        ts = model.step((s0, s1), {"0": a0, "1": a1})
        r = int(np.float64(ts.rewards["0"]).view(np.uint64))
        key = model.obs_key(ts.observations["0"])
        out[i] = (ts.state[0], ts.state[1], r & 0xFFFFFFFF, r >> 32, int(ts.terminations["0"]),
                  key & 0xFFFFFFFF, key >> 32, 0)
    return out


def shuffle_counters(model):
    """A model-stream counter for each value of the execution-order draw
    (driving.h drv_step2: j = model(2), the word's top bit)."""
    from posggym_baselines_amd import _native as N
    from posggym_baselines_amd.envs.driving import ENV_TREE_KEY
    words = np.zeros(64, dtype=np.uint32)
    assert N.load().pomcp_philox_words(model._env_seed, ENV_TREE_KEY, 2, 0, 64,
                                       words.ctypes.data_as(_PU32)) == 0
    j = (words >> 31).tolist()
    return {0: j.index(0), 1: j.index(1)}


def random_driving(model, n, seed):
    """Random pairs the model can hold: distinct free cells, a min-distance
    field of at most the cell's distance unless the vehicle is done."""
    rng = np.random.default_rng(seed)
    cells = [(x, y) for y in range(model.height) for x in range(model.width) if not model._wall[y][x]]
    rows = []
    for _ in range(n):
        ia, ib = rng.choice(len(cells), size=2, replace=False)
        v = []
        for (x, y) in (cells[ia], cells[ib]):
            dest = int(rng.integers(len(model.locs)))
            cur = model._dist[dest][y][x]
            flag = int(rng.integers(8))          # 1: reached, 2: crashed, else none
            flag = flag if flag in (1, 2) else 0
            mind = int(rng.integers(128)) if flag else int(rng.integers(cur + 1))
            initd = int(rng.integers(max(1, mind), 128))
            v.append(pack(x, y, int(rng.integers(4)), int(rng.integers(4)), dest, int(flag == 1),
                          int(flag == 2), mind, initd))
        rows.append((v[0], v[1], int(rng.integers(5)), int(rng.integers(5)), int(rng.integers(2))))
    return np.array(rows, dtype=np.uint32)


def random_pursuit_evasion(model, n, seed):
    rng = np.random.default_rng(seed)
    cells = [(y << 4) | x for y in range(model.height) for x in range(model.width)
             if not model._wall[y][x]]
    rows = []
    for _ in range(n):
        flag = int(rng.integers(8))              # 1: caught, 2: reached, else none
        flag = flag if flag in (1, 2) else 0
        v0 = (cells[int(rng.integers(len(cells)))] | (int(rng.integers(4)) << 8)
              | (int(rng.integers(len(model.evader_starts))) << 10)
              | (int(rng.integers(len(model.goals))) << 12) | (int(rng.integers(128)) << 14)
              | (flag << 21))
        v1 = (cells[int(rng.integers(len(cells)))] | (int(rng.integers(4)) << 8)
              | (int(rng.integers(len(model.pursuer_starts))) << 10))
        rows.append((v0, v1, int(rng.integers(4)), int(rng.integers(4)), 0))
    return np.array(rows, dtype=np.uint32)


def assert_rows_equal(got, ref, cases):
    bad = np.flatnonzero((got != ref).any(axis=1))
    assert len(bad) == 0, (len(bad), [(cases[i].tolist(), got[i].tolist(), ref[i].tolist()) for i in bad[:5]])


def test_driving_step_matches_host_model():
    from posggym_baselines_amd.envs import DrivingModel
    model = DrivingModel("14x14RoundAbout", seed=0)
    cases = np.concatenate([driving_cases(model), random_driving(model, N_RANDOM, 20261)])
    ref = host_rows(model, cases, shuffle_counters(model))
    assert_rows_equal(device_step(model, cases), ref, cases)


def test_pursuit_evasion_step_matches_host_model():
    from posggym_baselines_amd.envs import PursuitEvasionModel
    model = PursuitEvasionModel(seed=0)
    cases = random_pursuit_evasion(model, N_RANDOM, 20262)
    assert_rows_equal(device_step(model, cases), host_rows(model, cases), cases)
