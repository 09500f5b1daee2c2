"""The episode queue on the host (csrc/episode_queue.h through its twins):
``pomcp_host_log_drop`` -- k_log_drop's per-record decision -- against a numpy
filter on synthetic logs, ``pomcp_host_queue_assign`` -- k_queue_rank's
per-slot decision -- against a pure-Python restatement of the assignment rule,
a whole queue played on the CPU with the host episode twins and a scripted ego,
and the new record's size."""
import ctypes as C

import numpy as np
import pytest

from posggym_baselines_amd import _native as N
from test_episode_population_host import (CASES, DISCOUNT, EGO, env_handle, replay,
                                          scripted_ego)

ID_BITS = 26                    # csrc/pomcp_device.h kIdBits
PU32 = C.POINTER(C.c_uint32)
P32 = C.POINTER(C.c_int32)


def real_cut_base():
    """cut_base of the configuration the GPU episode tests run (pomcp_create:
    ovf_base = max_blocks * A * 6 + 1, cut_base = ovf_base + overflow_slots)."""
    from posggym_baselines_amd.planning import MCTSConfig
    from posggym_baselines_amd.planning.engine import plan_capacities
    import math
    cfg = MCTSConfig(num_sims=32, discount=0.95, search_time_limit=0.1, c=math.sqrt(2),
                     truncated=False, action_selection="ucb", pucb_exploration_fraction=0.25,
                     known_bounds=None, step_limit=None, epsilon=0.92, seed=0,
                     state_belief_only=True)
    cap = plan_capacities(cfg, 50, 32, 50, reroot=True, num_actions=5)
    cut = cap.max_blocks * 5 * 6 + 1 + cap.overflow_slots
    assert cut + cap.max_blocks * 5 < (1 << ID_BITS)
    return cut, cap.max_blocks * 5


def synthetic_log(n, rng, with_aux):
    cut, n_deferred = real_cut_base()
    lanes = rng.integers(0, 64, n, dtype=np.uint32)
    node = rng.integers(1, cut, n, dtype=np.uint32)
    deferred = rng.random(n) < 0.3
    node[deferred] = cut + rng.integers(0, n_deferred, int(deferred.sum()), dtype=np.uint32)
    ids = node | (lanes << np.uint32(ID_BITS))
    v0 = rng.integers(0, 2**32, n, dtype=np.uint32)
    v1 = rng.integers(0, 2**32, n, dtype=np.uint32)
    aux = rng.integers(0, 8, n, dtype=np.uint32) if with_aux else None
    return ids, v0, v1, aux, deferred


def masks(rng):
    return {"empty": 0, "full": 2**64 - 1, "lane0": 1, "lane63": 1 << 63,
            "random": int(rng.integers(1, 2**63)) | (1 << 17)}


@pytest.mark.parametrize("with_aux", [False, True])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2048, 2049, 5000])
def test_host_log_drop_equals_a_numpy_filter(n, with_aux):
    lib = N.load()
    rng = np.random.default_rng(1000 * n + with_aux)
    for name, mask in masks(rng).items():
        ids, v0, v1, aux, deferred = synthetic_log(n, rng, with_aux)
        if n >= 63:   # deferred records in and out of the mask, both lanes at the mask's ends
            ids[0] = (ids[0] & ((1 << ID_BITS) - 1)) | (0 << ID_BITS)
            ids[n - 1] = (ids[n - 1] & ((1 << ID_BITS) - 1)) | (63 << ID_BITS)
        keep = ((np.uint64(mask) >> (ids >> np.uint32(ID_BITS)).astype(np.uint64))
                & np.uint64(1)) == 0
        exp = [a[keep].copy() if a is not None else None for a in (ids, v0, v1, aux)]
        got = [a.copy() if a is not None else None for a in (ids, v0, v1, aux)]
        count = C.c_int64(-1)
        ptr = [a.ctypes.data_as(PU32) if a is not None else None for a in got]
        assert lib.pomcp_host_log_drop(*ptr, n, mask, C.byref(count)) == 0
        k = int(keep.sum())
        assert count.value == k, (name, n)
        for g, e in zip(got, exp):
            if g is not None:
                assert g[:k].tobytes() == e.tobytes(), (name, n)
        if name == "empty":
            assert k == n
        if name == "full":
            assert k == 0
        if name == "random" and n >= 2048:
            # deferred records were dropped and kept, by their lane tag alone
            assert (deferred & keep).any() and (deferred & ~keep).any()
    assert lib.pomcp_host_log_drop(None, None, None, None, 3, 1, C.byref(count)) == N.POMCP_E_INVALID
    assert lib.pomcp_host_log_drop(None, None, None, None, 0, 1, None) == N.POMCP_E_INVALID


# ----------------------------------------------------------- the assignment rule
def restated_assign(queue_index, finished, next_, n):
    """The rule of DESIGN.md §15 for one step: (decisions, next, refilled)."""
    out, refilled = [], 0
    for q, f in zip(queue_index, finished):
        if q < 0 or not f:
            out.append(-2)
        elif next_ < n:
            out.append(next_)
            next_ += 1
            refilled += 1
        else:
            out.append(-1)
    return out, next_, refilled


def host_assign(queue_index, finished, next_, n):
    B = len(queue_index)
    q = np.asarray(queue_index, dtype=np.int32)
    f = np.asarray(finished, dtype=np.int32)
    nx, refilled = C.c_int32(next_), C.c_int32(-1)
    out = np.full(B, 99, dtype=np.int32)
    rc = N.load().pomcp_host_queue_assign(q.ctypes.data_as(P32), f.ctypes.data_as(P32), B, n,
                                          C.byref(nx), out.ctypes.data_as(P32), C.byref(refilled))
    assert rc == 0
    return out.tolist(), nx.value, refilled.value


def test_host_queue_assign_equals_the_restatement():
    rng = np.random.default_rng(7)
    for B, n in [(1, 1), (1, 4), (6, 20), (64, 64), (65, 70), (70, 200), (1500, 1600)]:
        queue_index = list(range(B))
        next_ = B
        for step in range(60):
            finished = (rng.random(B) < 0.3).astype(int).tolist()
            if step % 7 == 3:
                finished = [1] * B      # more finished slots than entries left, sooner or later
            exp = restated_assign(queue_index, finished, next_, n)
            assert host_assign(queue_index, finished, next_, n) == exp, (B, n, step)
            next_ = exp[1]
            queue_index = [q if a == -2 else a for q, a in zip(queue_index, exp[0])]
        assert next_ == n and all(q == -1 for q in queue_index)
    lib = N.load()
    one = (C.c_int32 * 1)(0)
    nx = C.c_int32(0)    # next below the slot count: not a queue's state
    assert lib.pomcp_host_queue_assign(one, one, 1, 1, C.byref(nx), one, C.byref(nx)) == \
        N.POMCP_E_INVALID
    nx = C.c_int32(2)
    assert lib.pomcp_host_queue_assign(one, one, 2, 1, C.byref(nx), one, C.byref(nx)) == \
        N.POMCP_E_INVALID   # fewer entries than slots


# ------------------------------------------------------------ a whole queue
@pytest.mark.parametrize("env", list(CASES))
def test_a_whole_queue_on_the_cpu(env):
    """B = 6 slots, N = 20 entries, the host episode twins and a scripted ego:
    the schedule is the restatement's, every episode's environment side is the
    stand-alone episode's with that seed, every entry is played once."""
    lib = N.load()
    B, n = 6, 20
    env_id, grid, model = env_handle(env)
    seeds = [CASES[env][0][0] + 3 * i for i in range(n)]
    max_steps = CASES[env][1]
    until = N.UNTIL_AGENT_DONE
    ego = int(EGO)
    A = model.action_spaces[EGO].n
    pow_table = (C.c_double * max_steps)(*[DISCOUNT ** t for t in range(max_steps)])

    def reset(seed):
        st, key = N.PomcpEpisodeState(), C.c_uint64()
        assert lib.pomcp_host_episode_reset(env_id, C.byref(grid), ego, seed, C.byref(st),
                                            C.byref(key)) == 0
        return st

    states = [reset(seeds[b]) for b in range(B)]
    queue_index = list(range(B))
    next_ = B
    outs = {i: [] for i in range(n)}
    final = {}
    schedule = []          # (step, slot, entry that ended, decision)
    step = 0
    while any(q >= 0 for q in queue_index):
        for b in range(B):
            q = queue_index[b]
            if q < 0:
                continue
            st = states[b]
            i = N.PomcpEpisodeStepIn(root_absorbing=0, action=scripted_ego(seeds[q], st.res.len, A),
                                     search_depth=2, num_sims=8, min_value=-1.0, max_value=1.0)
            o = N.PomcpEpisodeStepOut()
            assert lib.pomcp_host_episode_step(env_id, C.byref(grid), ego, C.byref(i), pow_table,
                                               max_steps, until, C.byref(st), C.byref(o)) == 0
            assert o.stepped
            outs[q].append((o.ego_action, o.other_action, float(o.reward).hex(), o.obs_key))
        finished = [int(states[b].finished) for b in range(B)]
        got = host_assign(queue_index, finished, next_, n)
        assert got == restated_assign(queue_index, finished, next_, n), step
        for b, a in enumerate(got[0]):
            if a == -2:
                continue
            assert queue_index[b] not in final
            final[queue_index[b]] = bytes(states[b])
            schedule.append((step, b, queue_index[b], a))
            queue_index[b] = a
            if a >= 0:
                states[b] = reset(seeds[a])
        next_ = got[1]
        step += 1
        assert step <= n * max_steps
    assert sorted(final) == list(range(n))                 # every entry once
    assert sorted(a for *_, a in schedule if a >= 0) == list(range(B, n))
    assert sum(a == -1 for *_, a in schedule) == B         # every slot retired in the end
    # ascending slot order within a step, ascending entries over the steps
    handed = [(s, b, a) for s, b, _, a in schedule if a >= 0]
    assert handed == sorted(handed) and [a for *_, a in handed] == list(range(B, n))
    for i in range(n):
        st, _, ref = replay(env, seeds[i], None, until)    # the stand-alone episode
        assert outs[i] == ref, (env, i)
        assert final[i] == bytes(st), (env, i)
    assert len({len(v) for v in outs.values()}) > 1        # episodes of different lengths


# ------------------------------------------------------------------- layouts
def test_queue_row_is_128_bytes_and_the_old_records_keep_their_sizes(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    structs = {"pomcp_episode_queue_row": N.PomcpEpisodeQueueRow,
               "pomcp_episode_state": N.PomcpEpisodeState,
               "pomcp_episode_result": N.PomcpEpisodeResult,
               "pomcp_episode_pop_state": N.PomcpEpisodePopState,
               "pomcp_episode_belief_acc": N.PomcpEpisodeBeliefAcc}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "pomcp.h"', "int main(void){"]
    for st, cls in structs.items():
        lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
        for f, *_ in cls._fields_:
            lines.append(f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));')
    lines.append("return 0;}")
    (tmp_path / "probe.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"),
                    str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.run(
        [str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split("\n")
        if line)
    for st, cls in structs.items():
        assert int(out[st]) == C.sizeof(cls), st
        for f, *_ in cls._fields_:
            assert int(out[f"{st}.{f}"]) == getattr(cls, f).offset, f"{st}.{f}"
    assert int(out["pomcp_episode_queue_row"]) == 128
    dt = np.dtype(N.EPISODE_QUEUE_ROW_DTYPE)
    assert C.sizeof(N.PomcpEpisodeQueueRow) == dt.itemsize == 128
    for f, *_ in N.PomcpEpisodeQueueRow._fields_:
        assert dt.fields[f][1] == getattr(N.PomcpEpisodeQueueRow, f).offset, f
    assert C.sizeof(N.PomcpEpisodeState) == 120 and C.sizeof(N.PomcpEpisodeResult) == 80
    assert C.sizeof(N.PomcpEpisodePopState) == 8 and C.sizeof(N.PomcpEpisodeBeliefAcc) == 32
    assert N.load().pomcp_abi_version() == 7
