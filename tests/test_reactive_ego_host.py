"""State-reactive EGO policies, host side (no GPU): the prior
line the kernel writes (csrc/tm_prior.h through its host twin) against the
meta-policy's ``get_expected_action_probs`` and every policy's ``get_pi`` as
exact doubles -- the build's restatement always, the reference's own class when
it is present -- the table builders, and the refusals."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from golden_util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = "CooperativeReaching-v0"
H = [f"{ENV}/H{k}-v0" for k in range(1, 6)]
EGO, OTHER = "0", "1"
FIXED_EGO = [0.1, 0.3, 0.1, 0.1, 0.4]
MIXED = {"ego": {H[3]: None, "e_fixed": FIXED_EGO, H[0]: None},
         "meta": {H[0]: {H[3]: 0.5, "e_fixed": 0.25, H[0]: 0.25},
                  H[4]: {"e_fixed": 0.4, H[0]: 0.6},
                  "o_fixed": {H[0]: 0.2, H[3]: 0.3, "e_fixed": 0.5}}}


def p0(name):
    with open(os.path.join(GOLDEN, "reactive_ego", "p0_meta_policy.json")) as f:
        return {"ego": {h: None for h in H}, "meta": json.load(f)["meta_policy"][name]}


SETS = {"greedy": p0("greedy"), "softmax": p0("softmax"), "uniform": p0("uniform"),
        "mixed": MIXED}


def product(size=5, obs_distance=None):
    from posggym_baselines_amd.envs import CooperativeReachingModel
    return CooperativeReachingModel(size=size, obs_distance=obs_distance)


def ego_policy(model, agent, pid, row):
    from posggym_baselines_amd.planning.policies import FixedDistributionPolicy, GoalHeuristicPolicy
    if row is None:
        return GoalHeuristicPolicy.from_id(model, agent, pid)
    return FixedDistributionPolicy(model, agent, pid, row)


def meta_policy(model, ego, spec, cls=None):
    from posggym_baselines_amd.planning import POTMMCPMetaPolicy
    pols = {k: ego_policy(model, ego, k, v) for k, v in spec["ego"].items()}
    return (cls or POTMMCPMetaPolicy)(model, ego, pols, {k: dict(v) for k, v in spec["meta"].items()})


def mixture(model, other, spec):
    from posggym_baselines_amd.planning import OtherAgentMixturePolicy
    return OtherAgentMixturePolicy(model, other, {
        k: ego_policy(model, other, k, None if k in H else [0.3, 0.1, 0.1, 0.4, 0.1])
        for k in spec["meta"]})


def host_lines(model, tp, code, words):
    """pomcp_host_cr_prior_lines: [len(words)][5] doubles."""
    from posggym_baselines_amd import _native as N
    lib = N.load()
    desc = model.engine_env_desc()
    kinds = N.PomcpPolicyKinds()
    for k, (kind, p0_, p1_) in enumerate(tp.ego_kinds):
        kinds.kind[k], kinds.param0[k], kinds.param1[k] = kind, p0_, p1_
    w = (C.c_double * N.POMCP_MAX_TYPE_POLICIES)(*tp.ego_meta_weights)
    own = np.asarray(words, dtype=np.uint32)
    out = np.zeros((len(own), 5), dtype=np.float64)
    rc = lib.pomcp_host_cr_prior_lines(
        C.byref(desc), tp.num_ego, C.cast(tp.ego_pi, C.POINTER(C.c_double)),
        C.cast(tp.expected_prior, C.POINTER(C.c_double)), C.byref(kinds), w, code, len(own),
        own.ctypes.data_as(C.POINTER(C.c_uint32)), out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0
    return out


def words_and_states(size):
    """Every (start, position) pair of the grid: the ego's packed word and the
    heuristics' policy state."""
    cells = [(x, y) for y in range(size) for x in range(size)]
    out = []
    for sx, sy in cells:
        for x, y in cells:
            out.append((x | (y << 3) | (sx << 6) | (sy << 9), {"start": (sx, sy), "pos": (x, y)}))
    return out


@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("size", [4, 5])
def test_prior_line_equals_the_meta_policy_at_every_start_and_position(name, size):
    from oracle.ref_harness import import_reference, reference_available
    from posggym_baselines_amd.planning.potmmcp import type_policy_tables
    spec = SETS[name]
    model = product(size)
    metas = [meta_policy(model, EGO, spec)]
    if reference_available():      # the reference's own class over the same policies
        metas.append(meta_policy(model, EGO, spec, import_reference().POTMMCPMetaPolicy))
    tp = type_policy_tables(model, EGO, metas[0], mixture(model, OTHER, spec))
    pairs = words_and_states(size)
    words = [w for w, _ in pairs]
    ids = list(spec["ego"])
    lines = [host_lines(model, tp, code, words) for code in range(len(ids) + 1)]
    seen = set()
    for meta in metas:
        for i, (_, ps) in enumerate(pairs):
            state = {k: (ps if spec["ego"][k] is None else {}) for k in ids}
            exp = meta.get_expected_action_probs(None, state)
            assert lines[0][i].tolist() == [exp[a] for a in range(5)], (name, ps)
            seen.add(tuple(lines[0][i].tolist()))
            for k, pid in enumerate(ids):
                pi = meta.policies[pid].get_pi(state[pid]).probs
                assert lines[k + 1][i].tolist() == [pi[a] for a in range(5)], (name, pid, ps)
    assert len(seen) > 4                  # the expected prior is a function of the node
    assert not any(list(s) == [0.2] * 5 for s in seen) or name == "uniform"


def test_table_builders_attach_the_kinds_and_leave_fixed_sets_alone():
    from posggym_baselines_amd import _native as N
    from posggym_baselines_amd.planning import MCTSConfig, SearchPolicyWrapper
    from posggym_baselines_amd.planning.ipomcp import base_type_tables
    from posggym_baselines_amd.planning.other_policy import RandomOtherAgentPolicy
    from posggym_baselines_amd.planning.policies import (FixedDistributionPolicy,
                                                         GoalHeuristicPolicy)
    from posggym_baselines_amd.planning.potmmcp import expected_meta_weights, type_policy_tables
    model = product()
    K = N.POLICY_CR_GOAL
    spec = SETS["mixed"]
    meta = meta_policy(model, EGO, spec)
    tp = type_policy_tables(model, EGO, meta, mixture(model, OTHER, spec))
    assert tp.ego_kinds == [(K, 3, 0), (N.POLICY_FIXED, 0, 0), (K, 0, 0)]
    assert list(tp.ego_pi[0])[:5] == [0.2] * 5 and list(tp.ego_pi[1])[:5] == FIXED_EGO
    assert list(tp.expected_prior)[:5] == [0.2] * 5          # placeholders nothing reads
    assert tp.ego_meta_weights == expected_meta_weights(meta)
    assert abs(sum(tp.ego_meta_weights) - 1.0) < 1e-12
    assert tp.other_kinds == [(K, 0, 0), (K, 4, 0), (N.POLICY_FIXED, 0, 0)]
    soft = type_policy_tables(model, EGO, meta_policy(model, EGO, SETS["softmax"]),
                              mixture(model, OTHER, SETS["softmax"]))
    assert soft.ego_kinds == [(K, r, 0) for r in range(5)]
    # a fixed-only ego set: what it was, and no ego call is made
    fixed = {"ego": {"a": FIXED_EGO, "u": [0.2] * 5},
             "meta": {H[0]: {"a": 0.5, "u": 0.5}, H[1]: {"u": 1.0}}}
    fmeta = meta_policy(model, EGO, fixed)
    ftp = type_policy_tables(model, EGO, fmeta, mixture(model, OTHER, fixed))
    assert ftp.ego_kinds is None and ftp.ego_meta_weights is None
    exp = fmeta.get_expected_action_probs(None, fmeta.get_initial_state())
    assert list(ftp.expected_prior)[:5] == [exp[a] for a in range(5)]
    # the base planner: one search policy, weight 1.0
    cfg = MCTSConfig(discount=0.95, search_time_limit=0.1, c=1.4, truncated=False,
                     action_selection="pucb", state_belief_only=True)
    rnd = {OTHER: RandomOtherAgentPolicy(model, OTHER)}
    h3 = SearchPolicyWrapper(GoalHeuristicPolicy.from_id(model, EGO, H[2]))
    btp = base_type_tables(model, EGO, cfg, rnd, h3)
    assert btp.ego_kinds == [(K, 2, 0)] and btp.ego_meta_weights == [1.0]
    assert (btp.no_meta_draw, btp.ego_uniform, btp.num_ego) == (1, 0, 1)
    ftab = base_type_tables(model, EGO, cfg, rnd, SearchPolicyWrapper(
        FixedDistributionPolicy(model, EGO, "f", FIXED_EGO)))
    assert ftab.ego_kinds is None and list(ftab.ego_pi[0])[:5] == FIXED_EGO


def test_refusals():
    from posggym_baselines_amd.envs import DrivingModel
    from posggym_baselines_amd.planning import MCTSConfig, SearchPolicyWrapper
    from posggym_baselines_amd.planning.ipomcp import base_type_tables
    from posggym_baselines_amd.planning.other_policy import RandomOtherAgentPolicy
    from posggym_baselines_amd.planning.policies import GoalHeuristicPolicy, ShortestPathPolicy
    from posggym_baselines_amd.planning.potmmcp import type_policy_tables
    model, drv = product(), DrivingModel()
    cfg = MCTSConfig(discount=0.95, search_time_limit=0.1, c=1.4, truncated=False,
                     action_selection="pucb", state_belief_only=True)
    # a Driving shortest-path ego policy: the message it had
    sp = SearchPolicyWrapper(ShortestPathPolicy(drv, EGO, "sp", 0.8))
    with pytest.raises(NotImplementedError, match="other agent only, not as the search"):
        base_type_tables(drv, EGO, cfg, {OTHER: RandomOtherAgentPolicy(drv, OTHER)}, sp)
    # a heuristic built for the other agent used as the ego's
    spec = dict(SETS["mixed"])
    wrong = meta_policy(model, EGO, spec)
    wrong.policies[H[0]] = GoalHeuristicPolicy.from_id(model, OTHER, H[0])
    with pytest.raises(NotImplementedError, match="planning agent"):
        type_policy_tables(model, EGO, wrong, mixture(model, OTHER, spec))
    with pytest.raises(NotImplementedError, match="planning agent"):
        base_type_tables(model, EGO, cfg, {OTHER: RandomOtherAgentPolicy(model, OTHER)},
                         SearchPolicyWrapper(GoalHeuristicPolicy.from_id(model, OTHER, H[1])))
    # an ego heuristic on another environment than the planner's
    with pytest.raises(NotImplementedError, match="Driving-v1"):
        base_type_tables(drv, EGO, cfg, {OTHER: RandomOtherAgentPolicy(drv, OTHER)},
                         SearchPolicyWrapper(GoalHeuristicPolicy.from_id(model, EGO, H[1])))


def test_host_twin_rejects_bad_arguments():
    from posggym_baselines_amd import _native as N
    lib = N.load()
    model = product()
    desc = model.engine_env_desc()
    pi = (C.c_double * (8 * 8))(*([0.2] * 64))
    prior = (C.c_double * 8)(*([0.2] * 8))
    w = (C.c_double * 8)(*([0.5] * 8))
    own = (C.c_uint32 * 1)(0)
    out = (C.c_double * 5)()
    kinds = N.PomcpPolicyKinds()
    call = lambda n_ego, code: lib.pomcp_host_cr_prior_lines(
        C.byref(desc), n_ego, pi, prior, C.byref(kinds), w, code, 1, own, out)
    assert call(2, 0) == 0 and list(out) == [0.2] * 5
    assert call(0, 0) == N.POMCP_E_INVALID and call(9, 0) == N.POMCP_E_INVALID
    assert call(2, 3) == N.POMCP_E_INVALID and call(2, -1) == N.POMCP_E_INVALID
    kinds.kind[0], kinds.param0[0] = N.POLICY_CR_GOAL, 5
    assert call(2, 0) == N.POMCP_E_INVALID
    kinds.kind[0], kinds.param0[0] = N.POLICY_DRIVING_SHORTEST_PATH, 1
    assert call(2, 0) == N.POMCP_E_INVALID


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_prior_line_header_is_clean_under_the_sanitizers(tmp_path):
    """tests/native/tm_prior_sanitize.cpp walks csrc/tm_prior.h over every
    4-bit cell and start cell, every code and mixes of fixed and reactive
    policies at both ends of the count, compiled with ASan + UBSan."""
    exe = tmp_path / "tm_prior_sanitize"
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall",
         "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "include"),
         os.path.join(ROOT, "tests", "native", "tm_prior_sanitize.cpp"), "-o", str(exe)],
        check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    calls, bad = (int(x) for x in r.stdout.split())
    assert calls > 100000 and bad == 0
