"""Error returns of the C ABI on a device (include/pomcp.h, include/intmcp.h):
the status code and the text of ``pomcp_last_error`` / ``intmcp_last_error``
for calls out of order, bad arguments and an arena that overflows, and that
contexts are created and destroyed cleanly many times over.  Every case is a
status the host layer or a kernel reports by design.  (The configuration
errors of the two ``create`` functions need no GPU: tests/test_capi.py.)"""
import ctypes as C
import math

import numpy as np
import pytest

from posggym_baselines_amd import _native as N

pytestmark = pytest.mark.gpu

SIMS = 16
# epsilon 0.92 at discount 0.95: depth limit 2 (tests/test_gpu_dist.py's configuration)
CFG = dict(discount=0.95, search_time_limit=0.1, c=math.sqrt(2), truncated=False,
           action_selection="ucb", pucb_exploration_fraction=0.25, known_bounds=None,
           step_limit=None, epsilon=0.92, seed=17, state_belief_only=True)


def _pomcp_engine(num_trees=2, num_sims=SIMS, **kw):
    from gpu_util import product_config, product_model
    from posggym_baselines_amd.planning.engine import PomcpEngine
    cfg = product_config(CFG, num_sims)
    assert cfg.depth_limit == 2
    return PomcpEngine(product_model("Driving-v1"), "0", cfg, num_trees=num_trees,
                       num_sims=num_sims, searches=2, **kw)


def _intmcp_engine():
    from gpu_util import product_config, product_model
    from posggym_baselines_amd.planning.intmcp import IntmcpEngine
    return IntmcpEngine(product_model("Driving-v1"), "0", product_config(CFG, SIMS), num_pairs=1,
                        num_sims=SIMS, searches=2, nesting_level=1)


def _search_once(eng, n):
    keys = eng.synthetic_obs(1000)
    eng.update(np.full(n, -1, dtype=np.int32), keys)
    return eng.search(SIMS)


@pytest.fixture(scope="module")
def pomcp():
    eng = _pomcp_engine()
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def intmcp():
    eng = _intmcp_engine()
    yield eng
    eng.close()


# ----------------------------------------------------------------------- POMCP
def test_episodes_step_before_begin(pomcp):
    live = C.c_int32()
    rc = pomcp._lib.pomcp_episodes_step(pomcp._ctx, SIMS, C.byref(live))
    assert rc == N.POMCP_E_STATE
    assert pomcp._lib.pomcp_last_error(pomcp._ctx) == b"episodes_step: pomcp_episodes_begin first"


def test_belief_stats_before_any_update(pomcp):
    pomcp.reset()
    out = (N.PomcpBeliefCounts * pomcp.num_trees)()
    assert pomcp._lib.pomcp_belief_stats(pomcp._ctx, None, out) == N.POMCP_E_STATE
    assert (pomcp._lib.pomcp_last_error(pomcp._ctx)
            == b"belief_stats: no root belief yet (update first)")


def test_episodes_belief_acc_without_tracking(pomcp):
    out = (N.PomcpEpisodeBeliefAcc * pomcp.num_trees)()
    assert pomcp._lib.pomcp_episodes_belief_acc(pomcp._ctx, out) == N.POMCP_E_STATE
    assert (pomcp._lib.pomcp_last_error(pomcp._ctx)
            == b"episodes_belief_acc: pomcp_episodes_track_belief_acc(1, ..), "
               b"then pomcp_episodes_begin")


def test_set_search_kernel_unknown_kind(pomcp):
    assert pomcp._lib.pomcp_set_search_kernel(pomcp._ctx, 7) == N.POMCP_E_INVALID
    assert pomcp._lib.pomcp_set_search_kernel(pomcp._ctx, -1) == N.POMCP_E_INVALID


def test_two_block_arena_reports_arena_then_a_new_context_searches(monkeypatch):
    """Rank 1 of tests/test_gpu_dist.py's arena test, in one process: K = 4
    replica trees with keys 4..7, 64 simulations each, 2 blocks per tree."""
    from posggym_baselines_amd.planning import engine as E
    plan = E.plan_capacities

    def tiny(*a, **kw):
        caps = plan(*a, **kw)
        caps.max_blocks = 2
        return caps
    monkeypatch.setattr(E, "plan_capacities", tiny)
    eng = _pomcp_engine(num_trees=4, num_sims=64, tree_key_base=4)
    monkeypatch.undo()
    try:
        assert eng.capacities.max_blocks == 2
        keys = eng.synthetic_obs(1000)
        eng.update(np.full(4, -1, dtype=np.int32), keys)
        out = np.zeros(4, dtype=np.int32)
        rc = eng._lib.pomcp_search(eng._ctx, 64, out.ctypes.data_as(C.POINTER(C.c_int32)))
        assert rc == N.POMCP_E_ARENA
        assert b"tree 0: arena capacity exceeded" in eng._lib.pomcp_last_error(eng._ctx)
    finally:
        eng.close()
    eng = _pomcp_engine()
    try:
        assert eng.capacities.max_blocks > 2
        actions = _search_once(eng, 2)
        assert ((0 <= actions) & (actions < eng.A)).all()
    finally:
        eng.close()


# --------------------------------------------------------------------- I-NTMCP
def test_intmcp_search_level_without_that_level(intmcp):
    rc = intmcp._lib.intmcp_search_level(intmcp._ctx, 2, SIMS, N.INTMCP_BEGIN | N.INTMCP_FINAL, None)
    assert rc == N.POMCP_E_INVALID
    assert intmcp._lib.intmcp_last_error(intmcp._ctx) == b"search_level: no level 2"


@pytest.mark.parametrize("weights,why", [
    ([0.5, -0.1, 0.2, 0.2, 0.2], b"set_search_policy: negative or NaN weight"),
    ([0.0] * 5, b"set_search_policy: weights sum to zero")], ids=["negative", "zero"])
def test_intmcp_set_search_policy_bad_weights(intmcp, weights, why):
    w = (C.c_double * 5)(*weights)
    assert intmcp._lib.intmcp_set_search_policy(intmcp._ctx, 1, 0, w) == N.POMCP_E_INVALID
    assert intmcp._lib.intmcp_last_error(intmcp._ctx) == why


def test_intmcp_get_middle_support_without_a_middle_tree(intmcp):
    ne, npart = C.c_int32(), C.c_int32()
    rc = intmcp._lib.intmcp_get_middle_support(intmcp._ctx, 0, 1, None, 0, C.byref(ne), None, 0,
                                               C.byref(npart))
    assert rc == N.POMCP_E_INVALID
    assert (intmcp._lib.intmcp_last_error(intmcp._ctx)
            == b"get_middle_support: no middle tree 1 (nesting levels >= 2)")


def test_intmcp_search_levels_unknown_flag(intmcp):
    assert intmcp._lib.intmcp_search_levels(intmcp._ctx, SIMS, SIMS, 8, None) == N.POMCP_E_INVALID


# ------------------------------------------------------------ create / destroy
@pytest.mark.parametrize("make,n", [(_pomcp_engine, 2), (_intmcp_engine, 1)],
                         ids=["pomcp", "intmcp"])
def test_create_search_destroy_eight_times(make, n):
    actions = []
    for _ in range(8):
        eng = make()
        try:
            actions.append(_search_once(eng, n).tolist())
        finally:
            eng.close()
    assert len(actions[0]) == n
    assert all(a == actions[0] for a in actions)
