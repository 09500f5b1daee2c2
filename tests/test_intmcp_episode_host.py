"""The per-pair step of the batched I-NTMCP episodes (csrc/intmcp_episode.h,
the code k_im_episode_step / k_im_episode_unpark run) through its host twins
intmcp_host_episode_step / intmcp_host_episode_unpark, on hand-made pair
headers: which fields form the planner's part of the step, which step keeps
the header's search fields, what a finishing pair saves and sets (the park)
and that the unpark restores the saved words exactly."""
import ctypes as C

import pytest

from posggym_baselines_amd import _native as N
from posggym_baselines_amd.envs import DrivingModel, PursuitEvasionModel

MAX_STEPS = 50
GAMMA = 0.95
POW = (C.c_double * MAX_STEPS)(*[GAMMA ** t for t in range(MAX_STEPS)])
# a node's info word: parent action 2, path_ok, 3 registered children (order 1, 4, 0), statistics
INFO = 2 | (1 << 4) | (3 << 5) | (1 << 8) | (4 << 11) | (0 << 14) | (1 << 26)
ABS = N.INTMCP_ABSORBING_BIT


def env_handle(env):
    if env == "Driving-v1":
        return N.ENV_DRIVING, DrivingModel().pomcp_grid()
    return N.ENV_PURSUIT_EVASION, PursuitEvasionModel().pomcp_pe_grid()


class Pair:
    """One pair's episode on the host: the records the kernel keeps per pair."""

    def __init__(self, env="Driving-v1", env_seed=3000, ego=0, until=N.UNTIL_ALL_DONE,
                 max_steps=MAX_STEPS):
        self.lib = N.load()
        self.env_id, self.grid = env_handle(env)
        self.ego, self.until, self.max_steps = ego, until, max_steps
        self.st = N.PomcpEpisodeState()
        self.kept = N.IntmcpEpisodeKept(0, -1, 0, 0, 0)
        key = C.c_uint64()
        assert self.lib.pomcp_host_episode_reset(self.env_id, C.byref(self.grid), ego, env_seed,
                                                 C.byref(self.st), C.byref(key)) == 0

    def step(self, root):
        out = N.PomcpEpisodeStepOut()
        nxt = C.c_int32(99)
        assert self.lib.intmcp_host_episode_step(
            self.env_id, C.byref(self.grid), self.ego, C.byref(root), C.byref(self.kept), POW,
            self.max_steps, self.until, None, None, C.byref(self.st), C.byref(out),
            C.byref(nxt)) == 0
        return out, nxt.value

    def pomcp_step(self, st, root):
        """episode_step.h alone on a copy of the record: the yardstick for the
        fields im_episode_step_in takes from the pair."""
        i = N.PomcpEpisodeStepIn(root_absorbing=1 if root.info & ABS else 0,
                                 action=root.last_action, search_depth=root.search_depth,
                                 num_sims=root.num_sims, error=root.err,
                                 min_value=root.min_value, max_value=root.max_value)
        out = N.PomcpEpisodeStepOut()
        assert self.lib.pomcp_host_episode_step(self.env_id, C.byref(self.grid), self.ego,
                                                C.byref(i), POW, self.max_steps, self.until,
                                                C.byref(st), C.byref(out)) == 0
        return out


def root(action=3, sims=16, depth=7, err=0, mn=-1.5, mx=2.25, info=INFO):
    return N.IntmcpEpisodeRoot(last_action=action, num_sims=sims, search_depth=depth, err=err,
                               min_value=mn, max_value=mx, info=info)


def copy_state(st):
    c = N.PomcpEpisodeState()
    C.memmove(C.byref(c), C.byref(st), C.sizeof(st))
    return c


def raw(x):
    return bytes(memoryview(x).cast("B"))


@pytest.mark.parametrize("env", ["Driving-v1", "PursuitEvasion-v1"])
def test_a_searched_step_is_the_pomcp_step_on_the_pairs_fields(env):
    p = Pair(env, 3000 if env == "Driving-v1" else 2000)
    ref_st = copy_state(p.st)
    r = root()
    out, nxt = p.step(r)
    ref = p.pomcp_step(ref_st, root())
    assert raw(p.st) == raw(ref_st) and raw(out) == raw(ref)
    assert out.stepped == 1 and out.ego_action == 3 and nxt == 3
    res = p.st.res
    assert (res.len, res.searched_steps, res.num_sims_sum, res.search_depth_sum) == (1, 1, 16, 7)
    assert (res.min_value_sum, res.max_value_sum) == (-1.5, 2.25)
    assert p.st.finished == 0 and p.st.root_absorbing == 0
    # a real step: the header's search fields are kept, the root is left alone
    assert (p.kept.last_action, p.kept.num_sims, p.kept.search_depth) == (3, 16, 7)
    assert p.kept.parked == 0 and r.info == INFO


def test_a_step_whose_update_made_the_root_absorbing_is_searched_then_the_tail_is_not():
    p = Pair()
    p.step(root())
    # the update made the root absorbing: the search ran no simulation and wrote
    # action 0 (k_im_search on an absorbing root); the step still reaches the statistics
    r = root(action=0, sims=0, depth=0, info=INFO | ABS)
    out, nxt = p.step(r)
    assert out.stepped == 1 and out.ego_action == 0 and nxt == 0
    assert (p.st.res.len, p.st.res.searched_steps, p.st.res.num_sims_sum) == (2, 2, 16)
    assert p.st.root_absorbing == 1 and p.st.finished == 0
    assert (p.kept.last_action, p.kept.num_sims, p.kept.search_depth) == (0, 0, 0)
    assert p.kept.parked == 0 and r.info == INFO | ABS
    # absorbing before the step: the last action again, nothing reaches the statistics
    before = p.st.res.min_value_sum
    out, nxt = p.step(root(action=0, sims=0, depth=0, info=INFO | ABS))
    assert out.stepped == 1 and out.ego_action == 0 and nxt == 0
    assert (p.st.res.len, p.st.res.searched_steps, p.st.res.num_sims_sum) == (3, 2, 16)
    assert p.st.res.min_value_sum == before
    assert (p.kept.last_action, p.kept.num_sims, p.kept.search_depth) == (0, 0, 0)


def test_an_error_finishes_the_pair_without_a_park():
    p = Pair()
    p.step(root())
    r = root(action=-1, sims=5, depth=2, err=N.POMCP_E_ARENA)
    out, nxt = p.step(r)
    assert out.stepped == 0 and nxt == N.INTMCP_SKIP
    assert p.st.finished == 1 and p.st.res.error == N.POMCP_E_ARENA and p.st.res.len == 1
    # not a real step: the kept fields are the last good search's; the root is untouched
    assert (p.kept.last_action, p.kept.num_sims, p.kept.search_depth) == (3, 16, 7)
    assert p.kept.parked == 0 and r.info == INFO
    changed = C.c_int32(9)
    assert p.lib.intmcp_host_episode_unpark(C.byref(r), C.byref(p.kept), C.byref(changed)) == 0
    assert changed.value == 0 and r.info == INFO and r.last_action == -1


@pytest.mark.parametrize("tail", [False, True])
def test_park_then_unpark_restores_the_saved_words_exactly(tail):
    """Truncation after 2 steps finishes the pair: the root's info word is saved
    and gains the absorbing bit, the next update action is INTMCP_SKIP; later
    steps change nothing; the unpark puts back the info word and the header
    fields of the pair's last step (tail: that step found the root absorbing
    already, and its search fields are the zeros every such search writes)."""
    p = Pair(max_steps=2)
    info2 = INFO | (ABS if tail else 0)
    p.step(root(action=0, sims=0, depth=0, info=info2) if tail else root())
    r = root(action=0, sims=0, depth=0, info=info2) if tail else root(action=1, sims=12, depth=4)
    want = (r.last_action, r.num_sims, r.search_depth)
    out, nxt = p.step(r)
    assert out.stepped == 1 and p.st.finished == 1 and p.st.res.truncated == 1
    assert nxt == N.INTMCP_SKIP
    assert p.kept.parked == 1 and p.kept.info == info2 and r.info == info2 | ABS
    assert (p.kept.last_action, p.kept.num_sims, p.kept.search_depth) == want
    # while parked: a search of the absorbing root rewrites the three fields
    st0, kept0 = raw(p.st), raw(p.kept)
    for _ in range(3):
        r.last_action, r.num_sims, r.search_depth = 0, 0, 0
        before = raw(r)
        out, nxt = p.step(r)
        assert out.stepped == 0 and nxt == N.INTMCP_EPISODE_KEEP_INPUT
        assert (raw(p.st), raw(p.kept), raw(r)) == (st0, kept0, before)
    changed = C.c_int32()
    assert p.lib.intmcp_host_episode_unpark(C.byref(r), C.byref(p.kept), C.byref(changed)) == 0
    assert changed.value == 1 and p.kept.parked == 0
    assert r.info == info2 and (r.last_action, r.num_sims, r.search_depth) == want
    # idempotent
    after = raw(r)
    assert p.lib.intmcp_host_episode_unpark(C.byref(r), C.byref(p.kept), C.byref(changed)) == 0
    assert changed.value == 0 and raw(r) == after


def test_a_population_draws_the_other_agents_action():
    """PursuitEvasion against a one-policy population that always plays action
    2: the other agent's action is the population's."""
    lib = N.load()
    env_id, grid = env_handle("PursuitEvasion-v1")
    pop = N.PomcpEpisodePopulation()
    pop.num_policies = 1
    for a, v in enumerate([0.0, 0.0, 1.0, 0.0]):
        pop.pi[0][a] = v
    ps = N.PomcpEpisodePopState()
    st = N.PomcpEpisodeState()
    key = C.c_uint64()
    assert lib.pomcp_host_episode_reset_pop(env_id, C.byref(grid), 0, 2000, C.byref(pop),
                                            C.byref(st), C.byref(ps), C.byref(key)) == 0
    kept = N.IntmcpEpisodeKept(0, -1, 0, 0, 0)
    out = N.PomcpEpisodeStepOut()
    nxt = C.c_int32()
    r = root(action=1)
    assert lib.intmcp_host_episode_step(env_id, C.byref(grid), 0, C.byref(r), C.byref(kept), POW,
                                        MAX_STEPS, N.UNTIL_AGENT_DONE, C.byref(pop), C.byref(ps),
                                        C.byref(st), C.byref(out), C.byref(nxt)) == 0
    assert out.stepped == 1 and (out.ego_action, out.other_action) == (1, 2)
    assert nxt.value == (N.INTMCP_SKIP if st.finished else 1)


def test_bad_arguments_are_refused():
    lib = N.load()
    p = Pair()
    out, nxt, r = N.PomcpEpisodeStepOut(), C.c_int32(), root()
    args = [p.env_id, C.byref(p.grid), 0, C.byref(r), C.byref(p.kept), POW, MAX_STEPS,
            N.UNTIL_ALL_DONE, None, None, C.byref(p.st), C.byref(out), C.byref(nxt)]
    for i, bad in ((0, 99), (2, 2), (3, None), (4, None), (6, 0), (7, 5), (10, None), (12, None)):
        a = list(args)
        a[i] = bad
        assert lib.intmcp_host_episode_step(*a) == N.POMCP_E_INVALID, i
    assert lib.intmcp_host_episode_unpark(None, C.byref(p.kept), C.byref(nxt)) == N.POMCP_E_INVALID


def test_pinned_layouts_and_abi_version_are_unchanged():
    lib = N.load()
    assert lib.pomcp_abi_version() == 7 == N.POMCP_ABI_VERSION
    assert C.sizeof(N.PomcpEpisodeResult) == 80
    assert C.sizeof(N.PomcpEpisodeState) == 120
    assert C.sizeof(N.PomcpEpisodePopState) == 8
    assert C.sizeof(N.IntmcpEpisodeRoot) == 40 and C.sizeof(N.IntmcpEpisodeKept) == 32
    assert N.INTMCP_SKIP == -2


def test_the_new_symbols_resolve():
    lib = N.load()
    bound = {s[0] for s in N.INTMCP_SIGNATURES}
    for name in ("intmcp_episodes_set_population", "intmcp_episodes_begin", "intmcp_episodes_step",
                 "intmcp_episodes_results", "intmcp_episodes_states", "intmcp_episodes_pop_states",
                 "intmcp_episodes_timing", "intmcp_host_episode_step",
                 "intmcp_host_episode_unpark"):
        assert hasattr(lib, name) and name in bound, name
    # without a context every entry point refuses
    live = C.c_int32()
    assert lib.intmcp_episodes_step(None, 8, C.byref(live)) == N.POMCP_E_INVALID
    assert lib.intmcp_episodes_begin(None, None, None, 1, 0) == N.POMCP_E_INVALID
    assert lib.intmcp_episodes_results(None, None) == N.POMCP_E_INVALID
