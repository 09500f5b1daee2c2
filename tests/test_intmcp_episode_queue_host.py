"""The episode queue of the batched I-NTMCP episodes on the host: the per-slot
refill decision (csrc/intmcp_episode.h im_episode_refill, the code
k_im_queue_refill runs) through its twin intmcp_host_episode_refill -- a new
entry, a retired slot, a slot still playing, and a slot parked by
intmcp_host_episode_step in the same step -- and a whole small queue played
through pomcp_host_queue_assign plus the twin against the assignment rule
restated in Python."""
import ctypes as C

from posggym_baselines_amd import _native as N
from test_intmcp_episode_host import INFO, Pair, raw, root

ABS = N.INTMCP_ABSORBING_BIT
PLAYING, RETIRE = -2, -1          # csrc/episode_queue.h kQueuePlaying / kQueueRetire
KEEP = N.INTMCP_EPISODE_KEEP_INPUT
NEW = ("intmcp_reset_pairs", "intmcp_episodes_queue_begin", "intmcp_episodes_queue_rows",
       "intmcp_episodes_queue_slots", "intmcp_episodes_queue_finished",
       "intmcp_episodes_queue_timing", "intmcp_host_episode_refill")


def refill(assign, kept):
    nxt, did = C.c_int32(99), C.c_int32(99)
    assert N.load().intmcp_host_episode_refill(assign, C.byref(kept), C.byref(nxt),
                                               C.byref(did)) == 0
    return nxt.value, did.value


def test_the_new_symbols_resolve_and_are_bound():
    lib = N.load()
    bound = {s[0] for s in N.INTMCP_SIGNATURES}
    for name in NEW:
        assert hasattr(lib, name) and name in bound, name
    for name in ("intmcp_debug_arena_scan", "intmcp_debug_queue_cleared_bytes"):
        assert hasattr(lib, name) and name in {s[0] for s in N.DEBUG_SIGNATURES}, name


def test_every_new_entry_point_refuses_a_null_context():
    lib = N.load()
    one = (C.c_int32 * 1)(0)
    seeds = (C.c_uint64 * 1)(1)
    pw = (C.c_double * 1)(1.0)
    rows = (N.PomcpEpisodeQueueRow * 1)()
    st = (N.PomcpEpisodeState * 1)()
    ms = (C.c_double * 2)()
    scan = (C.c_int64 * 3)()
    assert lib.intmcp_reset_pairs(None, one, 1) == N.POMCP_E_INVALID
    assert lib.intmcp_episodes_queue_begin(None, seeds, 1, pw, 1, 0) == N.POMCP_E_INVALID
    assert lib.intmcp_episodes_queue_rows(None, rows) == N.POMCP_E_INVALID
    assert lib.intmcp_episodes_queue_slots(None, one) == N.POMCP_E_INVALID
    assert lib.intmcp_episodes_queue_finished(None, st, one) == N.POMCP_E_INVALID
    assert lib.intmcp_episodes_queue_timing(None, ms) == N.POMCP_E_INVALID
    assert lib.intmcp_debug_arena_scan(None, 0, 0, scan) == N.POMCP_E_INVALID
    assert lib.intmcp_debug_queue_cleared_bytes(None, scan) == N.POMCP_E_INVALID
    # the twin's own arguments
    kept = N.IntmcpEpisodeKept(0, -1, 0, 0, 0)
    nxt, did = C.c_int32(), C.c_int32()
    assert lib.intmcp_host_episode_refill(0, None, C.byref(nxt), C.byref(did)) == N.POMCP_E_INVALID
    assert lib.intmcp_host_episode_refill(0, C.byref(kept), None, C.byref(did)) == N.POMCP_E_INVALID
    assert lib.intmcp_host_episode_refill(0, C.byref(kept), C.byref(nxt), None) == N.POMCP_E_INVALID
    assert lib.intmcp_host_episode_refill(-3, C.byref(kept), C.byref(nxt),
                                          C.byref(did)) == N.POMCP_E_INVALID


def test_the_three_cases_of_the_refill():
    # a new entry: the side record cleared, an initial update next
    kept = N.IntmcpEpisodeKept(INFO, 3, 16, 7, 1, (C.c_int32 * 3)(5, 6, 7))
    assert refill(12, kept) == (-1, 1)
    assert raw(kept) == raw(N.IntmcpEpisodeKept(0, -1, 0, 0, 0))
    assert refill(0, kept) == (-1, 1)          # (entry 0 is an entry)
    # retired, still playing: nothing changes, the update input stays
    for assign in (RETIRE, PLAYING):
        for parked in (0, 1):
            kept = N.IntmcpEpisodeKept(INFO, 3, 16, 7, parked)
            before = raw(kept)
            assert refill(assign, kept) == (KEEP, 0)
            assert raw(kept) == before


def test_a_slot_parked_in_the_same_step_and_refilled_is_not_unparked_later():
    """Truncation after 2 steps parks the pair (intmcp_host_episode_step); the
    queue hands its slot a new entry in the same step."""
    p = Pair(max_steps=2)
    p.step(root())
    r = root(action=1, sims=12, depth=4)
    out, nxt = p.step(r)
    assert p.st.finished == 1 and nxt == N.INTMCP_SKIP
    assert p.kept.parked == 1 and p.kept.info == INFO and r.info == INFO | ABS
    nxt, did = refill(7, p.kept)
    assert (nxt, did) == (-1, 1) and p.kept.parked == 0
    # the new episode's root, as the per-pair reset writes it: the unpark at the
    # end of the batch leaves it alone
    fresh = root(action=-1, sims=0, depth=0, info=1 << 4)
    before = raw(fresh)
    changed = C.c_int32(9)
    assert p.lib.intmcp_host_episode_unpark(C.byref(fresh), C.byref(p.kept), C.byref(changed)) == 0
    assert changed.value == 0 and raw(fresh) == before
    # a retired slot instead stays parked and is restored
    q = Pair(max_steps=2)
    q.step(root())
    r = root(action=1, sims=12, depth=4)
    q.step(r)
    assert refill(RETIRE, q.kept) == (KEEP, 0) and q.kept.parked == 1
    r.last_action, r.num_sims, r.search_depth = 0, 0, 0
    assert q.lib.intmcp_host_episode_unpark(C.byref(r), C.byref(q.kept), C.byref(changed)) == 0
    assert changed.value == 1 and r.info == INFO
    assert (r.last_action, r.num_sims, r.search_depth) == (1, 12, 4)


def restated_schedule(B, lens):
    """The assignment rule on the episodes' lengths: per entry (slot, ordinal,
    start step), the refill sets per step and the step each slot retires at."""
    n = len(lens)
    out = [None] * n
    cur, left, order = list(range(B)), [lens[b] for b in range(B)], [0] * B
    for b in range(B):
        out[b] = (b, 0, 0)
    nxt, t, refills, retired = B, 0, [], {}
    while any(q >= 0 for q in cur):
        now = set()
        for b in range(B):
            if cur[b] >= 0:
                left[b] -= 1
        for b in range(B):
            if cur[b] >= 0 and left[b] == 0:
                if nxt < n:
                    order[b] += 1
                    cur[b], left[b] = nxt, lens[nxt]
                    out[nxt] = (b, order[b], t + 1)
                    now.add(b)
                    nxt += 1
                else:
                    cur[b] = -1
                    retired[b] = t
        refills.append(now)
        t += 1
    return out, refills, retired


def test_a_whole_queue_on_the_host_equals_the_restated_rule():
    """6 slots, 15 entries with scripted lengths (several slots finishing in
    one step, a step in which nothing finishes, the queue running dry while
    slots still play)."""
    lib = N.load()
    B, n = 6, 15
    lens = [3, 1, 3, 5, 1, 2, 2, 4, 1, 1, 3, 2, 6, 1, 2]
    slot_q = (C.c_int32 * B)(*range(B))
    finished = (C.c_int32 * B)()
    assign = (C.c_int32 * B)()
    nxt, refilled = C.c_int32(B), C.c_int32()
    left = [lens[b] for b in range(B)]
    order, start = [0] * B, [0] * B
    kept = [N.IntmcpEpisodeKept(0, -1, 0, 0, 0) for _ in range(B)]
    in_action = [-1] * B
    got, refills, retired = [None] * n, [], {}
    t = 0
    while any(q >= 0 for q in slot_q):
        assert t < 100
        # the step: a playing slot's next action is its ego's (here 1); a slot that
        # finishes is parked as im_episode_step parks it
        for b in range(B):
            if slot_q[b] < 0:
                continue
            left[b] -= 1
            finished[b] = 1 if left[b] == 0 else 0
            in_action[b] = N.INTMCP_SKIP if finished[b] else 1
            if finished[b]:
                kept[b].parked, kept[b].info = 1, INFO
        assert lib.pomcp_host_queue_assign(slot_q, finished, B, n, C.byref(nxt), assign,
                                           C.byref(refilled)) == 0
        now = set()
        for b in range(B):
            a = assign[b]
            if a != PLAYING:
                got[slot_q[b]] = (b, order[b], start[b])
                slot_q[b] = a
                if a == RETIRE:
                    retired[b] = t
            na, did = refill(a, kept[b])
            assert did == (1 if a >= 0 else 0)
            if did:
                now.add(b)
                order[b] += 1
                start[b] = t + 1
                left[b] = lens[a]
                finished[b] = 0
                assert kept[b].parked == 0
            if na != KEEP:
                in_action[b] = na
        assert refilled.value == len(now)
        # refilled slots start with an initial update, retired ones stay skipped
        for b in range(B):
            want = -1 if b in now else N.INTMCP_SKIP if slot_q[b] < 0 else 1
            assert in_action[b] == want, (t, b)
            assert kept[b].parked == (1 if slot_q[b] < 0 else 0)
        refills.append(now)
        t += 1
    exp, exp_refills, exp_retired = restated_schedule(B, lens)
    assert got == exp and refills == exp_refills and retired == exp_retired
    assert nxt.value == n and sorted(retired) == list(range(B))
    assert any(len(r) >= 2 for r in refills) and any(not r for r in refills[:-1])
    assert min(retired.values()) < max(retired.values())


def test_abi_and_row_layout_are_unchanged():
    assert N.load().pomcp_abi_version() == 7 == N.POMCP_ABI_VERSION
    assert C.sizeof(N.PomcpEpisodeQueueRow) == 128
    assert C.sizeof(N.IntmcpEpisodeKept) == 32
