"""The episode queue of root-parallel planners on the host:
``pomcp_host_group_drop_masks`` -- csrc/episode_group_queue.h, the per-tree
decision k_group_queue_trees takes and the search waves' drop masks it forms --
against a pure-Python restatement: tree b belongs to group b // K, a group that
takes a new entry (assign >= 0) sets the bits of all its trees, bit b % 64 of
mask b // 64; retiring (-1) and playing (-2) groups set none."""
import ctypes as C

import numpy as np
import pytest

from posggym_baselines_amd import _native as N

PLAYING, RETIRE = -2, -1     # csrc/episode_queue.h kQueuePlaying, kQueueRetire
P32 = C.POINTER(C.c_int32)
PU64 = C.POINTER(C.c_uint64)


def restated(assign, K, num_trees):
    masks = [0] * ((num_trees + 63) // 64)
    for b in range(num_trees):
        if assign[b // K] >= 0:
            masks[b // 64] |= 1 << (b % 64)
    return masks


def twin(assign, G, K, num_trees=None):
    num_trees = G * K if num_trees is None else num_trees
    a = np.ascontiguousarray(np.asarray(assign, dtype=np.int32))
    out = np.full((num_trees + 63) // 64, 0xDEADBEEF, dtype=np.uint64)
    rc = N.load().pomcp_host_group_drop_masks(a.ctypes.data_as(P32), G, K, num_trees,
                                              out.ctypes.data_as(PU64))
    assert rc == 0
    return [int(m) for m in out]


def test_groups_of_three_group_21_has_bits_in_two_masks():
    K, G = 3, 24
    assign = [PLAYING] * G
    assign[21] = 40                       # trees 63, 64, 65
    got = twin(assign, G, K)
    assert got == restated(assign, K, G * K) == [1 << 63, 0b11]
    # its neighbours in either wave, a retiring and a playing group next to them
    assign = [PLAYING] * G
    assign[20], assign[21], assign[22], assign[23], assign[0] = 24, RETIRE, 25, PLAYING, RETIRE
    got = twin(assign, G, K)
    assert got == restated(assign, K, G * K) == [0b111 << 60, 0b111 << 2]


def test_groups_of_seventy_share_the_middle_wave():
    K, G = 70, 2
    full = (1 << 64) - 1
    assert twin([5, PLAYING], G, K) == restated([5, PLAYING], K, 140) == [full, 0b111111, 0]
    # wave 1 is split at bit 6; wave 2 holds the last 12 trees
    assert twin([PLAYING, 5], G, K) == restated([PLAYING, 5], K, 140) == \
        [0, full & ~0b111111, (1 << 12) - 1]
    assert twin([2, 3], G, K) == [full, full, (1 << 12) - 1]
    assert twin([RETIRE, 3], G, K) == [0, full & ~0b111111, (1 << 12) - 1]


def test_groups_of_sixty_four_are_whole_waves():
    K, G = 64, 3
    full = (1 << 64) - 1
    for assign in ([PLAYING, 7, RETIRE], [3, PLAYING, 4], [RETIRE, RETIRE, 9]):
        got = twin(assign, G, K)
        assert got == restated(assign, K, G * K) == [full if a >= 0 else 0 for a in assign]


@pytest.mark.parametrize("K,G", [(3, 24), (70, 2), (64, 3), (2, 33), (5, 6), (129, 3)])
def test_none_all_and_random_assignments(K, G):
    B = G * K
    assert twin([PLAYING] * G, G, K) == [0] * ((B + 63) // 64)
    assert twin([RETIRE] * G, G, K) == [0] * ((B + 63) // 64)
    every = twin(list(range(G, 2 * G)), G, K)
    assert every == restated(list(range(G, 2 * G)), K, B)
    assert sum(bin(m).count("1") for m in every) == B      # every tree, nothing past the last
    rng = np.random.default_rng(19 + K)
    for _ in range(20):
        kind = rng.integers(0, 3, size=G)
        assign = [PLAYING if k == 0 else RETIRE if k == 1 else int(rng.integers(0, 1000))
                  for k in kind]
        assert twin(assign, G, K) == restated(assign, K, B)


def test_arguments_are_checked():
    lib = N.load()
    a = (C.c_int32 * 2)(PLAYING, 0)
    out = (C.c_uint64 * 3)()
    assert lib.pomcp_host_group_drop_masks(None, 2, 70, 140, out) == N.POMCP_E_INVALID
    assert lib.pomcp_host_group_drop_masks(a, 2, 70, 140, None) == N.POMCP_E_INVALID
    assert lib.pomcp_host_group_drop_masks(a, 2, 70, 139, out) == N.POMCP_E_INVALID
    assert lib.pomcp_host_group_drop_masks(a, 0, 70, 0, out) == N.POMCP_E_INVALID
    assert lib.pomcp_host_group_drop_masks(a, 2, 0, 0, out) == N.POMCP_E_INVALID
    bad = (C.c_int32 * 2)(-3, 0)
    assert lib.pomcp_host_group_drop_masks(bad, 2, 70, 140, out) == N.POMCP_E_INVALID
    assert lib.pomcp_host_group_drop_masks(a, 2, 70, 140, out) == 0
