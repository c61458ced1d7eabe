"""The ranking a workgroup of pair_cull_kernel hands its receivers out by (csrc/csf_handout.h), on the host: csf_handout_ranks
computes weight, classes and ranks with the kernel's own functions and constants, a wave's ballots spelled out as masks.  The
ranks of the receivers that have candidates must be a permutation of 0 .. n_wanted - 1 - a rank shared by two receivers would
leave one of them without its visit -, ordered by weight class, by index within a class; receivers without candidates get none."""
import ctypes as C

import numpy as np
import pytest

from cyclistsocialforce_amd import _ffi

T = (32, 16, 8)      # csf_handout.h: HANDOUT_T0 / T1 / T2


def ranks(cand, inside):
    lib = _ffi.load()
    cand, inside = np.ascontiguousarray(cand, dtype=np.uint32), np.ascontiguousarray(inside, dtype=np.uint32)
    n = len(cand)
    rank, weight = np.full(n, -7, dtype=np.int32), np.full(n, -7, dtype=np.int32)
    p32, pi = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    got = lib.csf_handout_ranks(cand.ctypes.data_as(p32), inside.ctypes.data_as(p32), n, rank.ctypes.data_as(pi), weight.ctypes.data_as(pi))
    return got, rank, weight


def weight_of(cand, inside):
    """sift passes: pairs of inside batches at 3, pairs of the others (+ an odd inside one) at 4"""
    ni = bin(cand & inside).count("1")
    rest = bin(cand & ~inside & 0xFFFFFFFF).count("1") + (ni & 1)
    return 3 * (ni // 2) + 4 * ((rest + 1) // 2)


def check(cand, inside):
    got, rank, weight = ranks(cand, inside)
    wanted = np.nonzero(np.asarray(cand) != 0)[0]
    assert got == len(wanted)
    assert (rank[np.asarray(cand) == 0] == -1).all()
    assert sorted(rank[wanted].tolist()) == list(range(len(wanted)))
    assert [int(w) for w in weight] == [weight_of(int(c), int(i)) for c, i in zip(cand, inside)]
    cls = np.array([sum(w < t for t in T) for w in weight])
    order = wanted[np.argsort(rank[wanted])]                       # receivers in the order they are handed out
    assert (np.diff(cls[order]) >= 0).all()                         # heavier classes first
    for c in range(4):
        assert (np.diff(order[cls[order] == c]) > 0).all()         # within a class: by index


@pytest.mark.parametrize("n", [32, 16, 8, 1])
def test_random_masks(n):
    rng = np.random.default_rng(n)
    for trial in range(200):
        density = rng.uniform(0.0, 1.0)
        cand = (rng.random((n, 32)) < density).astype(np.uint32) @ (1 << np.arange(32, dtype=np.uint64)).astype(np.uint64)
        cand = cand.astype(np.uint32)
        cand[rng.random(n) < 0.3] = 0                               # about half the visits are empty at the headline
        inside = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)   # (bits outside cand are ignored)
        check(cand, inside)


def test_edge_cases():
    check(np.zeros(32, np.uint32), np.zeros(32, np.uint32))                          # nobody wanted
    one = np.zeros(32, np.uint32); one[17] = 0x00010000
    check(one, np.zeros(32, np.uint32))                                              # one receiver
    check(np.full(32, 0xFFFFFFFF, np.uint32), np.zeros(32, np.uint32))               # all equal, heaviest
    check(np.full(32, 0xFFFFFFFF, np.uint32), np.full(32, 0xFFFFFFFF, np.uint32))    # all equal, all inside
    check(np.full(16, 0x1, np.uint32), np.zeros(16, np.uint32))                      # all equal, lightest
    w = np.array([0xFFFFFFFF, 0x1, 0xFFFF, 0x0, 0xFF, 0xFFFFFFFF, 0x3, 0xFFFF], np.uint32)
    got, rank, _ = ranks(w, np.zeros(8, np.uint32))
    assert got == 7 and rank.tolist() == [0, 5, 1, -1, 4, 2, 6, 3]                  # weights 64, 4, 32, -, 16, 64, 4, 32: classes 0, 3, 0, -, 1, 0, 3, 0


def test_bad_arguments():
    lib = _ffi.load()
    assert lib.csf_handout_ranks(None, None, 4, None, None) == -1
    z = (C.c_uint32 * 65)()
    r = (C.c_int32 * 65)()
    assert lib.csf_handout_ranks(z, z, 65, r, None) == -1
