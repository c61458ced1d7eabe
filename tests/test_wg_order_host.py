"""The order of a source chunk's receiver groups (csrc/csf_wg_order.h), on the host: csf_wg_order_ranks ranks with the very
function the order kernel counts with.  Whatever the costs are, the result must be a permutation of 0 .. n - 1 - the pair
kernel serves every group of a chunk exactly once only then -, with the costs not rising along it and equal costs in index order."""
import ctypes as C

import numpy as np
import pytest

from cyclistsocialforce_amd import _ffi


def order_of(cost):
    lib = _ffi.load()
    cost = np.ascontiguousarray(cost, dtype=np.uint32)
    order = np.full(len(cost), -7, dtype=np.int32)
    got = lib.csf_wg_order_ranks(cost.ctypes.data_as(C.POINTER(C.c_uint32)), len(cost), order.ctypes.data_as(C.POINTER(C.c_int32)))
    assert got == len(cost)
    return order


RNG = np.random.default_rng(5)
CASES = {
    "random": RNG.integers(0, 2**32, 512, dtype=np.uint64).astype(np.uint32),
    "few_values": RNG.integers(0, 4, 512).astype(np.uint32),
    "all_equal": np.full(512, 883719, dtype=np.uint32),
    "all_zero": np.zeros(512, dtype=np.uint32),
    "max_and_zero": np.where(RNG.random(512) < 0.5, 0xFFFFFFFF, 0).astype(np.uint32),
    "one": np.array([17], dtype=np.uint32),
    "513": RNG.integers(0, 1000, 513).astype(np.uint32),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_order_is_a_permutation_heaviest_first_ties_by_index(name):
    cost = CASES[name]
    order = order_of(cost)
    assert np.array_equal(np.sort(order), np.arange(len(cost)))
    along = cost[order].astype(np.int64)
    assert (np.diff(along) <= 0).all()
    assert (np.diff(order)[np.diff(along) == 0] > 0).all()
    assert np.array_equal(order, np.argsort(-cost.astype(np.int64), kind="stable"))


def test_bad_arguments():
    lib = _ffi.load()
    z = (C.c_uint32 * 4)()
    r = (C.c_int32 * 4)()
    assert lib.csf_wg_order_ranks(None, 4, r) == -1 and lib.csf_wg_order_ranks(z, 4, None) == -1 and lib.csf_wg_order_ranks(z, -1, r) == -1
    assert lib.csf_wg_order_ranks(z, 0, r) == 0
