"""Recording, host side (no GPU): csf_record_out has the same layout in the header and in the ctypes binding, the new entry points
are declared and exported, and the bookkeeping of a block of K recorded ticks (SocialForceIntersection._book_block) leaves the
trajectory ring, trajF, the force log and vehicle.i exactly as K single read-backs (_book_pull) do."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from cyclistsocialforce_amd import _ffi
from cyclistsocialforce_amd.intersection import SocialForceIntersection

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("csf_record", "csf_get_record", "csf_batch_get_record")


def test_record_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "csf.h")).read()
    declared = set(re.findall(r"\b(csf_[a-z_0-9]+)\s*\(", header))
    lib = _ffi.load()
    for s in NEW:
        assert s in declared and s in _ffi.SYMBOLS and hasattr(lib, s), s
    assert lib.csf_abi_version() == 9
    assert re.search(r"#define\s+CSF_REC_STATE\s+1u", header) and re.search(r"#define\s+CSF_REC_FORCE\s+2u", header)
    assert (_ffi.REC_STATE, _ffi.REC_FORCE) == (1, 2)


def test_record_out_layout_matches_the_header():
    src = r"""
#include <stddef.h>
#include <stdio.h>
#include "csf.h"
int main(void) {
    printf("%zu %zu %zu %zu\n", sizeof(csf_record_out), offsetof(csf_record_out, s), offsetof(csf_record_out, F),
           offsetof(csf_record_out, first_sample));
    return 0;
}
"""
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    T = _ffi.RecordOut
    assert got == [C.sizeof(T)] + [getattr(T, f).offset for f in ("s", "F", "first_sample")]


class _V:
    """what the bookkeeping touches of a vehicle"""

    def __init__(self, k, T, save):
        self._index, self.saveForces, self.drawing = k, save, None
        self.trajF = np.zeros((2, T))
        self._F, self._f_seen = [], 0

    def update_drawing(self, Fres=None):
        pass


def _mirror(n, T, ns, ti, save):
    """a SocialForceIntersection as far as _book_pull / _book_block go: the bulk mirror of n road users, no engine"""
    ins = object.__new__(SocialForceIntersection)
    ins.vehicles = [_V(k, T, save[k]) for k in range(n)]
    ins._traj = np.zeros((T, n + 2, ns))
    ins._S = np.zeros((n + 2, ns))
    ins._ti = np.r_[np.asarray(ti, dtype=np.int64), 0, 0]
    ins._fx, ins._fy = np.zeros(n + 2), np.zeros(n + 2)
    ins._flog, ins._flog_base = [], 0
    ins._drawn, ins._drawn_stale = [], True
    ins._have_force, ins._pos_stale = False, False
    ins.activate_sumo_cosimulation = False
    return ins


@pytest.mark.parametrize("n,T,K,ti", [(3, 50, 20, [0, 0, 0]), (3, 50, 50, [7, 7, 7]), (3, 50, 137, [49, 49, 49]), (4, 30, 12, [0, 5, 29, 17]),
                                      (4, 30, 95, [3, 0, 11, 29]), (1, 8, 8, [2]), (5, 16, 1, [1, 1, 1, 1, 2]), (2, 10, 5000, [0, 4])])
def test_a_block_of_ticks_is_booked_as_the_single_ticks_are(n, T, K, ti):
    """K ticks booked at once against K calls of _book_pull: road users that joined at the same tick and at different ones
    (unequal vehicle.i), K below, at and beyond the length of traj, and beyond the 4 096 entries the force log folds at"""
    rng = np.random.default_rng(n * 1000 + K)
    ns = 5
    S = rng.normal(size=(K, n, ns))
    F = rng.normal(size=(K, n, 2)) * 3.0
    save = [k % 2 == 0 for k in range(n)]
    a, b = _mirror(n, T, ns, ti, save), _mirror(n, T, ns, ti, save)
    for k in range(K):
        a._S[:n] = S[k]
        a._fx[:n], a._fy[:n] = F[k, :, 0], F[k, :, 1]
        a._book_pull(a._fx[:n], a._fy[:n], True, 1)
    b._S[:n] = S[-1]
    b._fx[:n], b._fy[:n] = F[-1, :, 0], F[-1, :, 1]
    b._book_block(S, F)
    assert np.array_equal(a._traj, b._traj)
    assert np.array_equal(a._ti, b._ti)
    assert a._have_force and b._have_force and b._pos_stale
    for u, w in zip(a.vehicles, b.vehicles):
        assert np.array_equal(u.trajF, w.trajF)
        a._fold_force_log(u); b._fold_force_log(w)
        assert u._F == w._F and len(u._F) == K
