"""Batches of independent scenes, host side (no GPU): the new entry points are declared and exported, csf_tick_out has the same
layout in the header and in the ctypes binding, and the Python wrappers refuse wrong arguments before they reach the library."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from cyclistsocialforce_amd import _ffi
from cyclistsocialforce_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("csf_batch_join", "csf_batch_leave", "csf_step_batch", "csf_step_batch_get_tick", "csf_batch_ticks")


def test_batch_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "csf.h")).read()
    declared = set(re.findall(r"\b(csf_[a-z_0-9]+)\s*\(", header))
    lib = _ffi.load()
    for s in NEW:
        assert s in declared and s in _ffi.SYMBOLS and hasattr(lib, s), s
    assert lib.csf_abi_version() == 9


def test_tick_out_layout_matches_the_header():
    src = r"""
#include <stddef.h>
#include <stdio.h>
#include "csf.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(csf_tick_out), offsetof(csf_tick_out, s_out), offsetof(csf_tick_out, dest_ptr),
           offsetof(csf_tick_out, znav), offsetof(csf_tick_out, Fx), offsetof(csf_tick_out, Fy), offsetof(csf_tick_out, tick));
    return 0;
}
"""
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    T = _ffi.TickOut
    want = [C.sizeof(T)] + [getattr(T, f).offset for f in ("s_out", "dest_ptr", "znav", "Fx", "Fy", "tick")]
    assert got == want


class _Fake(Engine):
    """an Engine that holds no library handle: only the wrappers' own checks can be reached"""

    def __init__(self, h=1, n=3, ns=5):
        self._h, self._n, self.ns, self._lib = C.c_void_p(h), n, ns, None

    @property
    def n(self):
        return self._n

    def close(self):
        self._h = None


def test_batch_wrappers_refuse_wrong_arguments_before_the_library():
    a, b = _Fake(1), _Fake(2)
    with pytest.raises(ValueError):
        Engine.batch_join([])
    with pytest.raises(TypeError):
        Engine.batch_join([a, object()])
    with pytest.raises(ValueError):
        Engine.batch_join([a, b, a])
    with pytest.raises(ValueError):
        Engine.step_batch([a, b], -1)
    with pytest.raises(ValueError):
        Engine.step_batch([a, b], 1.5)
    with pytest.raises(ValueError):
        Engine.step_batch_into([a, b], 1, [(None,) * 5])             # one output tuple per engine
    good = (np.zeros((3, 5)), np.zeros(3, dtype=np.int32), np.zeros((3, 3), dtype=np.uint8), np.zeros(3), np.zeros(3))
    for k, bad in enumerate((np.zeros((3, 4)), np.zeros(3, dtype=np.int64), np.zeros((3, 3)), np.zeros(4), np.zeros(6)[::2])):
        o = list(good)
        o[k] = bad
        with pytest.raises(ValueError):
            Engine.step_batch_into([a, b], 1, [good, tuple(o)])
    c = _Fake(3)
    c.close()
    with pytest.raises(ValueError):
        Engine.step_batch([a, c], 1)
