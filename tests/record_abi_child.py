"""Wrong calls of the recording entry points, through the raw C ABI (run as a script in a process of its own by
tests/test_gpu_record.py).  Every one is refused by a host-side check, with a message, and leaves the engines as untouched
twins are.  Prints "record abi ok" at the end."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.pop("CSF_PAIR_VARIANT", None)
from cyclistsocialforce_amd import _ffi, parameters  # noqa: E402
from cyclistsocialforce_amd.engine import Engine  # noqa: E402

E_ARG, E_STATE = -1, -4
L = _ffi.load()


def engine(n=4, seed=0):
    rng = np.random.default_rng(seed)
    s0 = np.c_[rng.uniform(0, 12, n), rng.uniform(0, 12, n), rng.uniform(-np.pi, np.pi, n), rng.uniform(3, 5, n), np.zeros(n)]
    e = Engine(parameters.default_pod("twod"), n)
    e.add_agents(s0, 5.0)
    dq = np.zeros((n, 2, 3))
    dq[:, 0, :2] = s0[:, :2]
    dq[:, 1, 0], dq[:, 1, 1] = s0[:, 0] + 50 * np.cos(s0[:, 2]), s0[:, 1] + 50 * np.sin(s0[:, 2])
    e.set_dest_queue(np.arange(n), np.arange(n + 1) * 2, dq.reshape(-1, 3), reset=True)
    return e


def arr(engines):
    return (C.c_void_p * len(engines))(*[None if e is None else e._h for e in engines])


def refused(rc, code, what, e=None):
    assert rc == code, f"{what}: {rc} (expected {code})"
    if e is not None:
        assert L.csf_last_error(e._h), f"{what}: no message"


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


a, b, c = engine(seed=1), engine(seed=2), engine(seed=3)
ta, tb, tc = engine(seed=1), engine(seed=2), engine(seed=3)
S, F = np.full((8, 4, 5), -7.0), np.full((8, 4, 2), -7.0)

# ---- csf_record -----------------------------------------------------------------------------------------------------------
refused(L.csf_record(None, 1, 8, 3), E_ARG, "record NULL engine")
refused(L.csf_record(a._h, 0, 8, 3), E_ARG, "record stride 0", a)
refused(L.csf_record(a._h, -2, 8, 3), E_ARG, "record stride < 0", a)
refused(L.csf_record(a._h, 1, 0, 3), E_ARG, "record capacity 0", a)
refused(L.csf_record(a._h, 1, -1, 3), E_ARG, "record capacity < 0", a)
refused(L.csf_record(a._h, 1, 8, 0), E_ARG, "record what 0", a)
refused(L.csf_record(a._h, 1, 8, 4), E_ARG, "record unknown bit", a)
refused(L.csf_record(a._h, 1, 8, 7), E_ARG, "record unknown bit beside known ones", a)
# ---- csf_get_record -------------------------------------------------------------------------------------------------------
refused(L.csf_get_record(None, 0, 1, ptr(S), ptr(F)), E_ARG, "get_record NULL engine")
refused(L.csf_get_record(a._h, 0, 1, ptr(S), ptr(F)), E_STATE, "get_record before csf_record", a)
a.step(5); ta.step(5)
assert a.small_ticks() == 5                                   # (the refused csf_record calls switched nothing on)
a.record(stride=1, capacity=8, forces=True)
b.record(stride=2, capacity=8, forces=False)
a.step(12); b.step(12); ta.step(12); tb.step(12)              # a: samples 0 .. 16 written from 5 on, the ring holds 9 .. 16
refused(L.csf_get_record(a._h, 9, 8, None, None), E_ARG, "get_record both outputs NULL", a)
refused(L.csf_get_record(a._h, -1, 2, ptr(S), ptr(F)), E_ARG, "get_record first < 0", a)
refused(L.csf_get_record(a._h, 9, -1, ptr(S), ptr(F)), E_ARG, "get_record count < 0", a)
refused(L.csf_get_record(a._h, 8, 2, ptr(S), ptr(F)), E_ARG, "get_record before the ring's oldest", a)
refused(L.csf_get_record(a._h, 15, 3, ptr(S), ptr(F)), E_ARG, "get_record beyond the newest", a)
refused(L.csf_get_record(b._h, 0, 2, ptr(S), ptr(F)), E_STATE, "get_record forces without a force ring", b)
assert (S == -7.0).all() and (F == -7.0).all()                # nothing was written
assert L.csf_get_record(a._h, 9, 8, ptr(S), ptr(F)) == 0
assert np.array_equal(S[-1], a.state()) and np.array_equal(F[-1], np.c_[a.forces()])
# ---- csf_batch_get_record -------------------------------------------------------------------------------------------------
S[:], F[:] = -7.0, -7.0
Sb = np.full((2, 4, 5), -7.0)
firsts = (C.c_int64 * 3)(-1, -1, -1)


def outs(rows):
    o = (_ffi.RecordOut * 3)()
    for i, (s, f) in enumerate(rows):
        o[i].s = None if s is None else s.ctypes.data
        o[i].F = None if f is None else f.ctypes.data
        o[i].first_sample = C.cast(C.byref(firsts, i * 8), C.POINTER(C.c_int64))
    return o


good = outs([(S, F), (Sb, None), (None, None)])
refused(L.csf_batch_get_record(None, 3, 2, good), E_ARG, "batch_get_record NULL")
refused(L.csf_batch_get_record(arr([a, b, c]), 3, 2, good), E_STATE, "batch_get_record of engines that are no batch", a)
Engine.batch_join([a, b, c])
refused(L.csf_batch_get_record(arr([a, b, c]), 0, 2, good), E_ARG, "batch_get_record count 0")
refused(L.csf_batch_get_record(arr([a, c, b]), 3, 2, good), E_ARG, "batch_get_record out of join order", c)
refused(L.csf_batch_get_record(arr([a, b]), 2, 2, good), E_ARG, "batch_get_record part of the batch", a)
refused(L.csf_batch_get_record(arr([a, None, c]), 3, 2, good), E_ARG, "batch_get_record NULL member")
refused(L.csf_batch_get_record(arr([a, b, c]), 3, 2, None), E_ARG, "batch_get_record out NULL", a)
refused(L.csf_batch_get_record(arr([a, b, c]), 3, -1, good), E_ARG, "batch_get_record n_last < 0", a)
refused(L.csf_batch_get_record(arr([a, b, c]), 3, 2, outs([(S, F), (Sb, None), (Sb, None)])), E_STATE, "batch_get_record names a member without a recording", c)
refused(L.csf_batch_get_record(arr([a, b, c]), 3, 2, outs([(S, F), (Sb, F), (None, None)])), E_STATE, "batch_get_record forces of a member without a force ring", b)
refused(L.csf_batch_get_record(arr([a, b, c]), 3, 9, good), E_ARG, "batch_get_record n_last beyond a's capacity", a)
refused(L.csf_batch_get_record(arr([a, b, c]), 3, 7, good), E_ARG, "batch_get_record n_last beyond what b holds", b)
assert (S == -7.0).all() and (F == -7.0).all() and (Sb == -7.0).all() and list(firsts) == [-1, -1, -1]
# after the refusals everything still works, and the engines are what untouched twins are
Engine.step_batch([a, b, c], 4)
for t in (ta, tb, tc):
    t.step(4)
assert L.csf_batch_get_record(arr([a, b, c]), 3, 2, good) == 0
assert list(firsts) == [19, 6, -1]
assert np.array_equal(S[1], a.state()) and np.array_equal(F[1], np.c_[a.forces()]) and np.array_equal(Sb[1], b.state())
for x, t in ((a, ta), (b, tb), (c, tc)):
    assert np.array_equal(x.state(), t.state()) and x.tick == t.tick
    for u, w in zip(x.forces(), t.forces()):
        assert np.array_equal(u, w)
    assert x.batch_ticks() == 4
for e in (a, b, c, ta, tb, tc):
    e.close()
print("record abi ok")
