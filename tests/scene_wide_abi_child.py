"""csf_scene_calib_load_wide through the raw C ABI, in a process of its own (run by tests/test_gpu_scene_wide.py): every refusal comes
back with its code and a message and leaves the engine empty and usable; after a wide load csf_step, csf_scene_calib_windows and what
4.10 refuses while a data set is held are refused; csf_scene_calib_clear frees everything and the engine ticks a small population on
the one-wave path again.  Prints "scene wide abi ok" at the end."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.pop("CSF_PAIR_VARIANT", None)
from scene_calib_common import VDES, field_sets, scenes  # noqa: E402
from cyclistsocialforce_amd import _ffi  # noqa: E402
from cyclistsocialforce_amd.engine import Engine  # noqa: E402

E_ARG, E_CAPACITY, E_STATE = -1, -3, -4
L = _ffi.load()
assert sys.argv[1] == "abi"
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731

T = 40
sets = field_sets("twod", 2)
k = len(sets)
riders = np.array([5, 44], dtype=np.int32)
s0, off, rows, _ = scenes("twod", riders, seed=2)
R = s0.shape[0]
lens = np.array([T, T - 10], dtype=np.int32)
obj = np.random.default_rng(1).normal(size=(T, R, 2))
feat = np.array([0, 1], dtype=np.int32)
n_lanes = np.array([3, 40], dtype=np.int32)
# scene 0: riders 0, 1, 2 on lanes 0, 1, 2; rider 3 takes lane 1 over at tick 20; rider 4 is never present
# scene 1 (30 ticks, 40 lanes - wide): riders 0 .. 39 on their own lanes, riders 40 .. 43 take lanes 0 .. 3 over at tick 15
lane = np.r_[[0, 1, 2, 1, 2], np.arange(40), np.arange(4)].astype(np.int32)
enter = np.r_[[0, 5, 0, 20, 17], np.zeros(40), np.full(4, 15)].astype(np.int32)
exit_ = np.r_[[T, 20, 30, T, 17], np.r_[np.full(4, 15), np.full(36, 30)], np.full(4, 30)].astype(np.int32)
vd = np.full(R, VDES)
Lsum = int(n_lanes.sum())
CAP = max(R, k * Lsum)
NAME = "csf_scene_calib_load_wide"


def load(e, nr=riders, nl=n_lanes, ln=lane, en=enter, ex=exit_, max_sets=k, wide_from=33):
    return L.csf_scene_calib_load_wide(e._h, nr.size, P(nr), P(nl), P(ln), P(en), P(ex), T, P(s0), P(vd), P(off), P(rows), P(lens), P(obj), 2, P(feat),
                                       max_sets, wide_from)


def expect(e, rc, code, what, name=NAME):
    msg = L.csf_last_error(e._h).decode()
    assert rc == code and (msg or code == 0), f"{what}: {rc} (expected {code}) {msg!r}"
    if code:
        assert name in msg, (what, msg)


def changed(arr, at, value):
    out = arr.copy()
    out[at] = value
    return out


def evaluate(e):
    return e.scene_calib_eval(sets, states=True)


# ---- CSF_E_ARG: the engine stays empty and usable ---------------------------------------------------------------------------------
assert L.csf_scene_calib_load_wide(None, 2, P(riders), P(n_lanes), P(lane), P(enter), P(exit_), T, P(s0), P(vd), P(off), P(rows), P(lens), P(obj), 2,
                                   P(feat), k, 33) == E_ARG
e = Engine(sets[0], CAP)
cases = [("no lanes", dict(nl=changed(n_lanes, 0, 0))), ("257 lanes", dict(nl=changed(n_lanes, 1, 257))),
         ("wide_from 0", dict(wide_from=0)), ("wide_from 258", dict(wide_from=258)), ("wide_from -1", dict(wide_from=-1)),
         ("40 lanes below wide_from", dict(wide_from=41)),
         ("a lane behind the scene's lanes", dict(ln=changed(lane, R - 1, 40))), ("a negative lane", dict(ln=changed(lane, 7, -1))),
         ("two riders of one lane overlap", dict(en=changed(enter, R - 1, 14))), ("two riders of one lane overlap (narrow scene)", dict(en=changed(enter, 3, 19))),
         ("an exit behind the scene's length", dict(ex=changed(exit_, R - 1, 31))), ("an empty roster", dict(nr=changed(riders, 0, 0)))]
for what, kw in cases:
    expect(e, load(e, **kw), E_ARG, what)
    assert e.n == 0, what
for name in ("nl", "ln", "en", "ex"):
    rc = L.csf_scene_calib_load_wide(e._h, 2, P(riders), *[None if name == a else P(v) for a, v in (("nl", n_lanes), ("ln", lane), ("en", enter), ("ex", exit_))],
                                     T, P(s0), P(vd), P(off), P(rows), P(lens), P(obj), 2, P(feat), k, 33)
    expect(e, rc, E_ARG, f"NULL {name}")
    assert e.n == 0
rc = L.csf_scene_calib_load_wide(e._h, 2, P(riders), P(n_lanes), P(lane), P(enter), P(exit_), T, None, P(vd), P(off), P(rows), P(lens), P(obj), 2, P(feat), k, 33)
expect(e, rc, E_ARG, "NULL s0")
small = Engine(sets[0], CAP - 1)
expect(small, load(small), E_CAPACITY, "a capacity below max(R, max_sets x lanes)")
assert small.n == 0
small.close()
# the old entry points keep their limit of 32 lanes, with their own names in the message
rc = L.csf_scene_calib_load_shared(e._h, 2, P(riders), P(n_lanes), P(lane), P(enter), P(exit_), T, P(s0), P(vd), P(off), P(rows), P(lens), P(obj), 2, P(feat), k)
expect(e, rc, E_ARG, "40 lanes by the shared load", "csf_scene_calib_load_shared")
assert "(1 .. 32)" in L.csf_last_error(e._h).decode() and e.n == 0
e.add_agents(s0[:4, : e.ns], 4.0)                                # usable after the refusals
e.step(2, sync=True)
assert e.small_ticks() == 2
e.remove_agents(np.arange(4))

# ---- the data set; what is refused while one is held --------------------------------------------------------------------------------
expect(e, load(e), 0, "the load")
e._scene_calib = (R, T)
before, st_before = evaluate(e)
assert e.scene_calib_launches() == 2                             # a narrow scene and a wide one
t = np.arange(T)[:, None]
here = (enter[None, :] <= t) & (t < exit_[None, :])
for s in range(k):
    assert np.array_equal(np.isnan(st_before[:, s * R: (s + 1) * R]).any(axis=2), ~here)
assert np.isfinite(before).all() and np.all(before[:, 4] == 0.0) and np.all(before[:, np.arange(R) != 4, 0] > 0.0)
expect(e, L.csf_scene_calib_windows(e._h, P(enter), P(exit_)), E_STATE, "windows on a wide data set", "csf_scene_calib_windows")
expect(e, L.csf_scene_calib_windows(e._h, None, None), E_STATE, "dropping the windows of a wide data set", "csf_scene_calib_windows")
expect(e, load(e), E_STATE, "a second data set")
expect(e, L.csf_step(e._h, 1), E_STATE, "csf_step", "")
one = np.array([4.0])
expect(e, L.csf_add_agents(e._h, 1, P(s0[:1].copy()), P(one)), E_STATE, "csf_add_agents", "")
idx = np.array([0], dtype=np.int32)
expect(e, L.csf_remove_agents(e._h, 1, P(idx)), E_STATE, "csf_remove_agents", "")
expect(e, L.csf_record(e._h, 1, 16, 1), E_STATE, "csf_record", "")
again, st_again = evaluate(e)
assert np.array_equal(again, before) and np.array_equal(st_again, st_before, equal_nan=True)
assert e.scene_calib_launches() == 4
# wide_from = 1 and wide_from = 33 agree on the wide scene bit for bit: it runs on the same kernel either way
x = Engine(sets[0], CAP)
expect(x, load(x, wide_from=1), 0, "wide_from = 1")
x._scene_calib = (R, T)
all_wide, st_all = evaluate(x)
assert x.scene_calib_launches() == 1
x.close()
assert np.array_equal(all_wide[:, 5:], before[:, 5:]) and np.array_equal(st_all.reshape(T, k, R, -1)[:, :, 5:], st_before.reshape(T, k, R, -1)[:, :, 5:], equal_nan=True)

# ---- clear: an ordinary engine again ----------------------------------------------------------------------------------------------
expect(e, L.csf_scene_calib_clear(e._h), 0, "clear")
assert e.n == 0
e._scene_calib = None
e.add_agents(s0[:4, : e.ns], 4.0)
e.step(3, sync=True)
assert e.small_ticks() == 2 + 3                                  # (counted since the engine was created)
e.remove_agents(np.arange(4))
expect(e, load(e), 0, "a second load")
e._scene_calib = (R, T)
got, got_st = evaluate(e)
assert np.array_equal(got, before) and np.array_equal(got_st, st_before, equal_nan=True)
e.close()
print("scene wide abi ok")
