"""csf_scene_calib_windows through the raw C ABI, in a process of its own (run by tests/test_gpu_scene_windows.py): every refusal
comes back with its code and a message and leaves the held windows in force; the windows survive csf_scene_calib_replay and
csf_scene_calib_road in either order; csf_scene_calib_clear frees them and the engine ticks a small population on the one-wave path
again.  Prints "scene windows abi ok" at the end."""
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

E_ARG, E_STATE = -1, -4
L = _ffi.load()
mode = sys.argv[1]
assert mode == "abi"
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731


def expect(e, rc, code, what):
    msg = L.csf_last_error(e._h).decode()
    assert rc == code and (msg or code == 0), f"{what}: {rc} (expected {code}) {msg!r}"
    if code:
        assert "csf_scene_calib_windows" in msg, (what, msg)


T = 60
sets = field_sets("twod", 3)
k = len(sets)
riders = np.array([3, 5], dtype=np.int32)
s0, off, rows, _ = scenes("twod", riders, seed=2)
R = s0.shape[0]
lens = np.array([T, T - 20], dtype=np.int32)
obj = np.random.default_rng(1).normal(size=(T, R, 2))
feat = np.array([0, 1], dtype=np.int32)
enter = np.array([0, 5, 0, 0, 10, 0, 20, 0], dtype=np.int32)
exit_ = np.array([T, T, 30, 40, 40, 25, 40, 0], dtype=np.int32)


def windows(e, en=enter, ex=exit_):
    return L.csf_scene_calib_windows(e._h, P(en), P(ex))


def loaded():
    e = Engine(sets[0], k * R)
    e.scene_calib_load(riders, s0, VDES, off, rows, obj, feat, lengths=lens, max_sets=k)
    return e


# ---- CSF_E_STATE: no data set, and the data set of csf_calib_load ---------------------------------------------------------------
assert L.csf_scene_calib_windows(None, P(enter), P(exit_)) == E_ARG
e = Engine(sets[0], k * R)
expect(e, windows(e), E_STATE, "windows without a data set")
expect(e, L.csf_scene_calib_windows(e._h, None, None), E_STATE, "dropping windows without a data set")
c0 = np.zeros((2, 8))
c0[:, 3] = 4.0
e.calib_load(c0, np.ones((5, 2)), np.zeros((5, 2)), np.zeros((5, 2, 1)), [0], max_sets=1)
expect(e, windows(e), E_STATE, "windows on the data set of csf_calib_load")
e.calib_clear()
e.close()

# ---- CSF_E_ARG: the held windows stay in force ------------------------------------------------------------------------------------
e = loaded()
plain, plain_st = e.scene_calib_eval(sets, states=True)
for first in (False, True):                                      # refused with no windows held, then with windows held
    if first:
        expect(e, windows(e), 0, "windows")
    before, st_before = e.scene_calib_eval(sets, states=True)
    expect(e, L.csf_scene_calib_windows(e._h, P(enter), None), E_ARG, "enter without exit")
    expect(e, L.csf_scene_calib_windows(e._h, None, P(exit_)), E_ARG, "exit without enter")
    for what, r, a, b in (("a negative entry", 1, -1, 10), ("an entry behind the exit", 2, 31, 30), ("an exit behind the scene's length", 4, 0, T - 19),
                          ("an exit behind the scene's length (first scene)", 0, 0, T + 1), ("the last rider", R - 1, 3, 2)):
        en, ex = enter.copy(), exit_.copy()
        en[r], ex[r] = a, b
        expect(e, windows(e, en, ex), E_ARG, what)
    with np.testing.assert_raises(ValueError):
        e.scene_calib_windows(enter[:-1], exit_[:-1])
    with np.testing.assert_raises(ValueError):
        e.scene_calib_windows(enter, None)
    after, st_after = e.scene_calib_eval(sets, states=True)
    assert np.array_equal(after, before) and np.array_equal(st_after, st_before), first
assert np.array_equal(st_before[:5, 1], np.tile(st_before[0, 1], (5, 1))) and not np.array_equal(st_before[5, 1], st_before[4, 1])   # rider 1 enters at tick 5
assert not np.array_equal(before, plain)
assert np.all(before[:, 7] == 0.0) and np.all(before[:, :7, 0] > 0.0)
launches = e.scene_calib_launches()
again, st_again = e.scene_calib_eval(sets, states=True)
assert np.array_equal(again, before) and np.array_equal(st_again, st_before)                 # two identical evaluations
assert e.scene_calib_launches() == launches + 1                                              # one launch per evaluation
perm = np.array([2, 0, 1])
sp, stp = e.scene_calib_eval([sets[i] for i in perm], states=True)
assert np.array_equal(sp, before[perm]) and np.array_equal(stp.reshape(T, k, R, -1), st_before.reshape(T, k, R, -1)[:, perm])

# ---- the windows survive csf_scene_calib_replay / csf_scene_calib_road, in either order -------------------------------------------
mask = np.zeros(R, dtype=bool)
mask[[0, 4]] = True
rep_rows = np.random.default_rng(3).normal(size=(T, 2, 4)) + s0[[0, 4], :4][None]
road = (np.array([1], dtype=np.int32), np.array([0, 3], dtype=np.int64), np.array([[-5.0, -3.0], [10.0, -3.0], [25.0, -3.0]]), np.array([2.0]), np.array([2.0]))


def full(order):
    x = loaded()
    for step in order:
        if step == "w":
            x.scene_calib_windows(enter, exit_)
        elif step == "p":
            x.scene_calib_replay(mask, rep_rows)
        else:
            x.scene_calib_road(*road)
    out = x.scene_calib_eval(sets, states=True)
    x.close()
    return out


want, want_st = full("wpr")
assert np.isfinite(want).all() and not np.array_equal(want, before)
for order in ("prw", "rwp", "pwr"):
    got, got_st = full(order)
    assert np.array_equal(got, want) and np.array_equal(got_st, want_st), order
e.scene_calib_replay(mask, rep_rows)
e.scene_calib_road(*road)
got, got_st = e.scene_calib_eval(sets, states=True)
assert np.array_equal(got, want) and np.array_equal(got_st, want_st)
e.scene_calib_replay(None)
e.scene_calib_road(None, None, None, None, None)
got, got_st = e.scene_calib_eval(sets, states=True)
assert np.array_equal(got, before) and np.array_equal(got_st, st_before)
expect(e, L.csf_scene_calib_windows(e._h, None, None), 0, "dropping the windows")
got, got_st = e.scene_calib_eval(sets, states=True)
assert np.array_equal(got, plain) and np.array_equal(got_st, plain_st)
expect(e, windows(e), 0, "windows again")

# ---- clear frees them with the rest: the engine is an ordinary engine again, and a new data set starts without windows ------------
expect(e, L.csf_scene_calib_clear(e._h), 0, "clear")
assert e.n == 0
e._scene_calib = None
expect(e, windows(e), E_STATE, "windows after clear")
e.add_agents(s0[:4], 4.0)
e.step(3, sync=True)
assert e.small_ticks() == 3
e.remove_agents(np.arange(4))
e.scene_calib_load(riders, s0, VDES, off, rows, obj, feat, lengths=lens, max_sets=k)
got, got_st = e.scene_calib_eval(sets, states=True)
assert np.array_equal(got, plain) and np.array_equal(got_st, plain_st)
e.close()
print("scene windows abi ok")
