"""csf_scene_calib_load_shared through the raw C ABI, in a process of its own (run by tests/test_gpu_scene_lanes.py): every refusal
comes back with its code and a message and leaves the engine empty and usable; csf_scene_calib_windows is refused on a shared data
set and so is what 4.10 refuses while a data set is held; replay, road and eval in two orders are array_equal; csf_scene_calib_clear
frees everything and the engine ticks a small population on the one-wave path again.  Prints "scene lanes abi ok" at the end."""
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

T = 60
sets = field_sets("twod", 3)
k = len(sets)
riders = np.array([5, 36], dtype=np.int32)                       # the second roster is above 32
s0, off, rows, _ = scenes("twod", riders, seed=2)
R = s0.shape[0]
lens = np.array([T, T - 20], dtype=np.int32)
obj = np.random.default_rng(1).normal(size=(T, R, 2))
feat = np.array([0, 1], dtype=np.int32)
n_lanes = np.array([3, 12], dtype=np.int32)
# scene 0: riders 0, 1, 2 on lanes 0, 1, 2; rider 3 takes lane 1 over at tick 30 with no idle tick; rider 4 is never present
# scene 1 (40 ticks): rider j on lane j % 12, three turns per lane: [0, 10), [12, 25), [25, 40)
lane = np.r_[[0, 1, 2, 1, 2], np.arange(36) % 12].astype(np.int32)
enter = np.r_[[0, 5, 0, 30, 17], np.repeat([0, 12, 25], 12)].astype(np.int32)
exit_ = np.r_[[T, 30, 40, T, 17], np.repeat([10, 25, 40], 12)].astype(np.int32)
vd = np.full(R, VDES)
Lsum = int(n_lanes.sum())
CAP = max(R, k * Lsum)


def load(e, nr=riders, nl=n_lanes, ln=lane, en=enter, ex=exit_, max_sets=k):
    return L.csf_scene_calib_load_shared(e._h, nr.size, P(nr), P(nl), P(ln), P(en), P(ex), T, P(s0), P(vd), P(off), P(rows), P(lens), P(obj), 2, P(feat),
                                         max_sets)


def expect(e, rc, code, what, name="csf_scene_calib_load_shared"):
    msg = L.csf_last_error(e._h).decode()
    assert rc == code and (msg or code == 0), f"{what}: {rc} (expected {code}) {msg!r}"
    if code:
        assert name in msg, (what, msg)


def evaluate(e):
    return e.scene_calib_eval(sets, states=True)


# ---- CSF_E_ARG: the engine stays empty and usable ---------------------------------------------------------------------------------
assert L.csf_scene_calib_load_shared(None, 2, P(riders), P(n_lanes), P(lane), P(enter), P(exit_), T, P(s0), P(vd), P(off), P(rows), P(lens), P(obj), 2,
                                     P(feat), k) == E_ARG
e = Engine(sets[0], CAP)


def changed(arr, at, value):
    out = arr.copy()
    out[at] = value
    return out


cases = [("no lanes", dict(nl=changed(n_lanes, 0, 0))), ("33 lanes", dict(nl=changed(n_lanes, 1, 33))),
         ("a negative lane", dict(ln=changed(lane, 2, -1))), ("a lane behind the scene's lanes", dict(ln=changed(lane, 0, 3))),
         ("a lane of the other scene", dict(ln=changed(lane, 4, 11))), ("the last rider's lane", dict(ln=changed(lane, R - 1, 12))),
         ("a negative entry", dict(en=changed(enter, 1, -1))), ("an entry behind the exit", dict(en=changed(enter, 2, 41))),
         ("an exit behind the scene's length", dict(ex=changed(exit_, R - 1, T - 19))), ("an exit behind the first scene's length", dict(ex=changed(exit_, 0, T + 1))),
         ("two riders of one lane overlap", dict(en=changed(enter, 3, 29))), ("two riders of one lane overlap (second scene)", dict(ex=changed(exit_, 5, 13))),
         ("an empty roster", dict(nr=changed(riders, 0, 0)))]
for what, kw in cases:
    expect(e, load(e, **kw), E_ARG, what)
    assert e.n == 0, what
for name in ("nl", "ln", "en", "ex"):
    rc = L.csf_scene_calib_load_shared(e._h, 2, P(riders), *[None if name == a else P(v) for a, v in (("nl", n_lanes), ("ln", lane), ("en", enter), ("ex", exit_))],
                                       T, P(s0), P(vd), P(off), P(rows), P(lens), P(obj), 2, P(feat), k)
    expect(e, rc, E_ARG, f"NULL {name}")
small = Engine(sets[0], CAP - 1)
expect(small, load(small), E_CAPACITY, "a capacity below max(R, max_sets x lanes)")
assert small.n == 0
small.close()
# (a rider that is never present may name any lane of its scene, also one that is taken at that tick)
expect(e, load(e, ln=changed(lane, 4, 0)), 0, "an empty window on a busy lane")
e._scene_calib = (R, T)
ghost, ghost_st = evaluate(e)
e.scene_calib_clear()
assert e.n == 0
e.add_agents(s0[:4, : e.ns], 4.0)                                # usable after the refusals
e.step(2, sync=True)
assert e.small_ticks() == 2
e.remove_agents(np.arange(4))

# ---- the data set; what 4.10 refuses while one is held ----------------------------------------------------------------------------
expect(e, load(e), 0, "the load")
e._scene_calib = (R, T)
before, st_before = evaluate(e)
assert np.array_equal(before, ghost) and np.array_equal(st_before, ghost_st, equal_nan=True)
t = np.arange(T)[:, None]
here = (enter[None, :] <= t) & (t < exit_[None, :])
for s in range(k):
    assert np.array_equal(np.isnan(st_before[:, s * R: (s + 1) * R]).any(axis=2), ~here)
assert np.all(before[:, 4] == 0.0) and np.all(before[:, np.arange(R) != 4, 0] > 0.0)
expect(e, L.csf_scene_calib_windows(e._h, P(enter), P(exit_)), E_STATE, "windows on a shared data set", "csf_scene_calib_windows")
expect(e, L.csf_scene_calib_windows(e._h, None, None), E_STATE, "dropping the windows of a shared data set", "csf_scene_calib_windows")
expect(e, load(e), E_STATE, "a second data set")
expect(e, L.csf_scene_calib_load(e._h, 1, P(riders[:1].copy()), T, P(s0), P(vd), P(off), P(rows), None, P(obj), 2, P(feat), 1), E_STATE, "csf_scene_calib_load",
       "csf_scene_calib_load")
expect(e, L.csf_step(e._h, 1), E_STATE, "csf_step", "")
one = np.array([4.0])
expect(e, L.csf_add_agents(e._h, 1, P(s0[:1].copy()), P(one)), E_STATE, "csf_add_agents", "")
idx = np.array([0], dtype=np.int32)
expect(e, L.csf_remove_agents(e._h, 1, P(idx)), E_STATE, "csf_remove_agents", "")
expect(e, L.csf_set_priority_rule(e._h, 1), E_STATE, "csf_set_priority_rule", "")
expect(e, L.csf_record(e._h, 1, 16, 1), E_STATE, "csf_record", "")
launches = e.scene_calib_launches()
again, st_again = evaluate(e)
assert np.array_equal(again, before) and np.array_equal(st_again, st_before, equal_nan=True)
assert e.scene_calib_launches() == launches + 1
perm = np.array([2, 0, 1])
sp, stp = e.scene_calib_eval([sets[i] for i in perm], states=True)
assert np.array_equal(sp, before[perm]) and np.array_equal(stp.reshape(T, k, R, -1), st_before.reshape(T, k, R, -1)[:, perm], equal_nan=True)

# ---- replay, road and eval in two orders ------------------------------------------------------------------------------------------
mask = np.zeros(R, dtype=bool)
mask[[3, 7]] = True
rep_rows = np.random.default_rng(3).normal(size=(T, 2, 4)) + s0[[3, 7], :4][None]
road = (np.array([0, 1], dtype=np.int32), np.array([0, 3, 5], dtype=np.int64),
        np.array([[-5.0, -3.0], [10.0, -3.0], [25.0, -3.0], [0.0, 40.0], [30.0, 40.0]]), np.array([2.0, 1.5]), np.array([2.0, 2.0]))


def full(order):
    x = Engine(sets[0], CAP)
    assert load(x) == 0
    x._scene_calib = (R, T)
    for step in order:
        if step == "p":
            x.scene_calib_replay(mask, rep_rows)
        else:
            x.scene_calib_road(*road)
    out = evaluate(x)
    x.close()
    return out


want, want_st = full("pr")
assert np.isfinite(want).all() and not np.array_equal(want, before) and np.all(want[:, [3, 7]] == 0.0)
got, got_st = full("rp")
assert np.array_equal(got, want) and np.array_equal(got_st, want_st, equal_nan=True)
assert np.array_equal(want_st[30:, 3, :4], rep_rows[30:, 0])                                 # inside its window rider 3 IS its recording
e.scene_calib_road(*road)
e.scene_calib_replay(mask, rep_rows)
got, got_st = evaluate(e)
assert np.array_equal(got, want) and np.array_equal(got_st, want_st, equal_nan=True)
f0, sg = np.array([1.0, 2.0, 3.0]), np.array([2.0, 2.5, 3.0])
over, _ = e.scene_calib_eval(sets, states=True, road_F0=f0, road_sigma=sg)
assert np.isfinite(over).all() and not np.array_equal(over, want)
e.scene_calib_replay(None)
e.scene_calib_road(None, None, None, None, None)
got, got_st = evaluate(e)
assert np.array_equal(got, before) and np.array_equal(got_st, st_before, equal_nan=True)
# the road limit is that of the scene's LANES: scene 1 has 12 lanes (P = 16: 1 024 vertices), its roster of 36 would allow 256
wide = np.c_[np.linspace(-20.0, 60.0, 600), np.full(600, -6.0)]
e.scene_calib_road(np.array([1], dtype=np.int32), np.array([0, 600], dtype=np.int64), wide, np.array([2.0]), np.array([2.0]))
assert np.isfinite(evaluate(e)[0]).all()
e.scene_calib_road(None, None, None, None, None)

# ---- clear: an ordinary engine again ----------------------------------------------------------------------------------------------
expect(e, L.csf_scene_calib_clear(e._h), 0, "clear")
assert e.n == 0
e._scene_calib = None
expect(e, L.csf_scene_calib_windows(e._h, P(enter), P(exit_)), E_STATE, "windows after clear", "csf_scene_calib_windows")
e.add_agents(s0[:4, : e.ns], 4.0)
e.step(3, sync=True)
assert e.small_ticks() == 2 + 3                                  # (counted since the engine was created)
e.remove_agents(np.arange(4))
expect(e, load(e), 0, "a second load")
e._scene_calib = (R, T)
got, got_st = evaluate(e)
assert np.array_equal(got, before) and np.array_equal(got_st, st_before, equal_nan=True)
e.close()
print("scene lanes abi ok")
