"""Scenes with road edges through the raw C ABI, in a process of its own (run by tests/test_gpu_scene_road.py): csf_scene_calib_road and
csf_scene_calib_eval_road driven with ctypes alone, against the Python wrapper on a twin; csf_scene_calib_eval is the new call with both
arrays NULL; after csf_scene_calib_clear a small population takes the one-wave tick.  Prints "scene road abi ok" at the end."""
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
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731


def expect(e, rc, code, what):
    msg = L.csf_last_error(e._h).decode()
    assert rc == code and (msg or code == 0), f"{what}: {rc} (expected {code}) {msg!r}"


T = 30
sets = field_sets("twod", 3)
k = len(sets)
riders = np.array([3, 5], dtype=np.int32)
s0, off, rows, _ = scenes("twod", riders, seed=4)
R = s0.shape[0]
vd = np.full(R, VDES)
obj = np.random.default_rng(1).normal(size=(T, R, 2))
feat = np.array([0, 1], dtype=np.int32)
tab = (_ffi.Params * k)(*sets)
xs = np.linspace(-20.0, 34.0, 130)
verts = np.ascontiguousarray(np.r_[np.c_[xs, np.full(130, -3.0)], np.c_[xs, np.full(130, 17.0)]])
es, roff = np.array([1, 1], dtype=np.int32), np.array([0, 130, 260], dtype=np.int64)
F0, sg = np.array([5.0, 7.0]), np.array([2.0, 2.5])
rf, rs = np.array([3.0, 0.0, 8.0]), np.array([2.0, 3.0, 1.5])

e, twin = Engine(sets[0], k * R), Engine(sets[0], k * R)
expect(e, L.csf_scene_calib_road(e._h, 2, P(es), P(roff), P(verts), P(F0), P(sg)), E_STATE, "road without a data set")
for x in (e, twin):
    expect(x, L.csf_scene_calib_load(x._h, 2, P(riders), T, P(s0), P(vd), P(off), P(rows), None, P(obj), 2, P(feat), k), 0, "load")
    x._scene_calib = (R, T)
bare = twin.scene_calib_eval(sets, states=True)
sums, st = np.full((k, R, 2), -7.0), np.zeros((T, k * R, 5))


def ev(f0, sigma, out=sums, states=st):
    return L.csf_scene_calib_eval_road(e._h, k, tab, C.sizeof(_ffi.Params), _ffi.ABI_VERSION, P(f0), P(sigma), P(out), 1, P(states))


expect(e, ev(rf, rs), E_STATE, "an override and no scene has a road")
assert np.all(sums == -7.0)
expect(e, ev(None, None), 0, "eval_road with both arrays NULL")
assert np.array_equal(sums, bare[0]) and np.array_equal(st, bare[1])
expect(e, L.csf_scene_calib_road(e._h, 2, P(es), P(roff), P(verts), P(F0), P(sg)), 0, "road")
twin.scene_calib_road(es, roff, verts, F0, sg)
want = twin.scene_calib_eval(sets, states=True)
assert not np.array_equal(want[1], bare[1])
expect(e, L.csf_scene_calib_eval(e._h, k, tab, C.sizeof(_ffi.Params), _ffi.ABI_VERSION, P(sums), 1, P(st)), 0, "eval")
assert np.array_equal(sums, want[0]) and np.array_equal(st, want[1])
expect(e, ev(rf, None), E_ARG, "road_F0 alone")
expect(e, ev(rf, rs), 0, "eval_road")
over = twin.scene_calib_eval(sets, states=True, road_F0=rf, road_sigma=rs)
assert np.array_equal(sums, over[0]) and np.array_equal(st, over[1]) and not np.array_equal(st, want[1])
first = slice(0, 3)                                           # the scene without a road does not feel the override
for kk in range(k):
    assert np.array_equal(st[:, kk * R:][:, first], bare[1][:, kk * R:][:, first])
assert np.array_equal(st[:, R: 2 * R], bare[1][:, R: 2 * R])     # the set with F0 = 0
expect(e, L.csf_scene_calib_road(e._h, 0, None, None, None, None, None), 0, "no edges")
expect(e, ev(None, None), 0, "eval after the roads are dropped")
assert np.array_equal(sums, bare[0]) and np.array_equal(st, bare[1])
expect(e, L.csf_scene_calib_road(e._h, 2, P(es), P(roff), P(verts), P(F0), P(sg)), 0, "road again")
expect(e, L.csf_scene_calib_clear(e._h), 0, "clear")
assert e.n == 0
expect(e, L.csf_scene_calib_road(e._h, 2, P(es), P(roff), P(verts), P(F0), P(sg)), E_STATE, "road after clear")
e.add_agents(s0[:4], 4.0)
e.step(3, sync=True)
assert e.small_ticks() == 3
e.close(); twin.close()
print("scene road abi ok")
