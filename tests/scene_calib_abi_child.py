"""Closed-loop calibration through the raw C ABI, in a process of its own (run by tests/test_gpu_scene_calib.py): every refusal of
csf_scene_calib_load / csf_scene_calib_eval comes back with its code and a message and leaves the engine as a twin that was never
asked; the calls a loaded engine refuses; after clear the engine is empty and steps again.  Prints "scene calib abi ok" at the end."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.pop("CSF_PAIR_VARIANT", None)
from scene_calib_common import VDES, field_sets, scenes  # noqa: E402
from cyclistsocialforce_amd import _ffi, parameters  # noqa: E402
from cyclistsocialforce_amd.engine import Engine  # noqa: E402

E_ARG, E_CAPACITY, E_STATE, E_ABI = -1, -3, -4, -6
L = _ffi.load()
mode = sys.argv[1]
assert mode == "abi"
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731


def expect(e, rc, code, what):
    msg = L.csf_last_error(e._h).decode()
    assert rc == code and (msg or code == 0), f"{what}: {rc} (expected {code}) {msg!r}"


T = 60
sets = field_sets("twod", 4)
k = len(sets)
riders = np.array([3, 5], dtype=np.int32)
s0, off, rows, _ = scenes("twod", riders, seed=2)
R = s0.shape[0]
vd = np.full(R, VDES)
lens = np.array([T, T - 20], dtype=np.int32)
obj = np.random.default_rng(1).normal(size=(T, R, 2))
feat = np.array([0, 1], dtype=np.int32)
tab = (_ffi.Params * k)(*sets)
sums = np.full((k, R, 2), -7.0)


def load(e, n_scn=2, nr=riders, T_=T, s0_=s0, vd_=vd, off_=off, rows_=rows, ln=lens, obj_=obj, n_feat=2, feat_=feat, max_sets=k):
    return L.csf_scene_calib_load(e._h, n_scn, P(nr), T_, P(s0_), P(vd_), P(off_), P(rows_), P(ln), P(obj_), n_feat, P(feat_), max_sets)


def evaluate(e, n=k, tab_=tab, size=C.sizeof(_ffi.Params), abi=_ffi.ABI_VERSION, out=sums, stride=1, states=None):
    return L.csf_scene_calib_eval(e._h, n, tab_, size, abi, P(out), stride, P(states))


# ---- csf_scene_calib_load refused: the engine stays empty and usable -----------------------------------------------------------
e = Engine(sets[0], k * R)
expect(e, evaluate(e), E_STATE, "eval without a data set")
expect(e, L.csf_scene_calib_clear(e._h), E_STATE, "clear without a data set")
n64 = C.c_int64(-7)
assert L.csf_scene_calib_launches(e._h, C.byref(n64)) == E_STATE and n64.value == -7
for what, kw in (("NULL n_riders", dict(nr=None)), ("NULL s0", dict(s0_=None)), ("NULL v_desired", dict(vd_=None)), ("NULL offsets", dict(off_=None)),
                 ("NULL rows", dict(rows_=None)), ("NULL objective", dict(obj_=None)), ("NULL feat", dict(feat_=None))):
    expect(e, load(e, **kw), E_ARG, what)
expect(e, load(e, nr=np.array([0, 8], dtype=np.int32)), E_ARG, "a scene of 0 riders")
expect(e, load(e, nr=np.array([33, 1], dtype=np.int32)), E_ARG, "a scene of 33 riders")
expect(e, load(e, ln=np.array([1, T + 1], dtype=np.int32)), E_ARG, "a length beyond n_ticks")
expect(e, load(e, ln=np.array([-1, 3], dtype=np.int32)), E_ARG, "a negative length")
expect(e, load(e, feat_=np.array([0, 6], dtype=np.int32)), E_ARG, "feature 6")
expect(e, load(e, n_feat=7), E_ARG, "7 features")
empty_q = off.copy()
empty_q[2] = empty_q[1]
expect(e, load(e, off_=empty_q), E_ARG, "a rider without a destination row")
expect(e, load(e, max_sets=257), E_ARG, "257 sets")
expect(e, load(e, max_sets=0), E_ARG, "0 sets")
expect(e, load(e, max_sets=k + 1), E_CAPACITY, "more sets than the capacity holds")
assert e.n == 0
e.add_agents(s0[:2], 4.0)
expect(e, load(e), E_STATE, "a non-empty engine")
e.remove_agents([0, 1])
e.set_road([0, 2], [[0.0, 0.0], [10.0, 0.0]], [1.0], [1.0])
expect(e, load(e), E_STATE, "an engine with a road")
e.close()
rec = Engine(sets[0], k * R)
rec.record(stride=1, capacity=16)
expect(rec, load(rec), E_STATE, "a recording engine")
assert rec.n == 0
rec.close()
a, b = Engine(sets[0], k * R), Engine(sets[0], k * R)
Engine.batch_join([a, b])
expect(a, load(a), E_STATE, "a member of a batch")
Engine.batch_leave([a, b])
a.close(); b.close()
u = Engine(parameters.default_pod("uncontrolled"), k * R)
expect(u, load(u, s0_=np.ascontiguousarray(s0[:, :4])), E_ARG, "an UncontrolledVehicle set")
u.close()
two = Engine(sets[0], k * R)
two.set_param_classes(sets[:2])
expect(two, load(two), E_STATE, "an engine with two parameter sets")
two.close()

# ---- csf_scene_calib_eval refused: the next evaluation equals a twin's ---------------------------------------------------------
e, twin = Engine(sets[0], k * R), Engine(sets[0], k * R)
for x in (e, twin):
    expect(x, load(x), 0, "load")
    x._scene_calib = (R, T)                                 # (what Engine.scene_calib_load notes: the data set went in through the raw ABI)
want = twin.scene_calib_eval(sets)
assert np.isfinite(want).all() and (want > 0).all()
expect(e, load(e), E_STATE, "a second data set")
expect(e, evaluate(e, n=k + 1), E_ARG, "more sets than max_sets")
expect(e, evaluate(e, n=0), E_ARG, "no sets")
expect(e, evaluate(e, size=C.sizeof(_ffi.Params) - 8), E_ABI, "a shorter csf_params")
expect(e, evaluate(e, abi=8), E_ABI, "another ABI")
expect(e, evaluate(e, tab_=None), E_ARG, "NULL params")
expect(e, evaluate(e, out=None), E_ARG, "NULL sums")
other = (_ffi.Params * k)(*sets)
other[3] = parameters.default_pod("planarpoint")
expect(e, evaluate(e, tab_=other), E_ARG, "a set of another class")
ts = (_ffi.Params * k)(*sets)
ts[1].t_s = 0.02
expect(e, evaluate(e, tab_=ts), E_ARG, "another t_s")
st = np.zeros((T, k * R, 5))
expect(e, evaluate(e, stride=0, states=st), E_ARG, "stride 0")
expect(e, evaluate(e, stride=0), E_ARG, "stride 0 without states")
assert np.all(sums == -7.0) and e.scene_calib_launches() == 0
# the other calls on a loaded engine
expect(e, L.csf_step(e._h, 1), E_STATE, "csf_step")
one = np.zeros(1)
expect(e, L.csf_add_agents(e._h, 1, P(s0[:1].copy()), P(one)), E_STATE, "csf_add_agents")
idx = np.zeros(1, dtype=np.int32)
expect(e, L.csf_remove_agents(e._h, 1, P(idx)), E_STATE, "csf_remove_agents")
expect(e, L.csf_set_params(e._h, C.byref(sets[1])), E_STATE, "csf_set_params")
expect(e, L.csf_set_param_classes(e._h, 2, tab), E_STATE, "csf_set_param_classes")
expect(e, L.csf_set_priority_rule(e._h, 1), E_STATE, "csf_set_priority_rule")
expect(e, L.csf_record(e._h, 1, 16, 1), E_STATE, "csf_record")
expect(e, L.csf_enable_history(e._h, 1, 16), E_STATE, "csf_enable_history")
expect(e, L.csf_set_dest_queue(e._h, 1, P(idx), P(np.array([0, 1], dtype=np.int64)), P(np.zeros(3)), 1), E_STATE, "csf_set_dest_queue")
F1 = np.zeros((1, 1))
expect(e, L.csf_calib_load(e._h, 1, 1, P(s0[:1].copy()), P(F1), P(F1), None, P(np.zeros((1, 1, 1))), 1, P(feat[:1].copy()), 1), E_STATE, "csf_calib_load")
spare = Engine(sets[0], k * R)
pair = (C.c_void_p * 2)(e._h, spare._h)
expect(e, L.csf_batch_join(pair, 2), E_STATE, "csf_batch_join")
spare.close()
assert e.n == k * R and e.state().shape == (k * R, 5)
expect(e, evaluate(e), 0, "eval")
assert np.array_equal(sums, want) and e.scene_calib_launches() == 1
expect(e, evaluate(e, stride=2, states=st), 0, "eval with states")
assert np.array_equal(sums, want) and np.array_equal(st[: T // 2], twin.scene_calib_eval(sets, states=True, stride=2)[1])
expect(e, L.csf_scene_calib_clear(e._h), 0, "clear")
assert e.n == 0
expect(e, evaluate(e), E_STATE, "eval after clear")
# the cleared engine is an ordinary engine again, and takes a data set again - also the one of csf_calib_load, which refuses this call
e.add_agents(s0[:4], 4.0)
e.step(3, sync=True)
assert e.small_ticks() == 3
e.remove_agents(np.arange(4))
expect(e, load(e), 0, "load after clear")
expect(e, evaluate(e), 0, "eval after the second load")
assert np.array_equal(sums, want)
expect(e, L.csf_scene_calib_clear(e._h), 0, "clear")
expect(e, L.csf_calib_load(e._h, 1, 1, P(s0[:1].copy()), P(F1), P(F1), None, P(np.zeros((1, 1, 1))), 1, P(feat[:1].copy()), 1), 0, "csf_calib_load on the cleared engine")
expect(e, load(e), E_STATE, "csf_scene_calib_load on an engine that holds the data set of csf_calib_load")
e.close(); twin.close()
print("scene calib abi ok")
