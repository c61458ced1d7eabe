"""csf_scene_calib_classes through the Engine and the raw C ABI, in a process of its own (run by tests/test_gpu_scene_mixed.py): every
refusal comes back with its code and a message that names the call and is followed by an array_equal evaluation - no data set, a shared
and a wide load, n_groups outside 2 .. 12, a group entry out of range, a class outside the six, NULL arrays, the class mismatch at
evaluation, plain scene_calib_eval with classes loaded; the call and csf_scene_calib_groups replace each other; dropping gives the
evaluation before the call; after clear the engine is empty and ticks a small population on the one-wave path.
Prints "scene_mixed_abi_child: ok" at the end."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.pop("CSF_PAIR_VARIANT", None)
from scene_calib_common import VDES  # noqa: E402
from scene_mixed_common import CLASSES, G, GROUPS, MODELS, mixed_scenes, mixed_sets  # noqa: E402
from cyclistsocialforce_amd import _ffi, parameters  # noqa: E402
from cyclistsocialforce_amd.engine import Engine, EngineError  # noqa: E402

E_ARG, E_STATE = -1, -4
L = _ffi.load()
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
NAME = "csf_scene_calib_classes"

sets = mixed_sets()
ones = [p[0] for p in sets]
_, _, _, per = mixed_scenes()
s0, off, dq = per[1]                                              # scene b: twod, bicycle, bicycle, invpend, twod
grp = GROUPS[1].astype(np.uint8)
n, T = 5, 30
feat = np.array([0, 2, 4, 5], dtype=np.int32)
obj = np.random.default_rng(5).normal(size=(T, n, feat.size))
wide = np.ascontiguousarray(s0)
size, abi = C.sizeof(_ffi.Params), _ffi.ABI_VERSION


def expect(e, rc, code, what, name=NAME):
    msg = L.csf_last_error(e._h).decode()
    assert rc == code and len(msg) > 20 and name in msg, f"{what}: {rc} (expected {code}) {msg!r}"
    return msg


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)


assert L.csf_scene_calib_classes(None, P(grp), G, P(MODELS), P(wide)) == E_ARG
assert L.csf_scene_calib_classes(None, None, 0, None, None) == E_ARG

# ---- no data set ----------------------------------------------------------------------------------------------------------------------------
e = Engine(ones[0], 64)
expect(e, L.csf_scene_calib_classes(e._h, P(grp), G, P(MODELS), P(wide)), E_STATE, "no data set")
expect(e, L.csf_scene_calib_classes(e._h, None, 0, None, None), E_STATE, "dropping with no data set")
try:
    e.scene_calib_classes(grp, MODELS, s0)
    raise AssertionError("Engine.scene_calib_classes without a data set")
except EngineError:
    pass

# ---- a plain load: the refusals, each followed by an array_equal evaluation -------------------------------------------------------------------
e.scene_calib_load([n], s0, VDES, off, dq, obj, feat, max_sets=3)
ns_own = e.ns
plain = e.scene_calib_eval(ones, states=True)
e.scene_calib_classes(grp, MODELS, s0)
assert e.ns == 8 and L.csf_num_states(e._h) == 8
want = e.scene_calib_eval_groups(sets, states=True)
assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
bad = grp.copy()
bad[3] = G
unc, neg, seven = MODELS.copy(), MODELS.copy(), MODELS.copy()
unc[2], neg[0], seven[5] = _ffi.UNCONTROLLED, -1, 7
tab = (_ffi.Params * (3 * G))(*[p for t in sets for p in t])
swapped = (_ffi.Params * (3 * G))(*[p for t in sets for p in (t[1], t[0]) + t[2:]])
out = np.zeros((3, n, 2))
cases = [("n_groups 1", lambda: L.csf_scene_calib_classes(e._h, P(grp), 1, P(MODELS), P(wide)), E_ARG, NAME),
         ("n_groups 0 with arrays", lambda: L.csf_scene_calib_classes(e._h, P(grp), 0, P(MODELS), P(wide)), E_ARG, NAME),
         ("n_groups 13", lambda: L.csf_scene_calib_classes(e._h, P(grp), 13, P(MODELS), P(wide)), E_ARG, NAME),
         ("n_groups -1", lambda: L.csf_scene_calib_classes(e._h, P(grp), -1, P(MODELS), P(wide)), E_ARG, NAME),
         ("a group entry >= n_groups", lambda: L.csf_scene_calib_classes(e._h, P(bad), G, P(MODELS), P(wide)), E_ARG, NAME),
         ("... also below the limit", lambda: L.csf_scene_calib_classes(e._h, P(grp), 2, P(MODELS), P(wide)), E_ARG, NAME),
         ("an UncontrolledVehicle", lambda: L.csf_scene_calib_classes(e._h, P(grp), G, P(unc), P(wide)), E_ARG, NAME),
         ("class -1", lambda: L.csf_scene_calib_classes(e._h, P(grp), G, P(neg), P(wide)), E_ARG, NAME),
         ("class 7", lambda: L.csf_scene_calib_classes(e._h, P(grp), G, P(seven), P(wide)), E_ARG, NAME),
         ("NULL s0", lambda: L.csf_scene_calib_classes(e._h, P(grp), G, P(MODELS), None), E_ARG, NAME),
         ("NULL models", lambda: L.csf_scene_calib_classes(e._h, P(grp), G, None, P(wide)), E_ARG, NAME),
         ("NULL group", lambda: L.csf_scene_calib_classes(e._h, None, G, P(MODELS), P(wide)), E_ARG, NAME),
         ("a wrong n_groups at eval", lambda: L.csf_scene_calib_eval_groups(e._h, 3, 2, tab, size, abi, None, None, P(out), 1, None), E_ARG,
          "csf_scene_calib_eval_groups"),
         ("records of other classes at eval", lambda: L.csf_scene_calib_eval_groups(e._h, 3, G, swapped, size, abi, None, None, P(out), 1, None), E_ARG,
          "csf_scene_calib_eval_groups"),
         ("another csf_params", lambda: L.csf_scene_calib_eval_groups(e._h, 3, G, tab, size - 8, abi, None, None, P(out), 1, None), -6, "csf_scene_calib_eval"),
         ("more than max_sets", lambda: L.csf_scene_calib_eval_groups(e._h, 4, G, tab, size, abi, None, None, P(out), 1, None), E_ARG, "csf_scene_calib_eval"),
         ("plain eval with classes loaded", lambda: L.csf_scene_calib_eval(e._h, 3, (_ffi.Params * 3)(*ones), size, abi, P(out), 1, None), E_STATE,
          "csf_scene_calib_eval"),
         ("plain eval_road with classes loaded",
          lambda: L.csf_scene_calib_eval_road(e._h, 3, (_ffi.Params * 3)(*ones), size, abi, None, None, P(out), 1, None), E_STATE, "csf_scene_calib_eval")]
for what, call, code, name in cases:
    rc = call()
    if code == -6:                                                # (the ABI refusal: whatever code it has, negative and with a message)
        assert rc < 0 and len(L.csf_last_error(e._h)) > 20, what
    else:
        msg = expect(e, rc, code, what, name)
        if what == "records of other classes at eval":            # the message names set, group and both classes
            assert "set 0" in msg and "group 0" in msg and "class 0" in msg and "class 1" in msg, msg
    assert e.ns == 8
    assert same(e.scene_calib_eval_groups(sets, states=True), want), what

# ---- the call and csf_scene_calib_groups replace each other; dropping is the load again ----------------------------------------------------
two = (grp > 0).astype(np.uint8)
e.scene_calib_groups(two, 2)
assert e.ns == ns_own
twod2 = [(p[0], p[0]) for p in sets]
grouped = e.scene_calib_eval_groups(twod2, states=True)
expect(e, L.csf_scene_calib_eval_groups(e._h, 3, G, tab, size, abi, None, None, P(out), 1, None), E_ARG, "six records after csf_scene_calib_groups",
       "csf_scene_calib_eval_groups")
e.scene_calib_classes(grp, MODELS, s0)                            # ... and back
assert e.ns == 8 and same(e.scene_calib_eval_groups(sets, states=True), want)
expect(e, L.csf_scene_calib_classes(e._h, P(bad), G, P(MODELS), P(wide)), E_ARG, "a refused call leaves the held classes in force")
assert same(e.scene_calib_eval_groups(sets, states=True), want)
e.scene_calib_groups(two, 2)
assert same(e.scene_calib_eval_groups(twod2, states=True), grouped)
e.scene_calib_classes(grp, MODELS, s0)
e.scene_calib_classes(None)
assert e.ns == ns_own and L.csf_num_states(e._h) == ns_own
assert same(e.scene_calib_eval(ones, states=True), plain)
# replay, windows and a road loaded BEFORE the classes keep working: the same evaluation as with them loaded AFTER
mask = np.array([0, 0, 0, 0, 1], dtype=bool)
enter, exit_ = np.array([0, 3, 0, 0, 0], dtype=np.int32), np.array([T, T, 20, T, T], dtype=np.int32)
road = (np.array([0], dtype=np.int32), np.array([0, 30], dtype=np.int64), np.c_[np.linspace(-10, 30, 30), np.full(30, -3.0)], 0.3, 2.0)
e.scene_calib_classes(grp, MODELS, s0)
e.scene_calib_replay(mask, want[1][:, :n][:, mask, :4])
e.scene_calib_windows(enter, exit_)
e.scene_calib_road(*road)
after = e.scene_calib_eval_groups(sets, states=True)
e.scene_calib_classes(None)
e.scene_calib_classes(grp, MODELS, s0)
assert same(e.scene_calib_eval_groups(sets, states=True), after)
assert np.all(after[0][:, 4] == 0.0) and not same(after, want)
e.scene_calib_clear()
assert e.n == 0 and e.ns == ns_own
e.add_agents(s0[:4, : e.ns], 4.0)                                # after clear: an ordinary engine on the one-wave path
e.step(3, sync=True)
assert e.small_ticks() == 3
e.remove_agents(np.arange(4))
# a reload starts without classes
e.scene_calib_load([n], s0, VDES, off, dq, obj, feat, max_sets=3)
assert same(e.scene_calib_eval(ones, states=True), plain)
e.scene_calib_clear()
# with classes held at the clear
e.scene_calib_load([n], s0, VDES, off, dq, obj, feat, max_sets=3)
e.scene_calib_classes(grp, MODELS, s0)
assert same(e.scene_calib_eval_groups(sets, states=True), want)
e.scene_calib_clear()
assert e.n == 0 and e.ns == ns_own and L.csf_num_states(e._h) == ns_own
e.close()

# ---- a shared and a wide load refuse the classes and evaluate as before -----------------------------------------------------------------------
for is_wide in (False, True):
    x = Engine(ones[0], 15)
    load = x.scene_calib_load_wide if is_wide else x.scene_calib_load_shared
    load([n], [n], np.arange(n), np.zeros(n, dtype=int), np.full(n, T), s0, VDES, off, dq, obj, feat, max_sets=3, **(dict(wide_from=1) if is_wide else {}))
    a = x.scene_calib_eval(ones, states=True)
    msg = expect(x, L.csf_scene_calib_classes(x._h, P(grp), G, P(MODELS), P(wide)), E_STATE, f"wide={is_wide}")
    assert "csf_scene_calib_load" in msg and "mixed classes" in msg
    expect(x, L.csf_scene_calib_classes(x._h, None, 0, None, None), E_STATE, f"dropping, wide={is_wide}")
    assert same(x.scene_calib_eval(ones, states=True), a)
    x.close()
assert parameters.default_pod(CLASSES[0]).model == MODELS[0]
print("scene_mixed_abi_child: ok")
