"""csf_scene_calib_lane_classes through the Engine and the raw C ABI, in a process of its own (run by tests/test_gpu_scene_lane_classes.py):
every refusal comes back with its code and a message and is followed by an array_equal evaluation - the call on a plain load, with no data
set and on csf_calib_load's, n_groups outside 2 .. 12, an entry out of range, a class outside the six, NULL arrays, a record of another
class at eval, plain evaluations with lane classes held; classes and lane groups replace each other; classes loaded before or after replay
and a road give the same bits; after clear the engine has its own state width and ticks a small population on the one-wave path.
Prints "scene lane classes abi ok" at the end."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.pop("CSF_PAIR_VARIANT", None)
from scene_calib_common import VDES  # noqa: E402
from scene_groups_common import group_sets  # noqa: E402
from scene_lane_classes_common import (G, MODELS, TAKE_CLASS_GROUP, TAKE_ENTER, TAKE_EXIT, TAKE_LANE, TAKE_T, firsts, loaded_classes,  # noqa: E402
                                       mixed_sets, take_class_scene, take_objective)
from cyclistsocialforce_amd import _ffi, parameters  # noqa: E402
from cyclistsocialforce_amd.engine import Engine, EngineError  # noqa: E402

E_ARG, E_STATE = -1, -4
L = _ffi.load()
assert sys.argv[1] == "abi"
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
NAME = "csf_scene_calib_lane_classes"

sets = mixed_sets()
ones = firsts(sets)
part, obj = take_class_scene(), take_objective()
s0, off, dq = part
GRP, S8 = TAKE_CLASS_GROUP, np.ascontiguousarray(s0)
feat = np.array([0, 2, 4, 5], dtype=np.int32)


def call(e, group=GRP, n=G, models=MODELS, s=S8):
    return L.csf_scene_calib_lane_classes(e._h if e is not None else None, P(group), n, P(models), P(s))


def expect(e, rc, code, what, name=NAME):
    msg = L.csf_last_error(e._h).decode()
    assert rc == code and len(msg) > 20 and name in msg, f"{what}: {rc} (expected {code}) {msg!r}"


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)


assert call(None) == E_ARG
assert L.csf_scene_calib_lane_classes(None, None, 0, None, None) == E_ARG

# ---- no data set, csf_calib_load's data set, a plain load ---------------------------------------------------------------------------------
e = Engine(ones[0], 64)
own = e.ns
expect(e, call(e), E_STATE, "no data set")
expect(e, L.csf_scene_calib_lane_classes(e._h, None, 0, None, None), E_STATE, "dropping with no data set")
try:
    e.scene_calib_lane_classes(GRP, MODELS, S8)
    raise AssertionError("Engine.scene_calib_lane_classes without a data set")
except EngineError:
    pass
e.scene_calib_load([7], s0, VDES, off, dq, np.nan_to_num(obj), feat, max_sets=3)
plain = e.scene_calib_eval(ones, states=True)
expect(e, call(e), E_STATE, "a plain load")
assert "csf_scene_calib_classes" in L.csf_last_error(e._h).decode()           # (the message names the call that load takes)
assert same(e.scene_calib_eval(ones, states=True), plain) and L.csf_num_states(e._h) == own
e.scene_calib_classes(GRP, MODELS, S8)                                        # ... and that call still works there
mixed = e.scene_calib_eval_groups(sets, states=True)
expect(e, L.csf_scene_calib_lane_classes(e._h, None, 0, None, None), E_STATE, "dropping on a plain load")
assert same(e.scene_calib_eval_groups(sets, states=True), mixed)
e.scene_calib_clear()
e.calib_load(s0[:2, :own], np.zeros((3, 2)), np.zeros((3, 2)), np.zeros((3, 2, 2)), [0, 1], max_sets=3)
expect(e, call(e), E_STATE, "csf_calib_load's data set")
assert "csf_calib_load" in L.csf_last_error(e._h).decode()
e.calib_clear()
e.close()

# ---- a shared and a wide load: the refusals, each followed by an array_equal evaluation ------------------------------------------------------
two = group_sets("twod", 3, 3)
grp3 = (np.arange(7) % 3).astype(np.uint8)
box = 28.0
lines = [np.c_[np.linspace(-20.0, box + 20.0, c), np.full(c, y)] for c, y in ((40, -3.0), (23, box + 3.0))]
roff = np.array([0, 40, 63], dtype=np.int64)
mask = np.array([False, True, False, False, False, False, False])
rep_rows = np.zeros((TAKE_T, 1, 4))
rep_rows[:, 0, 0] = s0[1, 0] + 0.05 * np.arange(TAKE_T)
rep_rows[:, 0, 1], rep_rows[:, 0, 2], rep_rows[:, 0, 3] = s0[1, 1], s0[1, 2], 1.0
for wide in (False, True):
    kw = dict(wide_from=1 if wide else None)
    e = loaded_classes(sets, [part], [(TAKE_LANE, 3)], TAKE_ENTER, TAKE_EXIT, obj, **kw)
    own = e.ns
    bare = e.scene_calib_eval(ones, states=True)
    e.scene_calib_lane_classes(GRP, MODELS, S8)
    assert e.ns == 8 and L.csf_num_states(e._h) == 8
    want = e.scene_calib_eval_groups(sets, states=True)
    assert np.isfinite(want[0]).all() and want[1].shape[2] == 8
    bad = GRP.copy()
    bad[5] = G
    huge = np.full(7, 255, dtype=np.uint8)
    m_unc, m_out, m_neg = MODELS.copy(), MODELS.copy(), MODELS.copy()
    m_unc[2], m_out[3], m_neg[0] = _ffi.UNCONTROLLED, 7, -1
    other = parameters.default_pod("bicycle")
    tab = (_ffi.Params * (3 * G))(*[p for t in sets for p in t])
    out = np.zeros((3, 7, 2))
    size, abi = C.sizeof(_ffi.Params), _ffi.ABI_VERSION
    cases = [("n_groups 1", lambda: call(e, n=1), E_ARG, NAME), ("n_groups 13", lambda: call(e, n=13), E_ARG, NAME),
             ("n_groups 0 with arrays", lambda: call(e, n=0), E_ARG, NAME), ("n_groups 2^30", lambda: call(e, n=1 << 30), E_ARG, NAME),
             ("an entry out of range", lambda: call(e, group=bad), E_ARG, NAME), ("entries of 255", lambda: call(e, group=huge), E_ARG, NAME),
             ("an UncontrolledVehicle", lambda: call(e, models=m_unc), E_ARG, NAME), ("class 7", lambda: call(e, models=m_out), E_ARG, NAME),
             ("class -1", lambda: call(e, models=m_neg), E_ARG, NAME),
             ("group NULL", lambda: L.csf_scene_calib_lane_classes(e._h, None, G, P(MODELS), P(S8)), E_ARG, NAME),
             ("models NULL", lambda: L.csf_scene_calib_lane_classes(e._h, P(GRP), G, None, P(S8)), E_ARG, NAME),
             ("s0 NULL", lambda: L.csf_scene_calib_lane_classes(e._h, P(GRP), G, P(MODELS), None), E_ARG, NAME),
             ("csf_scene_calib_classes on shared lanes", lambda: L.csf_scene_calib_classes(e._h, P(GRP), G, P(MODELS), P(S8)), E_STATE,
              "mixed classes need csf_scene_calib_load"),
             ("a wrong n_groups at eval", lambda: L.csf_scene_calib_eval_groups(e._h, 3, 2, tab, size, abi, None, None, P(out), 1, None), E_ARG,
              "csf_scene_calib_eval_groups"),
             ("plain eval with lane classes held", lambda: L.csf_scene_calib_eval(e._h, 3, (_ffi.Params * 3)(*ones), size, abi, P(out), 1, None), E_STATE,
              "csf_scene_calib_eval"),
             ("plain road eval with lane classes held",
              lambda: L.csf_scene_calib_eval_road(e._h, 3, (_ffi.Params * 3)(*ones), size, abi, None, None, P(out), 1, None), E_STATE, "csf_scene_calib_eval")]
    for what, fn, code, name in cases:
        expect(e, fn(), code, f"wide={wide}: {what}", name)
        assert L.csf_num_states(e._h) == 8, (wide, what)
        assert same(e.scene_calib_eval_groups(sets, states=True), want), (wide, what)
    try:                                                         # the class mismatch at evaluation names set, group and both classes
        e.scene_calib_eval_groups([p[:2] + (other,) + p[3:] for p in sets])
        raise AssertionError(f"wide={wide}: a record of another class was not refused")
    except EngineError as err:
        assert "group 2" in str(err) and "csf_scene_calib_eval_groups" in str(err)
    assert same(e.scene_calib_eval_groups(sets, states=True), want)
    # classes and lane groups replace each other; dropping gives the bare data set
    e.scene_calib_lane_groups(grp3, 3)
    assert e.ns == own and L.csf_num_states(e._h) == own
    grouped = e.scene_calib_eval_groups(two, states=True)
    e.scene_calib_lane_classes(GRP, MODELS, S8)
    assert e.ns == 8 and same(e.scene_calib_eval_groups(sets, states=True), want)
    e.scene_calib_lane_groups(grp3, 3)
    assert same(e.scene_calib_eval_groups(two, states=True), grouped)
    e.scene_calib_lane_classes(GRP, MODELS, S8)
    assert L.csf_scene_calib_lane_classes(e._h, None, 0, None, None) == 0
    assert L.csf_num_states(e._h) == own
    e.ns = own
    assert same(e.scene_calib_eval(ones, states=True), bare)
    # classes before or after replay and a road: the same bits
    e.scene_calib_lane_classes(GRP, MODELS, S8)
    e.scene_calib_replay(mask, rep_rows)
    e.scene_calib_road(np.zeros(2, dtype=np.int32), roff, np.concatenate(lines), 0.3, 2.0)
    after = e.scene_calib_eval_groups(sets, states=True)
    assert not np.array_equal(after[0], want[0]) and np.all(after[0][:, 1] == 0.0)
    e.scene_calib_lane_classes(None)
    e.scene_calib_lane_classes(GRP, MODELS, S8)                  # (replay and road are held: the classes come last)
    assert same(e.scene_calib_eval_groups(sets, states=True), after)
    # a reload drops the classes; after clear the engine is an ordinary one of its own width
    e.scene_calib_clear()
    assert e.n == 0 and e.ns == own and L.csf_num_states(e._h) == own
    e.add_agents(s0[:4, : e.ns], 4.0)
    e.step(3, sync=True)
    assert e.small_ticks() == 3
    e.remove_agents(np.arange(4))
    nr, nl = np.array([7], dtype=np.int32), np.array([3], dtype=np.int32)
    load = e.scene_calib_load_wide if wide else e.scene_calib_load_shared
    load(nr, nl, TAKE_LANE, TAKE_ENTER, TAKE_EXIT, s0, VDES, off, dq, obj, feat, max_sets=3, **(dict(wide_from=1) if wide else {}))
    assert same(e.scene_calib_eval(ones, states=True), bare)    # (no classes: the plain evaluation is taken, and it is today's)
    e.scene_calib_lane_classes(GRP, MODELS, S8)
    assert same(e.scene_calib_eval_groups(sets, states=True), want)
    e.close()
assert TAKE_T == obj.shape[0]
print("scene lane classes abi ok")
