"""csf_scene_calib_lane_groups through the Engine and the raw C ABI, in a process of its own (run by tests/test_gpu_scene_lane_groups.py):
every refusal comes back with its code and a message and is followed by an array_equal evaluation - the call on a plain load and with no
data set, n_groups 5, an entry out of range, a wrong n_groups and a record of another class at eval, plain scene_calib_eval with lane
groups loaded, NULL and hostile sizes; a reload drops the groups; after clear the engine ticks a small population on the one-wave path.
Prints "scene lane groups abi ok" at the end."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.pop("CSF_PAIR_VARIANT", None)
from scene_calib_common import VDES  # noqa: E402
from scene_lane_groups_common import (TAKE_ENTER, TAKE_EXIT, TAKE_G, TAKE_GROUP, TAKE_LANE, TAKE_T, firsts, group_sets, loaded_groups,  # noqa: E402
                                      take_objective, takeover_scene)
from cyclistsocialforce_amd import _ffi, parameters  # noqa: E402
from cyclistsocialforce_amd.engine import Engine, EngineError  # noqa: E402

E_ARG, E_STATE = -1, -4
L = _ffi.load()
assert sys.argv[1] == "abi"
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731

sets = group_sets("twod", 3, TAKE_G)
ones = firsts(sets)
part, obj = takeover_scene("twod"), take_objective()
s0, off, dq = part


def expect(e, rc, code, what, name="csf_scene_calib_lane_groups"):
    msg = L.csf_last_error(e._h).decode()
    assert rc == code and len(msg) > 20 and name in msg, f"{what}: {rc} (expected {code}) {msg!r}"


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)


assert L.csf_scene_calib_lane_groups(None, P(TAKE_GROUP), TAKE_G) == E_ARG
assert L.csf_scene_calib_lane_groups(None, None, 0) == E_ARG

# ---- no data set, csf_calib_load's data set, a plain load ---------------------------------------------------------------------------------
e = Engine(ones[0], 64)
expect(e, L.csf_scene_calib_lane_groups(e._h, P(TAKE_GROUP), TAKE_G), E_STATE, "no data set")
expect(e, L.csf_scene_calib_lane_groups(e._h, None, 0), E_STATE, "dropping with no data set")
try:
    e.scene_calib_lane_groups(TAKE_GROUP, TAKE_G)
    raise AssertionError("Engine.scene_calib_lane_groups without a data set")
except EngineError:
    pass
# (a plain load has no windows: every row of the objective is used, so none may be NaN)
e.scene_calib_load([7], s0, VDES, off, dq, np.nan_to_num(obj), np.array([0, 2, 4, 5], dtype=np.int32), max_sets=3)
plain = e.scene_calib_eval(ones, states=True)
rc = L.csf_scene_calib_lane_groups(e._h, P(TAKE_GROUP), TAKE_G)
expect(e, rc, E_STATE, "a plain load")
assert "csf_scene_calib_groups" in L.csf_last_error(e._h).decode()           # (the message names the call that load takes)
assert same(e.scene_calib_eval(ones, states=True), plain)
e.scene_calib_groups(TAKE_GROUP, TAKE_G)                                      # ... and that call still works there
grouped = e.scene_calib_eval_groups(sets, states=True)
expect(e, L.csf_scene_calib_lane_groups(e._h, None, 0), E_STATE, "dropping on a plain load")
assert same(e.scene_calib_eval_groups(sets, states=True), grouped)
e.scene_calib_clear()
# (csf_calib_load's data set: two sequences, three ticks of recorded forces)
e.calib_load(s0[:2], np.zeros((3, 2)), np.zeros((3, 2)), np.zeros((3, 2, 2)), [0, 1], max_sets=3)
expect(e, L.csf_scene_calib_lane_groups(e._h, P(TAKE_GROUP), TAKE_G), E_STATE, "csf_calib_load's data set")
assert "csf_calib_load" in L.csf_last_error(e._h).decode()
e.calib_clear()
e.close()

# ---- a shared and a wide load: the refusals, each followed by an array_equal evaluation ------------------------------------------------------
for wide in (False, True):
    e = loaded_groups(sets, [part], [(TAKE_LANE, 3)], TAKE_ENTER, TAKE_EXIT, obj, wide_from=1 if wide else None)
    bare = e.scene_calib_eval(ones, states=True)
    e.scene_calib_lane_groups(TAKE_GROUP, TAKE_G)
    want = e.scene_calib_eval_groups(sets, states=True)
    assert np.isfinite(want[0]).all() and not np.array_equal(want[0], bare[0])
    bad = TAKE_GROUP.copy()
    bad[5] = 3
    low = (np.minimum(TAKE_GROUP, 1) * 2).astype(np.uint8)
    huge = np.full(7, 255, dtype=np.uint8)
    other = parameters.default_pod("bicycle")
    tab = (_ffi.Params * (3 * TAKE_G))(*[p for t in sets for p in t])
    out = np.zeros((3, 7, 2))
    size, abi = C.sizeof(_ffi.Params), _ffi.ABI_VERSION
    cases = [("n_groups 5", lambda: L.csf_scene_calib_lane_groups(e._h, P(TAKE_GROUP), 5), E_ARG, "csf_scene_calib_lane_groups"),
             ("an entry out of range", lambda: L.csf_scene_calib_lane_groups(e._h, P(bad), 3), E_ARG, "csf_scene_calib_lane_groups"),
             ("... also below the limit of 4", lambda: L.csf_scene_calib_lane_groups(e._h, P(low), 2), E_ARG, "csf_scene_calib_lane_groups"),
             ("entries of 255", lambda: L.csf_scene_calib_lane_groups(e._h, P(huge), 4), E_ARG, "csf_scene_calib_lane_groups"),
             ("n_groups 2^30", lambda: L.csf_scene_calib_lane_groups(e._h, P(TAKE_GROUP), 1 << 30), E_ARG, "csf_scene_calib_lane_groups"),
             ("csf_scene_calib_groups on shared lanes", lambda: L.csf_scene_calib_groups(e._h, P(TAKE_GROUP), TAKE_G), E_STATE, "lanes"),
             ("a wrong n_groups at eval", lambda: L.csf_scene_calib_eval_groups(e._h, 3, 2, tab, size, abi, None, None, P(out), 1, None), E_ARG,
              "csf_scene_calib_eval_groups"),
             ("n_groups 0 at eval", lambda: L.csf_scene_calib_eval_groups(e._h, 3, 0, tab, size, abi, None, None, P(out), 1, None), E_ARG,
              "csf_scene_calib_eval_groups"),
             ("no records", lambda: L.csf_scene_calib_eval_groups(e._h, 3, TAKE_G, None, size, abi, None, None, P(out), 1, None), E_ARG, "csf_scene_calib_eval"),
             ("nowhere to put the sums", lambda: L.csf_scene_calib_eval_groups(e._h, 3, TAKE_G, tab, size, abi, None, None, None, 1, None), E_ARG,
              "csf_scene_calib_eval"),
             ("more than max_sets", lambda: L.csf_scene_calib_eval_groups(e._h, 4, TAKE_G, tab, size, abi, None, None, P(out), 1, None), E_ARG,
              "csf_scene_calib_eval"),
             ("plain eval with lane groups loaded", lambda: L.csf_scene_calib_eval(e._h, 3, (_ffi.Params * 3)(*ones), size, abi, P(out), 1, None), E_STATE,
              "csf_scene_calib_eval")]
    for what, call, code, name in cases:
        expect(e, call(), code, f"wide={wide}: {what}", name)
        assert same(e.scene_calib_eval_groups(sets, states=True), want), (wide, what)
    for what, call in (("a record of another class", lambda: e.scene_calib_eval_groups([p[:2] + (other,) for p in sets])),
                       ("another csf_params", None), ("plain eval with road parameters", lambda: e.scene_calib_eval(ones, road_F0=1.0, road_sigma=2.0))):
        if call is None:
            rc = L.csf_scene_calib_eval_groups(e._h, 3, TAKE_G, tab, size - 8, abi, None, None, P(out), 1, None)
            assert rc < 0 and len(L.csf_last_error(e._h)) > 20, what
        else:
            try:
                call()
                raise AssertionError(f"wide={wide}: {what} was not refused")
            except EngineError as err:
                assert len(str(err)) > 20
        assert same(e.scene_calib_eval_groups(sets, states=True), want), (wide, what)
    # dropping: NULL, and n_groups 1; then the groups once more
    for drop in (lambda: L.csf_scene_calib_lane_groups(e._h, None, TAKE_G), lambda: L.csf_scene_calib_lane_groups(e._h, P(TAKE_GROUP), 1)):
        assert drop() == 0
        assert same(e.scene_calib_eval(ones, states=True), bare)
        e.scene_calib_lane_groups(TAKE_GROUP, TAKE_G)
        assert same(e.scene_calib_eval_groups(sets, states=True), want)
    # a reload drops the groups
    e.scene_calib_clear()
    assert e.n == 0
    e.add_agents(s0[:4, : e.ns], 4.0)                            # after clear: an ordinary engine on the one-wave path
    e.step(3, sync=True)
    assert e.small_ticks() == 3
    e.remove_agents(np.arange(4))
    nr, nl = np.array([7], dtype=np.int32), np.array([3], dtype=np.int32)
    feat = np.array([0, 2, 4, 5], dtype=np.int32)
    load = e.scene_calib_load_wide if wide else e.scene_calib_load_shared
    load(nr, nl, TAKE_LANE, TAKE_ENTER, TAKE_EXIT, s0, VDES, off, dq, obj, feat, max_sets=3, **(dict(wide_from=1) if wide else {}))
    assert same(e.scene_calib_eval(ones, states=True), bare)    # (no groups: the plain evaluation is taken, and it is today's)
    expect(e, L.csf_scene_calib_eval_groups(e._h, 3, TAKE_G, tab, size, abi, None, None, P(out), 1, None), E_ARG, "groups at eval after a reload",
           "csf_scene_calib_eval_groups")
    e.scene_calib_lane_groups(TAKE_GROUP)                        # (n_groups: the largest entry + 1)
    assert same(e.scene_calib_eval_groups(sets, states=True), want)
    e.close()
assert TAKE_T == obj.shape[0]
print("scene lane groups abi ok")
