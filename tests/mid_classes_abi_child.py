"""csf_mid_classes through the raw C ABI and the environment knob, in a process of its own (run by tests/test_gpu_mid_classes.py): the
refusals - NULL, on outside 0 / 1, while a closed-loop calibration data set is held - come back with their code, change nothing and are each
followed by an array_equal step; CSF_MID_CLASSES=1 at creation gives the path without the call.  Prints "mid classes abi ok" at the end."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
for k in ("CSF_PAIR_VARIANT", "CSF_MID_CLASSES", "CSF_FUSED_MID", "CSF_MID_BELOW"):
    os.environ.pop(k, None)
from mid_classes_common import population  # noqa: E402
from scene_calib_common import VDES  # noqa: E402
from cyclistsocialforce_amd import _ffi  # noqa: E402
from cyclistsocialforce_amd.engine import Engine  # noqa: E402

E_ARG, E_STATE = -1, -4
L = _ffi.load()
TICKS = 12
POP = population("two", 40)
N = POP["n"]


def fill(e):
    e.set_param_classes(POP["pods"])
    e.add_agents(POP["s0"], VDES)
    e.set_dest_queue(np.arange(N), POP["off"], POP["dq"], reset=True)
    e.set_agent_class(np.arange(N), POP["cls"])
    return e


def fresh(capacity=N):
    return Engine(POP["pods"][0], capacity)


def stepped(e):
    e.step(TICKS, sync=True)
    return e.state(), e.forces()


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[1][1], b[1][1])


off_ref = stepped(fill(fresh()))                                     # the general path
on = fill(fresh())
assert L.csf_mid_classes(on._h, 1) == 0
on_ref = stepped(on)                                                 # the one-launch tick (its pair sums round differently: not the same bits)
assert on.mid_classes_ticks() == TICKS and on.mid_ticks() == TICKS
assert np.abs(on_ref[0][:, :2] - off_ref[0][:, :2]).max() < 1e-4 * POP["box"]

# ---- NULL, on outside 0 / 1: CSF_E_ARG, nothing changes --------------------------------------------------------------------------------------
n64 = C.c_int64(5)
assert L.csf_mid_classes(None, 1) == E_ARG and L.csf_mid_classes(None, 0) == E_ARG
assert L.csf_mid_classes_ticks(None, C.byref(n64)) == E_ARG and L.csf_mid_classes_ticks(on._h, None) == E_ARG and n64.value == 5
for bad in (2, -1, 7):
    e = fill(fresh())
    assert L.csf_mid_classes(e._h, bad) == E_ARG
    assert same(stepped(e), off_ref) and e.mid_classes_ticks() == 0   # the switch is still off
    e.close()
    e = fill(fresh())
    e.mid_classes(True)
    assert L.csf_mid_classes(e._h, bad) == E_ARG
    assert same(stepped(e), on_ref) and e.mid_classes_ticks() == TICKS   # ... or still on
    e.close()

# ---- while a closed-loop calibration data set is held: refused like csf_step ---------------------------------------------------------------
for held_on in (False, True):
    e = fresh(3 * N)
    e.mid_classes(held_on)
    feat = np.array([0, 1], dtype=np.int32)
    k = 3
    e.scene_calib_load([k], POP["s0"][:k, : e.ns], VDES, POP["off"][: k + 1], POP["dq"][: POP["off"][k]], np.zeros((5, k, 2)), feat, max_sets=3)
    rc = L.csf_mid_classes(e._h, 0 if held_on else 1)
    msg = L.csf_last_error(e._h).decode()
    assert rc == E_STATE and "csf_mid_classes" in msg and "csf_scene_calib_clear" in msg, (rc, msg)
    assert L.csf_step(e._h, 1) == E_STATE
    e.scene_calib_clear()
    got = stepped(fill(e))                                           # the switch is what it was before the refused call
    assert same(got, on_ref if held_on else off_ref) and e.mid_classes_ticks() == (TICKS if held_on else 0)
    e.close()

# ---- the switch can be turned off again ---------------------------------------------------------------------------------------------------
e = fill(fresh())
e.mid_classes(True)
e.mid_classes(False)
assert same(stepped(e), off_ref) and e.mid_classes_ticks() == 0 and e.mid_ticks() == 0
e.close()

# ---- CSF_MID_CLASSES=1 at creation: the path without the call; read once, in csf_create -----------------------------------------------------
os.environ["CSF_MID_CLASSES"] = "1"
e = fill(fresh())
os.environ.pop("CSF_MID_CLASSES")
late = fill(fresh())                                                 # created after the variable went: off
assert same(stepped(e), on_ref) and e.mid_classes_ticks() == TICKS
assert same(stepped(late), off_ref) and late.mid_classes_ticks() == 0
e.mid_classes(False)                                                 # the call overrides what the environment said
e.step(3, sync=True)
assert e.mid_classes_ticks() == TICKS and e.mid_ticks() == TICKS
e.close(); late.close()

# ---- CSF_FUSED_MID=0: no one-launch tick, nothing for the switch to do -------------------------------------------------------------------------
os.environ["CSF_FUSED_MID"] = "0"
e = fill(fresh())
os.environ.pop("CSF_FUSED_MID")
e.mid_classes(True)
assert same(stepped(e), off_ref) and e.mid_classes_ticks() == 0 and e.mid_ticks() == 0
e.close()
print("mid classes abi ok")
