"""csf_mid_road through the raw C ABI and the environment knob, in a process of its own (run by tests/test_gpu_mid_road.py): the refusals -
NULL, on outside 0 / 1, while a closed-loop calibration data set is held - come back with their code, change nothing and are each
followed by an array_equal step; CSF_MID_ROAD=1 at creation gives the path without the call.  Prints "mid road abi ok" at the end."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
for k in ("CSF_PAIR_VARIANT", "CSF_MID_ROAD", "CSF_FUSED_MID"):
    os.environ.pop(k, None)
from mid_road_common import box_for, member_inputs, road  # noqa: E402
from cyclistsocialforce_amd import _ffi, parameters  # noqa: E402
from cyclistsocialforce_amd.engine import Engine  # noqa: E402

E_ARG, E_STATE = -1, -4
L = _ffi.load()
N, TICKS = 50, 12
S0, OFF, DQ = member_inputs("twod", N, 0, 91)
ROAD = road("sigma2", box_for(N))
POD = parameters.default_pod("twod")


def fill(e):
    e.add_agents(S0, 5.0)
    e.set_dest_queue(np.arange(N), OFF, DQ, reset=True)
    e.set_road(*ROAD)
    return e


def stepped(e):
    e.step(TICKS, sync=True)
    return e.state(), e.forces()


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[1][1], b[1][1])


ref = stepped(fill(Engine(POD, N)))                                  # (the two paths give the same bits: mid_road_ticks tells them apart)
on = fill(Engine(POD, N))
assert L.csf_mid_road(on._h, 1) == 0
assert same(stepped(on), ref) and on.mid_road_ticks() == TICKS and on.mid_ticks() == TICKS

# ---- NULL, on outside 0 / 1: CSF_E_ARG, nothing changes --------------------------------------------------------------------------------------
n64 = C.c_int64(5)
assert L.csf_mid_road(None, 1) == E_ARG and L.csf_mid_road(None, 0) == E_ARG
assert L.csf_mid_road_ticks(None, C.byref(n64)) == E_ARG and L.csf_mid_road_ticks(on._h, None) == E_ARG and n64.value == 5
for bad in (2, -1, 7):
    e = fill(Engine(POD, N))
    assert L.csf_mid_road(e._h, bad) == E_ARG
    assert same(stepped(e), ref) and e.mid_road_ticks() == 0          # the switch is still off
    e.close()
    e = fill(Engine(POD, N))
    e.mid_road(True)
    assert L.csf_mid_road(e._h, bad) == E_ARG
    assert same(stepped(e), ref) and e.mid_road_ticks() == TICKS      # ... or still on
    e.close()

# ---- while a closed-loop calibration data set is held: refused like csf_step ---------------------------------------------------------------
for held_on in (False, True):
    e = Engine(POD, 3 * N)
    e.mid_road(held_on)
    feat = np.array([0, 1], dtype=np.int32)
    k = 3
    e.scene_calib_load([k], S0[:k, : e.ns], 5.0, OFF[: k + 1], DQ[: OFF[k]], np.zeros((5, k, 2)), feat, max_sets=3)
    rc = L.csf_mid_road(e._h, 0 if held_on else 1)
    msg = L.csf_last_error(e._h).decode()
    assert rc == E_STATE and "csf_mid_road" in msg and "csf_scene_calib_clear" in msg, (rc, msg)
    assert L.csf_step(e._h, 1) == E_STATE
    e.scene_calib_clear()
    got = stepped(fill(e))                                           # the switch is what it was before the refused call
    assert same(got, ref) and e.mid_road_ticks() == (TICKS if held_on else 0)
    e.close()

# ---- the switch can be turned off again ---------------------------------------------------------------------------------------------------
e = fill(Engine(POD, N))
e.mid_road(True)
e.mid_road(False)
assert same(stepped(e), ref) and e.mid_road_ticks() == 0 and e.mid_ticks() == TICKS
e.close()

# ---- CSF_MID_ROAD=1 at creation: the path without the call; read once, in csf_create ---------------------------------------------------------
os.environ["CSF_MID_ROAD"] = "1"
e = fill(Engine(POD, N))
os.environ.pop("CSF_MID_ROAD")
late = fill(Engine(POD, N))                                          # created after the variable went: off
assert same(stepped(e), ref) and e.mid_road_ticks() == TICKS
assert same(stepped(late), ref) and late.mid_road_ticks() == 0
e.mid_road(False)                                                    # the call overrides what the environment said
e.step(3, sync=True)
assert e.mid_road_ticks() == TICKS and e.mid_ticks() == TICKS + 3
e.close(); late.close()

# ---- CSF_FUSED_MID=0: no one-launch tick, nothing for the switch to do -------------------------------------------------------------------------
os.environ["CSF_FUSED_MID"] = "0"
e = fill(Engine(POD, N))
os.environ.pop("CSF_FUSED_MID")
e.mid_road(True)
e.step(TICKS, sync=True)
assert e.mid_road_ticks() == 0 and e.mid_ticks() == 0
e.close()
print("mid road abi ok")
