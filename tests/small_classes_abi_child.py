"""csf_small_classes through the raw C ABI and the environment knobs, in a process of its own (run by tests/test_gpu_small_classes.py): the
refusals - NULL, on = 2, while a closed-loop calibration data set is held - come back with their code, change nothing and are each followed
by an array_equal step; CSF_SMALL_CLASSES=1 at creation gives the path without the call; CSF_FUSED_SMALL=0 wins over it.
Prints "small classes abi ok" at the end."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
for k in ("CSF_PAIR_VARIANT", "CSF_SMALL_CLASSES", "CSF_FUSED_SMALL"):
    os.environ.pop(k, None)
from scene_calib_common import VDES  # noqa: E402
from small_classes_common import case  # noqa: E402
from cyclistsocialforce_amd import _ffi  # noqa: E402
from cyclistsocialforce_amd.engine import Engine  # noqa: E402

E_ARG, E_STATE = -1, -4
L = _ffi.load()
c = case("b")
n = c["s0"].shape[0]
TICKS = 12


def fill(e):
    e.set_param_classes(c["pods"])
    e.add_agents(c["s0"], VDES)
    e.set_dest_queue(np.arange(n), c["off"], c["dq"], reset=True)
    e.set_agent_class(np.arange(n), c["cls"])
    return e


def stepped(e):
    e.step(TICKS, sync=True)
    return e.state(), e.forces()


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[1][1], b[1][1])


ref_off = stepped(fill(Engine(c["pods"][0], n)))
on = fill(Engine(c["pods"][0], n))
assert L.csf_small_classes(on._h, 1) == 0
ref_on = stepped(on)
assert on.small_ticks() == TICKS                                     # (small_ticks tells the two paths apart below)

# ---- NULL, on outside 0 / 1: CSF_E_ARG, nothing changes --------------------------------------------------------------------------------------
assert L.csf_small_classes(None, 1) == E_ARG and L.csf_small_classes(None, 0) == E_ARG
for bad in (2, -1, 7):
    e = fill(Engine(c["pods"][0], n))
    assert L.csf_small_classes(e._h, bad) == E_ARG
    assert same(stepped(e), ref_off) and e.small_ticks() == 0        # the switch is still off
    e.close()
    e = fill(Engine(c["pods"][0], n))
    e.small_classes(True)
    assert L.csf_small_classes(e._h, bad) == E_ARG
    assert same(stepped(e), ref_on) and e.small_ticks() == TICKS     # ... or still on
    e.close()

# ---- while a closed-loop calibration data set is held: refused like csf_step ---------------------------------------------------------------
for held_on in (False, True):
    e = Engine(c["pods"][0], 3 * n)
    e.small_classes(held_on)
    feat = np.array([0, 1], dtype=np.int32)
    e.scene_calib_load([n], c["s0"][:, : e.ns], VDES, c["off"], c["dq"], np.zeros((5, n, 2)), feat, max_sets=3)
    rc = L.csf_small_classes(e._h, 0 if held_on else 1)
    msg = L.csf_last_error(e._h).decode()
    assert rc == E_STATE and "csf_small_classes" in msg and "csf_scene_calib_clear" in msg, (rc, msg)
    assert L.csf_step(e._h, 1) == E_STATE
    e.scene_calib_clear()
    got = stepped(fill(e))                                           # the switch is what it was before the refused call
    assert same(got, ref_on if held_on else ref_off) and e.small_ticks() == (TICKS if held_on else 0)
    e.close()

# ---- the switch can be turned off again ---------------------------------------------------------------------------------------------------
e = fill(Engine(c["pods"][0], n))
e.small_classes(True)
e.small_classes(False)
assert same(stepped(e), ref_off) and e.small_ticks() == 0
e.close()

# ---- CSF_SMALL_CLASSES=1 at creation: the path without the call; read once, in csf_create ----------------------------------------------------
os.environ["CSF_SMALL_CLASSES"] = "1"
e = fill(Engine(c["pods"][0], n))
os.environ.pop("CSF_SMALL_CLASSES")
late = fill(Engine(c["pods"][0], n))                                 # created after the variable went: off
assert same(stepped(e), ref_on) and e.small_ticks() == TICKS
assert same(stepped(late), ref_off) and late.small_ticks() == 0
e.small_classes(False)                                               # the call overrides what the environment said
e.step(3, sync=True)
assert e.small_ticks() == TICKS
e.close(); late.close()

# ---- CSF_FUSED_SMALL=0 wins over it --------------------------------------------------------------------------------------------------------
os.environ["CSF_SMALL_CLASSES"] = "1"
os.environ["CSF_FUSED_SMALL"] = "0"
e = fill(Engine(c["pods"][0], n))
os.environ.pop("CSF_SMALL_CLASSES"); os.environ.pop("CSF_FUSED_SMALL")
assert same(stepped(e), ref_off) and e.small_ticks() == 0
e.small_classes(True)
e.step(3, sync=True)
assert e.small_ticks() == 0
e.close()
print("small classes abi ok")
