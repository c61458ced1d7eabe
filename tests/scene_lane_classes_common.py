"""Shared by tests/test_gpu_scene_lane_classes.py, tests/test_scene_lane_classes_host.py and tests/scene_lane_classes_abi_child.py
(DESIGN.md 4.10j): vehicle classes on shared lanes and on wide scenes - a loaded engine, the takeover roster whose lanes change their
class, and the comparison of an evaluation with the general-path twins of tests/scene_groups_common.py."""
import numpy as np

from scene_groups_common import GENERAL_TOL, general_twin  # noqa: F401
from scene_lane_groups_common import (TAKE_ENTER, TAKE_EXIT, TAKE_LANE, TAKE_T, dist, firsts, loaded_groups, take_objective,  # noqa: F401
                                      twin_deviation, twin_extent_check)
from scene_lanes_common import FEAT, LANES_T, cat_parts, extent, inside  # noqa: F401
from scene_mixed_common import CLASSES, MODELS, WIDTH, mixed_sets  # noqa: F401
from scene_windows_common import one_scene

G = len(CLASSES)                                                # group g is of class CLASSES[g] (scene_mixed_common)
GROUP_OF = {m: g for g, m in enumerate(CLASSES)}


def groups_of(*classes):
    return np.array([GROUP_OF[m] for m in classes], dtype=np.uint8)


def widen(part):
    """(s0, off, dq) with the start states in the widest layout: missing columns 0"""
    s0, off, dq = part
    w = np.zeros((s0.shape[0], WIDTH))
    w[:, : min(s0.shape[1], WIDTH)] = s0[:, :WIDTH]
    return w, off, dq


def loaded_classes(sets, parts, lanes, enter, exit, obj, group=None, models=MODELS, wide_from=None, **kw):
    """scene_lane_groups_common.loaded_groups without groups - a shared load, or with wide_from a wide one, by an engine of the class of
    the candidates' first record - and then, with `group`, scene_calib_lane_classes; `parts` in the widest layout (widen)"""
    e = loaded_groups(sets, parts, lanes, enter, exit, obj, wide_from=wide_from, **kw)
    if group is not None:
        e.scene_calib_lane_classes(np.asarray(group), models, cat_parts(parts)[1])
    return e


# ---- the takeover roster of scene_lane_groups_common with classes by rider: lane 0 a BalancingRider, then a PlanarPoint; lane 1 a Bicycle,
# then a TwoD; lane 2 an InvPendulum, then a Bicycle; rider 6 - never present - a PlanarBicycle.  REVERSED: lane 1 a TwoD, then a Bicycle.
TAKE_CLASSES = ("balancingrider", "bicycle", "invpend", "planarpoint", "twod", "bicycle", "planarbike")
TAKE_CLASS_GROUP = groups_of(*TAKE_CLASSES)
TAKE_REVERSED = groups_of("balancingrider", "twod", "invpend", "planarpoint", "bicycle", "bicycle", "planarbike")
# the late riders 3, 4, 5 with their labels rotated, nothing else: every lane would keep a class that is not its rider's
TAKE_CLASS_SWAPPED = groups_of("balancingrider", "bicycle", "invpend", "twod", "bicycle", "planarpoint", "planarbike")
TAKE_REVERSED_SWAPPED = groups_of("balancingrider", "twod", "invpend", "bicycle", "twod", "planarpoint", "planarbike")
SWAP_MOVED = 1e-2                                               # what a stale class must move the comparison by (the issue's bar)


def take_class_scene():
    """(s0 [7, 8], off, dq): the mixed-window scene of 4.10d in the box scene_calib_common.scenes gives the BalancingRider - the scenes of
    scene_mixed_common with such a rider have the wider box too"""
    return widen(one_scene("balancingrider", 7, seed=41))


def class_twin_deviation(states, k, R, first, pods, grp, part, enter, exit, ticks, **hooks):
    """scene_lane_groups_common.twin_deviation where the twin may be narrower than the launch: the twin's state is as wide as the widest
    class AMONG ITS RECORDS, the evaluation's as wide as the widest loaded class - the rows beyond the twin's are rows no class of the
    scene has and must be exactly 0.  -> (largest difference over the twin's rows and the present cells, the twin)"""
    s0, off, dq = part
    n = s0.shape[0]
    tw = general_twin(pods, grp, s0, off, dq, ticks, enter=enter, exit=exit, **hooks)
    got = states[:ticks, k * R + first: k * R + first + n]
    here = inside(enter, exit, ticks)
    w = tw.shape[2]
    assert np.array_equal(np.isfinite(tw).all(axis=2), here)
    assert np.array_equal(np.isnan(got).any(axis=2), ~here) and np.array_equal(np.isnan(got).all(axis=2), ~here)
    assert np.all(got[here][:, w:] == 0.0)
    return (float(np.abs(got[here][:, :w] - tw[here]).max()) if here.any() else 0.0), tw
