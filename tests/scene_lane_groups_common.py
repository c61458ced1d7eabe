"""Shared by tests/test_gpu_scene_lane_groups.py and tests/scene_lane_groups_abi_child.py: rider groups on shared lanes
and on wide scenes - a loaded engine, the scene whose takeovers change a lane's group, and the comparison of an evaluation with the
general-path twins of tests/scene_groups_common.py."""
import numpy as np

from scene_groups_common import GENERAL_TOL, general_twin, group_sets  # noqa: F401
from scene_lanes_common import FEAT, LANES_T, extent, inside, loaded_shared
from scene_wide_common import loaded_wide
from scene_windows_common import one_scene


def firsts(sets):
    """record 0 of every candidate: what an engine is created with, and a candidate list of the length loaded_shared sizes max_sets by"""
    return [c[0] for c in sets]


def loaded_groups(sets, parts, lanes, enter, exit, obj, group=None, n_groups=None, wide_from=None, **kw):
    """scene_lanes_common.loaded_shared (wide_from: scene_wide_common.loaded_wide) for candidates of one record per group, then - with
    `group` - scene_calib_lane_groups"""
    if wide_from is None:
        e = loaded_shared(firsts(sets), parts, lanes, enter, exit, obj, **kw)
    else:
        e = loaded_wide(firsts(sets), parts, lanes, enter, exit, obj, wide_from=wide_from, **kw)
    if group is not None:
        e.scene_calib_lane_groups(np.asarray(group), n_groups)
    return e


# ---- the smallest shape that can go wrong: a roster of 7 on 3 lanes, every lane carries a rider of group a and then one of group b != a
TAKE_T = 60
TAKE_LANE = np.array([0, 1, 2, 0, 1, 2, 0], dtype=np.int32)
TAKE_ENTER = np.array([0, 0, 10, 30, 35, 40, 20], dtype=np.int32)   # lane 0: taken over at the tick it is left; lane 1: after an idle gap;
TAKE_EXIT = np.array([30, 20, 40, 60, 60, 60, 20], dtype=np.int32)  # lane 2: its first rider enters late; rider 6 is never present
TAKE_GROUP = np.array([0, 1, 0, 1, 2, 1, 2], dtype=np.uint8)        # group 2: rider 4 alone (from tick 35) and the rider nobody sees
TAKE_SWAPPED = np.array([0, 1, 0, 2, 1, 0, 2], dtype=np.uint8)      # the labels of the late riders 3, 4, 5 changed, nothing else
TAKE_G = 3


def takeover_scene(model):
    """(s0, off, dq) of the 7 riders: the mixed-window scene of 4.10d"""
    return one_scene(model, 7, seed=41)


def take_objective(ticks=TAKE_T):
    obj = np.random.default_rng(4).normal(size=(ticks, 7, len(FEAT)))
    obj[~inside(TAKE_ENTER, TAKE_EXIT, ticks)] = np.nan
    return obj


def dist(a, b):
    return np.hypot(a[..., 0] - b[..., 0], a[..., 1] - b[..., 1])


def twin_deviation(states, k, R, first, pods, grp, part, enter, exit, ticks, **hooks):
    """candidate k's scene (riders first .. first + n of R) against its general-path twin over the present cells: (largest difference
    over all state rows, the twin).  The launch has NaN exactly where the twin has."""
    s0, off, dq = part
    n = s0.shape[0]
    tw = general_twin(pods, grp, s0, off, dq, ticks, enter=enter, exit=exit, **hooks)
    got = states[:ticks, k * R + first: k * R + first + n]
    here = inside(enter, exit, ticks)
    assert np.array_equal(np.isfinite(tw).all(axis=2), here)
    assert np.array_equal(np.isnan(got).any(axis=2), ~here) and np.array_equal(np.isnan(got).all(axis=2), ~here)
    return (float(np.abs(got[here] - tw[here]).max()) if here.any() else 0.0), tw


def twin_extent_check(what, states, sets, R, first, grp, part, enter, exit, ticks=LANES_T, seed=9):
    """the bar of test_rosters_above_the_lanes_against_the_population_path with general_twin in window_twin's place: positions within
    1e-4 x extent of the twin over the present cells, and a second twin whose starts are moved by 1e-7 m within 1e-5 x extent of the
    first (asserted: a chaotic seed would hide a failure).  Every figure is printed before it is asserted."""
    s0, off, dq = part
    n = s0.shape[0]
    here = inside(enter, exit, ticks)
    s1 = s0.copy()
    s1[:, :2] += 1e-7 * np.random.default_rng(seed).choice([-1.0, 1.0], size=(n, 2))
    worst = chaos = 0.0
    for k, pods in enumerate(sets):
        _, tw = twin_deviation(states, k, R, first, pods, grp, part, enter, exit, ticks)
        got = states[:ticks, k * R + first: k * R + first + n]
        ext = extent(tw)
        dev = float(dist(got[here], tw[here]).max())
        per = general_twin(pods, grp, s1, off, dq, ticks, enter=enter, exit=exit)
        sens = float(dist(per[here], tw[here]).max())
        print(f"{what} candidate {k}: |launch - general-path twin| = {dev:.3e} m = {dev / ext:.2e} x extent; twin moved by 1e-7 m: {sens / ext:.2e} x extent")
        worst, chaos = max(worst, dev / ext), max(chaos, sens / ext)
        assert sens < 1e-5 * ext, (what, k, sens / ext)
        assert dev < 1e-4 * ext, (what, k, dev / ext)
    return worst, chaos
