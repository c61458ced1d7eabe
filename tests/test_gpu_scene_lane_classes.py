"""Vehicle classes on shared lanes and on wide scenes in a closed-loop calibration: csf_scene_calib_lane_classes +
csf_scene_calib_eval_groups on scene_lanes_mixed_kernel and scene_wide_mixed_kernel - against the mixed launch with windows, against twin
engines on the general path that hold the records as parameter classes, against lane groups where all groups are of one class, with
replay and road edges, the refusals and the optimiser.  The bounds are the siblings': GENERAL_TOL on every state row for scenes within 32
lanes and the takeover roster, 1e-4 x extent on positions for rosters above the lanes and wide crowds."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from scene_calib_common import VDES, twin_scene
from scene_groups_common import GENERAL_TOL, group_sets
from scene_lane_classes_common import (CLASSES, G, MODELS, SWAP_MOVED, TAKE_CLASS_GROUP, TAKE_CLASS_SWAPPED, TAKE_REVERSED, TAKE_REVERSED_SWAPPED,
                                       class_twin_deviation, groups_of, loaded_classes, mixed_sets, take_class_scene, widen)
from scene_lane_groups_common import TAKE_ENTER, TAKE_EXIT, TAKE_LANE, TAKE_T, firsts, loaded_groups, take_objective, twin_extent_check
from scene_lanes_common import FEAT, LANES_T, check_sums, greedy_lanes, inside, loaded_plain, peak, roster, sums_over_windows, windows_40, windows_48
from scene_wide_common import always, wide_crowd, windows_80
from scene_windows_common import mixed_windows, one_scene

pytestmark = [pytest.mark.gpu, pytest.mark.auto_variant]

ROUND6 = (np.arange(7) % 6).astype(np.uint8)
NARROW = 4                                                      # state rows 4 .. 7: what a PlanarPoint lacks


# ---- 1: one rider per lane is the mixed launch with windows ------------------------------------------------------------------------------
def test_one_rider_per_lane_is_the_mixed_launch_with_windows():
    """The 7-rider mixed-window scene of 4.10d with lane[r] = r, classes r % 6: csf_scene_calib_load_shared + csf_scene_calib_lane_classes
    against csf_scene_calib_load + csf_scene_calib_windows + csf_scene_calib_classes - the same P, the same source order, the one-wave
    kernel on both sides.  The issue's bound is GENERAL_TOL; measured on the MI355X the two are bit-identical (as 4.10h found for groups),
    so array_equal is what is asserted - on the sums and on every state row of the present cells."""
    ticks, sets = LANES_T, mixed_sets()
    part = take_class_scene()
    (enter, exit), _ = mixed_windows()
    here = inside(enter, exit, ticks)
    obj = np.random.default_rng(4).normal(size=(ticks, 7, len(FEAT)))
    obj[~here] = np.nan
    e = loaded_plain(firsts(sets), [part], obj, enter=enter, exit=exit)
    e.scene_calib_classes(ROUND6, MODELS, part[0])
    want, want_st = e.scene_calib_eval_groups(sets, states=True)
    e.close()
    e = loaded_classes(sets, [part], [(np.arange(7, dtype=np.int32), 7)], enter, exit, obj, ROUND6)
    assert e.ns == 8
    got, got_st = e.scene_calib_eval_groups(sets, states=True)
    assert e.scene_calib_launches() == 1
    e.close()
    assert np.isfinite(want).all() and np.isfinite(got).all() and got_st.shape == want_st.shape
    worst = 0.0
    for k in range(len(sets)):
        a, b = got_st[:, k * 7: (k + 1) * 7], want_st[:, k * 7: (k + 1) * 7]
        assert np.isnan(a[~here]).all() and np.isfinite(a[here]).all()
        worst = max(worst, float(np.abs(a[here] - b[here]).max()))
    same = worst == 0.0 and np.array_equal(got, want)
    print(f"largest |lane classes - mixed launch with windows| = {worst:.3e} ({'bit-identical' if same else 'NOT bit-identical'}; bound {GENERAL_TOL:g})")
    assert worst < GENERAL_TOL
    # (outside a window the plain load's sample shows what the slot holds and the lanes' sample is NaN: the present cells are compared)
    assert same


# ---- 2: a takeover changes the lane's class ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _take(wide, reverse=False):
    """the takeover roster with classes by rider (scene_lane_classes_common), evaluated once per kernel: wide = the same data set with
    wide_from = 1; reverse: lane 1 carries the TwoD first and then the Bicycle"""
    sets = mixed_sets()
    part, obj = take_class_scene(), take_objective()
    grp, swapped = (TAKE_REVERSED, TAKE_REVERSED_SWAPPED) if reverse else (TAKE_CLASS_GROUP, TAKE_CLASS_SWAPPED)
    e = loaded_classes(sets, [part], [(TAKE_LANE, 3)], TAKE_ENTER, TAKE_EXIT, obj, grp, wide_from=1 if wide else None)
    before = e.scene_calib_launches()
    sums, states = e.scene_calib_eval_groups(sets, states=True)
    launches = e.scene_calib_launches() - before
    again = e.scene_calib_eval_groups(sets, states=True)
    perm = [2, 0, 1]
    permuted = e.scene_calib_eval_groups([sets[i] for i in perm], states=True)
    e.scene_calib_lane_classes(swapped, MODELS, part[0])        # the late riders' class labels changed, the records left alone
    _, wrong = e.scene_calib_eval_groups(sets, states=True)
    e.close()
    return dict(sets=sets, part=part, obj=obj, grp=grp, sums=sums, states=states, launches=launches, again=again, perm=(perm, permuted), wrong=wrong)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("wide", [False, True])
def test_a_takeover_changes_the_lanes_class(wide, reverse):
    """7 riders on 3 lanes, T = 60: lane 0 carries a BalancingRider and is taken over by a PlanarPoint at the tick it is left, lane 1 a
    Bicycle and after an idle gap a TwoD (reverse: the TwoD first), lane 2's InvPendulum enters late and a Bicycle follows it; rider 6, a
    PlanarBicycle, is never present.  Every state row against general_twin at GENERAL_TOL over the present cells, on both kernels; the
    rows a PlanarPoint lacks are exactly 0 for rider 3 at every sample; the sums are exactly (0, 0) for rider 6; twice and with the
    candidates permuted array_equal.  With the late riders' class labels swapped and the records left alone the same comparison fails
    by more than 1e-2: the test sees a lane that keeps a stale class.  The seed is checked through twin_extent_check (a twin moved by
    1e-7 m stays within 1e-5 x extent)."""
    job = _take(wide, reverse)
    sets, states, grp = job["sets"], job["states"], job["grp"]
    assert job["launches"] == 1 and np.isfinite(job["sums"]).all() and states.shape[2] == 8
    worst, miss = 0.0, np.inf
    for k, pods in enumerate(sets):
        d, tw = class_twin_deviation(states, k, 7, 0, pods, grp, job["part"], TAKE_ENTER, TAKE_EXIT, TAKE_T)
        here = np.isfinite(tw[..., 0])
        w = float(np.abs(job["wrong"][:, k * 7: (k + 1) * 7][here] - tw[here]).max())
        print(f"wide={wide} reverse={reverse} candidate {k}: |launch - general-path twin| = {d:.3e} (bound {GENERAL_TOL:g}); with the late riders' "
              f"class labels swapped: {w:.3e} (must exceed {SWAP_MOVED:g})")
        worst, miss = max(worst, d), min(miss, w)
        assert d < GENERAL_TOL, (wide, reverse, k, d)
        assert w > SWAP_MOVED, (wide, reverse, k, w)
        rider3 = states[TAKE_ENTER[3]: TAKE_EXIT[3], k * 7 + 3]
        assert np.all(rider3[:, NARROW:] == 0.0) and np.isfinite(rider3[:, :NARROW]).all(), (wide, reverse, k)
    ref = sums_over_windows(states, job["obj"], FEAT, TAKE_ENTER, TAKE_EXIT, len(sets))
    f = check_sums(job["sums"], ref, TAKE_ENTER, TAKE_EXIT, len(FEAT))
    print(f"wide={wide} reverse={reverse}: largest deviation {worst:.3e}, smallest with swapped labels {miss:.3e}, sums at {f:.3f} of the bound 2 m 2^-53")
    assert np.all(job["sums"][:, 6] == 0.0) and np.all(job["sums"][:, :6, 0] > 0.0)
    assert np.array_equal(job["again"][0], job["sums"]) and np.array_equal(job["again"][1], states, equal_nan=True)
    perm, (ps, pst) = job["perm"]
    assert np.array_equal(ps, job["sums"][perm])
    assert np.array_equal(pst.reshape(TAKE_T, 3, 7, -1), states.reshape(TAKE_T, 3, 7, -1)[:, perm], equal_nan=True)
    twin_extent_check(f"takeover wide={wide} reverse={reverse}", states, sets, 7, 0, grp, job["part"], TAKE_ENTER, TAKE_EXIT, TAKE_T)


# ---- 3: rosters above the lanes ----------------------------------------------------------------------------------------------------------
def test_rosters_above_the_lanes_against_general_path_twins():
    """windows_40 (peak 12) and windows_48 on 32 lanes (P = 32: two source groups of lanes), classes r % 6, one data set on the one-wave
    kernel, against general_twin: positions within 1e-4 x extent, a second twin moved by 1e-7 m within 1e-5 x extent (asserted)."""
    ticks, sets = LANES_T, mixed_sets()
    parts = [widen(roster("balancingrider", 40, seed=61)), widen(roster("balancingrider", 48, seed=62))]
    wins = [windows_40(), windows_48()]
    lanes = [greedy_lanes(*w) for w in wins]
    assert [l[1] for l in lanes] == [12, 32] == [peak(*w, ticks) for w in wins]
    groups = [(np.arange(40) % 6).astype(np.uint8), (np.arange(48) % 6).astype(np.uint8)]
    enter, exit = np.concatenate([w[0] for w in wins]), np.concatenate([w[1] for w in wins])
    obj = np.random.default_rng(8).normal(size=(ticks, 88, len(FEAT)))
    obj[~inside(enter, exit, ticks)] = np.nan
    e = loaded_classes(sets, parts, lanes, enter, exit, obj, np.concatenate(groups))
    sums, states = e.scene_calib_eval_groups(sets, states=True)
    assert e.scene_calib_launches() == 1
    e.close()
    assert np.isfinite(sums).all() and np.all(sums[:, 7] == 0.0)
    check_sums(sums, sums_over_windows(states, obj, FEAT, enter, exit, len(sets)), enter, exit, len(FEAT))
    for q, first in enumerate((0, 40)):
        worst, chaos = twin_extent_check(f"roster {parts[q][0].shape[0]}", states, sets, 88, first, groups[q], parts[q], *wins[q])
        print(f"roster {parts[q][0].shape[0]}: largest deviation {worst:.2e} x extent, largest sensitivity to 1e-7 m {chaos:.2e} x extent")


# ---- 4: wide -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 65])
def test_wide_scenes_with_classes_against_general_path_twins(n):
    """n = 33 (P = 64, four source groups: the smallest wide scene) and n = 65 (P = 128: owners in two waves whose per-wave ballots
    differ - the second wave holds rider 64 alone, a PlanarBicycle), classes r % 6, everybody there throughout; positions within
    1e-4 x extent of general_twin, the sensitivity assertion of test 3."""
    sets = mixed_sets()
    part = widen(wide_crowd("balancingrider", n))
    lanes, enter, exit = always(n)
    grp = (np.arange(n) % 6).astype(np.uint8)
    obj = np.random.default_rng(8).normal(size=(LANES_T, n, len(FEAT)))
    e = loaded_classes(sets, [part], [lanes], enter, exit, obj, grp, wide_from=33)
    sums, states = e.scene_calib_eval_groups(sets, states=True)
    assert e.scene_calib_launches() == 1
    e.close()
    assert np.isfinite(sums).all() and np.isfinite(states).all() and np.all(sums[:, :, 0] > 0.0)
    check_sums(sums, sums_over_windows(states, obj, FEAT, enter, exit, len(sets)), enter, exit, len(FEAT))
    twin_extent_check(f"wide n = {n}", states, sets, n, 0, grp, part, enter, exit)


def test_a_roster_of_80_on_40_wide_lanes_whose_takeovers_change_classes():
    """rider r enters at tick r and stays 40 ticks, rider 7 never: 40 lanes of the wide kernel, five classes.  The follower of rider r on
    its lane is rider r + 40, and (r + 40) % 5 == r % 5: with classes r % 5 no takeover would change a class.  The classes are therefore
    (r + r // 40) % 5 - r % 5 for the first occupants, one further for their followers - so that every follower on a lane IS of another
    class (asserted).  The bar and the sensitivity assertion of test 3."""
    sets = mixed_sets()
    part = widen(wide_crowd("twod", 80))
    enter, exit = windows_80()
    lanes = greedy_lanes(enter, exit)
    assert lanes[1] == 40
    grp = ((np.arange(80) + np.arange(80) // 40) % 5).astype(np.uint8)
    lane = lanes[0]
    followers = [(a, b) for a in range(80) for b in range(80) if a != 7 and b != 7 and lane[a] == lane[b] and enter[b] >= exit[a] > enter[a]]
    assert len(followers) >= 30 and all(grp[a] != grp[b] for a, b in followers)
    obj = np.random.default_rng(6).normal(size=(LANES_T, 80, len(FEAT)))
    obj[~inside(enter, exit, LANES_T)] = np.nan
    e = loaded_classes(sets, [part], [lanes], enter, exit, obj, grp, wide_from=33)
    sums, states = e.scene_calib_eval_groups(sets, states=True)
    assert e.scene_calib_launches() == 1
    e.close()
    assert np.all(sums[:, 7] == 0.0) and np.all(sums[:, np.arange(80) != 7, 0] > 0.0) and np.isfinite(sums).all()
    check_sums(sums, sums_over_windows(states, obj, FEAT, enter, exit, len(sets)), enter, exit, len(FEAT))
    twin_extent_check("roster 80", states, sets, 80, 0, grp, part, enter, exit)


def test_a_narrow_and_a_wide_scene_are_two_launches_and_the_narrow_one_is_left_alone():
    """the takeover roster (3 lanes) and a wide scene of 33, wide_from = 33: one evaluation is two launches (csf_scene_calib_launches goes
    up by 2, by 1 on the shared load), and the narrow scene's sums and states are array_equal to the same scene alone on a shared load"""
    sets = mixed_sets()
    take, obj7 = take_class_scene(), take_objective()
    l33, en33, ex33 = always(33, TAKE_T)
    obj = np.concatenate([obj7, np.random.default_rng(5).normal(size=(TAKE_T, 33, len(FEAT)))], axis=1)
    grp = np.r_[TAKE_CLASS_GROUP, np.arange(33) % 6].astype(np.uint8)
    e = loaded_classes(sets, [take, widen(wide_crowd("balancingrider", 33))], [(TAKE_LANE, 3), l33], np.r_[TAKE_ENTER, en33], np.r_[TAKE_EXIT, ex33], obj, grp,
                       wide_from=33)
    before = e.scene_calib_launches()
    got, got_st = e.scene_calib_eval_groups(sets, states=True)
    assert e.scene_calib_launches() - before == 2
    e.close()
    alone = _take(False)
    assert alone["launches"] == 1
    assert np.isfinite(got).all() and np.array_equal(got[:, :7], alone["sums"]) and np.all(got[:, 7:, 0] > 0.0)
    a = got_st.reshape(TAKE_T, 3, 40, -1)
    assert np.array_equal(a[:, :, :7], alone["states"].reshape(TAKE_T, 3, 7, -1), equal_nan=True) and np.isfinite(a[:, :, 7:]).all()


# ---- 5: one class is today's -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("model", CLASSES)
def test_one_class_is_todays(model, wide):
    """All four groups are of one class: scene_calib_lane_classes against the same data through scene_calib_lane_groups (G = 4) on the
    takeover roster, on both kernels.  The issue's bound is GENERAL_TOL (another compilation of agent_body; the order of every sum is
    kept); measured on the MI355X the two are bit-identical for all six classes on both kernels (as 4.10i found on the plain load), so
    array_equal is what is asserted."""
    from cyclistsocialforce_amd.engine import MODEL_IDS
    sets = group_sets(model, 3, 4)
    part, obj = widen(one_scene(model, 7, seed=41)), take_objective()
    grp = (np.arange(7) % 4).astype(np.uint8)
    kw = dict(wide_from=1 if wide else None)
    e = loaded_groups(sets, [part], [(TAKE_LANE, 3)], TAKE_ENTER, TAKE_EXIT, obj, grp, 4, **kw)
    want, want_st = e.scene_calib_eval_groups(sets, states=True)
    e.close()
    e = loaded_classes(sets, [part], [(TAKE_LANE, 3)], TAKE_ENTER, TAKE_EXIT, obj, grp, [MODEL_IDS[model]] * 4, **kw)
    got, got_st = e.scene_calib_eval_groups(sets, states=True)
    e.close()
    here = np.isfinite(want_st)
    assert got_st.shape == want_st.shape and np.array_equal(np.isfinite(got_st), here) and np.isfinite(got).all()
    diff = float(np.abs(got_st[here] - want_st[here]).max())
    same = np.array_equal(got, want) and np.array_equal(got_st, want_st, equal_nan=True)
    print(f"{model} wide={wide}: one class through the class-carrying kernel against lane groups: {diff:.3e} ({'bit-identical' if same else 'NOT bit-identical'})")
    assert diff < GENERAL_TOL
    assert same


# ---- 6: labels are only labels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
def test_labels_are_only_labels(wide):
    """the labels permuted together with `models` and the records of every candidate: array_equal sums and states on both kernels - the
    sources of a receiver are summed in lane order whatever their group or class.  (Every record of a candidate of mixed_sets has one
    priority rule; the engine is created with the same record either way.)"""
    job = _take(wide)
    pi = np.array([3, 5, 0, 1, 2, 4])                            # group g becomes group pi[g]
    inv = np.argsort(pi)
    e = loaded_classes(job["sets"], [job["part"]], [(TAKE_LANE, 3)], TAKE_ENTER, TAKE_EXIT, job["obj"], pi[TAKE_CLASS_GROUP].astype(np.uint8), MODELS[inv],
                       wide_from=1 if wide else None)
    s1, st1 = e.scene_calib_eval_groups([tuple(p[g] for g in inv) for p in job["sets"]], states=True)
    e.close()
    assert np.array_equal(job["sums"], s1) and np.array_equal(job["states"], st1, equal_nan=True)


# ---- 7: no classes means today -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
def test_no_classes_means_today(wide):
    """after scene_calib_lane_classes(None) the plain evaluation is array_equal to the one before the call and the state width is the
    engine's own; scene_calib_lane_groups after the classes gives the grouped bits of an engine that never held classes"""
    job = _take(wide)
    ones = firsts(job["sets"])
    two = group_sets("twod", 3, 3)
    grp3 = (np.arange(7) % 3).astype(np.uint8)
    kw = dict(wide_from=1 if wide else None)
    e = loaded_groups(job["sets"], [job["part"]], [(TAKE_LANE, 3)], TAKE_ENTER, TAKE_EXIT, job["obj"], grp3, 3, **kw)   # (the same engine either way)
    grouped = e.scene_calib_eval_groups(two, states=True)
    e.close()
    e = loaded_classes(job["sets"], [job["part"]], [(TAKE_LANE, 3)], TAKE_ENTER, TAKE_EXIT, job["obj"], **kw)
    own = e.ns
    s0, st0 = e.scene_calib_eval(ones, states=True)
    e.scene_calib_lane_classes(TAKE_CLASS_GROUP, MODELS, job["part"][0])
    assert e.ns == 8
    s1, st1 = e.scene_calib_eval_groups(job["sets"], states=True)
    assert np.array_equal(s1, job["sums"]) and np.array_equal(st1, job["states"], equal_nan=True)
    e.scene_calib_lane_classes(None)
    assert e.ns == own
    s2, st2 = e.scene_calib_eval(ones, states=True)
    assert np.array_equal(s0, s2) and np.array_equal(st0, st2, equal_nan=True)
    e.scene_calib_lane_classes(TAKE_CLASS_GROUP, MODELS, job["part"][0])
    e.scene_calib_lane_groups(grp3, 3)                           # (replaces the classes)
    assert e.ns == own
    s3, st3 = e.scene_calib_eval_groups(two, states=True)
    e.close()
    assert np.array_equal(s3, grouped[0]) and np.array_equal(st3, grouped[1], equal_nan=True)


# ---- 8: replay and road edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
def test_replayed_riders_take_over_lanes_of_other_classes(wide):
    """6 riders on 4 lanes, T = 60: a replayed BalancingRider (rider 3, [15, 50)) follows a simulated InvPendulum (rider 2, [0, 15)) on its
    lane, and a replayed TwoD (rider 5, [20, 55)) follows a simulated Bicycle (rider 4, [0, 20)).  Rows 0 - 3 of the replayed riders ARE
    the recording inside their windows and their sums (0, 0); every state row against general_twin, which pushes the recording after
    every tick, at GENERAL_TOL."""
    from cyclistsocialforce_amd import parameters
    ticks = 60
    sets = mixed_sets()
    s0, off, dq = widen(one_scene("balancingrider", 6, seed=44))
    rec = twin_scene(parameters.default_pod("twod"), s0[:, :5], off, dq, ticks)[0]
    enter = np.array([0, 0, 0, 15, 0, 20], dtype=np.int32)
    exit = np.array([ticks, ticks, 15, 50, 20, 55], dtype=np.int32)
    s0 = s0.copy()
    for r in (3, 5):
        s0[r] = 0.0
        s0[r, :4] = rec[enter[r] - 1, r, :4]
    rec = rec.copy()
    rec[~inside(enter, exit, ticks)] = np.nan
    mask = np.array([False, False, False, True, False, True])
    grp = groups_of("planarbike", "planarpoint", "invpend", "balancingrider", "bicycle", "twod")
    lane, nl = greedy_lanes(enter, exit)
    assert nl == 4 and lane[3] == lane[2] and lane[5] == lane[4]
    obj = np.random.default_rng(1).normal(size=(ticks, 6, len(FEAT)))
    e = loaded_classes(sets, [(s0, off, dq)], [(lane, nl)], enter, exit, obj, grp, wide_from=1 if wide else None)
    rows = np.nan_to_num(rec[:, mask, :4])
    e.scene_calib_replay(mask, rows)
    sums, states = e.scene_calib_eval_groups(sets, states=True)
    e.close()
    assert np.all(sums[:, mask] == 0.0) and np.all(sums[:, ~mask, 0] > 0.0)
    for k, pods in enumerate(sets):
        dev, _ = class_twin_deviation(states, k, 6, 0, pods, grp, (s0, off, dq), enter, exit, ticks, replayed=mask, rec=rec)
        for r in (3, 5):
            assert np.array_equal(states[enter[r]: exit[r], k * 6 + r, :4], rec[enter[r]: exit[r], r, :4])
        print(f"wide={wide} candidate {k}: largest |launch - push_state twin| = {dev:.3e} (bound {GENERAL_TOL:g})")
        assert dev < GENERAL_TOL, (wide, k, dev)


@pytest.mark.parametrize("wide", [False, True])
def test_lane_classes_with_road_edges_and_road_parameters_per_candidate(wide):
    """the takeover roster with two polylines beside its box, F_0 and sigma of all vertices replaced per candidate (an integer sigma and a
    fractional one); against general_twin with that road set by set_road, at GENERAL_TOL"""
    from scene_road_common import box_of
    job = _take(wide)
    sets = job["sets"]
    f0s, sgs = np.array([0.4, 0.9, 0.2]), np.array([2.0, 3.0, 2.5])
    box = box_of("balancingrider", 7)
    lines = [np.c_[np.linspace(-20.0, box + 20.0, c), np.full(c, y)] for c, y in ((40, -3.0), (23, box + 3.0))]
    roff = np.array([0, 40, 63], dtype=np.int64)
    e = loaded_classes(sets, [job["part"]], [(TAKE_LANE, 3)], TAKE_ENTER, TAKE_EXIT, job["obj"], TAKE_CLASS_GROUP, wide_from=1 if wide else None)
    e.scene_calib_road(np.zeros(2, dtype=np.int32), roff, np.concatenate(lines), 0.3, 2.0)
    sums, states = e.scene_calib_eval_groups(sets, road_F0=f0s, road_sigma=sgs, states=True)
    sums2, _ = e.scene_calib_eval_groups(sets[::-1], road_F0=f0s[::-1], road_sigma=sgs[::-1], states=True)
    e.close()
    assert np.isfinite(sums).all() and not np.array_equal(sums, job["sums"]) and np.array_equal(sums2[::-1], sums)
    for k, pods in enumerate(sets):
        road = (roff, np.concatenate(lines), np.full(2, f0s[k]), np.full(2, sgs[k]))
        dev, _ = class_twin_deviation(states, k, 7, 0, pods, TAKE_CLASS_GROUP, job["part"], TAKE_ENTER, TAKE_EXIT, TAKE_T, road=road)
        print(f"wide={wide} candidate {k}: road, largest |launch - general-path twin| = {dev:.3e} (bound {GENERAL_TOL:g})")
        assert dev < GENERAL_TOL, (wide, k, dev)


# ---- 10: recovery ------------------------------------------------------------------------------------------------------------------------
def test_two_classes_f_0_are_recovered_on_a_roster_of_40():
    """TwoDBicycles and InvPendulumBicycles with true f_0 of 1.0 x and 1.6 x the default on the roster of 40 (windows_40: 12 lanes): the
    scene is recorded with the true sets on shared lanes, its leave-one-out scenes (ego_split: 39, rider 7 is never present) are fitted
    through InteractionCalibration(vehicle_type=[TwoDBicycle, InvPendulumBicycle], lane_classes=True) for (("f_0", 0), ("f_0", 1)) from
    a guess 20 % off; both values within 1e-3 relative."""
    from cyclistsocialforce_amd import calibration as cal, parameters, vehicle
    from cyclistsocialforce_amd.engine import MODEL_IDS
    base = [parameters.default_pod("twod"), parameters.default_pod("invpend")]
    true = np.array([base[0].f_0, 1.6 * base[1].f_0])
    s0, off, dq = widen(roster("invpend", 40, seed=61))
    enter, exit = windows_40()
    grp = (np.arange(40) % 2).astype(np.uint8)
    truth = [(parameters.default_pod("twod", f_0=true[0]), parameters.default_pod("invpend", f_0=true[1]))]
    e = loaded_classes(truth, [(s0, off, dq)], [greedy_lanes(enter, exit)], enter, exit, np.zeros((LANES_T, 40, 2)), grp,
                       [MODEL_IDS["twod"], MODEL_IDS["invpend"]], feat=np.array([0, 1], dtype=np.int32))
    _, traj = e.scene_calib_eval_groups(truth, states=True)
    e.close()
    data = cal.SceneData(s0, VDES, off, dq, traj[:, :, :4], group=grp, present=(enter, exit)).ego_split()
    assert len(data) == 39
    c = cal.InteractionCalibration([vehicle.TwoDBicycle, vehicle.InvPendulumBicycle], [("f_0", 0), ("f_0", 1)], data, data, [1, 1, 0, 0, 0, 0],
                                   max_sets=8, maxiter=400, xtol=1e-4, ftol=1e-30, lane_classes=True)
    guess = true * np.array([1.2, 0.8])
    f_start = float(c.evaluate([guess])[0])
    res = c.run(guess)
    rel = np.abs(res[0] - true) / true
    print(f"recovered f_0 = {res[0]} (true {true}): relative {rel}, objective {res[1]:.3e} from {f_start:.3e}, {res[2]} iterations")
    c.close()
    assert rel.max() < 1e-3


# ---- 11: refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_lifetime_in_a_fresh_process():
    """every refusal of csf_scene_calib_lane_classes and of the evaluation calls comes back with its code and a message and is followed by
    an array_equal evaluation; classes and lane groups replace each other; classes before or after replay and a road give the same
    bits; after clear the engine has its own state width and ticks a small population on the one-wave path"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k != "CSF_PAIR_VARIANT"}
    r = subprocess.run([sys.executable, os.path.join(here, "scene_lane_classes_abi_child.py"), "abi"], capture_output=True, text=True, timeout=600,
                       env={**env, "PYTHONPATH": os.path.dirname(here) + os.pathsep + here})
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "scene lane classes abi ok" in r.stdout
