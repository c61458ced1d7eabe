"""Rider groups on shared lanes and on wide scenes in a closed-loop calibration: csf_scene_calib_lane_groups +
csf_scene_calib_eval_groups on scene_lanes_groups_kernel and scene_wide_groups_kernel - against the grouped launch with windows, against
twin engines on the general path that hold per-vehicle parameter sets, against NumPy on the call's own states, against the evaluation
without groups, with replay and road edges, the refusals and the optimiser."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from scene_calib_common import MODELS, VDES, twin_scene
from scene_groups_common import GENERAL_TOL, group_sets
from scene_lane_groups_common import (TAKE_ENTER, TAKE_EXIT, TAKE_G, TAKE_GROUP, TAKE_LANE, TAKE_SWAPPED, TAKE_T, firsts, loaded_groups,
                                      take_objective, takeover_scene, twin_deviation, twin_extent_check)
from scene_lanes_common import (FEAT, LANES_T, TWIN_TOL, check_sums, greedy_lanes, inside, loaded_plain, peak, roster, sums_over_windows,
                                windows_40, windows_48)
from scene_wide_common import always, wide_crowd, windows_80
from scene_windows_common import mixed_windows, one_scene

pytestmark = [pytest.mark.gpu, pytest.mark.auto_variant]


# ---- 1: one rider per lane is the grouped launch with windows --------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_one_rider_per_lane_is_the_grouped_launch_with_windows(model):
    """The 7-rider mixed-window scene of 4.10d with lane[r] = r, groups r % 3: csf_scene_calib_load_shared + csf_scene_calib_lane_groups
    against csf_scene_calib_load + csf_scene_calib_windows + csf_scene_calib_groups - the same P, the same source order.  Expected
    array_equal; the two kernels are separate compilations of agent_body, so should it hold only at TWIN_TOL, that is asserted and the
    largest difference printed (the precedent of test_a_relay_equals_two_scenes_without_windows)."""
    ticks, sets = LANES_T, group_sets(model, 3, 3)
    part = one_scene(model, 7, seed=41)
    (enter, exit), _ = mixed_windows()
    grp = (np.arange(7) % 3).astype(np.uint8)
    here = inside(enter, exit, ticks)
    obj = np.random.default_rng(4).normal(size=(ticks, 7, len(FEAT)))
    obj[~here] = np.nan
    e = loaded_plain(firsts(sets), [part], obj, enter=enter, exit=exit)
    e.scene_calib_groups(grp, 3)
    want, want_st = e.scene_calib_eval_groups(sets, states=True)
    e.close()
    e = loaded_groups(sets, [part], [(np.arange(7, dtype=np.int32), 7)], enter, exit, obj, grp, 3)
    got, got_st = e.scene_calib_eval_groups(sets, states=True)
    assert e.scene_calib_launches() == 1
    e.close()
    assert np.isfinite(want).all() and np.isfinite(got).all()
    worst = 0.0
    for k in range(len(sets)):
        a, b = got_st[:, k * 7: (k + 1) * 7], want_st[:, k * 7: (k + 1) * 7]
        assert np.isnan(a[~here]).all() and np.isfinite(a[here]).all()
        worst = max(worst, float(np.abs(a[here] - b[here]).max()))
    same = worst == 0.0 and np.array_equal(got, want)
    print(f"{model}: largest |lane groups - grouped launch with windows| = {worst:.3e} ({'bit-identical' if same else 'NOT bit-identical'})")
    for k in range(len(sets)):
        a, b = got_st[:, k * 7: (k + 1) * 7], want_st[:, k * 7: (k + 1) * 7]
        np.testing.assert_allclose(a[here], b[here], rtol=TWIN_TOL, atol=TWIN_TOL, err_msg=f"candidate {k}")
    np.testing.assert_allclose(got, want, rtol=TWIN_TOL, atol=0.0)


# ---- 2: a takeover changes the lane's group ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _take(model, wide):
    """the takeover scene (scene_lane_groups_common) evaluated once per kernel: wide = the same data set with wide_from = 1"""
    sets = group_sets(model, 3, TAKE_G)
    part, obj = takeover_scene(model), take_objective()
    e = loaded_groups(sets, [part], [(TAKE_LANE, 3)], TAKE_ENTER, TAKE_EXIT, obj, TAKE_GROUP, TAKE_G, wide_from=1 if wide else None)
    sums, states = e.scene_calib_eval_groups(sets, states=True)
    launches = e.scene_calib_launches()
    again = e.scene_calib_eval_groups(sets, states=True)
    perm = [2, 0, 1]
    permuted = e.scene_calib_eval_groups([sets[i] for i in perm], states=True)
    e.scene_calib_lane_groups(TAKE_SWAPPED, TAKE_G)              # the late riders' labels changed, the records left alone
    _, wrong = e.scene_calib_eval_groups(sets, states=True)
    e.close()
    return dict(sets=sets, part=part, obj=obj, sums=sums, states=states, launches=launches, again=again, perm=(perm, permuted), wrong=wrong)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("model", MODELS)
def test_a_takeover_changes_the_lanes_group(model, wide):
    """A roster of 7 on 3 lanes, T = 60 (six riders ride; the seventh is never present): every lane carries a rider of group a and then
    one of group b != a - lane 0 is taken over at the very tick it is left, lane 1 after an idle gap, lane 2's first rider enters late;
    group 2 is carried by one late rider alone, so the ballot skips it at first.  Against general_twin at GENERAL_TOL on every state row
    over the present cells; the sums against NumPy on the call's own states, exactly (0, 0) for the absent rider; twice and permuted
    array_equal.  The same evaluation with the late riders' labels swapped, records left alone, differs from the twin by more than the
    tolerance: the test catches a lane that keeps its first rider's group.  wide: the same data set on scene_wide_groups_kernel."""
    job = _take(model, wide)
    sets, states = job["sets"], job["states"]
    assert job["launches"] == 1 and np.isfinite(job["sums"]).all()
    worst, miss = 0.0, np.inf
    for k, pods in enumerate(sets):
        d, tw = twin_deviation(states, k, 7, 0, pods, TAKE_GROUP, job["part"], TAKE_ENTER, TAKE_EXIT, TAKE_T)
        here = np.isfinite(tw[..., 0])
        w = float(np.abs(job["wrong"][:, k * 7: (k + 1) * 7][here] - tw[here]).max())
        print(f"{model} wide={wide} candidate {k}: |launch - general-path twin| = {d:.3e} (bound {GENERAL_TOL:g}); with the late riders' labels "
              f"swapped: {w:.3e}")
        worst, miss = max(worst, d), min(miss, w)
        assert d < GENERAL_TOL, (model, wide, k, d)
        assert w > GENERAL_TOL, (model, wide, k, w)
    ref = sums_over_windows(states, job["obj"], FEAT, TAKE_ENTER, TAKE_EXIT, len(sets))
    f = check_sums(job["sums"], ref, TAKE_ENTER, TAKE_EXIT, len(FEAT))
    print(f"{model} wide={wide}: largest deviation {worst:.3e}, smallest with swapped labels {miss:.3e}, sums at {f:.3f} of the bound 2 m 2^-53")
    assert np.all(job["sums"][:, 6] == 0.0) and np.all(job["sums"][:, :6, 0] > 0.0)
    assert np.array_equal(job["again"][0], job["sums"]) and np.array_equal(job["again"][1], states, equal_nan=True)
    perm, (ps, pst) = job["perm"]
    assert np.array_equal(ps, job["sums"][perm])
    assert np.array_equal(pst.reshape(TAKE_T, 3, 7, -1), states.reshape(TAKE_T, 3, 7, -1)[:, perm], equal_nan=True)


# ---- 3: rosters above the lanes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_rosters_above_the_lanes_against_general_path_twins(model):
    """windows_40 (peak 12) with groups r % 4 and windows_48 on 32 lanes (P = 32: two source groups of lanes) with groups r % 3, one data
    set, against general_twin at the bar of test_rosters_above_the_lanes_against_the_population_path: positions within 1e-4 x extent,
    a second twin moved by 1e-7 m within 1e-5 x extent of the first (asserted)."""
    ticks, sets = LANES_T, group_sets(model, 3, 4)
    parts = [roster(model, 40, seed=61), roster(model, 48, seed=62)]
    wins = [windows_40(), windows_48()]
    lanes = [greedy_lanes(*w) for w in wins]
    assert [l[1] for l in lanes] == [12, 32] == [peak(*w, ticks) for w in wins]
    groups = [(np.arange(40) % 4).astype(np.uint8), (np.arange(48) % 3).astype(np.uint8)]
    enter, exit = np.concatenate([w[0] for w in wins]), np.concatenate([w[1] for w in wins])
    obj = np.random.default_rng(8).normal(size=(ticks, 88, len(FEAT)))
    obj[~inside(enter, exit, ticks)] = np.nan
    e = loaded_groups(sets, parts, lanes, enter, exit, obj, np.concatenate(groups), 4)
    sums, states = e.scene_calib_eval_groups(sets, states=True)
    assert e.scene_calib_launches() == 1
    e.close()
    assert np.isfinite(sums).all() and np.all(sums[:, 7] == 0.0)
    check_sums(sums, sums_over_windows(states, obj, FEAT, enter, exit, len(sets)), enter, exit, len(FEAT))
    for q, first in enumerate((0, 40)):
        worst, chaos = twin_extent_check(f"{model} roster {parts[q][0].shape[0]}", states, sets, 88, first, groups[q], parts[q], *wins[q])
        print(f"{model} roster {parts[q][0].shape[0]}: largest deviation {worst:.2e} x extent, largest sensitivity to 1e-7 m {chaos:.2e} x extent")


# ---- 4: wide -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,n", [(m, n) for n in (33, 65) for m in MODELS])
def test_wide_scenes_with_groups_against_general_path_twins(model, n):
    """n = 33 (P = 64, G = 4) and n = 65 (P = 128: the owners cross a wave boundary, and with groups r % 4 over 65 lanes the second owning
    wave holds one rider - of group 0 - so it skips three of the four passes), everybody there throughout; the bar and the sensitivity
    assertion of test 3."""
    sets = group_sets(model, 3, 4)
    part = wide_crowd(model, n)
    lanes, enter, exit = always(n)
    grp = (np.arange(n) % 4).astype(np.uint8)
    obj = np.random.default_rng(8).normal(size=(LANES_T, n, len(FEAT)))
    e = loaded_groups(sets, [part], [lanes], enter, exit, obj, grp, 4, wide_from=33)
    sums, states = e.scene_calib_eval_groups(sets, states=True)
    assert e.scene_calib_launches() == 1
    e.close()
    assert np.isfinite(sums).all() and np.isfinite(states).all() and np.all(sums[:, :, 0] > 0.0)
    check_sums(sums, sums_over_windows(states, obj, FEAT, enter, exit, len(sets)), enter, exit, len(FEAT))
    twin_extent_check(f"{model} n = {n}", states, sets, n, 0, grp, part, enter, exit)


@pytest.mark.parametrize("model", ["twod", "invpend"])
def test_a_roster_of_80_on_40_wide_lanes_whose_takeovers_change_groups(model):
    """rider r enters at tick r and stays 40 ticks, rider 7 never: 40 lanes of the wide kernel; with groups r % 3 the follower of rider r
    on its lane - rider r + 40 - is of another group ((r + 40) % 3 != r % 3).  The bar and the sensitivity assertion of test 3."""
    sets = group_sets(model, 3, 3)
    part = wide_crowd(model, 80)
    enter, exit = windows_80()
    lanes = greedy_lanes(enter, exit)
    assert lanes[1] == 40
    grp = (np.arange(80) % 3).astype(np.uint8)
    lane = lanes[0]
    followers = [(a, b) for a in range(80) for b in range(80) if a != 7 and b != 7 and lane[a] == lane[b] and enter[b] >= exit[a] > enter[a]]
    assert len(followers) >= 30 and all(grp[a] != grp[b] for a, b in followers)
    obj = np.random.default_rng(6).normal(size=(LANES_T, 80, len(FEAT)))
    obj[~inside(enter, exit, LANES_T)] = np.nan
    e = loaded_groups(sets, [part], [lanes], enter, exit, obj, grp, 3, wide_from=33)
    sums, states = e.scene_calib_eval_groups(sets, states=True)
    assert e.scene_calib_launches() == 1
    e.close()
    assert np.all(sums[:, 7] == 0.0) and np.all(sums[:, np.arange(80) != 7, 0] > 0.0) and np.isfinite(sums).all()
    check_sums(sums, sums_over_windows(states, obj, FEAT, enter, exit, len(sets)), enter, exit, len(FEAT))
    twin_extent_check(f"{model} roster 80", states, sets, 80, 0, grp, part, enter, exit)


@pytest.mark.parametrize("model", MODELS)
def test_a_mixed_grouped_data_set_is_two_launches_and_leaves_the_narrow_scene_alone(model):
    """the takeover scene (3 lanes) and a wide scene of 33, wide_from = 33: one evaluation is two launches, and the narrow scene's sums
    and states are array_equal to the same scene evaluated alone on a shared load with lane groups"""
    sets = group_sets(model, 3, TAKE_G)
    take, obj7 = takeover_scene(model), take_objective()
    l33, en33, ex33 = always(33, TAKE_T)
    obj = np.concatenate([obj7, np.random.default_rng(5).normal(size=(TAKE_T, 33, len(FEAT)))], axis=1)
    grp = np.r_[TAKE_GROUP, np.arange(33) % 3].astype(np.uint8)
    e = loaded_groups(sets, [take, wide_crowd(model, 33)], [(TAKE_LANE, 3), l33], np.r_[TAKE_ENTER, en33], np.r_[TAKE_EXIT, ex33], obj, grp, TAKE_G,
                      wide_from=33)
    got, got_st = e.scene_calib_eval_groups(sets, states=True)
    assert e.scene_calib_launches() == 2
    e.close()
    alone = _take(model, False)
    assert np.isfinite(got).all() and np.array_equal(got[:, :7], alone["sums"]) and np.all(got[:, 7:, 0] > 0.0)
    a = got_st.reshape(TAKE_T, 3, 40, -1)
    assert np.array_equal(a[:, :, :7], alone["states"].reshape(TAKE_T, 3, 7, -1), equal_nan=True) and np.isfinite(a[:, :, 7:]).all()


# ---- 5: labels are only labels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("model", MODELS)
def test_labels_are_only_labels(model, wide):
    """swapping the labels 0 and 1 in `group` together with the two records of every candidate gives array_equal sums and states on both
    new kernels: the sources of a receiver are summed in lane order whatever their group.  Candidates 0 and 1 of group_sets: all their
    records share one priority rule (the rule of a candidate is its FIRST record's, which the swap would change in the last one)."""
    job = _take(model, wide)
    sets = job["sets"][:2]
    swapped = TAKE_GROUP.copy()
    swapped[TAKE_GROUP == 0], swapped[TAKE_GROUP == 1] = 1, 0
    e = loaded_groups(job["sets"], [job["part"]], [(TAKE_LANE, 3)], TAKE_ENTER, TAKE_EXIT, job["obj"], swapped, TAKE_G, wide_from=1 if wide else None)
    s1, st1 = e.scene_calib_eval_groups([(p[1], p[0], p[2]) for p in sets], states=True)
    e.close()
    assert np.array_equal(job["sums"][:2], s1) and np.array_equal(job["states"][:, :14], st1, equal_nan=True)


# ---- 6, 8: identical groups; no lane groups means today ------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("model", MODELS)
def test_identical_groups_and_no_groups(model, wide):
    """Candidates whose three records are one set agree with the ungrouped kernel's evaluation of that set at TWIN_TOL (another
    compilation of agent_body; the order of every sum is kept), the largest difference printed.  After scene_calib_lane_groups(None),
    and with n_groups = 1, the evaluation is array_equal to a never-grouped engine's: the kernels launched are the ungrouped ones."""
    job = _take(model, wide)
    ones = firsts(job["sets"])
    kw = dict(wide_from=1 if wide else None)
    plain = loaded_groups(job["sets"], [job["part"]], [(TAKE_LANE, 3)], TAKE_ENTER, TAKE_EXIT, job["obj"], **kw)
    s0, st0 = plain.scene_calib_eval(ones, states=True)
    s1, st1 = plain.scene_calib_eval_groups([(p,) for p in ones], states=True)      # (no groups loaded: n_groups == 1)
    plain.close()
    assert np.array_equal(s0, s1) and np.array_equal(st0, st1, equal_nan=True)
    e = loaded_groups(job["sets"], [job["part"]], [(TAKE_LANE, 3)], TAKE_ENTER, TAKE_EXIT, job["obj"], TAKE_GROUP, TAKE_G, **kw)
    same, same_st = e.scene_calib_eval_groups([(p, p, p) for p in ones], states=True)
    e.scene_calib_lane_groups(None)
    s2, st2 = e.scene_calib_eval(ones, states=True)
    s3, st3 = e.scene_calib_eval_groups([(p,) for p in ones], states=True)
    e.scene_calib_lane_groups(TAKE_GROUP, 1)                          # (n_groups <= 1 drops them as well)
    s4, st4 = e.scene_calib_eval(ones, states=True)
    e.close()
    for s, st in ((s2, st2), (s3, st3), (s4, st4)):
        assert np.array_equal(s0, s) and np.array_equal(st0, st, equal_nan=True)
    here = np.isfinite(st0)
    assert np.array_equal(np.isfinite(same_st), here)
    diff = float(np.abs(same_st[here] - st0[here]).max())
    print(f"{model} wide={wide}: identical groups against the ungrouped kernel: {diff:.3e} (bound {TWIN_TOL:g})")
    np.testing.assert_allclose(same_st[here], st0[here], rtol=TWIN_TOL, atol=TWIN_TOL)
    np.testing.assert_allclose(same, s0, rtol=TWIN_TOL, atol=0.0)


# ---- 7: with the other hooks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("model", MODELS)
def test_a_replayed_rider_of_group_1_follows_a_simulated_one(model, wide):
    """5 riders on 4 lanes, T = 60: rider 3 (group 0) is simulated over [0, 15) and the replayed rider 4 (group 1) follows it on the same
    lane over [15, 50).  Rows 0 - 3 of the replayed rider ARE its recording inside its window and its sums (0, 0); every state row of
    the simulated riders against general_twin, which pushes the recording after every tick, at GENERAL_TOL."""
    from cyclistsocialforce_amd import calibration as cal
    ticks, a, b = 60, 15, 50
    sets = group_sets(model, 3, 3)
    s0, off, dq = one_scene(model, 5, seed=44)
    rec = twin_scene(sets[1][0], s0, off, dq, ticks)[0]
    s0 = s0.copy()
    s0[4] = rec[a - 1, 4]
    rec = rec.copy()
    rec[:a, 4] = rec[b:, 4] = np.nan
    enter, exit = np.array([0, 0, 0, 0, a], dtype=np.int32), np.array([ticks, ticks, ticks, a, b], dtype=np.int32)
    mask = np.array([False, False, False, False, True])
    grp = np.array([0, 1, 2, 0, 1], dtype=np.uint8)
    d = cal.SceneData(s0, VDES, off, dq, rec[:, :, :4], replayed=mask, present=(enter, exit))
    lane, nl = d.lanes()
    assert nl == 4 and lane[4] == lane[3] == 3
    obj = np.random.default_rng(1).normal(size=(ticks, 5, len(FEAT)))
    e = loaded_groups(sets, [(s0, off, dq)], [(lane, nl)], enter, exit, obj, grp, 3, wide_from=1 if wide else None)
    e.scene_calib_replay(mask, d.replay_rows())
    sums, states = e.scene_calib_eval_groups(sets, states=True)
    e.close()
    assert np.all(sums[:, 4] == 0.0) and np.all(sums[:, :4, 0] > 0.0)
    for k, pods in enumerate(sets):
        dev, _ = twin_deviation(states, k, 5, 0, pods, grp, (s0, off, dq), enter, exit, ticks, replayed=mask, rec=rec)
        assert np.array_equal(states[a:b, k * 5 + 4, :4], rec[a:b, 4, :4])
        print(f"{model} wide={wide} candidate {k}: largest |launch - push_state twin| = {dev:.3e} (bound {GENERAL_TOL:g})")
        assert dev < GENERAL_TOL, (model, wide, k, dev)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("model", MODELS)
def test_lane_groups_with_road_edges_and_road_parameters_per_candidate(model, wide):
    """the takeover scene with two polylines beside its box, F_0 and sigma of all vertices replaced per candidate (an integer sigma and
    a fractional one); against general_twin with that road set by set_road, at GENERAL_TOL"""
    from scene_road_common import box_of
    job = _take(model, wide)
    sets = job["sets"]
    f0s, sgs = np.array([0.4, 0.9, 0.2]), np.array([2.0, 3.0, 2.5])
    box = box_of(model, 7)
    lines = [np.c_[np.linspace(-20.0, box + 20.0, c), np.full(c, y)] for c, y in ((40, -3.0), (23, box + 3.0))]
    roff = np.array([0, 40, 63], dtype=np.int64)
    e = loaded_groups(sets, [job["part"]], [(TAKE_LANE, 3)], TAKE_ENTER, TAKE_EXIT, job["obj"], TAKE_GROUP, TAKE_G, wide_from=1 if wide else None)
    e.scene_calib_road(np.zeros(2, dtype=np.int32), roff, np.concatenate(lines), 0.3, 2.0)
    sums, states = e.scene_calib_eval_groups(sets, road_F0=f0s, road_sigma=sgs, states=True)
    sums2, states2 = e.scene_calib_eval_groups(sets[::-1], road_F0=f0s[::-1], road_sigma=sgs[::-1], states=True)
    e.close()
    assert np.isfinite(sums).all() and not np.array_equal(sums, job["sums"]) and np.array_equal(sums2[::-1], sums)
    for k, pods in enumerate(sets):
        road = (roff, np.concatenate(lines), np.full(2, f0s[k]), np.full(2, sgs[k]))
        dev, _ = twin_deviation(states, k, 7, 0, pods, TAKE_GROUP, job["part"], TAKE_ENTER, TAKE_EXIT, TAKE_T, road=road)
        print(f"{model} wide={wide} candidate {k}: road, largest |launch - general-path twin| = {dev:.3e} (bound {GENERAL_TOL:g})")
        assert dev < GENERAL_TOL, (model, wide, k, dev)


# ---- 9: refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_lifetime_in_a_fresh_process():
    """every refusal of csf_scene_calib_lane_groups and of the evaluation calls comes back with its code and a message and is followed by
    an array_equal evaluation; a reload drops the groups; after clear the engine ticks a small population on the one-wave path"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k != "CSF_PAIR_VARIANT"}
    r = subprocess.run([sys.executable, os.path.join(here, "scene_lane_groups_abi_child.py"), "abi"], capture_output=True, text=True, timeout=600,
                       env={**env, "PYTHONPATH": os.path.dirname(here) + os.pathsep + here})
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "scene lane groups abi ok" in r.stdout


# ---- 10: recovery ------------------------------------------------------------------------------------------------------------------------
def test_two_groups_f_0_are_recovered_on_a_roster_of_40():
    """TwoD, two groups with true f_0 of 1.0 x and 1.6 x the default on the roster of 40 of test 3 (windows_40: 12 lanes): the scene is
    recorded with the true sets on shared lanes, its leave-one-out scenes (ego_split: 39, rider 7 is never present) are fitted through
    InteractionCalibration(lane_groups=True) for (("f_0", 0), ("f_0", 1)) from a guess 20 % off; both values within 1e-3 relative."""
    from cyclistsocialforce_amd import calibration as cal, parameters, vehicle
    base = parameters.default_pod("twod")
    true = np.array([base.f_0, 1.6 * base.f_0])
    s0, off, dq = roster("twod", 40, seed=61)
    enter, exit = windows_40()
    grp = (np.arange(40) % 2).astype(np.uint8)
    truth = [(parameters.default_pod("twod", f_0=true[0]), parameters.default_pod("twod", f_0=true[1]))]
    e = loaded_groups(truth, [(s0, off, dq)], [greedy_lanes(enter, exit)], enter, exit, np.zeros((LANES_T, 40, 2)), grp, 2, feat=np.array([0, 1], dtype=np.int32))
    _, traj = e.scene_calib_eval_groups(truth, states=True)
    e.close()
    data = cal.SceneData(s0, VDES, off, dq, traj[:, :, :4], group=grp, present=(enter, exit)).ego_split()
    assert len(data) == 39
    c = cal.InteractionCalibration(vehicle.TwoDBicycle, [("f_0", 0), ("f_0", 1)], data, data, [1, 1, 0, 0, 0, 0], group_params=[{}, {}],
                                   max_sets=8, maxiter=400, xtol=1e-4, ftol=1e-30, lane_groups=True)
    guess = true * np.array([1.2, 0.8])
    f_start = float(c.evaluate([guess])[0])
    res = c.run(guess)
    rel = np.abs(res[0] - true) / true
    print(f"recovered f_0 = {res[0]} (true {true}): relative {rel}, objective {res[1]:.3e} from {f_start:.3e}, {res[2]} iterations")
    c.close()
    assert rel.max() < 1e-3
