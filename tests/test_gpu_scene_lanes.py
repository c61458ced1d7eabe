"""Rosters that share the lanes of the one-wave tick in a closed-loop calibration: csf_scene_calib_load_shared
against the load without shared lanes, against the engine's own population path and against NumPy on the call's own trajectories."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from scene_calib_common import MODELS, VDES, twin_scene
from scene_lanes_common import (CROWDS, FEAT, LANES_T, TWIN_TOL, check_sums, extent, greedy_lanes, inside, loaded_plain, loaded_shared, peak, roster,
                                sets3, sums_over_windows, window_twin, windows_40, windows_48)
from scene_windows_common import mixed_windows, one_scene

pytestmark = [pytest.mark.gpu, pytest.mark.auto_variant]


@pytest.mark.parametrize("model", MODELS)
def test_one_rider_per_lane_is_the_launch_with_windows(model):
    """The 7-rider mixed-window scene of 4.10d with lane[r] = r and 7 lanes against csf_scene_calib_load + csf_scene_calib_windows: the
    same P, the same source groups, so any difference is the takeover.  Sums array_equal; states array_equal inside the windows and
    NaN outside."""
    ticks, sets = LANES_T, sets3(model)
    part = one_scene(model, 7, seed=41)
    (enter, exit), _ = mixed_windows()
    here = inside(enter, exit, ticks)
    obj = np.random.default_rng(4).normal(size=(ticks, 7, len(FEAT)))
    obj[~here] = np.nan
    e = loaded_plain(sets, [part], obj, enter=enter, exit=exit)
    want, want_st = e.scene_calib_eval(sets, states=True)
    e.close()
    e = loaded_shared(sets, [part], [(np.arange(7, dtype=np.int32), 7)], enter, exit, obj)
    got, got_st = e.scene_calib_eval(sets, states=True)
    assert e.scene_calib_launches() == 1
    e.close()
    assert np.isfinite(want).all() and np.array_equal(got, want)
    for k in range(len(sets)):
        a, b = got_st[:, k * 7: (k + 1) * 7], want_st[:, k * 7: (k + 1) * 7]
        assert np.array_equal(a[here], b[here]), (k, float(np.abs(a[here] - b[here]).max()))
        assert np.isnan(a[~here]).all() and np.isfinite(a[here]).all()


@pytest.mark.parametrize("gap", [False, True])
@pytest.mark.parametrize("model", MODELS)
def test_a_relay_equals_two_scenes_without_windows(model, gap):
    """Roster 2 K, K = 3, T = 120: riders r < K on lane r over [0, 60), riders K + r on the same lane over [60, 120) (gap: exit 50, entry
    70), the late riders on the short route.  Against two scenes WITHOUT shared lanes and without windows in one launch - riders
    0 .. K - 1, and riders K .. 2 K - 1 with their objective rows shifted to tick 0 - on the same lanes with the same n.  Expected
    array_equal in states and sums; should it hold only at TWIN_TOL, that is asserted and the largest difference printed.  The
    destination pointers of the late riders equal the second scene's: a late occupant walks its own queue."""
    K, ticks, sets = 3, LANES_T, sets3(model)
    out, back = (50, 70) if gap else (60, 60)
    span = out                                                   # both halves have this many ticks
    first, late = roster(model, K, seed=51), roster(model, K, seed=52, short=True)
    enter = np.r_[np.zeros(K), np.full(K, back)].astype(np.int32)
    exit = np.r_[np.full(K, out), np.full(K, back + span)].astype(np.int32)
    assert back + span <= ticks
    obj = np.random.default_rng(7).normal(size=(ticks, 2 * K, len(FEAT)))
    lane = np.r_[np.arange(K), np.arange(K)].astype(np.int32)
    e = loaded_shared(sets, [(np.concatenate([first[0], late[0]]), np.r_[first[1], late[1][1:] + first[2].shape[0]], np.concatenate([first[2], late[2]]))],
                      [(lane, K)], enter, exit, obj)
    got, got_st = e.scene_calib_eval(sets, states=True)
    _, ptr, _, _ = e.state(with_nav=True)
    e.close()
    flat = obj.copy()
    flat[:span, K:] = obj[back: back + span, K:]
    e = loaded_plain(sets, [first, late], flat, lengths=np.array([span, span], dtype=np.int32))
    want, want_st = e.scene_calib_eval(sets, states=True)
    _, ptr_w, _, _ = e.state(with_nav=True)
    e.close()
    R = 2 * K
    worst = 0.0
    for k in range(len(sets)):
        a = np.concatenate([got_st[:span, k * R: k * R + K], got_st[back: back + span, k * R + K: (k + 1) * R]], axis=1)
        b = want_st[:span, k * R: (k + 1) * R]
        assert np.isfinite(a).all() and np.isfinite(b).all()
        worst = max(worst, float(np.abs(a - b).max()))
    here = inside(enter, exit, ticks)
    for k in range(len(sets)):
        assert np.array_equal(np.isnan(got_st[:, k * R: (k + 1) * R]).any(axis=2), ~here)
    same = worst == 0.0 and np.array_equal(got, want)
    print(f"{model} gap={gap}: largest |relay - two scenes| = {worst:.3e} ({'bit-identical' if same else 'NOT bit-identical'})")
    for k in range(len(sets)):
        a = np.concatenate([got_st[:span, k * R: k * R + K], got_st[back: back + span, k * R + K: (k + 1) * R]], axis=1)
        np.testing.assert_allclose(a, want_st[:span, k * R: (k + 1) * R], rtol=TWIN_TOL, atol=TWIN_TOL, err_msg=f"set {k}")
    np.testing.assert_allclose(got, want, rtol=TWIN_TOL, atol=0.0)
    assert np.all(got[:, :, 0] > 0.0)
    ptr, ptr_w = np.asarray(ptr)[: len(sets) * K].reshape(len(sets), K), np.asarray(ptr_w)[: len(sets) * R].reshape(len(sets), R)
    assert np.array_equal(ptr, ptr_w[:, K:]), (ptr, ptr_w)


@functools.lru_cache(maxsize=None)
def _crowds(model):
    """test 3's data set - a roster of 40 with at most 12 present and a roster of 48 on 32 lanes, T = 120, 3 sets - evaluated once;
    NaN in the objective outside every window"""
    ticks, sets = LANES_T, sets3(model)
    parts, wins, lanes = [], [], []
    for n, (win, seed) in CROWDS.items():
        parts.append(roster(model, n, seed=seed))
        wins.append(win())
        lanes.append(greedy_lanes(*wins[-1]))
    assert [l[1] for l in lanes] == [12, 32] == [peak(*w, ticks) for w in wins]
    enter, exit = np.concatenate([w[0] for w in wins]), np.concatenate([w[1] for w in wins])
    obj = np.random.default_rng(8).normal(size=(ticks, 88, len(FEAT)))
    obj[~inside(enter, exit, ticks)] = np.nan
    e = loaded_shared(sets, parts, lanes, enter, exit, obj)
    sums, states = e.scene_calib_eval(sets, states=True)
    again, states_again = e.scene_calib_eval(sets, states=True)
    _, tenth = e.scene_calib_eval(sets, states=True, stride=10)
    one, one_st = e.scene_calib_eval([sets[1]], states=True)
    launches = e.scene_calib_launches()
    e.close()
    return dict(sets=sets, parts=parts, enter=enter, exit=exit, obj=obj, R=88, roff=np.array([0, 40, 88]), sums=sums, states=states,
                again=(again, states_again), tenth=tenth, one=(one, one_st), launches=launches)


@pytest.mark.parametrize("model", MODELS)
def test_rosters_above_the_lanes_against_the_population_path(model):
    """40 riders with a peak of 12 and 48 riders on 32 lanes (P = 32: two source groups) against window_twin, which adds and removes
    riders between 1-tick steps, over the present cells.  The bar is 4.10d's for a twin that leaves the one-wave path and whose slot
    order differs: positions within 1e-4 x extent; a second twin whose starts are moved by 1e-7 m stays within 1e-5 x extent of the
    first (asserted: the horizon is not chaotic for these seeds)."""
    job = _crowds(model)
    ticks, R, roff, states = LANES_T, job["R"], job["roff"], job["states"]
    here_all = inside(job["enter"], job["exit"], ticks)
    assert job["launches"] == 4 and np.isfinite(job["sums"]).all()
    rng = np.random.default_rng(9)
    worst = chaos = 0.0
    for q, (s0, off, dq) in enumerate(job["parts"]):
        enter, exit = job["enter"][roff[q]: roff[q + 1]], job["exit"][roff[q]: roff[q + 1]]
        here = here_all[:, roff[q]: roff[q + 1]]
        s1 = s0.copy()
        s1[:, :2] += 1e-7 * rng.choice([-1.0, 1.0], size=(s0.shape[0], 2))
        for k, pod in enumerate(job["sets"]):
            got = states[:, k * R + roff[q]: k * R + roff[q + 1]]
            assert np.array_equal(np.isnan(got).any(axis=2), ~here) and np.array_equal(np.isnan(got).all(axis=2), ~here)
            tw, small, _ = window_twin(pod, s0, off, dq, enter, exit, ticks)
            assert np.array_equal(np.isfinite(tw).all(axis=2), here)
            ext = extent(tw)
            dev = float(np.hypot(got[here][:, 0] - tw[here][:, 0], got[here][:, 1] - tw[here][:, 1]).max())
            per, _, _ = window_twin(pod, s1, off, dq, enter, exit, ticks)
            sens = float(np.hypot(per[here][:, 0] - tw[here][:, 0], per[here][:, 1] - tw[here][:, 1]).max())
            print(f"{model} roster {s0.shape[0]} set {k}: |launch - twin| = {dev:.3e} m = {dev / ext:.2e} x extent; twin moved by 1e-7 m: "
                  f"{sens / ext:.2e} x extent; one-wave ticks of the twin {int(small.sum())} of {ticks}")
            worst, chaos = max(worst, dev / ext), max(chaos, sens / ext)
            assert sens < 1e-5 * ext, (q, k, sens / ext)
            assert dev < 1e-4 * ext, (q, k, dev / ext)
    print(f"{model}: largest deviation {worst:.2e} x extent, largest sensitivity to 1e-7 m {chaos:.2e} x extent")


@pytest.mark.parametrize("model", MODELS)
def test_sums_and_samples_of_a_shared_data_set(model):
    """From test 3's evaluation: the sums against NumPy on the call's own states over the present cells (relative 2 m 2^-53), exactly
    (0, 0) for the rider that is never present; a stride-10 call is every tenth row of the stride-1 call; the same call twice and a
    single-set call are array_equal."""
    job = _crowds(model)
    K, R = len(job["sets"]), job["R"]
    ref = sums_over_windows(job["states"], job["obj"], FEAT, job["enter"], job["exit"], K)
    w = check_sums(job["sums"], ref, job["enter"], job["exit"], len(FEAT))
    print(f"{model}: sums over the windows at {w:.3f} of the bound 2 m 2^-53")
    never = job["enter"] == job["exit"]
    assert never.sum() == 1 and np.all(job["sums"][:, never] == 0.0) and np.all(job["sums"][:, ~never, 0] > 0.0)
    assert np.isnan(job["states"][:, [k * R + 7 for k in range(K)]]).all()
    assert np.array_equal(job["again"][0], job["sums"]) and np.array_equal(job["again"][1], job["states"], equal_nan=True)
    assert job["tenth"].shape[0] == LANES_T // 10 and np.array_equal(job["tenth"], job["states"][9::10], equal_nan=True)
    assert np.array_equal(job["one"][0][0], job["sums"][1]) and np.array_equal(job["one"][1], job["states"][:, R: 2 * R], equal_nan=True)


@pytest.mark.parametrize("model", MODELS)
def test_replay_on_a_shared_lane(model):
    """5 riders on 4 lanes, T = 100: rider 3 is simulated over [0, 15) and the replayed rider 4 follows it on the same lane over
    [15, 70), its recording NaN outside that window.  Inside its window the replayed rider IS its recording; the simulated riders
    against a twin in which rider 3 is removed and rider 4 added before tick 15, pushed onto its recording after every tick and
    removed before tick 70, at TWIN_TOL."""
    from cyclistsocialforce_amd import calibration as cal
    ticks, a, b = 100, 15, 70
    sets = sets3(model)
    s0, off, dq = one_scene(model, 5, seed=44)
    rec = twin_scene(sets[1], s0, off, dq, ticks)[0]
    s0 = s0.copy()
    s0[4] = rec[a - 1, 4]
    rec = rec.copy()
    rec[:a, 4] = rec[b:, 4] = np.nan
    enter, exit = np.array([0, 0, 0, 0, a], dtype=np.int32), np.array([ticks, ticks, ticks, a, b], dtype=np.int32)
    mask = np.array([False, False, False, False, True])
    d = cal.SceneData(s0, VDES, off, dq, rec[:, :, :4], replayed=mask, present=(enter, exit))
    lane, nl = d.lanes()
    assert nl == 4 and lane[4] == lane[3] == 3
    e = loaded_shared(sets, [(s0, off, dq)], [(lane, nl)], enter, exit, np.random.default_rng(1).normal(size=(ticks, 5, len(FEAT))))
    e.scene_calib_replay(mask, d.replay_rows())
    sums, states = e.scene_calib_eval(sets, states=True)
    e.close()
    here = inside(enter, exit, ticks)
    assert np.all(sums[:, 4] == 0.0) and np.all(sums[:, :4, 0] > 0.0)
    for k, pod in enumerate(sets):
        tw, small, _ = window_twin(pod, s0, off, dq, enter, exit, ticks, replayed=mask, rec=rec)
        got = states[:, k * 5: (k + 1) * 5]
        assert np.array_equal(np.isnan(got).any(axis=2), ~here)
        assert np.array_equal(got[a:b, 4, :4], rec[a:b, 4, :4])
        sim = here.copy()
        sim[:, 4] = False
        worst = float(np.abs(got[sim] - tw[sim]).max())
        print(f"{model} set {k}: largest |launch - push_state twin| over the simulated riders: {worst:.3e}; one-wave ticks of the twin "
              f"{int(small.sum())} of {ticks}")
        np.testing.assert_allclose(got[sim], tw[sim], rtol=TWIN_TOL, atol=TWIN_TOL, err_msg=f"set {k}")


def test_interaction_calibration_on_a_roster_of_40():
    """InteractionCalibration (TwoD) on a 40-rider SceneData: `evaluate` is the formula on the engine's own sums for both built-in
    errors, `simulate` has NaN exactly outside the windows; share_lanes=True on a roster of 20 with at most 6 present agrees with
    share_lanes=False within 1e-4 x extent (other lanes, another order of the pair sums: printed, no bits expected)."""
    from cyclistsocialforce_amd import calibration as cal, vehicle
    ticks = LANES_T
    rng = np.random.default_rng(10)
    s0, off, dq = roster("twod", 40, seed=61)
    enter, exit = windows_40()
    here = inside(enter, exit, ticks)
    traj = rng.normal(size=(ticks, 40, 4))
    traj[~here] = np.nan
    data = [cal.SceneData(s0, VDES, off, dq, traj, present=(enter, exit))]
    theta = np.array([[9.0, 0.9], [6.0, 0.7]])
    feat_ind = [1, 0, 1, 0, 0, 0]
    cells = int(here.sum())
    for func in (cal.calc_sse_timesteps, cal.calc_maesse_samples):
        c = cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0", "sigma_0"], data, data, feat_ind, error_func=func, max_sets=4)
        err = c.evaluate(theta)
        raw = c._dataset()["engine"].scene_calib_eval([c._pod(c._update_params_args_dict(v)) for v in theta])
        trajs, objectives = c.simulate(theta[0])
        c.close()
        for k in range(2):
            acc = [0.0, 0.0]
            for r in range(40):
                acc[0] += raw[k, r, 0]
                acc[1] += raw[k, r, 1]
            want = acc[0] if func is cal.calc_sse_timesteps else (acc[1] / (cells * 2.0)) ** 2
            assert err[k] == want and np.isfinite(want) and want > 0.0, (func.__name__, k, err[k], want)
        assert trajs[0].shape == objectives[0].shape == (ticks, 40, 2)
        assert np.array_equal(np.isnan(trajs[0]), np.repeat(~here[:, :, None], 2, axis=2))
        assert np.array_equal(np.isnan(objectives[0]), np.repeat(~here[:, :, None], 2, axis=2))
    # a roster of 20, 6 at once: packed onto 6 lanes or not
    s0, off, dq = roster("twod", 20, seed=63)
    enter = (5 * np.arange(20)).astype(np.int32)
    exit = np.minimum(enter + 30, ticks).astype(np.int32)
    here = inside(enter, exit, ticks)
    traj = rng.normal(size=(ticks, 20, 4))
    traj[~here] = np.nan
    d = cal.SceneData(s0, VDES, off, dq, traj, present=(enter, exit))
    assert d.lanes()[1] == 6
    out = {}
    for share in (False, True):
        c = cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0", "sigma_0"], [d], [d], [1, 1, 0, 0, 0, 0], max_sets=2, share_lanes=share)
        out[share] = (c.simulate(theta[0])[0][0], c.evaluate(theta))
        c.close()
    a, b = out[False][0], out[True][0]
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isnan(a[..., 0]), ~here)
    ext = extent(a)
    dev = float(np.hypot(a[here][:, 0] - b[here][:, 0], a[here][:, 1] - b[here][:, 1]).max())
    print(f"roster 20 on 6 lanes against 20 slots: {dev:.3e} m = {dev / ext:.2e} x extent; errors {out[False][1]} / {out[True][1]}")
    assert dev < 1e-4 * ext


def test_refusals_and_lifetime_in_a_fresh_process():
    """every refusal of csf_scene_calib_load_shared comes back with its code and a message and leaves the engine empty and usable;
    csf_scene_calib_windows is refused on a shared data set; replay, road and eval in two orders are array_equal; after clear the
    engine ticks a small population on the one-wave path"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k != "CSF_PAIR_VARIANT"}
    r = subprocess.run([sys.executable, os.path.join(here, "scene_lanes_abi_child.py"), "abi"], capture_output=True, text=True, timeout=600,
                       env={**env, "PYTHONPATH": os.path.dirname(here) + os.pathsep + here})
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "scene lanes abi ok" in r.stdout
