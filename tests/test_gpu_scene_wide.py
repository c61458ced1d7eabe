"""Scenes with more than 32 road users at once in a closed-loop calibration: csf_scene_calib_load_wide - one workgroup
of 256 threads per (candidate set, scene) - against the one-wave kernel on scenes both can run, against the engine's own population
path, and against NumPy on the call's own trajectories."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from scene_calib_common import MODELS, VDES
from scene_lanes_common import (FEAT, LANES_T, TWIN_TOL, check_sums, extent, greedy_lanes, inside, loaded_shared, peak, roster, sets3,
                                sums_over_windows, window_twin, windows_40, windows_48)
from scene_wide_common import always, edge_below, loaded_wide, pop_twin, wide_crowd, windows_80
from scene_windows_common import mixed_windows, one_scene

pytestmark = [pytest.mark.gpu, pytest.mark.auto_variant]


def _dist(a, b):
    return np.hypot(a[..., 0] - b[..., 0], a[..., 1] - b[..., 1])


# ---- 1: both kernels on scenes both can run ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_both_kernels_on_narrow_scenes(model):
    """The 7-rider mixed-window scene of 4.10d on 7 lanes and the roster of 48 on 32 lanes, one data set, loaded by
    csf_scene_calib_load_wide(wide_from = 1) - P = 64, four source groups - and by csf_scene_calib_load_shared - P = 8 and 32.  Only the
    order of the fp64 sums of the pair term differs: states inside the windows and sums at TWIN_TOL, the NaN pattern identical.  The
    largest difference is printed."""
    ticks, sets = LANES_T, sets3(model)
    parts = [one_scene(model, 7, seed=41), roster(model, 48, seed=62)]
    wins = [mixed_windows()[0], windows_48()]
    lanes = [(np.arange(7, dtype=np.int32), 7), greedy_lanes(*wins[1])]
    assert lanes[1][1] == 32
    enter, exit = np.concatenate([w[0] for w in wins]), np.concatenate([w[1] for w in wins])
    here = inside(enter, exit, ticks)
    R = 55
    obj = np.random.default_rng(4).normal(size=(ticks, R, len(FEAT)))
    obj[~here] = np.nan
    e = loaded_shared(sets, parts, lanes, enter, exit, obj)
    want, want_st = e.scene_calib_eval(sets, states=True)
    assert e.scene_calib_launches() == 1
    e.close()
    e = loaded_wide(sets, parts, lanes, enter, exit, obj, wide_from=1)
    got, got_st = e.scene_calib_eval(sets, states=True)
    assert e.scene_calib_launches() == 1                         # (every scene is wide: one kernel)
    e.close()
    assert np.isfinite(want).all() and np.isfinite(got).all()
    worst = 0.0
    for k in range(len(sets)):
        a, b = got_st[:, k * R: (k + 1) * R], want_st[:, k * R: (k + 1) * R]
        assert np.array_equal(np.isnan(a), np.isnan(b))
        assert np.isnan(a[~here]).all() and np.isfinite(a[here]).all()
        worst = max(worst, float(np.abs(a[here] - b[here]).max()))
    some = want != 0.0
    assert np.array_equal(got != 0.0, some)                      # (the rider that is never present: (0, 0) from both)
    rel = float(np.abs(got[some] / want[some] - 1.0).max())
    print(f"{model}: largest |wide - one-wave| over the states {worst:.3e}, over the sums (relative) {rel:.3e}")
    for k in range(len(sets)):
        a, b = got_st[:, k * R: (k + 1) * R], want_st[:, k * R: (k + 1) * R]
        np.testing.assert_allclose(a[here], b[here], rtol=TWIN_TOL, atol=TWIN_TOL, err_msg=f"set {k}")
    np.testing.assert_allclose(got, want, rtol=TWIN_TOL, atol=0.0)


# ---- 2, 3: wide scenes against the population path; determinism ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wide(model, n):
    """one wide scene of n road users without windows, T = 120, 3 sets, evaluated once (n = 65: and again, permuted, alone, sampled)"""
    ticks, sets = LANES_T, sets3(model)
    part = wide_crowd(model, n)
    lanes, enter, exit = always(n)
    obj = np.random.default_rng(8).normal(size=(ticks, n, len(FEAT)))
    e = loaded_wide(sets, [part], [lanes], enter, exit, obj)
    sums, states = e.scene_calib_eval(sets, states=True)
    job = dict(sets=sets, part=part, enter=enter, exit=exit, obj=obj, sums=sums, states=states, launches=[e.scene_calib_launches()])
    if n == 65:
        job["again"] = e.scene_calib_eval(sets, states=True)
        perm = [2, 0, 1]
        job["perm"] = (perm, e.scene_calib_eval([sets[i] for i in perm], states=True))
        job["one"] = e.scene_calib_eval([sets[1]], states=True)
        job["tenth"] = e.scene_calib_eval(sets, states=True, stride=10)[1]
        job["launches"].append(e.scene_calib_launches())
    e.close()
    return job


WIDE_CASES = [(m, n) for n in (33, 65) for m in MODELS] + [("twod", 130), ("invpend", 130)]


@pytest.mark.parametrize("model,n", WIDE_CASES)
def test_wide_scenes_against_the_population_path(model, n):
    """n = 33 (P = 64, G = 4, the owners in wave 0), 65 (P = 128, G = 2, the owners cross a wave boundary) and 130 (P = 256, G = 1, three
    owning waves) against a stand-alone engine of every set stepped T ticks on its own path, at the bar of
    test_rosters_above_the_lanes_against_the_population_path: positions within 1e-4 x extent, and a second twin whose starts are moved
    by 1e-7 m stays within 1e-5 x extent of the first (asserted).  The sums against NumPy on the call's own states (2 m 2^-53)."""
    job = _wide(model, n)
    ticks, states = LANES_T, job["states"]
    s0, off, dq = job["part"]
    assert job["launches"][0] == 1 and np.isfinite(job["sums"]).all() and np.isfinite(states).all()
    s1 = s0.copy()
    s1[:, :2] += 1e-7 * np.random.default_rng(9).choice([-1.0, 1.0], size=(n, 2))
    worst = chaos = 0.0
    for k, pod in enumerate(job["sets"]):
        got = states[:, k * n: (k + 1) * n]
        tw = pop_twin(pod, s0, off, dq, ticks)
        ext = extent(tw)
        dev = float(_dist(got, tw).max())
        sens = float(_dist(pop_twin(pod, s1, off, dq, ticks), tw).max())
        print(f"{model} n = {n} set {k}: |launch - twin| = {dev:.3e} m = {dev / ext:.2e} x extent; twin moved by 1e-7 m: {sens / ext:.2e} x extent")
        worst, chaos = max(worst, dev / ext), max(chaos, sens / ext)
        assert sens < 1e-5 * ext, (k, sens / ext)
        assert dev < 1e-4 * ext, (k, dev / ext)
    ref = sums_over_windows(states, job["obj"], FEAT, job["enter"], job["exit"], len(job["sets"]))
    w = check_sums(job["sums"], ref, job["enter"], job["exit"], len(FEAT))
    print(f"{model} n = {n}: largest deviation {worst:.2e} x extent, sensitivity {chaos:.2e} x extent, sums at {w:.3f} of the bound 2 m 2^-53")
    assert np.all(job["sums"][:, :, 0] > 0.0)


@pytest.mark.parametrize("model", MODELS)
def test_a_wide_evaluation_is_deterministic(model):
    """on the n = 65 job: the same call twice, the sets permuted, a single set and stride-10 samples are array_equal to the first call;
    every evaluation of a data set of wide scenes alone is one launch"""
    job = _wide(model, 65)
    K, n = len(job["sets"]), 65
    sums, states = job["sums"], job["states"]
    assert np.array_equal(job["again"][0], sums) and np.array_equal(job["again"][1], states)
    perm, (ps, pst) = job["perm"]
    assert np.array_equal(ps, sums[perm])
    assert np.array_equal(pst.reshape(LANES_T, K, n, -1), states.reshape(LANES_T, K, n, -1)[:, perm])
    assert np.array_equal(job["one"][0][0], sums[1]) and np.array_equal(job["one"][1], states[:, n: 2 * n])
    assert job["tenth"].shape[0] == LANES_T // 10 and np.array_equal(job["tenth"], states[9::10])
    assert job["launches"] == [1, 5]


# ---- 4: a mixed data set ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_a_mixed_data_set_is_two_launches_and_leaves_the_narrow_scenes_alone(model):
    """Scenes of 7, 65 and 12 lanes (the 12 lanes carry a roster of 40), wide_from = 33: the 7- and the 12-lane scene run on
    scene_lanes_kernel and their sums and states are array_equal to a csf_scene_calib_load_shared of those two alone; one evaluation
    is two launches."""
    ticks, sets = LANES_T, sets3(model)
    K = len(sets)
    w7, w40 = mixed_windows()[0], windows_40()
    parts = [one_scene(model, 7, seed=41), wide_crowd(model, 65), roster(model, 40, seed=61)]
    l65, en65, ex65 = always(65)
    lanes = [(np.arange(7, dtype=np.int32), 7), l65, greedy_lanes(*w40)]
    assert [l[1] for l in lanes] == [7, 65, 12] and peak(*w40, ticks) == 12
    enter, exit = np.concatenate([w7[0], en65, w40[0]]), np.concatenate([w7[1], ex65, w40[1]])
    R = 112
    obj = np.random.default_rng(5).normal(size=(ticks, R, len(FEAT)))
    narrow = np.r_[np.arange(7), np.arange(72, 112)]
    e = loaded_wide(sets, parts, lanes, enter, exit, obj)
    got, got_st = e.scene_calib_eval(sets, states=True)
    assert e.scene_calib_launches() == 2
    e.close()
    e = loaded_shared(sets, [parts[0], parts[2]], [lanes[0], lanes[2]], enter[narrow], exit[narrow], np.ascontiguousarray(obj[:, narrow]))
    want, want_st = e.scene_calib_eval(sets, states=True)
    assert e.scene_calib_launches() == 1
    e.close()
    assert np.isfinite(got).all() and np.array_equal(got[:, narrow], want)
    a = got_st.reshape(ticks, K, R, -1)[:, :, narrow]
    b = want_st.reshape(ticks, K, 47, -1)
    assert np.array_equal(a, b, equal_nan=True)
    here = inside(enter, exit, ticks)
    assert np.array_equal(np.isnan(got_st.reshape(ticks, K, R, -1)).any(axis=3), np.repeat(~here[:, None, :], K, axis=1))
    assert np.all(got[:, 7:72, 0] > 0.0)


# ---- 5: windows and shared lanes, wide ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_a_roster_of_80_on_40_wide_lanes(model):
    """Rider r enters at tick r and stays 40 ticks, rider 7 never: 40 lanes of the wide kernel, chains of up to two riders.  Against
    window_twin over the present cells at the bar of test_wide_scenes_against_the_population_path (a second twin moved by 1e-7 m
    asserted within 1e-5 x extent); NaN exactly outside the windows; the rider that is never present has the sums (0, 0)."""
    ticks, sets = LANES_T, sets3(model)
    s0, off, dq = wide_crowd(model, 80)
    enter, exit = windows_80()
    lanes = greedy_lanes(enter, exit)
    assert lanes[1] == 40 == peak(enter, exit, ticks)
    here = inside(enter, exit, ticks)
    obj = np.random.default_rng(6).normal(size=(ticks, 80, len(FEAT)))
    obj[~here] = np.nan
    e = loaded_wide(sets, [(s0, off, dq)], [lanes], enter, exit, obj)
    sums, states = e.scene_calib_eval(sets, states=True)
    assert e.scene_calib_launches() == 1
    e.close()
    assert np.all(sums[:, 7] == 0.0) and np.all(sums[:, np.arange(80) != 7, 0] > 0.0) and np.isfinite(sums).all()
    ref = sums_over_windows(states, obj, FEAT, enter, exit, len(sets))
    check_sums(sums, ref, enter, exit, len(FEAT))
    s1 = s0.copy()
    s1[:, :2] += 1e-7 * np.random.default_rng(9).choice([-1.0, 1.0], size=(80, 2))
    for k, pod in enumerate(sets):
        got = states[:, k * 80: (k + 1) * 80]
        assert np.array_equal(np.isnan(got).any(axis=2), ~here) and np.array_equal(np.isnan(got).all(axis=2), ~here)
        tw, _, _ = window_twin(pod, s0, off, dq, enter, exit, ticks)
        assert np.array_equal(np.isfinite(tw).all(axis=2), here)
        ext = extent(tw)
        dev = float(_dist(got[here], tw[here]).max())
        per, _, _ = window_twin(pod, s1, off, dq, enter, exit, ticks)
        sens = float(_dist(per[here], tw[here]).max())
        print(f"{model} roster 80 set {k}: |launch - twin| = {dev:.3e} m = {dev / ext:.2e} x extent; twin moved by 1e-7 m: {sens / ext:.2e} x extent")
        assert sens < 1e-5 * ext, (k, sens / ext)
        assert dev < 1e-4 * ext, (k, dev / ext)


# ---- 6: replay ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_replay_on_a_wide_scene(model):
    """The n = 65 scene with every odd rider replayed from a twin's recording: the replayed riders' sampled (x, y, psi, v) ARE the
    recording and their sums (0, 0); the simulated riders against window_twin(replayed=, rec=) - push_state after every tick - at the
    bar of test_wide_scenes_against_the_population_path."""
    ticks, sets, n = LANES_T, sets3(model), 65
    s0, off, dq = wide_crowd(model, n)
    rec = pop_twin(sets[1], s0, off, dq, ticks)
    mask = np.arange(n) % 2 == 1
    lanes, enter, exit = always(n)
    e = loaded_wide(sets, [(s0, off, dq)], [lanes], enter, exit, np.random.default_rng(1).normal(size=(ticks, n, len(FEAT))))
    e.scene_calib_replay(mask, np.ascontiguousarray(rec[:, mask, :4]))
    sums, states = e.scene_calib_eval(sets, states=True)
    e.close()
    assert np.all(sums[:, mask] == 0.0) and np.all(sums[:, ~mask, 0] > 0.0) and np.isfinite(states).all()
    for k, pod in enumerate(sets):
        got = states[:, k * n: (k + 1) * n]
        assert np.array_equal(got[:, mask, :4], rec[:, mask, :4])
        tw, _, _ = window_twin(pod, s0, off, dq, enter, exit, ticks, replayed=mask, rec=rec)
        ext = extent(tw)
        dev = float(_dist(got[:, ~mask], tw[:, ~mask]).max())
        print(f"{model} set {k}: largest |launch - push_state twin| over the simulated riders: {dev:.3e} m = {dev / ext:.2e} x extent")
        assert dev < 1e-4 * ext, (k, dev / ext)


# ---- 7: road --------------------------------------------------------------------------------------------------------------------------
def _road_call(edge):
    off, verts, f0, sg = edge
    return np.zeros(off.size - 1, dtype=np.int32), off, verts, f0, sg


@pytest.mark.parametrize("model", ["twod", "bicycle"])
def test_a_road_on_a_wide_scene(model):
    """The n = 33 scene with one edge of 100 vertices (padded 128, P = 64: 256 allowed) against a stand-alone engine with set_road, at
    the bar of test_wide_scenes_against_the_population_path; road_F0 / road_sigma for two sets give what two loads with those road
    parameters give, array_equal; a road of 257 vertices is refused."""
    from cyclistsocialforce_amd.engine import EngineError
    ticks, sets, n = LANES_T, sets3(model), 33
    s0, off, dq = wide_crowd(model, n)
    lanes, enter, exit = always(n)
    obj = np.random.default_rng(2).normal(size=(ticks, n, len(FEAT)))
    edge = edge_below(model, n)
    e = loaded_wide(sets, [(s0, off, dq)], [lanes], enter, exit, obj)
    bare, _ = e.scene_calib_eval(sets, states=True)
    e.scene_calib_road(*_road_call(edge))
    sums, states = e.scene_calib_eval(sets, states=True)
    assert np.isfinite(sums).all() and not np.array_equal(sums, bare)
    for k, pod in enumerate(sets):
        got = states[:, k * n: (k + 1) * n]
        tw = pop_twin(pod, s0, off, dq, ticks, road=edge)
        ext = extent(tw)
        dev = float(_dist(got, tw).max())
        print(f"{model} set {k}: |launch - twin with the road| = {dev:.3e} m = {dev / ext:.2e} x extent")
        assert dev < 1e-4 * ext, (k, dev / ext)
    over = ((4.0, 2.0), (7.5, 2.5))
    got, got_st = e.scene_calib_eval(sets[:2], states=True, road_F0=[o[0] for o in over], road_sigma=[o[1] for o in over])
    for count in (257, 300):
        with pytest.raises(EngineError):
            e.scene_calib_road(*_road_call(edge_below(model, n, count=count)))
    again, _ = e.scene_calib_eval(sets, states=True)             # (a refused road changes nothing)
    assert np.array_equal(again, sums)
    e.scene_calib_road(*_road_call(edge_below(model, n, count=256)))
    assert np.isfinite(e.scene_calib_eval(sets)).all()
    e.close()
    for k, (f0, sg) in enumerate(over):
        x = loaded_wide(sets, [(s0, off, dq)], [lanes], enter, exit, obj)
        x.scene_calib_road(*_road_call(edge_below(model, n, f0=f0, sigma=sg)))
        want, want_st = x.scene_calib_eval([sets[k]], states=True)
        x.close()
        assert np.array_equal(got[k], want[0]) and np.array_equal(got_st[:, k * n: (k + 1) * n], want_st)


# ---- 8: recovery ------------------------------------------------------------------------------------------------------------------------
def test_recovery_of_two_field_parameters_on_a_wide_scene():
    """InteractionCalibration on one wide scene, n = 40, T = 100, TwoD: the recorded trajectory is simulate() at theta* = (f_0, sigma_0)
    = the defaults x (1.2, 0.9).  From the defaults run_many reaches theta* within xtol = 1e-4 (iteration cap and ftol of
    tests/test_gpu_scene_calib.py::test_recovery_of_two_field_parameters); the error at theta* is exactly 0."""
    from cyclistsocialforce_amd import calibration as cal, parameters, vehicle
    n, ticks = 40, 100
    base = parameters.default_pod("twod")
    start = np.array([base.f_0, base.sigma_0])
    star = start * [1.2, 0.9]
    s0, off, dq = wide_crowd("twod", n)
    blank = cal.SceneData(s0, VDES, off, dq, np.zeros((ticks, n, 4)), wide=True)
    c = cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0", "sigma_0"], [blank], [blank], [1, 1, 1, 1, 0, 0], max_sets=1)
    traj = c.simulate(star)[0][0]
    c.close()
    assert traj.shape == (ticks, n, 4) and np.isfinite(traj).all()
    data = [cal.SceneData(s0, VDES, off, dq, traj, wide=True)]
    xtol = 1e-4
    c = cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0", "sigma_0"], data, data, [1, 1, 0, 0, 0, 0], max_sets=8, maxiter=400, xtol=xtol,
                                   ftol=1e-30)
    f_star, f_start = c.evaluate([star])[0], c.evaluate([start])[0]
    (x, f, it), = c.run_many([start])
    launches = c._dataset()["engine"].scene_calib_launches()
    c.close()
    print(f"recovery on 40 road users: theta* {star}, found {x} (|error| {np.abs(x - star).max():.3e}), f {f:.3e} from {f_start:.3e}, "
          f"{it} iterations, {launches} launches")
    assert f_star == 0.0 and f_start > 0.0
    assert np.abs(x - star).max() <= xtol, (x, star)


# ---- 9: the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_refusals_and_lifetime_in_a_fresh_process():
    """every refusal of csf_scene_calib_load_wide comes back with its code and a message and leaves the engine empty and usable; after a
    wide load csf_step and csf_scene_calib_windows are refused; after clear the engine ticks a small population on the one-wave path"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k != "CSF_PAIR_VARIANT"}
    r = subprocess.run([sys.executable, os.path.join(here, "scene_wide_abi_child.py"), "abi"], capture_output=True, text=True, timeout=600,
                       env={**env, "PYTHONPATH": os.path.dirname(here) + os.pathsep + here})
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "scene wide abi ok" in r.stdout
