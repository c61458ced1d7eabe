"""Calibration on closed-loop scenes: csf_scene_calib_load / csf_scene_calib_eval against the existing one-wave
path, NumPy on the call's own trajectories, the oracle, and the optimiser on top of it."""
import os
import subprocess
import sys

import numpy as np
import pytest

from scene_calib_common import (LENGTHS, MODELS, N_RIDERS, ORACLE_CASES, ORACLE_TICKS, SHORT, T, VDES, crowd, field_sets, oracle_case, oracle_run,
                                scenes, twin_scene)

pytestmark = [pytest.mark.gpu, pytest.mark.auto_variant]

FEAT = np.array([0, 2, 4, 5], dtype=np.int32)   # x, psi, delta, theta: rows 4 / 5 lie beyond n_states of some classes


def _sums_reference(states, obj, feat, lengths, roff, n_sets):
    """(sum d^2, sum |d|) per (set, rider) from the trajectories, in extended precision; d itself is the fp64 difference"""
    R, ns = obj.shape[1], states.shape[2]
    ref = np.zeros((n_sets, R, 2), dtype=np.longdouble)
    for k in range(n_sets):
        for q, ln in enumerate(lengths):
            for r in range(roff[q], roff[q + 1]):
                tr = np.zeros((ln, len(feat)))
                for c, f in enumerate(feat):
                    if f < ns:
                        tr[:, c] = states[:ln, k * R + r, f]
                d = (tr - obj[:ln, r, :]).astype(np.longdouble)
                ref[k, r, 0], ref[k, r, 1] = (d * d).sum(), np.abs(d).sum()
    return ref


def _check_sums(sums, ref, lengths, roff, n_feat):
    worst = 0.0
    for q, ln in enumerate(lengths):
        m = int(ln) * n_feat                    # accumulated terms, all non-negative: relative 2 m 2^-53 (the 2: fused multiply-adds)
        sl = slice(roff[q], roff[q + 1])
        for c in range(2):
            err = np.abs(sums[:, sl, c].astype(np.longdouble) - ref[:, sl, c])
            bound = 2.0 * m * 2.0 ** -53 * ref[:, sl, c]
            if m:
                worst = max(worst, float((err / np.maximum(ref[:, sl, c], np.longdouble(1e-300))).max()) / (2.0 * m * 2.0 ** -53))
            assert np.all(err <= bound), (q, c, err, bound)
    return worst


@pytest.mark.parametrize("model", MODELS)
def test_scenes_equal_the_one_wave_path_sums_equal_numpy_and_calls_are_independent(model):
    """5 scenes of 1, 2, 5, 17 and 32 riders (lengths T, 0, T - 37, T, 60) from crowd() and a sixth of 4 riders with a short route
    (length T) x 7 parameter sets in one launch.  The states at stride 1 and 10 against twin engines, each created with one set and
    stepping one scene alone through csf_step with csf_record (2e-7, the bar of test_gpu_calib.py against its twin); the per-rider
    sums against NumPy on the same call's states (relative 2 m 2^-53); and an evaluation depends neither on the one before, nor on
    the place of a set in the call, nor on the other sets.
    Within T ticks the destination pointers advance and the navigation state changes, both asserted on the twins and on the loaded
    engine.  crowd()'s only stop lies 61 m ahead and T = 200 ticks cover 10 m, so its riders pass their start row and the
    destination 8 m ahead and stay in the cruise state; the sixth scene (scene_calib_common.SHORT) is what leaves it: with every
    one of the 7 sets its riders reach the last leg of the route - where twod_dest reads row 0 of the position ring - and brake,
    and T > hist_len = 128, so the ring has wrapped over row 0 before the repeated calls below start from the image again."""
    from cyclistsocialforce_amd.engine import Engine
    sets = field_sets(model)
    s0, off, rows, per = scenes(model, seed=MODELS.index(model), short=(SHORT,))
    R, K = s0.shape[0], len(sets)
    roff = np.r_[0, np.cumsum(N_RIDERS)]
    obj = np.random.default_rng(1).normal(size=(T, R, len(FEAT)))
    e = Engine(sets[0], K * R)
    e.scene_calib_load(N_RIDERS, s0, VDES, off, rows, obj, FEAT, lengths=LENGTHS, max_sets=K)
    assert e.scene_calib_launches() == 0
    sums, states = e.scene_calib_eval(sets, states=True, stride=1)
    sums10, states10 = e.scene_calib_eval(sets, states=True, stride=10)
    assert e.scene_calib_launches() == 2
    assert states.shape == (T, K * R, e.ns) and states10.shape == (T // 10, K * R, e.ns) and sums.shape == (K, R, 2)
    assert np.isfinite(states).all() and np.isfinite(sums).all()
    assert np.array_equal(states10, states[9::10])
    # the twins
    worst, moved, arrived = 0.0, False, 0
    last_row = int(off[roff[SHORT] + 1] - off[roff[SHORT]]) - 1
    for k, pod in enumerate(sets):
        for q, (sq, oq, dq) in enumerate(per):
            ln = int(LENGTHS[q])
            if ln == 0:
                continue
            tw, ptr, zn = twin_scene(pod, sq, oq, dq, ln)
            got = states[:ln, k * R + roff[q]: k * R + roff[q + 1]]
            diff = float(np.abs(got - tw).max())
            worst = max(worst, diff)
            np.testing.assert_allclose(got, tw, rtol=2e-7, atol=2e-7, err_msg=f"set {k} scene {q}")
            moved = moved or bool((ptr >= 2).any())              # (row 0 is the start itself: 2 = the destination 8 m ahead is behind)
            if q == SHORT:
                assert (ptr == last_row).any(), f"set {k}: no rider of the short scene reached the last leg of its route"
                assert (zn[:, 0] == 0).any(), f"set {k}: no rider of the short scene left the cruise state"
                arrived += int((zn[:, 2] != 0).sum())
    print(f"{model}: largest |scene_calib_eval - csf_step twin| = {worst:.3e} ({'bit-identical' if worst == 0.0 else 'not bit-identical'})")
    assert moved, "no destination pointer advanced within T ticks"
    print(f"{model}: riders of the short scene that arrived at their stop within T ticks, over the 7 sets: {arrived} of {K * N_RIDERS[SHORT]}")
    assert not np.array_equal(states[:, :R], states[:, R: 2 * R])                 # the sets do differ
    # the read-backs of the loaded engine show the end of the last evaluation: pointers and navigation state moved there too
    _, ptr_e, zn_e, _ = e.state(with_nav=True)
    ptr_e, zn_e = np.asarray(ptr_e).reshape(K, R), np.asarray(zn_e).reshape(K, R, 3)
    assert (ptr_e >= 2).any()
    for k in range(K):
        sl = slice(roff[SHORT], roff[SHORT + 1])
        assert (ptr_e[k, sl] == last_row).any() and (zn_e[k, sl, 0] == 0).any(), k
    # an empty scene keeps its start state, an ended one its last
    q0 = int(np.flatnonzero(LENGTHS == 0)[0])
    for r in range(roff[q0], roff[q0 + 1]):
        assert np.array_equal(states[:, r], np.tile(states[0, r], (T, 1)))
        np.testing.assert_allclose(states[0, r, : s0.shape[1]], s0[r], rtol=0, atol=1e-14)   # (the yaw has been through limitAngle)
    q1 = 4
    for r in range(roff[q1], roff[q1 + 1]):
        assert np.array_equal(states[LENGTHS[q1]:, r], np.tile(states[LENGTHS[q1] - 1, r], (T - LENGTHS[q1], 1)))
    # the sums, per rider
    ref = _sums_reference(states, obj, FEAT, LENGTHS, roff, K)
    w = _check_sums(sums, ref, LENGTHS, roff, len(FEAT))
    print(f"{model}: sums at {w:.3f} of the bound 2 m 2^-53")
    assert np.all(sums[:, roff[q0]: roff[q0 + 1]] == 0.0)
    # independence
    assert np.array_equal(sums10, sums)
    assert np.array_equal(e.scene_calib_eval(sets), sums)                         # with and without states_out
    again, st_again = e.scene_calib_eval(sets, states=True)
    assert np.array_equal(again, sums) and np.array_equal(st_again, states)       # the same call twice
    perm = np.array([4, 0, 6, 2, 5, 1, 3])
    sp, stp = e.scene_calib_eval([sets[i] for i in perm], states=True)
    assert np.array_equal(sp, sums[perm])
    assert np.array_equal(stp.reshape(T, K, R, -1), states.reshape(T, K, R, -1)[:, perm])
    one, st1 = e.scene_calib_eval([sets[3]], states=True)
    assert np.array_equal(one[0], sums[3]) and np.array_equal(st1, states[:, 3 * R: 4 * R])
    e.scene_calib_clear()
    assert e.n == 0
    e.close()


@pytest.mark.parametrize("model", ["twod", "invpend", "planarpoint", "bicycle"])
def test_scenes_against_the_oracle(model):
    """The scenes of test_small_crowds_vs_oracle with n <= 8 of this class, built as there (crowd(n, seed = 10 n + rule, box 14):
    seeds twod 80, 51, 20, 10; invpend 60; planarpoint 81, 30; bicycle 70), three sets - the default and the first two of the
    `field` list of tests/test_gpu_hetero.py - in one launch per scene; orc.Population runs free for 200 ticks, positions at stride
    10 within 1e-4 x extent.  The oracle alone is not chaotic on that horizon for any (scene, set) used:
    tests/test_scene_calib_host.py::test_the_oracle_is_not_chaotic_on_the_horizon starts it from positions perturbed by 1e-7 m
    (three random sign patterns) and asserts 1e-5 x extent; measured, the largest deviation of the 24 cases was 2.7e-8 x extent
    (planarpoint, 3 riders, the second set), i.e. the perturbation grows by less than 4 in 200 ticks - no other seed was needed."""
    from cyclistsocialforce_amd.engine import Engine
    for m, n, rule, hfov in ORACLE_CASES:
        if m != model:
            continue
        s0, off, dq, pods = oracle_case(m, n, rule, hfov)
        e = Engine(pods[0], len(pods) * n)
        e.scene_calib_load([n], s0, 5.0, off, dq, np.zeros((ORACLE_TICKS, n, 1)), [0], max_sets=len(pods))
        _, states = e.scene_calib_eval(pods, states=True, stride=10)
        e.close()
        for k, pod in enumerate(pods):
            ref = oracle_run(pod, s0, off, dq)
            ext = max(np.ptp(ref[..., 0]), np.ptp(ref[..., 1]), 14.0)
            got = states[:, k * n: (k + 1) * n, :2]
            worst = float(np.hypot(got[..., 0] - ref[..., 0], got[..., 1] - ref[..., 1]).max())
            print(f"{m} n={n} rule={rule} hfov={hfov} set {k}: largest position deviation {worst:.3e} m = {worst / ext:.2e} x extent")
            assert worst < 1e-4 * ext, (m, n, rule, hfov, k)


def test_launches_per_call_do_not_grow():
    from cyclistsocialforce_amd.engine import Engine
    counts = []
    for ticks, n_sets, riders in ((50, 2, [3, 4]), (200, 7, [1, 2, 5, 17, 32])):
        sets = field_sets("twod", n_sets)
        s0, off, rows, _ = scenes("twod", np.array(riders), seed=5)
        R = s0.shape[0]
        e = Engine(sets[0], n_sets * R)
        e.scene_calib_load(riders, s0, VDES, off, rows, np.zeros((ticks, R, 1)), [0], max_sets=n_sets)
        assert e.scene_calib_launches() == 0
        a = e.scene_calib_eval(sets)
        assert e.scene_calib_launches() == 1
        b, _ = e.scene_calib_eval(sets, states=True, stride=3)
        counts.append(e.scene_calib_launches())
        assert np.array_equal(a, b)
        e.close()
    assert counts == [2, 2]


def _recovery_data(star):
    """4 scenes of 3 - 6 TwoD riders over 150 ticks whose recorded trajectories the engine itself produced at theta* = (f_0, sigma_0)"""
    from cyclistsocialforce_amd import calibration as cal, parameters
    from cyclistsocialforce_amd.engine import Engine
    data = []
    for q, n in enumerate((3, 4, 5, 6)):
        x, y, psi, v, off, dq = crowd(n, seed=300 + q, box=10.0)
        s0 = np.c_[x, y, psi, v, np.zeros(n)]
        pod = parameters.default_pod("twod", f_0=star[0], sigma_0=star[1])
        e = Engine(pod, n)
        e.scene_calib_load([n], s0, 5.0, off, dq, np.zeros((150, n, 1)), [0], max_sets=1)
        _, st = e.scene_calib_eval([pod], states=True)
        e.close()
        data.append(cal.SceneData(s0, 5.0, off, dq, st))
    return data


def test_recovery_of_two_field_parameters():
    """The objective is generated by the engine itself at theta* = (f_0, sigma_0) = (9, 0.9), not the defaults.  From two guesses,
    `run` (scipy.optimize.fmin) and run_many agree bit for bit on the shared guess, and both return theta within the optimiser's
    xtol of theta*; the iterations are printed."""
    from cyclistsocialforce_amd import calibration as cal, vehicle
    star = np.array([9.0, 0.9])
    data = _recovery_data(star)
    xtol = 1e-4
    c = cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0", "sigma_0"], data, data, [1, 1, 0, 0, 0, 0], max_sets=8, maxiter=400,
                                   xtol=xtol, ftol=1e-30)
    f_star = c.evaluate([star])[0]
    guesses = [star * [1.25, 0.85], star * [0.8, 1.2]]
    f_start = c.evaluate(guesses)
    res = c.run(guesses[0])
    many = c.run_many(guesses)
    print("recovery: run", res[0], res[1], "iterations", res[2], "| run_many", [(x, f, it) for x, f, it in many], "| f(theta*)", f_star, "f(guesses)", f_start)
    x, f, it = many[0]
    assert np.array_equal(x, res[0]) and f == res[1] and it == res[2]
    assert f_star == 0.0
    for (x, f, it), f0 in zip(many, f_start):
        assert np.abs(x - star).max() <= xtol, (x, star)
        assert f < 1e-6 * f0
    c.close()


def _child(mode, extra_env=None):
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k != "CSF_PAIR_VARIANT"}
    env.update(extra_env or {})
    r = subprocess.run([sys.executable, os.path.join(here, "scene_calib_abi_child.py"), mode], capture_output=True, text=True, timeout=600,
                       env={**env, "PYTHONPATH": os.path.dirname(here) + os.pathsep + here})
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert f"scene calib {mode} ok" in r.stdout


def test_refusals_and_lifetime_in_a_fresh_process():
    """every refusal of csf_scene_calib_load / csf_scene_calib_eval comes back with its code and a message and changes nothing; the
    calls a loaded engine refuses; after clear the engine is empty and steps again"""
    _child("abi")


def test_the_rate_tool_runs_both_legs_on_the_same_job(tmp_path):
    """tools/scene_calib_rate.py on a tiny cell: both legs run (the baseline through push_state, set_dest_pointer, step_batch with
    csf_record and batch_recorded), a line per cell is written, and on the first call - fresh engines - the baseline's error is
    the new path's.  Bound: trajectories that agree to 2e-7 (1 + |x|) with |x| <= 20 m move a sum of d^2 by at most 2 delta / rms(d)
    relative, and rms(d) >= 1 against the unit-normal objective: 2 x 4.2e-6 < 1e-5."""
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "rate.jsonl"
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "scene_calib_rate.py"), "--sets", "1,3", "--scenes", "3", "--ticks", "40", "--windows", "2",
                        "--models", "twod", "--out", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [json.loads(x) for x in out.read_text().splitlines()]
    assert [x["n_sets"] for x in lines] == [1, 3]
    for x in lines:
        assert x["base_ms"] is not None and x["new_ms"]["min"] > 0 and x["base_ms"]["min"] > 0
        assert x["first_call_rel_gap"] < 1e-5, x
