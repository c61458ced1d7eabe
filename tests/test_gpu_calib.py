"""Calibration on the device: csf_calib_load / csf_calib_eval against the existing replay path, the golden run,
NumPy on the call's own trajectories, and the optimiser on top of it."""
import os
import subprocess
import sys

import numpy as np
import pytest

from calib_common import LENGTHS, MODELS, T, data_set, pod_sets, twin_states

pytestmark = [pytest.mark.gpu, pytest.mark.auto_variant]

FEAT = np.array([0, 2, 4, 5], dtype=np.int32)   # x, psi, delta, theta: rows 4 / 5 lie beyond n_states of some classes


def _engine(model, sets, n_seq):
    from cyclistsocialforce_amd.engine import Engine
    return Engine(sets[0], len(sets) * n_seq)


def _sums_reference(states, obj, feat, lengths, n_sets):
    """(sum d^2, sum |d|) per (set, sequence) from the trajectories, in extended precision; d itself is the fp64 difference"""
    n_seq, ns = len(lengths), states.shape[2]
    ref = np.zeros((n_sets, n_seq, 2), dtype=np.longdouble)
    for k in range(n_sets):
        for q in range(n_seq):
            ln = lengths[q]
            tr = np.zeros((ln, len(feat)))
            for c, f in enumerate(feat):
                if f < ns:
                    tr[:, c] = states[:ln, k * n_seq + q, f]
            d = (tr - obj[:ln, q, :]).astype(np.longdouble)
            ref[k, q, 0], ref[k, q, 1] = (d * d).sum(), np.abs(d).sum()
    return ref


def _check_sums(sums, ref, lengths, n_feat):
    worst = 0.0
    for q, ln in enumerate(lengths):
        m = int(ln) * n_feat                    # accumulated terms, all non-negative: relative 2 m 2^-53 (the 2: fused multiply-adds)
        for c in range(2):
            err = np.abs(sums[:, q, c].astype(np.longdouble) - ref[:, q, c])
            bound = 2.0 * m * 2.0 ** -53 * ref[:, q, c]
            if m:
                worst = max(worst, float((err / np.maximum(ref[:, q, c], np.longdouble(1e-300))).max()) / (2.0 * m * 2.0 ** -53))
            assert np.all(err <= bound), (q, c, err, bound)
    return worst


@pytest.mark.parametrize("model", MODELS)
def test_trajectories_equal_the_replay_path_and_sums_equal_numpy(model):
    """5 sequences (unequal lengths, one empty) x 7 parameter sets in one launch, both fix_speed values, stride 1 and 10: the
    states against csf_replay_forces on a twin engine that holds the seven sets (2e-7, the bar of test_calibration_replay), and
    the sums against NumPy on the same call's states (relative 2 m 2^-53)."""
    sets = pod_sets(model)
    s0, Fx, Fy = data_set(model, seed=MODELS.index(model))
    rng = np.random.default_rng(1)
    obj = rng.normal(size=(T, len(LENGTHS), len(FEAT)))
    e = _engine(model, sets, len(LENGTHS))
    e.calib_load(s0, Fx, Fy, obj, FEAT, lengths=LENGTHS, max_sets=len(sets))
    worst = 0.0
    for fix_speed in (True, False):
        for stride in (1, 10):
            sums, states = e.calib_eval(sets, fix_speed=fix_speed, states=True, stride=stride)
            twin = twin_states(model, sets, s0, Fx, Fy, LENGTHS, fix_speed, stride)
            assert states.shape == twin.shape == (T // stride, len(sets) * len(LENGTHS), e.ns)
            assert np.isfinite(states).all()
            diff = float(np.abs(states - twin).max())
            worst = max(worst, diff)
            print(f"{model} fix_speed={fix_speed} stride={stride}: largest |calib_eval - csf_replay_forces| = {diff:.3e}")
            np.testing.assert_allclose(states, twin, rtol=2e-7, atol=2e-7)
            assert not np.array_equal(states[:, : len(LENGTHS)], states[:, len(LENGTHS): 2 * len(LENGTHS)])   # the sets do differ
            if stride == 1:
                ref = _sums_reference(states, obj, FEAT, LENGTHS, len(sets))
                w = _check_sums(sums, ref, LENGTHS, len(FEAT))
                print(f"{model} fix_speed={fix_speed}: sums at {w:.3f} of the bound 2 m 2^-53")
                assert np.all(sums[:, LENGTHS == 0] == 0.0)
            else:
                assert np.array_equal(sums, e.calib_eval(sets, fix_speed=fix_speed))     # the states do not change the sums
    # an empty sequence keeps its start state; a finished one its last
    sums, states = e.calib_eval(sets, fix_speed=True, states=True)
    q0 = int(np.flatnonzero(LENGTHS == 0)[0])
    assert np.array_equal(states[:, q0], np.tile(states[0, q0], (T, 1)))
    np.testing.assert_allclose(states[0, q0, : s0.shape[1]], s0[q0], rtol=0, atol=1e-14)      # (the yaw has been through limitAngle)
    q1 = 3
    assert np.array_equal(states[LENGTHS[q1]:, q1], np.tile(states[LENGTHS[q1] - 1, q1], (T - LENGTHS[q1], 1)))
    print(f"{model}: largest difference over all cases {worst:.3e} ({'bit-identical' if worst == 0.0 else 'not bit-identical'})")
    e.calib_clear()
    assert e.n == 0
    e.close()


def test_golden_run_is_reproduced_next_to_perturbed_sets(golden):
    """demo_a_Fdest replayed from demo_a_s[0] with the default TwoD set reproduces demo_a_s (2e-7), six perturbed sets in the same
    launch.  The run was recorded on a route: its queue is given to the vehicles, as test_calibration_replay gives it to its engine -
    with the fresh vehicle's one-row queue (its own start, vehicle.py:183-185) the TwoD controller brakes within 3 m of it
    (vehicle.py:1226-1232) and the replay leaves the recorded run."""
    r = golden("dest_force_runs")
    S, F = r["demo_a_s"], r["demo_a_Fdest"]
    n = 300
    sets = pod_sets("twod")
    feat = np.arange(5, dtype=np.int32)
    e = _engine("twod", sets, 1)
    e.calib_load(S[:1], F[:n, 0:1], F[:n, 1:2], S[1: n + 1, None, :], feat, max_sets=len(sets))
    dq = r["demo_a_dq"]
    e.set_dest_queue(np.arange(len(sets)), np.arange(len(sets) + 1) * dq.shape[0], np.tile(dq, (len(sets), 1)), reset=True)
    sums, states = e.calib_eval(sets, fix_speed=False, states=True)
    print("golden: largest |state - demo_a_s| =", float(np.abs(states[:, 0] - S[1: n + 1]).max()), "sums of the default set:", sums[0, 0])
    np.testing.assert_allclose(states[:, 0], S[1: n + 1], rtol=2e-7, atol=2e-7)
    assert sums[0, 0, 0] < n * 5 * (2e-7 * 30) ** 2 and np.all(sums[1:, 0, 0] > 100 * sums[0, 0, 0])
    e.close()


def _calibration(model_cls, data, error_func, feat_ind, **kw):
    from cyclistsocialforce_amd import calibration as cal
    return cal.DownhillSimplexCalibration(model_cls, ["k_p_v", "k_p_delta"], data, data, feat_ind, error_func=error_func, verbose=False, **kw)


def _bicycle_data(theta, seed=4, n_seq=3, ticks=150):
    """tracks (Fx, Fy, x, y, psi, v, delta) whose states csf_replay_forces produced with the Bicycle set theta = (k_p_v, k_p_delta)"""
    from cyclistsocialforce_amd import calibration as cal, vehicle
    from cyclistsocialforce_amd.engine import Engine
    s0, Fx, Fy = data_set("bicycle", seed=seed, n_seq=n_seq, ticks=ticks)
    lens = np.array([ticks, ticks - 37, ticks - 80])[:n_seq]
    pod = vehicle.Bicycle.PARAMS_TYPE(k_p_v=theta[0], k_p_delta=theta[1]).to_pod(vehicle.Bicycle.MODEL)
    e = Engine(pod, n_seq)
    e.add_agents(s0, 0.0)
    st = e.replay_forces(Fx, Fy, lengths=lens, fix_speed=False)
    e.close()
    tracks = []
    for q in range(n_seq):
        d = np.zeros((lens[q] + 1, 7))
        d[0, 2:] = s0[q]
        d[1:, 0], d[1:, 1], d[1:, 2:] = Fx[: lens[q], q], Fy[: lens[q], q], st[: lens[q], q]
        tracks.append(d)
    return cal.CalibrationData(tracks, [0, 0, 1, 1, 1, 1, 0], [1, 1, 0, 0, 0, 0, 0], feature_keys=["Fx", "Fy", "x", "y", "psi", "v", "delta"])


def test_error_functions_through_the_calibration_object():
    """both reference error functions, formed from the device's sums, equal error_func(trajs, objectives) on the trajectories of
    simulate_single (relative 2 m 2^-53, m all the terms accumulated into the figure; a feature beyond n_states is among them)"""
    from cyclistsocialforce_amd import calibration as cal, vehicle
    data = _bicycle_data((10.0, 10.0))
    rng = np.random.default_rng(2)
    for trk in data.tracks:                                         # an objective the model cannot meet: errors of order one
        trk.data[:, 2:] += rng.normal(size=trk.data[:, 2:].shape)
    obj6 = cal.CalibrationData([np.c_[t.data, rng.normal(size=(t.data.shape[0], 1))] for t in data.tracks], [0, 0, 1, 0, 1, 1, 0, 1],
                               [1, 1, 0, 0, 0, 0, 0, 0], feature_keys=["Fx", "Fy", "x", "y", "psi", "v", "delta", "theta"])
    theta = np.array([[8.0, 12.0], [10.0, 10.0], [13.0, 7.0]])
    for func in (cal.calc_sse_timesteps, cal.calc_maesse_samples):
        c = _calibration(vehicle.Bicycle, obj6, func, [1, 0, 1, 1, 0, 1], fix_speed=False, max_sets=4)   # x, psi, v and theta (no such row: 0)
        errs = c.evaluate(theta)
        for k, th in enumerate(theta):
            trajs, objectives = c.simulate_single(c._update_params_args_dict(th))
            assert all(np.all(t[:, 3] == 0.0) for t in trajs)
            want = func(trajs, objectives)
            m = sum(t.size for t in trajs)
            print(func.__name__, th, errs[k], want, abs(errs[k] - want) / want / (2 * m * 2.0 ** -53))
            assert abs(errs[k] - want) <= 2 * m * 2.0 ** -53 * want
        custom = _calibration(vehicle.Bicycle, obj6, lambda o, b: cal.calc_sse_timesteps(o, b), [1, 0, 1, 1, 0, 1], fix_speed=False, max_sets=2)
        if func is cal.calc_sse_timesteps:                          # a custom error function takes the trajectories: the same numbers
            np.testing.assert_allclose(custom.evaluate(theta), errs, rtol=1e-12)
        custom.close()
        c.close()


def test_an_evaluation_does_not_depend_on_the_one_before():
    """the same sets after a different call, and in another order: bit-identical sums"""
    for model in ("invpend", "planarpoint"):
        sets = pod_sets(model)
        s0, Fx, Fy = data_set(model, seed=9)
        obj = np.random.default_rng(3).normal(size=(T, len(LENGTHS), 2))
        e = _engine(model, sets, len(LENGTHS))
        e.calib_load(s0, Fx, Fy, obj, [0, 1], lengths=LENGTHS, max_sets=len(sets))
        first = e.calib_eval(sets, fix_speed=False)
        e.calib_eval(sets[3:5], fix_speed=True)
        e.calib_eval(sets[::-1][:6], fix_speed=False, states=True, stride=7)
        assert np.array_equal(e.calib_eval(sets, fix_speed=False), first)
        assert np.array_equal(e.calib_eval(sets[::-1], fix_speed=False), first[::-1])
        assert np.array_equal(e.calib_eval([sets[4]], fix_speed=False)[0], first[4])
        assert e.state().shape == (len(sets) * len(LENGTHS), e.ns)   # read-backs work on a loaded engine
        e.close()


def test_launches_per_call_do_not_grow():
    counts = []
    for n_sets, ticks in ((4, 120), (200, 300)):
        sets = pod_sets("twod", 2) * (n_sets // 2)
        s0, Fx, Fy = data_set("twod", seed=5, n_seq=2, ticks=ticks)
        e = _engine("twod", sets, 2)
        e.calib_load(s0, Fx, Fy, np.zeros((ticks, 2, 1)), [0], max_sets=n_sets)
        assert e.calib_launches() == 0
        a = e.calib_eval(sets)
        assert e.calib_launches() == 1
        b, _ = e.calib_eval(sets, states=True, stride=3)
        counts.append(e.calib_launches())
        assert np.array_equal(a, b) and np.array_equal(a[0], a[2])
        e.close()
    assert counts == [2, 2]


def test_recovery_of_two_parameters():
    """objective generated by csf_replay_forces at theta*; from a guess 30 % off `run` (scipy) and run_many([guess]) return the same
    xopt / fopt, and fopt is no larger than the smallest error among theta* with one parameter moved by +-1 %"""
    from cyclistsocialforce_amd import vehicle
    from cyclistsocialforce_amd import calibration as cal
    star = np.array([9.0, 11.0])
    data = _bicycle_data(star)
    c = _calibration(vehicle.Bicycle, data, cal.calc_sse_timesteps, [1, 1, 1, 1, 0, 0], fix_speed=False, maxiter=120, max_sets=8)
    guess = star * np.array([1.3, 0.7])
    res = c.run(guess)
    (x, f, it), = c.run_many([guess])
    print("recovery: xopt", res[0], "fopt", res[1], "iterations", res[2], "| run_many", x, f, it)
    assert np.array_equal(x, res[0]) and f == res[1] and it == res[2]
    near = c.evaluate([star * [1.01, 1], star * [0.99, 1], star * [1, 1.01], star * [1, 0.99]])
    print("errors at theta* with one parameter moved by 1 %:", near, "at theta*:", c.evaluate([star]))
    assert f <= near.min()
    err, vehicles = c.test()
    assert err == pytest.approx(f, rel=1e-9, abs=1e-18) and len(vehicles) == 3 and vehicles[0].traj.shape[0] == 6
    c.close()


def _child(mode, extra_env=None):
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k != "CSF_PAIR_VARIANT"}
    env.update(extra_env or {})
    r = subprocess.run([sys.executable, os.path.join(here, "calib_abi_child.py"), mode], capture_output=True, text=True, timeout=600,
                       env={**env, "PYTHONPATH": os.path.dirname(here) + os.pathsep + here})
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert f"calib {mode} ok" in r.stdout


def test_evaluation_state_with_poisoned_buffers():
    """CSF_DEBUG_POISON=1: nothing of an evaluation depends on what lies behind the population or the buffers"""
    _child("state", {"CSF_DEBUG_POISON": "1"})


def test_refusals_and_lifetime_in_a_fresh_process():
    """every refusal of csf_calib_load / csf_calib_eval comes back negative with a message and changes nothing; 30 load / eval /
    clear / destroy rounds lose no device memory"""
    _child("abi")
