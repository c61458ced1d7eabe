"""Riders that follow their recorded trajectory in a closed-loop calibration: csf_scene_calib_replay against a
twin stepped tick by tick through csf_push_state, against the evaluation without a replay, the oracle, and the optimiser on
leave-one-out scenes."""
import ctypes as C
import functools

import numpy as np
import pytest

from scene_calib_common import ORACLE_TICKS, VDES, crowd, field_sets, twin_scene
from scene_replay_common import (LENGTHS, N_RIDERS, ORACLE_REPLAYED, T, TRUE_SET, masks, oracle_recording, oracle_replay_run, replay_scenes)
from test_gpu_scene_calib import _check_sums, _sums_reference

pytestmark = [pytest.mark.gpu, pytest.mark.auto_variant]

FEAT = np.array([0, 2, 4, 5], dtype=np.int32)   # x, psi, delta, theta: rows 4 / 5 lie beyond n_states of some classes
CASES = [("twod", 0), ("twod", 1), ("bicycle", 0), ("invpend", 0), ("planarpoint", 0), ("planarbike", 0), ("balancingrider", 0)]
ROFF = np.r_[0, np.cumsum(N_RIDERS)]
R = int(ROFF[-1])
TWIN_TOL = 2e-7                                 # the bar of tests/test_gpu_scene_calib.py against its twin (rtol = atol)


def _sets(model, rule):
    sets = field_sets(model, 3)
    for p in sets:
        p.priority_rule = rule
    return sets


@functools.lru_cache(maxsize=None)
def _job(model, rule):
    """the data set of one class: scenes, candidate sets, the recording - one twin_scene run per scene with the true set - and the
    rows of the replayed riders as csf_scene_calib_replay takes them.  Rows behind a scene's length are never read: NaN there."""
    sets = _sets(model, rule)
    s0, off, rows, per = replay_scenes(model)
    rec = [twin_scene(sets[TRUE_SET], sq, oq, dq, T)[0] for sq, oq, dq in per[:5]]
    rec.append(np.full((T, 1, s0.shape[1]), np.nan))              # (the empty scene has no recording)
    rec = np.concatenate(rec, axis=1)                            # [T, R, n_states]
    per_mask, mask = masks()
    rep_rows = rec[:, mask, :4].copy()
    col = np.cumsum(mask) - 1                                    # rider -> its column of rep_rows
    for q, ln in enumerate(LENGTHS):
        riders = ROFF[q] + np.flatnonzero(per_mask[q])
        rep_rows[ln:, col[riders]] = np.nan
    obj = np.random.default_rng(1).normal(size=(T, R, len(FEAT)))
    return dict(sets=sets, s0=s0, off=off, rows=rows, per=per, rec=rec, per_mask=per_mask, mask=mask, rep_rows=rep_rows, obj=obj)


def _loaded(job, replay=True):
    from cyclistsocialforce_amd.engine import Engine
    e = Engine(job["sets"][0], len(job["sets"]) * R)
    e.scene_calib_load(N_RIDERS, job["s0"], VDES, job["off"], job["rows"], job["obj"], FEAT, lengths=LENGTHS, max_sets=len(job["sets"]))
    if replay:
        e.scene_calib_replay(job["mask"], job["rep_rows"])
    return e


def _replay_twin(pod, s0, off, dq, ticks, mask, rec):
    """the existing pieces: an engine with that set steps that scene alone, one tick per call, and after every tick (x, y, psi, v)
    of the replayed riders is replaced through csf_push_state; returns the states [ticks, n, n_states] behind the push"""
    from cyclistsocialforce_amd.engine import Engine
    n = s0.shape[0]
    e = Engine(pod, n)
    e.add_agents(s0, VDES)
    e.set_dest_queue(np.arange(n), off, dq, reset=True)
    idx = np.flatnonzero(mask).astype(np.int32)
    out = np.zeros((ticks, n, e.ns))
    for t in range(ticks):
        e.step(1)
        s = e.state()
        if idx.size:
            s[idx, :4] = rec[t, idx, :4]
            e.push_state(idx, s[idx])
        out[t] = s
    assert e.small_ticks() == ticks
    e.close()
    return out


@pytest.mark.parametrize("model,rule", CASES)
def test_replayed_scenes_equal_a_twin_that_pushes_the_recording_every_tick(model, rule):
    """Six scenes (2, 5, 32, 4, 3, 1 riders; lengths T, 25, T, T, T, 0 with T = 40; replayed: rider 1 / riders 0 and 3 / riders 0, 31
    and every third / none / all / the rider) x 3 sets in one launch against a twin per (set, scene): step(1), state(), the replayed
    riders' (x, y, psi, v) replaced, push_state.  All rows of the simulated riders within 2e-7 (rtol = atol, the bar of the twin
    test of tests/test_gpu_scene_calib.py; the expectation is 0); rows 0 - 3 of the replayed riders ARE the recording; their sums
    are (0, 0); the sums of the simulated riders are NumPy's on the returned states within 2 m 2^-53."""
    job = _job(model, rule)
    sets, mask, rec = job["sets"], job["mask"], job["rec"]
    K = len(sets)
    e = _loaded(job)
    sums, states = e.scene_calib_eval(sets, states=True)
    assert states.shape == (T, K * R, e.ns) and sums.shape == (K, R, 2)
    worst = 0.0
    for k, pod in enumerate(sets):
        for q, (sq, oq, dq) in enumerate(job["per"]):
            ln, sl, pm = int(LENGTHS[q]), slice(ROFF[q], ROFF[q + 1]), job["per_mask"][q]
            got = states[:, k * R + ROFF[q]: k * R + ROFF[q + 1]]
            if ln:
                tw = _replay_twin(pod, sq, oq, dq, ln, pm, rec[:, sl])
                assert np.isfinite(got[:ln][:, ~pm]).all()
                if (~pm).any():
                    worst = max(worst, float(np.abs(got[:ln][:, ~pm] - tw[:, ~pm]).max()))
                np.testing.assert_allclose(got[:ln][:, ~pm], tw[:, ~pm], rtol=TWIN_TOL, atol=TWIN_TOL, err_msg=f"set {k} scene {q}")
                assert np.array_equal(got[:ln][:, pm, :4], rec[:ln, sl][:, pm, :4]), (k, q)
                assert np.array_equal(got[ln:], np.tile(got[ln - 1], (T - ln, 1, 1))), (k, q)     # an ended scene keeps its last state
            else:
                assert np.array_equal(got, np.tile(got[0], (T, 1, 1)))
    print(f"{model} rule {rule}: largest |scene_calib_eval with replay - push_state twin| over the simulated riders = {worst:.3e} "
          f"({'bit-identical' if worst == 0.0 else 'not bit-identical'})")
    assert np.all(sums[:, mask] == 0.0)
    ref = _sums_reference(states, job["obj"], FEAT, LENGTHS, ROFF, K)
    ref[:, mask] = 0.0                                           # (a replayed rider adds nothing)
    w = _check_sums(sums, ref, LENGTHS, ROFF, len(FEAT))
    print(f"{model} rule {rule}: sums of the simulated riders at {w:.3f} of the bound 2 m 2^-53")
    live = ~mask & (LENGTHS[np.repeat(np.arange(len(N_RIDERS)), N_RIDERS)] > 0)
    assert np.all(sums[:, live] > 0.0)
    e.close()


def test_the_replay_acts_and_at_the_true_set_the_simulated_riders_follow_the_recording():
    """For a set other than the true one the simulated riders of scenes 1 - 3 differ from the same evaluation without a replay (their
    sources are elsewhere; the scenes are seeded so that each of these riders has a replayed one in view, scene_replay_common.SCENE_SEEDS);
    at the true set every simulated rider repeats the recording, all rows, within the twin bound - its sources are the recording
    it was made beside."""
    job = _job("twod", 0)
    sets, rec = job["sets"], job["rec"]
    e = _loaded(job)
    _, with_rep = e.scene_calib_eval(sets, states=True)
    e.scene_calib_replay(None)
    _, without = e.scene_calib_eval(sets, states=True)
    e.close()
    other = 0 if TRUE_SET != 0 else 2
    worst = 0.0
    for q in range(5):
        ln, pm = int(LENGTHS[q]), job["per_mask"][q]
        sim = ROFF[q] + np.flatnonzero(~pm)
        if q < 3:
            moved = [not np.array_equal(with_rep[:ln, other * R + r], without[:ln, other * R + r]) for r in sim]
            print(f"scene {q}: {sum(moved)} of {len(moved)} simulated riders differ from the evaluation without a replay")
            assert all(moved), (q, moved)
        if sim.size:
            got, want = with_rep[:ln, TRUE_SET * R + sim], rec[:ln, sim]
            worst = max(worst, float(np.abs(got - want).max()))
            np.testing.assert_allclose(got, want, rtol=TWIN_TOL, atol=TWIN_TOL, err_msg=f"scene {q}")
        if not pm.any():                                         # the scene without a replay is what it is without one
            assert np.array_equal(with_rep[:, ROFF[q]: ROFF[q + 1]], without[:, ROFF[q]: ROFF[q + 1]])
    print(f"at the true set: largest |simulated rider - recording| = {worst:.3e}")


def test_without_a_replay_an_evaluation_is_what_it_was_and_calls_are_independent():
    """After scene_calib_replay(None), and with a mask that marks nobody, sums and states equal - array_equal - those of an engine
    that never had a replay; with a replay the same call twice, a permuted list of sets and a single set give the same figures."""
    job = _job("twod", 0)
    sets = job["sets"]
    fresh = _loaded(job, replay=False)
    want, want_st = fresh.scene_calib_eval(sets, states=True)
    fresh.close()
    e = _loaded(job)
    sums, states = e.scene_calib_eval(sets, states=True)
    assert not np.array_equal(sums, want)
    again, st_again = e.scene_calib_eval(sets, states=True)
    assert np.array_equal(again, sums) and np.array_equal(st_again, states)
    assert np.array_equal(e.scene_calib_eval(sets), sums)
    perm = np.array([2, 0, 1])
    sp, stp = e.scene_calib_eval([sets[i] for i in perm], states=True)
    assert np.array_equal(sp, sums[perm])
    assert np.array_equal(stp.reshape(T, 3, R, -1), states.reshape(T, 3, R, -1)[:, perm])
    one, st1 = e.scene_calib_eval([sets[2]], states=True)
    assert np.array_equal(one[0], sums[2]) and np.array_equal(st1, states[:, 2 * R:])
    e.scene_calib_replay(None)
    got, got_st = e.scene_calib_eval(sets, states=True)
    assert np.array_equal(got, want) and np.array_equal(got_st, want_st)
    e.scene_calib_replay(job["mask"], job["rep_rows"])
    assert np.array_equal(e.scene_calib_eval(sets), sums)
    e.scene_calib_replay(np.zeros(R, dtype=bool))
    got, got_st = e.scene_calib_eval(sets, states=True)
    assert np.array_equal(got, want) and np.array_equal(got_st, want_st)
    e.scene_calib_clear()
    assert e.n == 0
    e.close()


def test_replayed_scene_against_the_oracle():
    """twod, 5 riders under the priority-to-the-right rule, riders 1 and 3 replayed from an oracle run with the second of the three
    oracle_fields sets; the three sets in one launch against orc.Population stepped tick by tick with its own push_state, 200
    ticks, positions of the simulated riders at stride 10 within 1e-4 x extent (the bound of test_scenes_against_the_oracle).  The
    oracle's own sensitivity on this case: tests/test_scene_replay_host.py::test_the_replayed_oracle_is_not_chaotic_on_the_horizon."""
    from cyclistsocialforce_amd.engine import Engine
    s0, off, dq, pods, rec = oracle_recording()
    n, sim = s0.shape[0], ~ORACLE_REPLAYED
    e = Engine(pods[0], len(pods) * n)
    e.scene_calib_load([n], s0, 5.0, off, dq, np.zeros((ORACLE_TICKS, n, 1)), [0], max_sets=len(pods))
    e.scene_calib_replay(ORACLE_REPLAYED, rec[:, ORACLE_REPLAYED, :4])
    _, states = e.scene_calib_eval(pods, states=True, stride=10)
    e.close()
    for k, pod in enumerate(pods):
        ref = oracle_replay_run(pod, s0, off, dq, rec, ORACLE_REPLAYED)
        ext = max(np.ptp(ref[..., 0]), np.ptp(ref[..., 1]), 14.0)
        got = states[:, k * n: (k + 1) * n, :2]
        worst = float(np.hypot(got[:, sim, 0] - ref[:, sim, 0], got[:, sim, 1] - ref[:, sim, 1]).max())
        print(f"set {k}: largest position deviation of a simulated rider {worst:.3e} m = {worst / ext:.2e} x extent")
        assert worst < 1e-4 * ext, k
        assert np.array_equal(got[:, ORACLE_REPLAYED], rec[9::10][:, ORACLE_REPLAYED, :2])


def test_refusals_change_nothing():
    """csf_scene_calib_replay without a data set and on the data set of csf_calib_load (CSF_E_STATE), without rows for a marked
    rider and with a non-finite row that a tick reads (CSF_E_ARG): negative, a message, and the next evaluation equals the one
    before - with and without a replay in place.  A non-finite row behind a scene's length is not read and not refused.  (The
    refusal for device memory - allocations and copies run before anything is replaced - is not provoked here.)"""
    from cyclistsocialforce_amd.engine import Engine
    E_ARG, E_STATE = -1, -4
    job = _job("twod", 0)
    sets, mask, rows = job["sets"], job["mask"], job["rep_rows"]
    m8 = np.ascontiguousarray(mask, dtype=np.uint8)
    P = lambda a: a.ctypes.data_as(C.c_void_p)                   # noqa: E731
    e = Engine(sets[0], len(sets) * R)
    L = e._lib
    assert L.csf_scene_calib_replay(e._h, P(m8), P(rows)) == E_STATE and b"csf_scene_calib_replay" in L.csf_last_error(e._h)
    s0 = np.zeros((2, 8))
    s0[:, 3] = 4.0
    e.calib_load(s0, np.ones((5, 2)), np.zeros((5, 2)), np.zeros((5, 2, 1)), [0], max_sets=1)
    assert L.csf_scene_calib_replay(e._h, P(m8), P(rows)) == E_STATE
    assert L.csf_scene_calib_replay(e._h, None, None) == E_STATE
    e.calib_clear()
    e.close()
    bad = rows.copy()
    bad[int(LENGTHS[1]) - 1, 1, 2] = np.inf                      # rider 0 of the second scene, its last tick
    for replay in (False, True):
        e = _loaded(job, replay=replay)
        before, st_before = e.scene_calib_eval(sets, states=True)
        assert L.csf_scene_calib_replay(e._h, P(m8), None) == E_ARG and b"rows" in L.csf_last_error(e._h)
        assert L.csf_scene_calib_replay(e._h, P(m8), P(bad)) == E_ARG and b"finite" in L.csf_last_error(e._h)
        with pytest.raises(ValueError):
            e.scene_calib_replay(mask[:-1], rows)
        with pytest.raises(ValueError):
            e.scene_calib_replay(mask, rows[:, :-1])
        after, st_after = e.scene_calib_eval(sets, states=True)
        assert np.array_equal(after, before) and np.array_equal(st_after, st_before)
        e.close()
    assert np.isnan(rows[int(LENGTHS[1]):, 1]).all()              # (what _loaded(replay=True) was accepted with)


def _ego_recovery_data(star):
    """3 scenes of 3 - 5 TwoD riders over 150 ticks recorded by the engine itself at theta* = (f_0, sigma_0), split into their 12
    leave-one-out scenes"""
    from cyclistsocialforce_amd import calibration as cal, parameters
    from cyclistsocialforce_amd.engine import Engine
    data = []
    for q, n in enumerate((3, 4, 5)):
        x, y, psi, v, off, dq = crowd(n, seed=300 + q, box=10.0)
        s0 = np.c_[x, y, psi, v, np.zeros(n)]
        pod = parameters.default_pod("twod", f_0=star[0], sigma_0=star[1])
        e = Engine(pod, n)
        e.scene_calib_load([n], s0, 5.0, off, dq, np.zeros((150, n, 1)), [0], max_sets=1)
        _, st = e.scene_calib_eval([pod], states=True)
        e.close()
        data.extend(cal.SceneData(s0, 5.0, off, dq, st).ego_split())
    return data


def test_recovery_of_two_field_parameters_on_leave_one_out_scenes():
    """The recovery test of tests/test_gpu_scene_calib.py with its numbers, on ego scenes: every rider in turn is the only simulated
    one, the others follow the recording made at theta* = (9, 0.9).  f(theta*) is exactly 0; from two guesses run_many returns theta
    within xtol = 1e-4 of theta* and the objective below 1e-6 of its start; `run` and run_many agree bit for bit from a guess."""
    from cyclistsocialforce_amd import calibration as cal, vehicle
    star = np.array([9.0, 0.9])
    data = _ego_recovery_data(star)
    assert len(data) == 12 and all((~d.replayed).sum() == 1 for d in data)
    xtol = 1e-4
    c = cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0", "sigma_0"], data, data, [1, 1, 0, 0, 0, 0], max_sets=8, maxiter=400,
                                   xtol=xtol, ftol=1e-30)
    f_star = c.evaluate([star])[0]
    guesses = [star * [1.25, 0.85], star * [0.8, 1.2]]
    f_start = c.evaluate(guesses)
    res = c.run(guesses[0])
    many = c.run_many(guesses)
    print("ego recovery: run", res[0], res[1], "iterations", res[2], "| run_many", [(x, f, it) for x, f, it in many], "| f(theta*)", f_star,
          "f(guesses)", f_start)
    x, f, it = many[0]
    assert np.array_equal(x, res[0]) and f == res[1] and it == res[2]
    assert f_star == 0.0
    for (x, f, it), f0 in zip(many, f_start):
        assert np.abs(x - star).max() <= xtol, (x, star)
        assert f < 1e-6 * f0
    trajs, objectives = c.simulate(star)
    assert all(t.shape == (150, 1, 2) and np.array_equal(t, o) for t, o in zip(trajs, objectives))
    c.close()
