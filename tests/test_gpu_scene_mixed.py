"""Several simulated vehicle classes in one scene of a closed-loop calibration: csf_scene_calib_classes and
csf_scene_calib_eval_groups against twin engines on the general path that hold one parameter set per group and class, against the literal
reference's recording of fifteen vehicles of five classes, against the oracle, against the grouped evaluation of one class, with the other
hooks, and the optimiser."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from scene_calib_common import VDES, crowd
from scene_groups_common import general_twin
from scene_mixed_common import (ACT_MOVED, ACT_TICKS, G, GENERAL_TOL, GROUP, GROUPS, HOOK_BOX, HOOK_CLASSES, HOOK_GROUP, HOOK_SEED, LENGTHS,
                                MODELS, N_RIDERS, ORACLE_GROUP, ORACLE_TICKS, R, ROFF, T, act_pods, act_scene, mixed_scenes, mixed_sets,
                                oracle_case, oracle_mixed_run, wide_state)
from test_gpu_scene_calib import _check_sums, _sums_reference

pytestmark = [pytest.mark.gpu, pytest.mark.auto_variant]

FEAT = np.array([0, 2, 4, 5], dtype=np.int32)   # x, psi, delta, theta: rows 4 / 5 lie beyond n_states of some classes
ONE_CLASS = ("twod", "bicycle", "invpend", "planarpoint", "planarbike", "balancingrider")


def _engine(pod, cap):
    from cyclistsocialforce_amd.engine import Engine
    return Engine(pod, cap)


@functools.lru_cache(maxsize=None)
def _job():
    s0, off, rows, per = mixed_scenes()
    obj = np.random.default_rng(1).normal(size=(T, R, len(FEAT)))
    return dict(sets=mixed_sets(), s0=s0, off=off, rows=rows, per=per, obj=obj)


def _loaded(job, classes=True, n_riders=N_RIDERS, lengths=LENGTHS, max_sets=3, group=GROUP):
    e = _engine(job["sets"][0][0], max_sets * int(np.sum(n_riders)))
    e.scene_calib_load(n_riders, job["s0"], VDES, job["off"], job["rows"], job["obj"], FEAT, lengths=lengths, max_sets=max_sets)
    if classes:
        e.scene_calib_classes(group, MODELS, job["s0"])
    return e


def _against_twins(states, sets, per, groups, lengths, roff, what, **hooks):
    """every (candidate, scene) of `states` against its general-path twin: all state rows of the riders the twin has, at every tick.  The
    twin holds the candidate's records as parameter classes: its state is as wide as the widest class AMONG THEM, the evaluation's as
    wide as the widest loaded class - the rows beyond the twin's are rows no class of the scene has, and stay 0."""
    n_all, worst = int(roff[-1]), 0.0
    for k, pods in enumerate(sets):
        for q, (sq, oq, dq) in enumerate(per):
            ln = int(lengths[q])
            if ln == 0:
                continue
            kw = {name: val[q] for name, val in hooks.items()}
            tw = general_twin(pods, groups[q], sq[:, : _twin_width(pods)], oq, dq, ln, **kw)
            got = states[:ln, k * n_all + roff[q]: k * n_all + roff[q + 1]]
            there = np.isfinite(tw[..., 0])
            assert np.isfinite(got[there]).all(), (k, q)
            w = tw.shape[2]
            d = float(np.abs(got[there][:, :w] - tw[there]).max()) if there.any() else 0.0
            assert np.all(got[there][:, w:] == 0.0), (what, k, q)
            worst = max(worst, d)
            print(f"{what}: candidate {k}, scene {q}: {d:.3e}")
            assert d < GENERAL_TOL, (what, k, q, d)
    print(f"{what}: largest |scene_calib_eval_groups - general-path twin| over all state rows and ticks = {worst:.3e} (bound {GENERAL_TOL:g})")
    return worst


def _twin_width(pods):
    from cyclistsocialforce_amd import _ffi
    return max(_ffi.N_STATES[p.model] for p in pods)


def test_mixed_scenes_against_general_path_twins():
    """Seven scenes in one data set - a: 2 riders (twod, invpend); b: 5 (twod, bicycle, bicycle, invpend, twod); c: 32 round robin over
    all six classes; d: 3, all Bicycles (group 1: nothing class-dependent may come from record 0, a TwoD's); e: one InvPendulum; f: 4,
    length 0; g: 25 riders, length 25 < T - x 3 candidates of six records that differ in field, field of view, gains and v_max_riding,
    candidate 1 with the second priority rule, in ONE launch: the states after every tick, every state row, against a twin engine per
    (candidate, scene) on the general path that holds the six records as parameter classes.  Bound: 2e-5 (scene_groups_common.py)."""
    job = _job()
    sets = job["sets"]
    e = _loaded(job)
    assert e.ns == 8
    before = e.scene_calib_launches()
    sums, states = e.scene_calib_eval_groups(sets, states=True)
    assert e.scene_calib_launches() == before + 1
    assert states.shape == (T, 3 * R, 8) and sums.shape == (3, R, 2)
    _against_twins(states, sets, job["per"], GROUPS, LENGTHS, ROFF, "scenes")
    w = _check_sums(sums, _sums_reference(states, job["obj"], FEAT, LENGTHS, ROFF, 3), LENGTHS, ROFF, len(FEAT))
    print(f"sums at {w:.3f} of the bound 2 m 2^-53")
    # f: length 0 - states and sums show nothing but the start; g: the samples behind its 25 ticks repeat the last state
    for k in range(3):
        f = states[:, k * R + ROFF[5]: k * R + ROFF[6]]
        start = np.tile(job["s0"][ROFF[5]: ROFF[6], :4], (T, 1, 1))
        assert np.array_equal(f[:, :, [0, 1, 3]], start[:, :, [0, 1, 3]]) and np.abs(f[:, :, 2] - start[:, :, 2]).max() < 1e-14   # (psi: limitAngle)
        assert np.all(f[:, :, 4:] == 0.0)
        g = states[:, k * R + ROFF[6]: k * R + ROFF[7]]
        assert np.array_equal(g[25:], np.tile(g[24], (T - 25, 1, 1)))
    assert np.all(sums[:, ROFF[5]: ROFF[6]] == 0.0)
    # rows a class lacks stay 0
    from cyclistsocialforce_amd import _ffi
    for r in range(R):
        assert np.all(states[:, r::R, _ffi.N_STATES[int(MODELS[GROUP[r]])]:] == 0.0), r
    # twice, and with the candidates permuted
    sums2, states2 = e.scene_calib_eval_groups(sets, states=True)
    assert np.array_equal(sums, sums2) and np.array_equal(states, states2)
    perm = [2, 0, 1]
    sums3, states3 = e.scene_calib_eval_groups([sets[k] for k in perm], states=True)
    assert e.scene_calib_launches() == before + 3
    for at, k in enumerate(perm):
        assert np.array_equal(sums3[at], sums[k]) and np.array_equal(states3[:, at * R: (at + 1) * R], states[:, k * R: (k + 1) * R])
    e.close()


def test_fifteen_vehicles_of_five_classes_against_the_literal_reference(golden):
    """tests/golden/mixed.npz as ONE scene: 15 vehicles of five classes, the 10 parameter sets of conftest.mixed_classes as 10 groups, 250
    ticks, one candidate, states at stride 10: positions within 1e-4 x extent of S[1:], the other rows within 2e-3 - the bounds of
    tests/test_gpu_hetero.py::test_several_vehicle_classes_golden for the general path on the same data."""
    from conftest import mixed_classes
    g = golden("mixed")
    pods, cls = mixed_classes(g)
    n = g["s0"].shape[0]
    S = g["S"]
    ticks = 10 * (S.shape[0] - 1)
    e = _engine(pods[0], n)
    e.scene_calib_load([n], g["s0"], g["vdes"], g["off"], g["dq"], np.zeros((ticks, n, 2)), [0, 1], max_sets=1)
    e.scene_calib_classes(cls, [p.model for p in pods], g["s0"])
    assert e.ns == 6
    before = e.scene_calib_launches()
    _, states = e.scene_calib_eval_groups([tuple(pods)], states=True, stride=10)
    assert e.scene_calib_launches() == before + 1
    extent = max(np.ptp(S[..., 0]), np.ptp(S[..., 1]), 1.0)
    pos = float(np.abs(states[:, :, :2] - S[1:, :, :2]).max()) / extent
    rest = float(np.abs(states[:, :, 2:] - S[1:, :, 2:]).max())
    print(f"mixed golden: positions {pos:.3e} x extent (bound 1e-4), other rows {rest:.3e} (bound 2e-3)")
    assert pos < 1e-4 and rest < 2e-3
    e.close()


@pytest.mark.parametrize("rule", [0, 1])
def test_mixed_scene_against_the_oracle(rule):
    """5 riders of three classes (twod, bicycle, invpend), 200 free ticks, 3 candidates: positions after every 10th tick within 1e-4 x
    extent of orc.Population with set_classes; tests/test_scene_mixed_host.py holds the oracle's own sensitivity below 1e-5 x extent"""
    s0, off, dq, pods = oracle_case(rule)
    e = _engine(pods[0][0], 3 * 5)
    e.scene_calib_load([5], s0, VDES, off, dq, np.zeros((ORACLE_TICKS, 5, 2)), [0, 1], max_sets=3)
    e.scene_calib_classes(ORACLE_GROUP, [p.model for p in pods[0]], s0)
    _, states = e.scene_calib_eval_groups(pods, states=True, stride=10)
    worst = 0.0
    for k, pd in enumerate(pods):
        ref = oracle_mixed_run(pd, ORACLE_GROUP, s0, off, dq, ORACLE_TICKS, stride=10)
        ext = max(np.ptp(ref[..., 0]), np.ptp(ref[..., 1]), 14.0)
        got = states[:, k * 5: (k + 1) * 5, :2]
        dev = float(np.hypot(got[..., 0] - ref[..., 0], got[..., 1] - ref[..., 1]).max()) / ext
        worst = max(worst, dev)
        assert dev < 1e-4, (rule, k, dev)
    print(f"rule {rule}: largest |scene_calib_eval_groups - oracle| = {worst:.2e} x extent")
    e.close()


@pytest.mark.parametrize("model", ONE_CLASS)
def test_one_class_is_todays(model):
    """all groups of ONE class through scene_calib_classes against the same data through scene_calib_groups (2e-5; whether it is
    array_equal is printed: the merged kernel is a compilation of its own), and after scene_calib_classes(None) the plain evaluation is
    array_equal to the one before the call"""
    from scene_groups_common import G as G4, GROUP as GROUP4, N_RIDERS as NR4, LENGTHS as LN4, R as R4, T as T4, group_scenes, group_sets
    from cyclistsocialforce_amd.engine import MODEL_IDS
    s0, off, rows, _ = group_scenes(model)
    sets = group_sets(model)
    obj = np.random.default_rng(1).normal(size=(T4, R4, len(FEAT)))
    e = _engine(sets[0][0], 3 * R4)
    e.scene_calib_load(NR4, s0, VDES, off, rows, obj, FEAT, lengths=LN4, max_sets=3)
    ns = e.ns
    p0, ps0 = e.scene_calib_eval([p[0] for p in sets], states=True)
    e.scene_calib_groups(GROUP4, G4)
    a, sa = e.scene_calib_eval_groups(sets, states=True)
    e.scene_calib_classes(GROUP4, [MODEL_IDS[model]] * G4, s0)
    assert e.ns == ns
    b, sb = e.scene_calib_eval_groups(sets, states=True)
    d = float(np.abs(sa - sb).max())
    print(f"{model}: one class through scene_calib_classes against scene_calib_groups: {d:.3e}, array_equal: {np.array_equal(sa, sb) and np.array_equal(a, b)}")
    assert d < GENERAL_TOL
    e.scene_calib_groups(GROUP4, G4)                               # (that call replaces the classes)
    a2, sa2 = e.scene_calib_eval_groups(sets, states=True)
    assert np.array_equal(a, a2) and np.array_equal(sa, sa2)
    e.scene_calib_classes(GROUP4, [MODEL_IDS[model]] * G4, s0)
    e.scene_calib_classes(None)
    assert e.ns == ns
    p1, ps1 = e.scene_calib_eval([p[0] for p in sets], states=True)
    assert np.array_equal(p0, p1) and np.array_equal(ps0, ps1)
    e.close()


def test_labels_are_only_labels():
    """permuting the group labels together with `models` and the records gives array_equal results (candidates 0 and 1: every record has the
    candidate's priority rule)"""
    job = _job()
    e = _loaded(job)
    s0, st0 = e.scene_calib_eval_groups(job["sets"][:2], states=True)
    perm = np.array([3, 5, 0, 1, 4, 2])                            # new label of old group g
    inv = np.argsort(perm)
    e.scene_calib_classes(perm[GROUP].astype(np.uint8), MODELS[inv], job["s0"])
    s1, st1 = e.scene_calib_eval_groups([tuple(p[inv[g]] for g in range(G)) for p in job["sets"][:2]], states=True)
    assert np.array_equal(s0, s1) and np.array_equal(st0, st1)
    e.close()


def test_the_classes_act():
    """two riders, one a Bicycle: swapping which of the two it is changes both trajectories by more than ACT_MOVED (a tenth of what the
    CPU oracle finds for the less affected rider: tests/test_scene_mixed_host.py)"""
    s0, off, dq = act_scene()
    tw, bi = act_pods()
    e = _engine(tw, 2)
    e.scene_calib_load([2], s0, VDES, off, dq, np.zeros((ACT_TICKS, 2, 2)), [0, 1], max_sets=1)
    out = []
    for grp in ([0, 1], [1, 0]):
        e.scene_calib_classes(np.array(grp, dtype=np.uint8), [tw.model, bi.model], s0)
        out.append(e.scene_calib_eval_groups([(tw, bi)], states=True)[1])
    moved = np.abs(out[0][..., :2] - out[1][..., :2]).max(axis=(0, 2))
    print(f"the classes act: the riders move by {moved} m")
    assert np.all(moved > ACT_MOVED)
    e.close()


# ---- the other hooks: one scene of 8 riders - two replayed (a BalancingRider and a TwoD), the simulated ones Bicycles and InvPendulums


@functools.lru_cache(maxsize=None)
def _hook_job():
    from cyclistsocialforce_amd.engine import MODEL_IDS
    x, y, psi, v, off, dq = crowd(8, seed=HOOK_SEED, box=HOOK_BOX)
    sets = mixed_sets(3, HOOK_CLASSES)
    return dict(s0=wide_state(x, y, psi, v), off=off, dq=dq, sets=sets, models=[MODEL_IDS[m] for m in HOOK_CLASSES],
                obj=np.random.default_rng(2).normal(size=(T, 8, len(FEAT))))


def _hook_engine(job):
    e = _engine(job["sets"][0][0], 3 * 8)
    e.scene_calib_load([8], job["s0"], VDES, job["off"], job["dq"], job["obj"], FEAT, max_sets=3)
    e.scene_calib_classes(HOOK_GROUP, job["models"], job["s0"])
    return e


def test_mixed_classes_with_replay():
    """a replayed BalancingRider and a replayed TwoD among simulated Bicycles and InvPendulums: rows 0 - 3 of the replayed riders ARE the
    recording, their sums exactly (0, 0), the rest matches the general-path twin that pushes the recording after every tick (2e-5)"""
    job = _hook_job()
    sets = job["sets"]
    e = _hook_engine(job)
    _, rec = e.scene_calib_eval_groups(sets[2:3], states=True)        # the recording: candidate 2, nobody replayed
    assert np.isfinite(rec).all()
    mask = (HOOK_GROUP == 2) | (HOOK_GROUP == 3)
    e.scene_calib_replay(mask, rec[:, mask, :4])
    sums, states = e.scene_calib_eval_groups(sets[:2], states=True)
    per = [(job["s0"], job["off"], job["dq"])]
    _against_twins(states, sets[:2], per, [HOOK_GROUP], [T], np.array([0, 8]), "replay", replayed=[mask], rec=[rec])
    for k in range(2):
        assert np.array_equal(states[:, k * 8: (k + 1) * 8][:, mask, :4], rec[:, mask, :4]), k
    assert np.all(sums[:, mask] == 0.0) and np.all(sums[:, ~mask] > 0.0)
    e.close()


def test_mixed_classes_with_presence_windows():
    """for ticks 0 - 11 no Bicycle is present (the ballot skips group 0), an InvPendulum enters at tick 7 and the TwoD leaves at 30:
    against the general-path twin whose riders join by add_agents + set_agent_class and leave by remove_agents (2e-5 on the present
    cells; absent cells are NaN in the twin and not compared)"""
    job = _hook_job()
    enter = np.where(HOOK_GROUP == 0, 12, 0)
    enter[1] = 7
    exit_ = np.full(8, T)
    exit_[3] = 30
    e = _hook_engine(job)
    e.scene_calib_windows(enter.astype(np.int32), exit_.astype(np.int32))
    sums, states = e.scene_calib_eval_groups(job["sets"], states=True)
    per = [(job["s0"], job["off"], job["dq"])]
    _against_twins(states, job["sets"], per, [HOOK_GROUP], [T], np.array([0, 8]), "windows", enter=[enter], exit=[exit_])
    sums2, states2 = e.scene_calib_eval_groups(job["sets"], states=True)
    assert np.array_equal(sums, sums2) and np.array_equal(states, states2)
    e.close()


def test_mixed_classes_with_road_edges_and_road_parameters_per_candidate():
    """two polylines beside the box, F_0 and sigma of all vertices replaced per candidate (an integer sigma and a fractional one):
    against the general-path twin with that road set by set_road (2e-5)"""
    job = _hook_job()
    f0s, sgs = np.array([0.4, 0.9, 0.2]), np.array([2.0, 3.0, 2.5])
    lines = [np.c_[np.linspace(-20.0, HOOK_BOX + 20.0, c), np.full(c, y)] for c, y in ((40, -3.0), (23, HOOK_BOX + 3.0))]
    roff = np.array([0, 40, 63], dtype=np.int64)
    e = _hook_engine(job)
    e.scene_calib_road(np.array([0, 0], dtype=np.int32), roff, np.concatenate(lines), 0.3, 2.0)
    sums, states = e.scene_calib_eval_groups(job["sets"], road_F0=f0s, road_sigma=sgs, states=True)
    worst = 0.0
    for k, pods in enumerate(job["sets"]):
        tw = general_twin(pods, HOOK_GROUP, job["s0"], job["off"], job["dq"], T, road=(roff, np.concatenate(lines), np.full(2, f0s[k]), np.full(2, sgs[k])))
        d = float(np.abs(states[:, k * 8: (k + 1) * 8] - tw).max())
        worst = max(worst, d)
        assert d < GENERAL_TOL, (k, d)
    print(f"road: largest |scene_calib_eval_groups - general-path twin| = {worst:.3e} (bound {GENERAL_TOL:g})")
    sums2 = e.scene_calib_eval_groups(job["sets"][::-1], road_F0=f0s[::-1], road_sigma=sgs[::-1])
    assert np.array_equal(sums2[::-1], sums)
    e.close()


def test_two_classes_f_0_are_recovered_from_leave_one_out_scenes():
    """InteractionCalibration(vehicle_type=[TwoDBicycle, InvPendulumBicycle]), true f_0 of 1.0 x and 1.6 x the default: 12 leave-one-out
    scenes (ego_split of three recorded scenes of 4 riders, 60 ticks), fitting (("f_0", 0), ("f_0", 1)) from a guess 20 % off with the
    settings of tests/test_gpu_scene_groups.py::test_two_groups_f_0_are_recovered_from_leave_one_out_scenes: theta within 1e-4 of theta*"""
    from cyclistsocialforce_amd import calibration as cal, parameters, vehicle
    base = parameters.default_pod("twod")
    true = np.array([base.f_0, 1.6 * base.f_0])
    grp = np.array([0, 1, 0, 1], dtype=np.uint8)
    types = [vehicle.TwoDBicycle, vehicle.InvPendulumBicycle]
    data = []
    for seed in (1230, 1222, 1224):
        x, y, psi, v, off, dq = crowd(4, seed=seed, box=8.0)
        s0 = wide_state(x, y, psi, v)
        pods = (parameters.default_pod("twod", f_0=true[0]), parameters.default_pod("invpend", f_0=true[1]))
        e = _engine(pods[0], 4)
        e.scene_calib_load([4], s0, VDES, off, dq, np.zeros((60, 4, 2)), [0, 1], max_sets=1)
        e.scene_calib_classes(grp, [p.model for p in pods], s0)
        _, traj = e.scene_calib_eval_groups([pods], states=True)
        e.close()
        data += cal.SceneData(s0, VDES, off, dq, traj[:, :, :4], group=grp).ego_split()
    assert len(data) == 12
    c = cal.InteractionCalibration(types, [("f_0", 0), ("f_0", 1)], data, data, [1, 1, 0, 0, 0, 0], max_sets=8, maxiter=400, xtol=1e-4, ftol=1e-30)
    guess = true * np.array([1.2, 0.8])
    f_start = float(c.evaluate([guess])[0])
    res = c.run(guess)
    print(f"recovered f_0 = {res[0]} (true {true}), objective {res[1]:.3e} from {f_start:.3e}, {res[2]} iterations")
    assert np.abs(res[0] - true).max() < 1e-4
    c.close()


def test_refusals_in_a_fresh_process():
    """tests/scene_mixed_abi_child.py: every refusal of csf_scene_calib_classes and of the evaluation with classes loaded, each followed by
    an array_equal evaluation, a shared and a wide load, and the engine after csf_scene_calib_clear"""
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, os.path.join(here, "scene_mixed_abi_child.py")], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stderr[-3000:]
    assert "scene_mixed_abi_child: ok" in out.stdout
