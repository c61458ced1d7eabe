"""Calibration on closed-loop scenes, host side (no GPU): the entry points are declared, exported and bound; InteractionCalibration
groups its vectors into launches of max_sets and forms both error functions from per-rider sums in a fixed order; run_many is
minimize_many; SceneData validates its arrays; the oracle is not chaotic on the horizon tests/test_gpu_scene_calib.py compares on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cyclistsocialforce_amd import _ffi, calibration as cal, vehicle
from cyclistsocialforce_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("csf_scene_calib_load", "csf_scene_calib_eval", "csf_scene_calib_launches", "csf_scene_calib_clear")


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "csf.h")).read()
    declared = set(re.findall(r"\b(csf_[a-z_0-9]+)\s*\(", header))
    lib = _ffi.load()
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    for s in NEW:
        assert s in declared and s in _ffi.SYMBOLS and hasattr(lib, s), s
        assert getattr(lib, s).restype in (C.c_int, C.c_int32), s
    assert lib.csf_abi_version() == 9 and _ffi.ABI_VERSION == 9
    assert lib.csf_scene_calib_load.argtypes == [vp, i32, vp, i64, vp, vp, vp, vp, vp, vp, i32, vp, i32]
    assert lib.csf_scene_calib_eval.argtypes == [vp, i32, C.POINTER(_ffi.Params), C.c_size_t, i32, vp, i32, vp]
    assert lib.csf_scene_calib_launches.argtypes == [vp, C.POINTER(i64)]
    assert lib.csf_scene_calib_clear.argtypes == [vp]
    n = C.c_int64(5)
    assert lib.csf_scene_calib_launches(None, C.byref(n)) == -1 and n.value == 5
    assert lib.csf_scene_calib_clear(None) == -1
    pod = _ffi.Params()
    p = np.zeros(8).ctypes.data_as(vp)
    assert lib.csf_scene_calib_eval(None, 1, C.byref(pod), C.sizeof(pod), 9, p, 1, None) == -1
    for m in ("scene_calib_load", "scene_calib_eval", "scene_calib_clear", "scene_calib_launches"):
        assert callable(getattr(Engine, m)), m


def _scene(rng, n, ticks, cols=4, length=None):
    s0 = rng.normal(size=(n, 5))
    dq = rng.normal(size=(2 * n, 3))
    return cal.SceneData(s0, 5.0, np.arange(n + 1) * 2, dq, rng.normal(size=(ticks, n, cols)), length=length)


def _bowl(p):
    return (p.f_0 - 4.0) ** 2 + 100.0 * (p.sigma_0 - 0.6) ** 2 + 1.0


class StubEngine:
    """what InteractionCalibration asks of an engine: the sums of a call are a known function of the set and the rider"""
    made = []

    def __init__(self, pod, capacity, device=0):
        self.capacity, self.calls, self.closed = capacity, [], False
        StubEngine.made.append(self)

    def scene_calib_load(self, nr, s0, vd, off, rows, obj, feat, lengths=None, max_sets=256):
        self.nr, self.R, self.T, self.lengths, self.max_sets, self.obj, self.off, self.rows = np.asarray(nr), s0.shape[0], obj.shape[0], lengths, max_sets, obj, off, rows

    def scene_calib_eval(self, pods, states=False, stride=1):
        assert 1 <= len(pods) <= self.max_sets
        self.calls.append(len(pods))
        r = np.arange(self.R)
        sums = np.zeros((len(pods), self.R, 2))
        for k, p in enumerate(pods):
            sums[k, :, 0] = _bowl(p) * 10.0 ** (r % 7 - 3) / 3.0       # (magnitudes that make the order of a sum visible)
            sums[k, :, 1] = _bowl(p) * 10.0 ** (-(r % 5)) / 7.0
        if not states:
            return sums
        st = np.zeros((self.T // stride, len(pods) * self.R, 5))
        for k, p in enumerate(pods):
            st[:, k * self.R: (k + 1) * self.R, 0] = p.f_0
        return sums, st

    def close(self):
        self.closed = True


def _calibration(data, error_func, max_sets=4, **kw):
    return cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0", "sigma_0"], data, data, [1, 1, 0, 0, 0, 0], error_func=error_func,
                                      max_sets=max_sets, engine_factory=StubEngine, **kw)


def test_evaluate_groups_vectors_into_launches_and_forms_both_errors_in_a_fixed_order():
    rng = np.random.default_rng(2)
    data = [_scene(rng, 3, 40), _scene(rng, 7, 25, length=20), _scene(rng, 1, 40)]
    theta = np.c_[rng.uniform(1, 9, 11), rng.uniform(0.3, 0.9, 11)]
    nr, lens, nf = np.array([3, 7, 1]), np.array([40, 20, 40]), 2
    roff = np.r_[0, np.cumsum(nr)]
    for func in (cal.calc_sse_timesteps, cal.calc_maesse_samples):
        StubEngine.made.clear()
        c = _calibration(data, func)
        err = c.evaluate(theta)
        eng, = StubEngine.made
        assert eng.calls == [4, 4, 3] and eng.capacity == 4 * 11 and eng.max_sets == 4
        assert np.array_equal(eng.nr, nr) and np.array_equal(eng.lengths, lens) and eng.obj.shape == (40, 11, 2)
        assert np.array_equal(eng.obj[:25, 3:10], data[1].traj[:, :, :2]) and np.all(eng.obj[25:, 3:10] == 0.0)
        assert np.array_equal(eng.off, np.arange(12) * 2) and eng.rows.shape == (22, 3)
        r = np.arange(11)
        for k, (f0, sg) in enumerate(theta):
            pod = c._pod({"f_0": f0, "sigma_0": sg})
            per = _bowl(pod) * 10.0 ** (r % 7 - 3) / 3.0 if func is cal.calc_sse_timesteps else _bowl(pod) * 10.0 ** (-(r % 5)) / 7.0
            total = 0.0
            for q in range(3):                                   # riders in rider order, then scenes in scene order
                acc = 0.0
                for i in range(roff[q], roff[q + 1]):
                    acc += per[i]
                total += acc if func is cal.calc_sse_timesteps else (acc / (lens[q] * nr[q] * float(nf))) ** 2
            assert err[k] == total, (func.__name__, k)
        c.close()
        assert eng.closed
    # another error function gets the trajectories per scene, [length, n_riders, n_feat]
    seen = []

    def custom(outs, objs):
        seen.append(([o.shape for o in outs], [o.shape for o in objs]))
        return float(outs[0][0, 0, 0])

    c = _calibration(data, custom, max_sets=8)
    err = c.evaluate(theta[:3])
    assert seen[0] == ([(40, 3, 2), (20, 7, 2), (40, 1, 2)],) * 2 and np.array_equal(err, [c._pod({"f_0": f}).f_0 for f in theta[:3, 0]])
    trajs, objectives = c.simulate(theta[0])
    assert [t.shape for t in trajs] == [(40, 3, 2), (20, 7, 2), (40, 1, 2)] and np.array_equal(objectives[1], data[1].traj[:20, :, :2])


def test_run_many_equals_minimize_many_on_the_same_function():
    rng = np.random.default_rng(4)
    c = _calibration([_scene(rng, 2, 10)], cal.calc_sse_timesteps, max_sets=3, maxiter=40)
    guesses = [np.array([5.0, 0.5]), np.array([2.0, 0.8])]
    res = c.run_many(guesses)
    want = cal.minimize_many(c.evaluate, guesses, maxiter=40)
    for (x, f, n), (x1, f1, n1) in zip(res, want):
        assert np.array_equal(x, x1) and f == f1 and n == n1
    best = min(res, key=lambda r: r[1])
    assert c.param_args_opt == {"f_0": best[0][0], "sigma_0": best[0][1]}
    assert all(k <= 3 for k in StubEngine.made[-1].calls)


def test_scene_data_validation():
    rng = np.random.default_rng(6)
    s0, dq, tr = rng.normal(size=(3, 5)), rng.normal(size=(6, 3)), rng.normal(size=(10, 3, 4))
    off = np.arange(4) * 2
    d = cal.SceneData(s0, [4.0, 5.0, 6.0], off, dq, tr)
    assert d.n == 3 and d.length == 10 and np.array_equal(d.v_desired, [4.0, 5.0, 6.0])
    assert cal.SceneData(s0, 5.0, off, dq, tr, length=0).length == 0
    bad = [dict(s0=s0[:, :3]), dict(s0=np.zeros((33, 5))), dict(s0=np.zeros((0, 5))), dict(v_desired=[1.0, 2.0]), dict(dest_offsets=[0, 2, 2, 6]),
           dict(dest_offsets=[0, 2, 4]), dict(dest_offsets=[0, 2, 4, 5]), dict(traj=tr[:, :2]), dict(traj=tr[0]), dict(traj=rng.normal(size=(10, 3, 7))),
           dict(length=11), dict(length=-1)]
    for kw in bad:
        args = dict(s0=s0, v_desired=5.0, dest_offsets=off, dest_xyz_stop=dq, traj=tr, length=None)
        args.update(kw)
        with pytest.raises(ValueError):
            cal.SceneData(**args)
    with pytest.raises(TypeError):
        cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0"], [tr], [], [1, 0, 0, 0, 0, 0])
    with pytest.raises(ValueError):                              # a feature the recorded trajectory lacks
        cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0"], [d], [d], [0, 0, 0, 0, 0, 1], engine_factory=StubEngine).evaluate([[7.0]])


def test_the_oracle_is_not_chaotic_on_the_horizon():
    """for every (scene, set) of test_gpu_scene_calib.py::test_scenes_against_the_oracle: an oracle run from start positions perturbed
    by 1e-7 m stays within 1e-5 x extent of the unperturbed one over the 200 ticks compared there"""
    from scene_calib_common import ORACLE_CASES, oracle_case, oracle_run
    rng = np.random.default_rng(7)
    worst = 0.0
    for m, n, rule, hfov in ORACLE_CASES:
        s0, off, dq, pods = oracle_case(m, n, rule, hfov)
        for k, pod in enumerate(pods):
            ref = oracle_run(pod, s0, off, dq)
            ext = max(np.ptp(ref[..., 0]), np.ptp(ref[..., 1]), 14.0)
            for _ in range(3):
                s1 = s0.copy()
                s1[:, :2] += 1e-7 * rng.choice([-1.0, 1.0], size=(n, 2))
                per = oracle_run(pod, s1, off, dq)
                dev = float(np.hypot(per[..., 0] - ref[..., 0], per[..., 1] - ref[..., 1]).max()) / ext
                worst = max(worst, dev)
                assert dev < 1e-5, (m, n, rule, hfov, k, dev)
    print(f"largest sensitivity of the oracle to 1e-7 m at the start: {worst:.2e} x extent")


def test_the_copied_scenes_are_those_of_the_small_crowd_test():
    """scene_calib_common.crowd is a deliberate copy of tests/test_gpu_small.py's (with the destinations' distances as a parameter)
    and ORACLE_CASES a transcription of that test's parametrisation: both are held to the original here, so neither drifts"""
    import test_gpu_small as orig
    from scene_calib_common import ORACLE_CASES, crowd
    for n, seed, box in ((1, 10, 14.0), (7, 70, 14.0), (17, 3, 22.0), (32, 321, 30.0)):
        for a, b in zip(crowd(n, seed, box), orig.crowd(n, seed, box)):
            assert np.array_equal(a, b)
    mark = [m for m in orig.test_small_crowds_vs_oracle.pytestmark if m.name == "parametrize"][0]
    held = ("twod", "invpend", "planarpoint", "bicycle")        # the classes that test holds to 1e-4 x extent over 400 free ticks
    assert ORACLE_CASES == [c for c in mark.args[1] if c[1] <= 8 and c[0] in held]
