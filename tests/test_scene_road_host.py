"""Scenes with road edges, host side (no GPU): the two entry points are declared, exported and bound; SceneData validates a road
against the limits of the one-wave tick and ego_split keeps it; InteractionCalibration loads the roads and routes "road_F_0" /
"road_sigma" to the overrides of an evaluation; and on the CPU oracle the roads of tests/test_gpu_scene_road.py act, and its oracle
cases are not chaotic on the horizon compared."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scene_road_common as rc
from cyclistsocialforce_amd import _ffi, calibration as cal, parameters, vehicle
from cyclistsocialforce_amd.engine import Engine
from scene_calib_common import MODELS, oracle_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("csf_scene_calib_road", "csf_scene_calib_eval_road")


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "csf.h")).read()
    declared = set(re.findall(r"\b(csf_[a-z_0-9]+)\s*\(", header))
    lib = _ffi.load()
    vp, i32 = C.c_void_p, C.c_int32
    for s in NEW:
        assert s in declared and s in _ffi.SYMBOLS and hasattr(lib, s), s
        assert getattr(lib, s).restype in (C.c_int, C.c_int32), s
    assert lib.csf_abi_version() == 9 and _ffi.ABI_VERSION == 9
    assert lib.csf_scene_calib_road.argtypes == [vp, i32, vp, vp, vp, vp, vp]
    assert lib.csf_scene_calib_eval_road.argtypes == [vp, i32, C.POINTER(_ffi.Params), C.c_size_t, i32, vp, vp, vp, i32, vp]
    assert lib.csf_scene_calib_road(None, 0, None, None, None, None, None) == -1
    pod = _ffi.Params()
    p = np.zeros(8).ctypes.data_as(vp)
    assert lib.csf_scene_calib_eval_road(None, 1, C.byref(pod), C.sizeof(pod), 9, None, None, p, 1, None) == -1
    assert callable(Engine.scene_calib_road)
    import cyclistsocialforce_amd
    import importlib.util
    spec = importlib.util.spec_from_file_location("compat_calibration", os.path.join(ROOT, "compat", "cyclistsocialforce", "calibration.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.SceneData is cal.SceneData and mod.InteractionCalibration is cal.InteractionCalibration and cyclistsocialforce_amd is not None


def _road(nv, edges=1, f0=0.1, sigma=2.0):
    per = nv // edges
    counts = [per] * (edges - 1) + [nv - per * (edges - 1)]
    verts = np.c_[np.linspace(-5.0, 20.0, nv), np.full(nv, -3.0)]
    return np.r_[0, np.cumsum(counts)], verts, np.full(edges, f0), np.full(edges, sigma)


def _scene(rng, n, ticks=10, road=None, replayed=None):
    s0 = rng.normal(size=(n, 5))
    return cal.SceneData(s0, 5.0, np.arange(n + 1) * 2, rng.normal(size=(2 * n, 3)), rng.normal(size=(ticks, n, 4)), replayed=replayed, road=road)


def test_scene_data_validates_its_road_and_ego_split_keeps_it():
    rng = np.random.default_rng(1)
    assert _scene(rng, 3).road is None
    d = _scene(rng, 3, road=_road(100, edges=2, f0=[0.1, 0.2], sigma=[2.0, 2.5]))
    off, verts, F0, sg = d.road
    assert np.array_equal(off, [0, 50, 100]) and verts.shape == (100, 2) and np.array_equal(F0, [0.1, 0.2]) and np.array_equal(sg, [2.0, 2.5])
    assert np.array_equal(_scene(rng, 2, road=(np.array([0, 4]), np.zeros((4, 2)), 0.3, 3.0)).road[2], [0.3])     # scalars: every edge
    # the limits of the one-wave tick: 2 048 vertices, and nv_pad x P <= 16 384
    for n, most in ((1, 2048), (2, 2048), (5, 2048), (8, 2048), (9, 1024), (16, 1024), (17, 512), (32, 512)):
        assert _scene(rng, n, road=_road(most)).road[1].shape[0] == most
        with pytest.raises(ValueError):
            _scene(rng, n, road=_road(most + 1))
    assert _scene(rng, 32, road=_road(449)).road is not None      # 449 pads to 512
    bad_v = np.zeros((10, 2)); bad_v[3, 1] = np.nan
    for road in ((np.array([0, 5, 4]), np.zeros((10, 2)), 0.1, 2.0), (np.array([0, 11]), np.zeros((10, 2)), 0.1, 2.0), (np.array([-1, 4]), np.zeros((10, 2)), 0.1, 2.0),
                 (np.array([0, 10]), bad_v, 0.1, 2.0), (np.array([0, 10]), np.zeros((10, 2)), np.inf, 2.0), (np.array([0, 10]), np.zeros((10, 2)), 0.1, np.nan),
                 (np.array([0, 5, 10]), np.zeros((10, 2)), [0.1, 0.2, 0.3], 2.0), (np.array([0, 10]), np.zeros((10, 2))), 7):
        with pytest.raises(ValueError):
            _scene(rng, 3, road=road)
    bad_v[3, 1] = 0.0
    # ego_split carries the road along
    d = _scene(rng, 4, road=_road(70), replayed=[False, True, False, False])
    parts = d.ego_split()
    assert len(parts) == 3 and all(np.array_equal(a, b) for p in parts for a, b in zip(p.road, d.road))


def _bowl(p):
    return (p.f_0 - 4.0) ** 2 + 1.0


class StubEngine:
    """what InteractionCalibration asks of an engine; the sums of a call are a known function of the set and of its road overrides"""
    made = []

    def __init__(self, pod, capacity, device=0):
        self.calls, self.roads, self.closed = [], [], False
        StubEngine.made.append(self)

    def scene_calib_load(self, nr, s0, vd, off, rows, obj, feat, lengths=None, max_sets=256):
        self.R, self.T, self.max_sets = s0.shape[0], obj.shape[0], max_sets

    def scene_calib_road(self, edge_scene, offsets, verts, F0, sigma):
        self.roads.append((np.array(edge_scene), np.array(offsets), np.array(verts), np.array(F0), np.array(sigma)))

    def scene_calib_eval(self, pods, states=False, stride=1, road_F0=None, road_sigma=None):
        self.calls.append((len(pods), None if road_F0 is None else np.array(road_F0), None if road_sigma is None else np.array(road_sigma)))
        sums = np.zeros((len(pods), self.R, 2))
        for k, p in enumerate(pods):
            sums[k, :, 0] = _bowl(p) + (0.0 if road_F0 is None else 10.0 * road_F0[k] + 100.0 * road_sigma[k])
        return (sums, np.zeros((self.T // stride, len(pods) * self.R, 5))) if states else sums

    def close(self):
        self.closed = True


def _calibration(keys, data, test=None, **kw):
    return cal.InteractionCalibration(vehicle.TwoDBicycle, keys, data, data if test is None else test, [1, 1, 0, 0, 0, 0], max_sets=4,
                                      engine_factory=StubEngine, **kw)


def test_road_keys_are_routed_to_the_overrides_and_the_roads_are_loaded():
    rng = np.random.default_rng(2)
    r1, r2 = _road(70, edges=2, f0=[0.1, 0.2], sigma=[2.0, 3.0]), _road(10)
    data = [_scene(rng, 3, road=r1), _scene(rng, 2), _scene(rng, 4, road=r2)]
    default = parameters.RoadElementParameters()
    # both keys: neither reaches PARAMS_TYPE (which has no such field and would raise), both reach the evaluation, launch by launch
    StubEngine.made.clear()
    c = _calibration(["f_0", "road_F_0", "road_sigma"], data)
    theta = np.c_[rng.uniform(1, 9, 6), rng.uniform(0.01, 0.5, 6), rng.uniform(1.0, 4.0, 6)]
    err = c.evaluate(theta)
    eng, = StubEngine.made
    assert [n for n, _, _ in eng.calls] == [4, 2]
    assert np.array_equal(np.concatenate([f for _, f, _ in eng.calls]), theta[:, 1]) and np.array_equal(np.concatenate([s for _, _, s in eng.calls]), theta[:, 2])
    for k, (f0, rf, rs) in enumerate(theta):
        assert c._pod({"f_0": f0, "road_F_0": rf, "road_sigma": rs}).f_0 == f0
        per, total = _bowl(c._pod({"f_0": f0})) + (10.0 * rf + 100.0 * rs), 0.0
        for n in (3, 2, 4):                                      # riders in rider order, then scenes in scene order
            acc = 0.0
            for _ in range(n):
                acc += per
            total += acc
        assert err[k] == total
    # the roads went in with the data set: scene of every edge, CSR offsets over the concatenated vertices, per-edge parameters
    (es, off, verts, F0, sg), = eng.roads
    assert np.array_equal(es, [0, 0, 2]) and np.array_equal(off, [0, 35, 70, 80])
    assert np.array_equal(verts, np.r_[r1[1], r2[1]]) and np.array_equal(F0, [0.1, 0.2, 0.1]) and np.array_equal(sg, [2.0, 3.0, 2.0])
    trajs, _ = c.simulate(theta[0])
    assert eng.calls[-1][0] == 1 and eng.calls[-1][1][0] == theta[0, 1] and eng.calls[-1][2][0] == theta[0, 2]
    c.close()
    # one key: the other keeps its value from RoadElementParameters()
    StubEngine.made.clear()
    c = _calibration(["road_F_0"], data)
    c.evaluate([[0.3], [0.4]])
    (n, f, s), = StubEngine.made[0].calls
    assert n == 2 and np.array_equal(f, [0.3, 0.4]) and np.array_equal(s, [default.sigma] * 2)
    c = _calibration(["road_sigma", "f_0"], data)
    c.evaluate([[2.5, 7.0]])
    (n, f, s), = StubEngine.made[-1].calls
    assert np.array_equal(f, [default.F_0]) and np.array_equal(s, [2.5])
    # no road key: the evaluation is asked as before, without overrides
    c = _calibration(["f_0"], data)
    c.evaluate([[7.0]])
    assert StubEngine.made[-1].calls == [(1, None, None)] and len(StubEngine.made[-1].roads) == 1
    # no scene with a road: nothing is loaded
    c = _calibration(["f_0"], [_scene(rng, 3)])
    c.evaluate([[7.0]])
    assert StubEngine.made[-1].roads == []


def test_road_keys_without_a_scene_road_and_bad_values_raise():
    rng = np.random.default_rng(3)
    bare, roaded = [_scene(rng, 3), _scene(rng, 2)], [_scene(rng, 3, road=_road(20))]
    for keys in (["road_F_0"], ["f_0", "road_sigma"], ["road_F_0", "road_sigma"]):
        with pytest.raises(ValueError):
            _calibration(keys, bare)
        with pytest.raises(ValueError):
            _calibration(keys, roaded, test=bare)
        with pytest.raises(ValueError):                          # a road without a vertex is no road
            _calibration(keys, [_scene(rng, 3, road=(np.array([0, 0]), np.zeros((0, 2)), 0.1, 2.0))])
        _calibration(keys, roaded, test=[]).close()
    c = _calibration(["road_F_0"], roaded)
    with pytest.raises(ValueError):                              # RoadElementParameters: F_0 >= 0
        c.evaluate([[-0.1]])


def test_the_road_acts_on_the_oracle():
    """the margin of tests/test_gpu_scene_road.py::test_the_road_acts: on the CPU oracle every rider of every roaded scene, with every
    one of the 7 sets, ends at least 1e-4 m - 100 x the 1e-6 m asserted on the device - from where it ends without the road"""
    least = np.inf
    for model, rule in [(m, 0) for m in MODELS] + [("twod", 1)]:
        _, _, _, per = rc.scenes(model, rc.N_RIDERS, seed=MODELS.index(model), short=(rc.SHORT,))
        for k, pod in enumerate(rc.rule_sets(model, rule)):
            for q, (s0, off, dq) in enumerate(per):
                road = rc.road_of(model, q)
                if road is None:
                    continue
                ln = int(rc.LENGTHS[q])
                a = rc.oracle_road_run(pod, s0, off, dq, road, ln, stride=ln)[-1]
                b = rc.oracle_road_run(pod, s0, off, dq, None, ln, stride=ln)[-1]
                d = np.hypot(a[:, 0] - b[:, 0], a[:, 1] - b[:, 1])
                least = min(least, float(d.min()))
                assert np.isfinite(a).all() and np.all(d >= 1e-4), (model, rule, k, q, d.min())
    print(f"the least a road moves a rider on the oracle: {least:.3e} m")


def test_the_oracle_is_not_chaotic_between_the_road_edges():
    """for every (case, set) of tests/test_gpu_scene_road.py::test_roaded_scenes_against_the_oracle: an oracle run from start positions
    perturbed by 1e-7 m (three random sign patterns) stays within 1e-5 x extent of the unperturbed one over the 200 ticks compared"""
    rng = np.random.default_rng(7)
    road, worst = rc.oracle_road(), 0.0
    for m, n, rule, hfov in rc.ORACLE_ROAD_CASES:
        s0, off, dq, pods = oracle_case(m, n, rule, hfov)
        for k, pod in enumerate(pods):
            ref = rc.oracle_road_run(pod, s0, off, dq, road, rc.ORACLE_TICKS)
            bare = rc.oracle_road_run(pod, s0, off, dq, None, rc.ORACLE_TICKS)
            ext = max(np.ptp(ref[..., 0]), np.ptp(ref[..., 1]), 14.0)
            assert np.abs(ref - bare).max() > 1e-3 * ext, (m, n, k)             # the road is felt: 10 x the bar of the comparison
            for _ in range(3):
                s1 = s0.copy()
                s1[:, :2] += 1e-7 * rng.choice([-1.0, 1.0], size=(n, 2))
                per = rc.oracle_road_run(pod, s1, off, dq, road, rc.ORACLE_TICKS)
                dev = float(np.hypot(per[..., 0] - ref[..., 0], per[..., 1] - ref[..., 1]).max()) / ext
                worst = max(worst, dev)
                assert dev < 1e-5, (m, n, rule, k, dev)
    print(f"largest sensitivity of the oracle to 1e-7 m at the start, between the road edges: {worst:.2e} x extent")


def test_the_oracle_cases_are_cases_of_the_scene_calibration_suite():
    from scene_calib_common import ORACLE_CASES
    assert all(c in ORACLE_CASES and c[1] <= 8 for c in rc.ORACLE_ROAD_CASES)
    assert sorted(c[0] for c in rc.ORACLE_ROAD_CASES) == ["bicycle", "planarpoint", "twod"]
