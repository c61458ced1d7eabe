"""Several simulated vehicle classes in one scene of a closed-loop calibration, host side (no GPU):
InteractionCalibration(vehicle_type=[...]) through a fake engine - the records per group, their classes and values, the calls made, the
ValueErrors -, the entry point declared, exported and bound, the recorded resource listing, and - with the CPU oracle - the seed choices
of tests/test_gpu_scene_mixed.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cyclistsocialforce_amd import _ffi, calibration as cal, vehicle
from cyclistsocialforce_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "csf.h")).read()
    declared = set(re.findall(r"\b(csf_[a-z_0-9]+)\s*\(", header))
    lib = _ffi.load()                                                # (the gfx950 library is built and loads)
    name = "csf_scene_calib_classes"
    assert name in declared and name in _ffi.SYMBOLS and hasattr(lib, name)
    assert lib.csf_scene_calib_classes.restype in (C.c_int, C.c_int32)
    assert lib.csf_scene_calib_classes.argtypes == [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    assert lib.csf_scene_calib_classes(None, None, 0, None, None) == -1
    assert lib.csf_abi_version() == 9 and _ffi.ABI_VERSION == 9      # (csf_params and the ABI version do not change)
    assert callable(Engine.scene_calib_classes)
    assert re.search(r"int csf_scene_calib_classes\(csf_engine \*e, const uint8_t \*group, int32_t n_groups, const int32_t \*models, const double \*s0\);", header)


def test_the_resource_listing_is_recorded():
    text = open(os.path.join(ROOT, "profiles", "scene_mixed_resource_usage.txt")).read()
    m = re.search(r"Existing kernel instances: (\d+); identical[^:]*: (\d+); changed: (\d+); gone: (\d+)", text)
    assert m and int(m.group(1)) == int(m.group(2)) > 0 and int(m.group(3)) == 0 and int(m.group(4)) == 0
    for win in (0, 1):
        assert f"scene_mixed_kernelILb{win}E" in text


def _arrays(rng, n, ticks, cols=4):
    return rng.normal(size=(n, 5)), np.arange(n + 1) * 2, rng.normal(size=(2 * n, 3)), rng.normal(size=(ticks, n, cols))


class FakeEngine:
    """what InteractionCalibration asks of an engine (tests/test_scene_groups_host.py), with classes: it notes every call, and the sums
    of a rider are a known function of ITS GROUP's record"""
    made = []

    def __init__(self, pod, capacity, device=0):
        self.pod, self.capacity, self.log, self.group, self.models, self.s0c, self.mask = pod, capacity, [], None, None, None, None
        FakeEngine.made.append(self)

    def scene_calib_load(self, nr, s0, vd, off, rows, obj, feat, lengths=None, max_sets=256):
        self.log.append("load")
        self.R, self.T = s0.shape[0], obj.shape[0]

    def scene_calib_load_shared(self, *a, **kw):
        raise AssertionError("a mixed data set is never loaded on shared lanes")

    scene_calib_load_wide = scene_calib_load_shared

    def scene_calib_classes(self, group, models=None, s0=None):
        self.log.append("classes")
        self.group, self.models, self.s0c = np.array(group), list(models), np.array(s0)

    def scene_calib_groups(self, group, n_groups=None):
        self.log.append("groups")
        self.group = np.array(group)

    def scene_calib_replay(self, replayed, rows=None):
        self.log.append("replay")
        self.mask = np.array(replayed, dtype=bool)

    def scene_calib_windows(self, enter, exit):
        self.log.append("windows")

    def scene_calib_road(self, *a):
        self.log.append("road")

    def scene_calib_eval(self, pods, states=False, stride=1, **kw):
        self.log.append("eval")
        return self.scene_calib_eval_groups([(p,) for p in pods], states=states, stride=stride, _plain=True, **kw)

    def scene_calib_eval_groups(self, pods, road_F0=None, road_sigma=None, states=False, stride=1, _plain=False):
        if not _plain:
            self.log.append("eval_groups")
        self.last, self.road = pods, (road_F0, road_sigma)
        grp = np.zeros(self.R, dtype=int) if self.group is None else self.group
        sim = np.ones(self.R, dtype=bool) if self.mask is None else ~self.mask
        r = np.arange(self.R)
        sums = np.zeros((len(pods), self.R, 2))
        st = np.zeros((self.T // stride, len(pods) * self.R, 8))
        for k, tup in enumerate(pods):
            f = np.array([tup[g].f_0 + 10.0 * tup[g].model for g in grp])
            sums[k, :, 0] = sim * f * (1.0 + r)
            sums[k, :, 1] = sim * f / (1.0 + r)
            st[:, k * self.R: (k + 1) * self.R, 0] = f + r[None, :]
        return (sums, st) if states else sums

    def close(self):
        pass


TYPES = [vehicle.TwoDBicycle, vehicle.Bicycle, vehicle.BalancingRiderBicycle]


def _data(rng, **kw):
    def scene(n, ticks, grp, mask=None, length=None, **more):
        s0, off, dq, tr = _arrays(rng, n, ticks)
        return cal.SceneData(s0, 5.0, off, dq, tr, length=length, replayed=mask, group=grp, **more)
    return [scene(3, 40, [0, 1, 2], **kw), scene(6, 25, [1, 0, 0, 2, 1, 0], mask=[0, 0, 1, 0, 0, 0], length=20), scene(2, 40, None)]


def _calibration(data, keys, error_func=cal.calc_sse_timesteps, types=TYPES, **kw):
    return cal.InteractionCalibration(types, keys, data, data, [1, 1, 0, 0, 0, 0], error_func=error_func, max_sets=4, engine_factory=FakeEngine, **kw)


def test_a_candidate_becomes_one_record_per_group_of_the_groups_class():
    rng = np.random.default_rng(41)
    data = _data(rng)
    gp = [dict(hfov=2.0), dict(hfov=3.0, p_0=33.0), {}]
    c = _calibration(data, ["sigma_0", ("f_0", 1), ("f_0", 0), ("p_decay", 1)], group_params=gp)
    args = c._update_params_args_dict([0.55, 7.0, 3.0, 4.5])
    p0, p1, p2 = c._pods(args)
    assert [p.model for p in (p0, p1, p2)] == [_ffi.TWOD, _ffi.BICYCLE, _ffi.BALANCINGRIDER]
    for p, t in zip((p0, p1, p2), TYPES):                         # a record is its class's PARAMS_TYPE(...).to_pod(MODEL)
        assert bytes(p)[-16:] == bytes(t.PARAMS_TYPE().to_pod(t.MODEL))[-16:]
    assert p0.sigma_0 == p1.sigma_0 == p2.sigma_0 == 0.55          # a shared key reaches all groups
    assert p0.f_0 == 3.0 and p1.f_0 == 7.0 and p2.f_0 == TYPES[2].PARAMS_TYPE().to_pod(_ffi.BALANCINGRIDER).f_0   # ("f_0", g): group g only
    assert p1.p_decay == 4.5 and p1.p_0 == 33.0 and p0.hfov == 2.0 and p1.hfov == 3.0   # group_params stay fixed
    FakeEngine.made.clear()
    err = c.evaluate([[0.55, 7.0, 3.0, 4.5]])
    eng, = FakeEngine.made
    assert eng.log == ["load", "classes", "replay", "eval_groups"]   # scene_calib_load, then scene_calib_classes; no scene_calib_groups
    assert eng.models == [_ffi.TWOD, _ffi.BICYCLE, _ffi.BALANCINGRIDER]
    assert np.array_equal(eng.group, [0, 1, 2, 1, 0, 0, 2, 1, 0, 0, 0])
    assert eng.s0c.shape == (11, 8) and np.array_equal(eng.s0c[:3, :5], data[0].s0) and np.all(eng.s0c[:, 5:] == 0.0)   # the widest layout
    assert eng.pod.model == _ffi.TWOD and eng.pod.hfov == 2.0     # the engine is created with group 0's record
    assert eng.capacity == 4 * 11
    (l0, l1, l2), = eng.last
    assert bytes(l0) == bytes(p0) and bytes(l1) == bytes(p1) and bytes(l2) == bytes(p2)
    f = np.array([(p0, p1, p2)[g].f_0 + 10.0 * (p0, p1, p2)[g].model for g in eng.group])
    per = f * (1.0 + np.arange(11)) * ~eng.mask
    assert err[0] == (per[0] + per[1] + per[2]) + sum(per[3:9]) + (per[9] + per[10])
    # the default group_params: G empty dicts; a custom error_func and simulate get the trajectories per scene
    seen = []
    c2 = _calibration(data, ["f_0"], error_func=lambda outs, objs: seen.append(outs) or 1.5)
    assert c2.group_params == [{}, {}, {}] and c2.evaluate([[2.0]])[0] == 1.5
    assert [o.shape for o in seen[0]] == [(40, 3, 2), (20, 5, 2), (40, 2, 2)]
    trajs, objectives = c2.simulate([2.0])
    assert [t.shape for t in trajs] == [(40, 3, 2), (20, 5, 2), (40, 2, 2)] and len(objectives) == 3
    c2.param_args_opt = c2._update_params_args_dict([2.0])
    assert c2.test() == float(c2.evaluate([[2.0]], test=True)[0])
    m = _calibration(data, ["f_0"], error_func=cal.calc_maesse_samples)
    assert np.isfinite(m.evaluate([[2.0], [3.0]])).all()


def test_windows_roads_and_road_keys_go_with_the_classes():
    rng = np.random.default_rng(42)
    road = (np.array([0, 4]), rng.normal(size=(4, 2)), 0.3, 2.0)
    data = _data(rng, road=road, present=([0, 2, 0], [40, 40, 30]))
    FakeEngine.made.clear()
    c = _calibration(data, ["f_0", "road_F_0"])
    c.evaluate([[2.0, 0.7]])
    eng, = FakeEngine.made
    assert eng.log == ["load", "classes", "replay", "road", "windows", "eval_groups"]
    assert np.array_equal(eng.road[0], [0.7]) and all(p.f_0 == 2.0 for p in eng.last[0])


def test_the_value_errors():
    rng = np.random.default_rng(43)
    s0, off, dq, tr = _arrays(rng, 3, 10)
    ok = cal.SceneData(s0, 5.0, off, dq, tr, group=[0, 1, 2])
    with pytest.raises(ValueError, match="group_params"):          # the length of group_params
        _calibration([ok], ["f_0"], group_params=[{}, {}])
    thirteen = [vehicle.TwoDBicycle] * 13
    with pytest.raises(ValueError, match="2 .. 12"):               # the limit of 12 ...
        _calibration([ok], ["f_0"], types=thirteen)
    twelve = _calibration([ok], ["f_0", ("f_0", 11)], types=[vehicle.TwoDBicycle] * 12)   # ... which is reached
    assert len(twelve._pods({"f_0": 2.0, ("f_0", 11): 3.0})) == 12
    with pytest.raises(ValueError, match="2 .. 12"):
        _calibration([ok], ["f_0"], types=[vehicle.TwoDBicycle])
    with pytest.raises(ValueError, match="six simulated"):
        _calibration([ok], ["f_0"], types=[vehicle.TwoDBicycle, vehicle.UncontrolledVehicle, vehicle.Bicycle])
    # a shared key that a class lacks: p_0 is a BicycleParameters's, not an InvPendulumBicycleParameters's (the TwoDBicycle's)
    with pytest.raises(ValueError, match=r"'p_0'.*InvPendulumBicycleParameters.*group 0"):
        _calibration([ok], ["p_0"])
    with pytest.raises(ValueError, match=r"v_max_walk.*group 1"):
        _calibration([ok], [("v_max_walk", 1)])
    assert _calibration([ok], [("v_max_walk", 0)])._pods({("v_max_walk", 0): 1.25})[0].v_max_walk == 1.25
    with pytest.raises(ValueError, match="group 1"):               # ... and in group_params: the constructor's TypeError, as a ValueError
        _calibration([ok], ["f_0"], group_params=[{}, dict(v_max_walk=3.0), {}])._pods({"f_0": 1.0})
    with pytest.raises(ValueError, match="params_keys"):
        _calibration([ok], [("f_0", 3)])
    with pytest.raises(ValueError, match="scene 0 of train_data"):  # a group nobody gave a class
        _calibration([cal.SceneData(s0, 5.0, off, dq, tr, group=[0, 3, 0])], ["f_0"])
    # shared lanes or a wide scene: refused when the data set is loaded, before an engine is made
    n = 40
    big = cal.SceneData(rng.normal(size=(n, 5)), 5.0, np.arange(n + 1), rng.normal(size=(n, 3)), rng.normal(size=(10, n, 4)),
                        present=(np.arange(n) % 2 * 5, np.arange(n) % 2 * 5 + 5), group=np.arange(n) % 3)
    wide = cal.SceneData(s0, 5.0, off, dq, tr, group=[0, 1, 2], wide=True)
    for data, kw in (([big], {}), ([wide], {}), ([ok], dict(share_lanes=True)), ([ok], dict(share_lanes=True, lane_groups=True))):
        FakeEngine.made.clear()
        c = _calibration(data, ["f_0"], **kw)
        with pytest.raises(ValueError, match="mixed classes run on Engine.scene_calib_load only"):
            c.evaluate([[2.0]])
        assert not FakeEngine.made


def test_a_single_vehicle_type_makes_the_calls_it_makes_today():
    rng = np.random.default_rng(44)
    s0, off, dq, tr = _arrays(rng, 3, 10)
    plain = cal.SceneData(s0, 5.0, off, dq, tr)
    FakeEngine.made.clear()
    c = cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0", "sigma_0"], [plain, plain], [plain], [1, 1, 0, 0, 0, 0], engine_factory=FakeEngine)
    c.evaluate([[2.0, 0.5]])
    assert FakeEngine.made[-1].log == ["load", "eval"]
    grouped = cal.SceneData(s0, 5.0, off, dq, tr, group=[0, 1, 0])
    c = cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0"], [grouped], [grouped], [1, 1, 0, 0, 0, 0], engine_factory=FakeEngine, group_params=[{}, {}])
    c.evaluate([[2.0]])
    assert FakeEngine.made[-1].log == ["load", "groups", "eval_groups"]
    for gp in ([], [{}] * 5):                                     # the limit of 4 and its message stay
        with pytest.raises(ValueError, match="1 .. 4 dicts"):
            cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0"], [grouped], [grouped], [1, 1, 0, 0, 0, 0], engine_factory=FakeEngine, group_params=gp)


def _sensitivity(pods, grp, s0, off, dq, ticks, rng, rows, stride=1):
    from scene_mixed_common import oracle_mixed_run
    ref = oracle_mixed_run(pods, grp, s0, off, dq, ticks, stride=stride, rows=rows)
    assert np.isfinite(ref).all()
    worst = 0.0
    for _ in range(2):
        s1 = s0.copy()
        s1[:, :2] += 1e-7 * rng.choice([-1.0, 1.0], size=(s0.shape[0], 2))
        worst = max(worst, float(np.abs(oracle_mixed_run(pods, grp, s1, off, dq, ticks, stride=stride, rows=rows) - ref).max()))
    return worst, ref


def test_the_mixed_oracle_is_not_chaotic_on_the_scenes():
    """the choice of scene_mixed_common.SEEDS (and of the hook scene of tests/test_gpu_scene_mixed.py), by the CPU oracle: for every scene
    that has ticks and each of the three candidates an oracle run with one parameter set per group and class, started from positions
    perturbed by 1e-7 m (two random sign patterns), stays within 2e-6 - a tenth of GENERAL_TOL - of the unperturbed one on EVERY state
    row over the scene's ticks.  Measured: at most 6.0e-7 (the scene of 32)."""
    from scene_mixed_common import GROUPS, LENGTHS, mixed_scenes, mixed_sets
    rng = np.random.default_rng(7)
    sets = mixed_sets()
    _, _, _, per = mixed_scenes()
    worst = 0.0
    for q, (s0, off, dq) in enumerate(per):
        if LENGTHS[q] == 0:
            continue
        for pods in sets:
            w, _ = _sensitivity(pods, GROUPS[q], s0, off, dq, int(LENGTHS[q]), rng, 8)
            worst = max(worst, w)
            assert w < 2e-6, (q, w)
    from scene_calib_common import crowd
    from scene_mixed_common import HOOK_BOX, HOOK_CLASSES, HOOK_GROUP, HOOK_SEED, wide_state
    x, y, psi, v, off, dq = crowd(8, seed=HOOK_SEED, box=HOOK_BOX)
    for pods in mixed_sets(3, HOOK_CLASSES):
        w, _ = _sensitivity(pods, HOOK_GROUP, wide_state(x, y, psi, v), off, dq, 40, rng, 8)
        worst = max(worst, w)
        assert w < 2e-6, ("hooks", w)
    print(f"largest sensitivity of the mixed oracle to 1e-7 m at the start, all state rows: {worst:.2e}")


def test_the_mixed_oracle_is_not_chaotic_on_the_horizon():
    """the case of tests/test_gpu_scene_mixed.py::test_mixed_scene_against_the_oracle: both priority rules, three candidates, 200 ticks:
    within 1e-5 x extent of the unperturbed run - a tenth of that test's bound.  Measured: 2.5e-8 x extent."""
    from scene_mixed_common import ORACLE_GROUP, ORACLE_TICKS, oracle_case
    rng = np.random.default_rng(7)
    worst = 0.0
    for rule in (0, 1):
        s0, off, dq, pods = oracle_case(rule)
        for pd in pods:
            w, ref = _sensitivity(pd, ORACLE_GROUP, s0, off, dq, ORACLE_TICKS, rng, 2, stride=10)
            ext = max(np.ptp(ref[..., 0]), np.ptp(ref[..., 1]), 14.0)
            worst = max(worst, w / ext)
            assert w / ext < 1e-5, (rule, w / ext)
    print(f"largest sensitivity of the mixed oracle case: {worst:.2e} x extent")


def test_the_classes_act_on_the_seeded_scene():
    """the choice of scene_mixed_common.ACT_SEED, by the CPU oracle: swapping which of the two riders is the Bicycle moves BOTH by more
    than ten times ACT_MOVED within ACT_TICKS (found: 0.15 m and 0.73 m)"""
    from scene_mixed_common import ACT_MOVED, ACT_TICKS, act_pods, act_scene, oracle_mixed_run
    s0, off, dq = act_scene()
    tw, bi = act_pods()
    a = oracle_mixed_run((tw, bi), [0, 1], s0, off, dq, ACT_TICKS)
    b = oracle_mixed_run((tw, bi), [1, 0], s0, off, dq, ACT_TICKS)
    moved = np.abs(a - b).max(axis=(0, 2))
    print(f"the classes act on the oracle: {moved} m")
    assert np.all(moved > 10.0 * ACT_MOVED)
