"""Rider groups with candidate parameter sets of their own in a closed-loop calibration, host side (no GPU):
params_keys per group and the G parameter sets of a candidate, SceneData's groups and ego_split, both built-in errors and a custom one
through a fake engine, the ValueErrors, the two entry points declared, exported and bound, the recorded resource comparison, and -
with the CPU oracle - the sensitivity of the GPU test's oracle case and the seeds at which the groups act."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cyclistsocialforce_amd import _ffi, calibration as cal, vehicle
from cyclistsocialforce_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "csf.h")).read()
    declared = set(re.findall(r"\b(csf_[a-z_0-9]+)\s*\(", header))
    lib = _ffi.load()                                                # (the gfx950 library is built and loads)
    for name in ("csf_scene_calib_groups", "csf_scene_calib_eval_groups"):
        assert name in declared and name in _ffi.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).restype in (C.c_int, C.c_int32)
    assert lib.csf_scene_calib_groups.argtypes == [C.c_void_p, C.c_void_p, C.c_int32]
    assert lib.csf_scene_calib_eval_groups.argtypes == [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(_ffi.Params), C.c_size_t, C.c_int32,
                                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    assert lib.csf_scene_calib_groups(None, None, 2) == -1
    assert lib.csf_scene_calib_eval_groups(None, 1, 1, None, 0, 0, None, None, None, 1, None) == -1
    assert lib.csf_abi_version() == 9 and _ffi.ABI_VERSION == 9      # (csf_params and the ABI version do not change)
    assert callable(Engine.scene_calib_groups) and callable(Engine.scene_calib_eval_groups)


def test_the_resource_usage_comparison_is_recorded():
    text = open(os.path.join(ROOT, "profiles", "scene_groups_resource_usage.txt")).read()
    m = re.search(r"Existing kernel instances: (\d+); identical[^:]*: (\d+); changed: (\d+); gone: (\d+)", text)
    assert m and int(m.group(1)) == int(m.group(2)) > 0 and int(m.group(3)) == 0 and int(m.group(4)) == 0
    for model in (0, 1, 2, 3, 4, 6):                             # the figures of the twelve new instances
        for win in (0, 1):
            assert f"scene_groups_kernelILi{model}ELb{win}E" in text


def _arrays(rng, n, ticks, cols=4):
    return rng.normal(size=(n, 5)), np.arange(n + 1) * 2, rng.normal(size=(2 * n, 3)), rng.normal(size=(ticks, n, cols))


def test_scene_data_takes_groups_and_ego_split_carries_them():
    rng = np.random.default_rng(31)
    s0, off, dq, tr = _arrays(rng, 4, 12)
    d = cal.SceneData(s0, 5.0, off, dq, tr)
    assert np.array_equal(d.group, [0, 0, 0, 0]) and not d.grouped
    d = cal.SceneData(s0, 5.0, off, dq, tr, group=[0, 2, 1, 0])
    assert np.array_equal(d.group, [0, 2, 1, 0]) and d.grouped and d.group.dtype == np.int32
    for bad in ([0, 1, 0], [[0, 1, 0, 1]], [0.0, 1.0, 0.0, 1.0], [0, -1, 0, 0], 1, ["a", "b", "c", "d"]):
        with pytest.raises(ValueError):
            cal.SceneData(s0, 5.0, off, dq, tr, group=bad)
    egos = d.ego_split()
    assert len(egos) == 4 and all(np.array_equal(g.group, [0, 2, 1, 0]) and g.grouped for g in egos)
    assert all(not g.grouped for g in cal.SceneData(s0, 5.0, off, dq, tr).ego_split())
    windowed = cal.SceneData(s0, 5.0, off, dq, tr, group=[1, 1, 0, 0], present=([0, 2, 0, 0], [12, 12, 9, 12]), replayed=[0, 0, 0, 1])
    assert all(np.array_equal(g.group, [1, 1, 0, 0]) for g in windowed.ego_split())


def _bowl(p):
    return (p.f_0 - 4.0) ** 2 + 100.0 * (p.sigma_0 - 0.6) ** 2 + 1.0


class FakeEngine:
    """what InteractionCalibration asks of an engine, as tests/test_scene_replay_host.py fakes it, with groups: the sums of a rider are
    a known function of ITS GROUP's set and the rider"""
    made = []

    def __init__(self, pod, capacity, device=0):
        self.pod, self.calls, self.group, self.n_groups, self.plain, self.mask = pod, [], None, 0, 0, None
        FakeEngine.made.append(self)

    def scene_calib_load(self, nr, s0, vd, off, rows, obj, feat, lengths=None, max_sets=256):
        self.R, self.T, self.max_sets = s0.shape[0], obj.shape[0], max_sets

    def scene_calib_replay(self, replayed, rows=None):
        self.mask = np.array(replayed, dtype=bool)

    def scene_calib_groups(self, group, n_groups=None):
        self.group, self.n_groups = np.array(group), n_groups

    def scene_calib_eval(self, pods, states=False, stride=1):
        self.plain += 1
        return self.scene_calib_eval_groups([(p,) for p in pods], states=states, stride=stride)

    def scene_calib_eval_groups(self, pods, road_F0=None, road_sigma=None, states=False, stride=1):
        self.calls.append(len(pods))
        self.last = pods
        r = np.arange(self.R)
        grp = np.zeros(self.R, dtype=int) if self.group is None else self.group
        sim = np.ones(self.R, dtype=bool) if self.mask is None else ~self.mask
        sums = np.zeros((len(pods), self.R, 2))
        st = np.zeros((self.T // stride, len(pods) * self.R, 5))
        for k, tup in enumerate(pods):
            assert len(tup) == max(self.n_groups, 1)
            bowl = np.array([_bowl(tup[g]) for g in grp])
            sums[k, :, 0] = sim * bowl * 10.0 ** (r % 7 - 3) / 3.0
            sums[k, :, 1] = sim * bowl * 10.0 ** (-(r % 5)) / 7.0
            st[:, k * self.R: (k + 1) * self.R, 0] = np.array([tup[g].f_0 for g in grp]) + r[None, :]
        return (sums, st) if states else sums

    def close(self):
        pass


def _data(rng):
    def scene(n, ticks, grp, mask=None, length=None):
        s0, off, dq, tr = _arrays(rng, n, ticks)
        return cal.SceneData(s0, 5.0, off, dq, tr, length=length, replayed=mask, group=grp)
    return [scene(3, 40, [0, 1, 0]), scene(7, 25, [1, 0, 0, 1, 1, 0, 1], mask=[0, 0, 1, 0, 0, 0, 1], length=20), scene(2, 40, None)]


KEYS = ["sigma_0", ("f_0", 1), ("f_0", 0)]
GP = [dict(hfov=2.0), dict(hfov=3.0, e_0=0.9)]


def _calibration(data, error_func, max_sets=4, keys=KEYS, gp=GP, **kw):
    return cal.InteractionCalibration(vehicle.TwoDBicycle, keys, data, data, [1, 1, 0, 0, 0, 0], error_func=error_func, max_sets=max_sets,
                                      engine_factory=FakeEngine, group_params=gp, **kw)


def test_a_candidate_becomes_one_parameter_set_per_group():
    rng = np.random.default_rng(32)
    c = _calibration(_data(rng), cal.calc_sse_timesteps)
    args = c._update_params_args_dict([0.55, 7.0, 3.0])
    assert args == {"sigma_0": 0.55, ("f_0", 1): 7.0, ("f_0", 0): 3.0}
    p0, p1 = c._pods(args)
    base = vehicle.TwoDBicycle.PARAMS_TYPE().to_pod(vehicle.TwoDBicycle.MODEL)
    assert p0.sigma_0 == p1.sigma_0 == 0.55                      # a shared key reaches all groups
    assert p0.f_0 == 3.0 and p1.f_0 == 7.0                       # ("f_0", g) reaches group g only
    assert p0.hfov == 2.0 and p1.hfov == 3.0 and p1.e_0 == 0.9 and p0.e_0 == base.e_0    # group_params stay fixed
    q0, q1 = c._pods({"sigma_0": 0.9})                           # a group's own key left out: the group's default
    assert q0.f_0 == q1.f_0 == base.f_0 and q0.hfov == 2.0 and q1.hfov == 3.0
    c.evaluate([[0.55, 7.0, 3.0]])
    eng, = FakeEngine.made[-1:]
    assert eng.n_groups == 2 and np.array_equal(eng.group, [0, 1, 0, 1, 0, 0, 1, 1, 0, 1, 0, 0]) and eng.plain == 0
    assert eng.pod.hfov == 2.0                                   # the engine is created with group 0's set
    (l0, l1), = eng.last
    assert bytes(l0) == bytes(p0) and bytes(l1) == bytes(p1)


def test_both_errors_a_custom_one_and_simulate_work_with_groups():
    rng = np.random.default_rng(33)
    data = _data(rng)
    theta = np.c_[rng.uniform(0.3, 0.9, 6), rng.uniform(1, 9, 6), rng.uniform(1, 9, 6)]
    nr, lens, nf = np.array([3, 7, 2]), np.array([40, 20, 40]), 2
    grp = np.concatenate([d.group for d in data])
    mask = np.concatenate([d.replayed for d in data])
    nsim = np.array([3, 5, 2])
    roff = np.r_[0, np.cumsum(nr)]
    for func in (cal.calc_sse_timesteps, cal.calc_maesse_samples):
        FakeEngine.made.clear()
        c = _calibration(data, func)
        err = c.evaluate(theta)
        eng, = FakeEngine.made
        assert eng.calls == [4, 2] and eng.plain == 0
        r = np.arange(12)
        for k, th in enumerate(theta):
            pods = c._pods(c._update_params_args_dict(th))
            bowl = np.array([_bowl(pods[g]) for g in grp])
            per = bowl * 10.0 ** (r % 7 - 3) / 3.0 if func is cal.calc_sse_timesteps else bowl * 10.0 ** (-(r % 5)) / 7.0
            total = 0.0
            for q in range(3):                                   # simulated riders in rider order, then scenes in scene order
                acc = 0.0
                for i in range(roff[q], roff[q + 1]):
                    if not mask[i]:
                        acc += per[i]
                total += acc if func is cal.calc_sse_timesteps else (acc / (lens[q] * nsim[q] * float(nf))) ** 2
            assert err[k] == total, (func.__name__, k)
        assert c.test([0.5, 2.0, 3.0]) == float(c.evaluate([[0.5, 2.0, 3.0]], test=True)[0])
        c.close()
    seen = []

    def custom(outs, objs):
        seen.append(outs)
        return float(sum(o[0, :, 0].sum() for o in outs))

    c = _calibration(data, custom, max_sets=8)
    err = c.evaluate([[0.5, 2.0, 3.0]])
    sim = [np.flatnonzero(~d.replayed) for d in data]
    assert [o.shape for o in seen[0]] == [(40, 3, 2), (20, 5, 2), (40, 2, 2)]
    for q, d in enumerate(data):                                 # column 0 of the fake's states: f_0 of the rider's group + rider
        assert np.array_equal(seen[0][q][0, :, 0], np.where(d.group[sim[q]] == 1, 2.0, 3.0) + roff[q] + sim[q])
    assert err[0] == float(sum(o[0, :, 0].sum() for o in seen[0]))
    trajs, objectives = c.simulate([0.5, 2.0, 3.0])
    assert [t.shape for t in trajs] == [(40, 3, 2), (20, 5, 2), (40, 2, 2)] and len(objectives) == 3
    # run / run_many / test reach the engine through evaluate and keep their optimum under the keys as given, tuples included
    c.param_args_opt = c._update_params_args_dict([0.5, 2.0, 3.0])
    assert set(c.param_args_opt) == set(KEYS) and c.test() == float(c.evaluate([[0.5, 2.0, 3.0]], test=True)[0])


def test_without_group_params_no_new_call_is_made():
    rng = np.random.default_rng(34)
    s0, off, dq, tr = _arrays(rng, 3, 10)
    plain = cal.SceneData(s0, 5.0, off, dq, tr)
    FakeEngine.made.clear()
    c = cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0", "sigma_0"], [plain, plain], [plain], [1, 1, 0, 0, 0, 0], engine_factory=FakeEngine)
    c.evaluate([[2.0, 0.5]])
    eng, = FakeEngine.made
    assert eng.group is None and eng.plain == 1 and len(eng.last[0]) == 1
    zeros = cal.SceneData(s0, 5.0, off, dq, tr, group=[0, 0, 0])   # (a scene that sets groups nobody defined parameters for: group 0 only)
    c = cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0"], [zeros], [zeros], [1, 1, 0, 0, 0, 0], engine_factory=FakeEngine)
    c.evaluate([[2.0]])
    assert FakeEngine.made[-1].group is None and FakeEngine.made[-1].plain == 1


def test_the_value_errors():
    rng = np.random.default_rng(35)
    s0, off, dq, tr = _arrays(rng, 3, 10)
    ok = cal.SceneData(s0, 5.0, off, dq, tr, group=[0, 1, 0])
    third = cal.SceneData(s0, 5.0, off, dq, tr, group=[0, 2, 0])
    with pytest.raises(ValueError, match="scene 1 of train_data"):           # a group nobody gave parameters
        _calibration([ok, third], cal.calc_sse_timesteps)
    with pytest.raises(ValueError, match="scene 0 of test_data"):
        cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0"], [ok], [third], [1, 1, 0, 0, 0, 0], engine_factory=FakeEngine, group_params=GP)
    with pytest.raises(ValueError, match="scene 0 of train_data"):           # ... and without group_params there is group 0 alone
        cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0"], [ok], [ok], [1, 1, 0, 0, 0, 0], engine_factory=FakeEngine)
    for keys in ([("f_0", 2)], [("f_0", -1)], [("f_0",)], [("f_0", 0, 1)], [(0, "f_0")], [("f_0", 1.0)], [("road_F_0", 0)], [5]):
        with pytest.raises(ValueError, match="params_keys"):
            _calibration([ok], cal.calc_sse_timesteps, keys=keys)
    with pytest.raises(ValueError, match="group_params"):                     # a key per group and no groups
        _calibration([ok], cal.calc_sse_timesteps, keys=[("f_0", 0)], gp=None)
    for gp in ([], [{}] * 5):
        with pytest.raises(ValueError, match="group_params"):
            _calibration([ok], cal.calc_sse_timesteps, keys=["f_0"], gp=gp)
    # groups on shared lanes or on a wide scene: refused when the data set is loaded, before an engine is made
    n = 40
    big = cal.SceneData(rng.normal(size=(n, 5)), 5.0, np.arange(n + 1), rng.normal(size=(n, 3)), rng.normal(size=(10, n, 4)),
                        present=(np.arange(n) % 2 * 5, np.arange(n) % 2 * 5 + 5), group=np.arange(n) % 2)
    wide = cal.SceneData(s0, 5.0, off, dq, tr, group=[0, 1, 0], wide=True)
    for data, kw in (([big], {}), ([wide], {}), ([ok], dict(share_lanes=True))):
        FakeEngine.made.clear()
        c = _calibration(data, cal.calc_sse_timesteps, keys=["f_0"], **kw)
        with pytest.raises(ValueError, match="shared lanes"):
            c.evaluate([[2.0]])
        assert not FakeEngine.made


def test_the_grouped_oracle_is_not_chaotic_on_the_horizon():
    """the case of tests/test_gpu_scene_groups.py::test_grouped_scene_against_the_oracle: for both priority rules and each of the three
    candidates an oracle run with per-group parameter sets, started from positions perturbed by 1e-7 m (three random sign patterns),
    stays within 1e-5 x extent of the unperturbed one over the 200 ticks compared there - a tenth of that test's bound.  Measured:
    1.2e-8 x extent."""
    from scene_groups_common import ORACLE_GROUP, oracle_case, oracle_group_run
    rng = np.random.default_rng(7)
    worst = 0.0
    for rule in (0, 1):
        s0, off, dq, pods = oracle_case(rule)
        for k, pd in enumerate(pods):
            ref = oracle_group_run(pd, ORACLE_GROUP, s0, off, dq)
            ext = max(np.ptp(ref[..., 0]), np.ptp(ref[..., 1]), 14.0)
            for _ in range(3):
                s1 = s0.copy()
                s1[:, :2] += 1e-7 * rng.choice([-1.0, 1.0], size=(5, 2))
                per = oracle_group_run(pd, ORACLE_GROUP, s1, off, dq)
                dev = float(np.hypot(per[..., 0] - ref[..., 0], per[..., 1] - ref[..., 1]).max()) / ext
                worst = max(worst, dev)
                assert dev < 1e-5, (rule, k, dev)
        # (the groups matter to this case: with group 1 on group 0's set the riders end elsewhere)
        same = oracle_group_run((pods[0][0], pods[0][0]), ORACLE_GROUP, s0, off, dq)
        assert np.abs(same - oracle_group_run(pods[0], ORACLE_GROUP, s0, off, dq)).max() > 1e-3
    print(f"largest sensitivity of the grouped oracle to 1e-7 m at the start: {worst:.2e} x extent")


def test_the_groups_act_on_the_seeded_scenes():
    """the choice of scene_groups_common.ACT_SCENES, by the CPU oracle: f_0 x 1.6 in group 1 alone moves every rider of both scenes by
    more than 1e-4 m within 40 ticks (found: 1.2e-2 m and 8.6e-3 m for the least affected rider; a rider that neither sees a group-1
    source nor anybody who does would not move at all)"""
    from scene_groups_common import ACT_SCENES, ACT_TICKS, act_pods, act_scene, oracle_group_run
    base, other = act_pods()
    for k in range(len(ACT_SCENES)):
        s0, off, dq, grp = act_scene(k)
        a = oracle_group_run((base, base), grp, s0, off, dq, ticks=ACT_TICKS, stride=1)
        b = oracle_group_run((base, other), grp, s0, off, dq, ticks=ACT_TICKS, stride=1)
        least = float(np.abs(a - b).max(axis=(0, 2)).min())
        print(f"acting scene {k}: the least affected rider moves by {least:.2e} m")
        assert least > 1e-4, k
