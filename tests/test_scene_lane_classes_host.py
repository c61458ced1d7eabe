"""Vehicle classes on shared lanes and on wide scenes in a closed-loop calibration, host side (no GPU): the new entry
point declared, exported and bound, `InteractionCalibration(vehicle_type=[...], lane_classes=True)` through a fake engine - the load call
and then `scene_calib_lane_classes` with the concatenated groups, the classes and the start states in the widest layout -, the default that
still raises before an engine is made, a single vehicle_type that makes exactly today's calls, the recorded resource comparison, and the
seeds of the GPU tests on the CPU oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cyclistsocialforce_amd import _ffi, calibration as cal, vehicle
from cyclistsocialforce_amd.engine import Engine
from scene_groups_common import GENERAL_TOL
from scene_lane_classes_common import extent, mixed_sets, take_class_scene, widen
from scene_lanes_common import LANES_T
from scene_mixed_common import oracle_mixed_run
from scene_wide_common import wide_crowd
from test_scene_lane_groups_host import FakeEngine as GroupsFake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "csf_scene_calib_lane_classes"


def test_the_entry_point_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "csf.h")).read()
    declared = set(re.findall(r"\b(csf_[a-z_0-9]+)\s*\(", header))
    lib = _ffi.load()                                                # (the gfx950 library is built and loads)
    assert NAME in declared and NAME in _ffi.SYMBOLS and hasattr(lib, NAME)
    assert lib.csf_scene_calib_lane_classes.restype in (C.c_int, C.c_int32)
    assert lib.csf_scene_calib_lane_classes.argtypes == [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    assert lib.csf_scene_calib_lane_classes(None, None, 2, None, None) == -1
    assert lib.csf_abi_version() == 9 and _ffi.ABI_VERSION == 9      # (csf_params and the ABI version do not change)
    assert callable(Engine.scene_calib_lane_classes)


def test_the_resource_usage_comparison_is_recorded():
    text = open(os.path.join(ROOT, "profiles", "scene_lane_classes_resource_usage.txt")).read()
    m = re.search(r"Existing kernel instances: (\d+); identical[^:]*: (\d+); changed: (\d+); gone: (\d+)", text)
    assert m and int(m.group(1)) == int(m.group(2)) >= 88 and int(m.group(3)) == 0 and int(m.group(4)) == 0
    for kernel in ("scene_lanes_mixed_kernel", "scene_wide_mixed_kernel"):   # the figures of the two new instances
        assert re.search(kernel + r"\S*: \d+ \d+ \d+ \d+ \d+ \d+ \| \d+, \d+", text), kernel
    assert "scene_mixed_kernelILb1E" in text and "scene_mixed_kernelILb0E" in text


class FakeEngine(GroupsFake):
    """tests/test_scene_lane_groups_host.py's fake engine with the two calls that hand over classes"""
    made = []

    def __init__(self, pod, capacity, device=0):
        super().__init__(pod, capacity, device)
        GroupsFake.made.remove(self)
        FakeEngine.made.append(self)
        self.models = self.s0 = None

    def _classes(self, name, group, models, s0):
        self.log.append(name)
        self.group, self.models, self.s0 = np.array(group), list(models), np.array(s0)
        self.n_groups = len(self.models)

    def scene_calib_classes(self, group, models=None, s0=None):
        self._classes("classes", group, models, s0)

    def scene_calib_lane_classes(self, group, models=None, s0=None):
        self._classes("lane_classes", group, models, s0)


TYPES = [vehicle.TwoDBicycle, vehicle.Bicycle]


def _scenes(rng):
    n = 40                                                       # a roster above 32: rider r is there over [2 r, 2 r + 6)
    big = cal.SceneData(rng.normal(size=(n, 5)), 5.0, np.arange(n + 1), rng.normal(size=(n, 3)), rng.normal(size=(90, n, 4)),
                        present=(2 * np.arange(n), 2 * np.arange(n) + 6), group=np.arange(n) % 2)
    small = cal.SceneData(rng.normal(size=(3, 5)), 5.0, np.arange(4), rng.normal(size=(3, 3)), rng.normal(size=(90, 3, 4)), group=[0, 1, 1])
    wide = cal.SceneData(rng.normal(size=(3, 5)), 5.0, np.arange(4), rng.normal(size=(3, 3)), rng.normal(size=(90, 3, 4)), group=[1, 1, 0], wide=True)
    return big, small, wide


def _calibration(data, vehicle_type=TYPES, keys=(("f_0", 1), ("f_0", 0)), **kw):
    return cal.InteractionCalibration(vehicle_type, list(keys), data, data, [1, 1, 0, 0, 0, 0], max_sets=4, engine_factory=FakeEngine, **kw)


def test_lane_classes_loads_as_today_and_then_hands_over_groups_classes_and_start_states():
    rng = np.random.default_rng(41)
    big, small, wide = _scenes(rng)
    for data, kw, load in (([big, small], {}, "load_shared"), ([small], dict(share_lanes=True), "load_shared"), ([small, wide], dict(wide_from=2), "load_wide"),
                           ([big, wide, small], {}, "load_wide")):     # a roster above 32; share_lanes; wide; narrow + wide
        FakeEngine.made.clear()
        c = _calibration(data, lane_classes=True, **kw)
        c.evaluate([[7.0, 3.0]])
        eng, = FakeEngine.made
        assert eng.log == [load, "lane_classes", "eval_groups"] and eng.plain == 0, eng.log
        grp = np.concatenate([d.group for d in data])
        assert np.array_equal(eng.group, grp) and eng.group.shape == (sum(d.n for d in data),)
        assert eng.models == [t.MODEL for t in TYPES] == [_ffi.TWOD, _ffi.BICYCLE]
        want = np.zeros((grp.size, 8))                           # the start states in the widest layout, missing columns 0
        want[:, :5] = np.concatenate([d.s0[:, :5] for d in data])
        assert eng.s0.shape == (grp.size, 8) and np.array_equal(eng.s0, want)
        packed = [d.lanes() for d in data]                       # the load is today's: every scene on its own lanes, the windows with it
        assert np.array_equal(eng.nl, [p[1] for p in packed]) and np.array_equal(eng.lane, np.concatenate([p[0] for p in packed]))
        assert np.array_equal(eng.enter, np.concatenate([d.enter for d in data])) and np.array_equal(eng.exit, np.concatenate([d.exit for d in data]))
        assert eng.capacity == max(grp.size, 4 * int(eng.nl.sum()))
        assert eng.kw == (dict(wide_from=kw.get("wide_from", 33)) if load == "load_wide" else {})
        (p0, p1), = eng.last
        assert p0.f_0 == 3.0 and p1.f_0 == 7.0 and p0.model == _ffi.TWOD and p1.model == _ffi.BICYCLE and eng.pod.model == _ffi.TWOD
        c.close()


def test_lane_classes_changes_nothing_on_a_plain_data_set():
    """a data set that needs neither shared lanes nor `wide` keeps scene_calib_load + scene_calib_classes whatever lane_classes says"""
    rng = np.random.default_rng(42)
    _, small, _ = _scenes(rng)
    for lc in (False, True):
        FakeEngine.made.clear()
        c = _calibration([small], lane_classes=lc)
        c.evaluate([[7.0, 3.0]])
        eng, = FakeEngine.made
        assert eng.log == ["load", "classes", "eval_groups"], eng.log


def test_the_default_still_raises_and_makes_no_engine():
    rng = np.random.default_rng(43)
    big, small, wide = _scenes(rng)
    for data, kw in (([big], {}), ([wide], {}), ([small], dict(share_lanes=True)), ([big], dict(lane_classes=False)), ([big], dict(lane_groups=True))):
        FakeEngine.made.clear()
        c = _calibration(data, **kw)
        with pytest.raises(ValueError, match="mixed classes run on Engine.scene_calib_load only") as err:
            c.evaluate([[7.0, 3.0]])
        assert "shared lanes" in str(err.value)                  # (today's text, which tests/test_calibration_calls_host.py pins)
        assert not FakeEngine.made


def test_a_single_vehicle_type_makes_exactly_todays_calls():
    rng = np.random.default_rng(44)
    big, small, wide = _scenes(rng)

    def plain(d):
        return cal.SceneData(d.s0, 5.0, d.dest_offsets, d.dest_xyz_stop, d.traj, present=(d.enter, d.exit), wide=d.wide)
    for lc in (False, True):
        for data, load in (([plain(big)], "load_shared"), ([plain(small), plain(wide)], "load_wide")):
            FakeEngine.made.clear()
            c = _calibration(data, vehicle_type=vehicle.TwoDBicycle, keys=["f_0"], lane_classes=lc)
            c.evaluate([[2.0]])
            eng, = FakeEngine.made
            assert eng.log == [load, "eval_groups"] and eng.plain == 1 and eng.group is None and eng.models is None, eng.log
        # ... and with groups of ONE class the call is scene_calib_lane_groups, as today
        FakeEngine.made.clear()
        c = _calibration([big], vehicle_type=vehicle.TwoDBicycle, group_params=[{}, {}], lane_groups=True, lane_classes=lc)
        c.evaluate([[7.0, 3.0]])
        eng, = FakeEngine.made
        assert eng.log == ["load_shared", "lane_groups", "eval_groups"] and eng.models is None, eng.log


# ---- the seeds of tests/test_gpu_scene_lane_classes.py on the CPU oracle, where it can express the scene: a population of several
# classes that is there throughout (csfo_set_classes, as oracle_mixed_run).  Moving every start by 1e-7 m keeps every compared row within a
# tenth of the bound the GPU test uses.
def _moved(s0, seed=9):
    s1 = s0.copy()
    s1[:, :2] += 1e-7 * np.random.default_rng(seed).choice([-1.0, 1.0], size=(s0.shape[0], 2))
    return s1


@pytest.mark.parametrize("n", [33, 65])
def test_the_wide_crowds_of_six_classes_are_not_chaotic_on_the_horizon(n):
    """wide_crowd("balancingrider", n), classes r % 6, LANES_T ticks: positions within 1e-5 x extent (the GPU bound is 1e-4 x extent)"""
    s0, off, dq = widen(wide_crowd("balancingrider", n))
    grp = (np.arange(n) % 6).astype(np.uint8)
    for k, pods in enumerate(mixed_sets()):
        a = oracle_mixed_run(pods, grp, s0, off, dq, LANES_T)
        b = oracle_mixed_run(pods, grp, _moved(s0), off, dq, LANES_T)
        ext = extent(a)
        sens = float(np.hypot(a[..., 0] - b[..., 0], a[..., 1] - b[..., 1]).max())
        print(f"n = {n} candidate {k}: moved by 1e-7 m: {sens / ext:.2e} x extent")
        assert np.isfinite(a).all() and sens < 1e-5 * ext, (n, k, sens / ext)


def test_the_one_rider_per_lane_scene_is_not_chaotic_on_the_horizon():
    """the 7 riders of take_class_scene(), classes r % 6, everybody there for LANES_T ticks (the oracle has no windows): every state row
    within GENERAL_TOL / 10"""
    s0, off, dq = take_class_scene()
    grp = (np.arange(7) % 6).astype(np.uint8)
    for k, pods in enumerate(mixed_sets()):
        a = oracle_mixed_run(pods, grp, s0, off, dq, LANES_T, rows=8)
        b = oracle_mixed_run(pods, grp, _moved(s0), off, dq, LANES_T, rows=8)
        sens = float(np.abs(a - b).max())
        print(f"candidate {k}: moved by 1e-7 m: {sens:.2e} (a tenth of the bound: {GENERAL_TOL / 10:g})")
        assert np.isfinite(a).all() and sens < GENERAL_TOL / 10, (k, sens)
