"""Rider groups on shared lanes and on wide scenes in a closed-loop calibration, host side (no GPU): the new entry
point declared, exported and bound, `InteractionCalibration(lane_groups=True)` through a fake engine - the load call and then
`scene_calib_lane_groups` with the concatenated groups -, the default that still raises before an engine is made, no new call without
group_params, and the recorded resource comparison."""
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
    name = "csf_scene_calib_lane_groups"
    assert name in declared and name in _ffi.SYMBOLS and hasattr(lib, name)
    assert lib.csf_scene_calib_lane_groups.restype in (C.c_int, C.c_int32)
    assert lib.csf_scene_calib_lane_groups.argtypes == [C.c_void_p, C.c_void_p, C.c_int32]
    assert lib.csf_scene_calib_lane_groups(None, None, 2) == -1
    assert lib.csf_abi_version() == 9 and _ffi.ABI_VERSION == 9      # (csf_params and the ABI version do not change)
    assert callable(Engine.scene_calib_lane_groups)


def test_the_resource_usage_comparison_is_recorded():
    text = open(os.path.join(ROOT, "profiles", "scene_lane_groups_resource_usage.txt")).read()
    m = re.search(r"Existing kernel instances: (\d+); identical[^:]*: (\d+); changed: (\d+); gone: (\d+)", text)
    assert m and int(m.group(1)) == int(m.group(2)) > 0 and int(m.group(3)) == 0 and int(m.group(4)) == 0
    for model in (0, 1, 2, 3, 4, 6):                             # the figures of the twelve new instances
        assert f"scene_lanes_groups_kernelILi{model}E" in text and f"scene_wide_groups_kernelILi{model}E" in text


class FakeEngine:
    """what InteractionCalibration asks of an engine on shared lanes, as tests/test_scene_groups_host.py fakes it: the calls in their
    order, and sums that are a known function of the rider's group's set"""
    made = []

    def __init__(self, pod, capacity, device=0):
        self.pod, self.capacity, self.log, self.group, self.n_groups, self.plain = pod, capacity, [], None, 0, 0
        FakeEngine.made.append(self)

    def _load(self, name, nr, nl, lane, enter, exit, s0, obj, max_sets, **kw):
        self.log.append(name)
        self.R, self.T, self.max_sets = s0.shape[0], obj.shape[0], max_sets
        self.nr, self.nl, self.lane, self.enter, self.exit, self.kw = np.array(nr), np.array(nl), np.array(lane), np.array(enter), np.array(exit), kw

    def scene_calib_load(self, nr, s0, vd, off, rows, obj, feat, lengths=None, max_sets=256):
        self.log.append("load")
        self.R, self.T, self.max_sets = s0.shape[0], obj.shape[0], max_sets

    def scene_calib_load_shared(self, nr, nl, lane, enter, exit, s0, vd, off, rows, obj, feat, lengths=None, max_sets=256):
        self._load("load_shared", nr, nl, lane, enter, exit, s0, obj, max_sets)

    def scene_calib_load_wide(self, nr, nl, lane, enter, exit, s0, vd, off, rows, obj, feat, lengths=None, max_sets=256, wide_from=33):
        self._load("load_wide", nr, nl, lane, enter, exit, s0, obj, max_sets, wide_from=wide_from)

    def scene_calib_windows(self, enter, exit):
        self.log.append("windows")

    def scene_calib_replay(self, replayed, rows=None):
        self.log.append("replay")

    def scene_calib_groups(self, group, n_groups=None):
        self.log.append("groups")
        self.group, self.n_groups = np.array(group), n_groups

    def scene_calib_lane_groups(self, group, n_groups=None):
        self.log.append("lane_groups")
        self.group, self.n_groups = np.array(group), n_groups

    def scene_calib_eval(self, pods, states=False, stride=1):
        self.plain += 1
        return self.scene_calib_eval_groups([(p,) for p in pods], states=states, stride=stride)

    def scene_calib_eval_groups(self, pods, road_F0=None, road_sigma=None, states=False, stride=1):
        self.log.append("eval_groups")
        self.last = pods
        grp = np.zeros(self.R, dtype=int) if self.group is None else self.group
        sums = np.zeros((len(pods), self.R, 2))
        for k, tup in enumerate(pods):
            assert len(tup) == max(self.n_groups, 1)
            sums[k, :, 0] = [tup[g].f_0 * (r + 1) for r, g in enumerate(grp)]
            sums[k, :, 1] = sums[k, :, 0] / 4.0
        st = np.zeros((self.T // stride, len(pods) * self.R, 5))
        return (sums, st) if states else sums

    def close(self):
        pass


GP = [dict(hfov=2.0), dict(hfov=3.0, e_0=0.9)]


def _scenes(rng):
    n = 40                                                       # a roster above 32: rider r is there over [2 r, 2 r + 6)
    big = cal.SceneData(rng.normal(size=(n, 5)), 5.0, np.arange(n + 1), rng.normal(size=(n, 3)), rng.normal(size=(90, n, 4)),
                        present=(2 * np.arange(n), 2 * np.arange(n) + 6), group=np.arange(n) % 2)
    small = cal.SceneData(rng.normal(size=(3, 5)), 5.0, np.arange(4), rng.normal(size=(3, 3)), rng.normal(size=(90, 3, 4)), group=[0, 1, 1])
    wide = cal.SceneData(rng.normal(size=(3, 5)), 5.0, np.arange(4), rng.normal(size=(3, 3)), rng.normal(size=(90, 3, 4)), group=[1, 1, 0], wide=True)
    return big, small, wide


def _calibration(data, keys=(("f_0", 1), ("f_0", 0)), gp=GP, **kw):
    return cal.InteractionCalibration(vehicle.TwoDBicycle, list(keys), data, data, [1, 1, 0, 0, 0, 0], max_sets=4, engine_factory=FakeEngine,
                                      group_params=gp, **kw)


def test_lane_groups_loads_as_today_and_then_hands_over_the_concatenated_groups():
    rng = np.random.default_rng(41)
    big, small, wide = _scenes(rng)
    for data, kw, load in (([big, small], {}, "load_shared"), ([small, wide], dict(wide_from=2), "load_wide"), ([small], dict(share_lanes=True), "load_shared"),
                           ([big, wide, small], {}, "load_wide")):
        FakeEngine.made.clear()
        c = _calibration(data, lane_groups=True, **kw)
        err = c.evaluate([[7.0, 3.0]])
        eng, = FakeEngine.made
        assert eng.log == [load, "lane_groups", "eval_groups"] and eng.plain == 0, eng.log
        grp = np.concatenate([d.group for d in data])
        assert eng.n_groups == 2 and np.array_equal(eng.group, grp) and eng.group.shape == (sum(d.n for d in data),)
        packed = [d.lanes() for d in data]                       # the load is today's: every scene on its own lanes, the windows with it
        assert np.array_equal(eng.nl, [p[1] for p in packed]) and np.array_equal(eng.lane, np.concatenate([p[0] for p in packed]))
        assert np.array_equal(eng.enter, np.concatenate([d.enter for d in data])) and np.array_equal(eng.exit, np.concatenate([d.exit for d in data]))
        assert eng.capacity == max(grp.size, 4 * int(eng.nl.sum()))
        assert eng.kw == (dict(wide_from=kw.get("wide_from", 33)) if load == "load_wide" else {})
        (p0, p1), = eng.last
        assert p0.f_0 == 3.0 and p1.f_0 == 7.0 and p0.hfov == 2.0 and p1.hfov == 3.0 and eng.pod.hfov == 2.0
        want = 0.0                                               # calc_sse_timesteps: riders in rider order, scenes in scene order
        at = 0
        for d in data:
            acc = 0.0
            for r in range(d.n):
                acc += (7.0 if d.group[r] else 3.0) * (at + r + 1)
            want += acc
            at += d.n
        assert err[0] == want
        c.close()


def test_lane_groups_changes_nothing_on_a_plain_data_set():
    """a data set that needs neither shared lanes nor `wide` keeps scene_calib_load + scene_calib_groups whatever lane_groups says"""
    rng = np.random.default_rng(42)
    _, small, _ = _scenes(rng)
    for lg in (False, True):
        FakeEngine.made.clear()
        c = _calibration([small], lane_groups=lg)
        c.evaluate([[7.0, 3.0]])
        eng, = FakeEngine.made
        assert eng.log == ["load", "groups", "eval_groups"], eng.log


def test_the_default_still_raises_and_makes_no_engine():
    rng = np.random.default_rng(43)
    big, small, wide = _scenes(rng)
    for data, kw in (([big], {}), ([wide], {}), ([small], dict(share_lanes=True)), ([big], dict(lane_groups=False))):
        FakeEngine.made.clear()
        c = _calibration(data, **kw)
        with pytest.raises(ValueError, match="shared lanes") as err:
            c.evaluate([[7.0, 3.0]])
        assert "lane_groups=True" in str(err.value)              # (the message names the way out)
        assert not FakeEngine.made


def test_without_group_params_no_new_call_is_made():
    rng = np.random.default_rng(44)
    big, small, wide = _scenes(rng)

    def plain(d):
        return cal.SceneData(d.s0, 5.0, d.dest_offsets, d.dest_xyz_stop, d.traj, present=(d.enter, d.exit), wide=d.wide)
    for data, load in (([plain(big)], "load_shared"), ([plain(small), plain(wide)], "load_wide")):
        for lg in (False, True):
            FakeEngine.made.clear()
            c = cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0"], data, data, [1, 1, 0, 0, 0, 0], max_sets=4, engine_factory=FakeEngine,
                                           lane_groups=lg)
            c.evaluate([[2.0]])
            eng, = FakeEngine.made
            assert eng.log == [load, "eval_groups"] and eng.plain == 1 and eng.group is None, eng.log
