"""Rosters that share the lanes of the one-wave tick, host side (no GPU): SceneData.lanes(), rosters above 32 and their
validation, the calls InteractionCalibration makes with and without shared lanes, both built-in errors and NaN placement on a shared
scene, and the entry point declared, exported and bound."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cyclistsocialforce_amd import _ffi, calibration as cal, vehicle
from cyclistsocialforce_amd.engine import Engine
from scene_calib_common import MODELS
from scene_lanes_common import CROWDS, LANES_T, extent, greedy_lanes, inside, oracle_windowed, peak, roster, sets3
from test_scene_windows_host import FakeEngine, _arrays, _bowl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "csf.h")).read()
    assert "csf_scene_calib_load_shared" in set(re.findall(r"\b(csf_[a-z_0-9]+)\s*\(", header))
    lib = _ffi.load()                                            # (the library as build() made it for gfx950)
    assert "csf_scene_calib_load_shared" in _ffi.SYMBOLS and hasattr(lib, "csf_scene_calib_load_shared")
    plain = list(lib.csf_scene_calib_load.argtypes)              # the same call with n_lanes, lane, enter, exit behind n_riders
    assert list(lib.csf_scene_calib_load_shared.argtypes) == plain[:3] + [C.c_void_p] * 4 + plain[3:]
    assert lib.csf_scene_calib_load_shared.restype in (C.c_int, C.c_int32)
    assert lib.csf_scene_calib_load_shared(None, 0, None, None, None, None, None, 0, None, None, None, None, None, None, 0, None, 0) == -1
    assert lib.csf_abi_version() == 9 and _ffi.ABI_VERSION == 9      # (no struct changes)
    assert callable(Engine.scene_calib_load_shared)


@pytest.mark.parametrize("model", MODELS)
def test_the_rosters_of_the_gpu_test_are_not_chaotic_on_the_horizon(model):
    """the seeds of tests/test_gpu_scene_lanes.py::test_rosters_above_the_lanes_against_the_population_path, by the CPU oracle: for the
    roster of 40 and the roster of 48, each of the three sets, a windowed oracle run (scene_lanes_common.oracle_windowed) started from
    positions moved by 1e-7 m stays within 1e-5 x extent of the unmoved one over the present cells of the 120 ticks - the bound that
    test asserts for its twin, a tenth of its bar against the launch.  A seed that fails here is changed, not the bound."""
    rng = np.random.default_rng(9)
    worst = 0.0
    for n, (win, seed) in CROWDS.items():
        s0, off, dq = roster(model, n, seed=seed)
        enter, exit = win()
        here = inside(enter, exit, LANES_T)
        s1 = s0.copy()
        s1[:, :2] += 1e-7 * rng.choice([-1.0, 1.0], size=(n, 2))
        for k, pod in enumerate(sets3(model)):
            ref = oracle_windowed(pod, s0, off, dq, enter, exit, LANES_T)
            assert np.array_equal(np.isfinite(ref).all(axis=2), here)
            per = oracle_windowed(pod, s1, off, dq, enter, exit, LANES_T)
            sens = float(np.hypot(per[here][:, 0] - ref[here][:, 0], per[here][:, 1] - ref[here][:, 1]).max()) / extent(ref)
            worst = max(worst, sens)
            assert sens < 1e-5, (n, k, sens)
    print(f"{model}: largest sensitivity of the windowed oracle to 1e-7 m at the start: {worst:.2e} x extent")


def _scene(rng, enter, exit, ticks, **kw):
    n = len(enter)
    s0, off, dq, tr = _arrays(rng, n, ticks)
    return cal.SceneData(s0, 5.0, off, dq, tr, present=(np.asarray(enter), np.asarray(exit)), **kw)


def test_lanes_on_random_windows():
    rng = np.random.default_rng(31)
    for trial in range(40):
        n, ticks = int(rng.integers(1, 60)), 50
        enter = rng.integers(0, ticks, n)
        exit = np.minimum(enter + rng.integers(0, 9, n), ticks)      # (some windows are empty)
        if peak(enter, exit, ticks) > 32:
            continue
        d = _scene(rng, enter, exit, ticks)
        lane, nl = d.lanes()
        again, nl2 = d.lanes()
        assert lane.dtype == np.int32 and lane.shape == (n,) and np.array_equal(lane, again) and nl == nl2
        assert nl == max(1, peak(enter, exit, ticks)), trial         # optimal: the brute-force peak
        want, want_nl = greedy_lanes(enter, exit)
        assert np.array_equal(lane, want) and nl == want_nl
        busy = exit > enter
        assert np.all(lane[~busy] == 0) and np.all((0 <= lane) & (lane < nl))
        for a in np.flatnonzero(busy):
            for b in np.flatnonzero(busy):
                if a < b and lane[a] == lane[b]:
                    assert exit[a] <= enter[b] or exit[b] <= enter[a], (trial, a, b)


def test_a_handover_at_the_same_tick_reuses_the_lane_and_empty_windows_take_nothing():
    rng = np.random.default_rng(32)
    # riders 0, 1 take lanes 0, 1; rider 2 enters at the tick rider 0 leaves: lane 0, and so does rider 3 after it; rider 5: lane 1
    d = _scene(rng, [0, 0, 10, 20, 5, 20], [10, 20, 20, 30, 5, 30], 30)
    lane, nl = d.lanes()
    assert nl == 2 and np.array_equal(lane, [0, 1, 0, 0, 0, 1])
    d = _scene(rng, [0, 0, 10, 10], [10, 20, 20, 30], 30)        # two at tick 10 and one lane free: a third lane
    assert d.lanes()[1] == 3 and np.array_equal(d.lanes()[0], [0, 1, 0, 2])
    d = _scene(rng, [3, 3, 3], [3, 3, 3], 10)
    assert d.lanes()[1] == 1 and np.array_equal(d.lanes()[0], [0, 0, 0])


def test_rosters_above_32_need_windows_that_keep_32_at_once():
    rng = np.random.default_rng(33)
    enter = 2 * np.arange(40)
    d = _scene(rng, enter, np.minimum(enter + 24, 100), 100)
    assert d.n == 40 and d.lanes()[1] == 12 and d.windowed
    s0, off, dq, tr = _arrays(rng, 33, 20)
    with pytest.raises(ValueError, match="32"):
        cal.SceneData(s0, 5.0, off, dq, tr)                      # as before: 33 road users without windows
    en, ex = np.zeros(34, dtype=int), np.full(34, 20)
    en[33], ex[33] = 7, 7                                        # an empty window counts for nothing ...
    en[0] = 6                                                    # ... and rider 0 enters late: 32 at ticks 0 .. 5, 33 from tick 6
    s0, off, dq, tr = _arrays(rng, 34, 20)
    with pytest.raises(ValueError, match=r"33 road users .* tick 6"):
        cal.SceneData(s0, 5.0, off, dq, tr, present=(en, ex))
    ex[1] = 6
    ok = cal.SceneData(s0, 5.0, off, dq, tr, present=(en, ex))
    assert ok.lanes()[1] == 32 and ok.lanes()[0][0] == ok.lanes()[0][1]
    # the road limit is that of the LANES: 12 lanes take 16 384 / 16 = 1 024 vertices, the roster of 40 would take 256
    verts = np.c_[np.linspace(0, 50, 600), np.zeros(600)]
    road = (np.array([0, 600]), verts, 2.0, 2.0)
    s0, off, dq, tr = _arrays(rng, 40, 100)
    cal.SceneData(s0, 5.0, off, dq, tr, present=(enter, np.minimum(enter + 24, 100)), road=road)
    with pytest.raises(ValueError):
        cal.SceneData(s0[:20], 5.0, off[:21], dq[:40], tr[:, :20], road=road)     # 20 road users without shared lanes: 512
    egos = d.ego_split()
    assert len(egos) == 40 and all(g.n == 40 and g.replayed.sum() == 39 and np.array_equal(g.enter, d.enter) for g in egos)


class LaneEngine(FakeEngine):
    """FakeEngine with the shared load: it keeps what it was passed"""

    def scene_calib_load_shared(self, nr, nl, lane, enter, exit, s0, vd, off, rows, obj, feat, lengths=None, max_sets=256):
        self.shared = dict(nr=np.array(nr), nl=np.array(nl), lane=np.array(lane), lengths=np.array(lengths), max_sets=max_sets)
        self.win = (np.array(enter), np.array(exit))
        self.R, self.T, self.obj = s0.shape[0], obj.shape[0], obj

    def scene_calib_windows(self, enter, exit):
        assert not hasattr(self, "shared"), "csf_scene_calib_windows is refused on a shared data set"
        super().scene_calib_windows(enter, exit)


def _calibration(data, func, **kw):
    return cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0", "sigma_0"], data, data, [1, 1, 0, 0, 0, 0], error_func=func, max_sets=4,
                                      engine_factory=LaneEngine, **kw)


def test_the_shared_load_is_used_for_a_roster_above_32_or_on_request_and_not_otherwise():
    rng = np.random.default_rng(34)
    small = _scene(rng, [0, 0, 10], [10, 20, 20], 20)
    enter = 2 * np.arange(40)
    big = _scene(rng, enter, np.minimum(enter + 24, 100), 100, length=100)
    FakeEngine.made.clear()
    _calibration([small], cal.calc_sse_timesteps).evaluate([[2.0, 0.5]])
    eng, = FakeEngine.made
    assert not hasattr(eng, "shared") and eng.window_calls == 1          # today's calls
    FakeEngine.made.clear()
    _calibration([small, big], cal.calc_sse_timesteps).evaluate([[2.0, 0.5]])
    eng, = FakeEngine.made
    assert eng.window_calls == 0
    assert np.array_equal(eng.shared["nr"], [3, 40]) and np.array_equal(eng.shared["nl"], [2, 12]) and eng.shared["max_sets"] == 4
    assert np.array_equal(eng.shared["lane"], np.r_[small.lanes()[0], big.lanes()[0]]) and np.array_equal(eng.shared["lengths"], [20, 100])
    assert np.array_equal(eng.win[0], np.r_[small.enter, big.enter]) and np.array_equal(eng.win[1], np.r_[small.exit, big.exit])
    assert eng.win[0].dtype == np.int32 and eng.shared["lane"].dtype == np.int32
    FakeEngine.made.clear()
    _calibration([small], cal.calc_sse_timesteps, share_lanes=True).evaluate([[2.0, 0.5]])
    eng, = FakeEngine.made
    assert np.array_equal(eng.shared["nl"], [2]) and np.array_equal(eng.shared["lane"], [0, 1, 0]) and eng.window_calls == 0


def test_both_errors_and_nan_placement_on_a_shared_scene():
    rng = np.random.default_rng(35)
    enter = 2 * np.arange(40)
    exit = np.minimum(enter + 24, 100)
    exit[7] = enter[7]
    mask = np.zeros(40, dtype=bool)
    mask[[3, 20]] = True
    n, ticks = 40, 100
    s0, off, dq, tr = _arrays(rng, n, ticks)
    t = np.arange(ticks)[:, None]
    here = (enter[None] <= t) & (t < exit[None])
    tr[~here] = np.nan
    d = cal.SceneData(s0, 5.0, off, dq, tr, replayed=mask, present=(enter, exit))
    cells = int((exit - enter)[~mask].sum())
    r = np.arange(n)
    act = ~mask & (exit > enter)
    for func in (cal.calc_sse_timesteps, cal.calc_maesse_samples):
        FakeEngine.made.clear()
        c = _calibration([d], func)
        err = c.evaluate([[2.0, 0.5]])[0]
        pod = c._pod({"f_0": 2.0, "sigma_0": 0.5})
        per = _bowl(pod) * 10.0 ** (r % 7 - 3) / 3.0 if func is cal.calc_sse_timesteps else _bowl(pod) * 10.0 ** (-(r % 5)) / 7.0
        acc = 0.0
        for i in range(n):
            acc += per[i] * act[i]
        assert err == (acc if func is cal.calc_sse_timesteps else (acc / (cells * 2.0)) ** 2)
        eng, = FakeEngine.made
        assert eng.rows.shape == (100, 2, 4) and np.isfinite(eng.rows).all()
    seen = []

    def custom(outs, objs):
        seen.append((outs, objs))
        return 0.0

    c = _calibration([d], custom)
    c.evaluate([[2.0, 0.5]])
    trajs, objectives = c.simulate([2.0, 0.5])
    want_nan = np.repeat(~here[:, ~mask, None], 2, axis=2)
    for outs, objs in seen + [(trajs, objectives)]:
        assert outs[0].shape == objs[0].shape == (100, 38, 2)
        assert np.array_equal(np.isnan(outs[0]), want_nan) and np.array_equal(np.isnan(objs[0]), want_nan)
