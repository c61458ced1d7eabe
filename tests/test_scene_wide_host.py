"""Scenes with more than 32 road users at once, host side (no GPU): SceneData(wide=True) and its validation, the
messages of wide=False unchanged, the call InteractionCalibration makes for a data set with a wide scene, the order the errors are
formed in, the seed of the GPU test's crowds on the CPU oracle, and the entry point declared, exported and bound."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cyclistsocialforce_amd import _ffi, calibration as cal, vehicle
from cyclistsocialforce_amd.engine import Engine
from scene_calib_common import MODELS, oracle_run
from scene_lanes_common import LANES_T, sets3
from scene_wide_common import WIDE_N, wide_crowd
from test_scene_windows_host import FakeEngine, _arrays, _bowl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "csf.h")).read()
    assert "csf_scene_calib_load_wide" in set(re.findall(r"\b(csf_[a-z_0-9]+)\s*\(", header))
    lib = _ffi.load()                                            # (the library as build() made it for gfx950)
    assert "csf_scene_calib_load_wide" in _ffi.SYMBOLS and hasattr(lib, "csf_scene_calib_load_wide")
    shared = list(lib.csf_scene_calib_load_shared.argtypes)      # the same call with wide_from behind max_sets
    assert list(lib.csf_scene_calib_load_wide.argtypes) == shared + [C.c_int32]
    assert lib.csf_scene_calib_load_wide.restype in (C.c_int, C.c_int32)
    assert lib.csf_scene_calib_load_wide(None, 0, None, None, None, None, None, 0, None, None, None, None, None, None, 0, None, 0, 33) == -1
    assert lib.csf_abi_version() == 9 and _ffi.ABI_VERSION == 9      # (no struct changes)
    assert callable(Engine.scene_calib_load_wide)


@pytest.mark.parametrize("model", MODELS)
def test_the_crowds_of_the_gpu_test_are_not_chaotic_on_the_horizon(model):
    """seed 72 of tests/test_gpu_scene_wide.py::test_wide_scenes_against_the_population_path, by the CPU oracle: for n = 33 and 65 (130
    for the two classes the GPU test runs there) and each of the three sets, a run started from positions moved by 1e-7 m stays within
    1e-5 x extent of the unmoved one over the 120 ticks - the bound that test asserts for its twin.  (Seed 71 does not pass: the
    BalancingRider reaches 6e-4.)  A seed that fails here is changed, not the bound."""
    worst = 0.0
    for n in WIDE_N:
        if n == 130 and model not in ("twod", "invpend"):
            continue
        s0, off, dq = wide_crowd(model, n)
        s1 = s0.copy()
        s1[:, :2] += 1e-7 * np.random.default_rng(9).choice([-1.0, 1.0], size=(n, 2))   # (the GPU test's own perturbation)
        for k, pod in enumerate(sets3(model)):
            ref = oracle_run(pod, s0, off, dq, ticks=LANES_T, stride=1)
            per = oracle_run(pod, s1, off, dq, ticks=LANES_T, stride=1)
            ext = max(float(np.ptp(ref[..., 0])), float(np.ptp(ref[..., 1])), 14.0)
            sens = float(np.hypot(per[..., 0] - ref[..., 0], per[..., 1] - ref[..., 1]).max()) / ext
            worst = max(worst, sens)
            assert sens < 1e-5, (n, k, sens)
    print(f"{model}: largest sensitivity of the oracle to 1e-7 m at the start: {worst:.2e} x extent")


def test_a_wide_scene_takes_256_at_once_and_names_tick_and_count():
    rng = np.random.default_rng(41)
    s0, off, dq, tr = _arrays(rng, 33, 20)
    d = cal.SceneData(s0, 5.0, off, dq, tr, wide=True)           # 33 without `present`
    assert d.wide and d.n == 33 and not d.windowed
    lane, nl = d.lanes()
    assert nl == 33 and np.array_equal(lane, np.arange(33)) and lane.dtype == np.int32
    s0, off, dq, tr = _arrays(rng, 256, 6)
    assert cal.SceneData(s0, 5.0, off, dq, tr, wide=True).lanes()[1] == 256
    s0, off, dq, tr = _arrays(rng, 257, 6)
    with pytest.raises(ValueError, match="256"):
        cal.SceneData(s0, 5.0, off, dq, tr, wide=True)           # 257 without windows
    en, ex = np.zeros(258, dtype=int), np.full(258, 20)
    en[257], ex[257] = 7, 7                                      # an empty window counts for nothing ...
    en[0] = 6                                                    # ... and rider 0 enters late: 256 at ticks 0 .. 5, 257 from tick 6
    s0, off, dq, tr = _arrays(rng, 258, 20)
    with pytest.raises(ValueError, match=r"257 road users .* tick 6; at most 256 at once"):
        cal.SceneData(s0, 5.0, off, dq, tr, present=(en, ex), wide=True)
    ex[1] = 6
    ok = cal.SceneData(s0, 5.0, off, dq, tr, present=(en, ex), wide=True)
    assert ok.lanes()[1] == 256 and ok.lanes()[0][0] == ok.lanes()[0][1]
    # a roster of 80 whose peak is 40
    enter = np.arange(80)
    s0, off, dq, tr = _arrays(rng, 80, 120)
    d = cal.SceneData(s0, 5.0, off, dq, tr, present=(enter, np.minimum(enter + 40, 120)), wide=True)
    assert d.lanes()[1] == 40
    egos = d.ego_split()
    assert len(egos) == 80 and all(g.wide and g.n == 80 and g.replayed.sum() == 79 and np.array_equal(g.enter, d.enter) for g in egos)
    s0, off, dq, tr = _arrays(rng, 40, 10)
    egos = cal.SceneData(s0, 5.0, off, dq, tr, wide=True).ego_split()
    assert len(egos) == 40 and all(g.wide and not g.windowed for g in egos)


def test_road_limits_of_a_wide_scene():
    """padded vertices x P <= 16 384 with P = 64, 128 or 256 - never below a wave, whatever kernel the scene ends up on"""
    rng = np.random.default_rng(42)

    def road(count):
        return np.array([0, count]), np.c_[np.linspace(0, 50, count), np.zeros(count)], 2.0, 2.0

    for n, most in ((7, 256), (33, 256), (64, 256), (65, 128), (128, 128), (129, 64), (256, 64)):
        s0, off, dq, tr = _arrays(rng, n, 5)
        assert cal.SceneData(s0, 5.0, off, dq, tr, wide=True, road=road(most)).road is not None
        with pytest.raises(ValueError, match=f"{most + 1} vertices"):
            cal.SceneData(s0, 5.0, off, dq, tr, wide=True, road=road(most + 1))
    # the LANES count, not the roster
    enter = np.arange(80)
    s0, off, dq, tr = _arrays(rng, 80, 120)
    cal.SceneData(s0, 5.0, off, dq, tr, present=(enter, np.minimum(enter + 40, 120)), wide=True, road=road(256))
    with pytest.raises(ValueError):
        cal.SceneData(s0, 5.0, off, dq, tr, present=(enter, np.minimum(enter + 70, 120)), wide=True, road=road(256))   # 70 lanes: 128


def test_without_wide_every_message_is_unchanged():
    rng = np.random.default_rng(43)
    s0, off, dq, tr = _arrays(rng, 33, 20)
    with pytest.raises(ValueError) as err:
        cal.SceneData(s0, 5.0, off, dq, tr)
    assert str(err.value) == "a scene has 1 .. 32 road users, or more with presence windows that keep at most 32 at once: s0 is [n, >= 4]"
    with pytest.raises(ValueError) as err:
        cal.SceneData(s0, 5.0, off, dq, tr, wide=False)
    assert str(err.value) == "a scene has 1 .. 32 road users, or more with presence windows that keep at most 32 at once: s0 is [n, >= 4]"
    en, ex = np.zeros(34, dtype=int), np.full(34, 20)
    en[33], ex[33], en[0] = 7, 7, 6
    s0, off, dq, tr = _arrays(rng, 34, 20)
    with pytest.raises(ValueError) as err:
        cal.SceneData(s0, 5.0, off, dq, tr, present=(en, ex))
    assert str(err.value) == "present: 33 road users are in the scene at tick 6; at most 32 at once"
    s0, off, dq, tr = _arrays(rng, 20, 20)
    verts = np.c_[np.linspace(0, 50, 600), np.zeros(600)]
    with pytest.raises(ValueError) as err:
        cal.SceneData(s0, 5.0, off, dq, tr, road=(np.array([0, 600]), verts, 2.0, 2.0))
    assert str(err.value) == "road: 600 vertices; a scene of 20 road users takes 512"
    d = cal.SceneData(s0, 5.0, off, dq, tr)
    assert d.wide is False and all(g.wide is False for g in d.ego_split())
    with pytest.raises(ValueError):
        cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0"], [d], [d], [1, 1, 0, 0, 0, 0], wide_from=0)
    with pytest.raises(ValueError):
        cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0"], [d], [d], [1, 1, 0, 0, 0, 0], wide_from=258)


class WideEngine(FakeEngine):
    """FakeEngine with the shared and the wide load: it keeps what it was passed"""

    def scene_calib_load_shared(self, nr, nl, lane, enter, exit, s0, vd, off, rows, obj, feat, lengths=None, max_sets=256):
        self.shared = dict(nr=np.array(nr), nl=np.array(nl), lane=np.array(lane), lengths=np.array(lengths), max_sets=max_sets)
        self.win = (np.array(enter), np.array(exit))
        self.R, self.T, self.obj = s0.shape[0], obj.shape[0], obj

    def scene_calib_load_wide(self, nr, nl, lane, enter, exit, s0, vd, off, rows, obj, feat, lengths=None, max_sets=256, wide_from=33):
        self.wide = dict(nr=np.array(nr), nl=np.array(nl), lane=np.array(lane), lengths=np.array(lengths), max_sets=max_sets, wide_from=wide_from,
                         s0=np.array(s0), off=np.array(off), feat=np.array(feat))
        self.win = (np.array(enter), np.array(exit))
        self.R, self.T, self.obj = s0.shape[0], obj.shape[0], obj

    def scene_calib_windows(self, enter, exit):
        raise AssertionError("csf_scene_calib_windows is refused on a data set that came with its lanes")


def _calibration(data, func, **kw):
    return cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0", "sigma_0"], data, data, [1, 1, 0, 0, 0, 0], error_func=func, max_sets=4,
                                      engine_factory=WideEngine, **kw)


def test_a_data_set_with_a_wide_scene_is_loaded_by_the_wide_call():
    rng = np.random.default_rng(44)
    s0, off, dq, tr = _arrays(rng, 3, 20)
    small = cal.SceneData(s0, 5.0, off, dq, tr, present=(np.array([0, 0, 10]), np.array([10, 20, 20])))
    s0w, offw, dqw, trw = _arrays(rng, 40, 30)
    big = cal.SceneData(s0w, 5.0, offw, dqw, trw, wide=True)
    enter = 2 * np.arange(40)
    s0r, offr, dqr, trr = _arrays(rng, 40, 100)
    relay = cal.SceneData(s0r, 5.0, offr, dqr, trr, present=(enter, np.minimum(enter + 24, 100)))
    FakeEngine.made.clear()
    _calibration([small, relay], cal.calc_sse_timesteps).evaluate([[2.0, 0.5]])
    eng, = FakeEngine.made
    assert hasattr(eng, "shared") and not hasattr(eng, "wide")   # no wide scene: the shared load, as before
    for kw, want in ((dict(), 33), (dict(wide_from=1), 1), (dict(wide_from=40), 40)):
        FakeEngine.made.clear()
        _calibration([small, big, relay], cal.calc_sse_timesteps, **kw).evaluate([[2.0, 0.5]])
        eng, = FakeEngine.made
        assert not hasattr(eng, "shared") and eng.wide["wide_from"] == want and eng.wide["max_sets"] == 4
        assert np.array_equal(eng.wide["nr"], [3, 40, 40]) and np.array_equal(eng.wide["nl"], [2, 40, 12])
        assert np.array_equal(eng.wide["lane"], np.r_[small.lanes()[0], np.arange(40), relay.lanes()[0]]) and eng.wide["lane"].dtype == np.int32
        assert np.array_equal(eng.wide["lengths"], [20, 30, 100])
        assert np.array_equal(eng.win[0], np.r_[small.enter, np.zeros(40), relay.enter]) and np.array_equal(eng.win[1], np.r_[small.exit, np.full(40, 30), relay.exit])
        assert eng.win[0].dtype == np.int32
        assert np.array_equal(eng.wide["s0"][3:43, :5], s0w) and np.array_equal(eng.wide["off"][3:44] - eng.wide["off"][3], offw)
        assert np.array_equal(eng.wide["feat"], [0, 1]) and eng.obj.shape == (100, 83, 2)
        assert np.array_equal(eng.obj[:30, 3:43], trw[:, :, :2])


def test_errors_on_a_wide_scene_are_formed_rider_then_scene():
    rng = np.random.default_rng(45)
    s0, off, dq, tr = _arrays(rng, 70, 50)
    mask = np.zeros(70, dtype=bool)
    mask[[3, 41]] = True
    wide = cal.SceneData(s0, 5.0, off, dq, tr, replayed=mask, wide=True)
    s0b, offb, dqb, trb = _arrays(rng, 4, 50)
    small = cal.SceneData(s0b, 5.0, offb, dqb, trb)
    r = np.arange(74)
    act = np.r_[~mask, np.ones(4, dtype=bool)]
    for func in (cal.calc_sse_timesteps, cal.calc_maesse_samples):
        FakeEngine.made.clear()
        c = _calibration([wide, small], func)
        err = c.evaluate([[2.0, 0.5], [3.0, 0.7]])
        for k, theta in enumerate(([2.0, 0.5], [3.0, 0.7])):
            pod = c._pod({"f_0": theta[0], "sigma_0": theta[1]})
            per = _bowl(pod) * 10.0 ** (r % 7 - 3) / 3.0 if func is cal.calc_sse_timesteps else _bowl(pod) * 10.0 ** (-(r % 5)) / 7.0
            scene = [0.0, 0.0]
            for i in range(70):                                  # the riders of a scene in rider order ...
                scene[0] += per[i] * act[i]
            for i in range(70, 74):
                scene[1] += per[i] * act[i]
            if func is cal.calc_sse_timesteps:
                want = 0.0
                for q in range(2):                               # ... then the scenes in scene order
                    want += scene[q]
            else:
                want = 0.0
                for q, cells in enumerate((68 * 50, 4 * 50)):
                    want += (scene[q] / (cells * 2.0)) ** 2
            assert err[k] == want, (func.__name__, k, err[k], want)
    trajs, objectives = _calibration([wide, small], cal.calc_sse_timesteps).simulate([2.0, 0.5])
    assert trajs[0].shape == objectives[0].shape == (50, 68, 2) and trajs[1].shape == (50, 4, 2)
    assert np.isfinite(trajs[0]).all() and np.isfinite(objectives[0]).all()
