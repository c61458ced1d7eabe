"""Road users that enter and leave a scene in a closed-loop calibration, host side (no GPU): SceneData's presence
windows and their validation, ego_split, the fill of replay rows outside a window, both built-in errors over the present cells, NaN
placement for a custom error, a data set without windows making today's calls, and the entry point declared, exported and bound."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cyclistsocialforce_amd import _ffi, calibration as cal, vehicle
from cyclistsocialforce_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "csf.h")).read()
    assert "csf_scene_calib_windows" in set(re.findall(r"\b(csf_[a-z_0-9]+)\s*\(", header))
    lib = _ffi.load()
    assert "csf_scene_calib_windows" in _ffi.SYMBOLS and hasattr(lib, "csf_scene_calib_windows")
    assert lib.csf_scene_calib_windows.restype in (C.c_int, C.c_int32)
    assert lib.csf_scene_calib_windows.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.csf_scene_calib_windows(None, None, None) == -1
    assert lib.csf_abi_version() == 9 and _ffi.ABI_VERSION == 9      # (no struct changes: csf_params and the ABI version stay)
    assert callable(Engine.scene_calib_windows)


def test_the_resource_usage_comparison_is_recorded():
    text = open(os.path.join(ROOT, "profiles", "scene_windows_resource_usage.txt")).read()
    m = re.search(r"Existing kernel instances: (\d+); identical[^:]*: (\d+); changed: (\d+)", text)
    assert m and int(m.group(1)) == int(m.group(2)) > 0 and int(m.group(3)) == 0
    for model in (0, 1, 2, 3, 4, 6):                             # the figures of the six new instances
        assert f"scene_eval_kernelILi{model}ELb1E" in text


def _arrays(rng, n, ticks, cols=4):
    return rng.normal(size=(n, 5)), np.arange(n + 1) * 2, rng.normal(size=(2 * n, 3)), rng.normal(size=(ticks, n, cols))


def test_scene_data_takes_windows_and_validates_them():
    rng = np.random.default_rng(21)
    s0, off, dq, tr = _arrays(rng, 4, 12)
    d = cal.SceneData(s0, 5.0, off, dq, tr)
    assert np.array_equal(d.enter, [0, 0, 0, 0]) and np.array_equal(d.exit, [12, 12, 12, 12]) and not d.windowed
    assert d.enter.dtype == np.int32 and d.exit.dtype == np.int32
    d = cal.SceneData(s0, 5.0, off, dq, tr, length=9)
    assert np.array_equal(d.exit, [9, 9, 9, 9]) and not d.windowed
    d = cal.SceneData(s0, 5.0, off, dq, tr, length=9, present=([0, 0, 0, 0], [9, 9, 9, 9]))
    assert not d.windowed                                        # (full windows are no windows)
    d = cal.SceneData(s0, 5.0, off, dq, tr, present=([0, 3, 5, 12], [12, 3, 9, 12]))
    assert d.windowed and np.array_equal(d.enter, [0, 3, 5, 12]) and np.array_equal(d.exit, [12, 3, 9, 12])
    ins = d.inside
    assert ins.shape == (12, 4) and ins[:, 0].all() and not ins[:, 1].any() and not ins[:, 3].any()
    assert np.array_equal(np.flatnonzero(ins[:, 2]), [5, 6, 7, 8])
    for bad in (([0, 0, 0], [12, 12, 12]), ([0, 0, 0, -1], [12, 12, 12, 12]), ([0, 0, 0, 7], [12, 12, 12, 6]), ([0, 0, 0, 0], [12, 12, 12, 13]),
                ([0.0, 0, 0, 0], [12, 12, 12, 12]), 5, ([0, 0, 0, 0],), np.zeros((2, 2, 2), dtype=int)):
        with pytest.raises(ValueError):
            cal.SceneData(s0, 5.0, off, dq, tr, present=bad)
    with pytest.raises(ValueError):                              # exit <= length, not <= the rows of traj
        cal.SceneData(s0, 5.0, off, dq, tr, length=9, present=([0, 0, 0, 0], [9, 9, 9, 10]))
    # traj outside a window is never read: NaN there is fine for a simulated rider anywhere, for a replayed one outside its window only
    hole = tr.copy()
    hole[:5, 2] = hole[9:, 2] = np.nan
    cal.SceneData(s0, 5.0, off, dq, hole, present=([0, 0, 5, 0], [12, 12, 9, 12]))
    cal.SceneData(s0, 5.0, off, dq, hole, replayed=[0, 0, 1, 0], present=([0, 0, 5, 0], [12, 12, 9, 12]))
    cal.SceneData(s0, 5.0, off, dq, hole, replayed=[0, 0, 1, 0], present=([0, 0, 7, 0], [12, 12, 7, 12]))
    for en, ex in ((4, 9), (5, 10), (0, 12)):
        with pytest.raises(ValueError):
            cal.SceneData(s0, 5.0, off, dq, hole, replayed=[0, 0, 1, 0], present=([0, 0, en, 0], [12, 12, ex, 12]))
    with pytest.raises(ValueError):
        cal.SceneData(s0, 5.0, off, dq, hole, replayed=[0, 0, 1, 0])


def test_ego_split_passes_the_windows_on():
    rng = np.random.default_rng(22)
    s0, off, dq, tr = _arrays(rng, 5, 9, cols=6)
    d = cal.SceneData(s0, 5.0, off, dq, tr, length=8, present=([0, 2, 0, 4, 0], [8, 8, 5, 4, 8]))
    egos = d.ego_split()
    assert len(egos) == 4                                        # rider 3 is never present: nobody's ego
    assert [int(np.flatnonzero(~g.replayed)[0]) for g in egos] == [0, 1, 2, 4]
    for g in egos:
        assert g.windowed and np.array_equal(g.enter, d.enter) and np.array_equal(g.exit, d.exit) and g.length == 8
        assert np.shares_memory(g.traj, d.traj)
    plain = cal.SceneData(s0, 5.0, off, dq, tr, length=8)
    assert all(not g.windowed and np.array_equal(g.exit, [8] * 5) for g in plain.ego_split())
    hole = tr.copy()
    hole[:2, 1] = np.nan
    cal.SceneData(s0, 5.0, off, dq, hole, length=8, present=([0, 2, 0, 4, 0], [8, 8, 5, 4, 8])).ego_split()
    with pytest.raises(ValueError):                              # as a replayed rider, rider 1 needs its rows from tick 1 on
        cal.SceneData(s0, 5.0, off, dq, hole, length=8, present=([0, 1, 0, 4, 0], [8, 8, 5, 4, 8])).ego_split()


def test_replay_rows_are_filled_with_the_nearest_row_inside_the_window():
    rng = np.random.default_rng(23)
    s0, off, dq, tr = _arrays(rng, 4, 12)
    tr[:3, 1] = tr[8:, 1] = np.nan
    tr[:, 3] = np.nan
    d = cal.SceneData(s0, 5.0, off, dq, tr, length=10, replayed=[1, 1, 0, 1], present=([0, 3, 0, 6], [10, 8, 10, 6]))
    rows = d.replay_rows()
    assert rows.shape == (12, 3, 4)
    assert np.array_equal(rows[:, 0], tr[:, 0, :4])                                          # a full window: the recording as it is
    assert np.array_equal(rows[3:8, 1], tr[3:8, 1, :4])
    assert np.array_equal(rows[:3, 1], np.tile(tr[3, 1, :4], (3, 1))) and np.array_equal(rows[8:10, 1], np.tile(tr[7, 1, :4], (2, 1)))
    assert np.array_equal(rows[:10, 2], np.tile(s0[3, :4], (10, 1)))                         # never present: its start state
    assert np.isfinite(rows[:10]).all()
    assert np.isnan(tr[:3, 1]).all()                                                         # (the scene's own traj is untouched)
    plain = cal.SceneData(s0, 5.0, off, dq, tr, replayed=[1, 0, 0, 0])
    assert np.array_equal(plain.replay_rows(), tr[:, [0], :4])


def _bowl(p):
    return (p.f_0 - 4.0) ** 2 + 100.0 * (p.sigma_0 - 0.6) ** 2 + 1.0


class FakeEngine:
    """what InteractionCalibration asks of an engine, as tests/test_scene_replay_host.py fakes it, with the windows: the sums of a
    rider are a known function of the set and the rider, (0, 0) for a replayed rider and for one that is never present"""
    made = []

    def __init__(self, pod, capacity, device=0):
        self.calls, self.mask, self.rows, self.win, self.window_calls = [], None, None, None, 0
        FakeEngine.made.append(self)

    def scene_calib_load(self, nr, s0, vd, off, rows, obj, feat, lengths=None, max_sets=256):
        self.R, self.T, self.obj = s0.shape[0], obj.shape[0], obj

    def scene_calib_replay(self, replayed, rows=None):
        self.mask, self.rows = np.array(replayed, dtype=bool), rows

    def scene_calib_windows(self, enter, exit):
        self.win, self.window_calls = (np.array(enter), np.array(exit)), self.window_calls + 1

    def scene_calib_eval(self, pods, states=False, stride=1):
        self.calls.append(len(pods))
        r = np.arange(self.R)
        act = np.ones(self.R, dtype=bool) if self.mask is None else ~self.mask
        if self.win is not None:
            act = act & (self.win[1] > self.win[0])
        sums = np.zeros((len(pods), self.R, 2))
        for k, p in enumerate(pods):
            sums[k, :, 0] = act * _bowl(p) * 10.0 ** (r % 7 - 3) / 3.0
            sums[k, :, 1] = act * _bowl(p) * 10.0 ** (-(r % 5)) / 7.0
        if not states:
            return sums
        st = np.zeros((self.T // stride, len(pods) * self.R, 5))
        for k, p in enumerate(pods):
            st[:, k * self.R: (k + 1) * self.R, 0] = p.f_0 + r[None, :]       # (column 0 names the set and the rider)
        return sums, st

    def close(self):
        pass


def _calibration(data, error_func, max_sets=4):
    return cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0", "sigma_0"], data, data, [1, 1, 0, 0, 0, 0], error_func=error_func,
                                      max_sets=max_sets, engine_factory=FakeEngine)


WINDOWS = [([0, 5, 0], [40, 30, 40]), ([0, 0, 3, 0, 10, 20, 0], [20, 20, 20, 15, 10, 20, 20]), None]


def _data(rng):
    def scene(n, ticks, mask, present, length=None):
        s0, off, dq, tr = _arrays(rng, n, ticks)
        if present is not None:
            t = np.arange(ticks)[:, None]
            tr[~((np.array(present[0])[None] <= t) & (t < np.array(present[1])[None]))] = np.nan
        return cal.SceneData(s0, 5.0, off, dq, tr, length=length, replayed=mask, present=present)
    return [scene(3, 40, [0, 1, 0], WINDOWS[0]), scene(7, 25, [1, 0, 0, 1, 1, 0, 1], WINDOWS[1], length=20), scene(2, 40, None, WINDOWS[2])]


def test_both_errors_are_formed_over_the_present_cells_and_the_windows_are_loaded_with_the_data_set():
    rng = np.random.default_rng(24)
    data = _data(rng)
    theta = np.c_[rng.uniform(1, 9, 6), rng.uniform(0.3, 0.9, 6)]
    nr, nf = np.array([3, 7, 2]), 2
    mask = np.concatenate([d.replayed for d in data])
    roff = np.r_[0, np.cumsum(nr)]
    # present cells of the simulated riders: scene 0 riders 0, 2: 40 + 40; scene 1 riders 1, 2, 5: 20 + 17 + 0; scene 2: 40 + 40
    cells = np.array([80, 37, 80])
    for func in (cal.calc_sse_timesteps, cal.calc_maesse_samples):
        FakeEngine.made.clear()
        c = _calibration(data, func)
        err = c.evaluate(theta)
        eng, = FakeEngine.made
        assert eng.calls == [4, 2] and eng.window_calls == 1
        assert np.array_equal(eng.win[0], [0, 5, 0, 0, 0, 3, 0, 10, 20, 0, 0, 0]) and np.array_equal(eng.win[1], [40, 30, 40, 20, 20, 20, 15, 10, 20, 20, 40, 40])
        # what went to scene_calib_replay is finite over every scene's length: the fill
        assert eng.rows.shape == (40, 5, 4) and np.isfinite(eng.rows[:, 0]).all() and np.isfinite(eng.rows[:20, 1:]).all()
        assert np.array_equal(eng.rows[:25, 0:1], data[0].replay_rows()[:25]) and np.array_equal(eng.rows[:25, 1:], data[1].replay_rows(), equal_nan=True)
        assert np.array_equal(eng.rows[:5, 0], np.tile(data[0].traj[5, 1, :4], (5, 1)))
        r = np.arange(12)
        act = ~mask & (eng.win[1] > eng.win[0])
        for k, (f0, sg) in enumerate(theta):
            pod = c._pod({"f_0": f0, "sigma_0": sg})
            per = _bowl(pod) * 10.0 ** (r % 7 - 3) / 3.0 if func is cal.calc_sse_timesteps else _bowl(pod) * 10.0 ** (-(r % 5)) / 7.0
            total = 0.0
            for q in range(3):                                   # riders in rider order, then scenes in scene order
                acc = 0.0
                for i in range(roff[q], roff[q + 1]):
                    acc += per[i] * act[i]
                total += acc if func is cal.calc_sse_timesteps else (acc / (cells[q] * float(nf))) ** 2
            assert err[k] == total, (func.__name__, k)
        c.close()


def test_a_custom_error_and_simulate_get_nan_outside_the_windows():
    rng = np.random.default_rng(25)
    data = _data(rng)
    seen = []

    def custom(outs, objs):
        seen.append((outs, objs))
        return float(sum(np.nansum(o) for o in outs))

    FakeEngine.made.clear()
    c = _calibration(data, custom, max_sets=8)
    c.evaluate([[2.0, 0.5], [3.0, 0.5]])
    trajs, objectives = c.simulate([2.0, 0.5])
    sim = [np.flatnonzero(~d.replayed) for d in data]
    roff = [0, 3, 10]
    for (outs, objs), f0 in ((seen[0], 2.0), (seen[1], 3.0), ((trajs, objectives), 2.0)):
        assert [o.shape for o in outs] == [(40, 2, 2), (20, 3, 2), (40, 2, 2)] == [o.shape for o in objs]
        for q, d in enumerate(data):
            want_nan = np.repeat(~d.inside[:, sim[q], None], 2, axis=2)
            assert np.array_equal(np.isnan(outs[q]), want_nan) and np.array_equal(np.isnan(objs[q]), want_nan), q
            ok = ~want_nan
            assert np.array_equal(objs[q][ok], d.traj[: d.length][:, sim[q], :2][ok])
            col0 = np.broadcast_to(c._pod({"f_0": f0}).f_0 + roff[q] + sim[q], (d.length, sim[q].size))      # the fake's column 0
            assert np.array_equal(outs[q][..., 0][ok[..., 0]], col0[ok[..., 0]])
    assert not np.isnan(trajs[2]).any()                          # the scene without windows among scenes with them
    assert np.isnan(data[0].traj[:5, 1]).all()                   # (the scenes' own traj is untouched by the NaN in the objectives)


def test_no_windows_no_call_and_a_scene_with_nobody_to_fit_is_refused():
    rng = np.random.default_rng(26)
    s0, off, dq, tr = _arrays(rng, 3, 10)

    class Strict(FakeEngine):                                    # today's engine: it has no scene_calib_windows at all
        scene_calib_windows = None

    plain = cal.SceneData(s0, 5.0, off, dq, tr)
    full = cal.SceneData(s0, 5.0, off, dq, tr, present=([0, 0, 0], [10, 10, 10]))
    FakeEngine.made.clear()
    for func in (cal.calc_sse_timesteps, cal.calc_maesse_samples, lambda a, b: 0.0):
        c = cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0", "sigma_0"], [plain, full], [plain], [1, 1, 0, 0, 0, 0], error_func=func,
                                       max_sets=4, engine_factory=Strict)
        c.evaluate([[2.0, 0.5]])
        c.simulate([2.0, 0.5])
    assert all(e.window_calls == 0 and e.win is None for e in FakeEngine.made)
    # without windows the MAE-SSE divisor is today's length x simulated riders x n_feat
    FakeEngine.made.clear()
    c = _calibration([plain, full], cal.calc_maesse_samples)
    pod = c._pod({"f_0": 2.0, "sigma_0": 0.5})
    per = _bowl(pod) * 10.0 ** (-(np.arange(6) % 5)) / 7.0
    want = ((per[0] + per[1] + per[2]) / (10 * 3 * 2.0)) ** 2 + ((per[3] + per[4] + per[5]) / (10 * 3 * 2.0)) ** 2
    assert c.evaluate([[2.0, 0.5]])[0] == want
    # a scene needs a simulated rider with a non-empty window
    ok = cal.SceneData(s0, 5.0, off, dq, tr, replayed=[1, 0, 1], present=([0, 4, 0], [10, 5, 10]))
    _calibration([ok], cal.calc_sse_timesteps).evaluate([[2.0, 0.5]])
    for nothing in (cal.SceneData(s0, 5.0, off, dq, tr, replayed=[1, 0, 1], present=([0, 4, 0], [10, 4, 10])),
                    cal.SceneData(s0, 5.0, off, dq, tr, present=([0, 4, 10], [0, 4, 10])), cal.SceneData(s0, 5.0, off, dq, tr, replayed=[1, 1, 1])):
        with pytest.raises(ValueError):
            _calibration([ok, nothing], cal.calc_sse_timesteps).evaluate([[2.0, 0.5]])


def test_a_plain_data_set_with_an_empty_scene_evaluates_as_it_did():
    """A scene of length 0 has the default windows enter == exit == 0 and is no windowed scene: it is loaded and evaluated as before
    there were windows - no scene_calib_windows call, calc_sse_timesteps the riders' sums, calc_maesse_samples the sum over
    length x simulated riders x n_feat = 0 (inf or nan, as np.mean of nothing) - also beside a scene with a replayed rider, and
    ego_split still gives one scene per simulated rider."""
    rng = np.random.default_rng(27)
    s0, off, dq, tr = _arrays(rng, 3, 10)
    full = cal.SceneData(s0, 5.0, off, dq, tr)
    empty = cal.SceneData(s0, 5.0, off, dq, tr, length=0)
    empty_rep = cal.SceneData(s0, 5.0, off, dq, tr, length=0, replayed=[0, 1, 0])
    assert not empty.windowed and not empty_rep.windowed and len(empty.ego_split()) == 3 and len(empty_rep.ego_split()) == 2
    data = [full, empty, empty_rep]
    per_sse = lambda pod: _bowl(pod) * 10.0 ** (np.arange(9) % 7 - 3) / 3.0       # noqa: E731
    per_sae = lambda pod: _bowl(pod) * 10.0 ** (-(np.arange(9) % 5)) / 7.0       # noqa: E731
    sim = np.array([1, 1, 1, 1, 1, 1, 1, 0, 1], dtype=bool)
    for func in (cal.calc_sse_timesteps, cal.calc_maesse_samples, lambda a, b: float(len(a))):
        FakeEngine.made.clear()
        c = _calibration(data, func)
        with np.errstate(all="ignore"):
            err = c.evaluate([[2.0, 0.5]])[0]
        eng, = FakeEngine.made
        assert eng.window_calls == 0 and eng.win is None
        pod = c._pod({"f_0": 2.0, "sigma_0": 0.5})
        if func is cal.calc_sse_timesteps:
            p = per_sse(pod) * sim
            assert err == (p[0] + p[1] + p[2]) + (p[3] + p[4] + p[5]) + (p[6] + p[7] + p[8])
        elif func is cal.calc_maesse_samples:
            p = per_sae(pod) * sim
            with np.errstate(all="ignore"):                      # the parent's divisor: length x simulated riders x n_feat
                want = ((p[0] + p[1] + p[2]) / (10 * 3 * 2.0)) ** 2 + (np.float64(p[3] + p[4] + p[5]) / (0 * 3 * 2.0)) ** 2 \
                    + (np.float64(p[6] + p[7] + p[8]) / (0 * 2 * 2.0)) ** 2
            assert np.array_equal(err, want, equal_nan=True) and not np.isfinite(err)
        else:
            assert err == 3.0
        trajs, objectives = c.simulate([2.0, 0.5])
        assert [t.shape for t in trajs] == [(10, 3, 2), (0, 3, 2), (0, 2, 2)] == [o.shape for o in objectives]
