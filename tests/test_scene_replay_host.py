"""Riders that follow their recorded trajectory in a closed-loop calibration, host side (no GPU): SceneData's
mask and default queue, ego_split, both built-in errors and a custom one formed over the simulated riders only, the refusal of a
scene without a simulated rider, and the entry point declared, exported and bound."""
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
    assert "csf_scene_calib_replay" in set(re.findall(r"\b(csf_[a-z_0-9]+)\s*\(", header))
    lib = _ffi.load()
    assert "csf_scene_calib_replay" in _ffi.SYMBOLS and hasattr(lib, "csf_scene_calib_replay")
    assert lib.csf_scene_calib_replay.restype in (C.c_int, C.c_int32)
    assert lib.csf_scene_calib_replay.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.csf_scene_calib_replay(None, None, None) == -1
    assert lib.csf_abi_version() == 9 and _ffi.ABI_VERSION == 9      # (csf_params and the ABI version do not change)
    assert callable(Engine.scene_calib_replay)


def _arrays(rng, n, ticks, cols=4):
    return rng.normal(size=(n, 5)), np.arange(n + 1) * 2, rng.normal(size=(2 * n, 3)), rng.normal(size=(ticks, n, cols))


def test_scene_data_takes_a_mask_and_gives_a_replayed_rider_its_start_as_queue():
    rng = np.random.default_rng(11)
    s0, off, dq, tr = _arrays(rng, 4, 12)
    d = cal.SceneData(s0, 5.0, off, dq, tr)
    assert d.replayed.dtype == bool and d.replayed.shape == (4,) and not d.replayed.any()
    d = cal.SceneData(s0, 5.0, off, dq, tr, replayed=[0, 1, 0, 1])
    assert np.array_equal(d.replayed, [False, True, False, True])
    assert np.array_equal(d.dest_offsets, off) and np.array_equal(d.dest_xyz_stop, dq)      # (complete queues stay as given)
    for mask in ([True, False], np.zeros((4, 1), dtype=bool), np.zeros(5, dtype=bool)):
        with pytest.raises(ValueError):
            cal.SceneData(s0, 5.0, off, dq, tr, replayed=mask)
    # (x, y, psi, v) over all `length` rows: three columns are too few, a hole in the recording is refused, one behind `length` is not
    with pytest.raises(ValueError):
        cal.SceneData(s0, 5.0, off, dq, tr[:, :, :3], replayed=[0, 1, 0, 0])
    cal.SceneData(s0, 5.0, off, dq, tr[:, :, :3], replayed=[0, 0, 0, 0])
    hole = tr.copy()
    hole[9, 1, 2] = np.nan
    with pytest.raises(ValueError):
        cal.SceneData(s0, 5.0, off, dq, hole, replayed=[0, 1, 0, 0])
    cal.SceneData(s0, 5.0, off, dq, hole, replayed=[0, 1, 0, 0], length=9)
    cal.SceneData(s0, 5.0, off, dq, hole, replayed=[1, 0, 1, 1])
    # a replayed rider without a queue gets (x0, y0, no stop); a simulated one must have a row
    off2, dq2 = np.array([0, 2, 2, 4, 4]), np.r_[dq[0:2], dq[4:6]]
    d = cal.SceneData(s0, 5.0, off2, dq2, tr, replayed=[0, 1, 0, 1])
    assert np.array_equal(d.dest_offsets, [0, 2, 3, 5, 6])
    assert np.array_equal(d.dest_xyz_stop, np.r_[dq[0:2], [[s0[1, 0], s0[1, 1], 0.0]], dq[4:6], [[s0[3, 0], s0[3, 1], 0.0]]])
    with pytest.raises(ValueError):
        cal.SceneData(s0, 5.0, off2, dq2, tr, replayed=[0, 1, 0, 0])
    with pytest.raises(ValueError):
        cal.SceneData(s0, 5.0, off2, dq2, tr)


def test_ego_split_gives_one_scene_per_simulated_rider_and_shares_the_arrays():
    rng = np.random.default_rng(12)
    s0, off, dq, tr = _arrays(rng, 5, 9, cols=6)
    d = cal.SceneData(s0, [4.0, 5.0, 6.0, 7.0, 8.0], off, dq, tr, length=7)
    egos = d.ego_split()
    assert len(egos) == 5
    for i, g in enumerate(egos):
        assert isinstance(g, cal.SceneData) and g.n == 5 and g.length == 7
        assert np.array_equal(g.replayed, np.arange(5) != i)
        assert np.shares_memory(g.s0, d.s0) and np.shares_memory(g.traj, d.traj) and np.shares_memory(g.dest_xyz_stop, d.dest_xyz_stop)
        assert np.shares_memory(g.dest_offsets, d.dest_offsets) and np.array_equal(g.v_desired, d.v_desired)
        assert not any(np.shares_memory(g.replayed, h.replayed) for h in egos if h is not g) and not np.shares_memory(g.replayed, d.replayed)
    assert not d.replayed.any()                                   # (the scene itself is unchanged)
    # a road user that is replayed in the scene is nobody's ego and stays replayed in every split
    d = cal.SceneData(s0, 5.0, off, dq, tr, replayed=[0, 0, 1, 0, 0])
    egos = d.ego_split()
    assert [int(np.flatnonzero(~g.replayed)[0]) for g in egos] == [0, 1, 3, 4] and all((~g.replayed).sum() == 1 for g in egos)
    with pytest.raises(ValueError):                               # the others need (x, y, psi, v)
        cal.SceneData(s0, 5.0, off, dq, tr[:, :, :2]).ego_split()


def _bowl(p):
    return (p.f_0 - 4.0) ** 2 + 100.0 * (p.sigma_0 - 0.6) ** 2 + 1.0


class FakeEngine:
    """what InteractionCalibration asks of an engine, as tests/test_scene_calib_host.py fakes it, with the replay: the sums of a
    simulated rider are a known function of the set and the rider, those of a replayed rider (0, 0) as the device returns them"""
    made = []

    def __init__(self, pod, capacity, device=0):
        self.calls, self.mask, self.rows, self.replays = [], None, None, 0
        FakeEngine.made.append(self)

    def scene_calib_load(self, nr, s0, vd, off, rows, obj, feat, lengths=None, max_sets=256):
        self.R, self.T, self.max_sets, self.off, self.dest = s0.shape[0], obj.shape[0], max_sets, off, rows

    def scene_calib_replay(self, replayed, rows=None):
        self.mask, self.rows, self.replays = None if replayed is None else np.array(replayed, dtype=bool), rows, self.replays + 1

    def scene_calib_eval(self, pods, states=False, stride=1):
        self.calls.append(len(pods))
        r = np.arange(self.R)
        sim = np.ones(self.R, dtype=bool) if self.mask is None else ~self.mask
        sums = np.zeros((len(pods), self.R, 2))
        for k, p in enumerate(pods):
            sums[k, :, 0] = sim * _bowl(p) * 10.0 ** (r % 7 - 3) / 3.0
            sums[k, :, 1] = sim * _bowl(p) * 10.0 ** (-(r % 5)) / 7.0
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


def _data(rng):
    def scene(n, ticks, mask, length=None):
        s0, off, dq, tr = _arrays(rng, n, ticks)
        return cal.SceneData(s0, 5.0, off, dq, tr, length=length, replayed=mask)
    return [scene(3, 40, [0, 1, 0]), scene(7, 25, [1, 0, 0, 1, 1, 0, 1], length=20), scene(2, 40, None)]


def test_both_errors_are_formed_over_the_simulated_riders_and_the_replay_is_loaded_with_the_data_set():
    rng = np.random.default_rng(13)
    data = _data(rng)
    theta = np.c_[rng.uniform(1, 9, 6), rng.uniform(0.3, 0.9, 6)]
    nr, lens, nf = np.array([3, 7, 2]), np.array([40, 20, 40]), 2
    mask = np.concatenate([d.replayed for d in data])
    nsim = np.array([2, 3, 2])
    roff = np.r_[0, np.cumsum(nr)]
    for func in (cal.calc_sse_timesteps, cal.calc_maesse_samples):
        FakeEngine.made.clear()
        c = _calibration(data, func)
        err = c.evaluate(theta)
        eng, = FakeEngine.made
        assert eng.calls == [4, 2] and eng.replays == 1 and np.array_equal(eng.mask, mask)
        # the recorded (x, y, psi, v) of the replayed riders, in rider order, zero behind the rows a scene has
        assert eng.rows.shape == (40, 5, 4)
        assert np.array_equal(eng.rows[:, 0], data[0].traj[:, 1, :4])
        assert np.array_equal(eng.rows[:25, 1:5], data[1].traj[:, [0, 3, 4, 6], :4]) and np.all(eng.rows[25:, 1:5] == 0.0)
        r = np.arange(12)
        for k, (f0, sg) in enumerate(theta):
            pod = c._pod({"f_0": f0, "sigma_0": sg})
            per = _bowl(pod) * 10.0 ** (r % 7 - 3) / 3.0 if func is cal.calc_sse_timesteps else _bowl(pod) * 10.0 ** (-(r % 5)) / 7.0
            total = 0.0
            for q in range(3):                                   # simulated riders in rider order, then scenes in scene order
                acc = 0.0
                for i in range(roff[q], roff[q + 1]):
                    if not mask[i]:
                        acc += per[i]
                total += acc if func is cal.calc_sse_timesteps else (acc / (lens[q] * nsim[q] * float(nf))) ** 2
            assert err[k] == total, (func.__name__, k)
        c.close()


def test_a_custom_error_and_simulate_get_the_simulated_riders_only():
    rng = np.random.default_rng(14)
    data = _data(rng)
    seen = []

    def custom(outs, objs):
        seen.append((outs, objs))
        return float(sum(o[0, :, 0].sum() for o in outs))

    FakeEngine.made.clear()
    c = _calibration(data, custom, max_sets=8)
    err = c.evaluate([[2.0, 0.5], [3.0, 0.5]])
    sim = [np.flatnonzero(~d.replayed) for d in data]
    assert [o.shape for o in seen[0][0]] == [(40, 2, 2), (20, 3, 2), (40, 2, 2)] == [o.shape for o in seen[0][1]]
    for q, d in enumerate(data):
        assert np.array_equal(seen[0][1][q], d.traj[: d.length][:, sim[q], :2])
    roff = [0, 3, 10]
    for k, f0 in enumerate((2.0, 3.0)):                          # column 0 of the fake's states is f_0 + rider
        for q in range(3):
            assert np.array_equal(seen[k][0][q][0, :, 0], c._pod({"f_0": f0}).f_0 + roff[q] + sim[q])
        assert err[k] == float(sum(o[0, :, 0].sum() for o in seen[k][0]))
    trajs, objectives = c.simulate([2.0, 0.5])
    assert [t.shape for t in trajs] == [(40, 2, 2), (20, 3, 2), (40, 2, 2)] and np.array_equal(objectives[1], data[1].traj[:20][:, sim[1], :2])


def test_a_scene_without_a_simulated_rider_is_refused_and_no_mask_never_touches_the_replay():
    rng = np.random.default_rng(15)
    s0, off, dq, tr = _arrays(rng, 3, 10)
    ok = cal.SceneData(s0, 5.0, off, dq, tr, replayed=[1, 0, 1])
    nothing = cal.SceneData(s0, 5.0, off, dq, tr, replayed=[1, 1, 1])
    with pytest.raises(ValueError):
        _calibration([ok, nothing], cal.calc_sse_timesteps).evaluate([[2.0, 0.5]])
    FakeEngine.made.clear()
    plain = cal.SceneData(s0, 5.0, off, dq, tr)
    _calibration([plain, plain], cal.calc_maesse_samples).evaluate([[2.0, 0.5]])
    assert FakeEngine.made[-1].replays == 0


def test_the_replayed_oracle_is_not_chaotic_on_the_horizon():
    """the case of tests/test_gpu_scene_replay.py::test_replayed_scene_against_the_oracle: for each of the three sets an oracle run
    whose replayed riders are pushed onto the recording every tick, started from positions perturbed by 1e-7 m (three random sign
    patterns), stays within 1e-5 x extent of the unperturbed one over the 200 ticks compared there - a tenth of that test's bound"""
    from scene_replay_common import ORACLE_REPLAYED, oracle_recording, oracle_replay_run
    s0, off, dq, pods, rec = oracle_recording()
    rng = np.random.default_rng(7)
    sim, worst = ~ORACLE_REPLAYED, 0.0
    for k, pod in enumerate(pods):
        ref = oracle_replay_run(pod, s0, off, dq, rec, ORACLE_REPLAYED)
        assert np.array_equal(ref[:, ORACLE_REPLAYED], rec[9::10][:, ORACLE_REPLAYED, :2])
        ext = max(np.ptp(ref[..., 0]), np.ptp(ref[..., 1]), 14.0)
        for _ in range(3):
            s1 = s0.copy()
            s1[:, :2] += 1e-7 * rng.choice([-1.0, 1.0], size=(s0.shape[0], 2))
            per = oracle_replay_run(pod, s1, off, dq, rec, ORACLE_REPLAYED)
            dev = float(np.hypot(per[:, sim, 0] - ref[:, sim, 0], per[:, sim, 1] - ref[:, sim, 1]).max()) / ext
            worst = max(worst, dev)
            assert dev < 1e-5, (k, dev)
    # with the set the recording was made with, the simulated riders repeat the recording: their sources are where they were
    true = oracle_replay_run(pods[1], s0, off, dq, rec, ORACLE_REPLAYED)
    assert np.abs(true - rec[9::10][:, :, :2]).max() < 1e-9
    print(f"largest sensitivity of the replayed oracle to 1e-7 m at the start: {worst:.2e} x extent")


def test_every_simulated_rider_of_the_first_three_scenes_feels_the_replay():
    """the choice of scene_replay_common.SCENE_SEEDS, by the CPU oracle: TwoD riders, the first set of field_sets free against the same
    set with the replayed riders pushed onto a recording made with the second set - every simulated rider of scenes 1 - 3 is moved
    by more than 1e-6 m within the scene's ticks (a rider that sees no replayed one would not move at all)"""
    from oracle import csf_oracle as orc
    from scene_calib_common import field_sets
    from scene_replay_common import LENGTHS, TRUE_SET, masks, replay_scenes

    def run(pod, s0, off, dq, ticks, rec=None, rep=None):
        pop = orc.Population(orc.Params.from_buffer_copy(bytes(pod)), s0, 5.0, off, dq)
        out = []
        for t in range(ticks):
            pop.step(1)
            s = pop.state()
            if rec is not None:
                s[rep, :4] = rec[t, rep, :4]
                pop.push_state(s)
            out.append(s.copy())
        return np.array(out)

    sets, per_mask = field_sets("twod", 3), masks()[0]
    for q, (s0, off, dq) in enumerate(replay_scenes("twod")[3][:3]):
        ln, pm = int(LENGTHS[q]), per_mask[q]
        rec = run(sets[TRUE_SET], s0, off, dq, ln)
        free, rep = run(sets[0], s0, off, dq, ln), run(sets[0], s0, off, dq, ln, rec, pm)
        least = min(float(np.abs(free[:, r, :2] - rep[:, r, :2]).max()) for r in np.flatnonzero(~pm))
        print(f"scene {q}: the least affected simulated rider moves by {least:.2e} m")
        assert least > 1e-6, q
