"""Recorded trajectories and forces (include/csf.h: csf_record, csf_get_record, csf_batch_get_record; csf_agent.hip: the sample
written by small_tick_body / agent_body, record_gather_kernel): an engine that records stays on the one-wave tick and in the
batched launch, and what it records is - bit for bit - what a twin stepped one tick at a time shows after every tick.  The
comparisons are between runs of the same kernel, which reloads its whole state from memory every tick: equality is the bar."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cyclistsocialforce_amd._ffi import EngineError
from oracle import csf_oracle as orc
from test_gpu_parity import MODELS, amd, make_engine  # noqa: F401  (amd: fixture)
from test_gpu_small import crowd
from test_gpu_batch import CLASSES, assert_same

pytestmark = [pytest.mark.gpu, pytest.mark.auto_variant]

SMALL_CROWDS = [("twod", 8, 0, None), ("twod", 5, 1, None), ("twod", 2, 0, 4.0), ("twod", 1, 0, None),
                ("invpend", 6, 0, None), ("planarpoint", 8, 1, 2.0), ("planarpoint", 3, 0, None),
                ("twod", 16, 0, None), ("twod", 13, 1, 2.0), ("invpend", 16, 0, 4.0), ("planarpoint", 11, 0, None), ("twod", 16, 0, 4.0),
                ("twod", 32, 0, None), ("planarpoint", 27, 1, 2.0), ("invpend", 32, 0, None), ("invpend", 32, 0, 4.0), ("twod", 19, 0, 4.0),
                ("bicycle", 7, 0, None), ("bicycle", 32, 1, None), ("bicycle", 12, 0, 4.0),
                ("balancingrider", 5, 0, None), ("balancingrider", 14, 1, 2.5), ("balancingrider", 32, 0, None)]   # tests/test_gpu_small.py


def rider_crowd(amd, model, n, road, seed=None, capacity=None):
    box = 14.0 if n <= 8 else (22.0 if n <= 16 else 30.0)
    if model == "balancingrider":
        box *= 2.0
    x, y, psi, v, off, dq = crowd(n, seed=7 * n + 1 if seed is None else seed, box=box)
    s0 = np.zeros((n, orc.N_STATES[MODELS[model]])); s0[:, 0] = x; s0[:, 1] = y; s0[:, 2] = psi; s0[:, 3] = v
    e = make_engine(amd, model, s0, 5.0, off, dq, capacity=capacity)
    if road:
        m = 300 if n <= 16 else 200                            # (a road the wave can stage: vertices x lanes per road user <= 16 384)
        xs = np.linspace(-20.0, box + 20.0, m)
        e.set_road(np.array([0, m, 2 * m]), np.r_[np.c_[xs, np.full(m, -3.0)], np.c_[xs, np.full(m, box + 3.0)]],
                   np.array([0.15, 0.2]), np.array([2.0, 2.5]))
    return e


def per_tick(twin, ticks):
    """(S [ticks, n, ns], F [ticks, n, 2]) of a twin stepped one tick at a time with the read-back of every tick"""
    S, F = [], []
    for _ in range(ticks):
        s, _, _, fx, fy, _ = twin.step_snapshot(1)
        S.append(s.copy())
        F.append(np.c_[fx, fy])
    return np.array(S), np.array(F)


@pytest.mark.parametrize("road", [False, True])
@pytest.mark.parametrize("model,n", [("twod", 3), ("bicycle", 32), ("invpend", 7), ("planarpoint", 16), ("planarbike", 5), ("balancingrider", 12)])
def test_one_engine_records_on_the_one_wave_path(amd, model, n, road):
    """200 ticks in one call against a twin stepped in 200 calls: every entry of every sample, states and forces; stride 3; a
    ring shorter than the run keeps the last samples and refuses the earlier ones"""
    a, b = rider_crowd(amd, model, n, road), rider_crowd(amd, model, n, road)
    a.record(stride=1, capacity=200)
    a.step(200)
    S, F = a.recorded(0, 200)
    assert a.small_ticks() == 200                              # (recording did not leave the one-wave path)
    rS, rF = per_tick(b, 200)
    assert np.array_equal(S, rS) and np.array_equal(F, rF)
    assert np.array_equal(a.history(0, 200), rS)               # (csf_get_history reads the same ring)
    c = rider_crowd(amd, model, n, road)
    c.record(stride=3, capacity=100)
    c.step(200)
    S3, F3 = c.recorded(0, 66)
    assert c.small_ticks() == 200
    assert np.array_equal(S3, rS[2::3]) and np.array_equal(F3, rF[2::3])
    d = rider_crowd(amd, model, n, road)
    d.record(stride=1, capacity=50)
    d.step(200)
    Sd, Fd = d.recorded(150, 50)
    assert np.array_equal(Sd, rS[150:]) and np.array_equal(Fd, rF[150:])
    Sd, Fd = d.recorded(180, 20)
    assert np.array_equal(Sd, rS[180:]) and np.array_equal(Fd, rF[180:])
    for first, count in ((149, 10), (0, 1), (190, 11)):
        with pytest.raises(EngineError, match="not in the ring"):
            d.recorded(first, count)
    assert_same(a, b, "after the read-backs")


def test_sample_numbers_continue_across_calls_and_a_pushed_state(amd):
    a, b = rider_crowd(amd, "twod", 6, True), rider_crowd(amd, "twod", 6, True)
    a.record(stride=1, capacity=64)
    rS, rF = [], []
    for c in (1, 5, 1, 20):
        a.step(c)
        s, f = per_tick(b, c)
        rS.append(s); rF.append(f)
    for e in (a, b):
        s = e.state()
        s[:, 3] *= 0.8
        e.push_state(np.arange(e.n, dtype=np.int32), s)
    a.step(7)
    s, f = per_tick(b, 7)
    rS.append(s); rF.append(f)
    S, F = a.recorded(0, 34)
    assert np.array_equal(S, np.concatenate(rS)) and np.array_equal(F, np.concatenate(rF))
    assert a.small_ticks() == 34
    S2, F2 = a.recorded(27, 7)
    assert np.array_equal(S2, S[27:]) and np.array_equal(F2, F[27:])


def test_sample_numbers_run_through_the_launches_of_a_long_call(amd):
    """65 540 ticks are two launches (2^16 + 4): stride 4 096, the last samples against a twin stepped in calls of 4 096"""
    a, b = rider_crowd(amd, "twod", 3, False), rider_crowd(amd, "twod", 3, False)
    a.record(stride=4096, capacity=8)
    a.step(65540)
    rS, rF = [], []
    for _ in range(16):
        b.step(4095)
        s, f = per_tick(b, 1)
        rS.append(s[0]); rF.append(f[0])
    b.step(4)
    S, F = a.recorded(8, 8)
    assert a.small_ticks() == 65540
    assert np.array_equal(S, np.array(rS[8:])) and np.array_equal(F, np.array(rF[8:]))
    assert_same(a, b, "after 65 540 ticks")


def member(amd, i):
    """member i of a mixed batch that the batched launch takes whole: class, population 1 .. 32, a small road for some"""
    model = CLASSES[i % 6]
    n = 1 + (7 * i + i // 6) % 32
    return rider_crowd(amd, model, n, i % 7 in (0, 3) and n <= 16, seed=1000 + i, capacity=40)


def test_batch_records_and_reads_back_in_one_gather(amd):
    """64 mixed members (all classes, roads, populations 1 .. 32): three in four record (some without forces), one keeps
    csf_enable_history (stepped in turn, as before), calls of 1, 5, 1, 20"""
    K = 64
    batch = [member(amd, i) for i in range(K)]
    twins = [member(amd, i) for i in range(K)]
    rec = [i for i in range(K) if i % 4 != 3]
    for i in rec:
        batch[i].record(stride=1, capacity=40, forces=(i % 5 != 0))
    batch[7].enable_history(1, 40)
    twins[7].enable_history(1, 40)                             # (the general path on both sides: another kernel, other rounding)
    amd.Engine.batch_join(batch)
    ref = [([], []) for _ in range(K)]
    for c in (1, 5, 1, 20):
        amd.Engine.step_batch(batch, c)
        for i, t in enumerate(twins):
            s, f = per_tick(t, c)
            ref[i][0].append(s); ref[i][1].append(f)
    got = amd.Engine.batch_recorded(batch, 27)
    for i in range(K):
        rS, rF = np.concatenate(ref[i][0]), np.concatenate(ref[i][1])
        if i in rec:
            S, F, first = got[i]
            assert batch[i].batch_ticks() == 27, i             # (recording did not take the member out of the batched launch)
            assert first == 0 and np.array_equal(S, rS), i
            if i % 5 != 0:
                assert np.array_equal(F, rF), i
            else:
                assert F is None
        else:
            assert got[i] is None
        assert_same(batch[i], twins[i], f"member {i}")
    assert batch[7].batch_ticks() == 0 and np.array_equal(batch[7].history(0, 27), np.concatenate(ref[7][0]))
    assert all(batch[i].batch_ticks() == 27 for i in range(K) if i != 7)
    # a later call returns the later samples; a subset of the members can be read
    amd.Engine.step_batch(batch, 3)
    sub = amd.Engine.batch_recorded(batch, 2, only=[batch[0], batch[5]])
    for i in (0, 5):
        s, f = per_tick(twins[i], 3)
        assert sub[i][2] == 28 and np.array_equal(sub[i][0], s[1:]), i
    assert all(sub[i] is None for i in range(K) if i not in (0, 5))


@pytest.mark.parametrize("how", ["mid", "general"])
def test_every_path_records_the_same_thing(amd, monkeypatch, how):
    """40 road users (the one-launch tick of a mid-size population) and a pinned pair kernel (the general path): recorded states
    and forces equal state() / forces() read per tick from a twin"""
    if how == "general":
        monkeypatch.setenv("CSF_PAIR_VARIANT", "0")
    n = 40 if how == "mid" else 9
    a, b = rider_crowd(amd, "twod", n, False, seed=77), rider_crowd(amd, "twod", n, False, seed=77)
    a.record(stride=1, capacity=64)
    a.step(1); a.step(30); a.step(9)
    S, F = a.recorded(0, 40)
    assert a.small_ticks() == 0
    if how == "mid":
        assert a.mid_ticks() > 0
    for t in range(40):
        b.step(1)
        fx, fy = b.forces()
        assert np.array_equal(S[t], b.state()), t
        assert np.array_equal(F[t], np.c_[fx, fy]), t


@pytest.mark.parametrize("model,n,rule,hfov", SMALL_CROWDS)
def test_recorded_small_crowds_vs_oracle(amd, model, n, rule, hfov):
    """the crowds of tests/test_gpu_small.py::test_small_crowds_vs_oracle, under that test's tolerances: the recorded forces of 30
    ticks (1e-4 of the largest force of the tick) and the recorded positions (1e-4 of the extent) - of all 400 ticks for a handful
    that test lets run free, of the first 10 for the denser crowds it shadows in windows of 10 from a common state"""
    box = 14.0 if n <= 8 else (22.0 if n <= 16 else 30.0)
    if model == "balancingrider":
        box *= 2.0
    x, y, psi, v, off, dq = crowd(n, seed=10 * n + rule, box=box)
    s0 = np.zeros((n, orc.N_STATES[MODELS[model]])); s0[:, 0] = x; s0[:, 1] = y; s0[:, 2] = psi; s0[:, 3] = v
    over = {} if hfov is None else {"hfov": hfov}
    e = make_engine(amd, model, s0, 5.0, off, dq, rule, **over)
    pop = orc.Population(orc.default_params(model, priority_rule=rule, **over), s0, 5.0, off, dq)
    ticks = 400 if n <= 8 else 30
    e.record(stride=1, capacity=ticks)
    e.step(ticks)
    S, F = e.recorded(0, ticks)
    assert e.small_ticks() == ticks and (e.status() == 0).all()
    ref = []
    for t in range(ticks):
        pop.step(1)
        ref.append(pop.state().copy())
        if t < 30:
            ofx, ofy = pop.forces()
            scale = max(np.hypot(ofx, ofy).max(), 1e-3)
            err = max(np.abs(F[t, :, 0] - ofx).max(), np.abs(F[t, :, 1] - ofy).max())
            assert err < 1e-4 * scale, (t, n, err, scale)
    ref = np.array(ref)
    span = ticks if n <= 8 else 10
    extent = max(np.ptp(ref[-1][:, 0]), np.ptp(ref[-1][:, 1]), 14.0)
    dev = np.hypot(S[:span, :, 0] - ref[:span, :, 0], S[:span, :, 1] - ref[:span, :, 1]).max()
    assert dev < 1e-4 * extent, (dev, extent)


def test_wrong_calls_in_a_fresh_process():
    """refused calls of csf_record, csf_get_record and csf_batch_get_record (host-side argument checks), each with a message and
    nothing changed: in a child process"""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "record_abi_child.py")], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "PYTHONPATH": os.path.dirname(here)})
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "record abi ok" in r.stdout


def _junctions(ax=None):
    """24 junctions of the demo's riders from varied starts (demoCSFstandalone.py:101-118): six classes, one junction with a
    custom destination force, one empty, one animated on an Agg canvas"""
    from cyclistsocialforce_amd.intersection import SocialForceIntersection
    from cyclistsocialforce_amd.vehicle import (BalancingRiderBicycle, Bicycle, InvPendulumBicycle, PlanarBicycle, PlanarPointBicycle,
                                                TwoDBicycle)

    def pull(veh):
        dx, dy = 30.0 - veh.s[0], 30.0 - veh.s[1]
        r = np.hypot(dx, dy)
        return 3.5 * dx / r + 0.4, 3.5 * dy / r - 0.2

    kinds = [TwoDBicycle, Bicycle, PlanarPointBicycle, InvPendulumBicycle, PlanarBicycle, BalancingRiderBicycle, TwoDBicycle]
    out = []
    for j in range(24):
        if j == 5:
            out.append(SocialForceIntersection([], id=f"j{j}"))
            continue
        cls = kinds[j % len(kinds)]
        dx, dy = 0.3 * j - 2.0, -0.5 * (j % 3)
        hook = {"dest_force_func": pull} if j == 9 else {}
        a = cls((-6 + dx, dy, 0.02 * j, 5, 0, 0, 0, 0), id="a", saveForces=True, **hook)
        a.params.v_desired_default = 4.5
        b = cls((15 + dx, -20 + dy, np.pi / 2, 5, 0, 0, 0, 0), id="b", saveForces=(j % 2 == 0))
        b.params.v_desired_default = 5.0
        c = cls((13 + dx, -20 - dy, np.pi / 2, 5, 0, 0, 0, 0), id="c", saveForces=True)
        c.params.v_desired_default = 5.0
        a.setDestinations((35, 64, 65), (0, 0, 0))
        b.setDestinations((15, 15, 15), (20, 49, 50))
        c.setDestinations((13, 13, 13), (20, 49, 50))
        kw = {"animate": True, "axes": ax} if (j == 14 and ax is not None) else {}
        out.append(SocialForceIntersection([a, b, c], id=f"j{j}", **kw))
    return out


def _same_vehicles(p, q, what):
    assert p.hist_n_vecs == q.hist_n_vecs, what
    for u, w in zip(p.vehicles, q.vehicles):
        assert np.array_equal(u.s, w.s), what
        assert np.array_equal(u.traj, w.traj), what
        if u.saveForces:
            assert np.array_equal(u.trajF, w.trajF), what
        assert np.array_equal(np.asarray(u.F), np.asarray(w.F)), what
        assert np.array_equal(u.znav, w.znav) and u.destpointer == w.destpointer and u.i == w.i, what


def test_intersections_advanced_together_equal_step_together():
    """150 ticks of 24 junctions through advance_together against 150 calls of step_together, then 3 500 more on a subset (longer
    than traj: 3 000 rows at t_s = 0.01)"""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    from cyclistsocialforce_amd import advance_together, step_together

    _, ax1 = plt.subplots(1, 1)
    _, ax2 = plt.subplots(1, 1)
    L1, L2 = _junctions(ax1), _junctions(ax2)
    for _ in range(150):
        step_together(L1)
    advance_together(L2, 150)
    for j, (p, q) in enumerate(zip(L1, L2)):
        _same_vehicles(p, q, f"junction {j} after 150 ticks")
        assert len(q.hist_n_vecs) == 150
    dense = [q for j, q in enumerate(L2) if j not in (5, 9, 14)]
    assert all(q.engine.batch_ticks() == 150 and q.engine.small_ticks() == 150 for q in dense)
    sub = [0, 2, 3, 5, 9, 11, 12]
    for _ in range(3500):
        step_together([L1[j] for j in sub])
    advance_together([L2[j] for j in sub], 3500)
    for j in sub:
        _same_vehicles(L1[j], L2[j], f"junction {j} after 3 650 ticks")
    plt.close("all")


def test_step_n_dense_equals_single_steps():
    """step_n(150, dense=True) against 150 calls of step(); step_n(150) as before: the final state, one row of traj"""
    a, b, c = _junctions()[:3], _junctions()[:3], _junctions()[:3]
    for p, q, r in zip(a, b, c):
        for _ in range(150):
            p.step()
        q.step_n(100, dense=True)
        q.step_n(50, dense=True)
        r.step_n(150)
        _same_vehicles(p, q, "dense")
        assert q.engine.small_ticks() == 150
        for u, w in zip(p.vehicles, r.vehicles):
            assert np.array_equal(u.s, w.s) and w.i == 150 % 3000
            assert np.array_equal(w.traj[:, 150], u.traj[:, 150]) and not w.traj[:, 1:150].any()
        assert r.hist_n_vecs == p.hist_n_vecs
