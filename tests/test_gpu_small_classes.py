"""The one-wave and the batched tick of small populations of SEVERAL PARAMETER SETS AND VEHICLE CLASSES (include/csf.h: csf_small_classes;
csf_small_classes.hip): with the switch on, up to 32 road users of any sets and classes - an UncontrolledVehicle population
too - are ticked by one wave, and the members of a batch in one further launch.  Against their general-path twins (the same population,
switch off), the golden trajectories of the literal reference, the CPU oracle, and through the mirror.  Needs a real MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import hetero_classes, mixed_classes, shadow_run
from small_classes_common import (GENERAL_TOL, SWAP_MOVED, TICKS, build, case, lacking_rows, oracle_case, oracle_population, single_population,
                                  unc_population)

pytestmark = [pytest.mark.gpu, pytest.mark.auto_variant]


def run_pair(c, ticks=TICKS, road=None):
    """the population with the switch on and its twin, states after every 1-tick call: ([ticks, n, ns], the same, the engines)"""
    a, b = build(c, True, road=road), build(c, False, road=road)
    A, B = [], []
    for _ in range(ticks):
        a.step(1); b.step(1)
        A.append(a.state()); B.append(b.state())
    assert a.small_ticks() == ticks and b.small_ticks() == 0
    assert (a.status() == 0).all() and (b.status() == 0).all()
    return np.array(A), np.array(B), a, b


# ---- 1. the path is taken (this test fails without the feature) -----------------------------------------------------------------
def test_the_path_is_taken_with_the_switch_on_and_only_then():
    for c in (case("a"), unc_population(6)):
        for on in (True, False):
            e = build(c, on)
            e.step(7); e.step(1); e.step(12)
            assert e.small_ticks() == (20 if on else 0), (on, c["s0"].shape)
            assert np.isfinite(e.state()).all() and (e.status() == 0).all()
            e.close()
    # a single set of a rider class keeps small_tick_kernel bit for bit, switch or no switch
    c = single_population()
    a, b = build(c, True), build(c, False)
    a.step(50); b.step(50)
    assert a.small_ticks() == 50 and b.small_ticks() == 50
    assert np.array_equal(a.state(), b.state())
    for u, w in zip(a.forces(), b.forces()):
        assert np.array_equal(u, w)


# ---- 2. against general-path twins ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rule", [("a", 0), ("b", 0), ("c", 0), ("d", 0), ("e", 0), ("f", 0), ("b", 1)])
def test_against_the_general_path_twin(name, rule):
    """40 ticks, every state row after every tick within GENERAL_TOL of the twin; the rows a class lacks exactly 0.  Measured (largest
    deviation over all rows and ticks): see DESIGN.md 4.6e."""
    c = case(name, rule)
    A, B, a, b = run_pair(c)
    dev = float(np.abs(A - B).max())
    print(f"case ({name}) rule {rule}: {c['s0'].shape[0]} road users, {len(c['pods'])} sets: largest deviation from the twin {dev:.2e}")
    lack = lacking_rows(c)
    assert np.all(A[:, lack] == 0.0) and np.all(B[:, lack] == 0.0)
    assert np.isfinite(A).all() and dev <= GENERAL_TOL, dev
    for u, w in zip(a.forces(), b.forces()):                      # the total force of the last tick, against the twin's
        assert np.abs(u - w).max() <= 1e-4 * max(np.abs(w).max(), 1.0)


# ---- 3. the literal reference ---------------------------------------------------------------------------------------------------------
def test_several_vehicle_classes_golden_on_the_one_wave_tick(golden):
    """tests/golden/mixed.npz - 15 vehicles, 5 classes, 10 sets, 250 ticks - with the bounds of
    tests/test_gpu_hetero.py::test_several_vehicle_classes_golden"""
    from cyclistsocialforce_amd.engine import Engine
    g = golden("mixed")
    pods, cls = mixed_classes(g)
    n = g["s0"].shape[0]
    e = Engine(pods[0], n)
    e.small_classes(True)
    e.set_param_classes(pods)
    e.add_agents(g["s0"], g["vdes"])
    e.set_dest_queue(np.arange(n), g["off"], g["dq"], reset=True)
    e.set_agent_class(np.arange(n), cls)
    S, F = g["S"], g["F"]
    extent = max(np.ptp(S[..., 0]), np.ptp(S[..., 1]), 1.0)
    worst = 0.0
    for k in range(1, S.shape[0]):
        e.step(10)
        got = e.state()
        worst = max(worst, np.abs(got[:, :2] - S[k][:, :2]).max() / extent)
        np.testing.assert_allclose(got[:, :2], S[k][:, :2], rtol=0, atol=1e-4 * extent, err_msg=f"sample {k}")
        np.testing.assert_allclose(got[:, 2:], S[k][:, 2:], rtol=0, atol=2e-3, err_msg=f"sample {k}")
        fx, fy = e.forces()
        np.testing.assert_allclose(np.c_[fx, fy], F[k - 1], rtol=0, atol=2e-3 * max(np.abs(F[k - 1]).max(), 1.0))
    assert (e.status() == 0).all() and e.small_ticks() == 10 * (S.shape[0] - 1)
    print(f"mixed.npz on the one-wave tick: worst position deviation / extent = {worst:.3e}")


@pytest.mark.parametrize("model", ["twod", "bicycle", "invpend"])
def test_individual_parameter_sets_golden_on_the_one_wave_tick(golden, model):
    """tests/golden/hetero.npz: four sets dealt over 10 - 16 vehicles of one class, with the bounds of
    tests/test_gpu_hetero.py::test_individual_parameter_sets_golden"""
    from cyclistsocialforce_amd.engine import Engine
    g = golden("hetero")
    pods, cls = hetero_classes(g, model)
    s0 = g[f"{model}_s0"]
    n = s0.shape[0]
    e = Engine(pods[0], n)
    e.small_classes(True)
    e.add_agents(s0, g[f"{model}_vdes"])
    e.set_dest_queue(np.arange(n), g[f"{model}_off"], g[f"{model}_dq"], reset=True)
    e.set_param_classes(pods, cls)
    S, F = g[f"{model}_S"], g[f"{model}_F"]
    extent = max(np.ptp(S[..., 0]), np.ptp(S[..., 1]), 1.0)
    worst = 0.0
    for k in range(1, S.shape[0]):
        e.step(10)
        got = e.state()
        worst = max(worst, np.abs(got[:, :2] - S[k][:, :2]).max() / extent)
        np.testing.assert_allclose(got[:, :2], S[k][:, :2], rtol=0, atol=1e-4 * extent, err_msg=f"{model} sample {k}")
        np.testing.assert_allclose(got[:, 3], S[k][:, 3], rtol=0, atol=2e-3, err_msg=f"{model} speed sample {k}")
        fx, fy = e.forces()
        np.testing.assert_allclose(np.c_[fx, fy], F[k - 1], rtol=0, atol=2e-3 * max(np.abs(F[k - 1]).max(), 1.0))
    assert (e.status() == 0).all() and e.small_ticks() == 10 * (S.shape[0] - 1)
    print(f"hetero.npz {model} on the one-wave tick: worst position deviation / extent = {worst:.3e}")


# ---- 4. the oracle ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [0, 1])
def test_five_riders_of_three_classes_vs_oracle(rule):
    """orc.Population.set_classes, 5 riders twod / bicycle / invpend: the total forces of every tick for 30 ticks within 1e-4 x scale, then
    200 ticks free within 1e-4 x extent (the seed: tests/test_small_classes_host.py::test_the_oracle_is_not_chaotic_on_the_horizon)"""
    c = oracle_case(rule)
    e, pop = build(c, True), oracle_population(c)
    worst = 0.0
    for t in range(30):
        e.step(1); pop.step(1)
        fx, fy = e.forces(); ofx, ofy = pop.forces()
        scale = max(np.hypot(ofx, ofy).max(), 1e-3)
        err = max(np.abs(fx - ofx).max(), np.abs(fy - ofy).max()) / scale
        worst = max(worst, err)
        assert err < 1e-4, (t, err)
    e2, pop2 = build(c, True), oracle_population(c)
    e2.step(200); pop2.step(200)
    got, ref = e2.state(), pop2.state()
    extent = max(np.ptp(ref[:, 0]), np.ptp(ref[:, 1]), 14.0)
    dev = np.abs(got[:, :2] - ref[:, :2]).max() / extent
    print(f"rule {rule}: forces vs oracle {worst:.1e} x scale over 30 ticks; positions after 200 ticks {dev:.1e} x extent")
    assert dev < 1e-4 and e.small_ticks() == 30 and e2.small_ticks() == 200 and (e2.status() == 0).all()


def test_thirty_two_riders_of_six_classes_shadowed_by_the_oracle():
    """case (c) of the twin test: the oracle shadows the engine's uninterrupted run in windows of 10 ticks (conftest.shadow_run)"""
    c = case("c")
    e, pop = build(c, True), oracle_population(c)
    worst, devs, got, ref = shadow_run(e, pop, TICKS, 10)
    print(f"case (c) in windows of 10: |dpos| worst {worst:.1e} m")
    assert worst < 1e-4 * c["box"] and e.small_ticks() == TICKS and (e.status() == 0).all()


# ---- 5. the sets are per road user ----------------------------------------------------------------------------------------------------
def test_the_sets_belong_to_the_road_users():
    c = case("a")
    swapped = dict(c, cls=c["cls"][::-1].copy())                   # the other rider owns the other set
    relabelled = dict(c, pods=c["pods"][::-1], cls=c["cls"][::-1].copy())   # the same owners, the sets numbered the other way round
    out = []
    for q in (c, swapped, relabelled):
        e = build(q, True)
        e.step(TICKS)
        assert e.small_ticks() == TICKS
        out.append(e.state())
    moved = np.abs(out[0][:, :2] - out[1][:, :2]).max(axis=1)
    print(f"the sets swapped between the two riders: moved by {moved} m")
    assert np.all(moved > SWAP_MOVED)
    assert np.array_equal(out[0], out[2])


# ---- 6. calls in between ------------------------------------------------------------------------------------------------------------------
def test_calls_between_steps():
    """set_agent_class, the table shrinking to one set (small_tick_kernel takes over, small_ticks keeps counting) and growing again,
    push_state, a 33rd road user arriving and leaving: the same calls on the twin, GENERAL_TOL at every stop"""
    c = case("d")                                                  # 32 TwoD riders of 32 sets
    a, b = build(c, True, capacity=40), build(c, False, capacity=40)
    pods = c["pods"]
    stops = []

    def stop(label, want_small):
        sa, sb = a.state(), b.state()
        dev = float(np.abs(sa - sb).max())
        stops.append((label, dev))
        assert sa.shape == sb.shape and dev <= GENERAL_TOL, (label, dev)
        assert a.small_ticks() == want_small, (label, a.small_ticks())

    for e in (a, b):
        e.step(5)
    stop("start", 5)
    for e in (a, b):
        e.set_agent_class(np.array([3, 9, 20]), np.array([1, 1, 30]))
        e.step(5)
    stop("set_agent_class", 10)
    for e in (a, b):
        e.set_param_classes(pods[:1], np.zeros(32, dtype=np.int32))   # one set: the rows first, then the table
        e.step(5)
    assert b.small_ticks() == 5                                    # (the twin, one set of a rider class: its own one-wave kernel)
    stop("one set", 15)
    for e in (a, b):
        e.set_param_classes(pods[:4], np.arange(32) % 4)
        e.step(5)
    stop("four sets", 20)
    for e in (a, b):
        s = e.state()
        s[:, 3] *= 0.9
        e.push_state(np.arange(32, dtype=np.int32), s)
        e.step(5)
    stop("push_state", 25)
    for e in (a, b):
        e.add_agents(np.array([[40.0, 40.0, 0.0, 4.0, 0.0]]), 5.0)
        e.set_dest_queue(np.array([32]), np.array([0, 2]), np.array([[40.0, 40.0, 0.0], [90.0, 40.0, 0.0]]), reset=True)
        e.set_agent_class(np.array([32]), np.array([2]))
        e.step(5)
    stop("33 road users", 25)                                      # (the general path)
    for e in (a, b):
        e.remove_agents(np.array([32], dtype=np.int32))
        e.step(5)
    stop("32 again, a dead slot behind them", 25)                  # (as tests/test_gpu_small.py: the slot stays behind)
    assert b.small_ticks() == 5 and (a.status() == 0).all() and (b.status() == 0).all()
    print("; ".join(f"{k}: {v:.1e}" for k, v in stops))


# ---- 7. road ----------------------------------------------------------------------------------------------------------------------------
def test_between_road_edges_with_fractional_sigma():
    c = case("b")
    xs = np.linspace(-20.0, 50.0, 700)
    road = (np.array([0, 700, 1400]), np.r_[np.c_[xs, np.full(700, -3.0)], np.c_[xs, np.full(700, 17.0)]], np.array([0.15, 0.2]), np.array([2.5, 2.5]))
    A, B, a, b = run_pair(c, road=road)
    dev = float(np.abs(A - B).max())
    print(f"case (b) between two road edges, sigma 2.5: largest deviation from the twin {dev:.2e}")
    assert dev <= GENERAL_TOL
    none = build(c, True)
    none.step(TICKS)
    assert np.abs(none.state()[:, :2] - A[-1][:, :2]).max() > 1e-6   # (the road acts)


# ---- 8. recording and read-back ---------------------------------------------------------------------------------------------------------
def test_recording_and_read_back():
    c = case("b")
    a, b = build(c, True), build(c, True)
    for e in (a, b):
        e.record(stride=1, capacity=64, forces=True)
    a.step(34)
    for _ in range(34):
        b.step(1)
    Sa, Fa = a.recorded(0, 34)
    Sb, Fb = b.recorded(0, 34)
    assert np.array_equal(Sa, Sb) and np.array_equal(Fa, Fb) and np.isfinite(Sa).all()
    assert np.array_equal(Sa[-1], a.state()) and np.array_equal(Fa[-1], np.c_[a.forces()])
    assert a.small_ticks() == 34 and b.small_ticks() == 34
    # step_into in one call against step and the getters
    p, q = build(c, True), build(c, True)
    n, ns = p.n, p.ns
    for k in (1, 6, 1, 17):
        s, ptr, zn, fx, fy = np.zeros((n, ns)), np.zeros(n, dtype=np.int32), np.zeros((n, 3), dtype=np.uint8), np.zeros(n), np.zeros(n)
        tick = p.step_into(k, s, ptr, zn, fx, fy)
        q.step(k)
        s2, ptr2, zn2, tick2 = q.state(with_nav=True)
        fx2, fy2 = q.forces()
        assert tick == tick2
        assert np.array_equal(s, s2) and np.array_equal(ptr, ptr2) and np.array_equal(zn.astype(bool), np.asarray(zn2).reshape(n, 3).astype(bool))
        assert np.array_equal(fx, fx2) and np.array_equal(fy, fy2)
    assert p.small_ticks() == 25 and q.small_ticks() == 25


# ---- 9. batch ---------------------------------------------------------------------------------------------------------------------------
def _reseeded(name, k):
    """case `name` on another crowd (the k-th copy of a batch)"""
    from scene_calib_common import crowd
    from small_classes_common import wide
    c = case(name)
    if k == 0:
        return c
    n, ns = c["s0"].shape
    x, y, psi, v, off, dq = crowd(n, seed=5000 + 10 * k + n, box=c["box"])
    if c["script"] is not None:                                    # (the car keeps its line)
        x[4], y[4], psi[4], v[4] = c["s0"][4, :4]
        dq[off[4]: off[5]] = c["dq"][c["off"][4]: c["off"][5]]
    return dict(c, s0=wide(x, y, psi, v, ns), off=off, dq=dq)


def _batch_members(on, with_classes=True):
    from scene_calib_common import crowd
    from small_classes_common import wide
    out, kinds = [], []
    if with_classes:
        xs = np.linspace(-20.0, 34.0, 400)                        # one member between road edges: the launch's LDS is sized by its road
        road = (np.array([0, 400, 800]), np.r_[np.c_[xs, np.full(400, -3.0)], np.c_[xs, np.full(400, 17.0)]], np.array([0.15, 0.2]), np.array([2.5, 2.5]))
        for k in range(3):
            for name in "abef":
                out.append(build(_reseeded(name, k), on, capacity=8, road=road if (name, k) == ("b", 1) else None))
                kinds.append(name)
    for seed in (77, 78):
        out.append(build(single_population(5, seed), on))
        kinds.append("single")
    c = single_population(5)
    x, y, psi, v, off, dq = crowd(33, seed=5, box=30.0)
    out.append(build(dict(c, s0=wide(x, y, psi, v, 5), off=off, dq=dq, cls=np.zeros(33, dtype=np.int32)), on))
    kinds.append("big")
    return out, kinds


def test_batch_of_members_of_several_sets_and_classes():
    """K = 12 members - cases (a), (b), (e), (f) three times over - beside two single-set members and one of 33 riders: every member equals
    its twin stepped alone with the same switch, bit for bit; one further launch per call for all twelve"""
    from cyclistsocialforce_amd.engine import Engine
    batch, kinds = _batch_members(True)
    twins, _ = _batch_members(True)
    plain, _ = _batch_members(True, with_classes=False)            # the same batch without the class members
    Engine.batch_join(batch)
    Engine.batch_join(plain)
    for calls, c in enumerate((1, 5, 1, 20)):
        l0, p0 = batch[0].batch_launches(), plain[0].batch_launches()
        Engine.step_batch(batch, c)
        Engine.step_batch(plain, c)
        for t in twins:
            t.step(c)
        dl, dp = batch[0].batch_launches() - l0, plain[0].batch_launches() - p0
        assert dl == dp + 1, (calls, dl, dp)                       # (the table is one run of slots in both: one copy each)
    for k, a, b in zip(kinds, batch, twins):
        assert np.array_equal(a.state(), b.state()), k
        for u, w in zip(a.forces(), b.forces()):
            assert np.array_equal(u, w), k
    assert [e.batch_ticks() for e in batch] == [0 if k == "big" else 27 for k in kinds]
    assert [e.small_ticks() for e in batch] == [0 if k == "big" else 27 for k in kinds]
    # with the switch off the class members are stepped in turn, as before
    off_batch, kinds = _batch_members(False)
    off_twins, _ = _batch_members(False)
    Engine.batch_join(off_batch)
    for c in (1, 5):
        Engine.step_batch(off_batch, c)
        for t in off_twins:
            t.step(c)
    for k, a, b in zip(kinds, off_batch, off_twins):
        assert np.array_equal(a.state(), b.state()), k
    assert [e.batch_ticks() for e in off_batch] == [6 if k == "single" else 0 for k in kinds]


# ---- 10. the mirror ---------------------------------------------------------------------------------------------------------------------
def _intersection(seed, on):
    from cyclistsocialforce_amd import parameters as P
    from cyclistsocialforce_amd.intersection import SocialForceIntersection
    from cyclistsocialforce_amd.vehicle import Bicycle, TwoDBicycle
    from scene_calib_common import crowd
    x, y, psi, v, off, dq = crowd(4, seed=seed)
    bikes = []
    for k in range(4):
        if k < 3:
            b = TwoDBicycle((x[k], y[k], psi[k], v[k], 0.0), id=str(k), params=P.InvPendulumBicycleParameters(hfov=1.5 + 0.5 * k, f_0=6.0 + k))
        else:
            b = Bicycle((x[k], y[k], psi[k], v[k], 0.0), id=str(k))
        rows = dq[off[k] + 1: off[k + 1]]
        b.setDestinations(rows[:, 0], rows[:, 1])
        bikes.append(b)
    ins = SocialForceIntersection(bikes)
    ins.set_small_classes(on)
    return ins, bikes


def test_through_the_mirror():
    """three TwoDBicycles with their own params= and one Bicycle: step() x 50 with the method on against the same with it off, and
    advance_together on four such intersections"""
    from cyclistsocialforce_amd.intersection import advance_together
    (ia, ba), (ib, bb) = _intersection(3020, True), _intersection(3020, False)
    for _ in range(50):
        ia.step(); ib.step()
    assert ia.engine.small_ticks() == 50 and ib.engine.small_ticks() == 0
    dev = max(float(np.abs(np.asarray(u.s) - np.asarray(w.s)).max()) for u, w in zip(ba, bb))
    print(f"the mirror, step() x 50: largest deviation {dev:.2e}")
    assert dev <= GENERAL_TOL
    seeds = (3020, 3033, 3014, 3045)
    on = [_intersection(s, True) for s in seeds]
    off = [_intersection(s, False) for s in seeds]
    advance_together([i for i, _ in on], 30)
    advance_together([i for i, _ in off], 30)
    for (i1, b1), (i2, b2) in zip(on, off):
        assert i1.engine.small_ticks() == 30 and i1.engine.batch_ticks() == 30 and i2.engine.small_ticks() == 0
        dev = max(float(np.abs(np.asarray(u.s) - np.asarray(w.s)).max()) for u, w in zip(b1, b2))
        assert dev <= GENERAL_TOL, dev
        for u, w in zip(b1, b2):
            assert u.traj.shape == w.traj.shape


# ---- the C ABI's refusals and the environment knobs, once, in a fresh process -----------------------------------------------------------
def test_abi_refusals_and_environment_knobs():
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "small_classes_abi_child.py")
    env = {k: v for k, v in os.environ.items() if k not in ("CSF_SMALL_CLASSES", "CSF_FUSED_SMALL", "CSF_PAIR_VARIANT")}
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "small classes abi ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
