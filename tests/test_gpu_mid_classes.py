"""The one-launch tick of mid-size populations of SEVERAL PARAMETER SETS AND VEHICLE CLASSES (include/csf.h: csf_mid_classes;
csf_mid_classes.hip): with the switch on, 33 ... 1 024 road users of any sets and of six classes - scripted
UncontrolledVehicles among them, no BalancingRiderBicycle - are ticked in ONE launch per tick, alone and as members of a batch.  Against
their general-path twins (the same population, switch off), against the CPU oracle from a common state and in shadowed windows, bit for bit
against themselves, with the road term inside the launch, across calls that change the population, and in a batch.  Needs a real MI355X.

Shapes: 33 (groups of 4, the last holds one live slot, one batch of 64 sources), 40, 65 (a second, nearly empty source batch), 257, 600;
2 sets, 33 riders of 33 sets, 257 riders over the full table of 256 sets, five classes / ten sets, four classes and scripted cars."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import hetero_classes, mixed_classes, shadow_run  # noqa: F401  (the suite's own helpers: one copy)
from mid_classes_common import (CASES, DEAD, DEAD_FORCE_CASES, FORCE_TOL, POS_TOL, ROW_TOL, TICKS, TWIN_CASES, WINDOW, build, lacking_rows,
                                oracle_population, population, road_of)
from scene_calib_common import VDES

pytestmark = [pytest.mark.gpu, pytest.mark.auto_variant]


def queues_ahead(s):
    """destination queues of arrivals as scene_calib_common.crowd makes them: the own position, then 8, 25, 60 and 61 m ahead, the last a stop"""
    reach = np.array([0.0, 8.0, 25.0, 60.0, 61.0])
    dq = np.zeros((len(s), 5, 3))
    dq[:, :, 0] = s[:, 0, None] + reach * np.cos(s[:, 2, None])
    dq[:, :, 1] = s[:, 1, None] + reach * np.sin(s[:, 2, None])
    dq[:, 4, 2] = 1.0
    return np.arange(len(s) + 1) * 5, dq.reshape(-1, 3)


def same_bits(a, b, what=""):
    assert np.array_equal(a.state(), b.state()), what
    for u, w in zip(a.forces(), b.forces()):
        assert np.array_equal(u, w), what
    assert np.array_equal(a.status(), b.status()), what


# ---- 1. the path is taken, and only then (this test fails without the feature) -------------------------------------------------------------
def test_the_path_is_taken_with_the_switch_on_and_only_then():
    for c in (population("two", 40), population("five", 257)):
        for on in (True, False):
            e = build(c, on)
            e.step(7); e.step(1); e.step(12)
            assert e.mid_classes_ticks() == (20 if on else 0), (on, c["kind"])
            assert e.mid_ticks() == (20 if on else 0), (on, c["kind"])
            assert np.isfinite(e.state()).all() and (e.status() == 0).all()
            e.close()
    # one set of a rider class keeps mid_tick_kernel bit for bit, switch or no switch
    c = population("one", 64)
    a, b = build(c, True), build(c, False)
    a.step(20); b.step(20)
    assert a.mid_ticks() == 20 and b.mid_ticks() == 20 and a.mid_classes_ticks() == 0
    same_bits(a, b)
    # 300 road users of ONE class keep the general path (tick.inc: measured slower there) - unless the launch sums their road term too
    c = population("two", 300)
    e, r = build(c, True), build(c, True, road=road_of(c["box"], 320), mid_road=True)
    e.step(5); r.step(5)
    assert (e.mid_classes_ticks(), e.mid_ticks(), r.mid_classes_ticks(), r.mid_road_ticks()) == (0, 0, 5, 5)
    # 32 road users and fewer are the one-wave tick's range (csf_small_classes): this switch leaves them where they were
    e = build(population("two", 32), True)
    e.step(5)
    assert e.mid_classes_ticks() == 0 and e.mid_ticks() == 0
    # a population of scripted UncontrolledVehicles alone takes the path too, and every car is where its script says
    c = population("unc", 40)
    e = build(c, True)
    e.step(20)
    idx, offs, rows = c["script"]
    assert e.mid_classes_ticks() == 20 and (e.status() == 0).all()
    np.testing.assert_allclose(e.state()[:, :4], rows[offs[:-1] + 20], rtol=0, atol=1e-12)
    # a BalancingRider set keeps the general path
    e = build(population("br", 40), True)
    e.step(5)
    assert e.mid_classes_ticks() == 0 and e.mid_ticks() == 0 and np.isfinite(e.state()).all()


# ---- 2. forces against the general-path twin and the oracle, from a common state ----------------------------------------------------------------
@pytest.mark.parametrize("kind,n,rule", CASES)
def test_forces_against_the_twin_and_the_oracle(kind, n, rule):
    """the total forces of the first tick within FORCE_TOL x the largest force of the twin, and of orc.Population.set_classes"""
    c = population(kind, n, rule)
    a, b, pop = build(c, True), build(c, False), oracle_population(c)
    a.step(1); b.step(1); pop.step(1)
    assert a.mid_classes_ticks() == 1 and b.mid_classes_ticks() == 0
    fa, fb, fo = np.c_[a.forces()], np.c_[b.forces()], np.c_[pop.forces()]
    et = np.abs(fa - fb).max() / max(np.hypot(fb[:, 0], fb[:, 1]).max(), 1.0)
    eo = np.abs(fa - fo).max() / max(np.hypot(fo[:, 0], fo[:, 1]).max(), 1.0)
    print(f"{kind} {n} rule {rule}: forces of one tick vs the twin {et:.1e}, vs the oracle {eo:.1e} (x the largest force)")
    assert et < FORCE_TOL and eo < FORCE_TOL, (et, eo)
    assert (a.status() == 0).all() and a.near_dropped() == 0


@pytest.mark.parametrize("kind,n,rule", DEAD_FORCE_CASES)
def test_forces_against_the_twin_with_dead_slots_and_poisoned_slack(monkeypatch, kind, n, rule):
    """the same against the twin with road users removed from the middle (37 slots with 33 road users alive: the group of slot 36 holds one
    live slot) and 0xFF
    bytes behind every array"""
    monkeypatch.setenv("CSF_DEBUG_POISON", "1")
    c = population(kind, n, rule)
    a, b = build(c, True, dead=DEAD), build(c, False, dead=DEAD)
    a.step(1); b.step(1)
    assert a.mid_classes_ticks() == 1 and a.n == n - len(DEAD)
    fa, fb = np.c_[a.forces()], np.c_[b.forces()]
    et = np.abs(fa - fb).max() / max(np.hypot(fb[:, 0], fb[:, 1]).max(), 1.0)
    print(f"{kind} {n} rule {rule}, {len(DEAD)} dead slots: forces of one tick vs the twin {et:.1e}")
    assert np.isfinite(fa).all() and et < FORCE_TOL, et


# ---- 3. trajectories ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,rule", CASES)
def test_trajectories_shadowed_by_the_oracle(kind, n, rule):
    """50 ticks uninterrupted, the oracle shadowing in windows of 10 (conftest.shadow_run): positions within POS_TOL x box, headings and the
    further rows within the bounds of tests/test_gpu_hetero.py::test_random_mixed_population_vs_oracle; rows a class lacks exactly 0; a
    scripted UncontrolledVehicle where its script says to 1e-12"""
    c = population(kind, n, rule)
    e, pop = build(c, True), oracle_population(c)
    worst, devs, got, ref = shadow_run(e, pop, TICKS, WINDOW)
    print(f"{kind} {n} rule {rule}: {TICKS} ticks in windows of {WINDOW}: |dpos| worst {worst:.1e} m = {worst / c['box']:.1e} x box")
    assert worst < POS_TOL * c["box"] and e.mid_classes_ticks() == TICKS and (e.status() == 0).all() and e.near_dropped() == 0
    dd = np.abs((got[:, 2:6] - ref[:, 2:6] + np.pi) % (2 * np.pi) - np.pi)
    off = (dd > ROW_TOL[: dd.shape[1]]).any(axis=1)
    assert off.sum() == 0, (np.where(off)[0], dd[off])
    assert np.all(got[lacking_rows(c)] == 0.0)
    if c["script"] is not None:
        idx, offs, rows = c["script"]
        np.testing.assert_allclose(got[idx, :4], rows[offs[:-1] + TICKS], rtol=0, atol=1e-12)


@pytest.mark.parametrize("kind,n,rule,dead", TWIN_CASES)
def test_trajectories_against_the_twin(kind, n, rule, dead):
    """10 one-tick calls from a common state: positions within POS_TOL x box of the general path's.  Measured: DESIGN.md 4.7c"""
    c = population(kind, n, rule)
    a, b = build(c, True, dead=dead), build(c, False, dead=dead)
    dev = 0.0
    for _ in range(10):
        a.step(1); b.step(1)
        sa, sb = a.state(), b.state()
        dev = max(dev, float(np.abs(sa[:, :2] - sb[:, :2]).max()))
    print(f"{kind} {n} rule {rule}, {len(dead)} dead: largest deviation from the twin over 10 ticks {dev:.2e} m = {dev / c['box']:.1e} x box")
    assert a.mid_classes_ticks() == 10 and b.mid_classes_ticks() == 0 and b.mid_ticks() == 0
    assert np.isfinite(sa).all() and dev < POS_TOL * c["box"]
    assert (a.status() == 0).all() and (b.status() == 0).all()


# ---- 4. bit-reproducibility ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,rule", [("five", 257, 1), ("cars", 65, 0)])
def test_bit_reproducible(monkeypatch, kind, n, rule):
    """the same population stepped twice gives the same bits (a receiver's partial sums are added in item order, whoever took which item), and
    one call of 37 ticks is 37 calls of one"""
    monkeypatch.setenv("CSF_DEBUG_POISON", "1")
    c = population(kind, n, rule)
    a, b, one = build(c, True, dead=DEAD), build(c, True, dead=DEAD), build(c, True, dead=DEAD)
    a.step(37); b.step(37)
    for _ in range(37):
        one.step(1)
    same_bits(a, b, "run twice")
    same_bits(a, one, "37 ticks in one call against 37 calls")
    assert a.mid_classes_ticks() == 37 and one.mid_classes_ticks() == 37


# ---- 5. road --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("verts", [320, 1100])
@pytest.mark.parametrize("n", [33, 257])
def test_the_road_term_inside_the_launch(n, verts):
    """csf_mid_road on as well: state, forces and status bit for bit those of the same population with road_kernel in front of the launch"""
    c = population("five", n, 0)
    road = road_of(c["box"], verts)
    a, b, none = build(c, True, road=road, mid_road=True), build(c, True, road=road), build(c, True)
    for k in (7, 1, 12):
        a.step(k); b.step(k)
    none.step(20)
    same_bits(a, b)
    assert a.mid_road_ticks() == 20 and b.mid_road_ticks() == 0 and a.mid_classes_ticks() == 20 and b.mid_classes_ticks() == 20
    assert np.abs(none.state()[:, :2] - a.state()[:, :2]).max() > 1e-9   # (the road acts)


# ---- 6. calls in between ------------------------------------------------------------------------------------------------------------------------
def test_calls_between_steps(monkeypatch):
    """set_agent_class, the table going from 4 sets to 1 (mid_tick_kernel takes over) and back, push_state, a departure and an arrival into the
    freed slot, growing past the population bound (CSF_MID_BELOW = 48 here: the general path) and shrinking to 32 (below the path's range: the
    general path still): the same calls on the twin,
    the expected path by the counters, the states within the twin bound at every stop"""
    monkeypatch.setenv("CSF_MID_BELOW", "48")
    c = population("sets", 40, 0)
    pods = c["pods"]
    c = dict(c, pods=pods[:4], cls=c["cls"] % 4)
    a, b = build(c, True, capacity=64), build(c, False, capacity=64)
    stops = []

    def stop(label, want_classes, want_mid):
        sa, sb = a.state(), b.state()
        dev = float(np.abs(sa[:, :2] - sb[:, :2]).max())
        stops.append((label, dev))
        assert sa.shape == sb.shape and dev < POS_TOL * c["box"], (label, dev)
        assert (a.mid_classes_ticks(), a.mid_ticks()) == (want_classes, want_mid), (label, a.mid_classes_ticks(), a.mid_ticks())
        assert (a.status() == 0).all() and (b.status() == 0).all(), label

    for e in (a, b):
        e.step(10)
    stop("start", 10, 10)
    for e in (a, b):
        e.set_agent_class(np.array([3, 9, 20]), np.array([1, 1, 2]))
        e.step(10)
    stop("set_agent_class", 20, 20)
    for e in (a, b):
        e.set_param_classes(pods[:1], np.zeros(40, dtype=np.int32))   # one set of a rider class: mid_tick_kernel, on both
        e.step(10)
    assert b.mid_ticks() == 10
    stop("one set", 20, 30)
    for e in (a, b):
        e.set_param_classes(pods[:4], np.arange(40) % 4)
        e.step(10)
    stop("four sets", 30, 40)
    for e in (a, b):
        s = e.state()
        s[:, 3] *= 0.9
        e.push_state(np.arange(40, dtype=np.int32), s)
        e.step(10)
    stop("push_state", 40, 50)
    arrival = np.zeros((1, a.ns)); arrival[0, :4] = [12.0, 9.0, 0.4, 4.0]
    for e in (a, b):
        e.replace_agents(np.array([7], dtype=np.int32), arrival, VDES, *queues_ahead(arrival))
        e.set_agent_class(np.array([39]), np.array([3]))
        e.step(10)
    assert a.n == 40
    stop("a departure and an arrival", 50, 60)
    more = np.zeros((10, a.ns))
    more[:, 0], more[:, 1], more[:, 2], more[:, 3] = np.linspace(2.0, 28.0, 10), -4.0, 1.5, 4.0
    offs, rows = queues_ahead(more)
    for e in (a, b):
        e.add_agents(more, VDES)
        e.set_dest_queue(np.arange(40, 50), offs, rows, reset=True)
        e.set_agent_class(np.arange(40, 50), np.arange(10) % 4)
        e.step(10)
    stop("50 road users: past the bound, the general path", 50, 60)
    for e in (a, b):
        e.remove_agents(np.arange(32, 50, dtype=np.int32))
        e.step(10)
    assert a.n == 32
    # (32 road users alive among 50 slots: the one-wave tick wants a population without dead slots - tests/test_gpu_small_classes.py -, and
    # the one-launch tick of mixed populations begins at 33 road users: the general path)
    stop("32 alive among 50 slots", 50, 60)
    assert b.mid_classes_ticks() == 0 and b.mid_ticks() == 10
    print("; ".join(f"{k}: {v:.1e}" for k, v in stops))


# ---- 7. batch -------------------------------------------------------------------------------------------------------------------------------------
MEMBERS = [("two", 33, 0, 0), ("five", 40, 0, 0), ("cars", 65, 0, 0), ("sets", 100, 0, 0), ("five", 120, 1, 0), ("two", 64, 1, 0),
           ("five", 50, 0, 320), ("cars", 90, 0, 320), ("sets", 33, 1, 1100), ("five", 77, 1, 0), ("one", 64, 0, 0), ("br", 40, 0, 0)]


def _members(roads=True):
    out = []
    for j, (kind, n, rule, verts) in enumerate(MEMBERS):
        c = population(kind, n, rule, seed=8200 + j)
        road = road_of(c["box"], verts) if verts and roads else None
        out.append(build(c, True, road=road, mid_road=True))
    return out


def _change(k, j, e):
    """change k of member j - the same on the member and on its twin: sets dealt anew, a road replaced"""
    kind, n, rule, verts = MEMBERS[j]
    if kind in ("two", "sets", "five") and (j + k) % 2 == 0:
        idx = np.arange(0, n, 3)
        cls = np.asarray(population(kind, n, rule, seed=8200 + j)["cls"])
        e.set_agent_class(idx, np.roll(cls, k + 1)[idx])
    if verts and k == 2:
        e.set_road(*road_of(0.9 * max(30.0, 3.2 * np.sqrt(n)), verts + 64))


def test_batch_of_mixed_mid_size_members():
    """twelve members - 33 ... 120 road users, classes and sets differing, both rules, three with roads, one uniform, one with a BalancingRider
    set - in calls of 50, 1, 1, 37 ticks, sets and roads changing in between: every member bit for bit its twin stepped alone with the same
    switches"""
    from cyclistsocialforce_amd.engine import Engine
    batch, twins = _members(), _members()
    Engine.batch_join(batch)
    for k, ticks in enumerate((50, 1, 1, 37)):
        Engine.step_batch(batch, ticks)
        for t in twins:
            t.step(ticks)
        for j, (x, y) in enumerate(zip(batch, twins)):
            same_bits(x, y, f"call {k}, member {j} {MEMBERS[j]}")
        if k in (0, 2):
            for j in range(len(MEMBERS)):
                _change(k, j, batch[j]); _change(k, j, twins[j])
    for j, (x, y) in enumerate(zip(batch, twins)):
        kind, n, rule, verts = MEMBERS[j]
        what = f"member {j} {MEMBERS[j]}"
        assert y.batch_mid_ticks() == 0 and x.mid_ticks() == y.mid_ticks() and x.mid_classes_ticks() == y.mid_classes_ticks(), what
        if kind == "br":
            assert x.batch_mid_ticks() == 0 and x.mid_ticks() == 0, what
        else:
            assert x.batch_mid_ticks() == 89 and x.mid_ticks() == 89, what
            assert x.mid_classes_ticks() == (0 if kind == "one" else 89), what
            assert x.mid_road_ticks() == (89 if verts else 0), what


def test_launches_do_not_grow_with_the_number_of_mixed_members():
    """4 and 12 mixed members of one rule without roads, 64 ticks in one call: the same number of launches and copies - ONE launch per tick
    whatever the members' classes"""
    from cyclistsocialforce_amd.engine import Engine
    kinds = ["two", "five", "cars", "sets"]
    counts = []
    for K in (4, 12):
        es = [build(population(kinds[j % 4], 40 + 7 * j, 0, seed=8300 + j), True) for j in range(K)]
        Engine.batch_join(es)
        Engine.step_batch(es, 64, sync=True)
        assert all(e.batch_mid_ticks() == 64 and e.mid_classes_ticks() == 64 for e in es)
        counts.append(es[0].batch_launches())
        for e in es:
            e.close()
    print("launches and copies for 64 ticks, 4 and 12 mixed members:", counts)
    assert counts[0] == counts[1] and 64 <= counts[0] <= 64 + 16, counts


# ---- 8. wrong calls, once, in a fresh process -------------------------------------------------------------------------------------------------
def test_abi_refusals_and_environment_knob():
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mid_classes_abi_child.py")
    env = {k: v for k, v in os.environ.items() if k not in ("CSF_MID_CLASSES", "CSF_FUSED_MID", "CSF_PAIR_VARIANT", "CSF_MID_BELOW")}
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mid classes abi ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
