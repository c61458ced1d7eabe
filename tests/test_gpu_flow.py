"""Flow on the MI355X (include/csf.h: csf_flow, csf_batch_flow; csf_flow.hip) against the definition in NumPy fp64
(tests/flow_common.py), applied to the states read back with Engine.recorded: engine and reference start from identical bits.

The comparison is BIT FOR BIT - every array of a result, the counters and the events - and no cell is left out.  That is derivable,
not measured: every input is the ring's fp64 bits, every operation is one IEEE operation in a stated order without contraction,
sqrt and division are correctly rounded, no transcendental is involved, every aggregate but in_dist is an integer, and in_dist is a
sequential sum in a stated order.

The layout is flow_common.layout's, relative to the side b of the box the riders start in: five lines - x = b/2, y = b/2 (pointing
west), the diagonal, a short one, and one at 2b that nobody reaches -, three areas - along y = b/2, along the diagonal, and one at 3b
that stays empty - and a grid of 8 x 8 cells over the box.  Every case from 33 riders up asserts from the reference alone that it is
not vacuous: crossings in both directions on each of the first three lines, at least one sign change on the short line refused by
the extent test, road users that enter or leave each of the first two areas, and samples outside the grid.  The hand-placed cases
assert at least one crossing.  What the reference finds on the engine's trajectories (seed 0; crossings of the first three lines by
direction, sign changes on the short line refused for the extent, riders entering or leaving the first two areas, samples outside
the grid): 33 riders 2 + 6, 1 + 3, 2 + 4; 3; 5, 8; 57 of 264 - 70: 2 + 6, 3 + 3, 5 + 4; 5; 11, 17; 100 of 560 - 257: 9 + 5, 3 + 10,
12 + 15; 11; 22, 22; 197 of 2 056 - 300: 5 + 6, 6 + 8, 8 + 12; 12; 25, 23; 198 of 2 400 - 1 100: 12 + 11, 14 + 7, 22 + 23; 23; 44, 60;
454 of 8 800.  No line or area had to be moved."""
import ctypes as C

import numpy as np
import pytest

import flow_common as fc

pytestmark = pytest.mark.gpu

INF = float("inf")
NAN = float("nan")
STRIDE = 20                     # x t_s = 0.01 s: a sample every 0.2 s
SAMPLES = 8
BOX = {33: 20.0, 70: 30.0, 257: 60.0, 300: 60.0, 1100: 100.0}     # (test_gpu_pet.py's)
SEED = 0


@pytest.fixture(scope="module")
def amd():
    from cyclistsocialforce_amd import _ffi, engine, parameters

    class NS:
        pass

    ns = NS()
    ns.Engine, ns.pod, ns.ffi, ns.engine = engine.Engine, parameters.default_pod, _ffi, engine
    return ns


def layout_of(n, box=None):
    """the layout of a population: the box's for the scattered ones; for the riders placed by hand (x = 0 ... 10, y = -1.5 ... 1) a
    box of 12 m whose lines they cross, moved so that the paths lie inside it"""
    if n <= 3:
        lines, areas, grid = fc.layout(12.0)
        lines[:, [0, 2]] -= 1.0
        lines[:, [1, 3]] -= 6.0
        areas[:, [0, 2]] -= 1.0
        areas[:, [1, 3]] -= 6.0
        return lines, areas, (-1.0, -6.0, grid[2], 8, 8)
    return fc.layout(box or BOX[n])


def crowd(amd, n, box=None, seed=SEED, ring=SAMPLES, stride=STRIDE, s0=None, history=False):
    """n road users scattered in a box (two or three: placed by hand), riding towards destinations ahead of them; ring: the capacity
    of a state ring of every `stride`-th tick (None: no recording; history: csf_enable_history's ring instead of csf_record's)"""
    pod = amd.pod("twod")
    ns = amd.ffi.N_STATES[pod.model]
    if s0 is None:
        s0 = fc.placed(n, ns=ns) if n in (2, 3) else fc.scatter(n, box or BOX.get(n, 6.0), seed, ns=ns)
    vdes = s0[:, 3].copy() if n in (2, 3) else 5.0               # (the placed riders keep their speeds: a slow one stays slow)
    e = amd.Engine(pod, max(n, 1))
    e.add_agents(s0, vdes)
    e.set_dest_queue(np.arange(n), *fc.with_queue(s0), reset=True)
    if ring and history:
        e.enable_history(stride=stride, capacity=ring)
    elif ring:
        e.record(stride=stride, capacity=ring, forces=False)
    return e


def recorded_crowd(amd, n, **kw):
    e = crowd(amd, n, **kw)
    e.step(kw.get("stride", STRIDE) * SAMPLES)
    return e


def not_vacuous(ref, n, what=""):
    both = ref.line_count.sum(0)                                  # [L, 2]
    c = ref.occupancy.shape[0]
    passing_through = ((ref.in_samples > 0) & (ref.in_samples < c)).sum(0)
    print(f"{what}: {n} riders, crossings by line and direction {both.tolist()}, sign changes refused for the extent {ref.refused.tolist()}, "
          f"riders entering or leaving an area {passing_through.tolist()}, {ref.n_outside} of {ref.n_exist} samples outside the grid")
    assert len(ref.crossings) >= 1, "vacuous: the reference finds no crossing"
    if n >= 33:
        assert (both[:3] >= 1).all(), f"vacuous: crossings by line and direction {both[:3].tolist()}"
        assert ref.refused[3] >= 1, f"vacuous: no sign change on the short line is refused for its extent ({ref.refused.tolist()})"
        assert (passing_through[:2] >= 1).all(), f"vacuous: riders entering or leaving the areas {passing_through.tolist()}"
        assert ref.n_outside >= 1, "vacuous: no sample outside the grid"
        assert both[4].sum() == 0 and ref.in_samples[:, 2].sum() == 0      # the line nobody reaches, the area that stays empty


def same_bits(got, ref, what=""):
    """every array of a Flow against the reference's (or another Flow's): the same bits, NaN where NaN"""
    for f in fc.ARRAYS:
        g, w = getattr(got, f), getattr(ref, f)
        if g is None or w is None:
            assert g is None and w is None, (what, f)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f, g.dtype, w.dtype, g.shape, w.shape)
        if not np.array_equal(g, w, equal_nan=g.dtype.kind == "f"):
            bad = np.argwhere(~((g == w) | ((g != g) & (w != w))))
            raise AssertionError(f"{what}: {f} differs in {len(bad)} of {g.size} cells, first {bad[:4].tolist()}: "
                                 + ", ".join(f"{g[tuple(b)]!r} ({np.asarray(g[tuple(b)]).tobytes().hex()}) against {w[tuple(b)]!r} ({np.asarray(w[tuple(b)]).tobytes().hex()})" for b in bad[:4]))
    assert got.n_outside == ref.n_outside, (what, got.n_outside, ref.n_outside)


def same_events(ev, ref_ev):
    assert ev.dtype == ref_ev.dtype and len(ev) == len(ref_ev)
    for f in ev.dtype.names:
        assert np.array_equal(ev[f], ref_ev[f]), f


def invariants(r, n, n_exist):
    """what holds of every result with events"""
    rows, L = r.line_count.shape[:2]
    assert np.array_equal(r.line_count.sum(0), r.cross_n.sum(0))
    assert r.n_events == int(r.line_count.sum()) == len(r.events)
    assert np.array_equal(fc.binned(r.events, rows, L), r.line_count)
    t, u, v, d = fc.earliest(r.events, n, L)
    assert np.array_equal(t, r.first_t) and np.array_equal(u, r.first_u, equal_nan=True) and np.array_equal(v, r.first_speed, equal_nan=True)
    assert np.array_equal(d, r.first_dir)
    assert np.array_equal(r.occupancy.sum(0), r.in_samples.sum(0))
    assert int(r.grid_count.sum()) + r.n_outside == n_exist


def check(e, first, count, what, vacuous=True, states=None, box=None):
    """flow(first, count, with events) against the reference on recorded(first, count); returns both"""
    S = e.recorded(first, count)[0] if states is None else states
    lines, areas, grid = layout_of(e.n, box)
    ref = fc.reference(S, lines, areas, grid)
    if vacuous:
        not_vacuous(ref, e.n, what)
    r = e.flow(first, count, lines, areas, grid, events=True)
    assert r.first == first
    same_bits(r, ref, what=what)
    same_events(r.events, fc.events(ref))
    invariants(r, e.n, ref.n_exist)
    return r, ref


# ---- 1, 2: against NumPy, not vacuous, the invariants ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 33, 70, 257, 300, 1100])
def test_against_numpy(amd, n):
    """one rider; the head-on pair and the slow rider ahead on the packed path; 33: the first size of the tiled path, one tile with
    a tail; 70 above a wave; 257 and 300 across the tile boundary; 1 100: five tiles"""
    e = recorded_crowd(amd, n)
    r, ref = check(e, 0, SAMPLES, f"n = {n}", vacuous=n > 1)
    assert r.line_count.shape == (SAMPLES - 1, 5, 2) and r.cross_n.shape == (n, 5, 2) and r.first_t.shape == (n, 5)
    assert r.occupancy.shape == (SAMPLES, 3) and r.in_dist.shape == (n, 3) and r.grid_count.shape == (8, 8)
    assert r.period == pytest.approx(0.2) and r.lines.shape == (5, 4) and r.areas.shape == (3, 5) and r.grid[3:] == (8, 8)
    if n in (2, 3):
        assert (ref.line_count.sum(0)[0] >= 1).all()             # the line across the road: the two that meet cross it, one each way
    # the helpers, on the device's arrays
    assert np.array_equal(r.cumulative(0)[-1], r.line_count[:, 0].sum(0)) and r.flow(0, 0.2).sum() == pytest.approx(r.line_count[:, 0].sum() / 1.4)
    assert np.array_equal(np.isnan(r.travel_time(0, 1, 0.2)), ~(np.isfinite(r.first_t[:, 0]) & np.isfinite(r.first_t[:, 1])))
    assert r.headways(0, 0.2).size == max(int(r.line_count[:, 0].sum()) - 1, 0) and r.density(0).shape == (SAMPLES,)
    # without events, and with a part of the layout alone: the same bits
    lines, areas, grid = layout_of(n)
    plain = e.flow(0, SAMPLES, lines, areas, grid)
    assert plain.events is None and plain.n_events == r.n_events
    same_bits(plain, r)
    part = e.flow(0, SAMPLES, lines=lines[1:3])
    assert part.occupancy.shape == (SAMPLES, 0) and part.in_dist.shape == (n, 0) and part.grid_count is None and part.n_outside == 0
    assert np.array_equal(part.line_count, r.line_count[:, 1:3]) and np.array_equal(part.first_t, r.first_t[:, 1:3])
    part = e.flow(0, SAMPLES, areas=areas[1:2], grid=grid)
    assert part.line_count.shape == (SAMPLES - 1, 0, 2) and part.n_events == 0 and np.array_equal(part.grid_count, r.grid_count)
    assert np.array_equal(part.in_dist, r.in_dist[:, 1:2]) and np.array_equal(part.occupancy, r.occupancy[:, 1:2])
    none = e.flow(0, SAMPLES)                                    # L = R = nx = 0
    assert none.line_count.shape == (SAMPLES - 1, 0, 2) and none.grid_count is None and none.n_events == 0 and none.n_outside == 0


# ---- 3. a sub-window ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 70])
def test_a_sub_window(amd, n):
    e = recorded_crowd(amd, n)
    lay = layout_of(n)
    full = e.flow(0, SAMPLES, *lay, events=True)
    sub = e.flow(2, 4, *lay, events=True)
    assert sub.first == 2 and sub.line_count.shape == (3, 5, 2) and sub.occupancy.shape == (4, 3)
    assert np.array_equal(sub.line_count, full.line_count[2:5]) and np.array_equal(sub.occupancy, full.occupancy[2:6])
    inside = full.events[(full.events["k"] >= 2) & (full.events["k"] < 5)]
    assert len(inside) == len(sub.events) >= 1
    for f in ("i", "l", "dir", "u", "speed"):
        assert np.array_equal(sub.events[f], inside[f]), f
    assert np.array_equal(sub.events["k"] + 2, inside["k"])      # (t counts from the call's first sample: k + t against (k - 2) + t)
    assert np.allclose(sub.events["t"] + 2.0, inside["t"], rtol=0, atol=1e-12)
    ref = fc.reference(e.recorded(2, 4)[0], *lay)
    same_bits(sub, ref)
    same_events(sub.events, fc.events(ref))
    for count in (0, 1):                                         # no interval
        one = e.flow(2, count, *lay, events=True)
        ref = fc.reference(e.recorded(2, count)[0], *lay)
        assert one.line_count.shape == (0, 5, 2) and one.occupancy.shape == (count, 3) and one.n_events == 0 and len(one.events) == 0
        assert np.isinf(one.first_t).all() and np.isnan(one.first_u).all() and (one.first_dir == 0).all() and (one.in_dist == 0.0).all()
        assert int(one.grid_count.sum()) + one.n_outside == count * n
        same_bits(one, ref)
    two = e.flow(2, 2, *lay, events=True)                        # one interval
    same_bits(two, fc.reference(e.recorded(2, 2)[0], *lay))


# ---- 4. non-finite -----------------------------------------------------------------------------------------------------------------------
def test_a_rider_whose_x_becomes_nan(amd):
    n = 70
    probe = recorded_crowd(amd, n)                               # the rider is one that, left alone, is inside the first area at sample 4 or later
    lay = layout_of(n)
    ref0 = fc.reference(probe.recorded(0, SAMPLES)[0], *lay)
    late = np.nonzero((ref0.in_last[:, 0] >= 4) | (ref0.first_t.min(axis=1) >= 3.0) & np.isfinite(ref0.first_t.min(axis=1)))[0]
    assert late.size >= 1
    gone = int(late[0])
    e = crowd(amd, n)
    e.step(4 * STRIDE)
    bad = e.state()[gone].copy()
    bad[0] = np.nan
    e.push_state([gone], bad)
    e.step(4 * STRIDE)
    S, _ = e.recorded(0, SAMPLES)
    assert np.isnan(S[4:, gone, 0]).all() and np.isfinite(S[:4, gone, 0]).all()
    r, ref = check(e, 0, SAMPLES, "n = 70, one rider NaN from sample 4 on", vacuous=False)
    assert len(ref.crossings) >= 1 and ref.n_exist == SAMPLES * n - 4
    assert (r.in_last[gone] < 4).all() and not ((r.events["i"] == gone) & (r.events["k"] >= 3)).any()
    quiet = fc.reference(S[:4], *lay)                            # what the rider did in its four samples is all it did
    assert np.array_equal(r.in_samples[gone], quiet.in_samples[gone]) and np.array_equal(r.cross_n[gone], quiet.cross_n[gone])
    assert np.array_equal(r.in_dist[gone], quiet.in_dist[gone])


# ---- 5. rings and ticks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 70])
def test_a_wrapped_ring(amd, n):
    """capacity 5, 8 samples taken: samples 3 .. 7 sit in slots 3, 4, 0, 1, 2"""
    s0 = None
    if n == 3:                                                   # (the three start further back, so that they cross inside the window)
        s0 = fc.placed(3)
        s0[0, 0] -= 3.0
        s0[1, 0] += 3.0
        s0[2, 0] -= 1.0
    e = crowd(amd, n, ring=5, s0=s0)
    e.step(8 * STRIDE)
    check(e, 3, 5, f"n = {n}, samples 3 .. 7 of a ring of 5")
    n0 = e.flow_launches()
    for first, count in ((0, 3), (2, 2), (0, 8), (4, 5), (8, 1)):
        with pytest.raises(amd.engine.EngineError):
            e.flow(first, count, *layout_of(n))
    assert e.flow_launches() == n0


def test_a_ring_of_enable_history(amd):
    e = crowd(amd, 70, history=True)
    e.step(STRIDE * SAMPLES)
    check(e, 0, SAMPLES, "n = 70, the ring of enable_history", states=e.history(0, SAMPLES))


@pytest.mark.auto_variant
@pytest.mark.parametrize("n", [3, 70, 3000])
def test_flow_between_steps_leaves_the_run_alone(amd, n):
    """the engine's own tick for the size - one wave, one launch, pair + per-agent launches -: step(5), flow, step(5) ends bit for
    bit where step(10) of a twin ends, and what the call returns is the reference's bits"""
    box = max(BOX.get(n, 0.0), 3.0 * np.sqrt(n))
    a, b = (crowd(amd, n, box, seed=90 + n, ring=16, stride=1) for _ in range(2))
    a.step(5)
    lay = layout_of(n, box)
    r = a.flow(0, 5, *lay, events=True)
    assert r.line_count.shape == (4, 5, 2) and a.flow_launches() == 2
    ref = fc.reference(a.recorded(0, 5)[0], *lay)
    same_bits(r, ref)
    same_events(r.events, fc.events(ref))
    invariants(r, n, ref.n_exist)
    ticks = (a.small_ticks(), a.mid_ticks())
    assert (ticks[0] > 0) == (n == 3) and (ticks[1] > 0) == (n == 70)
    a.step(5)
    b.step(10)
    assert np.array_equal(a.state(), b.state())
    fa, fb = a.forces(), b.forces()
    assert np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1])
    assert a.small_ticks() == b.small_ticks() and a.mid_ticks() == b.mid_ticks()
    assert np.array_equal(a.recorded(0, 10)[0], b.recorded(0, 10)[0])


# ---- 6. determinism ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 1100])
def test_the_call_made_twice_gives_the_same_bits(amd, n):
    e = recorded_crowd(amd, n)
    a = e.flow(0, SAMPLES, *layout_of(n), events=True)
    b = e.flow(0, SAMPLES, *layout_of(n), events=True)
    same_bits(a, b)
    same_events(a.events, b.events)
    assert a.n_events >= 1


# ---- 7. batch ----------------------------------------------------------------------------------------------------------------------------
def test_batch_equals_every_member_alone_in_two_launches(amd):
    rng = np.random.default_rng(600)
    box = 30.0
    lay = fc.layout(box)
    members = []
    for k in range(6):
        s0 = fc.placed(3)
        s0[:, :2] += rng.uniform(-0.2, 0.2, (3, 2)) + (box / 2 - 5.0, box / 2)   # the three meet at the middle of the box
        members.append(crowd(amd, 3, s0=s0))
    members.append(crowd(amd, 20, box, seed=7))
    members.append(crowd(amd, 70, box))
    silent = crowd(amd, 3, ring=None)                            # does not record
    engines = members[:4] + [silent] + members[4:]
    amd.Engine.batch_join(engines)
    amd.Engine.step_batch(engines, STRIDE * SAMPLES)
    n0 = [e.flow_launches() for e in engines]
    res = amd.Engine.batch_flow(engines, SAMPLES, *lay, events=True)
    assert engines[0].flow_launches() == n0[0] + 2               # the documented constant: the cells and the walk
    assert [e.flow_launches() for e in engines[1:]] == n0[1:]
    assert res[4] is None and all(r is not None for k, r in enumerate(res) if k != 4)
    for e, r in zip(engines, res):
        if r is None:
            continue
        alone = e.flow(0, SAMPLES, *lay, events=True)
        assert r.first == 0 and r.line_count.shape == (SAMPLES - 1, 5, 2) and r.cross_n.shape == (e.n, 5, 2) and r.period == pytest.approx(0.2)
        same_bits(r, alone)
        same_events(r.events, alone.events)
        ref = fc.reference(e.recorded(0, SAMPLES)[0], *lay)
        same_bits(r, ref)
        same_events(r.events, fc.events(ref))
        invariants(r, e.n, ref.n_exist)
        assert len(ref.crossings) >= 1, "vacuous: a member without a crossing"
    outs = (amd.ffi.FlowOut * len(engines))()                    # the non-recording member at the ABI: first_sample -2
    arr = (C.c_void_p * len(engines))(*[e._h for e in engines])
    pack = amd.engine._FlowPack([(1, 1)], *amd.engine._flow_layout("flow", *lay), [0])
    assert engines[0]._lib.csf_batch_flow(arr, len(engines), SAMPLES, C.byref(pack.layout), outs) == 0
    assert outs[4].first_sample == -2 and outs[4].n_events == 0 and outs[0].first_sample == 0 and outs[0].n_events == res[0].n_events
    n1 = engines[0].flow_launches()                              # more samples than a member's ring holds: refused before anything is written
    with pytest.raises(amd.engine.EngineError):
        amd.Engine.batch_flow(engines, SAMPLES + 1, *lay)
    assert engines[0].flow_launches() == n1
    amd.Engine.batch_leave(engines)


# ---- 8. events ---------------------------------------------------------------------------------------------------------------------------
def test_events(amd, monkeypatch):
    n = 70
    e = recorded_crowd(amd, n)
    lay = layout_of(n)
    r, ref = check(e, 0, SAMPLES, "events, n = 70")              # every crossing, sorted, equal to the reference's list
    ev = r.events
    key = list(zip(ev["i"].tolist(), ev["l"].tolist(), ev["k"].tolist()))
    assert key == sorted(key) and len(set(key)) == len(key) and len(ev) >= 5
    assert ((ev["u"] >= 0) & (ev["u"] <= 1)).all() and (np.abs(ev["dir"]) == 1).all() and ((ev["t"] >= ev["k"]) & (ev["t"] <= ev["k"] + 1)).all()
    # capacity 0 with a NULL buffer: counted, not stored
    lib = e._lib
    pack = amd.engine._FlowPack([(n, SAMPLES)], *amd.engine._flow_layout("flow", *lay), [0])
    out = amd.ffi.FlowOut()
    assert lib.csf_flow(e._h, 0, SAMPLES, C.byref(pack.layout), C.byref(out)) == 0 and out.n_events == r.n_events and out.first_sample == 0
    assert out.n_outside == r.n_outside
    # a capacity below the total: the total is still right, and what is stored is some of the crossings
    some = np.zeros(3, amd.engine.FLOW_EVENT_DTYPE)
    out.events, out.event_capacity = some.ctypes.data, 3
    assert lib.csf_flow(e._h, 0, SAMPLES, C.byref(pack.layout), C.byref(out)) == 0 and out.n_events == r.n_events > 3
    stored = {(int(s["i"]), int(s["l"]), int(s["k"])) for s in some}
    assert len(stored) == 3 and stored <= set(key)
    for s in some:
        assert s.tobytes() == ev[key.index((int(s["i"]), int(s["l"]), int(s["k"])))].tobytes()
    # a guess that is too small: exactly one second call, with the exact capacity
    calls = []

    class Counting:                                             # (the library, with the wrapper's calls counted)
        def __getattr__(self, name):
            if name != "csf_flow":
                return getattr(lib, name)

            def call(*args):
                calls.append(int(args[-1][0].event_capacity))
                return lib.csf_flow(*args)
            return call
    monkeypatch.setattr(amd.engine, "_flow_capacity_guess", lambda cells, lines: 3)
    e._lib = Counting()
    try:
        small = e.flow(0, SAMPLES, *lay, events=True)
    finally:
        e._lib = lib
    assert calls == [3, r.n_events]
    same_events(small.events, r.events)
    same_bits(small, r)


# ---- 9. launches -------------------------------------------------------------------------------------------------------------------------
def test_two_launches_per_call_that_covers_a_sample(amd):
    for n in (3, 300):
        e = recorded_crowd(amd, n)
        lay = layout_of(n)
        assert e.flow_launches() == 0
        for k, (first, count) in enumerate(((0, SAMPLES), (1, 2), (3, 3), (2, 1)), start=1):
            e.flow(first, count, *lay, events=k == 1)
            assert e.flow_launches() == 2 * k
        e.flow(2, 0, *lay)                                       # no sample: no launch
        assert e.flow_launches() == 8 and e.passing_launches() == 0 and e.pet_launches() == 0 and e.encounter_launches() == 0


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_have_a_message_and_no_side_effect(amd):
    from calib_common import data_set, pod_sets
    a, twin = (crowd(amd, 40, 30.0, seed=10, ring=4, stride=1) for _ in range(2))
    plain = crowd(amd, 40, 30.0, seed=10, ring=None)
    a.step(6); twin.step(6); plain.step(6)
    lib = a._lib
    n = 40
    lines, areas, grid = fc.layout(30.0)
    arrays = dict(lc=np.full((3, 5, 2), -7, np.int32), cn=np.full((n, 5, 2), -7, np.int32), ft=np.full((n, 5), -7.0), oc=np.full((4, 3), -7, np.int32),
                  di=np.full((n, 3), -7.0), gc=np.full((8, 8), -7, np.int32), ev=np.zeros(8, amd.engine.FLOW_EVENT_DTYPE))

    def out(**kw):
        o = amd.ffi.FlowOut()
        o.line_count, o.cross_n, o.first_t, o.occupancy, o.in_dist, o.grid_count = (arrays[f].ctypes.data for f in ("lc", "cn", "ft", "oc", "di", "gc"))
        o.n_events = o.n_outside = -7
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    keep = []

    def lay(lines=lines, areas=areas, grid=grid, **kw):
        """a csf_flow_layout as given, unchecked"""
        y = amd.ffi.FlowLayout()
        ln = np.zeros((0, 4)) if lines is None else np.ascontiguousarray(lines, dtype=np.float64)
        ar = np.zeros((0, 5)) if areas is None else np.ascontiguousarray(areas, dtype=np.float64)
        keep.extend((ln, ar))
        y.lines, y.areas, y.n_lines, y.n_areas = (ln.ctypes.data if len(ln) else None), (ar.ctypes.data if len(ar) else None), len(ln), len(ar)
        y.x0, y.y0, y.h, y.nx, y.ny = grid
        for k, v in kw.items():
            setattr(y, k, v)
        return y

    def line_with(at, v):
        ln = lines.copy()
        ln[1, at] = v
        return ln

    def area_with(at, v):
        ar = areas.copy()
        ar[1, at] = v
        return ar

    ev = arrays["ev"].ctypes.data
    ok = lay()
    cases = {
        "out NULL": (a, 2, 4, ok, None), "layout NULL": (a, 2, 4, None, out()),
        "n_lines < 0": (a, 2, 4, lay(n_lines=-1), out()), "n_lines 65": (a, 2, 4, lay(lines=np.tile(lines[:1], (65, 1))), out()),
        "n_areas < 0": (a, 2, 4, lay(n_areas=-1), out()), "n_areas 65": (a, 2, 4, lay(areas=np.tile(areas[:1], (65, 1))), out()),
        "lines NULL": (a, 2, 4, lay(lines=None, n_lines=2), out()), "areas NULL": (a, 2, 4, lay(areas=None, n_areas=1), out()),
        "a line NaN": (a, 2, 4, lay(lines=line_with(2, NAN)), out()), "a line inf": (a, 2, 4, lay(lines=line_with(0, INF)), out()),
        "a line of no length": (a, 2, 4, lay(lines=np.array([(1.0, 2.0, 1.0, 2.0)])), out()),
        "an area NaN": (a, 2, 4, lay(areas=area_with(1, NAN)), out()), "an area -inf": (a, 2, 4, lay(areas=area_with(3, -INF)), out()),
        "an area of no length": (a, 2, 4, lay(areas=np.array([(1.0, 2.0, 1.0, 2.0, 1.0)])), out()),
        "half_width NaN": (a, 2, 4, lay(areas=area_with(4, NAN)), out()), "half_width negative": (a, 2, 4, lay(areas=area_with(4, -0.5)), out()),
        "half_width inf": (a, 2, 4, lay(areas=area_with(4, INF)), out()),
        "h 0": (a, 2, 4, lay(h=0.0), out()), "h negative": (a, 2, 4, lay(h=-1.0), out()), "h NaN": (a, 2, 4, lay(h=NAN), out()), "h inf": (a, 2, 4, lay(h=INF), out()),
        "x0 NaN": (a, 2, 4, lay(x0=NAN), out()), "y0 inf": (a, 2, 4, lay(y0=INF), out()),
        "nx negative": (a, 2, 4, lay(nx=-8), out()), "ny negative": (a, 2, 4, lay(ny=-8), out()),
        "nx 0 alone": (a, 2, 4, lay(nx=0), out()), "ny 0 alone": (a, 2, 4, lay(ny=0), out()),
        "a grid above 2^20 cells": (a, 2, 4, lay(nx=1025, ny=1024), out()),
        "the current state has no interval": (a, -1, 1, ok, out()), "first below -1": (a, -2, 2, ok, out()),
        "no ring": (plain, 2, 4, ok, out()), "no ring, an empty window": (plain, 0, 0, ok, out()),
        "n_samples < 0": (a, 2, -1, ok, out()), "n_samples above 65535": (a, 2, 65536, ok, out()),
        "samples gone from the ring": (a, 1, 4, ok, out()), "samples not yet there": (a, 4, 3, ok, out()),
        "capacity < 0": (a, 2, 4, ok, out(events=ev, event_capacity=-1)),
        "capacity without a buffer": (a, 2, 4, ok, out(event_capacity=8)),
    }
    n0 = {id(e): e.flow_launches() for e in (a, plain)}
    for name, (e, first, count, y, o) in cases.items():
        rc = lib.csf_flow(e._h, first, count, None if y is None else C.byref(y), None if o is None else C.byref(o))
        assert rc in (-1, -4), (name, rc)
        assert lib.csf_last_error(e._h).decode(), name
        assert o is None or (o.n_events == -7 and o.n_outside == -7), name
        assert e.flow_launches() == n0[id(e)], name
    assert all((arrays[f] == -7).all() for f in ("lc", "cn", "ft", "oc", "di", "gc"))
    # the largest layout is allowed: 64 lines, 64 areas, 2^20 cells
    o = out(line_count=None, cross_n=None, first_t=None, occupancy=None, in_dist=None, grid_count=None)
    big = lay(lines=np.tile(lines[:1], (64, 1)), areas=np.tile(areas[:1], (64, 1)), nx=1024, ny=1024)
    assert lib.csf_flow(a._h, 2, 4, C.byref(big), C.byref(o)) == 0 and o.n_events >= 0 and o.first_sample == 2
    one = a.flow(2, 4, lines[:1], areas[:1], grid, events=True)
    assert o.n_events == 64 * one.n_events
    assert a.flow_launches() == n0[id(a)] + 4
    # the ordinary call writes every array
    o = out()
    assert lib.csf_flow(a._h, 2, 4, C.byref(ok), C.byref(o)) == 0 and o.first_sample == 2
    assert not any((arrays[f] == -7).any() for f in ("lc", "cn", "ft", "oc", "di", "gc"))
    assert a.flow_launches() == n0[id(a)] + 6
    for f in ("lc", "cn", "ft", "oc", "di", "gc"):
        arrays[f][:] = -7
    # a call without a sample succeeds and finds nothing, without a launch
    o = out()
    assert lib.csf_flow(a._h, 3, 0, C.byref(ok), C.byref(o)) == 0 and o.n_events == 0 and o.n_outside == 0 and o.first_sample == 3
    assert np.isinf(arrays["ft"]).all() and (arrays["cn"] == 0).all() and (arrays["di"] == 0.0).all() and (arrays["gc"] == 0).all()
    assert (arrays["lc"] == -7).all() and (arrays["oc"] == -7).all()      # (arrays without rows)
    assert a.flow_launches() == n0[id(a)] + 6
    # the refused engine is where its twin is
    assert np.array_equal(a.state(), twin.state())
    a.step(5); twin.step(5)
    assert np.array_equal(a.state(), twin.state())
    assert np.array_equal(a.recorded(7, 4)[0], twin.recorded(7, 4)[0])
    # a member of a loopback group
    g = [crowd(amd, 40, 30.0, seed=10, ring=4, stride=1) for _ in range(2)]
    amd.Engine.loopback_group(g)
    o = out()
    rc = lib.csf_flow(g[0]._h, 0, 2, C.byref(ok), C.byref(o))
    assert rc == -4 and lib.csf_last_error(g[0]._h).decode() and g[0].flow_launches() == 0 and o.n_events == -7
    # an engine that holds a calibration data set
    sets = pod_sets("twod", 2)
    cs0, cFx, cFy = data_set("twod", n_seq=2, ticks=20)
    c = amd.Engine(sets[0], 4)
    c.calib_load(cs0, cFx, cFy, np.zeros((20, 2, 2)), [0, 1], max_sets=2)
    rc = lib.csf_flow(c._h, 0, 2, C.byref(ok), C.byref(o))
    assert rc == -4 and lib.csf_last_error(c._h).decode() and c.flow_launches() == 0
    # the batched call: not a batch, NULL outs or layout, a bad layout, too many samples, too many cells
    outs = (amd.ffi.FlowOut * 2)()
    arr = (C.c_void_p * 2)(a._h, twin._h)
    assert lib.csf_batch_flow(arr, 2, 2, C.byref(ok), outs) == -4
    amd.Engine.batch_join([a, twin])
    n1 = a.flow_launches()
    assert lib.csf_batch_flow(arr, 2, 2, C.byref(ok), None) == -1
    assert lib.csf_batch_flow(arr, 2, 2, None, outs) == -1
    assert lib.csf_batch_flow(arr, 2, 2, C.byref(lay(h=0.0)), outs) == -1
    assert lib.csf_batch_flow(arr, 2, 2, C.byref(lay(lines=line_with(2, NAN))), outs) == -1
    assert lib.csf_batch_flow(arr, 2, -1, C.byref(ok), outs) == -1
    assert lib.csf_batch_flow(arr, 2, 5, C.byref(ok), outs) == -1                 # more than the ring of 4 holds
    assert a.flow_launches() == n1
    assert lib.csf_batch_flow(arr, 2, 2, C.byref(ok), outs) == 0 and a.flow_launches() == n1 + 2
    assert outs[0].first_sample == 9 and outs[1].first_sample == 9
    amd.Engine.batch_leave([a, twin])
    many = [crowd(amd, 2, ring=4, stride=1) for _ in range(17)]  # 17 members x 2^20 cells
    amd.Engine.batch_join(many)
    amd.Engine.step_batch(many, 4)
    outs = (amd.ffi.FlowOut * 17)()
    arr = (C.c_void_p * 17)(*[e._h for e in many])
    assert lib.csf_batch_flow(arr, 17, 2, C.byref(lay(nx=1024, ny=1024)), outs) == -1 and lib.csf_last_error(many[0]._h).decode()
    assert many[0].flow_launches() == 0
    with pytest.raises(ValueError):
        amd.Engine.batch_flow(many, 2, grid=(0.0, 0.0, 1.0, 1024, 1024))
    assert lib.csf_batch_flow(arr, 17, 2, C.byref(lay(nx=1024, ny=963)), outs) == 0 and many[0].flow_launches() == 2       # 17 x 986 112 cells: just below
    assert all(int(o.n_outside) >= 0 and o.first_sample == 2 for o in outs)
    amd.Engine.batch_leave(many)


# ---- 11. intersections -------------------------------------------------------------------------------------------------------------------
def test_intersections_together(amd):
    from cyclistsocialforce_amd import intersection as ci
    from cyclistsocialforce_amd.vehicle import TwoDBicycle
    lay = layout_of(3)
    scenes = []
    for k in range(3):
        s0 = fc.placed(3)
        s0[:, 0] += 0.2 * k
        vs = []
        for j, s in enumerate(s0):
            v = TwoDBicycle(tuple(s), id=f"s{k}r{j}")
            v.setDestinations(s[0] + np.array([30.0, 60.0]) * np.cos(s[2]), s[1] + np.array([30.0, 60.0]) * np.sin(s[2]))
            vs.append(v)
        scenes.append(ci.SocialForceIntersection(vs))
    ci.advance_together(scenes, 120)                              # (the dense route records every tick)
    res = ci.flow_together(scenes, 120, *lay, events=True)
    for k, (ins, r) in enumerate(zip(scenes, res)):
        alone = ins.flow(r.first, 120, *lay, events=True)
        same_bits(r, alone)
        same_events(r.events, alone.events)
        assert r.ids == alone.ids == [f"s{k}r{j}" for j in range(3)] and r.period == pytest.approx(0.01)
        assert list(r.event_i_id) == [r.ids[i] for i in r.events["i"]] and list(alone.event_i_id) == list(r.event_i_id)
        ref = fc.reference(ins.engine.recorded(r.first, 120)[0], *lay)
        assert len(ref.crossings) >= 1, "vacuous: the reference finds no crossing"
        same_bits(r, ref)
        same_events(r.events, fc.events(ref))
        invariants(r, 3, ref.n_exist)
    plain = ci.flow_together(scenes, 120, *lay)
    assert plain[0].events is None and plain[0].event_i_id is None and plain[0].ids == res[0].ids
