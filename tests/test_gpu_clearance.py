"""Road clearance on the MI355X (include/csf.h: csf_clearance, csf_batch_clearance; csf_clearance.hip) against the
definition in NumPy fp64 (tests/clearance_common.py), applied to the states read back with Engine.recorded: engine and reference start
from identical bits.

The comparison is BIT FOR BIT - every array of a result, the counters and the events - and no cell is left out.  That is derivable,
not measured: every input is the ring's fp64 bits or the road's, every operation is one IEEE operation in a stated order without
contraction, sqrt and division are correctly rounded, no transcendental is involved, and every aggregate is an integer or a minimum
taken with a strict `<` in a stated order.

The roads are clearance_common.road's, relative to the side b of the box the riders start in: a straight two-kerb path along
y = b/2 from b/4 to 3b/4 (two polylines mirrored about the midline, which share the segments the case asks for), a short polyline of
two segments, and one segment at 3b nobody comes near; a road of one segment lies on the box's diagonal.  The sizes are one segment, one
chunk of 512 exactly, one chunk + 1, and 1 283 (three chunks: each kerb lies across a chunk boundary).  clearance_common.mirrored is
the tie across chunks: a rider placed by hand runs along y = 0 between two kerbs at y = -+2 whose nearest segments lie in chunks 0
and 2.  Every case from 33 riders up asserts from the reference alone that it is not vacuous: nearest points with t == 0, t == 1
and in between, stations with a finite left, a finite right and only one of them, a crossing in each direction, a sign change
refused for the extent, riders with and without a near sample (d_event = b/16).  What the reference finds on the engine's
trajectories (seed 0; nearest points with t == 0 / t == 1 / between; stations with a finite left, a finite right, only one of them,
of all; crossings by direction; sign changes refused for the extent; riders with / without a near sample): 33 riders, 1 283 segments
72 / 82 / 110; 188, 197, 77 of 231; 4 + 2; 6 402; 10 / 23 - 33 riders, 512 segments the same but 187, 197, 78 and 2 549 refused (513:
2 552) - 257 riders, 1 283 and 513 segments 467 / 801 / 788; 1 608, 1 592, 398 of 1 799; 12 + 13; 25 605 and 10 205; 67 / 190.  One
polyline had to be moved: the road of one segment lay along the path's midline, where the 33 riders crossed it 2 + 0 times; it lies
on the box's diagonal from (b/4, b/4) to (3b/4, 3b/4) now, where they give 64 / 42 / 158; 132, 99, 231 of 231; 1 + 3; 2; 6 / 27."""
import ctypes as C

import numpy as np
import pytest

import clearance_common as cc

pytestmark = pytest.mark.gpu

INF = float("inf")
NAN = float("nan")
STRIDE = 20                     # x t_s = 0.01 s: a sample every 0.2 s
SAMPLES = 8
BOX = {33: 20.0, 70: 30.0, 257: 60.0}                            # (test_gpu_flow.py's)
SEED = 0
THREE_CHUNKS = 1283


@pytest.fixture(scope="module")
def amd():
    from cyclistsocialforce_amd import _ffi, engine, parameters

    class NS:
        pass

    ns = NS()
    ns.Engine, ns.pod, ns.ffi, ns.engine = engine.Engine, parameters.default_pod, _ffi, engine
    return ns


def road_of(n, S, box=None):
    """the road of a population and its d_event: the box's for the scattered ones; for the riders placed by hand (x = 0 ... 10,
    y = -1.5 ... 1) that of a box of 12 m, moved so that their paths lie inside it"""
    if n <= 3:
        return cc.road(12.0, S, shift=(-1.0, -6.0)), 0.75
    b = box or BOX[n]
    return cc.road(b, S), b / 16


def crowd(amd, n, box=None, seed=SEED, ring=SAMPLES, stride=STRIDE, s0=None, history=False):
    """n road users scattered in a box (one to three: placed by hand), riding towards destinations ahead of them; ring: the capacity
    of a state ring of every `stride`-th tick (None: no recording; history: csf_enable_history's ring instead of csf_record's)"""
    pod = amd.pod("twod")
    ns = amd.ffi.N_STATES[pod.model]
    if s0 is None:
        s0 = cc.placed(n, ns=ns) if n <= 3 else cc.scatter(n, box or BOX.get(n, 6.0), seed, ns=ns)
    vdes = s0[:, 3].copy() if n <= 3 else 5.0                    # (the placed riders keep their speeds: a slow one stays slow)
    e = amd.Engine(pod, max(n, 1))
    e.add_agents(s0, vdes)
    e.set_dest_queue(np.arange(n), *cc.with_queue(s0), reset=True)
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
    ex = ref.g >= 0
    t0, t1, mid = int((ref.t[ex] == 0).sum()), int((ref.t[ex] == 1).sum()), int(((ref.t[ex] > 0) & (ref.t[ex] < 1)).sum())
    fl, fr = np.isfinite(ref.left), np.isfinite(ref.right)
    st = ~np.isnan(ref.left)
    up, down = int((ref.crossings["dir"] > 0).sum()), int((ref.crossings["dir"] < 0).sum())
    near, far = int((ref.near_samples > 0).sum()), int((ref.near_samples == 0).sum())
    print(f"{what}: {n} riders, nearest points with t == 0 / t == 1 / between {t0} / {t1} / {mid}, stations with a finite left {int(fl.sum())}, "
          f"right {int(fr.sum())}, only one {int((st & (fl != fr)).sum())}, neither {int((st & ~fl & ~fr).sum())} of {int(st.sum())}, crossings {up} + {down}, "
          f"sign changes refused for the extent {ref.refused}, riders with / without a near sample {near} / {far}")
    if n >= 33:
        assert t0 >= 1 and t1 >= 1 and mid >= 1, "vacuous: the clamps"
        assert fl.sum() >= 1 and fr.sum() >= 1 and (st & (fl != fr)).sum() >= 1, "vacuous: the sides"
        assert up >= 1 and down >= 1 and ref.refused >= 1, "vacuous: the crossings"
        assert near >= 1 and far >= 1, "vacuous: the near samples"


def same_bits(got, ref, what="", fields=cc.ARRAYS):
    """every array of a Clearance against the reference's (or another Clearance's): the same bits, NaN where NaN"""
    for f in fields:
        g, w = getattr(got, f), getattr(ref, f)
        assert g is not None and w is not None, (what, f)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f, g.dtype, w.dtype, g.shape, w.shape)
        if not np.array_equal(g, w, equal_nan=g.dtype.kind == "f"):
            bad = np.argwhere(~((g == w) | ((g != g) & (w != w))))
            raise AssertionError(f"{what}: {f} differs in {len(bad)} of {g.size} cells, first {bad[:4].tolist()}: "
                                 + ", ".join(f"{g[tuple(b)]!r} ({np.asarray(g[tuple(b)]).tobytes().hex()}) against {w[tuple(b)]!r} ({np.asarray(w[tuple(b)]).tobytes().hex()})" for b in bad[:4]))


def same_events(ev, ref_ev):
    assert len(ev) == len(ref_ev) and ev.dtype.names == ref_ev.dtype.names
    for f in ev.dtype.names:
        assert np.array_equal(ev[f], ref_ev[f]), f


def invariants(r):
    """what holds of every result with events"""
    assert r.n_events == int(r.cross.sum()) == len(r.events) == int(r.cross_n.sum()) == int(r.cross_count.sum())
    assert np.array_equal(np.bincount(r.events["i"], minlength=r.cross_n.size), r.cross_n)
    assert np.array_equal(r.near_count.sum(), r.near_samples.sum())
    key = list(zip(*(r.events[f].tolist() for f in ("i", "k", "edge", "seg"))))
    assert key == sorted(key) and len(set(key)) == len(key)
    assert ((r.events["u"] >= 0) & (r.events["u"] <= 1)).all() and (np.abs(r.events["dir"]) == 1).all()
    ex = ~np.isnan(r.d)
    assert ((r.edge >= 0) == ex).all() and ((r.t[ex] >= 0) & (r.t[ex] <= 1)).all()
    with np.errstate(invalid="ignore"):
        assert (np.minimum(r.left, r.right)[~np.isnan(r.left)] >= r.d[:-1][~np.isnan(r.left)]).all()


def check(e, first, count, road, d_event, what, vacuous=True, states=None):
    """clearance(first, count, with events) against the reference on recorded(first, count); returns both"""
    S = e.recorded(first, count)[0] if states is None else states
    ref = cc.reference(S, road, d_event)
    if vacuous:
        not_vacuous(ref, e.n, what)
    r = e.clearance(first, count, road, d_event, events=True)
    assert r.first == first
    same_bits(r, ref, what=what)
    same_events(r.events, cc.events(ref))
    invariants(r)
    return r, ref


# ---- 1. against NumPy: populations and road sizes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, S", [(1, THREE_CHUNKS), (2, THREE_CHUNKS), (3, THREE_CHUNKS), (33, THREE_CHUNKS), (257, THREE_CHUNKS),
                                  (3, 1), (33, 1), (3, cc.CHUNK), (33, cc.CHUNK), (33, cc.CHUNK + 1), (257, cc.CHUNK + 1)])
def test_against_numpy(amd, n, S):
    """one to three riders placed by hand on the packed path; 33: the first size of the tiled path, one tile with a tail; 257: two
    tiles of road users - against one segment, one chunk exactly, one chunk + 1 and three chunks"""
    e = recorded_crowd(amd, n)
    road, d_event = road_of(n, S)
    assert len(cc.segments(*road)[0]) == S and amd.engine.CLEARANCE_CHUNK == cc.CHUNK
    r, ref = check(e, 0, SAMPLES, road, d_event, f"n = {n}, S = {S}")
    assert r.d.shape == (SAMPLES, n) and r.left.shape == (SAMPLES - 1, n) and r.d_min.shape == (n,) and r.near_count.shape == (SAMPLES,)
    assert r.cross_count.shape == (SAMPLES - 1,) and r.period == pytest.approx(0.2) and np.array_equal(r.offsets, road[0]) and r.d_event == d_event
    # the helpers, on the device's arrays
    lat = r.lateral_position()
    both = np.isfinite(r.left) & np.isfinite(r.right)
    assert np.array_equal(np.isnan(lat), ~both) and ((lat[both] >= 0) & (lat[both] <= 1)).all() and r.off_road().shape == r.cross.shape
    assert r.nearest_edge_share().sum() == pytest.approx(1.0)
    # without events, and without the per-sample arrays: the same bits
    plain = e.clearance(0, SAMPLES, road, d_event)
    assert plain.events is None and plain.n_events == r.n_events
    same_bits(plain, r)
    short = e.clearance(0, SAMPLES, road, d_event, per_sample=False)
    assert short.d is None and short.left is None and short.cross is None and short.n_events == r.n_events
    same_bits(short, r, fields=cc.USER + cc.SAMPLE)
    none = e.clearance(0, SAMPLES, road)                         # d_event = 0 finds none
    assert (none.near_samples == 0).all() and (none.near_first == -1).all() and (none.near_count == 0).all()
    same_bits(none, r, fields=cc.CELL + cc.STATION)


# ---- 2. the tie across chunks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("swapped", [False, True])
def test_a_tie_across_chunks_reports_the_lower_segment(amd, swapped):
    """a rider placed by hand runs exactly along y = 0 between two mirrored kerbs whose nearest segments lie in chunks 0 and 2: the
    same d2 from two chunks, and the first kerb's segment is the one to report - whichever kerb is first"""
    e = recorded_crowd(amd, 1, s0=cc.placed(1))
    road = cc.mirrored(swapped)
    S = e.recorded(0, SAMPLES)[0]
    assert (S[:, 0, 1] == 0.0).all() and (S[:, 0, 0] >= 0.0).all() and (S[:, 0, 0] < 10.0).all() and S[-1, 0, 0] > 5.0
    r, ref = check(e, 0, SAMPLES, road, 2.5, f"the tie, swapped = {swapped}", vacuous=False)
    assert (ref.d == 2.0).all() and (ref.edge == 0).all() and ((ref.seg >= 416) & (ref.seg < 456)).all()     # chunk 0; the mirror image: 640 + seg >= 1024
    # the direction of travel is +x: the kerb at y = +2 is on the left
    assert (ref.left == 2.0).all() and (ref.right == 2.0).all() and (ref.left_edge == (0 if swapped else 1)).all() and (ref.right_edge == (1 if swapped else 0)).all()
    assert (r.lateral_position() == 0.5).all() and (r.width() == 4.0).all() and r.n_events == 0 and (r.near_samples == SAMPLES).all()


# ---- 3. a sub-window -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 33])
def test_a_sub_window(amd, n):
    e = recorded_crowd(amd, n)
    road, d_event = road_of(n, cc.CHUNK + 1)
    full = e.clearance(0, SAMPLES, road, d_event, events=True)
    sub, ref = check(e, 2, 4, road, d_event, f"n = {n}, samples 2 .. 5", vacuous=False)
    assert sub.first == 2 and sub.d.shape == (4, n) and sub.left.shape == (3, n)
    same_bits(sub, full_rows(full, 2, 4), fields=cc.CELL + cc.STATION + cc.SAMPLE)
    for count in (0, 1):                                         # no station
        one = e.clearance(2, count, road, d_event, events=True)
        assert one.d.shape == (count, n) and one.left.shape == (0, n) and one.cross_count.shape == (0,) and one.n_events == 0 and len(one.events) == 0
        assert np.isinf(one.left_min).all() and (one.left_min_k == -1).all() and (one.cross_n == 0).all()
        same_bits(one, cc.reference(e.recorded(2, count)[0], road, d_event))
    check(e, 2, 2, road, d_event, "one station", vacuous=False)


def full_rows(full, first, count):
    """rows [first, first + count) of the per-sample arrays of a result, [first, first + count - 1) of the per-station ones"""
    class Rows:
        pass
    r = Rows()
    for f in cc.CELL + ("near_count",):
        setattr(r, f, getattr(full, f)[first:first + count])
    for f in cc.STATION + ("cross_count",):
        setattr(r, f, getattr(full, f)[first:first + count - 1])
    return r


# ---- 4. non-finite -------------------------------------------------------------------------------------------------------------------------
def test_a_rider_whose_x_becomes_nan(amd):
    n, gone = 33, 5
    e = crowd(amd, n)
    e.step(4 * STRIDE)
    bad = e.state()[gone].copy()
    bad[0] = np.nan
    e.push_state([gone], bad)
    e.step(4 * STRIDE)
    S, _ = e.recorded(0, SAMPLES)
    assert np.isnan(S[4:, gone, 0]).all() and np.isfinite(S[:4, gone, 0]).all()
    road, d_event = road_of(n, THREE_CHUNKS)
    r, ref = check(e, 0, SAMPLES, road, d_event, "n = 33, one rider NaN from sample 4 on", vacuous=False)
    assert ref.n_exist == SAMPLES * n - 4 and np.isnan(r.d[4:, gone]).all() and (r.edge[4:, gone] == -1).all() and np.isnan(r.t[4:, gone]).all()
    assert np.isnan(r.left[3:, gone]).all() and np.isfinite(r.d[:4, gone]).all() and (r.cross[3:, gone] == 0).all() and r.d_min_k[gone] < 4
    quiet = cc.reference(S[:4], road, d_event)                   # what the rider did in its four samples is all it did
    for f in cc.USER:
        assert getattr(r, f)[gone] == getattr(quiet, f)[gone], f


# ---- 5. rings and ticks --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 33])
def test_a_wrapped_ring(amd, n):
    """capacity 5, 8 samples taken: samples 3 .. 7 sit in slots 3, 4, 0, 1, 2"""
    e = crowd(amd, n, ring=5)
    e.step(8 * STRIDE)
    road, d_event = road_of(n, cc.CHUNK + 1)
    check(e, 3, 5, road, d_event, f"n = {n}, samples 3 .. 7 of a ring of 5", vacuous=False)
    n0 = e.clearance_launches()
    for first, count in ((0, 3), (2, 2), (0, 8), (4, 5), (8, 1)):
        with pytest.raises(amd.engine.EngineError):
            e.clearance(first, count, road)
    assert e.clearance_launches() == n0


def test_a_ring_of_enable_history(amd):
    e = crowd(amd, 33, history=True)
    e.step(STRIDE * SAMPLES)
    road, d_event = road_of(33, THREE_CHUNKS)
    check(e, 0, SAMPLES, road, d_event, "n = 33, the ring of enable_history", states=e.history(0, SAMPLES))


@pytest.mark.auto_variant
@pytest.mark.parametrize("n", [3, 70, 3000])
def test_clearance_between_steps_leaves_the_run_alone(amd, n):
    """the engine's own tick for the size - one wave, one launch, pair + per-agent launches -: step(5), clearance, step(5) ends bit
    for bit where step(10) of a twin ends, and what the call returns is the reference's bits"""
    box = max(BOX.get(n, 0.0), 3.0 * np.sqrt(n))
    a, b = (crowd(amd, n, box, seed=90 + n, ring=16, stride=1) for _ in range(2))
    a.step(5)
    road, d_event = road_of(n, cc.CHUNK + 1, box)
    r = a.clearance(0, 5, road, d_event, events=True)
    assert r.d.shape == (5, n) and a.clearance_launches() == amd.engine.CLEARANCE_LAUNCHES == 3
    ref = cc.reference(a.recorded(0, 5)[0], road, d_event)
    same_bits(r, ref)
    same_events(r.events, cc.events(ref))
    ticks = (a.small_ticks(), a.mid_ticks())
    assert (ticks[0] > 0) == (n == 3) and (ticks[1] > 0) == (n == 70)
    a.step(5)
    b.step(10)
    assert np.array_equal(a.state(), b.state())
    fa, fb = a.forces(), b.forces()
    assert np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1])
    assert a.small_ticks() == b.small_ticks() and a.mid_ticks() == b.mid_ticks()
    assert np.array_equal(a.recorded(0, 10)[0], b.recorded(0, 10)[0])


# ---- 6. determinism ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 257])
def test_the_call_made_twice_gives_the_same_bits(amd, n):
    e = recorded_crowd(amd, n)
    road, d_event = road_of(n, THREE_CHUNKS)
    a = e.clearance(0, SAMPLES, road, d_event, events=True)
    b = e.clearance(0, SAMPLES, road, d_event, events=True)
    same_bits(a, b)
    same_events(a.events, b.events)


# ---- 7. batch ------------------------------------------------------------------------------------------------------------------------------
def test_batch_equals_every_member_alone_in_three_launches(amd):
    rng = np.random.default_rng(600)
    box = 30.0
    road, d_event = cc.road(box, cc.CHUNK + 1), box / 16
    members = []
    for k in range(6):
        s0 = cc.placed(3)
        s0[:, :2] += rng.uniform(-0.2, 0.2, (3, 2)) + (box / 2 - 5.0, box / 2)   # the three meet at the middle of the box
        members.append(crowd(amd, 3, s0=s0))
    members.append(crowd(amd, 20, box, seed=7))
    members.append(crowd(amd, 70, box))
    silent = crowd(amd, 3, ring=None)                            # does not record
    engines = members[:4] + [silent] + members[4:]
    amd.Engine.batch_join(engines)
    amd.Engine.step_batch(engines, STRIDE * SAMPLES)
    n0 = [e.clearance_launches() for e in engines]
    res = amd.Engine.batch_clearance(engines, SAMPLES, road, d_event, events=True)
    assert engines[0].clearance_launches() == n0[0] + amd.engine.CLEARANCE_LAUNCHES      # the documented constant
    assert [e.clearance_launches() for e in engines[1:]] == n0[1:]
    assert res[4] is None and all(r is not None for k, r in enumerate(res) if k != 4)
    for e, r in zip(engines, res):
        if r is None:
            continue
        alone = e.clearance(0, SAMPLES, road, d_event, events=True)
        assert r.first == 0 and r.d.shape == (SAMPLES, e.n) and r.period == pytest.approx(0.2)
        same_bits(r, alone)
        same_events(r.events, alone.events)
        ref = cc.reference(e.recorded(0, SAMPLES)[0], road, d_event)
        same_bits(r, ref)
        same_events(r.events, cc.events(ref))
        invariants(r)
    short = amd.Engine.batch_clearance(engines, SAMPLES, road, d_event, per_sample=False)
    assert short[4] is None and short[0].d is None
    same_bits(short[-1], res[-1], fields=cc.USER + cc.SAMPLE)
    outs = (amd.ffi.ClearanceOut * len(engines))()               # the non-recording member at the ABI: first_sample -2
    arr = (C.c_void_p * len(engines))(*[e._h for e in engines])
    pack = amd.engine._ClearancePack([(1, 1)], *amd.engine._clearance_road("clearance", road), [0], True)
    assert engines[0]._lib.csf_batch_clearance(arr, len(engines), SAMPLES, C.byref(pack.road), d_event, outs) == 0
    assert outs[4].first_sample == -2 and outs[4].n_events == 0 and outs[0].first_sample == 0 and outs[0].n_events == res[0].n_events
    n1 = engines[0].clearance_launches()                         # more samples than a member's ring holds: refused before anything is written
    with pytest.raises(amd.engine.EngineError):
        amd.Engine.batch_clearance(engines, SAMPLES + 1, road)
    assert engines[0].clearance_launches() == n1
    amd.Engine.batch_leave(engines)


# ---- 8. events -----------------------------------------------------------------------------------------------------------------------------
def test_events(amd, monkeypatch):
    n = 257
    e = recorded_crowd(amd, n)
    road, d_event = road_of(n, cc.CHUNK + 1)
    r, ref = check(e, 0, SAMPLES, road, d_event, "events, n = 257")       # every crossing, sorted, equal to the reference's list
    ev = r.events
    key = list(zip(*(ev[f].tolist() for f in ("i", "k", "edge", "seg"))))
    assert len(ev) > 3
    # capacity 0 with a NULL buffer: counted, not stored
    lib = e._lib
    pack = amd.engine._ClearancePack([(n, SAMPLES)], *amd.engine._clearance_road("clearance", road), [0], True)
    out = amd.ffi.ClearanceOut()
    assert lib.csf_clearance(e._h, 0, SAMPLES, C.byref(pack.road), d_event, C.byref(out)) == 0 and out.n_events == r.n_events and out.first_sample == 0
    # a capacity below the total: the total is still right, and what is stored is some of the crossings
    some = np.zeros(3, amd.engine.CLEARANCE_EVENT_DTYPE)
    out.events, out.event_capacity = some.ctypes.data, 3
    assert lib.csf_clearance(e._h, 0, SAMPLES, C.byref(pack.road), d_event, C.byref(out)) == 0 and out.n_events == r.n_events > 3
    stored = {tuple(int(s[f]) for f in ("i", "k", "edge", "seg")) for s in some}
    assert len(stored) == 3 and stored <= set(key)
    for s in some:
        w = ev[key.index(tuple(int(s[f]) for f in ("i", "k", "edge", "seg")))]
        assert all(s[f] == w[f] for f in ev.dtype.names)
    # a guess that is too small: exactly one second call, with the exact capacity
    calls = []

    class Counting:                                             # (the library, with the wrapper's calls counted)
        def __getattr__(self, name):
            if name != "csf_clearance":
                return getattr(lib, name)

            def call(*args):
                calls.append(int(args[-1][0].event_capacity))
                return lib.csf_clearance(*args)
            return call
    monkeypatch.setattr(amd.engine, "_clearance_capacity_guess", lambda stations: 3)
    e._lib = Counting()
    try:
        small = e.clearance(0, SAMPLES, road, d_event, events=True)
    finally:
        e._lib = lib
    assert calls == [3, r.n_events]
    same_events(small.events, r.events)
    same_bits(small, r)


# ---- 9. launches ---------------------------------------------------------------------------------------------------------------------------
def test_three_launches_per_call_that_covers_a_sample(amd):
    for n in (3, 257):
        e = recorded_crowd(amd, n)
        road, d_event = road_of(n, THREE_CHUNKS)
        assert e.clearance_launches() == 0
        for k, (first, count) in enumerate(((0, SAMPLES), (1, 2), (3, 3), (2, 1)), start=1):
            e.clearance(first, count, road, d_event, events=k == 1)
            assert e.clearance_launches() == 3 * k
        e.clearance(2, 0, road, d_event)                         # no sample: no launch
        assert e.clearance_launches() == 12 and e.flow_launches() == 0 and e.passing_launches() == 0 and e.encounter_launches() == 0


# ---- 10. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_have_a_message_and_no_side_effect(amd):
    from calib_common import data_set, pod_sets
    a, twin = (crowd(amd, 40, 30.0, seed=10, ring=4, stride=1) for _ in range(2))
    plain = crowd(amd, 40, 30.0, seed=10, ring=None)
    a.step(6); twin.step(6); plain.step(6)
    lib = a._lib
    n = 40
    off, xy = cc.road(30.0, 7)
    arrays = dict(d=np.full((4, n), -7.0), cross=np.full((3, n), -7, np.int32), d_min=np.full(n, -7.0), cross_n=np.full(n, -7, np.int32),
                  near_count=np.full(4, -7, np.int32), cross_count=np.full(3, -7, np.int32), ev=np.zeros(8, amd.engine.CLEARANCE_EVENT_DTYPE))

    def out(**kw):
        o = amd.ffi.ClearanceOut()
        for f in ("d", "cross", "d_min", "cross_n", "near_count", "cross_count"):
            setattr(o, f, arrays[f].ctypes.data)
        o.n_events = -7
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    keep = []

    def rd(off=off, xy=xy, **kw):
        """a csf_clearance_road as given, unchecked"""
        y = amd.ffi.ClearanceRoad()
        o, v = np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(xy, dtype=np.float64)
        keep.extend((o, v))
        y.offsets, y.xy, y.n_edges = o.ctypes.data, v.ctypes.data, len(o) - 1
        for k, w in kw.items():
            setattr(y, k, w)
        return y

    def xy_with(row, col, v):
        q = xy.copy()
        q[row, col] = v
        return q

    flat = xy.copy()
    flat[4] = flat[3]                                            # edge 1, segment 0 has no length
    ev = arrays["ev"].ctypes.data
    ok = rd()
    big = np.zeros(((1 << 20) + 2, 2))
    big[:, 0] = np.arange(len(big))
    cases = {
        "out NULL": (a, 2, 4, ok, 1.0, None), "road NULL": (a, 2, 4, None, 1.0, out()),
        "n_edges 0": (a, 2, 4, rd(n_edges=0), 1.0, out()), "n_edges < 0": (a, 2, 4, rd(n_edges=-1), 1.0, out()),
        "offsets NULL": (a, 2, 4, rd(offsets=None), 1.0, out()), "xy NULL": (a, 2, 4, rd(xy=None), 1.0, out()),
        "a polyline of one vertex": (a, 2, 4, rd(off=[0, 3, 4, 9, 11]), 1.0, out()), "offsets that fall": (a, 2, 4, rd(off=[0, 6, 3, 9, 11]), 1.0, out()),
        "offsets that do not start at 0": (a, 2, 4, rd(off=[1, 3, 6, 9, 11]), 1.0, out()),
        "more than 2^20 segments": (a, 2, 4, rd(off=[0, len(big)], xy=big), 1.0, out()),
        "a coordinate NaN": (a, 2, 4, rd(xy=xy_with(4, 1, NAN)), 1.0, out()), "a coordinate inf": (a, 2, 4, rd(xy=xy_with(0, 0, INF)), 1.0, out()),
        "a segment of no length": (a, 2, 4, rd(xy=flat), 1.0, out()), "dd overflows": (a, 2, 4, rd(xy=xy_with(1, 0, 1e200)), 1.0, out()),
        "d_event negative": (a, 2, 4, ok, -0.5, out()), "d_event NaN": (a, 2, 4, ok, NAN, out()), "d_event inf": (a, 2, 4, ok, INF, out()),
        "the current state has no station": (a, -1, 1, ok, 1.0, out()), "first below -1": (a, -2, 2, ok, 1.0, out()),
        "no ring": (plain, 2, 4, ok, 1.0, out()), "no ring, an empty window": (plain, 0, 0, ok, 1.0, out()),
        "n_samples < 0": (a, 2, -1, ok, 1.0, out()), "n_samples above 65535": (a, 2, 65536, ok, 1.0, out()),
        "samples gone from the ring": (a, 1, 4, ok, 1.0, out()), "samples not yet there": (a, 4, 3, ok, 1.0, out()),
        "capacity < 0": (a, 2, 4, ok, 1.0, out(events=ev, event_capacity=-1)),
        "capacity without a buffer": (a, 2, 4, ok, 1.0, out(event_capacity=8)),
    }
    n0 = {id(e): e.clearance_launches() for e in (a, plain)}
    for name, (e, first, count, y, d_event, o) in cases.items():
        rc = lib.csf_clearance(e._h, first, count, None if y is None else C.byref(y), d_event, None if o is None else C.byref(o))
        assert rc in (-1, -4), (name, rc)
        assert lib.csf_last_error(e._h).decode(), name
        assert o is None or o.n_events == -7, name
        assert e.clearance_launches() == n0[id(e)], name
    assert all((arrays[f] == -7).all() for f in arrays if f != "ev")
    lib.csf_clearance(a._h, 2, 4, C.byref(rd(xy=flat)), 1.0, C.byref(out()))
    msg = lib.csf_last_error(a._h).decode()
    assert "edge 1" in msg and "segment 0" in msg, msg           # the message names edge and segment
    # the largest road is allowed: 2^20 segments (40 road users x 1 sample x 2^20 = 2^25.3 tests)
    o = out(d=None, cross=None, d_min=None, cross_n=None, near_count=None, cross_count=None)
    assert lib.csf_clearance(a._h, 2, 1, C.byref(rd(off=[0, len(big) - 1], xy=big[:-1])), 1.0, C.byref(o)) == 0 and o.n_events == 0 and o.first_sample == 2
    assert a.clearance_launches() == n0[id(a)] + 3
    # the ordinary call writes every array
    o = out()
    assert lib.csf_clearance(a._h, 2, 4, C.byref(ok), 1.0, C.byref(o)) == 0 and o.first_sample == 2 and o.n_events >= 0
    assert not any((arrays[f] == -7).any() for f in arrays if f != "ev")
    assert a.clearance_launches() == n0[id(a)] + 6
    for f in arrays:
        if f != "ev":
            arrays[f][:] = -7
    # a call without a sample succeeds and finds nothing, without a launch
    o = out()
    assert lib.csf_clearance(a._h, 3, 0, C.byref(ok), 1.0, C.byref(o)) == 0 and o.n_events == 0 and o.first_sample == 3
    assert np.isinf(arrays["d_min"]).all() and (arrays["cross_n"] == 0).all()
    assert all((arrays[f] == -7).all() for f in ("d", "cross", "near_count", "cross_count"))      # (arrays without rows)
    assert a.clearance_launches() == n0[id(a)] + 6
    # the refused engine is where its twin is
    assert np.array_equal(a.state(), twin.state())
    a.step(5); twin.step(5)
    assert np.array_equal(a.state(), twin.state())
    assert np.array_equal(a.recorded(7, 4)[0], twin.recorded(7, 4)[0])
    # a member of a loopback group
    g = [crowd(amd, 40, 30.0, seed=10, ring=4, stride=1) for _ in range(2)]
    amd.Engine.loopback_group(g)
    o = out()
    rc = lib.csf_clearance(g[0]._h, 0, 2, C.byref(ok), 1.0, C.byref(o))
    assert rc == -4 and lib.csf_last_error(g[0]._h).decode() and g[0].clearance_launches() == 0 and o.n_events == -7
    # an engine that holds a calibration data set
    sets = pod_sets("twod", 2)
    cs0, cFx, cFy = data_set("twod", n_seq=2, ticks=20)
    c = amd.Engine(sets[0], 4)
    c.calib_load(cs0, cFx, cFy, np.zeros((20, 2, 2)), [0, 1], max_sets=2)
    rc = lib.csf_clearance(c._h, 0, 2, C.byref(ok), 1.0, C.byref(o))
    assert rc == -4 and lib.csf_last_error(c._h).decode() and c.clearance_launches() == 0
    # the batched call: not a batch, NULL outs or road, a bad road, a bad threshold, too many samples, too many chunks
    outs = (amd.ffi.ClearanceOut * 2)()
    arr = (C.c_void_p * 2)(a._h, twin._h)
    assert lib.csf_batch_clearance(arr, 2, 2, C.byref(ok), 1.0, outs) == -4
    amd.Engine.batch_join([a, twin])
    n1 = a.clearance_launches()
    assert lib.csf_batch_clearance(arr, 2, 2, C.byref(ok), 1.0, None) == -1
    assert lib.csf_batch_clearance(arr, 2, 2, None, 1.0, outs) == -1
    assert lib.csf_batch_clearance(arr, 2, 2, C.byref(rd(xy=flat)), 1.0, outs) == -1
    assert lib.csf_batch_clearance(arr, 2, 2, C.byref(ok), -1.0, outs) == -1
    assert lib.csf_batch_clearance(arr, 2, -1, C.byref(ok), 1.0, outs) == -1
    assert lib.csf_batch_clearance(arr, 2, 5, C.byref(ok), 1.0, outs) == -1              # more than the ring of 4 holds
    assert a.clearance_launches() == n1
    assert lib.csf_batch_clearance(arr, 2, 2, C.byref(ok), 1.0, outs) == 0 and a.clearance_launches() == n1 + 3
    assert outs[0].first_sample == 9 and outs[1].first_sample == 9
    amd.Engine.batch_leave([a, twin])
    many = [crowd(amd, 2, ring=4, stride=1) for _ in range(33)]  # 33 members x 2 048 chunks
    amd.Engine.batch_join(many)
    amd.Engine.step_batch(many, 4)
    outs = (amd.ffi.ClearanceOut * 33)()
    arr = (C.c_void_p * 33)(*[e._h for e in many])
    assert lib.csf_batch_clearance(arr, 33, 2, C.byref(rd(off=[0, len(big) - 1], xy=big[:-1])), 1.0, outs) == -1 and lib.csf_last_error(many[0]._h).decode()
    assert many[0].clearance_launches() == 0
    assert lib.csf_batch_clearance(arr, 33, 2, C.byref(ok), 1.0, outs) == 0 and many[0].clearance_launches() == 3
    assert all(o.first_sample == 2 for o in outs)
    amd.Engine.batch_leave(many)
    # (sample, road user) cells x segments above 2^40: 16 400 road users x 64 samples x 2^20 segments
    wide = crowd(amd, 16400, 400.0, ring=64, stride=1)
    wide.step(64)
    o = out(d=None, cross=None, d_min=None, cross_n=None, near_count=None, cross_count=None)
    rc = lib.csf_clearance(wide._h, 0, 64, C.byref(rd(off=[0, len(big) - 1], xy=big[:-1])), 1.0, C.byref(o))
    assert rc == -1 and "2^40" in lib.csf_last_error(wide._h).decode() and wide.clearance_launches() == 0 and o.n_events == -7


# ---- 11. intersections ---------------------------------------------------------------------------------------------------------------------
def test_intersections_together(amd):
    from cyclistsocialforce_amd import intersection as ci
    from cyclistsocialforce_amd.vehicle import TwoDBicycle
    (off, xy), d_event = road_of(3, 7)
    edges = [ci.RoadEdge(xy[off[k]:off[k + 1]]) for k in range(len(off) - 1)]
    scenes = []
    for k in range(3):
        s0 = cc.placed(3)
        s0[:, 0] += 0.2 * k
        vs = []
        for j, s in enumerate(s0):
            v = TwoDBicycle(tuple(s), id=f"s{k}r{j}")
            v.setDestinations(s[0] + np.array([30.0, 60.0]) * np.cos(s[2]), s[1] + np.array([30.0, 60.0]) * np.sin(s[2]))
            vs.append(v)
        scenes.append(ci.SocialForceIntersection(vs))
    ci.advance_together(scenes, 120)                              # (the dense route records every tick)
    res = ci.clearance_together(scenes, 120, edges, d_event, events=True)
    for k, (ins, r) in enumerate(zip(scenes, res)):
        alone = ins.clearance(r.first, 120, (off, xy), d_event, events=True)
        same_bits(r, alone)
        same_events(r.events, alone.events)
        assert r.ids == alone.ids == [f"s{k}r{j}" for j in range(3)] and r.period == pytest.approx(0.01)
        assert list(r.event_i_id) == [r.ids[i] for i in r.events["i"]] and list(alone.event_i_id) == list(r.event_i_id)
        ref = cc.reference(ins.engine.recorded(r.first, 120)[0], (off, xy), d_event)
        same_bits(r, ref)
        same_events(r.events, cc.events(ref))
        invariants(r)
        with pytest.raises(ValueError):
            ins.clearance(r.first, 120)                          # road=None, and the intersection has no road_elements
    plain = ci.clearance_together(scenes, 120, (off, xy), d_event)
    assert plain[0].events is None and plain[0].event_i_id is None and plain[0].ids == res[0].ids
