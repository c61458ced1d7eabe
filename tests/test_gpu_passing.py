"""Following and passing on the MI355X (include/csf.h: csf_passing, csf_batch_passing; csf_passing.hip) against the
definition in NumPy fp64 (tests/passing_common.py), applied to the states read back with Engine.recorded: engine and reference
start from identical bits.

The comparison is BIT FOR BIT - the per-station, per-interval and run_* arrays, the counts and the events - and no cell is left
out.  That is derivable, not measured: every input is the ring's fp64 bits, every operation is one IEEE operation in a stated
order without contraction, sqrt and division are correctly rounded, and no transcendental is involved.

Every case with a population asserts from the reference alone that it is not vacuous: at least one passing, and from 33 riders on
at least one overtaking, one meeting, a quarter of the riders making a passing and a quarter with a leader at some station (seed 0
of every size on the CPU oracle's trajectories, band 1 m: 33 riders 48 passings of which 37 meetings, 23 riders that pass, 25 with
a leader; 70: 89 (73), 49, 53; 257: 369 (310), 190, 225; 300: 496 (414), 235, 261; 1 100: 2 447 (1 939), 933, 1 039)."""
import ctypes as C

import numpy as np
import pytest

import passing_common as pc

pytestmark = pytest.mark.gpu

INF = float("inf")
STRIDE = 20                     # x t_s = 0.01 s: a sample every 0.2 s
SAMPLES = 8
BAND, LAT_MAX = 1.0, 3.0
BOX = {33: 20.0, 70: 30.0, 257: 60.0, 300: 60.0, 1100: 100.0}     # (test_gpu_pet.py's)
SEED = 0
PER = pc.STATION + pc.INTERVAL


@pytest.fixture(scope="module")
def amd():
    from cyclistsocialforce_amd import _ffi, engine, parameters

    class NS:
        pass

    ns = NS()
    ns.Engine, ns.pod, ns.ffi, ns.engine = engine.Engine, parameters.default_pod, _ffi, engine
    return ns


def crowd(amd, n, box=None, seed=SEED, ring=SAMPLES, stride=STRIDE, s0=None, history=False):
    """n road users scattered in a box (two or three: placed by hand), riding towards destinations ahead of them; ring: the capacity
    of a state ring of every `stride`-th tick (None: no recording; history: csf_enable_history's ring instead of csf_record's)"""
    pod = amd.pod("twod")
    ns = amd.ffi.N_STATES[pod.model]
    if s0 is None:
        s0 = pc.placed(n, ns=ns) if n in (2, 3) else pc.scatter(n, box or BOX.get(n, 6.0), seed, ns=ns)
    vdes = s0[:, 3].copy() if n in (2, 3) else 5.0               # (the placed riders keep their speeds: a slow one stays slow)
    e = amd.Engine(pod, max(n, 1))
    e.add_agents(s0, vdes)
    e.set_dest_queue(np.arange(n), *pc.with_queue(s0), reset=True)
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
    X = ref.passings
    over, meet = int((X["kind"] > 0).sum()), int((X["kind"] < 0).sum())
    passers, led = int((ref.run_made.sum(1) > 0).sum()), int(np.isfinite(ref.run_gap).sum())
    print(f"{what}: {n} riders, {len(X)} passings ({over} overtakings, {meet} meetings), {passers} riders that pass, {led} with a leader")
    assert len(X) >= 1, "vacuous: the reference finds no passing"
    if n >= 33:
        assert over >= 1 and meet >= 1, f"vacuous: {over} overtakings, {meet} meetings"
        assert 4 * passers >= n, f"vacuous: {passers} of {n} riders make a passing"
        assert 4 * led >= n, f"vacuous: {led} of {n} riders have a leader"


def same_bits(got, ref, per_station=True, what=""):
    """every array of a Passing against the reference's (or another Passing's): the same bits, NaN where NaN"""
    for f in (PER if per_station else ()) + pc.RUN:
        g, w = getattr(got, f), getattr(ref, f)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f, g.dtype, w.dtype, g.shape, w.shape)
        if not np.array_equal(g, w, equal_nan=g.dtype.kind == "f"):
            bad = np.argwhere(~((g == w) | ((g != g) & (w != w))))
            raise AssertionError(f"{what}: {f} differs in {len(bad)} of {g.size} cells, first {bad[:4].tolist()}: "
                                 + ", ".join(f"{g[tuple(b)]!r} ({np.asarray(g[tuple(b)]).tobytes().hex()}) against {w[tuple(b)]!r} ({np.asarray(w[tuple(b)]).tobytes().hex()})" for b in bad[:4]))


def same_events(ev, ref_ev):
    assert ev.dtype == ref_ev.dtype and len(ev) == len(ref_ev)
    for f in ev.dtype.names:
        assert np.array_equal(ev[f], ref_ev[f], equal_nan=f == "cosine"), f


def invariants(r, n):
    """what holds of every result with lat_event = +inf"""
    assert r.n_events == len(r.events) == int(r.run_made.sum())
    assert np.array_equal(r.run_made.sum(0), r.run_by.sum(0))
    lat, w, t, kind = pc.by_from_events(r.events, n, r.by_lat.shape[0])      # the events, transposed, reproduce by_*
    assert np.array_equal(lat, r.by_lat) and np.array_equal(w, r.by_with) and np.array_equal(t, r.by_t, equal_nan=True) and np.array_equal(kind, r.by_kind)
    assert np.array_equal(np.bincount(r.events["i"], minlength=n), r.run_made.sum(1))
    assert np.array_equal(np.bincount(r.events["j"], minlength=n), r.run_by.sum(1))


def check(e, first, count, what, vacuous=True, states=None):
    """passing(first, count, every passing an event) against the reference on recorded(first, count); returns both"""
    S = e.recorded(first, count)[0] if states is None else states
    ref = pc.reference(S, BAND, LAT_MAX)
    if vacuous:
        not_vacuous(ref, e.n, what)
    r = e.passing(first, count, BAND, LAT_MAX, lat_event=INF)
    assert r.first == first
    same_bits(r, ref, what=what)
    same_events(r.events, pc.events(ref, INF))
    invariants(r, e.n)
    return r, ref


# ---- 1, 2, 3: against NumPy, not vacuous, the invariants ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 33, 70, 257, 300, 1100])
def test_against_numpy(amd, n):
    """one rider; the head-on pair and the slow rider ahead on the packed path; 33: the first size of the tiled path, one tile with
    a tail; 257 and 300 across the tile boundary; 1 100: five tiles whose partners are split over several chunks"""
    e = recorded_crowd(amd, n)
    r, ref = check(e, 0, SAMPLES, f"n = {n}", vacuous=n > 1)
    assert r.gap.shape == (SAMPLES - 1, n) and r.made_lat.shape == (SAMPLES - 2, n) and r.run_made.shape == (n, 3)
    assert r.period == pytest.approx(0.2)
    if n == 1:
        assert np.isinf(r.gap).all() and (r.gap_with == -1).all() and np.isinf(r.made_lat).all() and np.isnan(r.made_t).all()
        assert np.isinf(r.run_gap).all() and (r.run_gap_k == -1).all() and r.run_made.sum() == 0 and r.n_events == 0
    if n == 2:
        assert (ref.passings["kind"] < 0).all() and len(ref.passings) == 2        # the meeting, as either rider reports it
    if n == 3:
        assert (ref.passings["kind"] > 0).any() and np.isfinite(ref.run_gap[0])   # the slow rider is overtaken, and led before that
    s = r.in_seconds()
    assert np.array_equal(s.thw, r.thw * 0.2, equal_nan=True) and np.array_equal(s.made_t, r.made_t * 0.2, equal_nan=True)
    assert np.array_equal(s.events["t"], r.events["t"] * 0.2) and np.array_equal(s.events["closing"], r.events["closing"] / 0.2)
    assert np.array_equal(s.gap, r.gap, equal_nan=True) and np.array_equal(s.events["lat"], r.events["lat"])


# ---- 4. a sub-window ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 70])
def test_a_sub_window(amd, n):
    e = recorded_crowd(amd, n)
    full = e.passing(0, SAMPLES, BAND, LAT_MAX)
    sub = e.passing(2, 4, BAND, LAT_MAX)
    assert sub.first == 2 and sub.gap.shape == (3, n) and sub.made_lat.shape == (2, n) and sub.events is None
    for f in pc.STATION:
        assert np.array_equal(getattr(sub, f), getattr(full, f)[2:5], equal_nan=True), f
    for f in pc.INTERVAL:
        a, b = getattr(sub, f), getattr(full, f)[2:4]
        if f.endswith("_t"):                                     # (t counts from the call's first sample: k + s against (k - 2) + s)
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.allclose(a[~np.isnan(a)] + 2.0, b[~np.isnan(b)], rtol=0, atol=1e-12), f
        else:
            assert np.array_equal(a, b, equal_nan=True), f
    same_bits(sub, pc.reference(e.recorded(2, 4)[0], BAND, LAT_MAX))
    w = e.passing(0, SAMPLES, BAND, LAT_MAX, per_station=False)  # the road users' rows alone: the same bits
    assert w.gap is None and w.made_lat is None and w.by_kind is None and w.events is None and w.n_events == 0
    same_bits(w, full, per_station=False)
    for count in (0, 1):                                         # no station: nothing found
        one = e.passing(2, count, BAND, LAT_MAX, lat_event=INF)
        assert one.gap.shape == (0, n) and one.made_lat.shape == (0, n) and np.isinf(one.run_gap).all() and np.isinf(one.run_thw).all()
        assert (one.run_gap_with == -1).all() and (one.run_gap_k == -1).all() and (one.run_thw_k == -1).all() and np.isinf(one.run_made_lat).all()
        assert np.isnan(one.run_made_t).all() and np.isnan(one.run_by_t).all() and (one.run_made_kind == 0).all() and (one.run_by_with == -1).all()
        assert one.run_made.sum() == 0 and one.run_by.sum() == 0 and one.n_events == 0 and len(one.events) == 0
    two = e.passing(2, 2, BAND, LAT_MAX, lat_event=INF)          # one station, no interval
    assert two.gap.shape == (1, n) and two.made_lat.shape == (0, n) and two.n_events == 0
    same_bits(two, pc.reference(e.recorded(2, 2)[0], BAND, LAT_MAX))


# ---- 5. non-finite -----------------------------------------------------------------------------------------------------------------------
def test_a_rider_whose_x_becomes_nan(amd):
    n, gone = 70, 5
    e = crowd(amd, n)
    e.step(4 * STRIDE)
    bad = e.state()[gone].copy()
    bad[0] = np.nan
    e.push_state([gone], bad)
    e.step(4 * STRIDE)
    S, _ = e.recorded(0, SAMPLES)
    assert np.isnan(S[4:, gone, 0]).all() and np.isfinite(S[:4, gone, 0]).all()
    r, ref = check(e, 0, SAMPLES, "n = 70, one rider NaN from sample 4 on", vacuous=False)
    assert len(ref.passings) >= 1
    assert np.isnan(r.gap[3:, gone]).all() and np.isnan(r.thw[3:, gone]).all() and (r.gap_with[3:, gone] == -1).all()
    assert np.isnan(r.made_lat[3:, gone]).all() and (r.made_with[3:, gone] == -1).all() and not np.isnan(r.gap[:3, gone]).any()
    assert not np.isnan(np.delete(r.gap, gone, axis=1)).any() and not (r.gap_with[3:] == gone).any() and not (r.by_with[2:] == gone).any()


# ---- 6. rings and ticks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 70])
def test_a_wrapped_ring(amd, n):
    """capacity 5, 8 samples taken: samples 3 .. 7 sit in slots 3, 4, 0, 1, 2"""
    s0 = None
    if n == 3:                                                   # (the three start further apart, so that they meet inside the window)
        s0 = pc.placed(3)
        s0[1, 0] += 4.0
        s0[2, 0] += 1.2
    e = crowd(amd, n, ring=5, s0=s0)
    e.step(8 * STRIDE)
    check(e, 3, 5, f"n = {n}, samples 3 .. 7 of a ring of 5")
    n0 = e.passing_launches()
    for first, count in ((0, 3), (2, 2), (0, 8), (4, 5), (8, 1)):
        with pytest.raises(amd.engine.EngineError):
            e.passing(first, count)
    assert e.passing_launches() == n0


def test_a_ring_of_enable_history(amd):
    e = crowd(amd, 70, history=True)
    e.step(STRIDE * SAMPLES)
    check(e, 0, SAMPLES, "n = 70, the ring of enable_history", states=e.history(0, SAMPLES))


@pytest.mark.auto_variant
@pytest.mark.parametrize("n", [3, 70, 3000])
def test_passing_between_steps_leaves_the_run_alone(amd, n):
    """the engine's own tick for the size - one wave, one launch, pair + per-agent launches -: step(5), passing, step(5) ends bit for
    bit where step(10) of a twin ends, and what the call returns is the reference's bits"""
    box = max(BOX.get(n, 0.0), 3.0 * np.sqrt(n))
    a, b = (crowd(amd, n, box, seed=90 + n, ring=16, stride=1) for _ in range(2))
    a.step(5)
    r = a.passing(0, 5, BAND, LAT_MAX, lat_event=INF)
    assert r.gap.shape == (4, n) and a.passing_launches() == 2
    if n < 3000:
        same_bits(r, pc.reference(a.recorded(0, 5)[0], BAND, LAT_MAX))
    else:                                                        # (three samples: a few seconds of NumPy)
        same_bits(a.passing(0, 3, BAND, LAT_MAX), pc.reference(a.recorded(0, 3)[0], BAND, LAT_MAX))
        assert np.isfinite(r.run_gap).sum() * 4 >= n
    invariants(r, n)
    ticks = (a.small_ticks(), a.mid_ticks())
    assert (ticks[0] > 0) == (n == 3) and (ticks[1] > 0) == (n == 70)
    a.step(5)
    b.step(10)
    assert np.array_equal(a.state(), b.state())
    fa, fb = a.forces(), b.forces()
    assert np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1])
    assert a.small_ticks() == b.small_ticks() and a.mid_ticks() == b.mid_ticks()
    assert np.array_equal(a.recorded(0, 10)[0], b.recorded(0, 10)[0])


# ---- 7. determinism ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 1100])
def test_the_call_made_twice_gives_the_same_bits(amd, n):
    e = recorded_crowd(amd, n)
    a = e.passing(0, SAMPLES, BAND, LAT_MAX, lat_event=INF)
    b = e.passing(0, SAMPLES, BAND, LAT_MAX, lat_event=INF)
    same_bits(a, b)
    same_events(a.events, b.events)
    assert a.n_events >= 1


# ---- 8. batch ----------------------------------------------------------------------------------------------------------------------------
def test_batch_equals_every_member_alone_in_two_launches(amd):
    rng = np.random.default_rng(600)
    members = []
    for k in range(8):
        s0 = pc.placed(3)
        s0[:, :2] += rng.uniform(-0.2, 0.2, (3, 2))
        members.append(crowd(amd, 3, s0=s0))
    members.append(crowd(amd, 70))
    silent = crowd(amd, 3, ring=None)                            # does not record
    engines = members + [silent]
    amd.Engine.batch_join(engines)
    amd.Engine.step_batch(engines, STRIDE * SAMPLES)
    n0 = [e.passing_launches() for e in engines]
    res = amd.Engine.batch_passing(engines, SAMPLES, BAND, LAT_MAX, lat_event=INF)
    assert engines[0].passing_launches() == n0[0] + 2            # the documented constant: the pair launch and the window pass
    assert [e.passing_launches() for e in engines[1:]] == n0[1:]
    assert res[-1] is None and all(r is not None for r in res[:-1])
    for e, r in zip(members, res):
        alone = e.passing(0, SAMPLES, BAND, LAT_MAX, lat_event=INF)
        assert r.first == 0 and r.gap.shape == (SAMPLES - 1, e.n) and r.period == pytest.approx(0.2)
        same_bits(r, alone)
        same_events(r.events, alone.events)
    for at in (8, 5):
        ref = pc.reference(members[at].recorded(0, SAMPLES)[0], BAND, LAT_MAX)
        not_vacuous(ref, members[at].n, f"member {at} of the batch")
        same_bits(res[at], ref)
        same_events(res[at].events, pc.events(ref, INF))
    outs = (amd.ffi.PassingOut * len(engines))()                 # the non-recording member at the ABI: first_sample -2
    arr = (C.c_void_p * len(engines))(*[e._h for e in engines])
    assert engines[0]._lib.csf_batch_passing(arr, len(engines), SAMPLES, BAND, LAT_MAX, 0.0, outs) == 0
    assert outs[len(engines) - 1].first_sample == -2 and outs[len(engines) - 1].n_events == 0 and outs[0].first_sample == 0
    plain = amd.Engine.batch_passing(engines, SAMPLES, BAND, LAT_MAX, per_station=False)
    assert plain[3].gap is None and plain[3].events is None
    same_bits(plain[3], res[3], per_station=False)
    n1 = engines[0].passing_launches()                           # more samples than a member's ring holds: refused before anything is written
    with pytest.raises(amd.engine.EngineError):
        amd.Engine.batch_passing(engines, SAMPLES + 1)
    assert engines[0].passing_launches() == n1
    amd.Engine.batch_leave(engines)


# ---- 9. events ---------------------------------------------------------------------------------------------------------------------------
def test_events(amd, monkeypatch):
    n = 70
    e = recorded_crowd(amd, n)
    r, ref = check(e, 0, SAMPLES, "events, n = 70")              # every passing, sorted, equal to the reference's list
    ev = r.events
    key = list(zip(ev["i"].tolist(), ev["j"].tolist(), ev["k"].tolist()))
    assert key == sorted(key) and len(set(key)) == len(key) and (ev["i"] != ev["j"]).all() and len(ev) >= 5
    thr = float(np.median(np.abs(ev["lat"])))
    sub = e.passing(0, SAMPLES, BAND, LAT_MAX, lat_event=thr)
    same_events(sub.events, pc.events(ref, thr))
    assert 0 < sub.n_events < r.n_events
    same_bits(sub, r)                                            # the rows do not depend on the events
    off = e.passing(0, SAMPLES, BAND, LAT_MAX, lat_event=0.0)
    assert off.events is None and off.n_events == 0
    same_bits(off, r)
    # capacity 0 with a NULL buffer: counted, not stored
    lib = e._lib
    out = amd.ffi.PassingOut()
    assert lib.csf_passing(e._h, 0, SAMPLES, BAND, LAT_MAX, INF, C.byref(out)) == 0 and out.n_events == r.n_events and out.first_sample == 0
    # over capacity: the total is still right, and what is stored is one of the passings
    one = np.zeros(1, amd.engine.PASSING_EVENT_DTYPE)
    out.events, out.event_capacity = one.ctypes.data, 1
    assert lib.csf_passing(e._h, 0, SAMPLES, BAND, LAT_MAX, INF, C.byref(out)) == 0 and out.n_events == r.n_events
    assert (int(one["i"][0]), int(one["j"][0]), int(one["k"][0])) in set(key)
    # a guess that is too small: exactly one second call, with the exact capacity
    calls = []

    class Counting:                                             # (the library, with the wrapper's calls counted)
        def __getattr__(self, name):
            if name != "csf_passing":
                return getattr(lib, name)

            def call(*args):
                calls.append(int(args[-1][0].event_capacity))
                return lib.csf_passing(*args)
            return call
    monkeypatch.setattr(amd.engine, "_passing_capacity_guess", lambda cells: 3)
    e._lib = Counting()
    try:
        small = e.passing(0, SAMPLES, BAND, LAT_MAX, lat_event=INF)
    finally:
        e._lib = lib
    assert calls == [3, r.n_events] and r.n_events > 3
    same_events(small.events, r.events)


# ---- 10. launches ------------------------------------------------------------------------------------------------------------------------
def test_two_launches_per_call_that_covers_a_station(amd):
    for n in (3, 300):
        e = recorded_crowd(amd, n)
        assert e.passing_launches() == 0
        for k, (first, count) in enumerate(((0, SAMPLES), (1, 2), (3, 3)), start=1):
            e.passing(first, count, lat_event=INF if k == 1 else None)
            assert e.passing_launches() == 2 * k
        for count in (0, 1):
            e.passing(2, count)
        assert e.passing_launches() == 6 and e.pet_launches() == 0 and e.encounter_launches() == 0


# ---- 11. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_have_a_message_and_no_side_effect(amd):
    from calib_common import data_set, pod_sets
    a, twin = (crowd(amd, 40, 30.0, seed=10, ring=4, stride=1) for _ in range(2))
    plain = crowd(amd, 40, 30.0, seed=10, ring=None)
    a.step(6); twin.step(6); plain.step(6)
    lib = a._lib
    n = 40
    arrays = dict(g=np.full((3, n), -7.0), w=np.full((3, n), -7, np.int32), m=np.full((2, n), -7.0), rg=np.full(n, -7.0), rc=np.full((n, 3), -7, np.int32),
                  ev=np.zeros(8, amd.engine.PASSING_EVENT_DTYPE))

    def out(**kw):
        o = amd.ffi.PassingOut()
        o.gap, o.gap_with, o.made_lat, o.run_gap, o.run_made = (arrays[f].ctypes.data for f in ("g", "w", "m", "rg", "rc"))
        o.n_events = -7
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    ev = arrays["ev"].ctypes.data
    nan = float("nan")
    ok = (0.75, 3.0, 0.0)
    cases = {
        "out NULL": (a, 2, 4, ok, None),
        "the current state has no direction": (a, -1, 1, ok, out()), "first below -1": (a, -2, 2, ok, out()),
        "no ring": (plain, 2, 4, ok, out()), "no ring, an empty window": (plain, 0, 0, ok, out()),
        "n_samples < 0": (a, 2, -1, ok, out()), "n_samples above 65535": (a, 2, 65536, ok, out()),
        "samples gone from the ring": (a, 1, 4, ok, out()), "samples not yet there": (a, 4, 3, ok, out()),
        "band NaN": (a, 2, 4, (nan, 3.0, 0.0), out()), "band negative": (a, 2, 4, (-0.1, 3.0, 0.0), out()), "band -inf": (a, 2, 4, (-INF, 3.0, 0.0), out()),
        "lat_max NaN": (a, 2, 4, (0.75, nan, 0.0), out()), "lat_max 0": (a, 2, 4, (0.75, 0.0, 0.0), out()), "lat_max negative": (a, 2, 4, (0.75, -3.0, 0.0), out()),
        "lat_event NaN": (a, 2, 4, (0.75, 3.0, nan), out()), "lat_event -inf": (a, 2, 4, (0.75, 3.0, -INF), out()),
        "capacity < 0": (a, 2, 4, (0.75, 3.0, 2.0), out(events=ev, event_capacity=-1)),
        "capacity without a buffer": (a, 2, 4, (0.75, 3.0, 2.0), out(event_capacity=8)),
    }
    n0 = {id(e): e.passing_launches() for e in (a, plain)}
    for name, (e, first, count, (band, lat_max, lat_event), o) in cases.items():
        rc = lib.csf_passing(e._h, first, count, band, lat_max, lat_event, None if o is None else C.byref(o))
        assert rc in (-1, -4), (name, rc)
        assert lib.csf_last_error(e._h).decode(), name
        assert o is None or o.n_events == -7, name
        assert e.passing_launches() == n0[id(e)], name
    assert all((arrays[f] == -7).all() for f in ("g", "w", "m", "rg", "rc"))
    # +inf is allowed for all three
    o = out()
    assert lib.csf_passing(a._h, 2, 4, INF, INF, INF, C.byref(o)) == 0 and o.n_events >= 0 and o.first_sample == 2 and not (arrays["g"] == -7).any()
    assert a.passing_launches() == n0[id(a)] + 2
    for f in ("g", "w", "m", "rg", "rc"):
        arrays[f][:] = -7
    # small calls succeed and find nothing, without a launch
    for count in (0, 1):
        o = out()
        assert lib.csf_passing(a._h, 3, count, *ok, C.byref(o)) == 0 and o.n_events == 0 and o.first_sample == 3
        assert np.isinf(arrays["rg"]).all() and (arrays["rc"] == 0).all() and (arrays["g"] == -7.0).all() and (arrays["m"] == -7.0).all()
        arrays["rg"][:], arrays["rc"][:] = -7.0, -7
    assert a.passing_launches() == n0[id(a)] + 2
    # the refused engine is where its twin is
    assert np.array_equal(a.state(), twin.state())
    a.step(5); twin.step(5)
    assert np.array_equal(a.state(), twin.state())
    assert np.array_equal(a.recorded(7, 4)[0], twin.recorded(7, 4)[0])
    # a member of a loopback group
    g = [crowd(amd, 40, 30.0, seed=10, ring=4, stride=1) for _ in range(2)]
    amd.Engine.loopback_group(g)
    o = out()
    rc = lib.csf_passing(g[0]._h, 0, 2, *ok, C.byref(o))
    assert rc == -4 and lib.csf_last_error(g[0]._h).decode() and g[0].passing_launches() == 0 and o.n_events == -7
    # an engine that holds a calibration data set
    sets = pod_sets("twod", 2)
    cs0, cFx, cFy = data_set("twod", n_seq=2, ticks=20)
    c = amd.Engine(sets[0], 4)
    c.calib_load(cs0, cFx, cFy, np.zeros((20, 2, 2)), [0, 1], max_sets=2)
    rc = lib.csf_passing(c._h, 0, 2, *ok, C.byref(o))
    assert rc == -4 and lib.csf_last_error(c._h).decode() and c.passing_launches() == 0
    # the batched call: not a batch, NULL outs, bad shared arguments, too many samples
    outs = (amd.ffi.PassingOut * 2)()
    arr = (C.c_void_p * 2)(a._h, twin._h)
    assert lib.csf_batch_passing(arr, 2, 2, *ok, outs) == -4
    amd.Engine.batch_join([a, twin])
    n1 = a.passing_launches()
    assert lib.csf_batch_passing(arr, 2, 2, *ok, None) == -1
    assert lib.csf_batch_passing(arr, 2, 2, nan, 3.0, 0.0, outs) == -1
    assert lib.csf_batch_passing(arr, 2, 2, 0.75, 0.0, 0.0, outs) == -1
    assert lib.csf_batch_passing(arr, 2, 2, 0.75, 3.0, nan, outs) == -1
    assert lib.csf_batch_passing(arr, 2, -1, *ok, outs) == -1
    assert lib.csf_batch_passing(arr, 2, 5, *ok, outs) == -1                      # more than the ring of 4 holds
    assert a.passing_launches() == n1
    assert lib.csf_batch_passing(arr, 2, 2, *ok, outs) == 0 and a.passing_launches() == n1 + 2
    assert outs[0].first_sample == 9 and outs[1].first_sample == 9
    amd.Engine.batch_leave([a, twin])


# ---- 12. intersections -------------------------------------------------------------------------------------------------------------------
def test_intersections_together(amd):
    from cyclistsocialforce_amd import intersection as ci
    from cyclistsocialforce_amd.vehicle import TwoDBicycle
    scenes = []
    for k in range(3):
        s0 = pc.placed(3)
        s0[:, 0] += 0.2 * k
        vs = []
        for j, s in enumerate(s0):
            v = TwoDBicycle(tuple(s), id=f"s{k}r{j}")
            v.setDestinations(s[0] + np.array([30.0, 60.0]) * np.cos(s[2]), s[1] + np.array([30.0, 60.0]) * np.sin(s[2]))
            vs.append(v)
        scenes.append(ci.SocialForceIntersection(vs))
    ci.advance_together(scenes, 120)                              # (the dense route records every tick)
    res = ci.passing_together(scenes, 120, BAND, LAT_MAX, lat_event=INF)
    for k, (ins, r) in enumerate(zip(scenes, res)):
        alone = ins.passing(r.first, 120, BAND, LAT_MAX, lat_event=INF)
        same_bits(r, alone)
        same_events(r.events, alone.events)
        assert r.ids == [f"s{k}r{j}" for j in range(3)] and r.period == pytest.approx(0.01)
        for f, shape in (("gap_with", (119, 3)), ("made_with", (118, 3)), ("by_with", (118, 3)), ("run_gap_with", (3,)), ("run_thw_with", (3,)),
                         ("run_made_with", (3,)), ("run_by_with", (3,))):
            ids, idx = getattr(r, f + "_id"), getattr(r, f)
            assert ids.shape == shape == idx.shape, f
            assert all((a is None) == (j < 0) and (j < 0 or a == r.ids[j]) for a, j in zip(ids.ravel(), idx.ravel())), f
        assert list(r.event_i_id) == [r.ids[i] for i in r.events["i"]] and list(r.event_j_id) == [r.ids[j] for j in r.events["j"]]
        ref = pc.reference(ins.engine.recorded(r.first, 120)[0], BAND, LAT_MAX)
        not_vacuous(ref, 3, f"intersection {k}")
        same_bits(r, ref)
        same_events(r.events, pc.events(ref, INF))
        assert (r.run_made_with_id != None).any()                # noqa: E711  (element-wise)
