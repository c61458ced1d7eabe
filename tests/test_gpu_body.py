"""Body encounters on the MI355X (include/csf.h: csf_body_encounters, csf_batch_body_encounters; csf_body.hip) against
the definition in NumPy fp64 (tests/body_common.py), applied to the states read back with Engine.recorded / Engine.state: engine and
reference start from identical bits.

Tolerance: window minima against the same call's per-sample arrays, and a rider's row in different calls, bit for bit.  Against NumPy
the values 0 and +inf are exact and the partners equal; other gaps hold to rtol 1e-9 + 1e-9 m, other ttc to rtol 1e-9 + 1e-9 s.  The
only source of a difference is the last bit of the device's sincos: perturbing cos and sin by 1 ulp moved gaps by at most 7e-15 m and
ttc by at most 5e-14 s on these crowds, five orders under the bound.  A (sample, rider) cell is left out where a pair of it has
|sep| < 1e-6 m, or - approaching - |T_in - T_out| < 1e-6 (1 + |T_in|), |T_in| < 1e-6 or a finite ttc decided by an axis with
|g| < 1e-2 m/s, or its two smallest values are within 1e-9 relative without being equal (body_common.fragile); at most 1 % of a
test's cells may be left out, and every test prints the share."""
import ctypes as C

import numpy as np
import pytest

import body_common as bc
import encounter_common as ec

pytestmark = pytest.mark.gpu

BOX = {1: 6.0, 2: 6.0, 3: 6.0, 33: 20.0, 70: 40.0, 257: 80.0, 300: 80.0}
FIELDS = ("gap_min", "gap_with", "ttc_min", "ttc_with", "run_gap_min", "run_gap_with", "run_gap_sample", "run_ttc_min", "run_ttc_with",
          "run_ttc_sample", "overlap_n")


@pytest.fixture(scope="module")
def amd():
    from cyclistsocialforce_amd import _ffi, engine, parameters

    class NS:
        pass

    ns = NS()
    ns.Engine, ns.pod, ns.ffi, ns.engine = engine.Engine, parameters.default_pod, _ffi, engine
    return ns


def crowd(amd, n, box, seed, model="twod", record=None, s0=None):
    """n road users scattered in a box, riding towards destinations ahead of them; record: the capacity of a ring of every tick"""
    pod = amd.pod(model)
    if s0 is None:
        s0 = ec.scatter(n, box, seed, ns=amd.ffi.N_STATES[pod.model])
    e = amd.Engine(pod, max(n, 1))
    e.add_agents(s0, 5.0)
    e.set_dest_queue(np.arange(n), *ec.with_queue(s0), reset=True)
    if record:
        e.record(stride=1, capacity=record, forces=False)
    return e


def check_per_sample(r, S, ext, what=""):
    """the per-sample arrays of a BodyEncounters against the reference on the same states; returns the share of cells left out"""
    p = bc.pairs(S, ext)
    g, gj, t, tj = bc.per_sample(S, ext, p)
    out = bc.fragile(S, ext, p)
    keep = ~out
    share = float(out.mean()) if out.size else 0.0
    print(f"{what}: {out.size} cells, {int(out.sum())} left out ({100 * share:.2f} %), {int(np.isfinite(t).sum())} with a finite ttc, "
          f"{int((g == 0).sum())} overlapping")
    assert share <= 0.01
    assert r.gap_min.shape == g.shape and r.gap_with.dtype == np.int32 and r.ttc_with.dtype == np.int32
    for got, ref, name in ((r.gap_min, g, "gap"), (r.ttc_min, t, "ttc")):
        a, w = got[keep], ref[keep]
        assert np.array_equal(np.isnan(a), np.isnan(w)), name
        exact = np.isinf(w) | (w == 0.0) | np.isnan(w)
        assert np.array_equal(a[exact], w[exact], equal_nan=True), name           # +inf and 0 hold exactly
        if (~exact).any():
            print(f"    {name}: largest difference {np.abs(a[~exact] - w[~exact]).max():.3g}")
        np.testing.assert_allclose(a[~exact], w[~exact], rtol=1e-9, atol=1e-9)
    assert np.array_equal(r.gap_with[keep], gj[keep]) and np.array_equal(r.ttc_with[keep], tj[keep])
    return share


def check_window(r, first):
    """run_* and overlap_n are the reductions of the same call's per-sample arrays: bit for bit"""
    ref = bc.window(r.gap_min, r.gap_with, r.ttc_min, r.ttc_with, first)
    got = (r.run_gap_min, r.run_gap_with, r.run_gap_sample, r.run_ttc_min, r.run_ttc_with, r.run_ttc_sample, r.overlap_n)
    for g, w in zip(got, ref):
        assert g.dtype == w.dtype and np.array_equal(g, w)


def same_bits(a, b):
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f
    assert a.n_events == b.n_events and (a.events is None) == (b.events is None)
    if a.events is not None:
        assert np.array_equal(a.events, b.events)


def key(ev):
    return [(int(a), int(b), int(c)) for a, b, c in zip(ev["sample"], ev["i"], ev["j"])]


# ---- 1. per sample and window against NumPy ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 33, 70, 257, 300])
def test_per_sample_and_window_against_numpy(amd, n):
    """a population of one, the packed path (n <= 32) and its limit + 1, a wave tail, the 256-tile boundary in both directions"""
    e = crowd(amd, n, BOX[n], seed=100 + n, record=8)
    ext = bc.extents(n)
    e.step(5)
    S, _ = e.recorded(0, 5)
    r = e.body_encounters(0, 5, extents=ext)
    assert r.first == 0 and r.events is None and r.n_events == 0
    check_per_sample(r, S, ext, f"n = {n}")
    check_window(r, 0)
    assert np.array_equal(r.overlap_n, (r.gap_min == 0.0).sum(axis=0))
    if n == 1:
        assert np.isinf(r.gap_min).all() and np.isinf(r.ttc_min).all() and (r.gap_with == -1).all() and (r.ttc_with == -1).all()
        assert np.isinf(r.run_gap_min).all() and (r.run_gap_with == -1).all() and (r.run_gap_sample == -1).all() and (r.overlap_n == 0).all()
    # the current state is the last sample
    now = e.body_encounters(extents=ext)
    assert now.first == -1 and now.gap_min.shape == (1, n)
    for f in ("gap_min", "gap_with", "ttc_min", "ttc_with"):
        assert np.array_equal(getattr(now, f)[0], getattr(r, f)[4], equal_nan=True), f
    assert ((now.run_gap_sample == -1) & (now.run_ttc_sample == -1)).all()
    # without per_sample the window alone, the same bits
    w = e.body_encounters(0, 5, extents=ext, per_sample=False)
    assert w.gap_min is None
    for f in FIELDS[4:]:
        assert np.array_equal(getattr(w, f), getattr(r, f)), f


def test_one_triple_is_everybodys(amd):
    e = crowd(amd, 33, 20.0, seed=3)
    a = e.body_encounters(extents=bc.WIDE)
    same_bits(a, e.body_encounters(extents=np.tile(bc.WIDE, (33, 1))))
    check_per_sample(a, e.state()[None], bc.WIDE, "33 wide bodies")
    assert (a.overlap_n > 0).any()


# ---- 2. known answers on the device -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,si,sj,ei,ej,gap,ttc", bc.KNOWN, ids=[k[0] for k in bc.KNOWN])
def test_known_answers(amd, name, si, sj, ei, ej, gap, ttc):
    e = amd.Engine(amd.pod("twod"), 2)
    e.add_agents(np.array([si + (0.0,), sj + (0.0,)]), 5.0)
    r = e.body_encounters(extents=[ei, ej])
    if gap == 0.0:
        assert list(r.gap_min[0]) == [0.0, 0.0] and list(r.overlap_n) == [1, 1]
    elif gap is not None:
        np.testing.assert_allclose(r.gap_min[0], [gap, gap], rtol=1e-12)
    assert list(r.gap_with[0]) == [1, 0]
    if np.isinf(ttc) or ttc == 0.0:
        assert list(r.ttc_min[0]) == [ttc, ttc]
    else:
        np.testing.assert_allclose(r.ttc_min[0], [ttc, ttc], rtol=1e-12)
    assert r.ttc_min[0, 0] == r.ttc_min[0, 1] and r.gap_min[0, 0] == r.gap_min[0, 1]   # bitwise symmetric
    assert list(r.ttc_with[0]) == ([-1, -1] if np.isinf(ttc) else [1, 0])


@pytest.mark.parametrize("n", [8, 70])
def test_a_rider_that_is_not_finite_drops_out_alone(amd, n):
    e = crowd(amd, n, 20.0 if n == 8 else BOX[n], seed=7)
    ext = bc.extents(n)
    before = e.body_encounters(extents=ext)
    s = e.state()
    partner_of = np.bincount(np.r_[before.gap_with[0], before.ttc_with[0][before.ttc_with[0] >= 0]], minlength=n)
    gone = int(np.argmin(partner_of))                           # (the rider that is the partner of the fewest)
    bad = s[gone].copy()
    bad[0] = np.nan
    e.push_state([gone], bad)
    r = e.body_encounters(extents=ext)
    assert np.isnan(r.gap_min[0, gone]) and np.isnan(r.ttc_min[0, gone]) and r.gap_with[0, gone] == -1 and r.ttc_with[0, gone] == -1
    assert r.overlap_n[gone] == 0 and np.isinf(r.run_gap_min[gone]) and r.run_gap_with[gone] == -1
    S = e.state()[None]
    assert np.isnan(S[0, gone, 0])
    check_per_sample(r, S, ext, f"n = {n}, one not finite")
    check_window(r, -1)
    assert not (r.gap_with == gone).any() and not (r.ttc_with == gone).any()
    others = (before.gap_with[0] != gone) & (before.ttc_with[0] != gone)      # who did not have it as a partner keeps every bit
    others[gone] = False
    assert others.any()
    assert np.array_equal(r.gap_min[0, others], before.gap_min[0, others]) and np.array_equal(r.ttc_min[0, others], before.ttc_min[0, others])


# ---- 3. a wrapped ring --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 70])
def test_a_wrapped_ring(amd, n):
    e = crowd(amd, n, BOX[n], seed=31, record=4)
    ext = bc.extents(n)
    e.step(7)
    S, _ = e.recorded(3, 4)
    r = e.body_encounters(3, 4, extents=ext, gap_event=5.0)
    assert r.first == 3
    check_per_sample(r, S, ext, f"n = {n}, samples 3 .. 6 of a ring of 4")
    check_window(r, 3)
    assert r.run_gap_sample.min() >= 3 and r.run_gap_sample.max() <= 6
    assert r.n_events > 0 and r.events["sample"].min() >= 3 and r.events["sample"].max() <= 6
    n0 = e.body_encounter_launches()
    for first, count in ((0, 3), (2, 2), (0, 7), (4, 4)):
        with pytest.raises(amd.engine.EngineError):
            e.body_encounters(first, count, extents=ext)
    assert e.body_encounter_launches() == n0


# ---- 4. window minima -----------------------------------------------------------------------------------------------------------------------
def test_window_ties_go_to_the_earliest_sample_and_overlaps_are_counted(amd):
    """two riders side by side, 0.3 m apart at the same speed, overlap (gap = ttc = 0) in every sample: the window reports the first,
    and overlap_n is the count over the per-sample array"""
    for n in (3, 33):
        s0 = ec.scatter(n, BOX[n], seed=43)
        s0[1] = s0[0]
        s0[1, 0] += 0.3
        e = crowd(amd, n, BOX[n], seed=43, record=16, s0=s0)
        e.step(9)
        r = e.body_encounters(3, 6, extents=bc.extents(n))
        assert (r.gap_min[:, :2] == 0.0).all() and (r.ttc_min[:, :2] == 0.0).all()
        assert list(r.run_gap_min[:2]) == [0.0, 0.0] and list(r.run_gap_sample[:2]) == [3, 3]
        assert list(r.run_ttc_min[:2]) == [0.0, 0.0] and list(r.run_ttc_sample[:2]) == [3, 3]
        assert list(r.overlap_n[:2]) == [6, 6] and np.array_equal(r.overlap_n, (r.gap_min == 0.0).sum(axis=0))
        lone = r.overlap_n == 0
        assert lone.any() and (r.run_gap_min[lone] > 0).all()
        check_window(r, 3)


def test_window_over_many_samples(amd):
    n = 33
    e = crowd(amd, n, BOX[n], seed=41, record=64)
    e.step(10)
    e.step(30)
    r = e.body_encounters(5, 35, extents=bc.extents(n))
    check_window(r, 5)
    assert r.run_gap_sample.min() >= 5 and r.run_gap_sample.max() < 40 and np.isfinite(r.run_gap_min).all()
    S, _ = e.recorded(5, 35)
    check_per_sample(r, S, bc.extents(n), f"n = {n}, 35 samples")


# ---- 5. events ----------------------------------------------------------------------------------------------------------------------------
def test_events(amd):
    n, gap_event, ttc_event = 70, 1.5, 1.5
    e = crowd(amd, n, 40.0, seed=51, record=8)
    ext = bc.extents(n)
    e.step(5)
    S, _ = e.recorded(0, 5)
    p = bc.pairs(S, ext)
    r = e.body_encounters(0, 5, extents=ext, gap_event=gap_event, ttc_event=ttc_event)
    ref, edge = bc.events(S, ext, gap_event, ttc_event, first=0, p=p)
    assert len(edge) <= 0.01 * max(len(ref), 1)
    gk, rk = key(r.events), key(ref)
    assert gk == sorted(gk) and len(set(gk)) == len(gk)
    gi = [k for k, x in enumerate(gk) if x not in edge]
    ri = [k for k, x in enumerate(rk) if x not in edge]
    print(f"events: {len(ref)} in the reference, {r.n_events} on the device, {len(edge)} pairs that may fall either side")
    assert len(ref) > 20 and [gk[k] for k in gi] == [rk[k] for k in ri]
    assert r.n_events == len(r.events)
    for f in ("gap", "ttc"):
        g, w = r.events[f][gi], ref[f][ri]
        exact = np.isinf(w) | (w == 0.0)
        assert np.array_equal(g[exact], w[exact])
        np.testing.assert_allclose(g[~exact], w[~exact], rtol=1e-9, atol=1e-9)
    assert (r.events["i"] < r.events["j"]).all()
    # gap_event = 0 lists exactly the pairs with gap 0
    hits = e.body_encounters(0, 5, extents=ext, gap_event=0.0)
    ref0, edge0 = bc.events(S, ext, 0.0, None, first=0, p=p)
    assert len(ref0) > 0 and len(edge0) <= 0.01 * len(ref0) and [x for x in key(hits.events) if x not in edge0] == [x for x in key(ref0) if x not in edge0]
    assert (hits.events["gap"] == 0.0).all() and (hits.events["ttc"] == 0.0).all() and len(hits.collisions()) == hits.n_events
    assert np.array_equal(r.collisions(), hits.events)
    # a threshold that is off
    only_t = e.body_encounters(0, 5, extents=ext, gap_event=-1.0, ttc_event=ttc_event)
    ref_t, _ = bc.events(S, ext, None, ttc_event, first=0, p=p)
    only_g = e.body_encounters(0, 5, extents=ext, gap_event=gap_event, ttc_event=0.0)
    ref_g, _ = bc.events(S, ext, gap_event, None, first=0, p=p)
    assert [x for x in key(only_t.events) if x not in edge] == [x for x in key(ref_t) if x not in edge]
    assert [x for x in key(only_g.events) if x not in edge] == [x for x in key(ref_g) if x not in edge]
    assert 0 < only_t.n_events < r.n_events and 0 < only_g.n_events < r.n_events
    off = e.body_encounters(0, 5, extents=ext, gap_event=-1.0, ttc_event=-2.0)
    assert off.n_events == 0 and off.events is None
    plain = e.body_encounters(0, 5, extents=ext)
    for other in (off, r, hits):                                 # the per-sample bits do not depend on the events
        for f in FIELDS:
            assert np.array_equal(getattr(plain, f), getattr(other, f), equal_nan=True), f
    # capacity 1: the total is still the full count, and nothing is written past the one slot
    lib = e._lib
    out = amd.ffi.BodyOut()
    room = np.zeros(3, amd.engine.BODY_EVENT_DTYPE)
    room["sample"] = -7
    out.events, out.event_capacity = room.ctypes.data, 1
    extp = np.ascontiguousarray(ext).ctypes.data_as(C.c_void_p)
    assert lib.csf_body_encounters(e._h, 0, 5, extp, gap_event, ttc_event, C.byref(out)) == 0
    assert out.n_events == r.n_events and (int(room["sample"][0]), int(room["i"][0]), int(room["j"][0])) in set(gk)
    assert (room["sample"][1:] == -7).all()
    out.events, out.event_capacity = None, 0                     # counting alone
    assert lib.csf_body_encounters(e._h, 0, 5, extp, gap_event, ttc_event, C.byref(out)) == 0 and out.n_events == r.n_events
    # more events than the guessed capacity: one second call with the exact capacity
    calls = []

    class Counting:                                             # (the library, with the wrapper's calls counted)
        def __getattr__(self, name):
            if name != "csf_body_encounters":
                return getattr(lib, name)

            def call(*args):
                calls.append(int(args[-1][0].event_capacity))
                return lib.csf_body_encounters(*args)
            return call
    big = crowd(amd, 300, 30.0, seed=52)                          # 300 riders in a 30 m box: more events than the guessed capacity of 300
    big._lib = Counting()
    rb = big.body_encounters(extents=bc.extents(300), gap_event=5.0)
    big._lib = lib
    assert len(calls) == 2 and calls[0] < rb.n_events == calls[1] == len(rb.events)
    refb, edgeb = bc.events(big.state()[None], bc.extents(300), 5.0, None, first=-1)
    assert [x for x in key(rb.events) if x not in edgeb] == [x for x in key(refb) if x not in edgeb] and len(edgeb) <= 0.01 * len(refb)


# ---- 6. same bits ---------------------------------------------------------------------------------------------------------------------------
def test_a_riders_row_does_not_depend_on_the_call(amd):
    e = crowd(amd, 257, 80.0, seed=61, record=8)
    ext = bc.extents(257)
    e.step(5)
    r = e.body_encounters(0, 5, extents=ext, gap_event=1.0)
    same_bits(r, e.body_encounters(0, 5, extents=ext, gap_event=1.0))
    for k in range(5):
        one = e.body_encounters(k, 1, extents=ext)
        for f in ("gap_min", "gap_with", "ttc_min", "ttc_with"):
            assert np.array_equal(getattr(one, f)[0], getattr(r, f)[k], equal_nan=True), (f, k)


def test_sources_split_over_workgroups(amd):
    """one sample of 1 100 riders: a receiver tile's sources are split over five workgroups of one tile each, the last of 76 sources,
    and put together by the second pass - the same bits as in a call of 40 samples, which is not split"""
    e = crowd(amd, 1100, 100.0, seed=62, record=64)
    ext = bc.extents(1100)
    e.step(40)
    S, _ = e.recorded(39, 1)
    r = e.body_encounters(39, 1, extents=ext, gap_event=1.0, ttc_event=1.0)
    p = bc.pairs(S, ext)
    check_per_sample(r, S, ext, "n = 1100")
    check_window(r, 39)
    ref, edge = bc.events(S, ext, 1.0, 1.0, first=39, p=p)
    assert len(ref) > 100 and len(edge) <= 0.01 * len(ref) and [x for x in key(r.events) if x not in edge] == [x for x in key(ref) if x not in edge]
    long = e.body_encounters(0, 40, extents=ext)                 # 5 tiles x 40 samples: no split
    for f in ("gap_min", "gap_with", "ttc_min", "ttc_with"):
        assert np.array_equal(getattr(long, f)[39], getattr(r, f)[0], equal_nan=True), f
    now = e.body_encounters(extents=ext)                         # the current state is that sample
    for f in ("gap_min", "gap_with", "ttc_min", "ttc_with"):
        assert np.array_equal(getattr(now, f)[0], getattr(r, f)[0], equal_nan=True), f
    # a rider's partner has the rider at the same value or a smaller one: bitwise symmetric pairs, whatever chunk each sits in
    for v, w in ((r.gap_min[0], r.gap_with[0]), (r.ttc_min[0], r.ttc_with[0])):
        has = w >= 0
        assert has.any() and (v[w[has]] <= v[has]).all()


# ---- 7. batch -------------------------------------------------------------------------------------------------------------------------------
def test_batch_equals_every_member_alone_in_two_launches(amd):
    members = [crowd(amd, 3, 6.0, seed=700 + k, record=32) for k in range(64)] + [crowd(amd, 33, 20.0, seed=777, record=32)]
    silent = crowd(amd, 3, 6.0, seed=799)                        # does not record
    engines = members + [silent]
    exts = [bc.BIKE if k % 2 else bc.extents(e.n, every=2) for k, e in enumerate(engines)]
    amd.Engine.batch_join(engines)
    amd.Engine.step_batch(engines, 20)
    n0 = [e.body_encounter_launches() for e in engines]
    plain = amd.Engine.batch_body_encounters(engines, 20, extents=exts)
    assert engines[0].body_encounter_launches() == n0[0] + 2     # the documented constant: the pair launch and the window pass
    assert [e.body_encounter_launches() for e in engines[1:]] == n0[1:]
    res = amd.Engine.batch_body_encounters(engines, 20, extents=exts, gap_event=1.0, ttc_event=1.5)
    for u, w in zip(plain[:-1], res[:-1]):                        # (the per-sample bits do not depend on the events)
        for f in FIELDS:
            assert np.array_equal(getattr(u, f), getattr(w, f), equal_nan=True), f
    assert res[-1] is None and all(r is not None for r in res[:-1])
    found = 0
    for e, x, r in zip(members, exts, res):
        alone = e.body_encounters(0, 20, extents=x, gap_event=1.0, ttc_event=1.5)
        assert r.first == 0 and r.gap_min.shape == (20, e.n)
        same_bits(r, alone)
        found += r.n_events
    assert found > 0
    S, _ = members[-1].recorded(0, 20)
    check_per_sample(res[64], S, exts[64], "the 33-rider member of the batch")
    S, _ = members[5].recorded(0, 20)
    check_per_sample(res[5], S, exts[5], "a 3-rider member of the batch")
    # fewer samples than asked for: refused before anything is written
    n1 = engines[0].body_encounter_launches()
    with pytest.raises(amd.engine.EngineError):
        amd.Engine.batch_body_encounters(engines, 21, extents=exts)
    assert engines[0].body_encounter_launches() == n1
    amd.Engine.batch_leave(engines)


def test_intersections_together(amd):
    from cyclistsocialforce_amd import intersection as ci
    from cyclistsocialforce_amd.vehicle import TwoDBicycle, vehicle_extents
    scenes = []
    for k in range(3):
        s0 = ec.scatter(3, 8.0, seed=900 + k)
        vs = []
        for j, s in enumerate(s0):
            v = TwoDBicycle(tuple(s), id=f"s{k}r{j}")
            v.setDestinations(s[0] + np.array([30.0, 60.0]) * np.cos(s[2]), s[1] + np.array([30.0, 60.0]) * np.sin(s[2]))
            vs.append(v)
        scenes.append(ci.SocialForceIntersection(vs))
    ci.advance_together(scenes, 12)
    res = ci.body_encounters_together(scenes, 12, gap_event=2.0)
    for k, (ins, r) in enumerate(zip(scenes, res)):
        own = np.array([vehicle_extents(v) for v in ins.vehicles])
        assert np.array_equal(r.extents, own)
        alone = ins.body_encounters(r.first, 12, gap_event=2.0)
        same_bits(r, alone)
        same_bits(r, ins.body_encounters(r.first, 12, extents=own, gap_event=2.0))
        assert r.ids == [f"s{k}r{j}" for j in range(3)]
        assert list(r.run_gap_with_id) == [r.ids[j] for j in r.run_gap_with]
        assert r.gap_with_id.shape == (12, 3) and r.gap_with_id[0, 0] == r.ids[r.gap_with[0, 0]]
        assert all((a is None) == (j < 0) for a, j in zip(r.run_ttc_with_id, r.run_ttc_with))
        S, _ = ins.engine.recorded(r.first, 12)
        check_per_sample(r, S, own, f"intersection {k}")
        now = ins.body_encounters()
        assert np.array_equal(now.gap_min[0], r.gap_min[-1])
    wide = ci.body_encounters_together(scenes, 12, extents=bc.WIDE)
    assert all(np.array_equal(w.extents, np.tile(bc.WIDE, (3, 1))) for w in wide) and all((w.gap_min <= r.gap_min).all() for w, r in zip(wide, res))


# ---- 8. the engine is untouched -------------------------------------------------------------------------------------------------------------
@pytest.mark.auto_variant
@pytest.mark.parametrize("n", [3, 70, 3000])
def test_body_encounters_between_steps_leave_the_run_alone(amd, n):
    """the engine's own tick for the size - one wave, one launch, pair + per-agent launches -: step(5), body_encounters, step(5) ends
    bit for bit where step(10) of a twin ends"""
    box = max(BOX.get(n, 0.0), 3.0 * np.sqrt(n))
    ring = 16 if n < 3000 else None
    a, b = (crowd(amd, n, box, seed=90 + n, record=ring) for _ in range(2))
    ext = bc.extents(n)
    a.step(5)
    r = a.body_encounters(extents=ext, gap_event=1.0)
    if n < 3000:
        check_per_sample(r, a.state()[None], ext, f"n = {n}, the current state")
    else:                                                        # (the full reference holds dozens of n x n arrays: the invariants alone)
        assert r.n_events > 0 and (r.events["i"] < r.events["j"]).all() and (r.events["gap"] <= 1.0).all()
        has = r.gap_with[0] >= 0
        assert has.all() and (r.gap_min[0][r.gap_with[0]] <= r.gap_min[0]).all()
    if ring:
        w = a.body_encounters(0, 5, extents=ext)
        assert np.array_equal(w.gap_min[4], r.gap_min[0])
    a.step(5)
    b.step(10)
    assert np.array_equal(a.state(), b.state())
    fa, fb = a.forces(), b.forces()
    assert np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1])
    assert a.small_ticks() == b.small_ticks() and a.mid_ticks() == b.mid_ticks()
    if ring:
        Sa, _ = a.recorded(0, 10)
        Sb, _ = b.recorded(0, 10)
        assert np.array_equal(Sa, Sb)


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_have_a_message_and_no_side_effect(amd):
    from calib_common import data_set, pod_sets
    a, twin = (crowd(amd, 40, 30.0, seed=10, record=4) for _ in range(2))
    plain = crowd(amd, 40, 30.0, seed=10)                        # no ring
    a.step(6); twin.step(6); plain.step(6)
    lib = a._lib
    n = 40
    arrays = dict(d=np.full((4, n), -7.0), dj=np.full((4, n), -7, np.int32), ev=np.zeros(8, amd.engine.BODY_EVENT_DTYPE))
    good = np.ascontiguousarray(bc.extents(n))

    def ext(u=None, **kw):
        x = good.copy()
        for k, v in kw.items():
            x[u, ("front", "rear", "half_width").index(k)] = v
        return x

    def out(**kw):
        o = amd.ffi.BodyOut()
        o.gap_min, o.gap_with = arrays["d"].ctypes.data, arrays["dj"].ctypes.data
        o.n_events = -7
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    ev = arrays["ev"].ctypes.data
    nan, inf = float("nan"), float("inf")
    cases = {
        "out NULL": (a, 2, 4, good, 0.0, 0.0, None), "ext NULL": (a, 2, 4, None, 0.0, 0.0, out()),
        "front < 0": (a, 2, 4, ext(5, front=-0.1), 0.0, 0.0, out()), "rear < 0": (a, 2, 4, ext(5, rear=-0.1), 0.0, 0.0, out()),
        "no length": (a, 2, 4, ext(5, front=0.0, rear=0.0), 0.0, 0.0, out()), "no width": (a, 2, 4, ext(5, half_width=0.0), 0.0, 0.0, out()),
        "an extent NaN": (a, 2, 4, ext(5, rear=nan), 0.0, 0.0, out()), "an extent inf": (a, 2, 4, ext(5, front=inf), 0.0, 0.0, out()),
        "gap_event NaN": (a, 2, 4, good, nan, 0.0, out()), "gap_event inf": (a, 2, 4, good, inf, 0.0, out()),
        "ttc_event NaN": (a, 2, 4, good, 0.0, nan, out()), "ttc_event inf": (a, 2, 4, good, 0.0, inf, out()),
        "n_samples < 0": (a, 2, -1, good, 0.0, 0.0, out()),
        "samples gone from the ring": (a, 1, 4, good, 0.0, 0.0, out()), "samples not yet there": (a, 4, 3, good, 0.0, 0.0, out()),
        "first below -1": (a, -2, 1, good, 0.0, 0.0, out()), "two samples of the current state": (a, -1, 2, good, 0.0, 0.0, out()),
        "no ring, a window": (plain, 2, 4, good, 0.0, 0.0, out()), "no ring, an empty window": (plain, 0, 0, good, 0.0, 0.0, out()),
        "capacity < 0": (a, 2, 4, good, 2.0, 0.0, out(events=ev, event_capacity=-1)),
        "capacity without a buffer": (a, 2, 4, good, 2.0, 0.0, out(event_capacity=8)),
    }
    n0 = {id(e): e.body_encounter_launches() for e in (a, plain)}
    for name, (e, first, count, x, ge, te, o) in cases.items():
        xp = None if x is None else x.ctypes.data_as(C.c_void_p)
        rc = lib.csf_body_encounters(e._h, first, count, xp, ge, te, None if o is None else C.byref(o))
        assert rc in (-1, -4), (name, rc)
        msg = lib.csf_last_error(e._h).decode()
        assert msg, name
        if name in ("front < 0", "rear < 0", "no length", "no width", "an extent NaN", "an extent inf"):
            assert "road user 5" in msg, (name, msg)
        assert o is None or o.n_events == -7, name
        assert e.body_encounter_launches() == n0[id(e)], name
    assert (arrays["d"] == -7.0).all() and (arrays["dj"] == -7).all()
    gp = good.ctypes.data_as(C.c_void_p)
    # an empty window and an empty population succeed and find nothing
    o = out()
    assert lib.csf_body_encounters(a._h, 3, 0, gp, 2.0, 1.0, C.byref(o)) == 0 and o.n_events == 0 and (arrays["d"] == -7.0).all()
    empty = amd.Engine(amd.pod("twod"), 4)
    o = out()
    assert lib.csf_body_encounters(empty._h, -1, 1, gp, 2.0, 1.0, C.byref(o)) == 0 and o.n_events == 0
    r = empty.body_encounters(extents=bc.BIKE, gap_event=2.0)
    assert r.gap_min.shape == (1, 0) and r.n_events == 0 and len(r.events) == 0
    assert a.body_encounter_launches() == n0[id(a)] and empty.body_encounter_launches() == 0
    # the refused engine is where its twin is
    assert np.array_equal(a.state(), twin.state())
    a.step(5); twin.step(5)
    assert np.array_equal(a.state(), twin.state())
    Sa, _ = a.recorded(7, 4)
    St, _ = twin.recorded(7, 4)
    assert np.array_equal(Sa, St)
    # a member of a loopback group
    g = [crowd(amd, 40, 30.0, seed=10) for _ in range(2)]
    amd.Engine.loopback_group(g)
    o = out()
    rc = lib.csf_body_encounters(g[0]._h, -1, 1, gp, 0.0, 0.0, C.byref(o))
    assert rc == -4 and lib.csf_last_error(g[0]._h).decode() and g[0].body_encounter_launches() == 0 and o.n_events == -7
    # an engine that holds a calibration data set
    sets = pod_sets("twod", 2)
    cs0, cFx, cFy = data_set("twod", n_seq=2, ticks=20)
    c = amd.Engine(sets[0], 4)
    c.calib_load(cs0, cFx, cFy, np.zeros((20, 2, 2)), [0, 1], max_sets=2)
    rc = lib.csf_body_encounters(c._h, -1, 1, gp, 0.0, 0.0, C.byref(o))
    assert rc == -4 and lib.csf_last_error(c._h).decode() and c.body_encounter_launches() == 0
    # the batched call: not a batch, NULL outs, NULL exts, a bad extent, a bad threshold
    outs = (amd.ffi.BodyOut * 2)()
    arr = (C.c_void_p * 2)(a._h, twin._h)
    xs = (C.c_void_p * 2)(good.ctypes.data, good.ctypes.data)
    bad = ext(7, half_width=-1.0)
    xb = (C.c_void_p * 2)(good.ctypes.data, bad.ctypes.data)
    assert lib.csf_batch_body_encounters(arr, 2, 2, xs, 0.0, 0.0, outs) == -4
    amd.Engine.batch_join([a, twin])
    assert lib.csf_batch_body_encounters(arr, 2, 2, xs, 0.0, 0.0, None) == -1
    assert lib.csf_batch_body_encounters(arr, 2, 2, None, 0.0, 0.0, outs) == -1
    assert lib.csf_batch_body_encounters(arr, 2, 2, xb, 0.0, 0.0, outs) == -1 and "road user 7" in lib.csf_last_error(twin._h).decode()
    assert lib.csf_batch_body_encounters(arr, 2, 2, xs, nan, 0.0, outs) == -1
    assert lib.csf_batch_body_encounters(arr, 2, -1, xs, 0.0, 0.0, outs) == -1
    assert lib.csf_batch_body_encounters(arr, 2, 5, xs, 0.0, 0.0, outs) == -1      # more than the ring of 4 holds
    assert a.body_encounter_launches() == n0[id(a)]
    assert lib.csf_batch_body_encounters(arr, 2, 2, xs, -1.0, 0.0, outs) == 0 and a.body_encounter_launches() == n0[id(a)] + 2
    assert outs[0].first_sample == 9 and outs[1].first_sample == 9
    amd.Engine.batch_leave([a, twin])
