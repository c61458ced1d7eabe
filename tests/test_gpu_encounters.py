"""Encounter measures on the MI355X (include/csf.h: csf_encounters, csf_batch_encounters; csf_encounter.hip) against
the definition in NumPy fp64 (tests/encounter_common.py), applied to the states read back with Engine.recorded / Engine.state: engine
and reference start from identical bits.

Tolerance: d_min and ttc_min to rtol 1e-9, +inf and 0 exactly, partners equal.  The bound follows from the cancellation-free root:
where b^2 - a q >= 1e-9 b^2 the root's relative error is below 2e-11 (the device's sincos and the contraction-free products differ
from NumPy's in the last bit of u, which the root amplifies by at most 1 / sqrt(1e-9) / 2).  A (sample, rider) cell is left out where a
pair of it is within 1e-9 b^2 of the discriminant's zero while approaching, or within 1e-6 R^2 of touching, or its two smallest
values are within 1e-9 relative without being equal (encounter_common.fragile); at most 1 % of the cells may be left out."""
import ctypes as C

import numpy as np
import pytest

import encounter_common as ec
from conftest import mixed_classes

pytestmark = pytest.mark.gpu

RADIUS = 0.5
BOX = {1: 6.0, 2: 6.0, 3: 6.0, 33: 20.0, 70: 40.0, 257: 80.0, 300: 80.0}


@pytest.fixture(scope="module")
def amd():
    from cyclistsocialforce_amd import _ffi, engine, parameters

    class NS:
        pass

    ns = NS()
    ns.Engine, ns.pod, ns.ffi, ns.engine = engine.Engine, parameters.default_pod, _ffi, engine
    return ns


def crowd(amd, n, box, seed, model="twod", record=None, **over):
    """n road users scattered in a box, riding towards destinations ahead of them; record: the capacity of a ring of every tick"""
    pod = amd.pod(model, **over)
    s0 = ec.scatter(n, box, seed, ns=amd.ffi.N_STATES[pod.model])
    e = amd.Engine(pod, max(n, 1))
    e.add_agents(s0, 5.0)
    e.set_dest_queue(np.arange(n), *ec.with_queue(s0), reset=True)
    if record:
        e.record(stride=1, capacity=record, forces=False)
    return e


def check_per_sample(r, S, radius, what=""):
    """the per-sample arrays of an Encounters against the reference on the same states; returns the share of cells left out"""
    p = ec.pairs(S, radius)
    d, dj, t, tj = ec.per_sample(S, radius, p)
    out = ec.fragile(S, radius, p)
    keep = ~out
    share = float(out.mean()) if out.size else 0.0
    print(f"{what}: {out.size} cells, {int(out.sum())} left out, {int(np.isfinite(t).sum())} with a finite ttc, {int((t == 0).sum())} overlapping")
    assert share <= 0.01
    assert r.d_min.shape == d.shape and r.d_with.dtype == np.int32 and r.ttc_with.dtype == np.int32
    for got, ref in ((r.d_min, d), (r.ttc_min, t)):
        g, w = got[keep], ref[keep]
        assert np.array_equal(np.isnan(g), np.isnan(w))
        exact = np.isinf(w) | (w == 0.0) | np.isnan(w)
        assert np.array_equal(g[exact], w[exact], equal_nan=True)                 # +inf and 0 hold exactly
        np.testing.assert_allclose(g[~exact], w[~exact], rtol=1e-9, atol=0)
    assert np.array_equal(r.d_with[keep], dj[keep]) and np.array_equal(r.ttc_with[keep], tj[keep])
    return share


def check_window(r, first):
    """run_* are the reductions of the same call's per-sample arrays: bit for bit"""
    ref = ec.window(r.d_min, r.d_with, r.ttc_min, r.ttc_with, first)
    got = (r.run_d_min, r.run_d_with, r.run_d_sample, r.run_ttc_min, r.run_ttc_with, r.run_ttc_sample)
    for g, w in zip(got, ref):
        assert g.dtype == w.dtype and np.array_equal(g, w)


def same_bits(a, b):
    for f in ("d_min", "d_with", "ttc_min", "ttc_with", "run_d_min", "run_d_with", "run_d_sample", "run_ttc_min", "run_ttc_with", "run_ttc_sample"):
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f
    assert a.n_events == b.n_events and (a.events is None) == (b.events is None)
    if a.events is not None:
        assert np.array_equal(a.events, b.events)


# ---- 1. per sample against NumPy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 33, 70, 257, 300])
def test_per_sample_against_numpy(amd, n):
    """a population of one, the packed path (n <= 32) and its limit + 1, a wave tail, the 256-tile boundary in both directions"""
    e = crowd(amd, n, BOX[n], seed=100 + n, record=8)
    e.step(5)
    S, _ = e.recorded(0, 5)
    r = e.encounters(0, 5, radius=RADIUS)
    assert r.first == 0 and r.events is None and r.n_events == 0
    check_per_sample(r, S, RADIUS, f"n = {n}")
    check_window(r, 0)
    if n == 1:
        assert np.isinf(r.d_min).all() and np.isinf(r.ttc_min).all() and (r.d_with == -1).all() and (r.ttc_with == -1).all()
        assert np.isinf(r.run_d_min).all() and (r.run_d_with == -1).all() and (r.run_d_sample == -1).all()
    # the current state is the last sample
    now = e.encounters(radius=RADIUS)
    assert now.first == -1 and now.d_min.shape == (1, n)
    assert np.array_equal(now.d_min[0], r.d_min[4]) and np.array_equal(now.ttc_min[0], r.ttc_min[4], equal_nan=True)
    assert np.array_equal(now.d_with[0], r.d_with[4]) and np.array_equal(now.ttc_with[0], r.ttc_with[4])
    assert ((now.run_d_sample == -1) & (now.run_ttc_sample == -1)).all()
    # without per_sample the window alone, the same bits
    w = e.encounters(0, 5, radius=RADIUS, per_sample=False)
    assert w.d_min is None and np.array_equal(w.run_d_min, r.run_d_min) and np.array_equal(w.run_ttc_sample, r.run_ttc_sample)


# ---- 2. known answers on the device ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,si,sj,radius,d,ttc", ec.KNOWN, ids=[k[0] for k in ec.KNOWN])
def test_known_answers(amd, name, si, sj, radius, d, ttc):
    e = amd.Engine(amd.pod("twod"), 2)
    e.add_agents(np.array([si + (0.0,), sj + (0.0,)]), 5.0)
    r = e.encounters(radius=radius)
    np.testing.assert_allclose(r.d_min[0], [d, d], rtol=1e-12)
    assert list(r.d_with[0]) == [1, 0]
    if np.isinf(ttc) or ttc == 0.0:
        assert list(r.ttc_min[0]) == [ttc, ttc]
    else:
        np.testing.assert_allclose(r.ttc_min[0], [ttc, ttc], rtol=1e-12)
    assert r.ttc_min[0, 0] == r.ttc_min[0, 1] and r.d_min[0, 0] == r.d_min[0, 1]   # bitwise symmetric
    assert list(r.ttc_with[0]) == ([-1, -1] if np.isinf(ttc) else [1, 0])


@pytest.mark.parametrize("n", [8, 70])
def test_a_rider_that_is_not_finite_drops_out_alone(amd, n):
    e = crowd(amd, n, 20.0 if n == 8 else BOX[n], seed=7)
    before = e.encounters(radius=RADIUS)
    s = e.state()
    partner_of = np.bincount(np.r_[before.d_with[0], before.ttc_with[0][before.ttc_with[0] >= 0]], minlength=n)
    gone = int(np.argmin(partner_of))                           # (the rider that is the partner of the fewest)
    bad = s[gone].copy()
    bad[0] = np.nan
    e.push_state([gone], bad)
    r = e.encounters(radius=RADIUS)
    assert np.isnan(r.d_min[0, gone]) and np.isnan(r.ttc_min[0, gone]) and r.d_with[0, gone] == -1 and r.ttc_with[0, gone] == -1
    S = e.state()[None]
    assert np.isnan(S[0, gone, 0])
    check_per_sample(r, S, RADIUS, f"n = {n}, one not finite")
    assert not (r.d_with == gone).any() and not (r.ttc_with == gone).any()
    others = (before.d_with[0] != gone) & (before.ttc_with[0] != gone)        # who did not have it as a partner keeps every bit
    others[gone] = False
    assert others.any()
    assert np.array_equal(r.d_min[0, others], before.d_min[0, others]) and np.array_equal(r.ttc_min[0, others], before.ttc_min[0, others])


# ---- 3. a wrapped ring ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 70])
def test_a_wrapped_ring(amd, n):
    e = crowd(amd, n, BOX[n], seed=31, record=4)
    e.step(7)
    S, _ = e.recorded(3, 4)
    r = e.encounters(3, 4, radius=RADIUS, d_event=6.0)
    assert r.first == 3
    check_per_sample(r, S, RADIUS, f"n = {n}, samples 3 .. 6 of a ring of 4")
    check_window(r, 3)
    assert r.run_d_sample.min() >= 3 and r.run_d_sample.max() <= 6
    assert r.n_events > 0 and r.events["sample"].min() >= 3 and r.events["sample"].max() <= 6
    n0 = e.encounter_launches()
    for first, count in ((0, 3), (2, 2), (0, 7), (4, 4)):
        with pytest.raises(amd.engine.EngineError):
            e.encounters(first, count, radius=RADIUS)
    assert e.encounter_launches() == n0


# ---- 4. window minima --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 33])
def test_window_minima(amd, n):
    e = crowd(amd, n, BOX[n], seed=41, record=64)
    e.step(10)
    e.step(30)
    r = e.encounters(5, 35, radius=RADIUS)
    check_window(r, 5)
    assert r.run_d_sample.min() >= 5 and r.run_d_sample.max() < 40 and np.isfinite(r.run_d_min).all()
    S, _ = e.recorded(5, 35)
    check_per_sample(r, S, RADIUS, f"n = {n}, 35 samples")


def test_window_ties_go_to_the_earliest_sample(amd):
    """two riders side by side, 0.3 m apart at the same speed, overlap (ttc = 0) in every sample: the window reports the first"""
    for n in (3, 33):
        s0 = ec.scatter(n, BOX[n], seed=43)
        s0[1] = s0[0]
        s0[1, 0] += 0.3
        e = amd.Engine(amd.pod("twod"), n)
        e.add_agents(s0, 5.0)
        e.set_dest_queue(np.arange(n), *ec.with_queue(s0), reset=True)
        e.record(stride=1, capacity=16, forces=False)
        e.step(9)
        r = e.encounters(3, 6, radius=RADIUS)
        assert (r.ttc_min[:, :2] == 0.0).all() and (r.ttc_with[:, 0] == 1).all() and (r.ttc_with[:, 1] == 0).all()
        assert list(r.run_ttc_min[:2]) == [0.0, 0.0] and list(r.run_ttc_sample[:2]) == [3, 3] and list(r.run_ttc_with[:2]) == [1, 0]
        check_window(r, 3)


# ---- 5. events ---------------------------------------------------------------------------------------------------------------------------
def test_events(amd):
    n, d_event, ttc_event = 70, 2.0, 1.5
    e = crowd(amd, n, 40.0, seed=51, record=8)
    e.step(5)
    S, _ = e.recorded(0, 5)
    r = e.encounters(0, 5, radius=RADIUS, d_event=d_event, ttc_event=ttc_event)
    ref, edge = ec.events(S, RADIUS, d_event, ttc_event, first=0)
    assert len(edge) <= 0.01 * max(len(ref), 1)
    key = lambda ev: [(int(a), int(b), int(c)) for a, b, c in zip(ev["sample"], ev["i"], ev["j"])]   # noqa: E731
    gk, rk = key(r.events), key(ref)
    assert gk == sorted(gk) and len(set(gk)) == len(gk)
    gi = [k for k, x in enumerate(gk) if x not in edge]
    ri = [k for k, x in enumerate(rk) if x not in edge]
    print(f"events: {len(ref)} in the reference, {r.n_events} on the device, {len(edge)} within 1e-9 of a threshold")
    assert len(ref) > 20 and [gk[k] for k in gi] == [rk[k] for k in ri]
    assert r.n_events == len(r.events)
    for f in ("d", "ttc"):
        g, w = r.events[f][gi], ref[f][ri]
        exact = np.isinf(w) | (w == 0.0)
        assert np.array_equal(g[exact], w[exact])
        np.testing.assert_allclose(g[~exact], w[~exact], rtol=1e-9, atol=0)
    assert (r.events["i"] < r.events["j"]).all()
    # capacity 1: the total is still the full count, and the wrapper's second call returns all of them
    lib = e._lib
    out = amd.ffi.EncounterOut()
    one = np.zeros(1, amd.engine.EVENT_DTYPE)
    out.events, out.event_capacity = one.ctypes.data, 1
    assert lib.csf_encounters(e._h, 0, 5, RADIUS, d_event, ttc_event, C.byref(out)) == 0
    assert out.n_events == r.n_events and (int(one["sample"][0]), int(one["i"][0]), int(one["j"][0])) in set(gk)
    out.events, out.event_capacity = None, 0                     # counting alone
    assert lib.csf_encounters(e._h, 0, 5, RADIUS, d_event, ttc_event, C.byref(out)) == 0 and out.n_events == r.n_events
    calls = []

    class Counting:                                             # (the library, with the wrapper's calls counted)
        def __getattr__(self, name):
            if name != "csf_encounters":
                return getattr(lib, name)

            def call(*args):
                calls.append(int(args[-1][0].event_capacity))
                return lib.csf_encounters(*args)
            return call
    big = crowd(amd, 300, 30.0, seed=52)                          # 300 riders in a 30 m box: more events than the guessed capacity of 300
    big._lib = Counting()
    rb = big.encounters(radius=RADIUS, d_event=6.0)
    big._lib = lib
    assert len(calls) == 2 and calls[0] < rb.n_events == calls[1] == len(rb.events)
    refb, edgeb = ec.events(big.state()[None], RADIUS, 6.0, None, first=-1)
    assert not edgeb and key(rb.events) == key(refb)
    # a threshold <= 0 switches its kind off
    only_d = e.encounters(0, 5, radius=RADIUS, d_event=d_event, ttc_event=0.0)
    ref_d, _ = ec.events(S, RADIUS, d_event, None, first=0)
    only_t = e.encounters(0, 5, radius=RADIUS, d_event=-1.0, ttc_event=ttc_event)
    ref_t, _ = ec.events(S, RADIUS, None, ttc_event, first=0)
    assert [x for x in key(only_d.events) if x not in edge] == [x for x in key(ref_d) if x not in edge]
    assert [x for x in key(only_t.events) if x not in edge] == [x for x in key(ref_t) if x not in edge]
    assert 0 < only_d.n_events < r.n_events and 0 < only_t.n_events < r.n_events
    off = e.encounters(0, 5, radius=RADIUS, d_event=0.0, ttc_event=-2.0)
    assert off.n_events == 0 and off.events is None
    same_bits(e.encounters(0, 5, radius=RADIUS), off)            # the per-sample bits do not depend on the events


# ---- 6. same bits ------------------------------------------------------------------------------------------------------------------------
def test_a_riders_row_does_not_depend_on_the_call(amd):
    e = crowd(amd, 257, 80.0, seed=61, record=8)
    e.step(5)
    r = e.encounters(0, 5, radius=RADIUS, d_event=2.0)
    same_bits(r, e.encounters(0, 5, radius=RADIUS, d_event=2.0))
    for k in range(5):
        one = e.encounters(k, 1, radius=RADIUS)
        for f in ("d_min", "d_with", "ttc_min", "ttc_with"):
            assert np.array_equal(getattr(one, f)[0], getattr(r, f)[k], equal_nan=True), (f, k)


def test_sources_split_over_workgroups(amd):
    """few samples of many riders: a receiver tile's sources are split over several workgroups (1 100 riders: five chunks of one tile, the
    last of 76 sources; 4 300: nine chunks of two tiles, the last of one tile of 204) and put together by the second pass"""
    e = crowd(amd, 1100, 100.0, seed=62, record=4)
    e.step(2)
    S, _ = e.recorded(0, 2)
    r = e.encounters(0, 2, radius=RADIUS, d_event=2.0, ttc_event=1.0)
    check_per_sample(r, S, RADIUS, "n = 1100")
    check_window(r, 0)
    ref, edge = ec.events(S, RADIUS, 2.0, 1.0, first=0)
    key = lambda ev: [(int(a), int(b), int(c)) for a, b, c in zip(ev["sample"], ev["i"], ev["j"])]   # noqa: E731
    assert len(ref) > 100 and [x for x in key(r.events) if x not in edge] == [x for x in key(ref) if x not in edge]
    for k in range(2):                                           # one sample alone: the same bits
        one = e.encounters(k, 1, radius=RADIUS)
        assert np.array_equal(one.d_min[0], r.d_min[k]) and np.array_equal(one.ttc_min[0], r.ttc_min[k]) and np.array_equal(one.ttc_with[0], r.ttc_with[k])
    big = crowd(amd, 4300, 200.0, seed=63)
    rb = big.encounters(radius=RADIUS)
    st = big.state()
    D = np.sqrt((st[None, :, 0] - st[:, None, 0]) ** 2 + (st[None, :, 1] - st[:, None, 1]) ** 2)
    np.fill_diagonal(D, np.inf)
    np.testing.assert_allclose(rb.d_min[0], D.min(axis=1), rtol=1e-9, atol=0)
    assert np.array_equal(rb.d_with[0], D.argmin(axis=1))
    meets = np.isfinite(rb.ttc_min[0])
    assert meets.any() and (rb.ttc_with[0][meets] >= 0).all() and (rb.ttc_with[0][~meets] == -1).all()
    # a rider's ttc partner has the rider at the same ttc or a smaller one: bitwise symmetric pairs, whatever chunk each sits in
    j = rb.ttc_with[0][meets]
    assert (rb.ttc_min[0][j] <= rb.ttc_min[0][meets]).all()


# ---- 7. batch ----------------------------------------------------------------------------------------------------------------------------
def test_batch_equals_every_member_alone_in_two_launches(amd):
    members = [crowd(amd, 3, 6.0, seed=700 + k, record=32) for k in range(64)] + [crowd(amd, 33, 20.0, seed=777, record=32)]
    silent = crowd(amd, 3, 6.0, seed=799)                        # does not record
    engines = members + [silent]
    amd.Engine.batch_join(engines)
    amd.Engine.step_batch(engines, 20)
    n0 = [e.encounter_launches() for e in engines]
    plain = amd.Engine.batch_encounters(engines, 20, radius=RADIUS)
    assert engines[0].encounter_launches() == n0[0] + 2          # the documented constant: the pair launch and the window pass
    assert [e.encounter_launches() for e in engines[1:]] == n0[1:]
    res = amd.Engine.batch_encounters(engines, 20, radius=RADIUS, d_event=2.0, ttc_event=1.5)
    for u, w in zip(plain[:-1], res[:-1]):                        # (the per-sample bits do not depend on the events)
        assert np.array_equal(u.d_min, w.d_min) and np.array_equal(u.ttc_min, w.ttc_min, equal_nan=True) and np.array_equal(u.run_ttc_sample, w.run_ttc_sample)
    assert res[-1] is None and all(r is not None for r in res[:-1])
    found = 0
    for e, r in zip(members, res):
        alone = e.encounters(0, 20, radius=RADIUS, d_event=2.0, ttc_event=1.5)
        assert r.first == 0 and r.d_min.shape == (20, e.n)
        same_bits(r, alone)
        found += r.n_events
    assert found > 0
    S, _ = members[-1].recorded(0, 20)
    check_per_sample(res[64], S, RADIUS, "the 33-rider member of the batch")
    S, _ = members[5].recorded(0, 20)
    check_per_sample(res[5], S, RADIUS, "a 3-rider member of the batch")
    # fewer samples than asked for: refused before anything is written
    n1 = engines[0].encounter_launches()
    with pytest.raises(amd.engine.EngineError):
        amd.Engine.batch_encounters(engines, 21, radius=RADIUS)
    assert engines[0].encounter_launches() == n1
    amd.Engine.batch_leave(engines)


def test_intersections_together(amd):
    from cyclistsocialforce_amd import intersection as ci
    from cyclistsocialforce_amd.vehicle import TwoDBicycle
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
    res = ci.encounters_together(scenes, 12, radius=RADIUS, d_event=3.0)
    for k, (ins, r) in enumerate(zip(scenes, res)):
        alone = ins.encounters(r.first, 12, radius=RADIUS, d_event=3.0)
        same_bits(r, alone)
        assert r.ids == [f"s{k}r{j}" for j in range(3)]
        assert list(r.run_d_with_id) == [r.ids[j] for j in r.run_d_with]
        assert r.d_with_id.shape == (12, 3) and r.d_with_id[0, 0] == r.ids[r.d_with[0, 0]]
        assert all((a is None) == (j < 0) for a, j in zip(r.run_ttc_with_id, r.run_ttc_with))
        S, _ = ins.engine.recorded(r.first, 12)
        check_per_sample(r, S, RADIUS, f"intersection {k}")
        now = ins.encounters(radius=RADIUS)
        assert np.array_equal(now.d_min[0], r.d_min[-1])


# ---- 8. mixed classes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", ["small_classes", "mid_classes"])
def test_mixed_classes_read_rows_0_to_3(amd, golden, switch):
    g = golden("mixed")
    pods, cls = mixed_classes(g)
    n = g["s0"].shape[0]
    e = amd.Engine(pods[0], n)
    getattr(e, switch)(True)
    e.set_param_classes(pods)
    e.add_agents(g["s0"], g["vdes"])
    e.set_dest_queue(np.arange(n), g["off"], g["dq"], reset=True)
    e.set_agent_class(np.arange(n), cls)
    e.record(stride=1, capacity=8, forces=False)
    e.step(5)
    S, _ = e.recorded(0, 5)
    assert S.shape[2] == 6
    r = e.encounters(0, 5, radius=RADIUS)
    check_per_sample(r, S, RADIUS, f"mixed.npz, {switch}")
    check_window(r, 0)


def test_mixed_classes_mid_size_and_balancing_riders(amd):
    from mid_classes_common import build, population
    c = population("five", 65, 1)
    e = build(c, True)
    e.record(stride=1, capacity=8, forces=False)
    e.step(5)
    S, _ = e.recorded(0, 5)
    r = e.encounters(0, 5, radius=RADIUS)
    check_per_sample(r, S, RADIUS, "five classes, 65 road users, csf_mid_classes on")
    b = crowd(amd, 3, 6.0, seed=83, model="balancingrider", record=8)
    b.step(5)
    S, _ = b.recorded(0, 5)
    assert S.shape[2] == 8
    check_per_sample(b.encounters(0, 5, radius=RADIUS), S, RADIUS, "three BalancingRiderBicycles")


# ---- 9. the engine is untouched ------------------------------------------------------------------------------------------------------------
@pytest.mark.auto_variant
@pytest.mark.parametrize("n", [3, 70, 3000])
def test_encounters_between_steps_leave_the_run_alone(amd, n):
    """the engine's own tick for the size - one wave, one launch, pair + per-agent launches -: step(5), encounters, step(5) ends bit
    for bit where step(10) of a twin ends"""
    box = max(BOX.get(n, 0.0), 3.0 * np.sqrt(n))
    ring = 16 if n < 3000 else None
    a, b = (crowd(amd, n, box, seed=90 + n, record=ring) for _ in range(2))
    a.step(5)
    r = a.encounters(radius=RADIUS, d_event=2.0)
    if n < 3000:
        check_per_sample(r, a.state()[None], RADIUS, f"n = {n}, the current state")
    else:                                                        # (the full reference holds a dozen n x n arrays: distances alone)
        st = a.state()
        D = np.sqrt((st[None, :, 0] - st[:, None, 0]) ** 2 + (st[None, :, 1] - st[:, None, 1]) ** 2)
        np.fill_diagonal(D, np.inf)
        np.testing.assert_allclose(r.d_min[0], D.min(axis=1), rtol=1e-9, atol=0)
        assert np.array_equal(r.d_with[0], D.argmin(axis=1)) and r.n_events > 0 and (r.events["i"] < r.events["j"]).all()
    if ring:
        w = a.encounters(0, 5, radius=RADIUS)
        assert np.array_equal(w.d_min[4], r.d_min[0])
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


# ---- 10. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_have_a_message_and_no_side_effect(amd):
    from calib_common import data_set, pod_sets
    a, twin = (crowd(amd, 40, 30.0, seed=10, record=4) for _ in range(2))
    plain = crowd(amd, 40, 30.0, seed=10)                        # no ring
    a.step(6); twin.step(6); plain.step(6)
    lib = a._lib
    n = 40
    arrays = dict(d=np.full((4, n), -7.0), dj=np.full((4, n), -7, np.int32), ev=np.zeros(8, amd.engine.EVENT_DTYPE))

    def out(**kw):
        o = amd.ffi.EncounterOut()
        o.d_min, o.d_with = arrays["d"].ctypes.data, arrays["dj"].ctypes.data
        o.n_events = -7
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    ev = arrays["ev"].ctypes.data
    nan, inf = float("nan"), float("inf")
    cases = {
        "out NULL": (a, 2, 4, RADIUS, 0.0, 0.0, None),
        "radius < 0": (a, 2, 4, -0.5, 0.0, 0.0, out()), "radius NaN": (a, 2, 4, nan, 0.0, 0.0, out()), "radius inf": (a, 2, 4, inf, 0.0, 0.0, out()),
        "n_samples < 0": (a, 2, -1, RADIUS, 0.0, 0.0, out()),
        "samples gone from the ring": (a, 1, 4, RADIUS, 0.0, 0.0, out()), "samples not yet there": (a, 4, 3, RADIUS, 0.0, 0.0, out()),
        "first below -1": (a, -2, 1, RADIUS, 0.0, 0.0, out()), "two samples of the current state": (a, -1, 2, RADIUS, 0.0, 0.0, out()),
        "no ring, a window": (plain, 2, 4, RADIUS, 0.0, 0.0, out()), "no ring, an empty window": (plain, 0, 0, RADIUS, 0.0, 0.0, out()),
        "capacity < 0": (a, 2, 4, RADIUS, 2.0, 0.0, out(events=ev, event_capacity=-1)),
        "capacity without a buffer": (a, 2, 4, RADIUS, 2.0, 0.0, out(event_capacity=8)),
    }
    n0 = {id(e): e.encounter_launches() for e in (a, plain)}
    for name, (e, first, count, radius, de, te, o) in cases.items():
        rc = lib.csf_encounters(e._h, first, count, radius, de, te, None if o is None else C.byref(o))
        assert rc in (-1, -4), (name, rc)
        assert lib.csf_last_error(e._h).decode(), name
        assert o is None or o.n_events == -7, name
        assert e.encounter_launches() == n0[id(e)], name
    assert (arrays["d"] == -7.0).all() and (arrays["dj"] == -7).all()
    # an empty window and an empty population succeed and find nothing
    o = out()
    assert lib.csf_encounters(a._h, 3, 0, RADIUS, 2.0, 1.0, C.byref(o)) == 0 and o.n_events == 0 and (arrays["d"] == -7.0).all()
    empty = amd.Engine(amd.pod("twod"), 4)
    o = out()
    assert lib.csf_encounters(empty._h, -1, 1, RADIUS, 2.0, 1.0, C.byref(o)) == 0 and o.n_events == 0
    r = empty.encounters(radius=RADIUS, d_event=2.0)
    assert r.d_min.shape == (1, 0) and r.n_events == 0 and len(r.events) == 0
    assert a.encounter_launches() == n0[id(a)] and empty.encounter_launches() == 0
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
    rc = lib.csf_encounters(g[0]._h, -1, 1, RADIUS, 0.0, 0.0, C.byref(o))
    assert rc == -4 and lib.csf_last_error(g[0]._h).decode() and g[0].encounter_launches() == 0 and o.n_events == -7
    # an engine that holds a calibration data set
    sets = pod_sets("twod", 2)
    cs0, cFx, cFy = data_set("twod", n_seq=2, ticks=20)
    c = amd.Engine(sets[0], 4)
    c.calib_load(cs0, cFx, cFy, np.zeros((20, 2, 2)), [0, 1], max_sets=2)
    rc = lib.csf_encounters(c._h, -1, 1, RADIUS, 0.0, 0.0, C.byref(o))
    assert rc == -4 and lib.csf_last_error(c._h).decode() and c.encounter_launches() == 0
    # the batched call: not a batch, NULL outs, a bad radius
    outs = (amd.ffi.EncounterOut * 2)()
    arr = (C.c_void_p * 2)(a._h, twin._h)
    assert lib.csf_batch_encounters(arr, 2, 2, RADIUS, 0.0, 0.0, outs) == -4
    amd.Engine.batch_join([a, twin])
    assert lib.csf_batch_encounters(arr, 2, 2, RADIUS, 0.0, 0.0, None) == -1
    assert lib.csf_batch_encounters(arr, 2, 2, -1.0, 0.0, 0.0, outs) == -1
    assert lib.csf_batch_encounters(arr, 2, -1, RADIUS, 0.0, 0.0, outs) == -1
    assert lib.csf_batch_encounters(arr, 2, 5, RADIUS, 0.0, 0.0, outs) == -1      # more than the ring of 4 holds
    assert a.encounter_launches() == n0[id(a)]
    assert lib.csf_batch_encounters(arr, 2, 2, RADIUS, 0.0, 0.0, outs) == 0 and a.encounter_launches() == n0[id(a)] + 2
    assert outs[0].first_sample == 9 and outs[1].first_sample == 9
    amd.Engine.batch_leave([a, twin])
