"""Post-encroachment time on the MI355X (include/csf.h: csf_post_encroachment, csf_batch_post_encroachment; csf_pet.hip; DESIGN.md
4.13) against the definition in NumPy fp64 (tests/pet_common.py), applied to the states read back with Engine.recorded: engine and
reference start from identical bits.

The comparison is BIT FOR BIT - seg_*, run_*, run_count and the events - and no cell is left out.  That is derivable, not measured:
every input is the ring's fp64 bits, every operation is one IEEE operation in a stated order without contraction, fp64 division is
correctly rounded, and no transcendental is involved.

Every case with a population asserts that it is not vacuous: the reference alone finds at least one crossing and, from 33 riders
on, at least a quarter of the riders have a finite run_pet (seeds chosen with the CPU oracle)."""
import ctypes as C

import numpy as np
import pytest

import pet_common as pc
from conftest import mixed_classes

pytestmark = pytest.mark.gpu

INF = float("inf")
STRIDE = 20                     # x t_s = 0.01 s: a sample every 0.2 s
SAMPLES = 6
BOX = {33: 20.0, 70: 30.0, 257: 60.0, 300: 60.0, 1100: 100.0}
SEED = {33: 25, 70: 12, 257: 34, 300: 37, 1100: 6}
SEG = ("seg_pet", "seg_with", "seg_t_own", "seg_t_with")
RUN = ("run_pet", "run_with", "run_t_own", "run_t_with", "run_x", "run_y", "run_count")


@pytest.fixture(scope="module")
def amd():
    from cyclistsocialforce_amd import _ffi, engine, parameters

    class NS:
        pass

    ns = NS()
    ns.Engine, ns.pod, ns.ffi, ns.engine = engine.Engine, parameters.default_pod, _ffi, engine
    return ns


def crowd(amd, n, box=None, seed=None, model="twod", ring=8, stride=STRIDE, s0=None, **over):
    """n road users scattered in a box (two or three: on converging courses), riding towards destinations ahead of them; ring: the
    capacity of a state ring of every `stride`-th tick (None: no recording)"""
    pod = amd.pod(model, **over)
    ns = amd.ffi.N_STATES[pod.model]
    if s0 is None:
        s0 = pc.converging(n, ns=ns) if n in (2, 3) else pc.scatter(n, box or BOX.get(n, 6.0), SEED.get(n, 100 + n) if seed is None else seed, ns=ns)
    e = amd.Engine(pod, max(n, 1))
    e.add_agents(s0, 5.0)
    e.set_dest_queue(np.arange(n), *pc.with_queue(s0), reset=True)
    if ring:
        e.record(stride=stride, capacity=ring, forces=False)
    return e


def recorded_crowd(amd, n, **kw):
    e = crowd(amd, n, **kw)
    e.step(kw.get("stride", STRIDE) * SAMPLES)
    return e


def not_vacuous(ref, n, what=""):
    finite = int(np.isfinite(ref.run_pet).sum())
    print(f"{what}: {n} riders, {len(ref.crossings)} crossings as the riders report them, {finite} riders with a finite PET")
    assert len(ref.crossings) >= 1, "vacuous: the reference finds no crossing"
    if n >= 33:
        assert 4 * finite >= n, f"vacuous: {finite} of {n} riders have a finite PET"


def same_bits(got, ref, per_segment=True, what=""):
    """every array of a PostEncroachment against the reference's (or another PostEncroachment's): the same bits, NaN where NaN"""
    for f in (SEG if per_segment else ()) + RUN:
        g, w = getattr(got, f), getattr(ref, f)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f)
        assert np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), (what, f)


def same_events(ev, ref_ev):
    assert ev.dtype == ref_ev.dtype and len(ev) == len(ref_ev)
    for f in ev.dtype.names:
        assert np.array_equal(ev[f], ref_ev[f]), f


def check(e, first, count, what, n=None, vacuous=True):
    """post_encroachment(first, count, every crossing an event) against the reference on recorded(first, count); returns both"""
    S, _ = e.recorded(first, count)
    ref = pc.reference(S)
    if vacuous:
        not_vacuous(ref, e.n if n is None else n, what)
    r = e.post_encroachment(first, count, pet_event=INF)
    assert r.first == first
    same_bits(r, ref, what=what)
    same_events(r.events, pc.events(ref, INF))
    assert r.n_events == len(r.events) == int(r.run_count.sum()) // 2
    return r, ref


# ---- 1. against NumPy -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 33, 70, 257, 300])
def test_against_numpy(amd, n):
    """a population of one, two and three riders on converging courses, one tile of own segments with a tail (33 x 5 = 165), two tiles
    whose partners are split (70), the 256-tile boundary in both directions in riders (257, 300: six tiles, six chunks)"""
    e = recorded_crowd(amd, n)
    r, ref = check(e, 0, SAMPLES, f"n = {n}", vacuous=n > 1)
    assert r.seg_pet.shape == (SAMPLES - 1, n) and r.seg_with.dtype == np.int32 and r.run_count.dtype == np.int32
    assert r.period == pytest.approx(0.2)
    if n == 1:
        assert np.isinf(r.seg_pet).all() and (r.seg_with == -1).all() and np.isnan(r.seg_t_own).all() and np.isnan(r.seg_t_with).all()
        assert np.isinf(r.run_pet).all() and (r.run_with == -1).all() and (r.run_count == 0).all() and r.n_events == 0
    w = e.post_encroachment(0, SAMPLES, per_segment=False)       # the road users' rows alone: the same bits
    assert w.seg_pet is None and w.events is None and w.n_events == 0
    same_bits(w, r, per_segment=False)
    one = e.post_encroachment(2, 1, pet_event=INF)               # one sample is no path
    assert one.seg_pet.shape == (0, n) and np.isinf(one.run_pet).all() and (one.run_with == -1).all() and (one.run_count == 0).all()
    assert np.isnan(one.run_t_own).all() and np.isnan(one.run_x).all() and one.n_events == 0 and len(one.events) == 0
    s = r.in_seconds()
    assert np.array_equal(s.run_pet, r.run_pet * 0.2) and np.array_equal(s.seg_t_own, r.seg_t_own * 0.2, equal_nan=True)
    assert np.array_equal(s.events["t_i"], r.events["t_i"] * 0.2) and np.array_equal(s.run_x, r.run_x, equal_nan=True)


# ---- 2. non-finite ----------------------------------------------------------------------------------------------------------------------
def test_a_rider_that_is_not_finite(amd):
    n, gone = 70, 5
    e = crowd(amd, n)
    e.step(3 * STRIDE)
    bad = e.state()[gone].copy()
    bad[0] = np.nan
    e.push_state([gone], bad)
    e.step(3 * STRIDE)
    S, _ = e.recorded(0, SAMPLES)
    assert np.isnan(S[3:, gone, 0]).all() and np.isfinite(S[:3, gone, 0]).all()
    r, ref = check(e, 0, SAMPLES, "n = 70, one rider NaN from sample 3 on", vacuous=False)
    assert len(ref.crossings) >= 1
    assert np.isnan(r.seg_pet[2:, gone]).all() and (r.seg_with[2:, gone] == -1).all() and np.isnan(r.seg_t_own[2:, gone]).all()
    assert not np.isnan(r.seg_pet[:2, gone]).any()


# ---- 3. a wrapped ring ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 70])
def test_a_wrapped_ring(amd, n):
    """capacity 4, 7 samples taken: samples 3 .. 6 sit in slots 3, 0, 1, 2 (a sample every 0.4 s; the three riders start 7.5 m further
    back, so that they meet inside the window)"""
    s0 = None
    if n == 3:
        s0 = pc.converging(3)
        s0[:, 0] -= 7.5 * np.cos(s0[:, 2])
        s0[:, 1] -= 7.5 * np.sin(s0[:, 2])
    e = crowd(amd, n, seed=38 if n == 70 else None, ring=4, stride=40, s0=s0)
    e.step(7 * 40)
    r, ref = check(e, 3, 4, f"n = {n}, samples 3 .. 6 of a ring of 4")
    assert r.period == pytest.approx(0.4)
    n0 = e.pet_launches()
    for first, count in ((0, 3), (2, 2), (0, 7), (4, 4), (7, 1)):
        with pytest.raises(amd.engine.EngineError):
            e.post_encroachment(first, count)
    assert e.pet_launches() == n0


# ---- 4. layout independence -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [300, 1100])
def test_partners_split_over_workgroups(amd, n):
    """300 riders x 5 segments: 6 tiles of own segments, their partners in SIX chunks of one tile (the last of 220 segments); 1 100 x 5:
    22 tiles, ELEVEN chunks of two tiles (the last of 256 + 124) - put together by the window pass to the bits of one loop"""
    e = recorded_crowd(amd, n)
    r, ref = check(e, 0, SAMPLES, f"n = {n}")
    again = e.post_encroachment(0, SAMPLES, pet_event=INF)
    same_bits(again, r)
    same_events(again.events, r.events)
    # run_* are the reduction of the same call's seg_*: the earliest k on ties
    rp, rw, ro, rt, _ = pc.window(r.seg_pet, r.seg_with, r.seg_t_own, r.seg_t_with)
    assert np.array_equal(r.run_pet, rp) and np.array_equal(r.run_with, rw)
    assert np.array_equal(r.run_t_own, ro, equal_nan=True) and np.array_equal(r.run_t_with, rt, equal_nan=True)
    # a shorter window of the same recording: one chunk fewer, the same rows where the window's crossings are the same
    short = e.post_encroachment(1, 3)
    same_bits(short, pc.reference(e.recorded(1, 3)[0]))


# ---- 5. events --------------------------------------------------------------------------------------------------------------------------
def test_events(amd, monkeypatch):
    n = 70
    e = recorded_crowd(amd, n)
    r, ref = check(e, 0, SAMPLES, "events, n = 70")              # every crossing, sorted, equal to the reference's list
    ev = r.events
    key = list(zip(ev["i"].tolist(), ev["j"].tolist(), ev["k"].tolist(), ev["l"].tolist()))
    assert key == sorted(key) and len(set(key)) == len(key) and (ev["i"] < ev["j"]).all() and len(ev) >= 5
    pet = np.abs(ev["t_j"] - ev["t_i"])
    for u in range(n):                                           # bitwise symmetric: i's list holds what j reports
        mine = pet[(ev["i"] == u) | (ev["j"] == u)]
        assert (mine.min() if len(mine) else INF) == r.run_pet[u]
    thr = float(np.median(pet))
    sub = e.post_encroachment(0, SAMPLES, pet_event=thr)
    same_events(sub.events, pc.events(ref, thr))
    assert 0 < sub.n_events < r.n_events
    same_bits(sub, r)                                            # the rows do not depend on the events
    off = e.post_encroachment(0, SAMPLES, pet_event=0.0)
    assert off.events is None and off.n_events == 0
    same_bits(off, r)
    # capacity 0: the count alone
    lib = e._lib
    out = amd.ffi.PetOut()
    assert lib.csf_post_encroachment(e._h, 0, SAMPLES, INF, C.byref(out)) == 0 and out.n_events == r.n_events and out.first_sample == 0
    one = np.zeros(1, amd.engine.PET_EVENT_DTYPE)
    out.events, out.event_capacity = one.ctypes.data, 1
    assert lib.csf_post_encroachment(e._h, 0, SAMPLES, INF, C.byref(out)) == 0 and out.n_events == r.n_events
    assert (int(one["i"][0]), int(one["j"][0]), int(one["k"][0]), int(one["l"][0])) in set(key)
    # a guess that is too small: exactly one second call, with the exact capacity
    calls = []

    class Counting:                                             # (the library, with the wrapper's calls counted)
        def __getattr__(self, name):
            if name != "csf_post_encroachment":
                return getattr(lib, name)

            def call(*args):
                calls.append(int(args[-1][0].event_capacity))
                return lib.csf_post_encroachment(*args)
            return call
    monkeypatch.setattr(amd.engine, "_pet_capacity_guess", lambda segs: 3)
    e._lib = Counting()
    try:
        small = e.post_encroachment(0, SAMPLES, pet_event=INF)
    finally:
        e._lib = lib
    assert calls == [3, r.n_events] and r.n_events > 3
    same_events(small.events, r.events)


# ---- 6. batch ---------------------------------------------------------------------------------------------------------------------------
def test_batch_equals_every_member_alone_in_two_launches(amd):
    rng = np.random.default_rng(600)
    members = []
    for k in range(64):
        s0 = pc.converging(3)
        s0[:, :2] += rng.uniform(-0.3, 0.3, (3, 2))
        members.append(crowd(amd, 3, s0=s0))
    members.append(crowd(amd, 33))
    silent = crowd(amd, 3, ring=None)                            # does not record
    engines = members + [silent]
    amd.Engine.batch_join(engines)
    amd.Engine.step_batch(engines, STRIDE * SAMPLES)
    n0 = [e.pet_launches() for e in engines]
    res = amd.Engine.batch_post_encroachment(engines, SAMPLES, pet_event=INF)
    assert engines[0].pet_launches() == n0[0] + 2                # the documented constant: the pair launch and the window pass
    assert [e.pet_launches() for e in engines[1:]] == n0[1:]
    assert res[-1] is None and all(r is not None for r in res[:-1])
    crossed = 0
    for e, r in zip(members, res):
        alone = e.post_encroachment(0, SAMPLES, pet_event=INF)
        assert r.first == 0 and r.seg_pet.shape == (SAMPLES - 1, e.n) and r.period == pytest.approx(0.2)
        same_bits(r, alone)
        same_events(r.events, alone.events)
        crossed += int(np.isfinite(r.run_pet).any())
    assert crossed >= 48                                         # (the three-rider scenes are on converging courses)
    ref = pc.reference(members[-1].recorded(0, SAMPLES)[0])
    not_vacuous(ref, 33, "the 33-rider member of the batch")
    same_bits(res[64], ref)
    ref = pc.reference(members[5].recorded(0, SAMPLES)[0])
    not_vacuous(ref, 3, "a 3-rider member of the batch")
    same_bits(res[5], ref)
    same_events(res[5].events, pc.events(ref, INF))
    plain = amd.Engine.batch_post_encroachment(engines, SAMPLES, per_segment=False)
    assert plain[3].seg_pet is None and plain[3].events is None
    same_bits(plain[3], res[3], per_segment=False)
    # more samples than a member's ring holds: refused before anything is written
    n1 = engines[0].pet_launches()
    with pytest.raises(amd.engine.EngineError):
        amd.Engine.batch_post_encroachment(engines, SAMPLES + 1)
    assert engines[0].pet_launches() == n1
    amd.Engine.batch_leave(engines)


# ---- 7. mixed classes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", ["small_classes", "mid_classes"])
def test_mixed_classes_read_rows_0_and_1(amd, golden, switch):
    """15 road users of five classes with 5 or 6 states each, a sample every 0.5 s"""
    g = golden("mixed")
    pods, cls = mixed_classes(g)
    n = g["s0"].shape[0]
    e = amd.Engine(pods[0], n)
    getattr(e, switch)(True)
    e.set_param_classes(pods)
    e.add_agents(g["s0"], g["vdes"])
    e.set_dest_queue(np.arange(n), g["off"], g["dq"], reset=True)
    e.set_agent_class(np.arange(n), cls)
    e.record(stride=50, capacity=8, forces=False)
    e.step(50 * SAMPLES)
    assert e.recorded(0, SAMPLES)[0].shape[2] == 6
    check(e, 0, SAMPLES, f"mixed.npz, {switch}")


# ---- 8. the run is left alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.auto_variant
@pytest.mark.parametrize("n", [3, 70, 3000])
def test_post_encroachment_between_steps_leaves_the_run_alone(amd, n):
    """the engine's own tick for the size - one wave, one launch, pair + per-agent launches -: step(5), post_encroachment, step(5)
    ends bit for bit where step(10) of a twin ends"""
    box = max(BOX.get(n, 0.0), 3.0 * np.sqrt(n))
    a, b = (crowd(amd, n, box, seed=90 + n, ring=16, stride=1) for _ in range(2))
    a.step(5)
    r = a.post_encroachment(0, 5, pet_event=INF)
    assert r.seg_pet.shape == (4, n) and a.pet_launches() == 2
    if n < 3000:
        same_bits(r, pc.reference(a.recorded(0, 5)[0]))
    a.step(5)
    b.step(10)
    assert np.array_equal(a.state(), b.state())
    fa, fb = a.forces(), b.forces()
    assert np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1])
    assert a.small_ticks() == b.small_ticks() and a.mid_ticks() == b.mid_ticks()
    Sa, _ = a.recorded(0, 10)
    Sb, _ = b.recorded(0, 10)
    assert np.array_equal(Sa, Sb)


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_have_a_message_and_no_side_effect(amd):
    from calib_common import data_set, pod_sets
    a, twin = (crowd(amd, 40, 30.0, seed=10, ring=4, stride=1) for _ in range(2))
    plain = crowd(amd, 40, 30.0, seed=10, ring=None)
    a.step(6); twin.step(6); plain.step(6)
    lib = a._lib
    n = 40
    arrays = dict(p=np.full((3, n), -7.0), w=np.full((3, n), -7, np.int32), rp=np.full(n, -7.0), ev=np.zeros(8, amd.engine.PET_EVENT_DTYPE))

    def out(**kw):
        o = amd.ffi.PetOut()
        o.seg_pet, o.seg_with, o.run_pet = arrays["p"].ctypes.data, arrays["w"].ctypes.data, arrays["rp"].ctypes.data
        o.n_events = -7
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    ev = arrays["ev"].ctypes.data
    nan = float("nan")
    cases = {
        "out NULL": (a, 2, 4, 0.0, None),
        "the current state has no path": (a, -1, 1, 0.0, out()), "first below -1": (a, -2, 2, 0.0, out()),
        "no ring": (plain, 2, 4, 0.0, out()), "no ring, an empty window": (plain, 0, 0, 0.0, out()),
        "n_samples < 0": (a, 2, -1, 0.0, out()), "n_samples above 65535": (a, 2, 65536, 0.0, out()),
        "samples gone from the ring": (a, 1, 4, 0.0, out()), "samples not yet there": (a, 4, 3, 0.0, out()),
        "pet_event NaN": (a, 2, 4, nan, out()), "pet_event -inf": (a, 2, 4, -INF, out()),
        "capacity < 0": (a, 2, 4, 2.0, out(events=ev, event_capacity=-1)),
        "capacity without a buffer": (a, 2, 4, 2.0, out(event_capacity=8)),
    }
    n0 = {id(e): e.pet_launches() for e in (a, plain)}
    for name, (e, first, count, pe, o) in cases.items():
        rc = lib.csf_post_encroachment(e._h, first, count, pe, None if o is None else C.byref(o))
        assert rc in (-1, -4), (name, rc)
        assert lib.csf_last_error(e._h).decode(), name
        assert o is None or o.n_events == -7, name
        assert e.pet_launches() == n0[id(e)], name
    assert (arrays["p"] == -7.0).all() and (arrays["w"] == -7).all() and (arrays["rp"] == -7.0).all()
    # small calls succeed and find nothing, without a launch
    for count in (0, 1):
        o = out()
        assert lib.csf_post_encroachment(a._h, 3, count, INF, C.byref(o)) == 0 and o.n_events == 0 and o.first_sample == 3
        assert np.isinf(arrays["rp"]).all() and (arrays["p"] == -7.0).all()
        arrays["rp"][:] = -7.0
    assert a.pet_launches() == n0[id(a)]
    # the refused engine is where its twin is
    assert np.array_equal(a.state(), twin.state())
    a.step(5); twin.step(5)
    assert np.array_equal(a.state(), twin.state())
    assert np.array_equal(a.recorded(7, 4)[0], twin.recorded(7, 4)[0])
    # a member of a loopback group
    g = [crowd(amd, 40, 30.0, seed=10, ring=4, stride=1) for _ in range(2)]
    amd.Engine.loopback_group(g)
    o = out()
    rc = lib.csf_post_encroachment(g[0]._h, 0, 2, 0.0, C.byref(o))
    assert rc == -4 and lib.csf_last_error(g[0]._h).decode() and g[0].pet_launches() == 0 and o.n_events == -7
    # an engine that holds a calibration data set
    sets = pod_sets("twod", 2)
    cs0, cFx, cFy = data_set("twod", n_seq=2, ticks=20)
    c = amd.Engine(sets[0], 4)
    c.calib_load(cs0, cFx, cFy, np.zeros((20, 2, 2)), [0, 1], max_sets=2)
    rc = lib.csf_post_encroachment(c._h, 0, 2, 0.0, C.byref(o))
    assert rc == -4 and lib.csf_last_error(c._h).decode() and c.pet_launches() == 0
    # the batched call: not a batch, NULL outs, a bad threshold, too many samples
    outs = (amd.ffi.PetOut * 2)()
    arr = (C.c_void_p * 2)(a._h, twin._h)
    assert lib.csf_batch_post_encroachment(arr, 2, 2, 0.0, outs) == -4
    amd.Engine.batch_join([a, twin])
    assert lib.csf_batch_post_encroachment(arr, 2, 2, 0.0, None) == -1
    assert lib.csf_batch_post_encroachment(arr, 2, 2, nan, outs) == -1
    assert lib.csf_batch_post_encroachment(arr, 2, -1, 0.0, outs) == -1
    assert lib.csf_batch_post_encroachment(arr, 2, 5, 0.0, outs) == -1            # more than the ring of 4 holds
    assert a.pet_launches() == n0[id(a)]
    assert lib.csf_batch_post_encroachment(arr, 2, 2, 0.0, outs) == 0 and a.pet_launches() == n0[id(a)] + 2
    assert outs[0].first_sample == 9 and outs[1].first_sample == 9
    amd.Engine.batch_leave([a, twin])


# ---- 10. intersections ------------------------------------------------------------------------------------------------------------------
def test_intersections_together(amd):
    from cyclistsocialforce_amd import intersection as ci
    from cyclistsocialforce_amd.vehicle import TwoDBicycle
    scenes = []
    for k in range(3):
        s0 = pc.converging(3)
        s0[:, 0] += 0.2 * k
        vs = []
        for j, s in enumerate(s0):
            v = TwoDBicycle(tuple(s), id=f"s{k}r{j}")
            v.setDestinations(s[0] + np.array([30.0, 60.0]) * np.cos(s[2]), s[1] + np.array([30.0, 60.0]) * np.sin(s[2]))
            vs.append(v)
        scenes.append(ci.SocialForceIntersection(vs))
    ci.advance_together(scenes, 120)                              # (the dense route records every tick)
    res = ci.post_encroachment_together(scenes, 120, pet_event=INF)
    for k, (ins, r) in enumerate(zip(scenes, res)):
        alone = ins.post_encroachment(r.first, 120, pet_event=INF)
        same_bits(r, alone)
        same_events(r.events, alone.events)
        assert r.ids == [f"s{k}r{j}" for j in range(3)] and r.period == pytest.approx(0.01)
        assert all((a is None) == (j < 0) and (j < 0 or a == r.ids[j]) for a, j in zip(r.run_with_id, r.run_with))
        assert r.seg_with_id.shape == (119, 3)
        assert all((a is None) == (j < 0) and (j < 0 or a == r.ids[j]) for a, j in zip(r.seg_with_id.ravel(), r.seg_with.ravel()))
        assert list(r.event_i_id) == [r.ids[i] for i in r.events["i"]] and list(r.event_j_id) == [r.ids[j] for j in r.events["j"]]
        ref = pc.reference(ins.engine.recorded(r.first, 120)[0])
        not_vacuous(ref, 3, f"intersection {k}")
        same_bits(r, ref)
