"""The lifetime of a recording (include/csf.h: csf_record, csf_enable_history - "the lifetime of a recording"): a state ring has a
first valid sample k0 = tick / stride of the moment it was started, or of the last change of the roster (csf_add_agents,
csf_remove_agents, csf_replace_agents), and every reader - csf_get_history, csf_get_record, csf_batch_get_record, the four analyses
and their batch forms - refuses what lies before it, before anything is written, launched or counted.

The reference of every test is an independent TWIN engine stepped one tick per call with a read-back after each (per_tick), never
the ring under test; the bar is bit identity, which tests/test_gpu_record.py establishes between a long call and such a twin.  Where
the roster changes the twin carries a ring of its own kind (of one sample, never read), so that the change takes the same way
through the host mirror on both sides.

Without the rule (the engine before it) the rings were wrong in silence.  Samples from before the ring existed came back as zeros
(test_a_ring_begun_mid_run, test_a_ring_restarted, test_wrapping_after_a_late_start, the analyses, the batch forms), and samples
written under another roster were read with the new one's row length or named another road user (test_arrivals_departures_a_swap,
test_intersection_swaps_a_rider_between_dense_calls).

The windows of the analyses (ring begun at tick 4 of a sample per tick for the encounters, at tick 25 of a sample every 20 ticks
for the others, eight samples instead of the suites' six to eight) were chosen on the CPU oracle's trajectories of the suites' own
crowds so that the suites' own not_vacuous conditions hold: 3 and 70 riders - post-encroachment 4 and 38 crossings (3 and 29 riders
with a finite PET); passing 5 (1 overtaking) and 78 (16 overtakings, 62 meetings; 48 riders pass, 52 have a leader); flow crossings
of the first three lines both ways, 5 sign changes refused on the short line, 15 and 18 riders entering or leaving the areas, 119
samples outside the grid; encounters 10 of 15 and 267 of 350 cells with a finite time to collision (the three riders have one in
their first eleven ticks only: hence the early start of that ring)."""
import ctypes as C

import numpy as np
import pytest

import encounter_common as ec
import flow_common as fc
import passing_common as pac
import pet_common as pc
import test_gpu_encounters as t_enc
import test_gpu_flow as t_flow
import test_gpu_passing as t_pas
import test_gpu_pet as t_pet
from cyclistsocialforce_amd._ffi import EngineError
from test_gpu_batch import assert_same
from test_gpu_record import _same_vehicles, per_tick, rider_crowd

pytestmark = [pytest.mark.gpu, pytest.mark.auto_variant]

INF = float("inf")
REFUSED = "not in the ring"
# the writers of the ring (tests/test_gpu_record.py::test_every_path_records_the_same_thing): the one-wave tick, the one-launch tick
# of a mid-size population, the general path (a pinned pair kernel), and csf_enable_history's ring (the general path as well)
PATHS = {"wave": 3, "mid": 40, "general": 9, "history": 9}


@pytest.fixture(scope="module")
def amd():
    from cyclistsocialforce_amd import _ffi, engine, parameters

    class NS:
        pass

    ns = NS()
    ns.Engine, ns.pod, ns.ffi, ns.engine = engine.Engine, parameters.default_pod, _ffi, engine
    return ns


def twins(amd, monkeypatch, how, room=0):
    """two engines of the same crowd on the path `how`, with room for `room` arrivals"""
    if how in ("general", "history"):
        monkeypatch.setenv("CSF_PAIR_VARIANT", "0")
    n = PATHS[how]
    return [rider_crowd(amd, "twod", n, False, seed=77, capacity=n + room) for _ in range(2)]


def begin(e, how, stride, capacity):
    if how == "history":
        e.enable_history(stride, capacity)
    else:
        e.record(stride=stride, capacity=capacity)


def read(e, how, first, count):
    """(S, F) of the ring: csf_get_record, or csf_get_history for the ring of csf_enable_history (F None)"""
    return (e.history(first, count), None) if how == "history" else e.recorded(first, count)


def took_its_path(e, how):
    assert (e.small_ticks() > 0) == (how == "wave") and (e.mid_ticks() > 0) == (how == "mid"), (how, e.small_ticks(), e.mid_ticks())


def same_samples(got, S, F, what=""):
    assert got[0].shape == S.shape, (what, got[0].shape, S.shape)
    assert np.array_equal(got[0], S), what
    if got[1] is not None:
        assert np.array_equal(got[1], F), what


def refused(call, *args, **kw):
    with pytest.raises(EngineError, match=REFUSED) as err:
        call(*args, **kw)
    return str(err.value)


# ---- 1. a ring begun mid-run ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride,begun", [(1, 25), (3, 25), (3, 24)])
@pytest.mark.parametrize("how", list(PATHS))
def test_a_ring_begun_mid_run(amd, monkeypatch, how, stride, begun):
    """ring begun at tick 25 (24), 20 more ticks: k0 = 25 for a sample per tick, 8 for one every third (sample 8 is tick 27 both
    times); what is readable equals the twin's ticks, what lies before is refused and nothing has changed"""
    a, b = twins(amd, monkeypatch, how)
    a.step(begun)
    begin(a, how, stride, 64)
    a.step(20)
    S, F = per_tick(b, begun + 20)                                # S[t - 1]: the state after tick t
    took_its_path(a, how)
    k0, have = begun // stride, (begun + 20) // stride
    assert (k0, have) == {(1, 25): (25, 45), (3, 25): (8, 15), (3, 24): (8, 14)}[stride, begun]
    at = [(k + 1) * stride - 1 for k in range(k0, have)]          # sample k is tick (k + 1) * stride
    assert at[0] == {1: 25, 3: 26}[stride]                       # (tick 26, tick 27)
    same_samples(read(a, how, k0, have - k0), S[at], F[at], "the whole stretch")
    assert np.array_equal(a.history(k0, have - k0), S[at])       # (csf_get_history reads the same ring)
    same_samples(read(a, how, k0, 1), S[at[:1]], F[at[:1]], "the first readable sample")
    same_samples(read(a, how, have - 3, 3), S[at[-3:]], F[at[-3:]], "the last three")
    for call, first, count in ((a.recorded, k0 - 1, 2), (a.recorded, 0, min(10, have)), (a.history, 0, have), (a.history, k0 - 1, 1),
                               (a.recorded, k0 - 1, 0)):
        msg = refused(call, first, count)
        assert f"first readable sample {k0}" in msg, msg
        assert_same(a, b, f"after the refused {call.__name__}({first}, {count})")
    same_samples(read(a, how, k0, have - k0), S[at], F[at], "after the refusals")


# ---- 2. a ring restarted ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", list(PATHS))
def test_a_ring_restarted(amd, monkeypatch, how):
    """a ring of every tick, 10 ticks, a ring of every second tick, 12 ticks: samples 5 .. 10 of the new numbering (ticks 12 .. 22)
    are readable and the twin's, sample 4 (tick 10: the old ring's) is refused"""
    a, b = twins(amd, monkeypatch, how)
    begin(a, how, 1, 64)
    a.step(10)
    begin(a, how, 2, 16)
    a.step(12)
    S, F = per_tick(b, 22)
    at = [2 * k + 1 for k in range(5, 11)]
    same_samples(read(a, how, 5, 6), S[at], F[at])
    same_samples(read(a, how, 7, 2), S[at[2:4]], F[at[2:4]])
    for first, count in ((4, 1), (4, 3), (0, 11), (0, 5)):
        assert "first readable sample 5" in refused(a.recorded, first, count)
        refused(a.history, first, count)
    assert_same(a, b, "after the refusals")


# ---- 3. arrivals, departures, a swap ----------------------------------------------------------------------------------------------------
def newcomers(e, k):
    s = np.zeros((k, e.ns))
    s[:, :4] = [(3.0 + 2.0 * j, 4.0 + j, 0.3, 4.0) for j in range(k)]
    off = np.arange(k + 1) * 2
    rows = np.array([row for j in range(k) for row in ((s[j, 0], s[j, 1], 0.0), (80.0, 30.0 + j, 0.0))])
    return s, off, rows


def arrive(e):
    s, off, rows = newcomers(e, 2)
    e.add_agents(s, 5.0)
    e.set_dest_queue(np.arange(e.n - 2, e.n), off, rows, reset=True)
    return 2


def leave(e):
    e.remove_agents(np.array([1], dtype=np.int32))
    return -1


def swap(e):
    e.replace_agents([1], *newcomers(e, 1)[:1], 5.0, *newcomers(e, 1)[1:])
    return 0


@pytest.mark.parametrize("change", [arrive, leave, swap])
@pytest.mark.parametrize("how", ["wave", "mid", "history"])
def test_arrivals_departures_a_swap(amd, monkeypatch, how, change):
    """recording from tick 0, 10 ticks, a refused arrival (nothing changes: samples 0 .. 9 stay readable), the change of the roster
    on both engines, 10 ticks: samples 10 .. 19 are the twin's ticks 11 .. 20 of the new roster, and no window that begins before
    sample 10 is served"""
    a, b = twins(amd, monkeypatch, how, room=2)
    begin(a, how, 1, 64)
    begin(b, how, 1, 1)                                          # (the same way through the host mirror; never read)
    n0 = a.n
    a.step(10)
    S1, F1 = per_tick(b, 10)
    # tests/hostile_caller.py: an arrival without a queue row; arrivals beyond the capacity
    s, _, _ = newcomers(a, 1)
    with pytest.raises(EngineError, match="queue must have a row"):
        a.replace_agents([], s, 5.0, [0, 0], np.zeros((0, 3)))
    with pytest.raises(EngineError, match="capacity"):
        a.add_agents(np.zeros((3, a.ns)), 5.0)
    with pytest.raises(EngineError, match="out of range"):
        a.remove_agents(np.array([n0], dtype=np.int32))
    assert a.n == n0
    same_samples(read(a, how, 0, 10), S1, F1, "after the refused arrivals")
    same_samples(read(a, how, 3, 4), S1[3:7], F1[3:7])
    assert_same(a, b, "after the refused arrivals")
    grown = change(a)
    assert change(b) == grown and a.n == b.n == n0 + grown
    for first, count in ((0, 10), (9, 1), (3, 4)):                # at once: the old roster's samples are gone
        refused(a.recorded, first, count)
    a.step(10)
    S2, F2 = per_tick(b, 10)
    assert S2.shape[1] == n0 + grown
    took_its_path(a, how)
    same_samples(read(a, how, 10, 10), S2, F2, "the new stretch")
    same_samples(read(a, how, 14, 3), S2[4:7], F2[4:7])
    assert np.array_equal(a.history(10, 10), S2)
    for first in range(10):
        for count in (0, 1, 10 - first, 11 - first, 20 - first):
            msg = refused(a.recorded, first, count)
            assert "first readable sample 10" in msg, msg
            refused(a.history, first, count)
    assert_same(a, b, "after the refusals")
    same_samples(read(a, how, 10, 10), S2, F2, "after the refusals")


def test_a_pushed_state_a_desired_speed_and_a_queue_leave_the_stretch_alone(amd):
    """csf_push_state, csf_set_v_desired and csf_set_dest_queue do not change the roster: samples from before them stay readable"""
    a, b = (rider_crowd(amd, "twod", 6, True) for _ in range(2))
    a.record(stride=1, capacity=64)
    a.step(8)
    S, F = per_tick(b, 8)
    for e in (a, b):
        s = e.state()
        s[:, 3] *= 0.8
        e.push_state(np.arange(e.n, dtype=np.int32), s)
        e.set_v_desired(np.arange(e.n, dtype=np.int32), np.full(e.n, 4.5))
        e.set_dest_queue(np.array([2]), np.array([0, 2]), np.array([[1.0, 2.0, 0.0], [60.0, 30.0, 0.0]]), reset=True)
    a.step(7)
    S2, F2 = per_tick(b, 7)
    same_samples(a.recorded(0, 15), np.concatenate([S, S2]), np.concatenate([F, F2]))


# ---- 4. wrapping after a late start -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", list(PATHS))
def test_wrapping_after_a_late_start(amd, monkeypatch, how):
    """capacity 8, ring begun at tick 21, 30 more ticks: the last 8 samples are the twin's, one more is refused by the capacity"""
    a, b = twins(amd, monkeypatch, how)
    a.step(21)
    begin(a, how, 1, 8)
    a.step(30)
    S, F = per_tick(b, 51)
    same_samples(read(a, how, 43, 8), S[43:], F[43:])
    same_samples(read(a, how, 47, 2), S[47:49], F[47:49])
    for first, count in ((42, 9), (42, 1), (21, 8), (0, 8)):
        assert "first readable sample 43" in refused(a.recorded, first, count)
    assert_same(a, b, "after the refusals")


# ---- 5. the four analyses on a ring begun late ------------------------------------------------------------------------------------------
def back(s0, metres):
    """the riders that far back along their headings (tests/test_gpu_pet.py::test_a_wrapped_ring: so that they meet inside the window)"""
    s0 = s0.copy()
    s0[:, 0] -= metres * np.cos(s0[:, 2])
    s0[:, 1] -= metres * np.sin(s0[:, 2])
    return s0


def late_pair(make, stride, begun, count):
    """(a, S, k0): engine a of make(), its ring of every `stride`-th tick begun at tick `begun` and run until `count` samples are
    readable from k0 on; S [count, n, ns] those samples as a twin stepped tick by tick shows them"""
    a, b = make(), make()
    k0 = begun // stride
    ticks = (k0 + count) * stride
    a.step(begun)
    a.record(stride=stride, capacity=count + 2, forces=False)
    a.step(ticks - begun)
    S = per_tick(b, ticks)[0][stride - 1::stride][k0:k0 + count]
    assert S.shape[0] == count and np.array_equal(a.recorded(k0, count)[0], S)
    assert (a.small_ticks() > 0) == (a.n <= 32) and (a.mid_ticks() > 0) == (a.n > 32)
    return a, S, k0


def refused_without_a_launch(call, launches, k0, count):
    n0 = launches()
    for first, c in ((k0 - 1, 2), (0, count), (k0 - 1, count + 1), (0, 1)):
        refused(call, first, c)
    assert launches() == n0


@pytest.mark.parametrize("n", [3, 70])
def test_encounters_on_a_ring_begun_late(amd, n):
    a, S, k0 = late_pair(lambda: t_enc.crowd(amd, n, t_enc.BOX[n], seed=100 + n), 1, 4, 5)
    assert k0 == 4
    ttc = ec.per_sample(S, t_enc.RADIUS)[2]
    assert np.isfinite(ttc).any(), "vacuous: the reference finds no finite time to collision"
    r = a.encounters(k0, 5, radius=t_enc.RADIUS)
    assert r.first == k0
    t_enc.check_per_sample(r, S, t_enc.RADIUS, f"n = {n}, samples {k0} .. {k0 + 4}")
    t_enc.check_window(r, k0)
    refused_without_a_launch(lambda f, c: a.encounters(f, c, radius=t_enc.RADIUS), a.encounter_launches, k0, 5)
    now = a.encounters(radius=t_enc.RADIUS)                      # (the current state is no sample of the ring)
    assert np.array_equal(now.d_min[0], r.d_min[4])


@pytest.mark.parametrize("n", [3, 70])
def test_post_encroachment_on_a_ring_begun_late(amd, n):
    s0 = back(pc.converging(3), 1.25) if n == 3 else None
    a, S, k0 = late_pair(lambda: t_pet.crowd(amd, n, ring=None, s0=s0), 20, 25, 8)
    assert k0 == 1
    ref = pc.reference(S)
    t_pet.not_vacuous(ref, n, f"n = {n}, samples 1 .. 8")
    r = a.post_encroachment(k0, 8, pet_event=INF)
    assert r.first == k0
    t_pet.same_bits(r, ref)
    t_pet.same_events(r.events, pc.events(ref, INF))
    refused_without_a_launch(a.post_encroachment, a.pet_launches, k0, 8)


@pytest.mark.parametrize("n", [3, 70])
def test_passing_on_a_ring_begun_late(amd, n):
    a, S, k0 = late_pair(lambda: t_pas.crowd(amd, n, ring=None), 20, 25, 8)
    ref = pac.reference(S, t_pas.BAND, t_pas.LAT_MAX)
    t_pas.not_vacuous(ref, n, f"n = {n}, samples 1 .. 8")
    r = a.passing(k0, 8, t_pas.BAND, t_pas.LAT_MAX, lat_event=INF)
    assert r.first == k0 == 1
    t_pas.same_bits(r, ref)
    t_pas.same_events(r.events, pac.events(ref, INF))
    t_pas.invariants(r, n)
    refused_without_a_launch(lambda f, c: a.passing(f, c, t_pas.BAND, t_pas.LAT_MAX), a.passing_launches, k0, 8)


@pytest.mark.parametrize("n", [3, 70])
def test_flow_on_a_ring_begun_late(amd, n):
    a, S, k0 = late_pair(lambda: t_flow.crowd(amd, n, ring=None), 20, 25, 8)
    lay = t_flow.layout_of(n)
    ref = fc.reference(S, *lay)
    t_flow.not_vacuous(ref, n, f"n = {n}, samples 1 .. 8")
    r = a.flow(k0, 8, *lay, events=True)
    assert r.first == k0 == 1
    t_flow.same_bits(r, ref)
    t_flow.same_events(r.events, fc.events(ref))
    t_flow.invariants(r, n, ref.n_exist)
    refused_without_a_launch(lambda f, c: a.flow(f, c, *lay), a.flow_launches, k0, 8)


# ---- 6. the batch forms -----------------------------------------------------------------------------------------------------------------
def sentinel(arrays):
    """every byte of the arrays 0xA5; returns their copies"""
    for x in arrays:
        x.view(np.uint8).reshape(-1)[:] = 0xA5
    return [x.copy() for x in arrays]


def test_batch_forms_with_a_late_member(amd):
    """three members: one records from tick 0, one since 6 ticks, one not at all.  The last 6 samples are served to all five batched
    calls and equal each member's own call and its twin; the last 7 are refused, naming the late member, with every output as it was"""
    def make():
        return [rider_crowd(amd, "twod", n, False, seed=300 + n, capacity=8) for n in (3, 5, 4)]
    batch, twin = make(), make()
    batch[0].record(stride=1, capacity=64)
    for e in batch:
        e.step(10)
    batch[1].record(stride=1, capacity=64)
    amd.Engine.batch_join(batch)
    amd.Engine.step_batch(batch, 6)
    ref = [per_tick(t, 16) for t in twin]
    assert all(e.batch_ticks() == 6 for e in batch)
    got = amd.Engine.batch_recorded(batch, 6)
    assert got[2] is None
    for i in (0, 1):
        S, F, first = got[i]
        assert first == 10
        same_samples((S, F), ref[i][0][10:], ref[i][1][10:], f"member {i}")
        same_samples(batch[i].recorded(10, 6), S, F, f"member {i} alone")
    lay = fc.layout(14.0)
    calls = {
        "encounters": (lambda: amd.Engine.batch_encounters(batch, 6, radius=0.5, d_event=2.0, ttc_event=3.0),
                       lambda e: e.encounters(10, 6, radius=0.5, d_event=2.0, ttc_event=3.0), t_enc.same_bits),
        "pet": (lambda: amd.Engine.batch_post_encroachment(batch, 6, pet_event=INF), lambda e: e.post_encroachment(10, 6, pet_event=INF),
                lambda r, w: (t_pet.same_bits(r, w), t_pet.same_events(r.events, w.events))),
        "passing": (lambda: amd.Engine.batch_passing(batch, 6, 1.0, 3.0, lat_event=INF), lambda e: e.passing(10, 6, 1.0, 3.0, lat_event=INF),
                    lambda r, w: (t_pas.same_bits(r, w), t_pas.same_events(r.events, w.events))),
        "flow": (lambda: amd.Engine.batch_flow(batch, 6, *lay, events=True), lambda e: e.flow(10, 6, *lay, events=True),
                 lambda r, w: (t_flow.same_bits(r, w), t_flow.same_events(r.events, w.events))),
    }
    for name, (together, alone, same) in calls.items():
        res = together()
        assert res[2] is None, name
        for i in (0, 1):
            assert res[i].first == 10, (name, i)
            same(res[i], alone(batch[i]))
    # on the twins' states: the path-based analyses bit for bit, the encounters as their suite compares them
    for i in (0, 1):
        S = ref[i][0][10:]
        t_pet.same_bits(calls["pet"][0]()[i], pc.reference(S))
        t_pas.same_bits(calls["passing"][0]()[i], pac.reference(S, 1.0, 3.0))
        t_flow.same_bits(calls["flow"][0]()[i], fc.reference(S, *lay))
        t_enc.check_per_sample(calls["encounters"][0]()[i], S, 0.5, f"member {i}")
    # the last 7: member 1 has 6
    lib = batch[0]._lib
    arr = (C.c_void_p * 3)(*[e._h for e in batch])
    shapes = [(e.n, 7) for e in batch]
    launches = [(e.encounter_launches(), e.pet_launches(), e.passing_launches(), e.flow_launches()) for e in batch]
    late = "member 1: the last 7 samples are not in the ring"

    def refused_raw(name, rc, arrays, before):
        msg = lib.csf_last_error(batch[1]._h).decode()
        assert rc == -1 and late in msg and "first readable sample 10" in msg, (name, rc, msg)
        for x, w in zip(arrays, before):
            assert x.tobytes() == w.tobytes(), name

    p = amd.engine._EncounterPack(shapes, True, [8, 8, 8])
    arrays = list(p.per) + list(p.run) + [p.events]
    before = sentinel(arrays) + [p._tab.copy()]
    refused_raw("encounters", lib.csf_batch_encounters(arr, 3, 7, 0.5, 2.0, 3.0, p.outs), arrays + [p._tab], before)
    p = amd.engine._PetPack(shapes, True, [8, 8, 8])
    arrays = list(p.seg) + list(p.run) + [p.events]
    before = sentinel(arrays) + [p._tab.copy()]
    refused_raw("pet", lib.csf_batch_post_encroachment(arr, 3, 7, INF, p.outs), arrays + [p._tab], before)
    p = amd.engine._PassingPack(shapes, True, [8, 8, 8])
    arrays = list(p.station) + list(p.interval) + list(p.run) + list(p.count) + [p.events]
    before = sentinel(arrays) + [p._tab.copy()]
    refused_raw("passing", lib.csf_batch_passing(arr, 3, 7, 1.0, 3.0, INF, p.outs), arrays + [p._tab], before)
    p = amd.engine._FlowPack(shapes, *amd.engine._flow_layout("flow", *lay), [8, 8, 8])
    arrays = list(p.arrays.values()) + [p.events]
    before = sentinel(arrays) + [p._tab.copy()]
    refused_raw("flow", lib.csf_batch_flow(arr, 3, 7, C.byref(p.layout), p.outs), arrays + [p._tab], before)
    outs = (amd.ffi.RecordOut * 3)()
    firsts = (C.c_int64 * 3)(-7, -7, -7)
    arrays = []
    for i in (0, 1):
        S, F = np.zeros((7, batch[i].n, batch[i].ns)), np.zeros((7, batch[i].n, 2))
        outs[i].s, outs[i].F = S.ctypes.data, F.ctypes.data
        outs[i].first_sample = C.cast(C.byref(firsts, i * C.sizeof(C.c_int64)), C.POINTER(C.c_int64))
        arrays += [S, F]
    before = sentinel(arrays)
    refused_raw("get_record", lib.csf_batch_get_record(arr, 3, 7, outs), arrays, before)
    assert list(firsts) == [-7, -7, -7]
    with pytest.raises(EngineError, match=late):
        amd.Engine.batch_recorded(batch, 7)
    with pytest.raises(EngineError, match=late):
        amd.Engine.batch_flow(batch, 7, *lay)
    assert launches == [(e.encounter_launches(), e.pet_launches(), e.passing_launches(), e.flow_launches()) for e in batch]
    for e, t in zip(batch, twin):
        assert_same(e, t, "after the refusals")
    amd.Engine.batch_leave(batch)


# ---- 7. the Python layer ----------------------------------------------------------------------------------------------------------------
def _scene():
    from cyclistsocialforce_amd.intersection import SocialForceIntersection
    from cyclistsocialforce_amd.vehicle import TwoDBicycle
    vs = []
    for j, s in enumerate(fc.placed(3)):
        v = TwoDBicycle(tuple(s), id=f"r{j}", saveForces=True)
        v.setDestinations(s[0] + np.array([30.0, 60.0]) * np.cos(s[2]), s[1] + np.array([30.0, 60.0]) * np.sin(s[2]))
        vs.append(v)
    return SocialForceIntersection(vs)


def _swap_a_rider(ins):
    from cyclistsocialforce_amd.vehicle import TwoDBicycle
    ins.remove_road_users_by_id(["r1"])
    v = TwoDBicycle((6.0, 2.5, -0.2, 4.0, 0.0), id="new", saveForces=True)
    v.setDestinations(6.0 + np.array([30.0, 60.0]) * np.cos(-0.2), 2.5 + np.array([30.0, 60.0]) * np.sin(-0.2))
    ins.add_road_user(v)


def test_intersection_swaps_a_rider_between_dense_calls():
    """step_n(40, dense=True), one rider swapped for another (the same n), step_n(40, dense=True): the vehicles are a twin's that
    took 80 calls of step(), flow over the second stretch is the reference's on the twin's states, and a window that reaches into
    the first stretch - where row 1 was another rider - raises.

    The twin's engine carries a ring of one sample that nobody reads, as the twins of test_arrivals_departures_a_swap do: an engine
    with a ring takes a change of its roster through the host mirror and closes the leaver's slot, one without patches the device
    in place and the arrival takes the leaver's slot - the pair sums then run over the sources in another order and the states
    differ in their last bits (seen on the MI355X without this ring: rider r0 after 80 ticks, x equal to all printed digits)."""
    ins, twin = _scene(), _scene()
    twin.engine.record(stride=1, capacity=1)
    ins.step_n(40, dense=True)
    _swap_a_rider(ins)
    ins.step_n(40, dense=True)
    S = []
    for t in range(80):
        if t == 40:
            _swap_a_rider(twin)
        twin.step()
        S.append(np.array([np.asarray(v.s, dtype=float)[:5] for v in twin.vehicles]))
    S = np.array(S)
    assert ins.get_road_user_ids() == twin.get_road_user_ids() == ["r0", "r2", "new"]
    _same_vehicles(twin, ins, "after the swap")
    assert ins.engine.small_ticks() == 80
    assert np.array_equal(ins.engine.recorded(40, 40)[0], S[40:])
    lines = np.array([(x, -6.0, x, 6.0) for x in np.arange(-2.0, 14.5, 1.0)])      # a line every metre across the riders' way
    _, areas, grid = t_flow.layout_of(3)
    ref = fc.reference(S[40:], lines, areas, grid)
    assert len(ref.crossings) >= 3, "vacuous: the reference finds no crossing in the second stretch"
    r = ins.flow(40, 40, lines, areas, grid, events=True)
    assert r.first == 40 and r.ids == ["r0", "r2", "new"]
    t_flow.same_bits(r, ref)
    t_flow.same_events(r.events, fc.events(ref))
    n0 = ins.engine.flow_launches()
    for first, count in ((39, 10), (0, 40), (0, 80), (20, 40)):
        refused(ins.flow, first, count, lines, areas, grid)
        refused(ins.passing, first, count)
        refused(ins.post_encroachment, first, count)
        refused(ins.encounters, first, count)
    assert ins.engine.flow_launches() == n0
