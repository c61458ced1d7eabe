"""Following and passing (include/csf.h: csf_passing), the parts that need no GPU: the layout of the two structs against
the header, the Python argument checks, and the NumPy reference of tests/passing_common.py against hand-computed cases."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import passing_common as pc
from cyclistsocialforce_amd import _ffi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAN = float("nan")


def test_struct_layouts_equal_the_header(tmp_path):
    """sizeof and every offsetof of csf_passing_event and csf_passing_out: include/csf.h through gcc, the binding's structs, and the
    NumPy dtype the events are returned as"""
    structs = {"csf_passing_event": _ffi.PassingEvent, "csf_passing_out": _ffi.PassingOut}
    lines = []
    for name, cls in structs.items():
        lines.append(f'    printf("{name} sizeof %zu\\n", sizeof({name}));')
        lines += [f'    printf("{name} {f} %zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_]
    c = tmp_path / "layout.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "csf.h"\nint main(void) {\n' + "\n".join(lines) + "\n    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        s, f, v = line.split()
        got.setdefault(s, {})[f] = int(v)
    assert got["csf_passing_event"]["sizeof"] == 48
    for name, cls in structs.items():
        assert got[name].pop("sizeof") == ctypes.sizeof(cls), name
        assert len(got[name]) == len(cls._fields_)
        for f, _ in cls._fields_:
            assert got[name][f] == getattr(cls, f).offset, (name, f)
    # every member of the header is named in the binding, in order
    header = open(os.path.join(ROOT, "include", "csf.h")).read()
    for name, cls in structs.items():
        body = header[header.index("typedef struct %s {" % name):header.index("} %s;" % name)]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        body = body[body.index("{") + 1:]
        declared = [m.strip(" *") for stmt in body.split(";") if stmt.strip() for m in stmt.split(None, 1)[1].split(",")]   # `type a, *b;`
        assert declared == [f for f, _ in cls._fields_], name
    for dt in (engine.PASSING_EVENT_DTYPE, pc.EVENT_DTYPE):
        assert dt.itemsize == ctypes.sizeof(_ffi.PassingEvent)
        assert list(dt.names) == [f for f, _ in _ffi.PassingEvent._fields_]
        for f, _ in _ffi.PassingEvent._fields_:
            assert dt.fields[f][1] == getattr(_ffi.PassingEvent, f).offset, f
    # the arrays of a result, in the order of the header's pointers
    P = engine.Passing
    assert [f for f, _ in P.STATION + P.INTERVAL + P.RUN + P.COUNT] == [f for f, _ in _ffi.PassingOut._fields_[:27]]
    assert {"csf_passing", "csf_batch_passing", "csf_passing_launches"} <= set(_ffi.SYMBOLS)


class NoDevice:
    """stands where the library would: any call through it is the device call that must not happen"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was reached: an argument check let the call through")


def bare_engine():
    e = object.__new__(engine.Engine)
    e._lib, e._h = NoDevice(), None
    return e


@pytest.mark.parametrize("kw", [
    dict(first=None, count=None), dict(first=0, count=None), dict(first=None, count=4), dict(first=-1, count=1), dict(first=-1, count=4),
    dict(first=0, count=-1), dict(first=0.5, count=4), dict(first=0, count=4.5), dict(first=0, count=65536), dict(first="0", count=4),
    dict(first=0, count=4, band=NAN), dict(first=0, count=4, band=-0.5), dict(first=0, count=4, band="wide"), dict(first=0, count=4, band=None),
    dict(first=0, count=4, lat_max=NAN), dict(first=0, count=4, lat_max=0.0), dict(first=0, count=4, lat_max=-1.0), dict(first=0, count=4, lat_max=[3.0]),
    dict(first=0, count=4, lat_event=NAN), dict(first=0, count=4, lat_event=-INF), dict(first=0, count=4, lat_event="near"),
    dict(first=0, count=4, lat_event=[1.0]),
])
def test_python_argument_checks_raise_before_any_device_call(kw):
    e = bare_engine()
    with pytest.raises((ValueError, TypeError)):
        e.passing(**kw)
    shared = {k: v for k, v in kw.items() if k not in ("first", "count")}
    if shared:
        with pytest.raises((ValueError, TypeError)):
            engine.Engine.batch_passing([e], 4, **shared)


def test_batch_argument_checks():
    e = bare_engine()
    for n_last in (-1, 1.5, 65536, None):
        with pytest.raises((ValueError, TypeError)):
            engine.Engine.batch_passing([e], n_last)
    with pytest.raises(ValueError):
        engine.Engine.batch_passing([], 4)                       # no engines
    with pytest.raises(TypeError):
        engine.Engine.batch_passing([object()], 4)


def test_the_pack_of_output_arrays_and_in_seconds():
    pack = engine._PassingPack([(3, 4), (0, 4), (5, 1)], True, [7, 0, 2])
    o = pack.outs
    assert o[0].event_capacity == 7 and o[1].event_capacity == 0 and not o[1].events and o[2].event_capacity == 2
    assert o[2].events - o[0].events == 7 * 48
    assert o[1].gap - o[0].gap == 9 * 8 and o[1].gap_with - o[0].gap_with == 9 * 4 and o[1].thw - o[0].thw == 9 * 8      # 3 stations x 3
    assert o[1].made_lat - o[0].made_lat == 6 * 8 and o[1].by_kind - o[0].by_kind == 6 * 4                               # 2 intervals x 3
    assert o[2].run_gap - o[0].run_gap == 3 * 8 and o[2].run_thw_k - o[0].run_thw_k == 3 * 4 and o[2].run_by_t - o[0].run_by_t == 3 * 8
    assert o[2].run_made - o[0].run_made == 9 * 4 and o[2].run_by - o[0].run_by == 9 * 4
    assert len({getattr(o[0], f) for f, _ in _ffi.PassingOut._fields_[:28]}) == 28           # 27 arrays and the events: all apart
    r = pack.result(0, True, 0.2)
    assert r.gap.shape == (3, 3) and r.gap_with.dtype == np.int32 and r.made_lat.shape == (2, 3) and r.by_kind.dtype == np.int32
    assert r.run_gap.shape == (3,) and r.run_gap_k.dtype == np.int32 and r.run_made.shape == (3, 3) and r.run_by.dtype == np.int32
    assert r.events.dtype == engine.PASSING_EVENT_DTYPE and r.period == 0.2 and not r.seconds and r.ids is None
    last = pack.result(2, False, None)
    assert last.gap.shape == (0, 5) and last.made_lat.shape == (0, 5) and last.events is None and last.run_made.shape == (5, 3)
    assert engine._PassingPack([(3, 2)], True, [0]).result(0, False, None).made_t.shape == (0, 3)
    bare = engine._PassingPack([(3, 4)], False, [0])
    assert bare.result(0, False, None).gap is None and bare.result(0, False, None).by_lat is None and not bare.outs[0].gap and not bare.outs[0].by_kind
    assert bare.outs[0].run_gap and bare.outs[0].run_by
    assert engine._passing_capacity_guess(3) == 64 and engine._passing_capacity_guess(500) == 500 and engine._passing_capacity_guess(10 ** 7) == 65536
    r.gap[:], r.thw[:], r.made_t[:], r.by_t[:], r.made_lat[:], r.run_thw[:], r.run_made_t[:], r.run_by_t[:], r.run_gap[:] = 4.0, 2.0, 1.0, 3.0, 0.5, 2.0, 1.0, 3.0, 4.0
    r.events = np.zeros(1, engine.PASSING_EVENT_DTYPE)
    r.events["t"], r.events["lat"], r.events["closing"], r.events["cosine"] = 3.0, 0.5, 0.4, -1.0
    s = r.in_seconds()
    assert s.seconds and (s.thw == 0.4).all() and (s.made_t == 0.2).all() and (s.by_t == 3.0 * 0.2).all() and (s.run_by_t == 3.0 * 0.2).all()
    assert (s.gap == 4.0).all() and (s.made_lat == 0.5).all() and (s.run_gap == 4.0).all() and (s.run_thw == 0.4).all()
    assert s.events["t"][0] == 3.0 * 0.2 and s.events["closing"][0] == 0.4 / 0.2 and s.events["lat"][0] == 0.5 and s.events["cosine"][0] == -1.0
    assert r.events["t"][0] == 3.0 and r.events["closing"][0] == 0.4 and s.in_seconds() is s
    with pytest.raises(ValueError):
        last.in_seconds()


# ---- the reference against hand-computed cases: values to rtol 1e-12, counts, partners and kinds exact -----------------------------------
def close(a, b):
    np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)


def one_passing(r, i, j, k, kind, t, lat, closing, cosine):
    X = r.passings[(r.passings["i"] == i) & (r.passings["j"] == j)]
    assert len(X) == 1 and int(X["k"][0]) == k and int(X["kind"][0]) == kind
    close(X["t"], [t]); close(X["lat"], [lat]); close(X["closing"], [closing])
    if cosine is None:
        assert np.isnan(X["cosine"][0])
    else:
        close(X["cosine"], [cosine])
    # the rows of the passer and of the passed carry the same bits
    assert r.made_with[k, i] == j and r.made_kind[k, i] == kind and r.made_lat[k, i] == X["lat"][0] and r.made_t[k, i] == X["t"][0]
    assert r.by_with[k, j] == i and r.by_kind[k, j] == kind and r.by_lat[k, j] == X["lat"][0] and r.by_t[k, j] == X["t"][0]


def test_reference_overtake():
    """i from (0, 0) at +1.2 along x, j from (3, 1) at +0.8: i passes j in interval 7, s = 0.5"""
    r = pc.reference(pc.OVERTAKE, band=1.5)
    assert len(r.passings) == 1
    one_passing(r, 0, 1, 7, +1, 7.5, 1.0, 0.4, 1.0)
    assert r.run_made.tolist() == [[1, 0, 0], [0, 0, 0]] and r.run_by.tolist() == [[0, 0, 0], [1, 0, 0]]
    assert np.isinf(np.delete(r.made_lat[:, 0], 7)).all() and np.isinf(r.made_lat[:, 1]).all() and np.isinf(r.by_lat[:, 0]).all()
    assert r.made_lat.shape == (10, 2) and r.gap.shape == (11, 2)
    k = np.arange(8)
    assert (r.gap_with[:8, 0] == 1).all() and (r.gap_with[8:, 0] == -1).all() and np.isinf(r.gap[8:, 0]).all() and np.isinf(r.thw[8:, 0]).all()
    close(r.gap[:8, 0], 3.0 - 0.4 * k); close(r.thw[:8, 0], (3.0 - 0.4 * k) / 1.2)
    assert (r.gap_with[8:, 1] == 0).all() and (r.gap_with[:8, 1] == -1).all() and np.isinf(r.gap[:8, 1]).all()
    close(r.gap[8:, 1], 0.4 * np.arange(8, 11) - 3.0); close(r.thw[8:, 1], (0.4 * np.arange(8, 11) - 3.0) / 0.8)
    assert r.run_gap_k.tolist() == [7, 8] and r.run_gap_with.tolist() == [1, 0] and r.run_thw_k.tolist() == [7, 8]
    assert r.run_gap[0] == r.gap[7, 0] and r.run_thw[1] == r.thw[8, 1]
    assert r.run_made_with.tolist() == [1, -1] and r.run_by_with.tolist() == [-1, 0] and r.run_made_kind.tolist() == [1, 0]
    assert r.run_made_lat[0] == r.made_lat[7, 0] and np.isinf(r.run_made_lat[1]) and np.isnan(r.run_made_t[1]) and r.run_by_t[1] == r.made_t[7, 0]
    narrow = pc.reference(pc.OVERTAKE, band=0.5)                 # j rides 1 m to the side: outside the corridor
    assert np.isinf(narrow.gap).all() and (narrow.gap_with == -1).all() and np.isinf(narrow.thw).all() and (narrow.run_gap_k == -1).all()
    assert len(narrow.passings) == 1                            # (the band does not bear on passings)


def test_reference_meeting():
    """i from (0, 0) at +1 along x, j from (9, -1.5) at -1: each passes the other in interval 4, at 4.5; neither ever leads the other"""
    r = pc.reference(pc.MEETING, band=INF)
    assert len(r.passings) == 2
    one_passing(r, 0, 1, 4, -1, 4.5, -1.5, 2.0, -1.0)
    one_passing(r, 1, 0, 4, -1, 4.5, -1.5, 2.0, -1.0)
    for f in ("lat", "t", "kind"):                               # made and by carry the same bits, of either rider and across the two
        a, b = getattr(r, "made_" + f), getattr(r, "by_" + f)
        assert np.array_equal(a[:, 0], b[:, 1], equal_nan=True) and np.array_equal(a[:, 1], b[:, 0], equal_nan=True), f
        assert np.array_equal(a, b, equal_nan=True), f
    assert np.array_equal(r.made_with, r.by_with) and r.made_with[4].tolist() == [1, 0]
    assert r.run_made.tolist() == [[0, 1, 0], [0, 1, 0]] and r.run_by.tolist() == [[0, 1, 0], [0, 1, 0]]
    assert np.isinf(r.gap).all() and (r.gap_with == -1).all()    # dot < 0


def test_reference_a_stationary_partner():
    r = pc.reference(pc.STATIONARY)
    assert len(r.passings) == 1
    one_passing(r, 0, 1, 4, 0, 4.5, 0.5, 1.0, None)              # kind 0, cosine NaN
    assert r.run_made.tolist() == [[0, 0, 1], [0, 0, 0]] and r.run_by.tolist() == [[0, 0, 0], [0, 0, 1]]
    assert np.isinf(r.gap[:, 1]).all() and np.isinf(r.thw[:, 1]).all() and (r.gap_with[:, 1] == -1).all()      # exists, does not move
    assert np.isinf(r.made_lat[:, 1]).all() and not np.isnan(r.made_lat).any()
    assert (r.gap_with[:5, 0] == 1).all() and (r.gap_with[5:, 0] == -1).all()                                  # the leader while it is ahead
    close(r.gap[:5, 0], 4.5 - np.arange(5)); close(r.thw[:5, 0], 4.5 - np.arange(5))


def test_reference_a_lateral_offset_above_lat_max():
    r = pc.reference(pc.TOO_WIDE, band=INF)
    assert len(r.passings) == 0 and np.isinf(r.made_lat).all() and np.isinf(r.by_lat).all() and r.run_made.sum() == 0 and r.run_by.sum() == 0
    assert (r.made_with == -1).all() and np.isnan(r.made_t).all() and (r.made_kind == 0).all() and np.isnan(r.run_made_t).all()
    assert (r.gap_with[:8, 0] == 1).all()                        # (it is still ahead)
    assert len(pc.reference(pc.TOO_WIDE, lat_max=3.5).passings) == 1       # <= : exactly at the bound counts
    assert len(pc.reference(pc.TOO_WIDE, lat_max=INF).passings) == 1


def test_reference_exactly_abeam_at_a_sample():
    """j is at x = 4 exactly in sample 4, as i is (g = 0): counted once, in the interval that ends there, with s = 1"""
    r = pc.reference(pc.ABEAM, band=1.0)
    assert len(r.passings) == 1
    X = r.passings[0]
    assert (X["i"], X["j"], X["k"], X["kind"]) == (0, 1, 3, 1) and X["t"] == 4.0 and X["lat"] == 1.0 and X["closing"] == 0.5
    assert np.isinf(r.made_lat[4, 0]) and r.made_lat[3, 0] == 1.0
    assert r.gap_with[3, 0] == 1 and r.gap_with[4, 0] == -1      # g = 0 is not ahead


def test_reference_a_nan_sample():
    """i's x is NaN in sample 7: stations 6 and 7 of i do not exist, so intervals 5 (reads station 6), 6 and 7 are gone and with
    them the overtaking of interval 7; nobody else's rows change except where i was the partner"""
    whole = pc.reference(pc.OVERTAKE, band=1.5)
    S = pc.OVERTAKE.copy()
    S[7, 0, 0] = np.nan
    r = pc.reference(S, band=1.5)
    assert np.isnan(r.gap[[6, 7], 0]).all() and np.isnan(r.thw[[6, 7], 0]).all() and (r.gap_with[[6, 7], 0] == -1).all()
    assert np.isnan(r.made_lat[[6, 7], 0]).all() and (r.made_with[[6, 7], 0] == -1).all() and np.isnan(r.made_t[[6, 7], 0]).all()
    assert np.isinf(r.by_lat[:, 0]).all()
    keep = [0, 1, 2, 3, 4, 5, 8, 9, 10]
    for f in pc.STATION:
        assert np.array_equal(getattr(r, f)[keep, 0], getattr(whole, f)[keep, 0], equal_nan=True), f
    assert len(r.passings) == 0 and r.run_made.sum() == 0 and np.isinf(r.by_lat[:, 1]).all() and whole.by_with[7, 1] == 0
    assert r.run_gap_k[0] == 5 and r.run_gap[0] == whole.gap[5, 0]
    # j: i is nobody's partner at stations 6 and 7 - j was behind nobody there anyway -, and its leader again from station 8 on
    for f in pc.STATION:
        assert np.array_equal(getattr(r, f)[:, 1], getattr(whole, f)[:, 1], equal_nan=True), f
    # a third rider far away keeps every row
    far = pc.line((100.0, 100.0), (0.0, 1.0), pc.C_HAND)
    a = pc.reference(pc.states(*np.swapaxes(pc.OVERTAKE[:, :, :2], 0, 1), far), band=1.5)
    b = pc.reference(pc.states(*np.swapaxes(S[:, :, :2], 0, 1), far), band=1.5)
    for f in pc.STATION + pc.INTERVAL:
        assert np.array_equal(getattr(a, f)[:, 2], getattr(b, f)[:, 2], equal_nan=True), f


def test_reference_ties_go_to_the_lowest_partner():
    twin = pc.line((3.0, 1.0), (0.8, 0.0), pc.C_HAND)
    r = pc.reference(pc.states(pc.line((0.0, 0.0), (1.2, 0.0), pc.C_HAND), twin, twin), band=1.5)
    assert (r.gap_with[:8, 0] == 1).all() and r.made_with[7, 0] == 1 and r.run_made[0].tolist() == [2, 0, 0] and r.run_made_with[0] == 1
    assert r.by_with[7, 1] == 0 and r.by_with[7, 2] == 0
    # two passers of one rider at the same clearance: the lowest passer
    twin = pc.line((0.0, 0.0), (1.2, 0.0), pc.C_HAND)
    r = pc.reference(pc.states(pc.line((3.0, 1.0), (0.8, 0.0), pc.C_HAND), twin, twin), band=1.5)
    assert r.by_with[7, 0] == 1 and r.run_by[0].tolist() == [2, 0, 0] and r.run_by_with[0] == 1 and r.made_with[7, 2] == 0


def test_reference_random_walks():
    """the multiset of made passings equals the multiset of received ones; the counts add up"""
    rng = np.random.default_rng(5)
    S = np.zeros((8, 40, 5))
    S[0, :, :2] = rng.uniform(0, 20, (40, 2))
    S[1:, :, :2] = S[0, :, :2] + np.cumsum(rng.normal(0.6, 1.0, (7, 40, 2)), axis=0)
    r = pc.reference(S, band=1.0)
    X = r.passings
    assert len(X) > 40 and (X["kind"] > 0).any() and (X["kind"] < 0).any()
    assert int(r.run_made.sum()) == int(r.run_by.sum()) == len(X) and np.array_equal(r.run_made.sum(0), r.run_by.sum(0))
    made = sorted((int(k), int(i), int(w), float(lat), float(t), int(kind)) for k, i in zip(*np.nonzero(r.made_with >= 0))
                  for w, lat, t, kind in [(r.made_with[k, i], r.made_lat[k, i], r.made_t[k, i], r.made_kind[k, i])])
    listed = {(int(e["k"]), int(e["i"]), int(e["j"]), float(e["lat"]), float(e["t"]), int(e["kind"])) for e in X}
    assert set(made) <= listed
    by = {(int(k), int(r.by_with[k, j]), int(j), float(r.by_lat[k, j]), float(r.by_t[k, j]), int(r.by_kind[k, j])) for k, j in zip(*np.nonzero(r.by_with >= 0))}
    assert by <= listed
    # per passer and per passed the counts of the list
    assert np.array_equal(np.bincount(X["i"], minlength=40), r.run_made.sum(1)) and np.array_equal(np.bincount(X["j"], minlength=40), r.run_by.sum(1))
    lat, w, t, kind = pc.by_from_events(pc.events(r, INF), 40, 6)
    assert np.array_equal(lat, r.by_lat) and np.array_equal(w, r.by_with) and np.array_equal(t, r.by_t, equal_nan=True) and np.array_equal(kind, r.by_kind)
    assert len(pc.events(r, 1.0)) < len(X) and (np.abs(pc.events(r, 1.0)["lat"]) < 1.0).all()
    ev = pc.events(r, INF)
    key = list(zip(ev["i"].tolist(), ev["j"].tolist(), ev["k"].tolist()))
    assert key == sorted(key) and len(set(key)) == len(key)
    # small calls
    assert pc.reference(S[:1]).gap.shape == (0, 40) and pc.reference(S[:2]).made_lat.shape == (0, 40) and pc.reference(S[:2]).gap.shape == (1, 40)
    assert len(pc.reference(S[:2]).passings) == 0 and np.isinf(pc.reference(S[:1]).run_gap).all()
    alone = pc.reference(S[:, :1])
    assert np.isinf(alone.gap).all() and np.isinf(alone.made_lat).all() and len(alone.passings) == 0
