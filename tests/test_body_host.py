"""Body encounters (include/csf.h: csf_body_encounters), the parts that need no GPU: the layout of the two structs
against the header, the Python argument checks, vehicle_extents, and the NumPy reference of tests/body_common.py - its bitwise
symmetry on a scattered crowd and the hand-computed cases."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import body_common as bc
import encounter_common as ec
from cyclistsocialforce_amd import _ffi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layouts_equal_the_header(tmp_path):
    """sizeof and every offsetof of csf_body_event and csf_body_out: include/csf.h through gcc, the binding's structs, and the NumPy
    dtype the events are returned as"""
    structs = {"csf_body_event": _ffi.BodyEvent, "csf_body_out": _ffi.BodyOut}
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
    for dt in (engine.BODY_EVENT_DTYPE, bc.EVENT_DTYPE):
        assert dt.itemsize == ctypes.sizeof(_ffi.BodyEvent)
        for f, _ in _ffi.BodyEvent._fields_:
            assert dt.fields[f][1] == getattr(_ffi.BodyEvent, f).offset, f
    names = {"csf_body_encounters", "csf_batch_body_encounters", "csf_body_encounter_launches"}
    assert names <= set(_ffi.SYMBOLS) and all(re.search(r"\bint %s\(" % s, header) for s in names)


class NoDevice:
    """stands where the library would: any call through it is the device call that must not happen"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was reached: an argument check let the call through")


class Bare(engine.Engine):
    """an Engine of three road users without a device behind it"""
    n = 3

    def __init__(self):
        self._lib, self._h = NoDevice(), 1

    def __del__(self):
        pass


OK = dict(extents=bc.BIKE)


@pytest.mark.parametrize("kw", [
    dict(), dict(extents=None), dict(extents="long"), dict(extents=(1.0, 1.0)), dict(extents=np.ones((2, 3))), dict(extents=np.ones((3, 2))),
    dict(extents=(1.0, 1.0, 0.0)), dict(extents=(-0.1, 1.0, 0.5)), dict(extents=(1.0, -0.1, 0.5)), dict(extents=(0.0, 0.0, 0.5)),
    dict(extents=(1.0, 1.0, float("nan"))), dict(extents=(float("inf"), 1.0, 0.5)), dict(extents=[bc.BIKE, bc.BIKE, (1.0, 1.0, -1.0)]),
    dict(OK, gap_event=float("nan")), dict(OK, gap_event=float("inf")), dict(OK, ttc_event="soon"), dict(OK, ttc_event=float("nan")),
    dict(OK, ttc_event=float("inf")), dict(OK, gap_event=True),
    dict(OK, count=2), dict(OK, first=0), dict(OK, first=-1, count=1), dict(OK, first=0, count=-1), dict(OK, first=0.5, count=1),
    dict(OK, first=0, count=1.5), dict(OK, first=0, count=65536),
])
def test_python_argument_checks_raise_before_any_device_call(kw):
    e = Bare()
    with pytest.raises((ValueError, TypeError)):
        e.body_encounters(**kw)
    if "first" not in kw and "count" not in kw:
        with pytest.raises((ValueError, TypeError)):
            engine.Engine.batch_body_encounters([e], 4, **kw)


def test_a_refused_extent_names_the_road_user():
    with pytest.raises(ValueError, match="road user 2"):
        Bare().body_encounters(extents=[bc.BIKE, bc.BIKE, (1.0, 1.0, 0.0)])
    with pytest.raises(ValueError, match="member 1.*road user 0"):
        engine.Engine.batch_body_encounters([Bare(), Bare()], 4, extents=[bc.BIKE, (0.0, 0.0, 1.0)])


def test_batch_argument_checks():
    e = Bare()
    for n_last in (-1, 1.5, 65536, None):
        with pytest.raises((ValueError, TypeError)):
            engine.Engine.batch_body_encounters([e], n_last, extents=bc.BIKE)
    with pytest.raises(ValueError):
        engine.Engine.batch_body_encounters([], 4, extents=bc.BIKE)      # no engines
    with pytest.raises(TypeError):
        engine.Engine.batch_body_encounters([object()], 4, extents=bc.BIKE)
    with pytest.raises(ValueError):
        engine.Engine.batch_body_encounters([e, Bare()], 4, extents=[bc.BIKE])   # one entry for two members
    ext = engine._batch_body_extents("t", [bc.BIKE, bc.extents(3)], [3, 3])
    assert ext[0].shape == (3, 3) and ext[0].flags.c_contiguous and np.array_equal(ext[1], bc.extents(3))
    assert all(np.array_equal(a, np.tile(bc.WIDE, (3, 1))) for a in engine._batch_body_extents("t", bc.WIDE, [3, 3]))


def test_events_wanted_and_the_pack_of_output_arrays():
    assert not engine._body_events_wanted(None, None) and not engine._body_events_wanted(-1.0, 0.0)
    assert engine._body_events_wanted(0.0, None) and engine._body_events_wanted(None, 1.5)
    assert engine._body_thresholds("t", None, None) == (-1.0, 0.0) and engine._body_thresholds("t", 0, 2) == (0.0, 2.0)
    pack = engine._BodyPack([(3, 4), (0, 4), (5, 0)], True, [7, 0, 2])
    o = pack.outs
    assert o[0].event_capacity == 7 and o[1].event_capacity == 0 and not o[1].events and o[2].event_capacity == 2
    assert o[2].events - o[0].events == 7 * 32 and o[1].gap_min - o[0].gap_min == 12 * 8 and o[1].run_gap_with - o[0].run_gap_with == 3 * 4
    assert o[1].overlap_n - o[0].overlap_n == 3 * 8 and o[2].ttc_with - o[0].ttc_with == 12 * 4
    r = pack.result(0, bc.extents(3), True)
    assert r.gap_min.shape == (4, 3) and r.ttc_with.dtype == np.int32 and r.run_gap_sample.shape == (3,) and r.events.dtype == engine.BODY_EVENT_DTYPE
    assert r.overlap_n.dtype == np.int64 and r.overlap_n.shape == (3,) and r.extents.shape == (3, 3)
    r = pack.result(2, bc.extents(5), False)                     # an empty window: nobody, at no sample, no overlap
    assert r.gap_min.shape == (0, 5) and np.isinf(r.run_ttc_min).all() and (r.run_gap_with == -1).all() and (r.run_gap_sample == -1).all()
    assert r.events is None and (r.overlap_n == 0).all() and r.collisions() is None
    assert engine._BodyPack([(3, 4)], False, [0]).result(0, None, False).gap_min is None


def test_vehicle_extents():
    from cyclistsocialforce_amd import parameters, vehicle

    class Of:
        def __init__(self, params):
            self.params = params

    bike = Of(parameters.BicycleParameters())
    f, r, w = vehicle.vehicle_extents(bike)
    assert (f, r, w) == (bike.params.l_2 + 0.325, bike.params.l_1 + 0.325, 0.225)
    long_bike = Of(parameters.BicycleParameters(l=None, l_1=0.5, l_2=0.85))
    np.testing.assert_allclose(vehicle.vehicle_extents(long_bike), bc.BIKE, rtol=1e-15)
    car = Of(parameters.CarParameters(length=4, width=2.0))
    assert vehicle.vehicle_extents(car) == (2.0, 2.0, 1.0)

    class Sledge:
        params = object()

    with pytest.raises(ValueError, match="Sledge"):
        vehicle.vehicle_extents(Sledge())


@pytest.mark.parametrize("n,box", [(33, 10.0), (70, 40.0)])
def test_reference_is_bitwise_symmetric_on_a_scattered_crowd(n, box):
    S = ec.scatter(n, box, seed=5)[None]
    p = bc.pairs(S, bc.extents(n))
    assert np.array_equal(p.GAP, p.GAP.transpose(0, 2, 1)) and np.array_equal(p.TTC, p.TTC.transpose(0, 2, 1))
    off = ~np.eye(n, dtype=bool)
    G, T = p.GAP[0][off], p.TTC[0][off]
    assert (G == 0).any() and (G > 0).any() and np.isfinite(T).any() and np.isinf(T).any() and ((T > 0) & np.isfinite(T)).any()
    assert np.array_equal(G == 0, T == 0)                        # overlapping now, and only then


@pytest.mark.parametrize("name,si,sj,ei,ej,gap,ttc", bc.KNOWN, ids=[k[0] for k in bc.KNOWN])
def test_reference_against_hand_computed_cases(name, si, sj, ei, ej, gap, ttc):
    S = np.array([[si, sj]])
    gm, gj, tm, tj = bc.per_sample(S, np.array([ei, ej]))
    if gap is not None:
        if gap == 0.0:
            assert list(gm[0]) == [0.0, 0.0]
        else:
            np.testing.assert_allclose(gm[0], [gap, gap], rtol=1e-14)
    assert list(gj[0]) == [1, 0]
    if np.isinf(ttc) or ttc == 0.0:
        assert list(tm[0]) == [ttc, ttc]
    else:
        np.testing.assert_allclose(tm[0], [ttc, ttc], rtol=1e-12)
    assert list(tj[0]) == ([-1, -1] if np.isinf(ttc) else [1, 0])
    p = bc.pairs(S, np.array([ei, ej]))
    assert p.GAP[0, 0, 1] == p.GAP[0, 1, 0] and p.TTC[0, 0, 1] == p.TTC[0, 1, 0]   # bitwise symmetric


def test_a_disc_would_get_these_wrong():
    """the issue's three examples: side by side at 0.6 m two bicycles do not touch; a wheel overlaps the wheel in front at 1.5 m
    between the points; a 4 x 2 m vehicle among cyclists"""
    side = np.array([[(0.0, 0.0, 0.0, 5.0), (0.0, 0.6, 0.0, 5.0)]])
    g, _, t, _ = bc.per_sample(side, bc.BIKE)
    np.testing.assert_allclose(g[0], [0.15, 0.15], rtol=1e-14)
    assert np.isinf(t).all()
    row = np.array([[(0.0, 0.0, 0.0, 5.0), (1.5, 0.0, 0.0, 5.0)]])
    g, _, t, _ = bc.per_sample(row, bc.BIKE)
    assert list(g[0]) == [0.0, 0.0] and list(t[0]) == [0.0, 0.0]
    car = np.array([[(0.0, 0.0, 0.0, 0.0), (0.0, 1.5, 0.0, 5.0), (3.0, 0.0, 0.0, 5.0)]])
    g, gj, _, _ = bc.per_sample(car, np.array([(2.0, 2.0, 1.0), bc.BIKE, bc.BIKE]))
    np.testing.assert_allclose(g[0], [0.175, 0.275, 0.175], rtol=1e-13)
    assert list(gj[0]) == [2, 0, 0]


def test_reference_ties_non_finite_riders_window_and_events():
    SQ = (1.0, 1.0, 0.5)                                        # (no offset of the centre: the gaps are exact)
    # three in a row, 4 m apart: the middle one is equally far from both - the lowest j wins
    S = np.array([[(0.0, 0.0, 0.0, 5.0), (4.0, 0.0, 0.0, 5.0), (8.0, 0.0, 0.0, 5.0)]])
    gm, gj, tm, tj = bc.per_sample(S, SQ)
    assert list(gm[0]) == [2.0, 2.0, 2.0] and list(gj[0]) == [1, 0, 1] and np.isinf(tm).all() and (tj == -1).all()
    S2 = S.copy()
    S2[0, 1, 2] = np.nan                                        # the middle one drops out: its row NaN / -1, the others find each other
    gm, gj, tm, tj = bc.per_sample(S2, SQ)
    assert np.isnan(gm[0, 1]) and np.isnan(tm[0, 1]) and gj[0, 1] == -1 and tj[0, 1] == -1
    assert list(gm[0, [0, 2]]) == [6.0, 6.0] and list(gj[0, [0, 2]]) == [2, 0]
    gm, gj, tm, tj = bc.per_sample(S[:, :1], SQ)
    assert np.isinf(gm[0, 0]) and np.isinf(tm[0, 0]) and gj[0, 0] == -1 and tj[0, 0] == -1
    # the window takes the earliest sample on ties, skips NaN rows and counts the samples with gap 0
    d = np.array([[3.0, np.nan], [0.0, 5.0], [0.0, 5.0]])
    w = np.array([[1, -1], [1, 0], [1, 0]], dtype=np.int32)
    rd, rw, rs, _, _, _, ov = bc.window(d, w, d, w, first=10)
    assert list(rd) == [0.0, 5.0] and list(rw) == [1, 0] and list(rs) == [11, 11] and list(ov) == [2, 0] and ov.dtype == np.int64
    # events: i < j, gap <= gap_event or ttc < ttc_event, sorted; gap_event 0 lists exactly the collisions
    S3 = np.array([[(0.0, 0.0, 0.0, 5.0), (1.5, 0.0, 0.0, 5.0), (21.0, 0.0, np.pi, 5.0)]])
    ev, edge = bc.events(S3, bc.BIKE, 0.0, 2.0, first=7)
    assert [(int(e["sample"]), int(e["i"]), int(e["j"])) for e in ev] == [(7, 0, 1), (7, 0, 2), (7, 1, 2)] and not edge
    assert ev["gap"][0] == 0.0 and ev["ttc"][0] == 0.0 and np.isclose(ev["ttc"][1], 1.865) and np.isclose(ev["gap"][2], 17.15)
    ev, _ = bc.events(S3, bc.BIKE, 0.0, None, first=7)
    assert [(int(e["i"]), int(e["j"])) for e in ev] == [(0, 1)]
    assert len(bc.events(S3, bc.BIKE, -1.0, 0.0, first=7)[0]) == 0
