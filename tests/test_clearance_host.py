"""Road clearance (include/csf.h: csf_clearance), the parts that need no GPU: the layout of the three structs against
the header, the Python argument checks, the NumPy reference of tests/clearance_common.py against hand-computed dyadic cases, and the
helpers of engine.Clearance on a hand-made result."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import clearance_common as cc
from cyclistsocialforce_amd import _ffi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAN = float("nan")


def test_struct_layouts_equal_the_header(tmp_path):
    """sizeof and every offsetof of csf_clearance_road, csf_clearance_event and csf_clearance_out: include/csf.h through gcc, the
    binding's structs, and the NumPy dtype the events are returned as"""
    structs = {"csf_clearance_road": _ffi.ClearanceRoad, "csf_clearance_event": _ffi.ClearanceEvent, "csf_clearance_out": _ffi.ClearanceOut}
    lines = []
    for name, cls in structs.items():
        lines.append(f'    printf("{name} sizeof %zu\\n", sizeof({name}));')
        lines += [f'    printf("{name} {f} %zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_]
    c = tmp_path / "layout.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "csf.h"\nint main(void) {\n' + "\n".join(lines) + "\n    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = {}
    for row in subprocess.check_output([str(exe)], text=True).splitlines():
        s, f, v = row.split()
        got.setdefault(s, {})[f] = int(v)
    assert got["csf_clearance_event"]["sizeof"] == 40
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
        declared = [re.findall(r"\w+", part)[-1] for stmt in body.split(";") if stmt.strip() for part in stmt.split(",")]
        assert declared == [f for f, _ in cls._fields_], name
    for dt in (engine.CLEARANCE_EVENT_DTYPE, cc.EVENT_DTYPE):
        assert dt.itemsize == ctypes.sizeof(_ffi.ClearanceEvent) == 40
        assert list(dt.names) == [f for f, _ in _ffi.ClearanceEvent._fields_]
        for f, _ in _ffi.ClearanceEvent._fields_:
            assert dt.fields[f][1] == getattr(_ffi.ClearanceEvent, f).offset, f
    # the arrays of a result, in the order of the header's pointers
    assert [f for f, _ in engine.Clearance.ARRAYS] == [f for f, _ in _ffi.ClearanceOut._fields_[:23]] == list(cc.ARRAYS)
    assert engine.CLEARANCE_CHUNK == cc.CHUNK
    declared = set(re.findall(r"\b(csf_\w+)\s*\(", header))
    for s in ("csf_clearance", "csf_batch_clearance", "csf_clearance_launches"):
        assert s in _ffi.SYMBOLS and s in declared, s


class NoDevice:
    """stands where the library would: any call through it is the device call that must not happen"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was reached: an argument check let the call through")


def bare_engine():
    e = object.__new__(engine.Engine)
    e._lib, e._h = NoDevice(), None
    return e


ROAD = ([0, 2], [(0.0, 0.0), (4.0, 0.0)])


class Edge:
    def __init__(self, v):
        self.vertices = v

    def edges(self):
        return [self]


@pytest.mark.parametrize("kw", [
    dict(first=None, count=None), dict(first=0, count=None), dict(first=-1, count=1), dict(first=0, count=-1), dict(first=0.5, count=4),
    dict(first=0, count=4.5), dict(first=0, count=65536), dict(first="0", count=4),
    dict(first=0, count=4, road=None), dict(first=0, count=4, road=[]), dict(first=0, count=4, road="kerb"), dict(first=0, count=4, road=([0], np.zeros((0, 2)))),
    dict(first=0, count=4, road=([0, 1], [(0.0, 0.0)])),                                       # a polyline of one vertex
    dict(first=0, count=4, road=([0, 2, 3], [(0.0, 0.0), (1.0, 0.0), (2.0, 0.0)])),            # ... as the second
    dict(first=0, count=4, road=([0, 3, 2, 5], np.arange(10.0).reshape(5, 2))),                # offsets that fall
    dict(first=0, count=4, road=([1, 3], [(0.0, 0.0), (1.0, 0.0), (2.0, 0.0)])),               # offsets that do not start at 0
    dict(first=0, count=4, road=([0, 2], [(0.0, 0.0), (1.0, 0.0), (2.0, 0.0)])),               # ... or end at V
    dict(first=0, count=4, road=([0.0, 2.0], [(0.0, 0.0), (1.0, 0.0)])),                       # ... or are not whole numbers
    dict(first=0, count=4, road=([0, 2], [(0.0, 0.0, 1.0), (1.0, 0.0, 1.0)])),
    dict(first=0, count=4, road=([0, 2], [(0.0, NAN), (1.0, 0.0)])), dict(first=0, count=4, road=([0, 2], [(0.0, 0.0), (INF, 0.0)])),
    dict(first=0, count=4, road=([0, 3], [(0.0, 0.0), (1.0, 0.0), (1.0, 0.0)])),               # a segment of no length
    dict(first=0, count=4, road=([0, 2], [(0.0, 0.0), (1e200, 0.0)])),                         # dd overflows
    dict(first=0, count=4, road=[Edge([(0.0, 0.0)])]), dict(first=0, count=4, road=[Edge([(0.0, 0.0), (0.0, 0.0)])]),
    dict(first=0, count=4, road=([0, (1 << 20) + 2], np.zeros(((1 << 20) + 2, 2)))),           # more than 2^20 segments
    dict(first=0, count=4, road=ROAD, d_event=-1.0), dict(first=0, count=4, road=ROAD, d_event=NAN), dict(first=0, count=4, road=ROAD, d_event=INF),
    dict(first=0, count=4, road=ROAD, d_event="near"), dict(first=0, count=4, road=ROAD, d_event=None),
])
def test_python_argument_checks_raise_before_any_device_call(kw):
    e = bare_engine()
    kw = dict(kw)
    kw.setdefault("road", ROAD)
    with pytest.raises((ValueError, TypeError)):
        e.clearance(**kw)
    shared = {k: v for k, v in kw.items() if k not in ("first", "count")}
    if "road" in shared and (shared["road"] is not ROAD or "d_event" in shared):
        with pytest.raises((ValueError, TypeError)):
            engine.Engine.batch_clearance([e], 4, **shared)


def test_batch_argument_checks():
    e = bare_engine()
    for n_last in (-1, 1.5, 65536, None):
        with pytest.raises((ValueError, TypeError)):
            engine.Engine.batch_clearance([e], n_last, ROAD)
    with pytest.raises(ValueError):
        engine.Engine.batch_clearance([], 4, ROAD)               # no engines
    with pytest.raises(TypeError):
        engine.Engine.batch_clearance([object()], 4, ROAD)


def test_the_road_as_elements_or_as_a_pair():
    from cyclistsocialforce_amd.intersection import RoadEdge, RoadSegmentCollection, StraightRoadSegment, flatten_road_elements
    seg = StraightRoadSegment((0.0, 0.0, 0.0), 2.0, 1.0, ds=0.25)
    col = RoadSegmentCollection([seg])
    lone = RoadEdge([(0.0, 5.0), (1.0, 5.0), (2.0, 6.0)])
    off, xy = engine._clearance_road("clearance", [col, lone])
    want = flatten_road_elements([col, lone])
    assert off.dtype == np.int64 and np.array_equal(off, want[0]) and np.array_equal(xy, want[1]) and off.tolist() == [0, 5, 10, 13]
    again = engine._clearance_road("clearance", (off, xy))
    assert np.array_equal(again[0], off) and np.array_equal(again[1], xy)
    assert np.array_equal(engine._clearance_road("clearance", lone)[1], lone.vertices)     # (a lone element)
    # the step between two polylines is no segment: the first may end where the second starts
    off, xy = engine._clearance_road("clearance", ([0, 2, 4], [(0.0, 0.0), (1.0, 0.0), (1.0, 0.0), (2.0, 0.0)]))
    assert off.tolist() == [0, 2, 4]


def test_the_pack_of_output_arrays():
    off, xy = engine._clearance_road("clearance", ROAD)
    pack = engine._ClearancePack([(3, 4), (0, 4), (5, 1)], off, xy, [7, 0, 2], True)
    o, y = pack.outs, pack.road
    assert y.n_edges == 1 and y.offsets == off.ctypes.data and y.xy == xy.ctypes.data
    assert o[0].event_capacity == 7 and o[1].event_capacity == 0 and not o[1].events and o[2].events - o[0].events == 7 * 40
    assert o[1].d - o[0].d == 12 * 8 and o[2].d == o[1].d and o[1].edge - o[0].edge == 12 * 4 and o[1].left - o[0].left == 9 * 8
    assert o[1].cross - o[0].cross == 9 * 4 and o[1].d_min - o[0].d_min == 3 * 8 and o[1].cross_n - o[0].cross_n == 3 * 4
    assert o[1].near_count - o[0].near_count == 4 * 4 and o[2].near_count - o[1].near_count == 4 * 4 and o[1].cross_count - o[0].cross_count == 3 * 4
    assert len({getattr(o[0], f) for f, _ in _ffi.ClearanceOut._fields_[:24]}) == 24           # 23 arrays and the events: all apart
    r = pack.result(0, True, 0.2, 0.5)
    assert r.d.shape == (4, 3) and r.seg.dtype == np.int32 and r.left.shape == (3, 3) and r.cross.shape == (3, 3) and r.d_min.shape == (3,)
    assert r.near_count.shape == (4,) and r.cross_count.shape == (3,) and r.events.dtype == engine.CLEARANCE_EVENT_DTYPE
    assert r.period == 0.2 and r.d_event == 0.5 and r.ids is None and r.offsets.tolist() == [0, 2]
    last = pack.result(2, False, None, 0.5)
    assert last.d.shape == (1, 5) and last.left.shape == (0, 5) and last.cross_count.shape == (0,) and last.events is None
    bare = engine._ClearancePack([(3, 4)], off, xy, [0], False)                                # per_sample=False: no per-cell pointer
    b = bare.result(0, False, None, 0.0)
    assert b.d is None and b.left is None and b.cross is None and b.d_min.shape == (3,) and b.near_count.shape == (4,)
    assert not bare.outs[0].d and not bare.outs[0].cross and bare.outs[0].d_min and bare.outs[0].near_count


# ---- the reference against hand-computed cases: every number below is dyadic, so every operation is exact ----------------------------
ONE = cc.pack([(0.0, 0.0), (4.0, 0.0)])


def at(*points):
    """one sample of road users standing at the points"""
    return cc.states(*[[p] for p in points])


def test_a_point_abeam_of_a_segment_and_beyond_each_end():
    ref = cc.reference(at((1.0, 2.0), (-3.0, 4.0), (7.0, 4.0), (2.0, NAN)), ONE, d_event=4.0)
    assert ref.d[0, :3].tolist() == [2.0, 5.0, 5.0] and np.isnan(ref.d[0, 3])
    assert ref.t[0, :3].tolist() == [0.25, 0.0, 1.0] and np.isnan(ref.t[0, 3])
    assert ref.edge[0].tolist() == [0, 0, 0, -1] and ref.seg[0].tolist() == [0, 0, 0, -1]
    assert ref.d_min.tolist() == [2.0, 5.0, 5.0, INF] and ref.d_min_k.tolist() == [0, 0, 0, -1] and ref.d_min_seg.tolist() == [0, 0, 0, -1]
    assert ref.near_samples.tolist() == [1, 0, 0, 0] and ref.near_first.tolist() == [0, -1, -1, -1] and ref.near_count.tolist() == [1]
    assert ref.left.shape == (0, 4) and ref.cross_count.shape == (0,) and ref.n_exist == 3
    assert cc.reference(at((1.0, 2.0)), ONE, d_event=2.0).near_samples.tolist() == [0]         # d < d_event, strictly
    assert cc.reference(at((1.0, 2.0)), ONE, d_event=0.0).near_samples.tolist() == [0]


def test_a_point_equidistant_from_two_segments_takes_the_lower():
    lo, hi = [(0.0, -1.0), (4.0, -1.0)], [(0.0, 1.0), (4.0, 1.0)]
    for first, second in ((lo, hi), (hi, lo)):
        ref = cc.reference(at((2.0, 0.0)), cc.pack(first, second))
        assert ref.d[0, 0] == 1.0 and ref.edge[0, 0] == 0 and ref.seg[0, 0] == 0 and ref.t[0, 0] == 0.5
    bent = cc.pack([(0.0, 0.0), (4.0, 0.0), (4.0, 4.0)])         # a point on the shared vertex: d = 0 on both, t = 1 of the first
    ref = cc.reference(at((4.0, 0.0), (6.0, -2.0)), bent)
    assert ref.d[0].tolist() == [0.0, 8.0 ** 0.5] and ref.seg[0].tolist() == [0, 0] and ref.t[0].tolist() == [1.0, 1.0]
    assert 8.0 ** 0.5 == np.sqrt(8.0)


def test_left_and_right_of_the_direction_of_travel():
    kerbs = cc.pack([(0.0, 2.0), (4.0, 2.0)], [(0.0, -1.0), (4.0, -1.0)])
    east = cc.states(cc.line((1.0, 0.0), (1.0, 0.0), 3))
    ref = cc.reference(east, kerbs)
    assert ref.left[:, 0].tolist() == [2.0, 2.0] and ref.right[:, 0].tolist() == [1.0, 1.0]
    assert ref.left_edge[:, 0].tolist() == [0, 0] and ref.right_edge[:, 0].tolist() == [1, 1]
    assert ref.left_min.tolist() == [2.0] and ref.left_min_k.tolist() == [0] and ref.right_min.tolist() == [1.0] and ref.right_min_k.tolist() == [0]
    west = cc.reference(east[::-1], kerbs)                       # ridden backwards, the sides swap
    assert west.left[:, 0].tolist() == [1.0, 1.0] and west.right_edge[:, 0].tolist() == [0, 0]
    still = cc.reference(cc.states(cc.line((1.0, 0.0), (0.0, 0.0), 3)), kerbs)                 # z == 0: neither side
    assert np.isinf(still.left).all() and np.isinf(still.right).all() and (still.left_edge == -1).all() and (still.right_edge == -1).all()
    assert still.left_min.tolist() == [INF] and still.left_min_k.tolist() == [-1] and still.d[:, 0].tolist() == [1.0, 1.0, 1.0]
    outside = cc.reference(cc.states(cc.line((1.0, 3.0), (1.0, 0.0), 2)), kerbs)               # both kerbs on the right: the nearer one
    assert outside.left[0, 0] == INF and outside.right[0, 0] == 1.0 and outside.right_edge[0, 0] == 0 and outside.left_edge[0, 0] == -1
    gone = east.copy()
    gone[2, 0, 0] = NAN                                          # the last sample is missing: station 1 does not exist
    ref = cc.reference(gone, kerbs)
    assert ref.left[0, 0] == 2.0 and np.isnan(ref.left[1, 0]) and np.isnan(ref.right[1, 0]) and ref.left_edge[1, 0] == -1 and ref.cross[1, 0] == 0
    ahead = cc.reference(cc.states(cc.line((-2.0, 0.0), (1.0, 0.0), 2)), ONE)                  # straight ahead: neither side
    assert ahead.left[0, 0] == INF and ahead.right[0, 0] == INF and ahead.d[0, 0] == 2.0


def only(ref):
    assert len(ref.crossings) == 1
    e = ref.crossings[0]
    return tuple(int(e[f]) for f in ("i", "k", "edge", "seg", "dir")) + (float(e["t"]), float(e["u"]))


def test_a_station_that_crosses_a_segment():
    north = cc.states(cc.line((1.0, -3.0), (0.0, 2.0), 4))       # y = -3, -1, 1, 3 at x = 1
    ref = cc.reference(north, ONE)
    assert only(ref) == (0, 1, 0, 0, -1, 1.5, 0.25)               # from the right of A -> B
    assert ref.cross[:, 0].tolist() == [0, 1, 0] and ref.cross_n.tolist() == [1] and ref.cross_count.tolist() == [0, 1, 0]
    back = cc.reference(north[::-1], ONE)
    assert only(back) == (0, 1, 0, 0, 1, 1.5, 0.25)
    beyond = cc.reference(cc.states(cc.line((6.0, -3.0), (0.0, 2.0), 4)), ONE)                 # u = 1.5: the sign changes, no crossing
    assert len(beyond.crossings) == 0 and beyond.sign_changes == 1 and beyond.refused == 1 and beyond.cross_n.tolist() == [0]
    ends = cc.reference(cc.states(cc.line((4.0, -3.0), (0.0, 2.0), 4), cc.line((0.0, -3.0), (0.0, 2.0), 4)), ONE)   # u = 1 and u = 0: crossings
    assert [float(e["u"]) for e in ends.crossings] == [1.0, 0.0] and ends.cross_n.tolist() == [1, 1] and ends.cross_count.tolist() == [0, 2, 0]


def test_a_path_through_a_shared_vertex_counts_on_both_segments():
    two = cc.pack([(0.0, 0.0), (4.0, 0.0), (8.0, 0.0)])
    ref = cc.reference(cc.states(cc.line((4.0, -1.0), (0.0, 2.0), 2)), two)
    assert [(int(e["seg"]), float(e["u"]), float(e["t"])) for e in ref.crossings] == [(0, 1.0, 0.5), (1, 0.0, 0.5)]
    assert ref.cross[0, 0] == 2 and ref.cross_n.tolist() == [2]


def test_small_calls():
    for S in (np.zeros((0, 3, 5)), np.zeros((1, 3, 5)), np.zeros((4, 0, 5)), np.zeros((4, 1, 5))):
        c, n = S.shape[:2]
        ref = cc.reference(S, cc.road(8.0, 7), d_event=1.0)
        assert ref.d.shape == (c, n) and ref.left.shape == (max(c - 1, 0), n) and ref.d_min.shape == (n,) and ref.near_count.shape == (c,)
        assert ref.cross_count.shape == (max(c - 1, 0),) and len(ref.crossings) == 0
    off, xy = cc.road(8.0, 7)
    assert off.tolist() == [0, 3, 6, 9, 11] and len(cc.segments(off, xy)[0]) == 7
    assert len(cc.segments(*cc.road(8.0, 1))[0]) == 1 and len(cc.segments(*cc.road(8.0, 513))[0]) == 513
    ax, ay, bx, by, edge_of, seg_in = cc.segments(*cc.mirrored())
    assert len(ax) == 1281 and edge_of[416] == 0 and edge_of[640 + 416] == 1 and seg_in[640 + 416] == 416 and ax[416] == 0.0 and ay[640] == 2.0


# ---- the helpers of engine.Clearance on a hand-made result --------------------------------------------------------------------------
def hand_made():
    r = engine.Clearance()
    for f in engine.Clearance.__slots__:
        setattr(r, f, None)
    r.offsets = np.array([0, 3, 6])
    r.left = np.array([[2.0, INF], [1.0, 3.0], [NAN, 0.5]])
    r.right = np.array([[1.0, 1.0], [3.0, INF], [NAN, 1.5]])
    r.cross = np.array([[0, 1], [1, 0], [0, 2]], np.int32)
    r.edge = np.array([[0, 1], [0, 1], [1, 1], [-1, 0]], np.int32)
    return r


def test_the_helpers_of_a_clearance():
    r = hand_made()
    lat = r.lateral_position()
    assert lat[0, 0] == 1.0 / 3.0 and lat[1, 0] == 0.75 and lat[2, 1] == 0.75 and np.isnan(lat[0, 1]) and np.isnan(lat[1, 1]) and np.isnan(lat[2, 0])
    w = r.width()
    assert w[0, 0] == 3.0 and w[1, 0] == 4.0 and w[0, 1] == INF and np.isnan(w[2, 0]) and w[2, 1] == 2.0
    assert r.off_road().tolist() == [[False, True], [True, True], [True, True]]
    assert r.nearest_edge_share().tolist() == [3.0 / 7.0, 4.0 / 7.0]
    r.left = r.edge = None
    for f in (r.lateral_position, r.width, r.off_road, r.nearest_edge_share):
        with pytest.raises(ValueError):
            f()
    none = hand_made()
    none.edge[:] = -1
    assert np.isnan(none.nearest_edge_share()).all()
