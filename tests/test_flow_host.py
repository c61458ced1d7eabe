"""Flow (include/csf.h: csf_flow), the parts that need no GPU: the layout of the three structs against the header,
the Python argument checks, the NumPy reference of tests/flow_common.py against hand-computed dyadic cases, and the helpers of
engine.Flow on a hand-made result."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import flow_common as fc
from cyclistsocialforce_amd import _ffi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAN = float("nan")


def test_struct_layouts_equal_the_header(tmp_path):
    """sizeof and every offsetof of csf_flow_layout, csf_flow_event and csf_flow_out: include/csf.h through gcc, the binding's
    structs, and the NumPy dtype the events are returned as"""
    structs = {"csf_flow_layout": _ffi.FlowLayout, "csf_flow_event": _ffi.FlowEvent, "csf_flow_out": _ffi.FlowOut}
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
    assert got["csf_flow_event"]["sizeof"] == 40
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
    for dt in (engine.FLOW_EVENT_DTYPE, fc.EVENT_DTYPE):
        assert dt.itemsize == ctypes.sizeof(_ffi.FlowEvent) == 40
        assert list(dt.names) == [f for f, _ in _ffi.FlowEvent._fields_]
        for f, _ in _ffi.FlowEvent._fields_:
            assert dt.fields[f][1] == getattr(_ffi.FlowEvent, f).offset, f
    # the arrays of a result, in the order of the header's pointers
    assert [f for f, _ in engine.Flow.ARRAYS] == [f for f, _ in _ffi.FlowOut._fields_[:12]] == list(fc.ARRAYS)
    declared = set(re.findall(r"\b(csf_\w+)\s*\(", header))
    for s in ("csf_flow", "csf_batch_flow", "csf_flow_launches"):
        assert s in _ffi.SYMBOLS and s in declared, s


class NoDevice:
    """stands where the library would: any call through it is the device call that must not happen"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was reached: an argument check let the call through")


def bare_engine():
    e = object.__new__(engine.Engine)
    e._lib, e._h = NoDevice(), None
    return e


LINE = [(0.0, 0.0, 1.0, 0.0)]
AREA = [(0.0, 0.0, 1.0, 0.0, 0.5)]


@pytest.mark.parametrize("kw", [
    dict(first=None, count=None), dict(first=0, count=None), dict(first=None, count=4), dict(first=-1, count=1), dict(first=-1, count=4),
    dict(first=0, count=-1), dict(first=0.5, count=4), dict(first=0, count=4.5), dict(first=0, count=65536), dict(first="0", count=4),
    dict(first=0, count=4, lines=[(0.0, 0.0, 1.0)]), dict(first=0, count=4, lines=[(0.0, 0.0, 0.0, 0.0)]), dict(first=0, count=4, lines=[(0.0, NAN, 1.0, 0.0)]),
    dict(first=0, count=4, lines=[(0.0, 0.0, INF, 0.0)]), dict(first=0, count=4, lines=LINE * 65), dict(first=0, count=4, lines="across"),
    dict(first=0, count=4, areas=LINE), dict(first=0, count=4, areas=[(1.0, 1.0, 1.0, 1.0, 0.5)]), dict(first=0, count=4, areas=[(0.0, 0.0, 1.0, 0.0, NAN)]),
    dict(first=0, count=4, areas=[(0.0, 0.0, 1.0, 0.0, -0.5)]), dict(first=0, count=4, areas=[(0.0, 0.0, 1.0, 0.0, INF)]), dict(first=0, count=4, areas=AREA * 65),
    dict(first=0, count=4, areas=[(0.0, 0.0, NAN, 0.0, 0.5)]),
    dict(first=0, count=4, grid=(0.0, 0.0, 1.0, 4)), dict(first=0, count=4, grid=(0.0, 0.0, 0.0, 4, 4)), dict(first=0, count=4, grid=(0.0, 0.0, -1.0, 4, 4)),
    dict(first=0, count=4, grid=(0.0, 0.0, NAN, 4, 4)), dict(first=0, count=4, grid=(0.0, 0.0, INF, 4, 4)), dict(first=0, count=4, grid=(NAN, 0.0, 1.0, 4, 4)),
    dict(first=0, count=4, grid=(0.0, INF, 1.0, 4, 4)), dict(first=0, count=4, grid=(0.0, 0.0, 1.0, 0, 4)), dict(first=0, count=4, grid=(0.0, 0.0, 1.0, 4, 0)),
    dict(first=0, count=4, grid=(0.0, 0.0, 1.0, -4, 4)), dict(first=0, count=4, grid=(0.0, 0.0, 1.0, 4.5, 4)), dict(first=0, count=4, grid=(0.0, 0.0, 1.0, 1025, 1024)),
])
def test_python_argument_checks_raise_before_any_device_call(kw):
    e = bare_engine()
    with pytest.raises((ValueError, TypeError)):
        e.flow(**kw)
    shared = {k: v for k, v in kw.items() if k not in ("first", "count")}
    if shared:
        with pytest.raises((ValueError, TypeError)):
            engine.Engine.batch_flow([e], 4, **shared)


def test_batch_argument_checks():
    e = bare_engine()
    for n_last in (-1, 1.5, 65536, None):
        with pytest.raises((ValueError, TypeError)):
            engine.Engine.batch_flow([e], n_last, lines=LINE)
    with pytest.raises(ValueError):
        engine.Engine.batch_flow([], 4, lines=LINE)              # no engines
    with pytest.raises(TypeError):
        engine.Engine.batch_flow([object()], 4, lines=LINE)


def test_the_pack_of_output_arrays():
    lines, areas, grid = engine._flow_layout("flow", LINE * 2, AREA * 3, (1.0, 2.0, 0.5, 4, 3))
    pack = engine._FlowPack([(3, 4), (0, 4), (5, 1)], lines, areas, grid, [7, 0, 2])
    o, y = pack.outs, pack.layout
    assert (y.n_lines, y.n_areas, y.x0, y.y0, y.h, y.nx, y.ny) == (2, 3, 1.0, 2.0, 0.5, 4, 3) and y.lines == lines.ctypes.data and y.areas == areas.ctypes.data
    assert o[0].event_capacity == 7 and o[1].event_capacity == 0 and not o[1].events and o[2].event_capacity == 2
    assert o[2].events - o[0].events == 7 * 40
    assert o[1].line_count - o[0].line_count == 3 * 2 * 2 * 4 and o[2].line_count - o[1].line_count == 48   # 3 intervals x 2 lines x 2, with or without road users
    assert o[1].cross_n - o[0].cross_n == 3 * 2 * 2 * 4 and o[1].first_t - o[0].first_t == 3 * 2 * 8 and o[1].first_dir - o[0].first_dir == 3 * 2 * 4
    assert o[1].occupancy - o[0].occupancy == 4 * 3 * 4 and o[2].occupancy - o[1].occupancy == 4 * 3 * 4
    assert o[1].in_samples - o[0].in_samples == 3 * 3 * 4 and o[1].in_dist - o[0].in_dist == 3 * 3 * 8 and o[2].in_last == o[1].in_last
    assert o[1].grid_count - o[0].grid_count == 12 * 4 and o[2].grid_count - o[1].grid_count == 12 * 4
    assert len({getattr(o[0], f) for f, _ in _ffi.FlowOut._fields_[:13]}) == 13               # 12 arrays and the events: all apart
    r = pack.result(0, True, 0.2)
    assert r.line_count.shape == (3, 2, 2) and r.cross_n.shape == (3, 2, 2) and r.first_t.shape == (3, 2) and r.first_dir.dtype == np.int32
    assert r.occupancy.shape == (4, 3) and r.in_dist.shape == (3, 3) and r.in_dist.dtype == np.float64 and r.grid_count.shape == (3, 4)
    assert r.events.dtype == engine.FLOW_EVENT_DTYPE and r.period == 0.2 and r.ids is None and r.grid == (1.0, 2.0, 0.5, 4, 3)
    last = pack.result(2, False, None)
    assert last.line_count.shape == (0, 2, 2) and last.occupancy.shape == (1, 3) and last.events is None and last.cross_n.shape == (5, 2, 2)
    bare = engine._FlowPack([(3, 4)], *engine._flow_layout("flow", None, None, None), [0])
    b = bare.result(0, False, None)
    assert b.line_count.shape == (3, 0, 2) and b.occupancy.shape == (4, 0) and b.grid_count is None and bare.layout.nx == 0 and not bare.layout.lines


# ---- the reference against hand-computed cases: every number below is dyadic, so every operation is exact ----------------------------
ACROSS = [(2.5, 0.0, 2.5, 1.0)]                                  # the left of A -> B is x < 2.5


def only(ref):
    assert len(ref.crossings) == 1
    e = ref.crossings[0]
    return int(e["i"]), int(e["l"]), int(e["k"]), int(e["dir"]), float(e["t"]), float(e["u"]), float(e["speed"])


def test_a_rider_across_a_line():
    S = fc.states(fc.line((0.0, 0.5), (1.0, 0.0), 6))
    ref = fc.reference(S, ACROSS)
    assert only(ref) == (0, 0, 2, 1, 2.5, 0.5, 1.0)
    assert ref.line_count.shape == (5, 1, 2) and ref.line_count[2, 0].tolist() == [1, 0] and ref.line_count.sum() == 1
    assert ref.cross_n[0, 0].tolist() == [1, 0] and ref.first_t[0, 0] == 2.5 and ref.first_u[0, 0] == 0.5
    assert ref.first_speed[0, 0] == 1.0 and ref.first_dir[0, 0] == 1
    back = fc.reference(S[::-1], ACROSS)                         # the same path ridden backwards: from the right, in interval 2
    assert only(back) == (0, 0, 2, -1, 2.5, 0.5, 1.0) and back.line_count[2, 0].tolist() == [0, 1]
    two = fc.reference(fc.states(fc.line((0.0, 0.5), (2.0, 0.0), 4), fc.line((0.0, 0.25), (0.0, 0.0), 4)), ACROSS)   # twice as fast; one stands
    assert only(two) == (0, 0, 1, 1, 1.25, 0.5, 2.0)
    assert np.isinf(two.first_t[1, 0]) and np.isnan(two.first_u[1, 0]) and np.isnan(two.first_speed[1, 0]) and two.first_dir[1, 0] == 0


def test_a_step_that_ends_exactly_on_the_line():
    """a point on the line counts as on the right: coming from the left the crossing is in the interval that ends there, coming
    from the right in the interval that starts there"""
    on = [(2.0, 0.0, 2.0, 1.0)]
    left = fc.reference(fc.states(fc.line((0.0, 0.5), (1.0, 0.0), 5)), on)
    assert only(left) == (0, 0, 1, 1, 2.0, 0.5, 1.0)
    right = fc.reference(fc.states(fc.line((4.0, 0.5), (-1.0, 0.0), 5)), on)
    assert only(right) == (0, 0, 2, -1, 2.0, 0.5, 1.0)


def test_touch_and_return_crosses_twice():
    on = [(2.0, 0.0, 2.0, 1.0)]
    S = fc.states([(0.0, 0.5), (1.0, 0.5), (2.0, 0.5), (1.0, 0.5), (0.0, 0.5)])
    ref = fc.reference(S, on)
    assert [(int(e["k"]), int(e["dir"]), float(e["t"])) for e in ref.crossings] == [(1, 1, 2.0), (2, -1, 2.0)]
    assert ref.cross_n[0, 0].tolist() == [1, 1] and ref.first_dir[0, 0] == 1 and ref.first_t[0, 0] == 2.0
    assert ref.line_count[:, 0].tolist() == [[0, 0], [1, 0], [0, 1], [0, 0]]
    # for the reversed line the rider stays on the right throughout (the touched point counts as right): no crossing
    assert len(fc.reference(S, [(2.0, 1.0, 2.0, 0.0)]).crossings) == 0


def test_a_sign_change_beyond_the_lines_end_is_no_crossing():
    S = fc.states(fc.line((0.0, 1.5), (1.0, 0.0), 6), fc.line((0.0, -0.25), (1.0, 0.0), 6), fc.line((0.0, 1.0), (1.0, 0.0), 6), fc.line((0.0, 0.0), (1.0, 0.0), 6))
    ref = fc.reference(S, ACROSS)                                # u = 1.5, -0.25: refused; u = 1 and u = 0, the ends themselves: crossings
    assert ref.sign_changes[0] == 4 and ref.refused[0] == 2
    assert [(int(e["i"]), float(e["u"])) for e in ref.crossings] == [(2, 1.0), (3, 0.0)]
    assert ref.cross_n[:, 0, 0].tolist() == [0, 0, 1, 1] and ref.line_count.sum() == 2


def test_reversing_a_line_swaps_the_direction_columns():
    rev = lambda q: [(bx, by, ax, ay) for ax, ay, bx, by in q]   # noqa: E731
    S = fc.states(fc.line((0.0, 0.5), (1.0, 0.0), 6), fc.line((5.0, 0.25), (-1.0, 0.0), 6), fc.line((0.0, 1.5), (1.0, 0.0), 6))
    a, b = fc.reference(S, ACROSS), fc.reference(S, rev(ACROSS))
    assert a.line_count.sum() == 2 and a.cross_n[:, 0].tolist() == [[1, 0], [0, 1], [0, 0]]
    assert np.array_equal(a.line_count, b.line_count[:, :, ::-1]) and np.array_equal(a.cross_n, b.cross_n[:, :, ::-1])
    assert np.array_equal(a.first_dir, b.first_dir - 2 * b.first_dir) and np.array_equal(a.first_t, b.first_t) and np.array_equal(a.first_speed, b.first_speed, equal_nan=True)
    assert np.array_equal(a.first_u, 1.0 - b.first_u, equal_nan=True)
    # a step that ends on the line: the point belongs to the other side of the reversed line, so the crossing moves one interval on,
    # and the road user's counts swap
    on = [(2.0, 0.0, 2.0, 1.0)]
    S = fc.states(fc.line((0.0, 0.5), (1.0, 0.0), 5))
    a, b = fc.reference(S, on), fc.reference(S, rev(on))
    assert a.cross_n[0, 0].tolist() == [1, 0] and b.cross_n[0, 0].tolist() == [0, 1] and only(a)[2] == 1 and only(b)[2] == 2


def test_a_rider_on_the_edge_of_an_area_is_inside():
    area = [(0.0, 0.0, 4.0, 0.0, 1.0)]                           # dd = 16, ld = 4, half_width * ld = 4
    S = fc.states([(4.0, 1.0)], [(4.0, -1.0)], [(0.0, 0.0)], [(4.5, 0.0)], [(4.0, 1.25)], [(-0.5, 0.0)], [(2.0, NAN)])
    ref = fc.reference(S, areas=area)
    assert ref.in_samples[:, 0].tolist() == [1, 1, 1, 0, 0, 0, 0] and ref.occupancy.tolist() == [[3]]
    assert ref.in_first[:, 0].tolist() == [0, 0, 0, -1, -1, -1, -1] and ref.in_last[:, 0].tolist() == [0, 0, 0, -1, -1, -1, -1]
    assert (ref.in_dist == 0.0).all() and ref.line_count.shape == (0, 0, 2) and ref.n_exist == 6


def test_a_tilted_area():
    area = [(0.0, 0.0, 3.0, 4.0, 1.0)]                           # dd = 25, ld = 5, half_width * ld = 5
    pts = [(1.0, 3.0), (1.0, 3.25), (3.0, 4.0), (2.0, 1.0), (2.25, 1.0), (3.75, 5.0), (-0.25, 0.0), (1.5, 2.0)]
    #      cr = 5: edge   5.75: out   g = 25, end   cr = -5: edge  -6: out     g = 31.25: out  g < 0: out  the centre line
    ref = fc.reference(fc.states(*[[p] for p in pts]), areas=area)
    assert ref.in_samples[:, 0].tolist() == [1, 0, 1, 1, 0, 0, 0, 1] and ref.occupancy.tolist() == [[4]]


def test_in_dist_of_a_rider_that_enters_and_leaves():
    xs = [0.0, 1.0, 2.0, 2.5, 3.5, 5.5, 6.0]                     # stations of 1, 1, 0.5, 1, 2, 0.5 m
    S = fc.states([(x, 0.0) for x in xs])
    ref = fc.reference(S, areas=[(1.5, 0.0, 4.5, 0.0, 0.5)])
    assert ref.occupancy[:, 0].tolist() == [0, 0, 1, 1, 1, 0, 0]
    assert (ref.in_samples[0, 0], ref.in_first[0, 0], ref.in_last[0, 0]) == (3, 2, 4)
    assert ref.in_dist[0, 0] == 3.5                              # the stations that START inside: 0.5 + 1 + 2
    S[5, 0, 0] = NAN                                             # the sample after the last one inside is missing: station 4 does not exist
    assert fc.reference(S, areas=[(1.5, 0.0, 4.5, 0.0, 0.5)]).in_dist[0, 0] == 1.5
    assert fc.reference(S[:5], areas=[(1.5, 0.0, 4.5, 0.0, 0.5)]).in_dist[0, 0] == 1.5   # ... or is outside the call


def test_the_edges_of_the_grid():
    grid = (1.0, 2.0, 0.5, 4, 2)                                 # x in [1, 3), y in [2, 3)
    pts = [(1.0, 2.0), (3.0, 2.0), (2.75, 2.75), (1.0, 3.0), (0.75, 2.0), (1.0, 1.75), (NAN, 2.0)]
    ref = fc.reference(fc.states(*[[p] for p in pts]), grid=grid)
    want = np.zeros((2, 4), np.int32)
    want[0, 0], want[1, 3] = 1, 1
    assert np.array_equal(ref.grid_count, want) and ref.n_outside == 4 and ref.n_exist == 6
    assert fc.reference(fc.states(*[[p] for p in pts])).grid_count is None


def test_small_calls():
    lines, areas, grid = fc.layout(8.0)
    for S in (np.zeros((0, 3, 5)), np.zeros((1, 3, 5)), np.zeros((4, 0, 5)), np.zeros((4, 1, 5))):
        c, n = S.shape[:2]
        ref = fc.reference(S, lines, areas, grid)
        assert ref.line_count.shape == (max(c - 1, 0), 5, 2) and ref.occupancy.shape == (c, 3) and ref.cross_n.shape == (n, 5, 2)
        assert ref.line_count.sum() == 0 and ref.grid_count.sum() + ref.n_outside == c * n == ref.n_exist
        bare = fc.reference(S)
        assert bare.line_count.shape == (max(c - 1, 0), 0, 2) and bare.in_dist.shape == (n, 0) and bare.grid_count is None and bare.n_outside == 0


# ---- the helpers of engine.Flow on a hand-made result ----------------------------------------------------------------------------------
def hand_made():
    r = engine.Flow()
    for f in engine.Flow.__slots__:
        setattr(r, f, None)
    r.lines = np.array([(0.0, 0.0, 0.0, 4.0), (10.0, 0.0, 10.0, 4.0)])
    r.areas = np.array([(0.0, 2.0, 10.0, 2.0, 2.0)])             # 10 m x 4 m
    r.line_count = np.zeros((4, 2, 2), np.int32)
    r.line_count[0, 0, 0], r.line_count[1, 0, 0], r.line_count[3, 0, 1] = 1, 2, 1
    r.line_count[2, 1, 0], r.line_count[3, 1, 0] = 1, 1
    r.first_t = np.array([[0.5, 2.5], [1.25, 3.75], [1.5, INF], [INF, INF]])
    ev = np.zeros(4, engine.FLOW_EVENT_DTYPE)
    ev["l"], ev["t"], ev["speed"] = [0, 0, 0, 1], [1.5, 0.5, 1.25, 2.5], [1.0, 2.0, 4.0, 8.0]
    r.events, r.n_events = ev, 4
    r.occupancy = np.array([[0], [2], [4], [2], [0]], np.int32)
    r.in_samples = np.array([[3], [4], [1], [0]], np.int32)
    r.in_dist = np.array([[6.0], [8.0], [2.0], [0.0]])
    return r


def test_the_helpers_of_a_flow():
    r, dt = hand_made(), 0.5
    assert r.flow(0, dt).tolist() == [1.5, 0.5] and r.flow(1, dt).tolist() == [1.0, 0.0]                    # 3 and 1 crossings in 2 s
    assert r.cumulative(0).tolist() == [[1, 0], [3, 0], [3, 0], [3, 1]] and r.cumulative(1)[:, 0].tolist() == [0, 0, 1, 2]
    tt = r.travel_time(0, 1, dt)
    assert tt[:2].tolist() == [1.0, 1.25] and np.isnan(tt[2:]).all()
    mean, harmonic = r.speeds(0, dt)                             # 2, 4 and 8 m/s
    assert mean == pytest.approx(14.0 / 3.0) and harmonic == pytest.approx(3.0 / (0.5 + 0.25 + 0.125))
    assert r.speeds(1, dt) == (16.0, 16.0)
    assert r.headways(0, dt).tolist() == [0.375, 0.125] and r.headways(1, dt).size == 0
    assert r.density(0).tolist() == [0.0, 0.05, 0.1, 0.05, 0.0]
    q, k, v = r.edie(0, dt)                                      # 16 m and 8 x 0.5 s over 40 m^2 x 2.5 s
    assert q == pytest.approx(0.16) and k == pytest.approx(0.04) and v == pytest.approx(4.0)
    r.events = None
    with pytest.raises(ValueError):
        r.speeds(0, dt)
    with pytest.raises(ValueError):
        r.headways(0, dt)
    empty = hand_made()
    empty.events = empty.events[:0]
    assert all(math.isnan(x) for x in empty.speeds(0, dt))
    empty.in_samples[:], empty.in_dist[:] = 0, 0.0
    assert empty.edie(0, dt)[:2] == (0.0, 0.0) and math.isnan(empty.edie(0, dt)[2])
