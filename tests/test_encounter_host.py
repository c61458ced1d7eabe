"""Encounter measures (include/csf.h: csf_encounters), the parts that need no GPU: the layout of the two structs
against the header, the Python argument checks, and the NumPy reference of tests/encounter_common.py against hand-computed cases."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import encounter_common as ec
from cyclistsocialforce_amd import _ffi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layouts_equal_the_header(tmp_path):
    """sizeof and every offsetof of csf_encounter_event and csf_encounter_out: include/csf.h through gcc, the binding's structs, and
    the NumPy dtype the events are returned as"""
    structs = {"csf_encounter_event": _ffi.EncounterEvent, "csf_encounter_out": _ffi.EncounterOut}
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
    import re
    for name, cls in structs.items():
        body = header[header.index("typedef struct %s {" % name):header.index("} %s;" % name)]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        body = body[body.index("{") + 1:]
        declared = [m.strip(" *") for stmt in body.split(";") if stmt.strip() for m in stmt.split(None, 1)[1].split(",")]   # `type a, *b;`
        assert declared == [f for f, _ in cls._fields_], name
    for dt in (engine.EVENT_DTYPE, ec.EVENT_DTYPE):
        assert dt.itemsize == ctypes.sizeof(_ffi.EncounterEvent)
        for f, _ in _ffi.EncounterEvent._fields_:
            assert dt.fields[f][1] == getattr(_ffi.EncounterEvent, f).offset, f
    assert {"csf_encounters", "csf_batch_encounters", "csf_encounter_launches"} <= set(_ffi.SYMBOLS)


class NoDevice:
    """stands where the library would: any call through it is the device call that must not happen"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was reached: an argument check let the call through")


def bare_engine(n=3):
    e = object.__new__(engine.Engine)
    e._lib, e._h = NoDevice(), None
    return e


@pytest.mark.parametrize("kw", [
    dict(radius=-0.1), dict(radius=float("nan")), dict(radius=float("inf")), dict(radius="wide"), dict(radius=None),
    dict(d_event=float("nan")), dict(ttc_event="soon"), dict(ttc_event=float("nan")),
    dict(count=2), dict(first=0), dict(first=-1, count=1), dict(first=0, count=-1), dict(first=0.5, count=1), dict(first=0, count=1.5),
    dict(first=0, count=65536),
])
def test_python_argument_checks_raise_before_any_device_call(kw):
    e = bare_engine()
    with pytest.raises((ValueError, TypeError)):
        e.encounters(**kw)
    if "first" not in kw and "count" not in kw:
        with pytest.raises((ValueError, TypeError)):
            engine.Engine.batch_encounters([e], 4, **kw)


def test_batch_argument_checks():
    e = bare_engine()
    for n_last in (-1, 1.5, 65536, None):
        with pytest.raises((ValueError, TypeError)):
            engine.Engine.batch_encounters([e], n_last)
    with pytest.raises(ValueError):
        engine.Engine.batch_encounters([], 4)                    # no engines
    with pytest.raises(TypeError):
        engine.Engine.batch_encounters([object()], 4)


def test_events_wanted_and_the_pack_of_output_arrays():
    assert not engine._events_wanted(None, None) and not engine._events_wanted(0.0, -1.0)
    assert engine._events_wanted(2.0, None) and engine._events_wanted(None, 1.5)
    pack = engine._EncounterPack([(3, 4), (0, 4), (5, 0)], True, [7, 0, 2])
    o = pack.outs
    assert o[0].event_capacity == 7 and o[1].event_capacity == 0 and not o[1].events and o[2].event_capacity == 2
    assert o[2].events - o[0].events == 7 * 32 and o[1].d_min - o[0].d_min == 12 * 8 and o[1].run_d_with - o[0].run_d_with == 3 * 4
    r = pack.result(0, 0.5, True)
    assert r.d_min.shape == (4, 3) and r.ttc_with.dtype == np.int32 and r.run_d_sample.shape == (3,) and r.events.dtype == engine.EVENT_DTYPE
    r = pack.result(2, 0.5, False)                               # an empty window: nobody, at no sample
    assert r.d_min.shape == (0, 5) and np.isinf(r.run_ttc_min).all() and (r.run_d_with == -1).all() and (r.run_d_sample == -1).all()
    assert r.events is None
    assert engine._EncounterPack([(3, 4)], False, [0]).result(0, 0.5, False).d_min is None


@pytest.mark.parametrize("name,si,sj,radius,d,ttc", ec.KNOWN, ids=[k[0] for k in ec.KNOWN])
def test_reference_against_hand_computed_cases(name, si, sj, radius, d, ttc):
    S = np.array([[si, sj]])
    dm, dj, tm, tj = ec.per_sample(S, radius)
    np.testing.assert_allclose(dm[0], [d, d], rtol=1e-14)
    assert list(dj[0]) == [1, 0]
    if np.isinf(ttc) or ttc == 0.0:
        assert list(tm[0]) == [ttc, ttc]
    else:
        np.testing.assert_allclose(tm[0], [ttc, ttc], rtol=1e-12)
    assert list(tj[0]) == ([-1, -1] if np.isinf(ttc) else [1, 0])
    p = ec.pairs(S, radius)
    assert p.D[0, 0, 1] == p.D[0, 1, 0] and p.T[0, 0, 1] == p.T[0, 1, 0]   # bitwise symmetric


def test_reference_ties_non_finite_riders_and_a_population_of_one():
    # three in a row, 4 m apart: the middle one is equally far from both - the lowest j wins
    S = np.array([[(0.0, 0.0, 0.0, 5.0), (4.0, 0.0, 0.0, 5.0), (8.0, 0.0, 0.0, 5.0)]])
    dm, dj, tm, tj = ec.per_sample(S, 0.5)
    assert list(dm[0]) == [4.0, 4.0, 4.0] and list(dj[0]) == [1, 0, 1] and np.isinf(tm).all() and (tj == -1).all()
    S2 = S.copy()
    S2[0, 1, 2] = np.nan                                        # the middle one drops out: its row NaN / -1, the others find each other
    dm, dj, tm, tj = ec.per_sample(S2, 0.5)
    assert np.isnan(dm[0, 1]) and np.isnan(tm[0, 1]) and dj[0, 1] == -1 and tj[0, 1] == -1
    assert list(dm[0, [0, 2]]) == [8.0, 8.0] and list(dj[0, [0, 2]]) == [2, 0]
    dm, dj, tm, tj = ec.per_sample(S[:, :1], 0.5)
    assert np.isinf(dm[0, 0]) and np.isinf(tm[0, 0]) and dj[0, 0] == -1 and tj[0, 0] == -1
    # the window takes the earliest sample on ties and skips NaN rows
    d = np.array([[3.0, np.nan], [2.0, 5.0], [2.0, 5.0]])
    w = np.array([[1, -1], [1, 0], [1, 0]], dtype=np.int32)
    rd, rw, rs, _, _, _ = ec.window(d, w, d, w, first=10)
    assert list(rd) == [2.0, 5.0] and list(rw) == [1, 0] and list(rs) == [11, 11]
    # events: i < j, either threshold, sorted
    S3 = np.array([[(0.0, 0.0, 0.0, 5.0), (1.5, 0.0, 0.0, 5.0), (21.0, 0.0, np.pi, 5.0)]])
    ev, edge = ec.events(S3, 0.5, 2.0, 2.5, first=7)
    assert [(int(e["sample"]), int(e["i"]), int(e["j"])) for e in ev] == [(7, 0, 1), (7, 0, 2), (7, 1, 2)] and not edge
    assert ev["d"][0] == 1.5 and np.isinf(ev["ttc"][0]) and ev["ttc"][1] == 2.0
    assert len(ec.events(S3, 0.5, 0.0, -1.0, first=7)[0]) == 0
