"""Post-encroachment time (include/csf.h: csf_post_encroachment), the parts that need no GPU: the layout of the two
structs against the header, the Python argument checks, and the NumPy reference of tests/pet_common.py against hand-computed cases."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pet_common as pc
from cyclistsocialforce_amd import _ffi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def test_struct_layouts_equal_the_header(tmp_path):
    """sizeof and every offsetof of csf_pet_event and csf_pet_out: include/csf.h through gcc, the binding's structs, and the NumPy
    dtype the events are returned as"""
    structs = {"csf_pet_event": _ffi.PetEvent, "csf_pet_out": _ffi.PetOut}
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
    assert got["csf_pet_event"]["sizeof"] == 48
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
    for dt in (engine.PET_EVENT_DTYPE, pc.EVENT_DTYPE):
        assert dt.itemsize == ctypes.sizeof(_ffi.PetEvent)
        for f, _ in _ffi.PetEvent._fields_:
            assert dt.fields[f][1] == getattr(_ffi.PetEvent, f).offset, f
    assert {"csf_post_encroachment", "csf_batch_post_encroachment", "csf_pet_launches"} <= set(_ffi.SYMBOLS)


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
    dict(first=0, count=4, pet_event=float("nan")), dict(first=0, count=4, pet_event=-INF), dict(first=0, count=4, pet_event="soon"),
    dict(first=0, count=4, pet_event=[1.0]),
])
def test_python_argument_checks_raise_before_any_device_call(kw):
    e = bare_engine()
    with pytest.raises((ValueError, TypeError)):
        e.post_encroachment(**kw)
    if set(kw) == {"first", "count", "pet_event"}:
        with pytest.raises((ValueError, TypeError)):
            engine.Engine.batch_post_encroachment([e], 4, pet_event=kw["pet_event"])


def test_batch_argument_checks():
    e = bare_engine()
    for n_last in (-1, 1.5, 65536, None):
        with pytest.raises((ValueError, TypeError)):
            engine.Engine.batch_post_encroachment([e], n_last)
    with pytest.raises(ValueError):
        engine.Engine.batch_post_encroachment([], 4)             # no engines
    with pytest.raises(TypeError):
        engine.Engine.batch_post_encroachment([object()], 4)


def test_the_pack_of_output_arrays_and_in_seconds():
    pack = engine._PetPack([(3, 4), (0, 4), (5, 1)], True, [7, 0, 2])
    o = pack.outs
    assert o[0].event_capacity == 7 and o[1].event_capacity == 0 and not o[1].events and o[2].event_capacity == 2
    assert o[2].events - o[0].events == 7 * 48 and o[1].seg_pet - o[0].seg_pet == 9 * 8 and o[1].seg_with - o[0].seg_with == 9 * 4
    assert o[2].run_count - o[0].run_count == 3 * 4 and o[2].run_y - o[0].run_y == 3 * 8
    r = pack.result(0, True, 0.2)
    assert r.seg_pet.shape == (3, 3) and r.seg_with.dtype == np.int32 and r.run_count.dtype == np.int32 and r.run_x.shape == (3,)
    assert r.events.dtype == engine.PET_EVENT_DTYPE and r.period == 0.2 and not r.seconds
    assert pack.result(2, False, None).seg_pet.shape == (0, 5) and pack.result(2, False, None).events is None
    assert engine._PetPack([(3, 4)], False, [0]).result(0, False, None).seg_pet is None
    assert engine._pet_capacity_guess(3) == 64 and engine._pet_capacity_guess(500) == 500 and engine._pet_capacity_guess(10 ** 7) == 65536
    r.seg_pet[:], r.seg_t_own[:], r.seg_t_with[:], r.run_pet[:], r.run_t_own[:], r.run_t_with[:] = 2.0, 1.0, 3.0, 2.0, 1.0, 3.0
    r.run_x[:] = 7.0
    r.events = np.zeros(1, engine.PET_EVENT_DTYPE)
    r.events["t_i"], r.events["t_j"], r.events["x"] = 1.0, 3.0, 7.0
    s = r.in_seconds()
    assert s.seconds and (s.seg_pet == 0.4).all() and (s.run_t_with == 3.0 * 0.2).all() and (s.run_x == 7.0).all()
    assert s.events["t_j"][0] == 3.0 * 0.2 and s.events["x"][0] == 7.0 and r.events["t_j"][0] == 3.0 and s.in_seconds() is s
    with pytest.raises(ValueError):
        pack.result(2, False, None).in_seconds()


# ---- the reference against hand-computed cases: values to rtol 1e-12, counts and partners exact ------------------------------------------
def close(a, b):
    np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)


def test_reference_perpendicular():
    """i from (0, 0) at +5 m per sample along x, j from (12, 20) at -4 m per sample along y: one crossing, at (12, 0)"""
    r = pc.reference(pc.PERPENDICULAR)
    assert list(r.run_count) == [1, 1] and list(r.run_with) == [1, 0]
    close(r.run_t_own, [2.4, 5.0]); close(r.run_t_with, [5.0, 2.4]); close(r.run_pet, [2.6, 2.6])
    close(r.run_x, [12.0, 12.0])
    assert abs(r.run_y[0]) < 1e-12 and abs(r.run_y[1]) < 1e-12
    assert r.run_pet[0] == r.run_pet[1] and r.run_t_own[0] == r.run_t_with[1] and r.run_t_own[1] == r.run_t_with[0]   # the same bits
    assert np.isfinite(r.seg_pet).sum() == 2 and r.seg_pet[2, 0] == r.run_pet[0] and r.seg_pet[5, 1] == r.run_pet[1]
    assert r.seg_with[2, 0] == 1 and r.seg_with[5, 1] == 0 and (np.delete(r.seg_with.ravel(), [4, 11]) == -1).all()
    ev = pc.events(r, INF)
    assert len(ev) == 1 and tuple(ev[["i", "j", "k", "l"]][0]) == (0, 1, 2, 5) and ev["t_i"][0] == r.run_t_own[0] and ev["x"][0] == r.run_x[0]
    assert len(pc.events(r, 2.5)) == 0 and len(pc.events(r, 2.7)) == 1


def test_reference_through_a_shared_vertex():
    """j is at (10, 0) exactly in sample 2, as i is: the half-open intervals count the crossing on exactly one segment of each path"""
    r = pc.reference(pc.SHARED_VERTEX)
    assert list(r.run_count) == [1, 1] and list(r.run_with) == [1, 0]
    assert list(r.run_t_own) == [2.0, 2.0] and list(r.run_t_with) == [2.0, 2.0] and list(r.run_pet) == [0.0, 0.0]
    assert list(r.run_x) == [10.0, 10.0] and list(r.run_y) == [0.0, 0.0]
    assert np.isfinite(r.seg_pet).sum() == 2 and r.seg_pet[2, 0] == 0.0 and r.seg_pet[2, 1] == 0.0


@pytest.mark.parametrize("name", list(pc.NO_CROSSING))
def test_reference_no_crossing(name):
    r = pc.reference(pc.NO_CROSSING[name])
    assert (r.run_count == 0).all() and np.isinf(r.run_pet).all() and (r.run_with == -1).all() and np.isnan(r.run_t_own).all()
    assert np.isinf(r.seg_pet).all() and (r.seg_with == -1).all() and np.isnan(r.seg_t_own).all() and np.isnan(r.seg_t_with).all()
    assert np.isnan(r.run_x).all() and np.isnan(r.run_y).all() and len(pc.events(r, INF)) == 0


def test_reference_a_weave_crosses_twice():
    """j crosses i's path at x = 7.5 (t_j = 0.5, t_i = 1.5: PET 1.0) and at x = 18.5 (t_j = 2.5, t_i = 3.7: PET 1.2)"""
    r = pc.reference(pc.WEAVE)
    assert list(r.run_count) == [2, 2] and list(r.run_with) == [1, 0]
    close(r.run_pet, [1.0, 1.0]); close(r.run_t_own, [1.5, 0.5]); close(r.run_t_with, [0.5, 1.5]); close(r.run_x, [7.5, 7.5])
    close(r.seg_pet[[1, 3], 0], [1.0, 1.2]); close(r.seg_pet[[0, 2], 1], [1.0, 1.2])
    close(r.seg_t_own[3, 0], 3.7); close(r.seg_t_with[3, 0], 2.5)
    assert np.isfinite(r.seg_pet).sum() == 4 and r.seg_pet[1, 0] == r.run_pet[0]      # the smaller PET, with its k
    ev = pc.events(r, INF)
    assert [tuple(e) for e in ev[["i", "j", "k", "l"]]] == [(0, 1, 1, 0), (0, 1, 3, 2)]
    M = pc.pet_matrix(pc.WEAVE)
    assert np.array_equal(M, M.T)


def test_reference_a_rider_with_a_nan_sample():
    """i's x is NaN in sample 2: its segments 1 and 2 do not exist; its crossing on segment 3 stays, the one on segment 1 goes - and
    j's rows change only where those two segments were the partner"""
    whole = pc.reference(pc.WEAVE)
    S = pc.WEAVE.copy()
    S[2, 0, 0] = np.nan
    r = pc.reference(S)
    assert np.isnan(r.seg_pet[[1, 2], 0]).all() and (r.seg_with[[1, 2], 0] == -1).all()
    assert np.isnan(r.seg_t_own[[1, 2], 0]).all() and np.isnan(r.seg_t_with[[1, 2], 0]).all()
    keep = [0, 3, 4, 5, 6]
    for f in ("seg_pet", "seg_with", "seg_t_own", "seg_t_with"):
        assert np.array_equal(getattr(r, f)[keep, 0], getattr(whole, f)[keep, 0], equal_nan=True), f
    assert list(r.run_count) == [1, 1] and r.run_pet[0] == whole.seg_pet[3, 0] and r.run_t_own[0] == whole.seg_t_own[3, 0]
    was_partner = (whole.seg_with[:, 1] == 0) & np.isin(np.floor(whole.seg_t_with[:, 1]), [1, 2])
    assert list(np.nonzero(was_partner)[0]) == [0]
    assert np.isinf(r.seg_pet[0, 1]) and r.seg_with[0, 1] == -1 and np.isnan(r.seg_t_own[0, 1])
    for f in ("seg_pet", "seg_with", "seg_t_own", "seg_t_with"):
        assert np.array_equal(getattr(r, f)[1:, 1], getattr(whole, f)[1:, 1], equal_nan=True), f


def test_reference_ties_and_symmetry_on_random_paths():
    """two partners at the same PET: the lowest j wins, and with one partner twice the lowest l; random paths are bitwise symmetric"""
    twin = pc.line((12.0, 20.0), (0.0, -4.0))
    r = pc.reference(pc.states(pc.I_PATH, twin, twin))
    assert r.run_with[0] == 1 and r.run_count[0] == 2 and r.seg_with[2, 0] == 1
    rng = np.random.default_rng(5)
    S = np.zeros((8, 40, 5))
    S[0, :, :2] = rng.uniform(0, 20, (40, 2))
    S[1:, :, :2] = S[0, :, :2] + np.cumsum(rng.normal(0, 1.5, (7, 40, 2)), axis=0)
    M = pc.pet_matrix(S)
    assert np.isfinite(M).sum() > 40 and np.array_equal(M, M.T)
    ref = pc.reference(S)
    rp, rw, ro, rt, _ = pc.window(ref.seg_pet, ref.seg_with, ref.seg_t_own, ref.seg_t_with)
    assert np.array_equal(ref.run_pet, rp) and np.array_equal(ref.run_with, rw) and int(ref.run_count.sum()) == len(ref.crossings)
    assert len(pc.events(ref, INF)) * 2 == len(ref.crossings)
    assert len(pc.reference(S[:1]).crossings) == 0 and pc.reference(S[:1]).seg_pet.shape == (0, 40)
    assert np.isinf(pc.reference(S[:, :1]).seg_pet).all()
