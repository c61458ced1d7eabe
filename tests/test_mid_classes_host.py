"""The one-launch tick of mid-size populations of several sets and classes, host side (no GPU): both entry points declared,
exported and bound with the right signatures, NULL refused without a device; Engine.mid_classes / mid_classes_ticks and the mirror's
set_mid_classes forward (fake engines); the recorded resource figures; and - with the CPU oracle - that the seeds of
tests/test_gpu_mid_classes.py's populations are finite and not chaotic over a window."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cyclistsocialforce_amd import _ffi, intersection
from cyclistsocialforce_amd.engine import Engine
from mid_classes_common import ALL_CASES, POS_TOL, WINDOW, oracle_population, population, ulp32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "csf.h")).read()
    declared = set(re.findall(r"\b(csf_[a-z_0-9]+)\s*\(", header))
    lib = _ffi.load()                                                # (the gfx950 library is built and loads)
    for name in ("csf_mid_classes", "csf_mid_classes_ticks"):
        assert name in declared and name in _ffi.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"int csf_mid_classes\(csf_engine \*e, int32_t on\);", header)
    assert re.search(r"int csf_mid_classes_ticks\(const csf_engine \*e, int64_t \*n_ticks\);", header)
    assert lib.csf_mid_classes.restype in (C.c_int, C.c_int32) and lib.csf_mid_classes_ticks.restype in (C.c_int, C.c_int32)
    assert lib.csf_mid_classes.argtypes == [C.c_void_p, C.c_int32]
    assert lib.csf_mid_classes_ticks.argtypes == [C.c_void_p, C.POINTER(C.c_int64)]
    for on in (0, 1, 2):
        assert lib.csf_mid_classes(None, on) == -1                   # (CSF_E_ARG: no engine)
    n = C.c_int64(7)
    assert lib.csf_mid_classes_ticks(None, C.byref(n)) == -1 and n.value == 7
    assert lib.csf_mid_classes_ticks(None, None) == -1
    assert lib.csf_abi_version() == _ffi.ABI_VERSION                 # (the library and the binding agree: this change moves neither)
    src = open(os.path.join(ROOT, "cyclistsocialforce_amd", "_ffi.py")).read()
    assert 'if hasattr(L, "csf_mid_classes"):' in src                # (bound where the library exports it)


class FakeLib:
    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def csf_mid_classes(self, h, on):
        self.calls.append((h, on))
        return self.rc

    def csf_mid_classes_ticks(self, h, ref):
        ref._obj.value = 43
        return self.rc

    def csf_last_error(self, h):
        return b"csf_mid_classes: refused"

    def csf_destroy(self, h):
        pass


def test_engine_mid_classes_forwards():
    e = Engine.__new__(Engine)
    e._lib, e._h = FakeLib(), "handle"
    e.mid_classes()
    e.mid_classes(False)
    e.mid_classes(on=True)
    assert e._lib.calls == [("handle", 1), ("handle", 0), ("handle", 1)]
    assert e.mid_classes_ticks() == 43
    e._lib = FakeLib(rc=-4)
    try:
        e.mid_classes()
        raise AssertionError("a refused call raises")
    except _ffi.EngineError as err:
        assert "-4" in str(err) and "csf_mid_classes" in str(err)
    e._h = None


class FakeEngine:
    made = []

    def __init__(self, pod, capacity, device=0):
        self.calls, self.ns = [], 5
        FakeEngine.made.append(self)

    def mid_classes(self, on=True):
        self.calls.append(on)


class FakeVehicle:
    N_STATES = 5

    def _pod(self, rule):
        return b"pod"


def test_the_mirrors_method_forwards_now_or_when_the_engine_is_made(monkeypatch):
    import inspect
    sig = inspect.signature(intersection.SocialForceIntersection.__init__)
    assert "mid_classes" not in sig.parameters                     # (the constructor's signature stays the reference's + what it had)
    ins = intersection.SocialForceIntersection([])
    assert ins._mid_classes is None
    ins.set_mid_classes()                                           # no engine yet: kept, and told to the engine when it is made
    assert ins._mid_classes is True and ins._engine is None
    monkeypatch.setattr(intersection, "Engine", FakeEngine)
    FakeEngine.made.clear()
    ins.vehicles = [FakeVehicle()]
    ins._flush_pending = lambda: None
    e = ins._engine_ready()
    assert FakeEngine.made == [e] and e.calls == [True]
    ins._engine_ready()
    assert e.calls == [True]                                        # (once per engine)
    ins.set_mid_classes(False)                                      # an engine there: forwarded at once
    ins.set_mid_classes(on=True)
    assert e.calls == [True, False, True] and ins._mid_classes is True
    other = intersection.SocialForceIntersection([])               # never asked: the engine keeps its own default (CSF_MID_CLASSES)
    other.vehicles = [FakeVehicle()]
    other._flush_pending = lambda: None
    assert other._engine_ready().calls == []
    from compat.cyclistsocialforce import intersection as dropin   # the drop-in name has it too
    assert dropin.SocialForceIntersection.set_mid_classes is intersection.SocialForceIntersection.set_mid_classes


def test_the_resource_figures_are_recorded():
    """profiles/mid_classes_resource_usage.txt: the eight new instances within what a workgroup of eight waves can hold, without scratch;
    the existing instances of csf_mid.hip, csf_pair.hip, csf_agent.hip and csf_small_classes.hip stated unchanged"""
    text = open(os.path.join(ROOT, "profiles", "mid_classes_resource_usage.txt")).read()
    new = re.findall(r"^void csf::mid_classes_(?:batch_)?kernel<(?:true|false), (?:true|false)>\n\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", text, flags=re.M)
    assert len(new) == 8
    for r in new:
        vgpr, agpr, scratch, occ, lds, vspill = int(r[0]), int(r[1]), int(r[3]), int(r[4]), int(r[5]), int(r[6])
        assert vgpr + agpr <= 256 and scratch == 0 and vspill == 0 and occ >= 2 and lds <= 65536
    for unit in ("csf_mid.hip", "csf_pair.hip", "csf_agent.hip", "csf_small_classes.hip"):
        assert re.search(rf"^{re.escape(unit)}: device code IDENTICAL to the parent build", text, flags=re.M), unit


@pytest.mark.parametrize("kind,n,rule", ALL_CASES)
def test_the_oracle_is_not_chaotic_on_the_seeds(kind, n, rule):
    """every population of GPU tests 2 and 3 on the CPU oracle alone: finite, and a start moved by one fp32 ulp of the coordinate bound stays
    within a tenth of the window's bar over a window - so that what the GPU test sees at the bar is the kernel's, not the crowd's"""
    c = population(kind, n, rule)
    moved = dict(c, s0=c["s0"].copy())
    moved["s0"][::2, 0] += ulp32(c["box"])                         # (every other road user: neighbours move against each other)
    a, b = oracle_population(c), oracle_population(moved)
    a.step(WINDOW); b.step(WINDOW)
    sa, sb = a.state(), b.state()
    fx, fy = a.forces()
    assert np.isfinite(sa).all() and np.isfinite(fx).all() and np.isfinite(fy).all()
    keep = np.ones(n, dtype=bool)
    if c["script"] is not None:
        keep[c["script"][0]] = False                                # (a scripted car is where its script says, moved or not)
    drift = np.abs(sa[keep, :2] - sb[keep, :2]).max()
    print(f"{kind} {n} rule {rule}: a start moved by {ulp32(c['box']):.1e} m is {drift:.1e} m off after {WINDOW} ticks (a tenth of the bar: {0.1 * POS_TOL * c['box']:.1e})")
    assert drift <= 0.1 * POS_TOL * c["box"]
