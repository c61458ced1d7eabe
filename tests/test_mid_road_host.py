"""The road term inside the one-launch tick, host side (no GPU): both entry points declared, exported and bound with the
right signatures, NULL refused without a device; Engine.mid_road / mid_road_ticks and the mirror's set_mid_road forward (fake engines);
the recorded resource comparison; and - with the CPU oracle - that the oracle alone is finite on the inputs of
tests/test_gpu_mid_road.py::test_road_members_of_a_batch_vs_oracle."""
import ctypes as C
import os
import re

import numpy as np

from cyclistsocialforce_amd import _ffi, intersection
from cyclistsocialforce_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "csf.h")).read()
    declared = set(re.findall(r"\b(csf_[a-z_0-9]+)\s*\(", header))
    lib = _ffi.load()                                                # (the gfx950 library is built and loads)
    for name in ("csf_mid_road", "csf_mid_road_ticks"):
        assert name in declared and name in _ffi.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"int csf_mid_road\(csf_engine \*e, int32_t on\);", header)
    assert re.search(r"int csf_mid_road_ticks\(const csf_engine \*e, int64_t \*n_ticks\);", header)
    assert lib.csf_mid_road.restype in (C.c_int, C.c_int32) and lib.csf_mid_road_ticks.restype in (C.c_int, C.c_int32)
    assert lib.csf_mid_road.argtypes == [C.c_void_p, C.c_int32]
    assert lib.csf_mid_road_ticks.argtypes == [C.c_void_p, C.POINTER(C.c_int64)]
    for on in (0, 1, 2):
        assert lib.csf_mid_road(None, on) == -1                      # (CSF_E_ARG: no engine)
    n = C.c_int64(7)
    assert lib.csf_mid_road_ticks(None, C.byref(n)) == -1 and n.value == 7
    assert lib.csf_mid_road_ticks(None, None) == -1
    assert lib.csf_abi_version() == 9 and _ffi.ABI_VERSION == 9      # (csf_params and the ABI version do not change)


class FakeLib:
    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def csf_mid_road(self, h, on):
        self.calls.append((h, on))
        return self.rc

    def csf_mid_road_ticks(self, h, ref):
        ref._obj.value = 41
        return self.rc

    def csf_last_error(self, h):
        return b"csf_mid_road: refused"

    def csf_destroy(self, h):
        pass


def test_engine_mid_road_forwards():
    e = Engine.__new__(Engine)
    e._lib, e._h = FakeLib(), "handle"
    e.mid_road()
    e.mid_road(False)
    e.mid_road(on=True)
    assert e._lib.calls == [("handle", 1), ("handle", 0), ("handle", 1)]
    assert e.mid_road_ticks() == 41
    e._lib = FakeLib(rc=-4)
    try:
        e.mid_road()
        raise AssertionError("a refused call raises")
    except _ffi.EngineError as err:
        assert "-4" in str(err) and "csf_mid_road" in str(err)
    e._h = None


class FakeEngine:
    made = []

    def __init__(self, pod, capacity, device=0):
        self.calls, self.ns = [], 5
        FakeEngine.made.append(self)

    def mid_road(self, on=True):
        self.calls.append(on)


class FakeVehicle:
    N_STATES = 5

    def _pod(self, rule):
        return b"pod"


def test_the_mirrors_method_forwards_now_or_when_the_engine_is_made(monkeypatch):
    import inspect
    sig = inspect.signature(intersection.SocialForceIntersection.__init__)
    assert "mid_road" not in sig.parameters                        # (the constructor's signature stays the reference's + what it had)
    ins = intersection.SocialForceIntersection([])
    assert ins._mid_road is None
    ins.set_mid_road()                                              # no engine yet: kept, and told to the engine when it is made
    assert ins._mid_road is True and ins._engine is None
    monkeypatch.setattr(intersection, "Engine", FakeEngine)
    FakeEngine.made.clear()
    ins.vehicles = [FakeVehicle()]
    ins._flush_pending = lambda: None
    e = ins._engine_ready()
    assert FakeEngine.made == [e] and e.calls == [True]
    ins._engine_ready()
    assert e.calls == [True]                                        # (once per engine)
    ins.set_mid_road(False)                                         # an engine there: forwarded at once
    ins.set_mid_road(on=True)
    assert e.calls == [True, False, True] and ins._mid_road is True
    other = intersection.SocialForceIntersection([])               # never asked: the engine keeps its own default (CSF_MID_ROAD)
    other.vehicles = [FakeVehicle()]
    other._flush_pending = lambda: None
    assert other._engine_ready().calls == []
    from compat.cyclistsocialforce import intersection as dropin   # the drop-in name has it too
    assert dropin.SocialForceIntersection.set_mid_road is intersection.SocialForceIntersection.set_mid_road


def test_the_resource_comparison_is_recorded():
    """profiles/mid_road_resource_usage.txt: the ten ROAD = false instances of each kernel with the figures they had, and the new ones
    within what a workgroup of twelve (eight) waves can hold"""
    text = open(os.path.join(ROOT, "profiles", "mid_road_resource_usage.txt")).read()
    verdicts = re.findall(r"^  figures (EQUAL|DIFFER); instruction stream (IDENTICAL|differs)", text, flags=re.M)
    mid = text.split("== csf_pair.hip")[0]
    assert len(re.findall(r"^  figures EQUAL; instruction stream IDENTICAL", mid, flags=re.M)) == 20
    assert all(v[0] == "EQUAL" for v in verdicts)
    new = re.findall(r"^void csf::mid_(?:tick|batch)_kernel<\d+, (?:true|false), true>\n\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", mid, flags=re.M)
    assert len(new) == 20
    for r in new:
        vgpr, agpr, scratch, occ, lds = int(r[0]), int(r[1]), int(r[3]), int(r[4]), int(r[5])
        assert vgpr + agpr <= 256 and scratch == 0 and occ >= 2 and lds <= 65536


def test_the_oracle_alone_is_finite_on_the_batched_road_members():
    """the four members of test_road_members_of_a_batch_vs_oracle, 20 ticks on the CPU oracle: every force and state finite"""
    from mid_road_common import ORACLE_MEMBERS, oracle_member
    for m in ORACLE_MEMBERS:
        pop = oracle_member(m)
        for _ in range(20):
            pop.step(1)
            fx, fy = pop.forces()
            assert np.isfinite(fx).all() and np.isfinite(fy).all(), m
        assert np.isfinite(pop.state()).all(), m
