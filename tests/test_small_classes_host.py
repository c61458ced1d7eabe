"""The one-wave tick of several parameter sets and vehicle classes, host side (no GPU): the entry point declared, exported
and bound; Engine.small_classes and the mirror's set_small_classes forward (fake engines); the recorded resource comparison; and - with
the CPU oracle - the seed choices that tests/test_gpu_small_classes.py rests on."""
import ctypes as C
import os
import re

import numpy as np

from cyclistsocialforce_amd import _ffi, intersection
from cyclistsocialforce_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "csf.h")).read()
    declared = set(re.findall(r"\b(csf_[a-z_0-9]+)\s*\(", header))
    lib = _ffi.load()                                                # (the gfx950 library is built and loads)
    name = "csf_small_classes"
    assert name in declared and name in _ffi.SYMBOLS and hasattr(lib, name)
    assert re.search(r"int csf_small_classes\(csf_engine \*e, int32_t on\);", header)
    assert lib.csf_small_classes.restype in (C.c_int, C.c_int32)
    assert lib.csf_small_classes.argtypes == [C.c_void_p, C.c_int32]
    for on in (0, 1, 2):
        assert lib.csf_small_classes(None, on) == -1                 # (CSF_E_ARG: no engine)
    assert lib.csf_abi_version() == 9 and _ffi.ABI_VERSION == 9      # (csf_params and the ABI version do not change)


class FakeLib:
    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def csf_small_classes(self, h, on):
        self.calls.append((h, on))
        return self.rc

    def csf_last_error(self, h):
        return b"csf_small_classes: refused"

    def csf_destroy(self, h):
        pass


def test_engine_small_classes_forwards():
    e = Engine.__new__(Engine)
    e._lib, e._h = FakeLib(), "handle"
    e.small_classes()
    e.small_classes(False)
    e.small_classes(on=True)
    assert e._lib.calls == [("handle", 1), ("handle", 0), ("handle", 1)]
    e._lib = FakeLib(rc=-4)
    try:
        e.small_classes()
        raise AssertionError("a refused call raises")
    except _ffi.EngineError as err:
        assert "-4" in str(err) and "csf_small_classes" in str(err)
    e._h = None


class FakeEngine:
    made = []

    def __init__(self, pod, capacity, device=0):
        self.calls, self.ns = [], 5
        FakeEngine.made.append(self)

    def small_classes(self, on=True):
        self.calls.append(on)


class FakeVehicle:
    N_STATES = 5

    def _pod(self, rule):
        return b"pod"


def test_the_mirrors_method_forwards_now_or_when_the_engine_is_made(monkeypatch):
    import inspect
    sig = inspect.signature(intersection.SocialForceIntersection.__init__)
    assert "small_classes" not in sig.parameters                  # (the constructor's signature stays the reference's + what it had)
    ins = intersection.SocialForceIntersection([])
    assert ins._small_classes is None
    # no engine yet: kept, and told to the engine when it is made
    ins.set_small_classes()
    assert ins._small_classes is True and ins._engine is None
    monkeypatch.setattr(intersection, "Engine", FakeEngine)
    FakeEngine.made.clear()
    ins.vehicles = [FakeVehicle()]
    ins._flush_pending = lambda: None
    e = ins._engine_ready()
    assert FakeEngine.made == [e] and e.calls == [True]
    ins._engine_ready()
    assert e.calls == [True]                                        # (once per engine)
    # an engine there: forwarded at once
    ins.set_small_classes(False)
    ins.set_small_classes(on=True)
    assert e.calls == [True, False, True] and ins._small_classes is True
    # never asked: the engine keeps its own default (CSF_SMALL_CLASSES)
    other = intersection.SocialForceIntersection([])
    other.vehicles = [FakeVehicle()]
    other._flush_pending = lambda: None
    assert other._engine_ready().calls == []
    from compat.cyclistsocialforce import intersection as dropin   # the drop-in name has it too
    assert dropin.SocialForceIntersection.set_small_classes is intersection.SocialForceIntersection.set_small_classes


def test_the_resource_comparison_is_recorded():
    text = open(os.path.join(ROOT, "profiles", "small_classes_resource_usage.txt")).read()
    m = re.search(r"Existing kernel instances: (\d+); identical[^:]*: (\d+); changed: (\d+); gone: (\d+)", text)
    assert m and int(m.group(1)) == int(m.group(2)) > 0 and int(m.group(3)) == 0 and int(m.group(4)) == 0
    rows = re.findall(r"^  (_ZN3csf\S+): (.*?)   (identical|CHANGED.*|GONE)$", text, flags=re.M)
    assert len(rows) == int(m.group(1)) and all(r[2] == "identical" for r in rows)   # every existing-instance row: the same before and after
    for family in ("small_tick_kernel", "small_batch_kernel", "agent_kernel", "scene_eval_kernel", "scene_mixed_kernel"):
        assert any(family in r[0] for r in rows), family
    new = re.findall(r"^  (_ZN3csf\d+small_classes\w+): (\d+) (\d+) (\d+) (\d+) (\d+) (\d+) \| (\d+), (\d+)", text, flags=re.M)
    assert len(new) == 2 and {("batch" in r[0]) for r in new} == {True, False}
    for r in new:
        vgpr, agpr, lds = int(r[1]), int(r[2]), int(r[6])
        assert vgpr <= 256 and agpr <= 256 and lds <= 65536        # (what a workgroup of gfx950 can hold)


# ---- the seeds, by the CPU oracle ----------------------------------------------------------------------------------------------------------
def _run(c, ticks, s0=None, cls=None):
    from small_classes_common import oracle_population
    c = dict(c)
    if s0 is not None:
        c["s0"] = s0
    if cls is not None:
        c["cls"] = cls
    pop = oracle_population(c)
    if c["script"] is not None:                                    # (the oracle takes the scripts as CSR over all road users)
        idx, off, rows = c["script"]
        full = np.zeros(c["s0"].shape[0] + 1, dtype=np.int64)
        for k, a in enumerate(idx):
            full[a + 1:] += off[k + 1] - off[k]
        pop.set_script(full, rows)
    out = []
    for _ in range(ticks):
        pop.step(1)
        out.append(pop.state().copy())
    return np.array(out)


def _sensitivity(c, ticks, rng):
    ref = _run(c, ticks)
    assert np.isfinite(ref).all()
    worst = 0.0
    for _ in range(2):
        s1 = c["s0"].copy()
        s1[:, :2] += 1e-7 * rng.choice([-1.0, 1.0], size=(s1.shape[0], 2))
        worst = max(worst, float(np.abs(_run(c, ticks, s1) - ref).max()))
    return worst, ref


def test_the_oracle_is_not_chaotic_on_the_cases():
    """the seeds of small_classes_common.case (a) .. (f): an oracle run started from positions moved by 1e-7 m (two random sign patterns)
    stays within 2e-6 - a tenth of GENERAL_TOL - of the unmoved one on EVERY state row over the 40 ticks.  Measured: at most 7.3e-7 (case c)."""
    from small_classes_common import GENERAL_TOL, TICKS, case
    rng = np.random.default_rng(7)
    worst = 0.0
    for name, rule in (("a", 0), ("b", 0), ("b", 1), ("c", 0), ("d", 0), ("e", 0), ("f", 0)):
        w, _ = _sensitivity(case(name, rule), TICKS, rng)
        worst = max(worst, w)
        assert w < 0.1 * GENERAL_TOL, (name, rule, w)
    print(f"largest sensitivity of the oracle to 1e-7 m at the start, all state rows: {worst:.2e}")


def test_the_oracle_is_not_chaotic_on_the_horizon():
    """the case of test_five_riders_of_three_classes_vs_oracle: both priority rules, 200 ticks: within 1e-5 x extent - a tenth of that
    test's bound.  Measured: 2.1e-8 x extent."""
    from small_classes_common import oracle_case
    rng = np.random.default_rng(7)
    for rule in (0, 1):
        w, ref = _sensitivity(oracle_case(rule), 200, rng)
        ext = max(np.ptp(ref[..., 0]), np.ptp(ref[..., 1]), 14.0)
        assert w / ext < 1e-5, (rule, w / ext)


def test_a_swap_of_the_sets_moves_the_riders():
    """test_the_sets_belong_to_the_road_users: with the two sets of case (a) swapped between the two riders BOTH move by more than ten times
    SWAP_MOVED within the 40 ticks (found: 0.11 m and 0.35 m)"""
    from small_classes_common import SWAP_MOVED, TICKS, case
    c = case("a")
    a = _run(c, TICKS)
    b = _run(c, TICKS, cls=c["cls"][::-1].copy())
    moved = np.abs(a - b)[..., :2].max(axis=(0, 2))
    print(f"the sets swapped on the oracle: {moved} m")
    assert np.all(moved > 10.0 * SWAP_MOVED)
