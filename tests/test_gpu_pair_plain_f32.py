"""Instantiations of pair_cull_kernel (csf_pair.hip) that tests/test_gpu_sift_bookkeeping.py does not reach - priority to the
right (P2R, on the four-wave workgroup 4 096 riders get), two parameter sets in the class-segmented order (SEG, eight waves), 16
receivers per wide workgroup of eight waves (CSF_EXPERT=1 CSF_RPB=16 CSF_WIDE=1: an 8-way shard's kernel) - against a recording
of the build before the reach test and the field pass were issued as plain f32 instructions: a half of v_pk_fma_f32 and a v_fma_f32
are the same IEEE operation, and the plain form keeps the packed form's pairing of products and fused multiply-adds
(csf_field.h: keep_half, field_twod_half), so the kept set, its order in the queue, the passes and every sum must be what they
were - to the last bit, and the kernel's own counters as integers.

tests/golden/pair_plain_f32_<case>.npz (tests/golden/make_golden_pair_plain_f32.py, populations in tests/pair_plain_f32_common.py):
three ticks of three populations of 4 096 TwoDBicycle riders.  The same populations are held against the CPU oracle with the bounds
of test_gpu_sift_bookkeeping.py::test_the_same_ticks_vs_oracle."""
import numpy as np
import pytest

import pair_plain_f32_common as pp
from oracle import csf_oracle as orc
from test_gpu_parity import amd  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.cull_variant]

_runs = {}


def engine_run(amd, monkeypatch, case):
    """the engine's three ticks of a case: run once, shared by the tests of the case, not modified"""
    if case not in _runs:
        pp.set_env(case, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
        _runs[case] = pp.run(amd.Engine, amd.pod, case)
    return _runs[case]


@pytest.mark.parametrize("case", list(pp.CASES))
def test_forces_states_and_counters_are_the_recorded_bits(amd, monkeypatch, case):
    g = np.load(pp.fixture_path(case))
    r = engine_run(amd, monkeypatch, case)
    # the kernel's counters: pairs evaluated, sources tested, full passes, partial passes - as integers
    print(case, "counts", r["counts"].tolist())
    assert np.array_equal(r["counts"], g["counts"]), (r["counts"].tolist(), g["counts"].tolist())
    for t in range(pp.TICKS):
        # total forces of tick t: every float64 with == on its bits
        assert np.array_equal(r["fx"][t].view(np.uint64), g["fx"][t].view(np.uint64)), (case, t, int((r["fx"][t] != g["fx"][t]).sum()))
        assert np.array_equal(r["fy"][t].view(np.uint64), g["fy"][t].view(np.uint64)), (case, t, int((r["fy"][t] != g["fy"][t]).sum()))
        assert pp.digest(np.c_[r["fx"][t], r["fy"][t]]) == str(g["force_digests"][t]), (case, t)
        # states after tick t: the digest of their bytes (equal digests: equal bits), the last tick's also value by value
        assert pp.digest(r["states"][t]) == str(g["state_digests"][t]), (case, t)
    assert np.array_equal(r["states"][-1].view(np.uint64), g["states_last"].view(np.uint64))
    assert r["near_dropped"] == 0 and r["status_ok"]
    if case == "rpb16":
        # The riders are those of sift_bookkeeping_common's `headline`, which runs the four-wave workgroup on tiles of 1 024 sources.
        # Here a visit covers a tile of 2 048: the same riders are evaluated in other passes - pass counters equal to that fixture's
        # would mean the launch-shape knobs were not honoured and the wide 16-receiver instantiation was not reached.
        h = np.load(pp.sb.fixture_path("headline"))["counts"]
        assert (r["counts"][:, 2] != h[:, 2]).all() and (r["counts"][:, 3] != h[:, 3]).all(), (r["counts"].tolist(), h.tolist())


@pytest.mark.parametrize("case", list(pp.CASES))
def test_the_same_ticks_vs_oracle(amd, monkeypatch, case):
    """positions 1e-4 of the distance covered; forces of EVERY receiver 1e-4 of the largest force, median 2e-6, 99.9 % 2e-5"""
    r = engine_run(amd, monkeypatch, case)
    c = pp.CASES[case]
    s0, off, dq = pp.population(case)
    if c["sets"] is None:
        pop = orc.Population(orc.default_params("twod", priority_rule=c["rule"]), s0, 5.0, off, dq)
    else:
        tab = [orc.Params.from_buffer_copy(bytes(amd.pod("twod", priority_rule=c["rule"], **kw))) for kw in c["sets"]]
        pop = orc.Population(tab[0], s0, 5.0, off, dq)
        pop.set_classes(tab, pp.classes(case))
    pop.step(pp.TICKS)
    got, ref = r["states"][-1], pop.state()
    moved = np.abs(ref[:, :2] - s0[:, :2]).max()
    err = np.abs(got[:, :2] - ref[:, :2]).max()
    fx, fy = r["fx"][-1], r["fy"][-1]
    ox, oy = pop.forces()
    scale = np.hypot(ox, oy).max()
    df = np.abs(np.c_[fx - ox, fy - oy]).max(axis=1)
    print(f"{case}: max |dpos| after {pp.TICKS} ticks = {err:.3e} m (moved up to {moved:.3f} m); force error / max force: median "
          f"{np.median(df) / scale:.2e}, 99.9 % {np.percentile(df, 99.9) / scale:.2e}, max {df.max() / scale:.2e} (receiver {int(df.argmax())})")
    assert err < 1e-4 * moved
    assert np.median(df) < 2e-6 * scale and np.percentile(df, 99.9) < 2e-5 * scale
    assert df.max() < 1e-4 * scale
    assert r["near_dropped"] == 0 and r["status_ok"]
    assert np.isfinite(r["far_radius"])
