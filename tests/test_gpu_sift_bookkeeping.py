"""The sift -> queue -> field passes of pair_cull_kernel (csf_pair.hip) against a recording of the build before their address and
queue bookkeeping was rewritten: the record addresses of the field-of-view sift, the queue append (a slot is `qx ^ 2 L`, the head of
the ring only ever at entry 0 or CHUNK) and the queue reads of the field passes compute no physics, so the kept set, its order in the
queue, the passes and every sum must be what they were - to the last bit, and the kernel's own counters as integers.

tests/golden/sift_bookkeeping_<case>.npz (tests/golden/make_golden_sift_bookkeeping.py, populations in
tests/sift_bookkeeping_common.py): three ticks of four populations of TwoDBicycle riders at the smallest size the wide cull-first
workgroup runs at - the headline's density, a crowd whose queue wraps many times, a ragged last tile, and the every-pair append path.
The same populations are held against the CPU oracle with the bounds of test_gpu_parity.py::test_full_size_ticks_vs_oracle."""
import numpy as np
import pytest

import sift_bookkeeping_common as sb
from oracle import csf_oracle as orc
from test_gpu_parity import amd  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.cull_variant]

_runs = {}


def engine_run(amd, monkeypatch, case):
    """the engine's three ticks of a case: run once, shared by the tests of the case, not modified"""
    if case not in _runs:
        sb.set_env(case, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
        _runs[case] = sb.run(amd.Engine, amd.pod, case)
    return _runs[case]


@pytest.mark.parametrize("case", list(sb.CASES))
def test_forces_states_and_counters_are_the_recorded_bits(amd, monkeypatch, case):
    g = np.load(sb.fixture_path(case))
    r = engine_run(amd, monkeypatch, case)
    # the kernel's counters: pairs evaluated, sources tested, full passes, partial passes - as integers
    print(case, "counts", r["counts"].tolist())
    assert np.array_equal(r["counts"], g["counts"]), (r["counts"].tolist(), g["counts"].tolist())
    for t in range(sb.TICKS):
        # total forces of tick t: every float64 with == on its bits
        assert np.array_equal(r["fx"][t].view(np.uint64), g["fx"][t].view(np.uint64)), (case, t, int((r["fx"][t] != g["fx"][t]).sum()))
        assert np.array_equal(r["fy"][t].view(np.uint64), g["fy"][t].view(np.uint64)), (case, t, int((r["fy"][t] != g["fy"][t]).sum()))
        assert sb.digest(np.c_[r["fx"][t], r["fy"][t]]) == str(g["force_digests"][t]), (case, t)
        # states after tick t: the digest of their bytes (equal digests: equal bits), the last tick's also value by value
        assert sb.digest(r["states"][t]) == str(g["state_digests"][t]), (case, t)
    assert np.array_equal(r["states"][-1].view(np.uint64), g["states_last"].view(np.uint64))
    assert r["near_dropped"] == 0 and r["status_ok"]


@pytest.mark.parametrize("case", list(sb.CASES))
def test_the_same_ticks_vs_oracle(amd, monkeypatch, case):
    """positions 1e-4 of the distance covered; forces of EVERY receiver 1e-4 of the largest force, median 2e-6, 99.9 % 2e-5"""
    r = engine_run(amd, monkeypatch, case)
    s0, off, dq = sb.population(case)
    pop = orc.Population(orc.default_params("twod", **sb.overrides(case)), s0, 5.0, off, dq)
    pop.step(sb.TICKS)
    got, ref = r["states"][-1], pop.state()
    moved = np.abs(ref[:, :2] - s0[:, :2]).max()
    err = np.abs(got[:, :2] - ref[:, :2]).max()
    fx, fy = r["fx"][-1], r["fy"][-1]
    ox, oy = pop.forces()
    scale = np.hypot(ox, oy).max()
    df = np.abs(np.c_[fx - ox, fy - oy]).max(axis=1)
    print(f"{case}: max |dpos| after {sb.TICKS} ticks = {err:.3e} m (moved up to {moved:.3f} m); force error / max force: median "
          f"{np.median(df) / scale:.2e}, 99.9 % {np.percentile(df, 99.9) / scale:.2e}, max {df.max() / scale:.2e} (receiver {int(df.argmax())})")
    assert err < 1e-4 * moved
    assert np.median(df) < 2e-6 * scale and np.percentile(df, 99.9) < 2e-5 * scale
    assert df.max() < 1e-4 * scale
    assert r["near_dropped"] == 0 and r["status_ok"]
    if sb.CASES[case]["far_eps"] is None:
        assert np.isfinite(r["far_radius"])
    else:
        assert np.isinf(r["far_radius"])
