"""The paths of pair_cull_kernel (csf_pair.hip) on which a tile is filled again or addressed differently - receivers in binned
order, the workgroup of four waves, several tiles per workgroup in slot order - against a recording of the build before the tile of
the plain f32 variants went from four arrays to one 16-byte record per source (one ds_read_b128 per source in the sift and the
field pass, queue entries 16 x index): the layout computes no physics, the same values reach the same instructions in the same
order, so forces, states, the kernel's counters, the dropped near pairs and the kernel's name must be what they were - by equality.

tests/golden/pair_tile_layout_<case>.npz (tests/golden/make_golden_pair_tile_layout.py, populations in
tests/pair_tile_layout_common.py): three ticks of three populations.  The same populations are held against the CPU oracle with
the bounds of test_gpu_pair_plain_f32.py::test_the_same_ticks_vs_oracle."""
import numpy as np
import pytest

import pair_tile_layout_common as tl
from oracle import csf_oracle as orc
from test_gpu_parity import amd  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.cull_variant]

_runs = {}


def engine_run(amd, monkeypatch, case):
    """the engine's three ticks of a case: run once, shared by the tests of the case, not modified"""
    if case not in _runs:
        tl.set_env(case, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
        _runs[case] = tl.run(amd.Engine, amd.pod, case)
    return _runs[case]


@pytest.mark.parametrize("case", list(tl.CASES))
def test_forces_states_and_counters_are_the_recorded_bits(amd, monkeypatch, case):
    g = np.load(tl.fixture_path(case))
    r = engine_run(amd, monkeypatch, case)
    print(case, "counts", r["counts"].tolist(), "far radius", r["far_radius"])
    # the kernel's counters - pairs evaluated, sources tested, full passes, partial passes -, the dropped near pairs, the kernel
    assert np.array_equal(r["counts"], g["counts"]), (r["counts"].tolist(), g["counts"].tolist())
    assert np.array_equal(r["near_dropped"], g["near_dropped"]) and (r["near_dropped"] == 0).all()
    assert r["kernels"].tolist() == g["kernels"].tolist() == ["pair_cull_kernel"] * tl.TICKS
    assert r["far_radius"] == float(g["far_radius"])
    # the case ran the launch shape it is meant for: not the counters and the far-field radius of its contrast shape
    assert tl.other_shape(r["counts"], r["far_radius"], g["contrast_counts"], g["contrast_far_radius"])
    for t in range(tl.TICKS):
        # forces and states of tick t: the digest of their bytes (equal digests: equal bits)
        assert tl.digest(np.c_[r["fx"][t], r["fy"][t]]) == str(g["force_digests"][t]), (case, t)
        assert tl.digest(r["states"][t]) == str(g["state_digests"][t]), (case, t)
    # the last tick's forces and positions also value by value, every float64 with == on its bits
    assert np.array_equal(r["fx"][-1].view(np.uint64), g["fx_last"].view(np.uint64)), int((r["fx"][-1] != g["fx_last"]).sum())
    assert np.array_equal(r["fy"][-1].view(np.uint64), g["fy_last"].view(np.uint64)), int((r["fy"][-1] != g["fy_last"]).sum())
    assert np.array_equal(np.ascontiguousarray(r["states"][-1][:, :2]).view(np.uint64), g["xy_last"].view(np.uint64))
    assert r["status_ok"]


@pytest.mark.parametrize("case", list(tl.CASES))
def test_the_same_ticks_vs_oracle(amd, monkeypatch, case):
    """positions 1e-4 of the distance covered; forces of EVERY receiver 1e-4 of the largest force, median 2e-6, 99.9 % 2e-5"""
    r = engine_run(amd, monkeypatch, case)
    s0, off, dq = tl.population(case)
    pop = orc.Population(orc.default_params("twod"), s0, 5.0, off, dq)
    pop.step(tl.TICKS)
    got, ref = r["states"][-1], pop.state()
    moved = np.abs(ref[:, :2] - s0[:, :2]).max()
    err = np.abs(got[:, :2] - ref[:, :2]).max()
    fx, fy = r["fx"][-1], r["fy"][-1]
    ox, oy = pop.forces()
    scale = np.hypot(ox, oy).max()
    df = np.abs(np.c_[fx - ox, fy - oy]).max(axis=1)
    print(f"{case}: max |dpos| after {tl.TICKS} ticks = {err:.3e} m (moved up to {moved:.3f} m); force error / max force: median "
          f"{np.median(df) / scale:.2e}, 99.9 % {np.percentile(df, 99.9) / scale:.2e}, max {df.max() / scale:.2e} (receiver {int(df.argmax())})")
    assert err < 1e-4 * moved
    assert np.median(df) < 2e-6 * scale and np.percentile(df, 99.9) < 2e-5 * scale
    assert df.max() < 1e-4 * scale
    assert (r["near_dropped"] == 0).all() and r["status_ok"]
    assert np.isfinite(r["far_radius"])
