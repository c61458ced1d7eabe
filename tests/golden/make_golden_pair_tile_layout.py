"""Records tests/golden/pair_tile_layout_<case>.npz on an MI355X with the library that is loaded (CSF_LIB selects another build):
    python3 tests/golden/make_golden_pair_tile_layout.py [output directory]
The fixture was recorded with the build BEFORE the tile of the plain f32 variants of pair_cull_kernel became one 16-byte record per
source; the populations and what is recorded are in tests/pair_tile_layout_common.py.  Per case and tick: the SHA-256 of the bytes
of the total forces and of the states, the four counters of csf_count_pairs, the near pairs dropped and the kernel's name; of the
last tick also the forces and the positions in full.  Every case is run a second time in the launch shape it must NOT have taken
(CONTRAST): that run's counters and far-field radius are stored beside the case's, and the two must differ."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import pair_tile_layout_common as tl  # noqa: E402


def main(outdir):
    from cyclistsocialforce_amd import engine, parameters

    os.makedirs(outdir, exist_ok=True)
    ok = True
    for case in tl.CASES:
        runs = []
        for contrast in (False, True):
            tl.set_env(case, os.environ.__setitem__, lambda k: os.environ.pop(k, None), contrast=contrast)
            runs.append(tl.run(engine.Engine, parameters.default_pod, case))
        r, c = runs
        print(case, "far radius", r["far_radius"], "counts", r["counts"].tolist(), "near dropped", r["near_dropped"].tolist(), r["kernels"].tolist())
        print(case, "contrast: far radius", c["far_radius"], "counts", c["counts"].tolist())
        assert r["status_ok"] and (r["near_dropped"] == 0).all() and (r["kernels"] == "pair_cull_kernel").all(), case
        other = tl.other_shape(r["counts"], r["far_radius"], c["counts"], c["far_radius"])
        print(case, "ran another shape than its contrast:", other)
        ok = ok and other
        np.savez_compressed(os.path.join(outdir, f"pair_tile_layout_{case}.npz"), fx_last=r["fx"][-1], fy_last=r["fy"][-1],
                            xy_last=r["states"][-1][:, :2],
                            force_digests=np.array([tl.digest(np.c_[x, y]) for x, y in zip(r["fx"], r["fy"])]),
                            state_digests=np.array([tl.digest(s) for s in r["states"]]), counts=r["counts"],
                            near_dropped=r["near_dropped"], kernels=r["kernels"], far_radius=np.float64(r["far_radius"]),
                            contrast_counts=c["counts"], contrast_far_radius=np.float64(c["far_radius"]))
    assert ok, "a case reproduced the counters and the far-field radius of its contrast shape: its knobs were not honoured"


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
