"""Records tests/golden/pair_plain_f32_<case>.npz on an MI355X with the library that is loaded (CSF_LIB selects another build):
    python3 tests/golden/make_golden_pair_plain_f32.py [output directory]
The fixture was recorded with the build BEFORE the reach test and the field pass of pair_cull_kernel were issued as plain f32
instructions; the populations and what is recorded are in tests/pair_plain_f32_common.py.  Per case, as
make_golden_sift_bookkeeping.py: the total forces of every tick and the states after the last one in full, the SHA-256 of the bytes
of the forces and of the states of every tick, and the four counters of csf_count_pairs per tick."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import pair_plain_f32_common as pp  # noqa: E402


def main(outdir):
    from cyclistsocialforce_amd import engine, parameters

    os.makedirs(outdir, exist_ok=True)
    for case in pp.CASES:
        pp.set_env(case, os.environ.__setitem__, lambda k: os.environ.pop(k, None))
        r = pp.run(engine.Engine, parameters.default_pod, case)
        assert r["near_dropped"] == 0 and r["status_ok"], case
        np.savez_compressed(os.path.join(outdir, f"pair_plain_f32_{case}.npz"), fx=r["fx"], fy=r["fy"], states_last=r["states"][-1],
                            force_digests=np.array([pp.digest(np.c_[x, y]) for x, y in zip(r["fx"], r["fy"])]),
                            state_digests=np.array([pp.digest(s) for s in r["states"]]), counts=r["counts"])
        print(case, "far radius", r["far_radius"], "counts", r["counts"].tolist())


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
