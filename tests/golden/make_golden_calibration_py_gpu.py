"""Records tests/golden/calibration_py_gpu.npz on an MI355X with the library that is loaded:
    python3 tests/golden/make_golden_calibration_py_gpu.py [output directory]
The fixture was recorded with cyclistsocialforce_amd/calibration.py as it was BEFORE it was split into layers; the data sets and
what is recorded are in tests/test_gpu_calibration_py.py (`run_case`).  Keys: <case>__<label>."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_gpu_calibration_py as t  # noqa: E402


def main(outdir):
    os.makedirs(outdir, exist_ok=True)
    out = {}
    for name in t.CASES:
        got = t.run_case(name)
        for label in t.FUNCS:
            assert np.isfinite(got[label]).all() and np.all(got[label] > 0), (name, label, got[label])
            print(name, label, got[label].tolist())
        print(name, "NaN in the trajectories:", int(sum(np.isnan(v).sum() for k, v in got.items() if k.startswith("traj"))))
        out.update({f"{name}__{label}": v for label, v in got.items()})
    np.savez_compressed(os.path.join(outdir, "calibration_py_gpu.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
