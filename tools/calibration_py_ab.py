"""Host time of cyclistsocialforce_amd/calibration.py against another version of the same file, A/B in one process:
    python3 tools/calibration_py_ab.py --parent OLD_calibration.py [--cpu] [--rounds 5]
OLD_calibration.py is a copy of the file at the commit to compare with (git show COMMIT:cyclistsocialforce_amd/calibration.py); it is
loaded as a second module of the package.  One data set - 8 scenes x 8 riders, 64 ticks, 256 vectors, max_sets = 256 -, the two versions
alternating round by round.  --cpu: an engine that returns at once (zeros of the right shape), so only the Python is timed: the first
`_dataset()` load of a fresh object (the median over the round's --calls objects) and the median `evaluate` call of a round.  Otherwise the real engine on the GPU: ms per `evaluate` under
calc_sse_timesteps (sums only) and under a custom error function (the states=True path).  One JSON line per figure: the rounds of
both versions, their medians, the parent's spread (max - min) and whether the candidate's median is within it."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_SCENES, N_RIDERS, TICKS, VECTORS = 8, 8, 64, 256


class InstantEngine:
    """every call returns at once; an evaluation gives zeros of the engine's shapes"""

    def __init__(self, pod, capacity, device=0):
        pass

    def scene_calib_load(self, nr, s0, vd, off, rows, obj, feat, lengths=None, max_sets=256):
        self.R, self.T = s0.shape[0], obj.shape[0]

    def scene_calib_eval(self, pods, states=False, stride=1):
        sums = np.zeros((len(pods), self.R, 2))
        return (sums, np.zeros((self.T // stride, len(pods) * self.R, 5))) if states else sums

    def close(self):
        pass


def custom(outputs, objectives):
    return sum(float(np.abs(o - b).sum()) for o, b in zip(outputs, objectives))


def scenes(cal):
    from scene_calib_common import crowd
    out = []
    for q in range(N_SCENES):
        x, y, psi, v, off, dq = crowd(N_RIDERS, seed=500 + q, box=14.0)
        s0 = np.c_[x, y, psi, v, np.zeros(N_RIDERS)]
        traj = np.random.default_rng(600 + q).normal(size=(TICKS, N_RIDERS, 4)) + s0[None, :, :4]
        out.append(cal.SceneData(s0, 5.0, off, dq, traj))
    return out


def one_round(cal, cpu, calls):
    """{figure: milliseconds} of one round of one version"""
    from cyclistsocialforce_amd import vehicle
    data, out = scenes(cal), {}
    vectors = np.array([7.0, 0.5])[None, :] * (1.0 + 0.001 * np.arange(VECTORS))[:, None]
    for label, func in (("sse", cal.calc_sse_timesteps), ("custom", custom)):
        kw = dict(engine_factory=InstantEngine) if cpu else {}
        loads = []
        for k in range(calls if label == "sse" else 1):           # the first load of a fresh object, `calls` objects a round
            if k:
                c.close()
            c = cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0", "sigma_0"], data, data, [1, 1, 0, 0, 0, 0], error_func=func, max_sets=256, **kw)
            t0 = time.perf_counter()
            c._dataset()
            loads.append(1e3 * (time.perf_counter() - t0))
        if label == "sse":
            out["load"] = float(np.median(loads))
        c.evaluate(vectors)                                       # (warm)
        times = []
        for _ in range(calls if label == "sse" else max(3, calls // 4)):
            t0 = time.perf_counter()
            c.evaluate(vectors)
            times.append(1e3 * (time.perf_counter() - t0))
        out["evaluate " + label] = float(np.median(times))
        c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    from cyclistsocialforce_amd import calibration as new
    spec = importlib.util.spec_from_file_location("cyclistsocialforce_amd._calibration_parent", a.parent)
    old = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(old)
    one_round(old, a.cpu, 2), one_round(new, a.cpu, 2)            # (both warm before the first round that counts)
    got = {"parent": [], "candidate": []}
    for _ in range(a.rounds):
        got["parent"].append(one_round(old, a.cpu, a.calls))
        got["candidate"].append(one_round(new, a.cpu, a.calls))
    for fig in got["parent"][0]:
        p, c = [r[fig] for r in got["parent"]], [r[fig] for r in got["candidate"]]
        spread = max(p) - min(p)
        print(json.dumps({"engine": "instant (cpu)" if a.cpu else "gpu", "figure": fig, "unit": "ms", "parent": [round(x, 4) for x in p],
                          "candidate": [round(x, 4) for x in c], "parent_median": round(float(np.median(p)), 4),
                          "candidate_median": round(float(np.median(c)), 4), "parent_spread": round(spread, 4),
                          "within": bool(np.median(c) <= np.median(p) + spread)}))


if __name__ == "__main__":
    main()
