#!/usr/bin/env python3
"""Time of ONE evaluation of the calibration objective for n_sets candidate parameter sets (GPU box): (b) csf_calib_eval - the data
set resident, all sets and sequences in one launch, the error summed on the device - against (a) what a caller had before:
csf_replay_forces once per set on an engine that holds the sequences (a fresh population per set, one launch per tick, every
state copied back) plus the NumPy error on the trajectories.  16 sequences x 1 000 ticks, TwoDBicycle and InvPendulumBicycle,
n_sets in 1, 4, 16, 64, 256; the two paths alternate window by window in one process.  One JSON line per cell: medians of the
windows with min / max, milliseconds per evaluation of all n_sets.

    python tools/calib_rate.py [--sets 1,4,16,64,256] [--seq 16] [--ticks 1000] [--windows 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.pop("CSF_PAIR_VARIANT", None)
from cyclistsocialforce_amd import _ffi, parameters  # noqa: E402
from cyclistsocialforce_amd.calibration import calc_sse_timesteps  # noqa: E402
from cyclistsocialforce_amd.engine import Engine  # noqa: E402


def data_set(model, n_seq, ticks, seed=0):
    rng = np.random.default_rng(seed)
    base = parameters.default_pod(model)
    s0 = np.zeros((n_seq, _ffi.N_STATES[base.model]))
    s0[:, 0], s0[:, 1] = rng.uniform(-20, 20, n_seq), rng.uniform(-20, 20, n_seq)
    s0[:, 2], s0[:, 3] = rng.uniform(-np.pi, np.pi, n_seq), rng.uniform(3, 5, n_seq)
    t = np.arange(ticks)[:, None] * base.t_s
    phi = s0[None, :, 2] + 0.4 * np.sin(rng.uniform(0.5, 1.5, n_seq)[None, :] * t)
    mag = 4.0 + 0.5 * np.sin(0.8 * t + rng.uniform(0, 6, n_seq)[None, :])
    return base, s0, mag * np.cos(phi), mag * np.sin(phi)


def pod_sets(base, n):
    out = []
    for k in range(n):
        p = _ffi.Params.from_buffer_copy(base)
        p.k_p_v = base.k_p_v * (1.0 + 0.002 * k)
        out.append(p)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="1,4,16,64,256")
    ap.add_argument("--seq", type=int, default=16)
    ap.add_argument("--ticks", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--models", default="twod,invpend")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for model in a.models.split(","):
        base, s0, Fx, Fy = data_set(model, a.seq, a.ticks)
        feat = np.array([0, 1, 2], dtype=np.int32)
        obj = np.random.default_rng(1).normal(size=(a.ticks, a.seq, 3))
        objectives = [obj[:, q] for q in range(a.seq)]
        for n_sets in [int(x) for x in a.sets.split(",")]:
            sets = pod_sets(base, n_sets)
            new = Engine(base, n_sets * a.seq)
            new.calib_load(s0, Fx, Fy, obj, feat, max_sets=n_sets)
            old = Engine(base, a.seq)

            def parent_path():
                errs = np.zeros(n_sets)
                for k, p in enumerate(sets):
                    if old.n:
                        old.remove_agents(np.arange(old.n))
                    old.set_params(p)
                    old.add_agents(s0, 0.0)
                    st = old.replay_forces(Fx, Fy, fix_speed=True)
                    errs[k] = calc_sse_timesteps([st[:, q][:, feat] for q in range(a.seq)], objectives)
                return errs

            def new_path():
                return new.calib_eval(sets, fix_speed=True)[:, :, 0].sum(axis=1)

            e_old, e_new = parent_path(), new_path()        # warm both, and they agree
            agree = float(np.max(np.abs(e_old - e_new) / e_old))
            w_old, w_new = [], []
            for _ in range(a.windows):
                t0 = time.perf_counter(); parent_path(); w_old.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter(); new_path(); w_new.append((time.perf_counter() - t0) * 1e3)
            line = {"model": model, "n_seq": a.seq, "ticks": a.ticks, "n_sets": n_sets,
                    "replay_per_set_ms": round(float(np.median(w_old)), 3), "replay_per_set_min_max": [round(min(w_old), 3), round(max(w_old), 3)],
                    "calib_eval_ms": round(float(np.median(w_new)), 3), "calib_eval_min_max": [round(min(w_new), 3), round(max(w_new), 3)],
                    "speedup": round(float(np.median(w_old) / np.median(w_new)), 2),
                    "median_below_baseline_min": bool(np.median(w_new) < min(w_old)), "largest_relative_difference_of_the_errors": agree}
            print(json.dumps(line), flush=True)
            lines.append(line)
            new.close(); old.close()
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
