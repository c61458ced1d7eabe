#!/usr/bin/env python3
"""Resident time per tick of K independent MID-SIZE scenes in one batch (GPU box): (b) the batched one-launch tick (csf_step_batch:
one launch of mid_batch_kernel per vehicle class and tick for all members) against (a) the same call with CSF_BATCH_MID=0, which
steps the mid-size members in turn - one mid_tick_kernel launch per member and tick, what the batch did before.  Two sets of equal
engines (the knob is read when an engine is created), each in its own batch, alternate window by window in one process; calls of
100 ticks with one wait.  K x n TwoDBicycle, and one InvPendulumBicycle and one Bicycle column; one leg with csf_record on and one
csf_batch_get_record per call.  Cells with K x n above --most road users are left out (and named).  One JSON line per cell: medians
of the windows with min / max, microseconds per tick of the whole set.

    python tools/batch_mid_rate.py [--ks 1,4,16,64,256] [--ns 40,100,300,1024] [--windows 5] [--most 80000] [--out FILE]
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
from cyclistsocialforce_amd.engine import Engine  # noqa: E402


def scene(model, n, seed):
    """n riders in a box of ~10 m^2 each, heading for destinations 50 .. 150 m out"""
    rng = np.random.default_rng(seed)
    box = max(30.0, 3.2 * np.sqrt(n))
    x, y = rng.uniform(0, box, n), rng.uniform(0, box, n)
    psi, v = rng.uniform(-np.pi, np.pi, n), rng.uniform(3, 6, n)
    reach = np.array([50.0, 100.0, 150.0])
    dq = np.zeros((n, 4, 3))
    dq[:, 0, 0], dq[:, 0, 1] = x, y
    dq[:, 1:, 0] = x[:, None] + reach * np.cos(psi)[:, None]
    dq[:, 1:, 1] = y[:, None] + reach * np.sin(psi)[:, None]
    s0 = np.zeros((n, _ffi.N_STATES[parameters.default_pod(model).model]))
    s0[:, 0], s0[:, 1], s0[:, 2], s0[:, 3] = x, y, psi, v
    e = Engine(parameters.default_pod(model), n)
    e.add_agents(s0, 5.0)
    e.set_dest_queue(np.arange(n), np.arange(n + 1) * 4, dq.reshape(-1, 3), reset=True)
    return e


def make_set(model, n, K, batch_mid, record):
    if batch_mid:
        os.environ.pop("CSF_BATCH_MID", None)
    else:
        os.environ["CSF_BATCH_MID"] = "0"
    es = [scene(model, n, 100 + i) for i in range(K)]
    os.environ.pop("CSF_BATCH_MID", None)
    if record:
        for e in es:
            e.record(1, 128, True)
    Engine.batch_join(es)
    return es


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,4,16,64,256")
    ap.add_argument("--ns", default="40,100,300,1024")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--most", type=int, default=80000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ks, ns = [int(k) for k in a.ks.split(",")], [int(n) for n in a.ns.split(",")]
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    cells = [("twod", n, K, False) for n in ns for K in ks] + [("invpend", 100, K, False) for K in ks] + [("bicycle", 100, K, False) for K in ks]
    cells.append(("twod", 100, 64, True))
    for model, n, K, record in cells:
        if K * n > a.most:
            emit({"model": model, "n": n, "K": K, "skipped": f"K x n above {a.most}"})
            continue
        sets = {"in_turn": make_set(model, n, K, False, record), "batched": make_set(model, n, K, True, record)}

        def call(es):
            Engine.step_batch(es, 100, sync=not record)
            if record:
                Engine.batch_recorded(es, 100)

        for es in sets.values():                                  # (code objects loaded, clocks up, buffers made)
            call(es)
            call(es)
        win = {k: [] for k in sets}
        for _ in range(max(3, a.windows)):
            for k, es in sets.items():
                t0 = time.perf_counter()
                call(es)
                win[k].append((time.perf_counter() - t0) * 1e6 / 100)
        enq = []
        for _ in range(3):
            t0 = time.perf_counter()
            Engine.step_batch(sets["batched"], 100)
            enq.append((time.perf_counter() - t0) * 1e6 / 100)
            sets["batched"][0].sync()
        ta, tb = win["in_turn"], win["batched"]
        emit({"model": model, "n": n, "K": K, "record": record, "ticks_per_call": 100,
              "in_turn_us_per_tick": {"median": round(float(np.median(ta)), 2), "min": round(min(ta), 2), "max": round(max(ta), 2)},
              "batched_us_per_tick": {"median": round(float(np.median(tb)), 2), "min": round(min(tb), 2), "max": round(max(tb), 2)},
              "speedup": round(float(np.median(ta)) / float(np.median(tb)), 2),
              "batched_median_below_in_turn_min": bool(np.median(tb) < min(ta)),
              "batched_host_enqueue_us_per_tick": round(float(np.median(enq)), 2),
              "batch_mid_ticks": [sets["in_turn"][0].batch_mid_ticks(), sets["batched"][0].batch_mid_ticks()],
              "healthy": bool(np.isfinite(sets["batched"][0].state()).all())})
        for es in sets.values():
            for e in es:
                e.close()


if __name__ == "__main__":
    main()
