#!/usr/bin/env python3
"""Time of the flow measures (GPU box; run it under a time limit, e.g. `timeout 900 python tools/flow_rate.py`).

Host-clock time per call of Engine.flow / Engine.batch_flow (every array and the events; the transfer and the wait included) for
the workloads of tools/passing_rate.py

    16k8     16 384 riders x 8 samples
    1k       1 024 riders x 100 samples
    scenes   1 024 three-rider scenes x 100 samples, one batch

each at the five lines and three areas of tests/flow_common.layout and a grid of 64 x 64 cells, and beside each the only route the
parent commit offers, in the same process: Engine.recorded / Engine.batch_recorded and the definitions of include/csf.h in NumPy on
the host (tests/flow_common.reference), the read-back included.  Where that takes long only a part is formed and ITS time is scaled
to the whole: the first `--host-riders` road users of a population, the first `--host-scenes` scenes of the batch; the read-back is
always whole and is not scaled.  host_fraction says what was formed.  A call is warmed up and then repeated until the window is at least `--seconds`
long; the median and the mean over the window are given.  One JSON line per shape, appended to --out (profiles/flow_rate.txt).

    python tools/flow_rate.py [--seconds 1.0] [--shapes 16k8,1k,scenes] [--stride 1] [--host-riders 2048] [--host-scenes 64] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.pop("CSF_PAIR_VARIANT", None)
import flow_common as fc  # noqa: E402
from cyclistsocialforce_amd import parameters  # noqa: E402
from cyclistsocialforce_amd.engine import Engine  # noqa: E402


def crowd(n, box, seed, ring, stride):
    s0 = fc.scatter(n, box, seed)
    e = Engine(parameters.default_pod("twod"), n)
    e.add_agents(s0, 5.0)
    e.set_dest_queue(np.arange(n), *fc.with_queue(s0), reset=True)
    e.record(stride=stride, capacity=ring, forces=False)
    return e


def window_ms(f, seconds):
    """(median, mean, calls) of f's wall time in ms over a window of at least `seconds`"""
    ts = []
    t_end = time.perf_counter() + seconds
    while not ts or time.perf_counter() < t_end:
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, float(np.mean(ts)) * 1e3, len(ts)


def equal(r, ref, riders):
    """the device's arrays against the reference's over the road users the reference formed, bit for bit"""
    per_user = ("cross_n", "first_t", "first_u", "first_speed", "first_dir", "in_samples", "in_first", "in_last", "in_dist")
    ok = all(np.array_equal(getattr(r, f)[:riders], getattr(ref, f), equal_nan=True) for f in per_user)
    if riders == r.cross_n.shape[0]:
        ok = ok and all(np.array_equal(getattr(r, f), getattr(ref, f)) for f in ("line_count", "occupancy", "grid_count")) and r.n_outside == ref.n_outside
    return bool(ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="the least length of a timing window")
    ap.add_argument("--shapes", default="16k8,1k,scenes")
    ap.add_argument("--stride", type=int, default=1, help="ticks per sample of the recording")
    ap.add_argument("--host-riders", type=int, default=2048, help="road users the host route forms where all of them take long")
    ap.add_argument("--host-scenes", type=int, default=64, help="scenes of the batch the host route forms")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    for shape in a.shapes.split(","):
        if shape == "scenes":
            m, n, samples, box = 1024, 3, 100, 6.0
            lines, areas, grid = fc.layout(box)
            grid = (0.0, 0.0, box / 64, 64, 64)
            engines = [crowd(3, box, 1000 + k, 128, a.stride) for k in range(m)]
            Engine.batch_join(engines)
            Engine.step_batch(engines, samples * a.stride, sync=True)
            dev = lambda: Engine.batch_flow(engines, samples, lines, areas, grid, events=True)   # noqa: E731
            part = min(a.host_scenes, m)
            host_fraction = part / m

            read = lambda: Engine.batch_recorded(engines, samples)                   # noqa: E731  (every scene is read back ...)
            form = lambda rec: [fc.reference(r[0], lines, areas, grid) for r in rec[:part]]   # noqa: E731  (... `part` of them are formed)
            first = dev()
            ref = form(read())
            same = all(equal(r, w, n) for r, w in zip(first, ref))
            crossings = sum(r.n_events for r in first)
        else:
            m, (n, samples) = 1, {"1k": (1024, 100), "16k8": (16384, 8)}[shape]
            box = 3.0 * np.sqrt(n)
            lines, areas, grid = fc.layout(box)
            grid = (0.0, 0.0, box / 64, 64, 64)
            e = crowd(n, box, n, max(samples, 8), a.stride)
            e.step(samples * a.stride, sync=True)
            engines = [e]
            dev = lambda: e.flow(0, samples, lines, areas, grid, events=True)       # noqa: E731
            rows = min(a.host_riders, n)
            host_fraction = rows / n
            read = lambda: e.recorded(0, samples)[0]                                 # noqa: E731
            form = lambda S: fc.reference(S, lines, areas, grid, limit=rows)         # noqa: E731
            first = dev()
            ref = form(read())
            same = equal(first, ref, rows)
            crossings = first.n_events
        dev()                                                        # warm-up: buffers grown, code loaded
        dev_med, dev_mean, dev_calls = window_ms(dev, a.seconds)
        read_med, _, _ = window_ms(read, a.seconds)
        kept = read()
        form_med, _, host_calls = window_ms(lambda: form(kept), a.seconds)
        host_ms = read_med + form_med / host_fraction               # the read-back is whole; what was formed of it is scaled
        rec = {"shape": shape, "engines": m, "riders": n, "samples": samples, "stride": a.stride, "cells": m * samples * n,
               "lines": len(lines), "areas": len(areas), "grid": [grid[3], grid[4]], "crossings": int(crossings),
               "flow_ms_median": round(dev_med, 3), "flow_ms_mean": round(dev_mean, 3), "flow_calls": dev_calls,
               "host_route_ms": round(host_ms, 1), "read_back_ms": round(read_med, 3), "host_route_calls": host_calls,
               "host_fraction": round(host_fraction, 6), "speed_up": round(host_ms / dev_med, 1), "rows_equal_host_route": same}
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        for e in engines:
            e.close()


if __name__ == "__main__":
    main()
