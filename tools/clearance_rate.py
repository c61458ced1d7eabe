#!/usr/bin/env python3
"""Time of the road clearance measures (GPU box; run it under a time limit, e.g. `timeout 900 python tools/clearance_rate.py`).

Host-clock time per call of Engine.clearance / Engine.batch_clearance (every array and the events; the upload of the road, the
transfer and the wait included) for the workloads of tools/flow_rate.py

    16k8     16 384 riders x 8 samples
    1k       1 024 riders x 100 samples
    scenes   1 024 three-rider scenes x 100 samples, one batch

each against the road of the curve scenario (examples/curve_force_field.curve_road: 1 530 vertices, the riders scattered in a box
around its middle), and beside each the only route the parent commit offers, in the same process: Engine.recorded /
Engine.batch_recorded and the definitions of include/csf.h in NumPy on the host (tests/clearance_common.reference), the read-back
included.  Where that takes long only a part is formed and ITS time is scaled to the whole: the first `--host-riders` road users of
a population, the first `--host-scenes` scenes of the batch; the read-back is always whole and is not scaled.  host_fraction says
what was formed.  A call is warmed up and then repeated until the window is at least `--seconds` long; the median and the mean over
the window are given.  One JSON line per shape, appended to --out (profiles/clearance_rate.txt).

    python tools/clearance_rate.py [--seconds 1.0] [--shapes 16k8,1k,scenes] [--stride 1] [--host-riders 256] [--host-scenes 16] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "examples"))
os.environ.pop("CSF_PAIR_VARIANT", None)
import clearance_common as cc  # noqa: E402
from curve_force_field import curve_road  # noqa: E402
from cyclistsocialforce_amd import parameters  # noqa: E402
from cyclistsocialforce_amd.engine import Engine, _clearance_road  # noqa: E402


def crowd(n, box, middle, seed, ring, stride):
    s0 = cc.scatter(n, box, seed)
    s0[:, :2] += np.asarray(middle) - box / 2
    e = Engine(parameters.default_pod("twod"), n)
    e.add_agents(s0, 5.0)
    e.set_dest_queue(np.arange(n), *cc.with_queue(s0), reset=True)
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
    ok = all(np.array_equal(getattr(r, f)[:, :riders], getattr(ref, f), equal_nan=True) for f in cc.CELL + cc.STATION)
    ok = ok and all(np.array_equal(getattr(r, f)[:riders], getattr(ref, f), equal_nan=True) for f in cc.USER)
    ev = r.events[r.events["i"] < riders]
    ok = ok and len(ev) == len(ref.crossings) and all(np.array_equal(ev[f], ref.crossings[f]) for f in ev.dtype.names)
    if riders == r.d_min.shape[0]:
        ok = ok and all(np.array_equal(getattr(r, f), getattr(ref, f)) for f in cc.SAMPLE)
    return bool(ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="the least length of a timing window")
    ap.add_argument("--shapes", default="16k8,1k,scenes")
    ap.add_argument("--stride", type=int, default=1, help="ticks per sample of the recording")
    ap.add_argument("--host-riders", type=int, default=256, help="road users the host route forms where all of them take long")
    ap.add_argument("--host-scenes", type=int, default=16, help="scenes of the batch the host route forms")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    road = _clearance_road("clearance_rate", [curve_road()])
    middle = (road[1].min(axis=0) + road[1].max(axis=0)) / 2
    segs = len(road[1]) - (len(road[0]) - 1)
    d_event = 1.0
    for shape in a.shapes.split(","):
        if shape == "scenes":
            m, n, samples, box = 1024, 3, 100, 6.0
            engines = [crowd(3, box, middle, 1000 + k, 128, a.stride) for k in range(m)]
            Engine.batch_join(engines)
            Engine.step_batch(engines, samples * a.stride, sync=True)
            dev = lambda: Engine.batch_clearance(engines, samples, road, d_event, events=True)   # noqa: E731
            part = min(a.host_scenes, m)
            host_fraction = part / m
            read = lambda: Engine.batch_recorded(engines, samples)                   # noqa: E731  (every scene is read back ...)
            form = lambda rec: [cc.reference(r[0], road, d_event) for r in rec[:part]]   # noqa: E731  (... `part` of them are formed)
            first = dev()
            ref = form(read())
            same = all(equal(r, w, n) for r, w in zip(first, ref))
            crossings = sum(r.n_events for r in first)
        else:
            m, (n, samples) = 1, {"1k": (1024, 100), "16k8": (16384, 8)}[shape]
            box = 3.0 * np.sqrt(n)
            e = crowd(n, box, middle, n, max(samples, 8), a.stride)
            e.step(samples * a.stride, sync=True)
            engines = [e]
            dev = lambda: e.clearance(0, samples, road, d_event, events=True)       # noqa: E731
            rows = min(a.host_riders, n)
            host_fraction = rows / n
            read = lambda: e.recorded(0, samples)[0]                                 # noqa: E731
            form = lambda S: cc.reference(S, road, d_event, limit=rows)              # noqa: E731
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
               "segments": segs, "tests": m * samples * n * segs, "crossings": int(crossings),
               "clearance_ms_median": round(dev_med, 3), "clearance_ms_mean": round(dev_mean, 3), "clearance_calls": dev_calls,
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
