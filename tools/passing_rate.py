#!/usr/bin/env python3
"""Time of the following and passing measures (GPU box; run it under a time limit, e.g. `timeout 900 python tools/passing_rate.py`).

Median wall time per call of Engine.passing / Engine.batch_passing (per-station and per-interval arrays and the road users' rows,
no events; the transfer included) and, for a single engine, the median time of the main launch itself (its own HIP events, through
csf_profile_enable: kernel 0) for the workloads of tools/encounter_rate.py

    scenes   1 024 three-rider scenes x 100 samples, one batch
    1k       1 024 riders x 100 samples
    16k8     16 384 riders x 8 samples

and beside each the only route the parent commit offers, in the same process: Engine.recorded / Engine.batch_recorded and the
definitions of include/csf.h in NumPy on the host (tests/passing_common.reference, station by station).  Where that takes minutes
only a part is formed and the time is scaled to the whole: the first `--host-riders` road users as followers and passers of a
population, the first `--host-scenes` scenes of the batch; host_fraction says what was timed.  Ordered pairs per second count
every (station, i, j != i) once - the kernel forms both directions of a passing for it (PAIR_FLOPS fp64 operations, none of them
an FMA).  One JSON line per shape.

    python tools/passing_rate.py [--calls 7] [--shapes scenes,1k,16k8] [--stride 1] [--host-riders 128] [--host-scenes 32] [--out FILE]
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
import passing_common as pc  # noqa: E402
from cyclistsocialforce_amd import parameters  # noqa: E402
from cyclistsocialforce_amd.engine import Engine  # noqa: E402

# csf_passing.hip: eight differences and five terms of two products and a sum per ordered pair and station
PAIR_FLOPS = 23
PEAK_FP64 = 78e12
BAND, LAT_MAX = 0.75, 3.0


def crowd(n, box, seed, ring, stride):
    s0 = pc.scatter(n, box, seed)
    e = Engine(parameters.default_pod("twod"), n)
    e.add_agents(s0, 5.0)
    e.set_dest_queue(np.arange(n), *pc.with_queue(s0), reset=True)
    e.record(stride=stride, capacity=ring, forces=False)
    return e


def median_ms(f, calls):
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def equal(r, ref, riders=None):
    """the device's rows of what the passer or follower reports against the reference's, bit for bit (riders: the road users the
    reference formed)"""
    k = ref.gap.shape[1] if riders is None else riders
    return bool(all(np.array_equal(getattr(r, f)[:, :k], getattr(ref, f)[:, :k], equal_nan=True)
                    for f in ("gap", "gap_with", "thw", "made_lat", "made_with", "made_t", "made_kind")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--shapes", default="scenes,1k,16k8")
    ap.add_argument("--stride", type=int, default=1, help="ticks per sample of the recording (1: encounter_rate's)")
    ap.add_argument("--host-riders", type=int, default=128, help="followers and passers the host route forms where all of them take minutes")
    ap.add_argument("--host-scenes", type=int, default=32, help="scenes of the batch the host route forms")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    for shape in a.shapes.split(","):
        if shape == "scenes":
            m, n, samples = 1024, 3, 100
            engines = [crowd(3, 6.0, 1000 + k, 128, a.stride) for k in range(m)]
            Engine.batch_join(engines)
            Engine.step_batch(engines, samples * a.stride, sync=True)
            dev = lambda: Engine.batch_passing(engines, samples, BAND, LAT_MAX)   # noqa: E731
            part = min(a.host_scenes, m)
            host_fraction = part / m

            def host():                                          # (every scene is read back; `part` of them are formed)
                return [pc.reference(r[0], BAND, LAT_MAX) for r in Engine.batch_recorded(engines, samples)[:part]]
            first = dev()
            ref = host()
            same = all(equal(r, w) and np.array_equal(r.by_lat, w.by_lat) for r, w in zip(first, ref))
            passings = sum(int(r.run_made.sum()) for r in first)
            launch_us = None
        else:
            m, (n, samples) = 1, {"1k": (1024, 100), "16k8": (16384, 8)}[shape]
            e = crowd(n, 3.0 * np.sqrt(n), n, max(samples, 8), a.stride)
            e.step(samples * a.stride, sync=True)
            engines = [e]
            dev = lambda: e.passing(0, samples, BAND, LAT_MAX)       # noqa: E731
            rows = min(a.host_riders, n)
            host_fraction = rows / n
            host = lambda: pc.reference(e.recorded(0, samples)[0], BAND, LAT_MAX, limit=rows)   # noqa: E731
            first = dev()
            ref = host()
            same = equal(first, ref, rows)
            passings = int(first.run_made.sum())
        dev()                                                        # warm-up: buffers grown, code loaded
        if m == 1:
            e.profile(1)
            e.profile_kernels()
        dev_ms = median_ms(dev, a.calls)
        if m == 1:
            launch_us = float(np.median(e.profile_samples(kernel="pair")))
            e.profile(0)
        host_ms = median_ms(host, 1) / host_fraction
        pairs = m * (samples - 1) * n * (n - 1)
        rec = {"shape": shape, "engines": m, "riders": n, "samples": samples, "stride": a.stride, "stations": m * (samples - 1) * n,
               "ordered_pairs": pairs, "passings": passings, "calls": a.calls, "passing_ms_median": round(dev_ms, 3),
               "main_launch_us_median": None if launch_us is None else round(launch_us, 2),
               "host_route_ms": round(host_ms, 1), "host_fraction": round(host_fraction, 6),
               "speed_up": round(host_ms / dev_ms, 1), "rows_equal_host_route": same}
        if launch_us is not None:
            rate = pairs / (launch_us * 1e-6)
            rec["pairs_per_s"] = round(rate, 0)
            rec["fraction_of_fp64_vector_peak"] = round(rate * PAIR_FLOPS / PEAK_FP64, 4)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        for e in engines:
            e.close()


if __name__ == "__main__":
    main()
