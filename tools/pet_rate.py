#!/usr/bin/env python3
"""Time of the post-encroachment measures (GPU box; run it under a time limit, e.g. `timeout 900 python tools/pet_rate.py`).

Median wall time per call of Engine.post_encroachment / Engine.batch_post_encroachment (per-segment arrays and the road users' rows,
no events; the transfer included) and, for a single engine, the median time of the main launch itself (its own HIP events, through
csf_profile_enable: kernel 0) for the workloads of tools/encounter_rate.py

    scenes   1 024 three-rider scenes x 100 samples, one batch
    1k       1 024 riders x 100 samples
    16k8     16 384 riders x 8 samples

and beside each the only route the parent commit offers, in the same process: Engine.recorded / Engine.batch_recorded and the
definitions of include/csf.h in NumPy on the host (tests/pet_common.reference, chunked over own segments).  Where that takes minutes
only the first `--host-segments` own segments are formed and the time is scaled to all of them: host_fraction says what was timed.
Segment tests per second are set against the 78 TFLOP/s vector fp64 peak at the 9 operations of den, ns and nt per test (TEST_FLOPS)
- a nominal figure: the box test, four compares, comes first and lets most tests skip the 9 operations.  One JSON line per shape.

    python tools/pet_rate.py [--calls 7] [--shapes scenes,1k,16k8] [--stride 1] [--host-segments 512] [--out FILE]
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
import pet_common as pc  # noqa: E402
from cyclistsocialforce_amd import parameters  # noqa: E402
from cyclistsocialforce_amd.engine import Engine  # noqa: E402

# csf_pet.hip: two products and a subtraction for each of den, ns, nt.  None of them is an FMA (no contraction), so the kernel can
# reach half of a peak that counts an FMA as two.
TEST_FLOPS = 9
PEAK_FP64 = 78e12


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


def equal(r, ref, rows=None):
    """the device's rows against the reference's, bit for bit (rows: the own segments the reference formed)"""
    m, n = ref.seg_pet.shape
    got, want = r.seg_pet.ravel(), ref.seg_pet.ravel()
    gw, ww = r.seg_with.ravel(), ref.seg_with.ravel()
    k = m * n if rows is None else min(rows, m * n)
    return bool(np.array_equal(got[:k], want[:k], equal_nan=True) and np.array_equal(gw[:k], ww[:k]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--shapes", default="scenes,1k,16k8")
    ap.add_argument("--stride", type=int, default=1, help="ticks per sample of the recording (1: encounter_rate's)")
    ap.add_argument("--host-segments", type=int, default=512, help="own segments the host route forms where all of them take minutes")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    for shape in a.shapes.split(","):
        host_fraction = 1.0
        if shape == "scenes":
            m, n, samples = 1024, 3, 100
            engines = [crowd(3, 6.0, 1000 + k, 128, a.stride) for k in range(m)]
            Engine.batch_join(engines)
            Engine.step_batch(engines, samples * a.stride, sync=True)
            dev = lambda: Engine.batch_post_encroachment(engines, samples)   # noqa: E731

            def host():
                return [pc.reference(r[0]) for r in Engine.batch_recorded(engines, samples)]
            first = dev()
            ref = host()
            same = all(equal(r, w) for r, w in zip(first, ref))
            crossings = sum(int(w.run_count.sum()) for w in ref)
            host_calls = min(a.calls, 3)
            launch_us = None
        else:
            m, (n, samples) = 1, {"1k": (1024, 100), "16k8": (16384, 8)}[shape]
            e = crowd(n, 3.0 * np.sqrt(n), n, max(samples, 8), a.stride)
            e.step(samples * a.stride, sync=True)
            engines = [e]
            dev = lambda: e.post_encroachment(0, samples)            # noqa: E731
            segs = (samples - 1) * n
            rows = min(a.host_segments, segs)
            host_fraction = rows / segs
            host = lambda: pc.reference(e.recorded(0, samples)[0], limit=rows)   # noqa: E731
            first = dev()
            ref = host()
            same = equal(first, ref, rows)
            crossings = int(first.run_count.sum())
            host_calls = 1
        dev()                                                        # warm-up: buffers grown, code loaded
        if m == 1:
            e.profile(1)
            e.profile_kernels()
        dev_ms = median_ms(dev, a.calls)
        if m == 1:
            launch_us = float(np.median(e.profile_samples(kernel="pair")))
            e.profile(0)
        host_ms = median_ms(host, host_calls) / host_fraction
        segs = m * (samples - 1) * n
        tests = m * ((samples - 1) * n) * ((samples - 1) * (n - 1))
        rec = {"shape": shape, "engines": m, "riders": n, "samples": samples, "stride": a.stride, "segments": segs, "segment_tests": tests,
               "crossings": crossings, "calls": a.calls, "pet_ms_median": round(dev_ms, 3),
               "main_launch_us_median": None if launch_us is None else round(launch_us, 2),
               "host_route_ms": round(host_ms, 1), "host_calls": host_calls, "host_fraction": round(host_fraction, 6),
               "speed_up": round(host_ms / dev_ms, 1), "rows_equal_host_route": same}
        if launch_us is not None:
            rate = tests / (launch_us * 1e-6)
            rec["tests_per_s"] = round(rate, 0)
            rec["fraction_of_fp64_vector_peak"] = round(rate * TEST_FLOPS / PEAK_FP64, 4)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        for e in engines:
            e.close()


if __name__ == "__main__":
    main()
