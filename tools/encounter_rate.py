#!/usr/bin/env python3
"""Time of the encounter measures (GPU box; run it under a time limit, e.g. `timeout 900 python tools/encounter_rate.py`).

Median wall time per call of Engine.encounters / Engine.batch_encounters (per-sample arrays and window minima, no events; the
transfer included) and, for a single engine, the median time of the pair launch itself (its own HIP events, through
csf_profile_enable: kernel 0) for

    scenes   1 024 three-rider scenes x 100 samples, one batch
    1k       1 024 riders x 100 samples
    16k      16 384 riders x 1 sample
    16k8     16 384 riders x 8 samples

and beside each the only route the parent commit offers, in the same process: Engine.recorded / Engine.batch_recorded and the
definitions of include/csf.h in NumPy on the host (host_route below; one call where a call takes seconds - host_calls says how many).
Pairs per second are set against the 78 TFLOP/s vector fp64 peak at 20 fp64 operations per pair (PAIR_FLOPS).  One JSON line per shape.

    python tools/encounter_rate.py [--calls 7] [--shapes scenes,1k,16k,16k8] [--out FILE]
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
from cyclistsocialforce_amd import parameters  # noqa: E402
from cyclistsocialforce_amd.engine import Engine  # noqa: E402

RADIUS = 0.5
# csf_encounter.hip, enc_pair where nothing is near: 4 subtractions, 3 each for w.w, c.c, w.c, 1 for q, 3 for the discriminant, 3 for
# the bound of the ttc test - and 6 compares, not counted.  None of them is an FMA (no contraction), so the kernel can reach half
# of a peak that counts an FMA as two.
PAIR_FLOPS = 20
PEAK_FP64 = 78e12


def host_route(S, radius, rows=1024):
    """d_min, d_with, ttc_min, ttc_with [count, n] of states S [count, n, ns]: the definitions, all n^2 pairs per sample, `rows`
    receivers at a time"""
    count, n = S.shape[:2]
    d, dj, t, tj = np.empty((count, n)), np.empty((count, n), np.int32), np.empty((count, n)), np.empty((count, n), np.int32)
    R2 = (2.0 * radius) ** 2
    for k in range(count):
        x, y, psi, v = S[k, :, 0], S[k, :, 1], S[k, :, 2], S[k, :, 3]
        ux, uy = v * np.cos(psi), v * np.sin(psi)
        for lo in range(0, n, rows):
            hi = min(n, lo + rows)
            wx, wy = x[None, :] - x[lo:hi, None], y[None, :] - y[lo:hi, None]
            cx, cy = ux[None, :] - ux[lo:hi, None], uy[None, :] - uy[lo:hi, None]
            ww, a, b = wx * wx + wy * wy, cx * cx + cy * cy, wx * cx + wy * cy
            q = ww - R2
            disc = b * b - a * q
            with np.errstate(invalid="ignore", divide="ignore"):
                T = np.where(q <= 0, 0.0, np.where((b >= 0) | (a == 0) | (disc < 0), np.inf, q / (-b + np.sqrt(np.maximum(disc, 0.0)))))
            D = np.sqrt(ww)
            own = np.arange(lo, hi)
            D[own - lo, own] = np.inf
            T[own - lo, own] = np.inf
            d[k, lo:hi], t[k, lo:hi] = D.min(axis=1), T.min(axis=1)
            dj[k, lo:hi] = np.where(np.isinf(d[k, lo:hi]), -1, D.argmin(axis=1))
            tj[k, lo:hi] = np.where(np.isinf(t[k, lo:hi]), -1, T.argmin(axis=1))
    return d, dj, t, tj


def crowd(n, box, seed, ring):
    rng = np.random.default_rng(seed)
    s0 = np.zeros((n, 5))
    s0[:, 0], s0[:, 1] = rng.uniform(0, box, n), rng.uniform(0, box, n)
    s0[:, 2], s0[:, 3] = rng.uniform(-np.pi, np.pi, n), rng.uniform(3, 6, n)
    ahead = np.array([50.0, 99.0, 100.0])
    dq = np.zeros((n, 4, 3))
    dq[:, 0, 0], dq[:, 0, 1] = s0[:, 0], s0[:, 1]
    dq[:, 1:, 0] = s0[:, 0, None] + ahead[None, :] * np.cos(s0[:, 2])[:, None]
    dq[:, 1:, 1] = s0[:, 1, None] + ahead[None, :] * np.sin(s0[:, 2])[:, None]
    e = Engine(parameters.default_pod("twod"), n)
    e.add_agents(s0, 5.0)
    e.set_dest_queue(np.arange(n), np.arange(n + 1) * 4, dq.reshape(-1, 3), reset=True)
    e.record(stride=1, capacity=ring, forces=False)
    return e


def median_ms(f, calls):
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--shapes", default="scenes,1k,16k,16k8")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    for shape in a.shapes.split(","):
        if shape == "scenes":
            m, n, samples = 1024, 3, 100
            engines = [crowd(3, 6.0, 1000 + k, 128) for k in range(m)]
            Engine.batch_join(engines)
            Engine.step_batch(engines, samples, sync=True)
            dev = lambda: Engine.batch_encounters(engines, samples, radius=RADIUS)   # noqa: E731

            def host():
                S = np.stack([r[0] for r in Engine.batch_recorded(engines, samples)])        # [m, samples, 3, ns]
                return host_route(S.reshape(m * samples, n, -1), RADIUS)
            host_calls = a.calls
            first = dev()
            ref = host()
            same = all(np.array_equal(r.d_with, ref[1][k * samples:(k + 1) * samples]) for k, r in enumerate(first))
            launch_us = None
        else:
            m, (n, samples) = 1, {"1k": (1024, 100), "16k": (16384, 1), "16k8": (16384, 8)}[shape]
            e = crowd(n, 3.0 * np.sqrt(n), n, max(samples, 8))
            e.step(samples, sync=True)
            engines = [e]
            dev = lambda: e.encounters(0, samples, radius=RADIUS)   # noqa: E731
            host = lambda: host_route(e.recorded(0, samples)[0], RADIUS)   # noqa: E731
            host_calls = a.calls if n * n * samples <= 2e8 else 1
            first = dev()
            ref = host() if host_calls > 1 else None
            same = None if ref is None else bool(np.array_equal(first.d_with, ref[1]))
        dev()                                                        # warm-up: buffers grown, code loaded
        if m == 1:
            e.profile(1)
            e.profile_kernels()
        dev_ms = median_ms(dev, a.calls)
        if m == 1:
            launch_us = float(np.median(e.profile_samples(kernel="pair")))
            e.profile(0)
        if host_calls == 1:
            t0 = time.perf_counter()
            ref = host()
            host_ms = (time.perf_counter() - t0) * 1e3
            same = bool(np.array_equal(first.d_with, ref[1]))
        else:
            host_ms = median_ms(host, host_calls)
        pairs = m * samples * n * (n - 1)
        rec = {"shape": shape, "engines": m, "riders": n, "samples": samples, "pairs": pairs, "calls": a.calls,
               "encounters_ms_median": round(dev_ms, 3), "pair_launch_us_median": None if launch_us is None else round(launch_us, 2),
               "host_route_ms": round(host_ms, 1), "host_calls": host_calls, "speed_up": round(host_ms / dev_ms, 1),
               "partners_equal_host_route": same}
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
