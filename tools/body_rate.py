#!/usr/bin/env python3
"""Time of the body encounters (GPU box; run it under a time limit, e.g. `timeout 900 python tools/body_rate.py`).

Median wall time per call of Engine.body_encounters / Engine.batch_body_encounters (per-sample arrays and window minima, no events;
the upload of the extents and the transfer included: the host clock around calls that end in the synchronise) and, for a single
engine, the median time of the pair launch itself (its own HIP events, through csf_profile_enable: kernel 0) for

    scenes   1 024 three-rider scenes x 100 samples, one batch
    1k       1 024 riders x 100 samples
    16k8     16 384 riders x 8 samples

Every 7th road user is 4.6 x 1.8 m, the others are bicycles (tests/body_common.py: extents).  Beside each, in the same process:

    host route   the only route the parent commit offers: Engine.recorded / Engine.batch_recorded and the definition in NumPy
                 (tests/body_common.py) on the read-back.  Where that takes minutes a stated share of the (sample, receiver) rows is
                 computed and the time scaled (host_share).
    encounters   Engine.encounters / batch_encounters (discs of 0.5 m) on the same recording.

and the share of the pairs of one sample that pass each of the kernel's two filters, from a replay of the kernel's loop in NumPy
(filter_shares: every receiver of `1k`, the first 512 receivers of `16k8`, sample 0).  Pairs per second are set against the 78 TFLOP/s
vector fp64 peak at FILTER_FLOPS operations per pair.  One JSON line per shape.

    python tools/body_rate.py [--calls 7] [--shapes scenes,1k,16k8] [--out FILE]
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
import body_common as bc  # noqa: E402
from cyclistsocialforce_amd import parameters  # noqa: E402
from cyclistsocialforce_amd.engine import Engine  # noqa: E402

# csf_body.hip, body_pair where both filters fail: 4 subtractions, 3 each for w.w, c.c, w.c, 1 for rad_i + rad_j, 3 for the gap bound
# ((best + rr)^2 widened), 3 for q, 1 for b^2, 2 for the discriminant, 1 for its allowance, 3 for the bound of the ttc test - and 8
# compares, not counted.  None is an FMA (no contraction), so the kernel can reach half of a peak that counts an FMA as two.
FILTER_FLOPS = 30
# ... and body_exact behind them, nothing overlapping: 6 for cr, sr, 12 for the places, 12 for the rates, 16 for the reaches, 8 for
# sep, 8 corners x 15, 8 subtractions for the slabs - about 180 operations, 8 divisions and a square root
EXACT_FLOPS = 180
PEAK_FP64 = 78e12


def host_route(S, ext, rows=256, share=1):
    """gap_min, gap_with, ttc_min, ttc_with of states S [count, n, ns] by the definition, all n^2 pairs per sample, `rows` receivers
    at a time; share > 1: only every share-th block of receivers (the caller scales the time)"""
    count, n = S.shape[:2]
    g, gj, t, tj = np.full((count, n), np.nan), np.full((count, n), -1, np.int32), np.full((count, n), np.nan), np.full((count, n), -1, np.int32)
    block = 0
    for k in range(count):
        for lo in range(0, n, rows):
            block += 1
            if block % share:
                continue
            p = bc.pairs(S[k:k + 1], ext, rows=slice(lo, min(n, lo + rows)))
            hi = lo + p.GAP.shape[1]
            g[k, lo:hi], t[k, lo:hi] = p.GAP[0].min(axis=1), p.TTC[0].min(axis=1)
            gj[k, lo:hi] = np.where(np.isinf(g[k, lo:hi]), -1, p.GAP[0].argmin(axis=1))
            tj[k, lo:hi] = np.where(np.isinf(t[k, lo:hi]), -1, p.TTC[0].argmin(axis=1))
    return g, gj, t, tj


def filter_shares(S, ext, receivers):
    """csf_body.hip's loop over the sources of sample S [1, n, ns] for the first `receivers` road users, in NumPy: the share of the
    pairs that pass the gap filter, the ttc filter, either (= the pairs that reach body_exact)"""
    n = S.shape[1]
    x, y, psi, v = (S[0, :, c] for c in range(4))
    cs, sn = np.cos(psi), np.sin(psi)
    L, W, o = 0.5 * (ext[:, 0] + ext[:, 1]), ext[:, 2], 0.5 * (ext[:, 0] - ext[:, 1])
    mx, my, ux, uy, rad = x + o * cs, y + o * sn, v * cs, v * sn, np.sqrt(L * L + W * W)
    R = slice(0, receivers)
    best_g, best_t = np.full(receivers, np.inf), np.full(receivers, np.inf)
    true_g, true_t = best_g.copy(), best_t.copy()
    n_g = n_t = n_any = 0
    for lo in range(0, n, 256):
        p = bc.pairs(S, ext, rows=R, cols=slice(lo, min(n, lo + 256)))
        true_g, true_t = np.minimum(true_g, p.GAP[0].min(axis=1)), np.minimum(true_t, p.TTC[0].min(axis=1))
        for j in range(lo, lo + p.GAP.shape[2]):
            ok = np.arange(receivers) != j
            wx, wy, cx, cy = mx[j] - mx[R], my[j] - my[R], ux[j] - ux[R], uy[j] - uy[R]
            ww, ca, cb = wx * wx + wy * wy, cx * cx + cy * cy, wx * cx + wy * cy
            rr = rad[R] + rad[j]
            with np.errstate(invalid="ignore", over="ignore"):
                bg = best_g + rr
                f_g = ok & (best_g > 0.0) & (ww <= bg * bg * 1.000000002)
                q = ww * 0.999999998 - rr * rr
                bb = cb * cb
                meets = ok & ((q <= 0.0) | ((cb < 0.0) & (bb - ca * q >= -1e-9 * bb)))
                f_t = meets & (best_t > 0.0) & ((q <= 0.0) | (q * 0.999999 <= best_t * (-2.0 * cb)))
            go = f_g | f_t
            n_g, n_t, n_any = n_g + int(f_g.sum()), n_t + int(f_t.sum()), n_any + int(go.sum())
            G, T = p.GAP[0, :, j - lo], p.TTC[0, :, j - lo]
            best_g = np.where(go & (G < best_g), G, best_g)
            best_t = np.where(go & (T < best_t), T, best_t)
    assert np.array_equal(best_g, true_g) and np.array_equal(best_t, true_t)   # a filter changes no bit
    pairs = receivers * (n - 1)
    return {"gap": round(n_g / pairs, 4), "ttc": round(n_t / pairs, 4), "either": round(n_any / pairs, 4)}


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
    ap.add_argument("--shapes", default="scenes,1k,16k8")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    for shape in a.shapes.split(","):
        shares = None
        if shape == "scenes":
            m, n, samples, host_share = 1024, 3, 100, 1
            engines = [crowd(3, 6.0, 1000 + k, 128) for k in range(m)]
            ext = bc.extents(n)
            Engine.batch_join(engines)
            Engine.step_batch(engines, samples, sync=True)
            dev = lambda: Engine.batch_body_encounters(engines, samples, extents=[ext] * m)   # noqa: E731
            disc = lambda: Engine.batch_encounters(engines, samples, radius=0.5)   # noqa: E731

            def host():
                S = np.stack([r[0] for r in Engine.batch_recorded(engines, samples)])        # [m, samples, 3, ns]
                return bc.per_sample(S.reshape(m * samples, n, -1), ext)
            first = dev()
            ref = host()
            same = all(np.array_equal(r.gap_with, ref[1][k * samples:(k + 1) * samples]) for k, r in enumerate(first))
            host_calls = 3
        else:
            m, (n, samples, host_share, recv) = 1, {"1k": (1024, 100, 25, 1024), "16k8": (16384, 8, 64, 512)}[shape]
            e = crowd(n, 3.0 * np.sqrt(n), n, max(samples, 8))
            ext = bc.extents(n)
            e.step(samples, sync=True)
            engines = [e]
            dev = lambda: e.body_encounters(0, samples, extents=ext)   # noqa: E731
            disc = lambda: e.encounters(0, samples, radius=0.5)   # noqa: E731
            host = lambda: host_route(e.recorded(0, samples)[0], ext, share=host_share)   # noqa: E731
            first = dev()
            ref = host()
            done = ref[1] >= 0
            same = bool(done.any() and np.array_equal(first.gap_with[done], ref[1][done]))
            shares = filter_shares(e.recorded(0, 1)[0], ext, recv)
            host_calls = 1
        dev(), disc()                                                # warm-up: buffers grown, code loaded
        launch_us = disc_launch_us = None
        if m == 1:
            e.profile(1)
            e.profile_kernels()
        dev_ms = median_ms(dev, a.calls)
        if m == 1:
            launch_us = float(np.median(e.profile_samples(kernel="pair")[-a.calls:]))
            e.profile(0)
            e.profile(1)
            e.profile_kernels()
        disc_ms = median_ms(disc, a.calls)
        if m == 1:
            disc_launch_us = float(np.median(e.profile_samples(kernel="pair")[-a.calls:]))
            e.profile(0)
        host_ms = median_ms(host, host_calls) * host_share
        pairs = m * samples * n * (n - 1)
        rec = {"shape": shape, "engines": m, "riders": n, "samples": samples, "pairs": pairs, "calls": a.calls,
               "body_encounters_ms_median": round(dev_ms, 3), "pair_launch_us_median": None if launch_us is None else round(launch_us, 2),
               "encounters_ms_median": round(disc_ms, 3), "encounters_pair_launch_us_median": None if disc_launch_us is None else round(disc_launch_us, 2),
               "body_over_encounters": round(dev_ms / disc_ms, 2),
               "host_route_ms": round(host_ms, 1), "host_share": f"1/{host_share}", "host_calls": host_calls, "speed_up": round(host_ms / dev_ms, 1),
               "partners_equal_host_route": same, "filter_pass_share": shares}
        if launch_us is not None:
            rate = pairs / (launch_us * 1e-6)
            flops = FILTER_FLOPS + (shares["either"] * EXACT_FLOPS if shares else 0.0)
            rec["launch_over_encounters_launch"] = round(launch_us / disc_launch_us, 2)
            rec["pairs_per_s"] = round(rate, 0)
            rec["fp64_operations_per_pair"] = round(flops, 1)
            rec["fraction_of_fma_free_fp64_ceiling"] = round(rate * flops / (PEAK_FP64 / 2), 4)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        for e in engines:
            e.close()


if __name__ == "__main__":
    main()
