#!/usr/bin/env python3
"""Resident time per tick of K independent small scenes (GPU box): one batch (csf_step_batch: one launch per vehicle class for
every one-wave member) against the same K engines stepped in turn by csf_step.  Scenes of 3, 16 and 32 TwoDBicycle and of 3
BalancingRiderBicycle; calls of 100 ticks, and calls of 1 tick with the read-back (what step_together does every tick).  Medians over
repeated windows after a warm-up; the host time of one batched call (enqueue only, and with its wait) as well.  One JSON line per
(scene, K, mode).

    python tools/batch_rate.py [--ks 1,16,256,1024,4096] [--scenes twod3,twod16,twod32,br3] [--windows 5] [--out FILE]
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

SCENES = {"twod3": ("twod", 3), "twod16": ("twod", 16), "twod32": ("twod", 32), "br3": ("balancingrider", 3)}


def scene(model, n, seed):
    """n riders in a box at the density of the reference's demos, heading for destinations 50 .. 150 m out"""
    rng = np.random.default_rng(seed)
    box = 14.0 if n <= 8 else 30.0
    if model == "balancingrider":
        box *= 2.0
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


def median_us(fn, ticks, windows, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(windows):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e6 / ticks, [round(t * 1e6 / ticks, 3) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,16,256,1024,4096")
    ap.add_argument("--scenes", default="twod3,twod16,twod32,br3")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for name in a.scenes.split(","):
        model, n = SCENES[name]
        engines = [scene(model, n, 100 + i) for i in range(max(ks))]
        for e in engines[:4]:
            e.step(50, sync=True)                                # (code objects loaded, clocks up)
        for K in ks:
            es = engines[:K]
            bufs = [(np.zeros((n, e.ns)), np.zeros(n, dtype=np.int32), np.zeros((n, 3), dtype=np.uint8), np.zeros(n), np.zeros(n)) for e in es]
            win = a.windows if K <= 1024 else max(3, a.windows - 2)
            # in turn: csf_step on every engine, one wait at the end (100 ticks) / csf_step_get_tick on every engine (1 tick)
            def turn100():
                for e in es:
                    e.step(100)
                for e in es:
                    e.sync()

            def turn1():
                for e, b in zip(es, bufs):
                    e.step_into(1, *b)

            us_t100, w_t100 = median_us(turn100, 100, win)
            us_t1, w_t1 = median_us(turn1, 1, win * 4)
            Engine.batch_join(es)
            bt0 = es[0].batch_ticks()

            def batch100():
                Engine.step_batch(es, 100, sync=True)

            def batch1():
                Engine.step_batch_into(es, 1, bufs)

            us_b100, w_b100 = median_us(batch100, 100, win)
            us_b1, w_b1 = median_us(batch1, 1, win * 4)
            # host time of one batched call: enqueue only (100 ticks, no wait), and the waited call is the 1-tick read-back above
            enq = []
            for _ in range(win):
                t0 = time.perf_counter()
                Engine.step_batch(es, 100)
                enq.append(time.perf_counter() - t0)
                es[0].sync()
            batched = es[0].batch_ticks() - bt0
            Engine.batch_leave(es)
            for mode, us_t, us_b, wt, wb in (("100_ticks", us_t100, us_b100, w_t100, w_b100), ("1_tick_readback", us_t1, us_b1, w_t1, w_b1)):
                emit({"scene": name, "model": model, "n": n, "K": K, "mode": mode, "in_turn_us_per_tick": round(us_t, 3),
                      "batch_us_per_tick": round(us_b, 3), "speedup": round(us_t / us_b, 2), "batch_us_per_scene_tick": round(us_b / K, 4),
                      "in_turn_windows": wt, "batch_windows": wb})
            emit({"scene": name, "K": K, "mode": "host_enqueue_100_ticks", "batch_call_host_us": round(float(np.median(enq)) * 1e6, 2),
                  "per_member_host_us": round(float(np.median(enq)) * 1e6 / K, 4), "member0_batch_ticks": batched})
        for e in engines:
            e.close()


if __name__ == "__main__":
    main()
