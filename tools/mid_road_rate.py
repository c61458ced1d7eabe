#!/usr/bin/env python3
"""Resident time per tick of mid-size scenes WITH A ROAD (GPU box): the road term summed inside the one-launch tick
(csf_mid_road on) against the same build with the switch off - a road launch in front of every tick, and inside a batch the member
stepped in turn.  Two sets of equal engines alternate window by window in one process; calls of 100 ticks with one wait; medians of the
windows with min / max, microseconds per tick (of the whole set, for a batch).

    python tools/mid_road_rate.py single [--cells twod:64,twod:256,twod:1024,invpend:100] [--nvs 320,2048]
    python tools/mid_road_rate.py batch  [--ks 4,16,64] [--ns 100,1024] [--nvs 320]
    python tools/mid_road_rate.py plain  [--cells twod:64,twod:1024,invpend:100] [--k 64]    (no road: the untouched paths, one build -
                                          run it under CSF_LIB=<parent build> and under this one in turn, tools/ab.sh builds them)
    common: [--windows 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
for k in ("CSF_PAIR_VARIANT", "CSF_MID_ROAD"):
    os.environ.pop(k, None)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from batch_mid_rate import scene  # noqa: E402
from cyclistsocialforce_amd.engine import Engine  # noqa: E402

TICKS = 100


def with_road(e, n, nv):
    """two kerbs of nv / 2 vertices each, 3 m outside the box the riders start in, the reference's default sigma = 3"""
    box = max(30.0, 3.2 * np.sqrt(n))
    h = nv // 2
    xs = np.linspace(-20.0, box + 20.0, h)
    xs2 = np.linspace(-20.0, box + 20.0, nv - h)
    e.set_road(np.array([0, h, nv]), np.r_[np.c_[xs, np.full(h, -3.0)], np.c_[xs2, np.full(nv - h, box + 3.0)]], np.array([0.15, 0.2]), np.array([3.0, 3.0]))
    return e


def stats(w):
    return {"median": round(float(np.median(w)), 2), "min": round(min(w), 2), "max": round(max(w), 2)}


def alternate(calls, windows):
    for c in calls.values():                                      # (code objects loaded, clocks up, buffers made)
        c()
        c()
    win = {k: [] for k in calls}
    for _ in range(max(3, windows)):
        for k, c in calls.items():
            t0 = time.perf_counter()
            c()
            win[k].append((time.perf_counter() - t0) * 1e6 / TICKS)
    return win


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["single", "batch", "plain"])
    ap.add_argument("--cells", default=None)
    ap.add_argument("--nvs", default=None)
    ap.add_argument("--ks", default="4,16,64")
    ap.add_argument("--ns", default="100,1024")
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def cells(default):
        return [(c.split(":")[0], int(c.split(":")[1])) for c in (a.cells or default).split(",")]

    if a.mode == "single":
        for model, n in cells("twod:64,twod:256,twod:1024,invpend:100"):
            for nv in [int(v) for v in (a.nvs or "320,2048").split(",")]:
                es = {"two_launches": with_road(scene(model, n, 100), n, nv), "one_launch": with_road(scene(model, n, 100), n, nv)}
                es["one_launch"].mid_road(True)
                win = alternate({k: (lambda e=e: e.step(TICKS, sync=True)) for k, e in es.items()}, a.windows)
                t2, t1 = win["two_launches"], win["one_launch"]
                emit({"mode": "single", "model": model, "n": n, "nv": nv, "ticks_per_call": TICKS,
                      "two_launches_us_per_tick": stats(t2), "one_launch_us_per_tick": stats(t1),
                      "speedup": round(float(np.median(t2)) / float(np.median(t1)), 3),
                      "one_launch_median_below_two_launch_min": bool(np.median(t1) < min(t2)),
                      "mid_road_ticks": [es["two_launches"].mid_road_ticks(), es["one_launch"].mid_road_ticks()],
                      "mid_ticks": [es["two_launches"].mid_ticks(), es["one_launch"].mid_ticks()],
                      "same_state": bool(np.array_equal(es["two_launches"].state(), es["one_launch"].state()))})
                for e in es.values():
                    e.close()
    elif a.mode == "batch":
        for n in [int(v) for v in a.ns.split(",")]:
            for K in [int(v) for v in a.ks.split(",")]:
                for nv in [int(v) for v in (a.nvs or "320").split(",")]:
                    sets = {}
                    for name, on in (("in_turn", False), ("batched", True)):
                        es = [with_road(scene("twod", n, 100 + i), n, nv) for i in range(K)]
                        for e in es:
                            e.mid_road(on)
                        Engine.batch_join(es)
                        sets[name] = es
                    win = alternate({k: (lambda es=es: Engine.step_batch(es, TICKS, sync=True)) for k, es in sets.items()}, a.windows)
                    ta, tb = win["in_turn"], win["batched"]
                    emit({"mode": "batch", "model": "twod", "n": n, "K": K, "nv": nv, "ticks_per_call": TICKS,
                          "in_turn_us_per_tick": stats(ta), "batched_us_per_tick": stats(tb),
                          "speedup": round(float(np.median(ta)) / float(np.median(tb)), 2),
                          "batched_median_below_in_turn_min": bool(np.median(tb) < min(ta)),
                          "batch_mid_ticks": [sets["in_turn"][0].batch_mid_ticks(), sets["batched"][0].batch_mid_ticks()],
                          "mid_road_ticks": [sets["in_turn"][0].mid_road_ticks(), sets["batched"][0].mid_road_ticks()],
                          "same_state": bool(np.array_equal(sets["in_turn"][0].state(), sets["batched"][0].state()))})
                    for es in sets.values():
                        for e in es:
                            e.close()
    else:
        lib = os.environ.get("CSF_LIB", "this build")
        for model, n in cells("twod:64,twod:1024,invpend:100"):
            e = scene(model, n, 100)
            win = alternate({"one_launch": lambda: e.step(TICKS, sync=True)}, a.windows)["one_launch"]
            emit({"mode": "plain", "lib": lib, "model": model, "n": n, "us_per_tick": stats(win), "mid_ticks": e.mid_ticks()})
            e.close()
        es = [scene("twod", 100, 100 + i) for i in range(a.k)]
        Engine.batch_join(es)
        win = alternate({"batched": lambda: Engine.step_batch(es, TICKS, sync=True)}, a.windows)["batched"]
        emit({"mode": "plain", "lib": lib, "model": "twod", "n": 100, "K": a.k, "us_per_tick": stats(win), "batch_mid_ticks": es[0].batch_mid_ticks()})
        for e in es:
            e.close()


if __name__ == "__main__":
    main()
