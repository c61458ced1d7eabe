#!/usr/bin/env python3
"""Resident time per tick of MIXED mid-size scenes (GPU box): several parameter sets, several vehicle classes, scripted
UncontrolledVehicles - ticked in one launch (csf_mid_classes on; csf_mid_classes.hip) against the same build with the switch off: the general
path, a pair launch and a per-agent launch per class every tick (what the parent commit takes), and inside a batch the member stepped in
turn.  Two sets of equal engines alternate window by window in one process; calls of 100 ticks with one wait; medians of the windows with
min / max, microseconds per tick (of the whole set, for a batch).

    python tools/mid_classes_rate.py single [--ns 64,256,600,1024,1279] [--kinds two,sets32,five,cars] [--nvs 0,320]
    python tools/mid_classes_rate.py batch  [--ks 4,16,64] [--n 100]
    python tools/mid_classes_rate.py plain  [--cells twod:64,twod:1024] [--k 64]      (the untouched paths, one build - run it under
                                             CSF_LIB=<parent build> and under this one in turn, tools/ab.sh builds them)
    common: [--windows 5] [--out FILE]

kinds: two     two TwoD sets, dealt alternately
       sets32  32 TwoD sets (one class: one pass of the per-agent phases)
       five    five classes, ten sets, drawn at random (tests/test_gpu_hetero.py::test_random_mixed_population_vs_oracle)
       cars    four cyclists' classes and every eighth road user a scripted UncontrolledVehicle
       three   twod, bicycle, planarpoint dealt in turn (the batch's members)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
for k in ("CSF_PAIR_VARIANT", "CSF_MID_ROAD", "CSF_MID_CLASSES", "CSF_MID_BELOW"):
    os.environ.pop(k, None)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from batch_mid_rate import scene  # noqa: E402
from mid_road_rate import alternate, stats, with_road  # noqa: E402
from cyclistsocialforce_amd import _ffi, parameters  # noqa: E402
from cyclistsocialforce_amd.engine import Engine  # noqa: E402

TICKS = 100
ORDER = ("twod", "bicycle", "invpend", "planarpoint", "planarbike")
OWN = {"twod": dict(hfov=1.0, f_0=10.0), "bicycle": dict(hfov=3.4, p_0=40.0, p_decay=4.0), "invpend": dict(hfov=2.5, e_0=0.9, k_p_v=12.0, v_max_walk=3.5),
       "planarpoint": dict(hfov=1.5, f_0=5.0, poles=[-3.0 + 0j]), "planarbike": dict(hfov=2.8, sigma_0=0.6)}


def sets_of(kind, n, rng):
    """(parameter sets, the set of every road user, slots of scripted cars)"""
    cars = np.zeros(0, dtype=int)
    if kind == "two":
        pods, cls = [parameters.default_pod("twod"), parameters.default_pod("twod", f_0=8.0, hfov=2.0)], np.arange(n) % 2
    elif kind == "sets32":
        pods = [parameters.default_pod("twod", hfov=2.0 + 0.03 * k, f_0=5.0 + 0.1 * k) for k in range(32)]
        cls = np.arange(n) % 32
    elif kind == "five":
        pods = [parameters.default_pod(m) for m in ORDER] + [parameters.default_pod(m, **OWN[m]) for m in ORDER]
        cls = rng.integers(0, len(pods), n)
    elif kind == "cars":
        pods = [parameters.default_pod(m) for m in ("twod", "bicycle", "invpend", "planarpoint")] + [parameters.default_pod("uncontrolled", hfov=2.5, f_0=9.0)]
        cls = np.arange(n) % 4
        cars = np.arange(3, n, 8)
        cls[cars] = 4
    elif kind == "three":
        pods, cls = [parameters.default_pod(m) for m in ("twod", "bicycle", "planarpoint")], np.arange(n) % 3
    else:
        raise KeyError(kind)
    return pods, np.asarray(cls, dtype=np.int32), cars


def mixed_scene(kind, n, seed, on, nv=0):
    """batch_mid_rate.scene's crowd with the sets of `kind`; the cars drive their start heading at their start speed for 100 000 ticks"""
    rng = np.random.default_rng(seed)
    box = max(30.0, 3.2 * np.sqrt(n))
    x, y = rng.uniform(0, box, n), rng.uniform(0, box, n)
    psi, v = rng.uniform(-np.pi, np.pi, n), rng.uniform(3, 4.8, n)
    reach = np.array([50.0, 100.0, 150.0])
    dq = np.zeros((n, 4, 3))
    dq[:, 0, 0], dq[:, 0, 1] = x, y
    dq[:, 1:, 0] = x[:, None] + reach * np.cos(psi)[:, None]
    dq[:, 1:, 1] = y[:, None] + reach * np.sin(psi)[:, None]
    pods, cls, cars = sets_of(kind, n, rng)
    ns = max(_ffi.N_STATES[p.model] for p in pods)
    s0 = np.zeros((n, ns))
    s0[:, 0], s0[:, 1], s0[:, 2], s0[:, 3] = x, y, psi, v
    e = Engine(pods[0], n)
    e.mid_classes(on)
    e.set_param_classes(pods)
    e.add_agents(s0, 5.0)
    e.set_dest_queue(np.arange(n), np.arange(n + 1) * 4, dq.reshape(-1, 3), reset=True)
    e.set_agent_class(np.arange(n), cls)
    if len(cars):
        t = np.arange(4096) * 0.01                                 # (a script that ends leaves the car where it is: vehicle.py:964-979)
        rows = np.concatenate([np.c_[x[j] + v[j] * t * np.cos(psi[j]), y[j] + v[j] * t * np.sin(psi[j]), np.full(t.size, psi[j]), np.full(t.size, v[j])] for j in cars])
        e.set_script(cars, np.arange(len(cars) + 1) * t.size, rows)
    if nv:
        with_road(e, n, nv)
        e.mid_road(on)                                             # (the one launch sums the road too; off: road_kernel in front, as the parent)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["single", "batch", "plain"])
    ap.add_argument("--ns", default="64,256,600,1024,1279")
    ap.add_argument("--kinds", default="two,sets32,five,cars")
    ap.add_argument("--nvs", default="0,320")
    ap.add_argument("--ks", default="4,16,64")
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--cells", default="twod:64,twod:1024")
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

    if a.mode == "single":
        for kind in a.kinds.split(","):
            for n in [int(v) for v in a.ns.split(",")]:
                for nv in [int(v) for v in a.nvs.split(",")]:
                    es = {"general": mixed_scene(kind, n, 100, False, nv), "one_launch": mixed_scene(kind, n, 100, True, nv)}
                    win = alternate({k: (lambda e=e: e.step(TICKS, sync=True)) for k, e in es.items()}, a.windows)
                    tg, t1 = win["general"], win["one_launch"]
                    sg, s1 = es["general"].state(), es["one_launch"].state()
                    emit({"mode": "single", "kind": kind, "n": n, "nv": nv, "ticks_per_call": TICKS,
                          "general_us_per_tick": stats(tg), "one_launch_us_per_tick": stats(t1),
                          "speedup": round(float(np.median(tg)) / float(np.median(t1)), 3),
                          "one_launch_median_below_general_min": bool(np.median(t1) < min(tg)),
                          "mid_classes_ticks": [es["general"].mid_classes_ticks(), es["one_launch"].mid_classes_ticks()],
                          "mid_ticks": [es["general"].mid_ticks(), es["one_launch"].mid_ticks()],
                          "finite": bool(np.isfinite(s1).all() and np.isfinite(sg).all())})
                    for e in es.values():
                        e.close()
    elif a.mode == "batch":
        for K in [int(v) for v in a.ks.split(",")]:
            sets = {}
            for name, on in (("in_turn", False), ("batched", True)):
                es = [mixed_scene("three", a.n, 100 + i, on) for i in range(K)]
                Engine.batch_join(es)
                sets[name] = es
            win = alternate({k: (lambda es=es: Engine.step_batch(es, TICKS, sync=True)) for k, es in sets.items()}, a.windows)
            ta, tb = win["in_turn"], win["batched"]
            emit({"mode": "batch", "kind": "three", "n": a.n, "K": K, "ticks_per_call": TICKS,
                  "in_turn_us_per_tick": stats(ta), "batched_us_per_tick": stats(tb),
                  "speedup": round(float(np.median(ta)) / float(np.median(tb)), 2),
                  "batched_median_below_in_turn_min": bool(np.median(tb) < min(ta)),
                  "batch_mid_ticks": [sets["in_turn"][0].batch_mid_ticks(), sets["batched"][0].batch_mid_ticks()],
                  "mid_classes_ticks": [sets["in_turn"][0].mid_classes_ticks(), sets["batched"][0].mid_classes_ticks()]})
            for es in sets.values():
                for e in es:
                    e.close()
    else:
        lib = os.environ.get("CSF_LIB", "this build")
        for model, n in [(c.split(":")[0], int(c.split(":")[1])) for c in a.cells.split(",")]:
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
