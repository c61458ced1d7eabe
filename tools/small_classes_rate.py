#!/usr/bin/env python3
"""Resident time per tick of small populations of several parameter sets and vehicle classes (GPU box): the general path
(csf_small_classes off: a pair launch and a per-agent launch per class and tick) against the one-wave tick (switch on), the two legs
alternating window by window in one process; beside them the same riders with ONE set of the TwoD class on small_tick_kernel - what a
scene of that size costs on the one-wave tick.  Then K three-rider two-set scenes through csf_step_batch in calls of 100 ticks, switch on
against the same members with the switch off (stepped in turn inside the batch).  Medians over the windows; one JSON line per population.

    python tools/small_classes_rate.py [--ticks 1000] [--windows 5] [--ks 1,16,256,1024] [--out FILE]
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
os.environ.pop("CSF_SMALL_CLASSES", None)
from cyclistsocialforce_amd import _ffi, parameters  # noqa: E402
from cyclistsocialforce_amd.engine import Engine  # noqa: E402

RIDERS = ("twod", "bicycle", "invpend", "planarpoint", "planarbike", "balancingrider")
SEVEN = RIDERS + ("uncontrolled",)


def sets_of(kind):
    """(pods, the set of every road user)"""
    pod = parameters.default_pod
    if kind == "twod3_2sets":
        return [pod("twod"), pod("twod", hfov=2.0, f_0=10.0)], [0, 1, 0]
    if kind == "mixed8_3classes":
        return [pod("twod"), pod("bicycle"), pod("invpend", hfov=2.5)], [k % 3 for k in range(8)]
    if kind == "twod32_32sets":
        return [pod("twod", f_0=6.0 + 0.1 * k, hfov=2.0 + 0.05 * k) for k in range(32)], list(range(32))
    if kind == "mixed32_7classes":
        return [pod(m) for m in SEVEN], [k % 7 for k in range(32)]
    raise KeyError(kind)


def population(pods, cls, seed, on, one_set=False):
    """the riders in a box at the density of the reference's demos, heading for destinations 50 .. 650 m out; one_set: all of them TwoD
    riders of one set (small_tick_kernel's population of that size)"""
    n = len(cls)
    rng = np.random.default_rng(seed)
    box = 14.0 if n <= 8 else 30.0
    if any(p.model == _ffi.BALANCINGRIDER for p in pods):
        box *= 2.0
    x, y = rng.uniform(0, box, n), rng.uniform(0, box, n)
    psi, v = rng.uniform(-np.pi, np.pi, n), rng.uniform(3, 6, n)
    reach = 50.0 * np.arange(1, 14)
    dq = np.zeros((n, 14, 3))
    dq[:, 0, 0], dq[:, 0, 1] = x, y
    dq[:, 1:, 0] = x[:, None] + reach * np.cos(psi)[:, None]
    dq[:, 1:, 1] = y[:, None] + reach * np.sin(psi)[:, None]
    if one_set:
        pods, cls = [parameters.default_pod("twod")], [0] * n
    ns = max(_ffi.N_STATES[p.model] for p in pods)
    s0 = np.zeros((n, ns))
    s0[:, 0], s0[:, 1], s0[:, 2], s0[:, 3] = x, y, psi, v
    e = Engine(pods[0], n)
    e.small_classes(on)
    e.set_param_classes(pods)
    e.add_agents(s0, 5.0)
    e.set_dest_queue(np.arange(n), np.arange(n + 1) * 14, dq.reshape(-1, 3), reset=True)
    e.set_agent_class(np.arange(n), np.asarray(cls))
    cars = [k for k in range(n) if pods[cls[k]].model == _ffi.UNCONTROLLED]
    if cars:                                                        # a prescribed straight line of 3 000 rows each
        t = np.arange(3000) * 0.01
        rows = np.concatenate([np.c_[x[k] + v[k] * t * np.cos(psi[k]), y[k] + v[k] * t * np.sin(psi[k]), np.full(3000, psi[k]), np.full(3000, v[k])]
                               for k in cars])
        e.set_script(np.array(cars), np.arange(len(cars) + 1) * 3000, rows)
    return e


def alternate(legs, ticks, windows):
    """legs: {name: callable that runs `ticks` ticks and waits}; window by window in turn -> {name: (median us per tick, windows)}"""
    for fn in legs.values():
        fn()                                                        # (code objects loaded, clocks up)
    ts = {k: [] for k in legs}
    for _ in range(windows):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    return {k: (float(np.median(v)) * 1e6 / ticks, [round(t * 1e6 / ticks, 3) for t in v]) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--ks", default="1,16,256,1024")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for kind in ("twod3_2sets", "mixed8_3classes", "twod32_32sets", "mixed32_7classes"):
        pods, cls = sets_of(kind)
        off, on, one = population(pods, cls, 11, False), population(pods, cls, 11, True), population(pods, cls, 11, True, one_set=True)
        legs = {"general": lambda: off.step(a.ticks, sync=True), "one_wave": lambda: on.step(a.ticks, sync=True),
                "one_set_twod": lambda: one.step(a.ticks, sync=True)}
        got = alternate(legs, a.ticks, a.windows)
        t_on, t_one = on.small_ticks(), one.small_ticks()
        assert off.small_ticks() == 0 and t_on == (a.windows + 1) * a.ticks and t_one == t_on
        healthy = bool(np.isfinite(on.state()).all() and np.isfinite(off.state()).all())
        emit({"population": kind, "n": len(cls), "sets": len(pods), "classes": len({p.model for p in pods}), "ticks_per_window": a.ticks,
              "general_us_per_tick": round(got["general"][0], 3), "one_wave_us_per_tick": round(got["one_wave"][0], 3),
              "one_set_twod_us_per_tick": round(got["one_set_twod"][0], 3), "speedup": round(got["general"][0] / got["one_wave"][0], 2),
              "over_one_set": round(got["one_wave"][0] / got["one_set_twod"][0], 3), "general_windows": got["general"][1],
              "one_wave_windows": got["one_wave"][1], "one_set_twod_windows": got["one_set_twod"][1], "healthy": healthy})
        for e in (off, on, one):
            e.close()

    pods, cls = sets_of("twod3_2sets")
    ks = [int(k) for k in a.ks.split(",")]
    offs = [population(pods, cls, 100 + i, False) for i in range(max(ks))]
    ons = [population(pods, cls, 100 + i, True) for i in range(max(ks))]
    ones = [population(pods, cls, 100 + i, True, one_set=True) for i in range(max(ks))]
    for K in ks:
        groups = {"switch_off": offs[:K], "switch_on": ons[:K], "one_set_twod": ones[:K]}
        for es in groups.values():
            Engine.batch_join(es)
        l0 = {k: es[0].batch_launches() for k, es in groups.items()}
        legs = {k: (lambda es=es: Engine.step_batch(es, 100, sync=True)) for k, es in groups.items()}
        got = alternate(legs, 100, a.windows if K <= 256 else max(3, a.windows - 2))
        calls = 1 + (a.windows if K <= 256 else max(3, a.windows - 2))
        launches = {k: (es[0].batch_launches() - l0[k]) / calls for k, es in groups.items()}
        batched = {k: es[0].batch_ticks() for k, es in groups.items()}
        for es in groups.values():
            Engine.batch_leave(es)
        emit({"population": "twod3_2sets", "K": K, "mode": "step_batch_100_ticks", "switch_off_us_per_tick": round(got["switch_off"][0], 3),
              "switch_on_us_per_tick": round(got["switch_on"][0], 3), "one_set_twod_us_per_tick": round(got["one_set_twod"][0], 3),
              "speedup": round(got["switch_off"][0] / got["switch_on"][0], 2), "switch_on_us_per_scene_tick": round(got["switch_on"][0] / K, 4),
              "launches_per_call": launches, "member0_batch_ticks": batched, "switch_off_windows": got["switch_off"][1],
              "switch_on_windows": got["switch_on"][1], "one_set_twod_windows": got["one_set_twod"][1]})
    for e in offs + ons + ones:
        e.close()


if __name__ == "__main__":
    main()
