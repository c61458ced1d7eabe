#!/usr/bin/env python3
"""What recorded trajectories cost, and what they save (GPU box).  K independent scenes of 3 TwoDBicycle riders, all legs in one
process, their windows alternating, medians over the windows:

  a  csf_step_batch in calls of 100 ticks, nothing recorded
  b  the same with csf_record on every member and one csf_batch_get_record per call (every tick's states and forces on the host)
  c  csf_step_batch_get_tick in calls of 1 tick - the only way to the same data without the recording
  d  advance_together(L, 100) on K SocialForceIntersections of the same riders
  e  step_together(L, 100) on K more

One JSON line per K with the microseconds per tick of every leg, the windows themselves, the two phases of b (the stepping call
with its wait, the read-back) and the ratios c / b, e / d, b / a.

    python tools/record_rate.py [--ks 1,16,256,1024] [--windows 5] [--legs abcde] [--out FILE]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cyclistsocialforce_amd.engine import Engine  # noqa: E402
from batch_rate import scene  # noqa: E402

TICKS = 100


def junction(i):
    from cyclistsocialforce_amd.intersection import SocialForceIntersection
    from cyclistsocialforce_amd.vehicle import TwoDBicycle

    rng = np.random.default_rng(500 + i)
    vs = []
    for k in range(3):
        x, y, psi, v = rng.uniform(0, 14), rng.uniform(0, 14), rng.uniform(-np.pi, np.pi), rng.uniform(3, 6)
        b = TwoDBicycle((x, y, psi, v, 0), id=str(k), saveForces=True)
        b.setDestinations(x + np.array([50.0, 100.0, 150.0]) * np.cos(psi), y + np.array([50.0, 100.0, 150.0]) * np.sin(psi))
        vs.append(b)
    return SocialForceIntersection(vs, id=f"j{i}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,16,256,1024")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--legs", default="abcde")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.windows < 3:
        ap.error("at least 3 windows")
    out = open(a.out, "a") if a.out else None
    from cyclistsocialforce_amd import advance_together, step_together

    for K in [int(k) for k in a.ks.split(",")]:
        plain = [scene("twod", 3, 100 + i) for i in range(K)]
        rec = [scene("twod", 3, 100 + i) for i in range(K)]
        for e in rec:
            e.record(stride=1, capacity=TICKS, forces=True)
        Engine.batch_join(plain)
        Engine.batch_join(rec)
        bufs = [(np.zeros((3, e.ns)), np.zeros(3, dtype=np.int32), np.zeros((3, 3), dtype=np.uint8), np.zeros(3), np.zeros(3)) for e in plain]
        L1 = [junction(i) for i in range(K)] if "d" in a.legs else []
        L2 = [junction(i) for i in range(K)] if "e" in a.legs else []
        phases = {"step": [], "read": []}

        def leg_a():
            Engine.step_batch(plain, TICKS, sync=True)

        def leg_b():
            t0 = time.perf_counter()
            Engine.step_batch(rec, TICKS, sync=True)
            t1 = time.perf_counter()
            Engine.batch_recorded(rec, TICKS)
            phases["step"].append((t1 - t0) * 1e6 / TICKS)
            phases["read"].append((time.perf_counter() - t1) * 1e6 / TICKS)

        def leg_c():
            for _ in range(TICKS):
                Engine.step_batch_into(plain, 1, bufs)

        legs = {"a": leg_a, "b": leg_b, "c": leg_c, "d": lambda: advance_together(L1, TICKS), "e": lambda: step_together(L2, TICKS)}
        legs = {k: f for k, f in legs.items() if k in a.legs}
        for f in legs.values():                                   # warm-up: code objects, buffers, batches joined
            f()
        phases = {"step": [], "read": []}
        win = {k: [] for k in legs}
        for _ in range(a.windows):
            for k, f in legs.items():
                t0 = time.perf_counter()
                f()
                win[k].append((time.perf_counter() - t0) * 1e6 / TICKS)
        med = {k: float(np.median(v)) for k, v in win.items()}
        line = {"K": K, "riders": 3, "ticks_per_call": TICKS,
                "us_per_tick": {k: round(v, 3) for k, v in med.items()}, "windows": {k: [round(x, 3) for x in v] for k, v in win.items()}}
        if "b" in legs:
            line["b_phases_us_per_tick"] = {k: round(float(np.median(v)), 3) for k, v in phases.items()}
            line["rec_member0_batch_ticks"] = rec[0].batch_ticks()
        for name, (num, den) in {"c_over_b": ("c", "b"), "e_over_d": ("e", "d"), "b_over_a": ("b", "a")}.items():
            if num in med and den in med:
                line[name] = round(med[num] / med[den], 2)
        s = json.dumps(line)
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()
        for e in plain + rec:
            e.close()
        del L1, L2


if __name__ == "__main__":
    main()
