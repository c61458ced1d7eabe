#!/usr/bin/env python3
"""Who rode behind whom and who passed whom: the reference's stand-alone demo (demo/demoCSFstandalone.py:94-146: three cyclists in open
space, 7 s of simulated time) run with every tick recorded on the device - step_n(..., dense=True) - and its recording turned into
gaps, headways, overtakings and meetings on the device (SocialForceIntersection.passing; include/csf.h: csf_passing).

For every rider: whom it passed or met, when, and at what lateral clearance (positive: the other was on its left); by whom it was
passed; and its smallest gap and time headway to a leader in the corridor ahead of it.

The ring of the dense route holds the last DENSE_CHUNK ticks, and the report covers those.

    python examples/passing_report.py [--model 2d] [--t-end 7.0] [--band 0.75] [--lat-max 3.0]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cyclistsocialforce_amd.intersection import DENSE_CHUNK, SocialForceIntersection  # noqa: E402
from cyclistsocialforce_amd.vehicle import (Bicycle, InvPendulumBicycle, PlanarBicycle, PlanarPointBicycle, TwoDBicycle)  # noqa: E402

MODELS = {"2d": TwoDBicycle, "planartwowheel": Bicycle, "invpendulum": InvPendulumBicycle, "planarpoint": PlanarPointBicycle,
          "planarbike": PlanarBicycle}
KINDS = {1: "overtook", -1: "met", 0: "passed"}


def three_cyclists(cls):
    """demoCSFstandalone.py:96-118"""
    a = cls((-23 + 17, 0, 0, 5, 0, 0, 0, 0), id="a")
    a.params.v_desired_default = 4.5
    b = cls((0 + 15, -20, np.pi / 2, 5, 0, 0, 0, 0), id="b")
    b.params.v_desired_default = 5.0
    c = cls((-2 + 15, -20, np.pi / 2, 5, 0, 0, 0, 0), id="c")
    c.params.v_desired_default = 5.0
    a.setDestinations((35, 64, 65), (0, 0, 0))
    b.setDestinations((15, 15, 15), (20, 49, 50))
    c.setDestinations((13, 13, 13), (20, 49, 50))
    return a, b, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="2d", choices=sorted(MODELS))
    ap.add_argument("--t-end", type=float, default=7.0, help="simulated time [s]")
    ap.add_argument("--band", type=float, default=0.75, help="half the width of the corridor ahead in which a leader is looked for [m]")
    ap.add_argument("--lat-max", type=float, default=3.0, help="the largest lateral clearance at which a passing counts [m]")
    args = ap.parse_args()
    riders = three_cyclists(MODELS[args.model])
    scene = SocialForceIntersection(riders)
    t_s = riders[0].params.t_s
    ticks = int(round(args.t_end / t_s))
    done = 0
    while done < ticks:
        k = min(ticks - done, DENSE_CHUNK)
        scene.step_n(k, dense=True)
        done += k
    first = max(0, ticks - DENSE_CHUNK)                          # the samples the ring still holds
    r = scene.passing(first, ticks - first, args.band, args.lat_max, lat_event=float("inf"), per_station=False).in_seconds()
    at = lambda t: t + (first + 1) * t_s                         # noqa: E731  (sample k is the state after tick k + 1)
    print(f"{args.model}: {ticks} ticks of {t_s} s, from t = {at(0.0):.2f} s on, {scene.engine.passing_launches()} launches, {r.n_events} passings")
    for i, name in enumerate(r.ids):
        made, by = int(r.run_made[i].sum()), int(r.run_by[i].sum())
        print(f"  {name}: made {made} passing{'s' if made != 1 else ''} ({r.run_made[i, 0]} overtaking, {r.run_made[i, 1]} meeting), was passed {by} time{'s' if by != 1 else ''}")
        for e, b in zip(r.events[r.events["i"] == i], r.event_j_id[r.events["i"] == i]):
            print(f"    {KINDS[int(e['kind'])]} {b} at t = {at(e['t']):5.2f} s, {abs(e['lat']):4.2f} m to its {'left' if e['lat'] > 0 else 'right'}, "
                  f"closing at {e['closing']:5.2f} m/s (cosine of the courses {e['cosine']:5.2f})")
        if r.run_by_with[i] >= 0:
            print(f"    closest passing received: by {r.run_by_with_id[i]} at t = {at(r.run_by_t[i]):5.2f} s, {abs(r.run_by_lat[i]):4.2f} m clear")
        if r.run_gap_with[i] < 0:
            print("    followed nobody")
        else:
            print(f"    smallest gap {r.run_gap[i]:5.2f} m behind {r.run_gap_with_id[i]} at t = {at(r.run_gap_k[i] * t_s):5.2f} s; "
                  f"smallest headway {r.run_thw[i]:5.2f} s behind {r.run_thw_with_id[i]} at t = {at(r.run_thw_k[i] * t_s):5.2f} s")


if __name__ == "__main__":
    main()
