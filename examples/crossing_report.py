#!/usr/bin/env python3
"""Who crossed whose path, where, who was first and how long after: the reference's stand-alone demo (demo/demoCSFstandalone.py:94-146:
three cyclists in an encroachment conflict in open space, 7 s of simulated time) run with every tick recorded on the device -
step_n(..., dense=True) - and its recording turned into post-encroachment times on the device
(SocialForceIntersection.post_encroachment; include/csf.h: csf_post_encroachment).

For every rider: the crossing of its path with the smallest post-encroachment time - whose path, where, who was there first and the
PET in seconds - and the number of crossings on its path; then every crossing of every pair.

A crossing couples every sample of one path with every sample of another, so a path is ONE window of the ring: the ring of the dense
route holds the last DENSE_CHUNK ticks, and the report covers those (the riders start 20 m apart: the first seconds hold no crossing).

    python examples/crossing_report.py [--model 2d] [--t-end 7.0]
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
    r = scene.post_encroachment(first, ticks - first, pet_event=float("inf"), per_segment=False).in_seconds()
    at = lambda t: t + (first + 1) * t_s                         # noqa: E731  (sample k is the state after tick k + 1)
    print(f"{args.model}: {ticks} ticks of {t_s} s, paths from t = {at(0.0):.2f} s on, {scene.engine.pet_launches()} launches, {r.n_events} crossings")
    for i, name in enumerate(r.ids):
        if r.run_with[i] < 0:
            print(f"  {name}: crossed nobody's path")
            continue
        leader = name if r.run_t_own[i] < r.run_t_with[i] else r.run_with_id[i]
        print(f"  {name}: crossed the path of {r.run_with_id[i]} at ({r.run_x[i]:6.2f}, {r.run_y[i]:6.2f}); {leader} was there first; "
              f"{name} at t = {at(r.run_t_own[i]):5.2f} s, {r.run_with_id[i]} at t = {at(r.run_t_with[i]):5.2f} s: PET {r.run_pet[i]:5.2f} s "
              f"({r.run_count[i]} crossing{'s' if r.run_count[i] != 1 else ''} on its path)")
    for e, a, b in zip(r.events, r.event_i_id, r.event_j_id):
        print(f"    {a}-{b}: at ({e['x']:6.2f}, {e['y']:6.2f}), {a} at t = {at(e['t_i']):5.2f} s, {b} at t = {at(e['t_j']):5.2f} s, "
              f"PET {abs(e['t_j'] - e['t_i']):5.2f} s")


if __name__ == "__main__":
    main()
