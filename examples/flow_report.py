#!/usr/bin/env python3
"""Flow, density and speed of a two-way cycle path at several demand levels: what a traffic engineer reads off a simulation, formed
on the device from the recording (SocialForceIntersection.flow, intersection.flow_together; include/csf.h: csf_flow).

A straight corridor of 12 m along x in open space carries riders both ways, those heading east 0.9 m south of its axis, those
heading west 0.9 m north of it; nothing but the other riders keeps them there, so they spread sideways as demand grows.  An
upstream counting line at x = 5 m and a downstream one at x = 20 m cross the corridor, and the stretch between them is an area.
Every demand level - riders per direction, at even spacing on the 24 m ahead of the stretch - is a scene of its own; all scenes are
ticked together with every tick recorded on the device (advance_together) and measured together in two launches, one transfer and
one wait (flow_together).

Per level: the flow over either line by direction, the mean density of the stretch, Edie's generalised flow, density and space-mean
speed of the stretch - one point of the speed-density diagram a social-force model is validated against -, the speeds at the
upstream line, and the distribution of the travel times from line to line.

    python examples/flow_report.py [--levels 2,4,8] [--ticks 512] [--speed 5.0]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cyclistsocialforce_amd.intersection import DENSE_CHUNK, SocialForceIntersection, advance_together, flow_together  # noqa: E402
from cyclistsocialforce_amd.vehicle import TwoDBicycle  # noqa: E402

X_UP, X_DOWN, HALF_WIDTH, LANE = 5.0, 20.0, 6.0, 0.9
LINES = [(X_UP, -HALF_WIDTH, X_UP, HALF_WIDTH), (X_DOWN, -HALF_WIDTH, X_DOWN, HALF_WIDTH)]      # the left of A -> B is the west
AREAS = [(X_UP, 0.0, X_DOWN, 0.0, HALF_WIDTH)]
APPROACH = 24.0


def path_scene(level, speed, name):
    """`level` riders per direction: eastbound on y = -LANE from just west of the upstream line back, westbound on y = +LANE from just
    east of the downstream line back"""
    riders = []
    for j in range(level):
        back = 1.0 + j * APPROACH / level
        for x, y, psi, tag in ((X_UP - back, -LANE, 0.0, "e"), (X_DOWN + back, LANE, np.pi, "w")):
            v = TwoDBicycle((x, y, psi, speed, 0.0), id=f"{name}{tag}{j}")
            v.params.v_desired_default = speed
            ahead = np.array([60.0, 119.0, 120.0]) * np.cos(psi)
            v.setDestinations(x + ahead, np.full(3, y))
            riders.append(v)
    return SocialForceIntersection(riders)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", default="2,4,8", help="riders per direction of every scene")
    ap.add_argument("--ticks", type=int, default=DENSE_CHUNK, help=f"ticks to simulate; the last {DENSE_CHUNK} are measured")
    ap.add_argument("--speed", type=float, default=5.0, help="desired speed [m/s]")
    args = ap.parse_args()
    levels = [int(v) for v in args.levels.split(",")]
    scenes = [path_scene(level, args.speed, f"L{level}") for level in levels]
    dt = scenes[0].vehicles[0].params.t_s
    advance_together(scenes, args.ticks)
    n_last = min(args.ticks, DENSE_CHUNK)
    results = flow_together(scenes, n_last, LINES, AREAS, events=True)
    launches = scenes[0].engine.flow_launches()
    print(f"{len(scenes)} scenes, the last {n_last} ticks of {dt} s, {launches} launches")
    print("level  up east/west [1/s]  down east/west [1/s]  density [1/m2]  Edie q [1/(m s)]  k [1/m2]  v [m/s]  speed at up: mean / space-mean [m/s]")
    for level, r in zip(levels, results):
        up, down = r.flow(0, dt), r.flow(1, dt)
        q, k, v = r.edie(0, dt)
        mean, harmonic = r.speeds(0, dt)
        print(f"{level:5d}  {up[0]:7.3f} / {up[1]:<7.3f}  {down[0]:9.3f} / {down[1]:<7.3f}  {r.density(0).mean():14.4f}  {q:16.4f}  {k:8.4f}  {v:7.3f}  "
              f"{mean:7.3f} / {harmonic:.3f}")
    print("travel time from line to line [s]: riders, min / median / max")
    for level, r in zip(levels, results):
        for name, a, b in (("east", 0, 1), ("west", 1, 0)):
            heading = np.array([i.rstrip("0123456789").endswith(name[0]) for i in r.ids])
            tt = r.travel_time(a, b, dt)[heading]
            tt = tt[np.isfinite(tt) & (tt > 0)]
            if tt.size:
                print(f"  level {level:3d} {name}: {tt.size:3d}, {tt.min():.2f} / {np.median(tt):.2f} / {tt.max():.2f}")
            else:
                print(f"  level {level:3d} {name}: nobody crossed both lines inside the window")
        n_curve = r.cumulative(0)[:, 0] - r.cumulative(1)[:, 0]    # eastbound riders between the lines, from the two N-curves
        print(f"  level {level:3d}: at most {int(n_curve.max())} eastbound riders between the lines at once; "
              f"{int((r.cross_n[:, 0].sum(axis=1) > 0).sum())} of {len(r.ids)} riders crossed the upstream line, {int((r.in_samples[:, 0] > 0).sum())} were on the stretch")


if __name__ == "__main__":
    main()
