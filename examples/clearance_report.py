#!/usr/bin/env python3
"""How close to the kerb a few riders come in the reference's curve scenario, where across the width of the path they ride, and
whether anybody leaves the road: formed on the device from the recording (SocialForceIntersection.clearance; include/csf.h:
csf_clearance).

The road is scenarios/curve-scenario.py's - a straight of 25 m, a right and a left quarter circle of 10 m radius, a straight of
20 m, 5 m wide, a vertex every 0.1 m: 1 530 vertices -, and it is measured as the fp64 polylines the scene was built from, not as
the engine's packed fp32 vertices.  Every tick is recorded on the device (step_n(dense=True)); one call then measures every sample
of every rider against every segment of the road.

Per rider: the closest approach to either kerb with the sample and the edge, the closest approach on the left and on the right, the
samples spent within --near metres of a kerb, and the crossings of an edge.  Then the lateral-position profile: the mean position
across the path - 0 on the right kerb, 1 on the left one - over tenths of the ride.

    python examples/clearance_report.py [--ticks 512] [--near 1.0]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from curve_force_field import curve_road  # noqa: E402
from cyclistsocialforce_amd.intersection import DENSE_CHUNK, SocialForceIntersection  # noqa: E402
from cyclistsocialforce_amd.vehicle import TwoDBicycle  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=DENSE_CHUNK, help=f"ticks to simulate; the last {DENSE_CHUNK} are measured")
    ap.add_argument("--near", type=float, default=1.0, help="a sample closer to a kerb than this counts as near [m]")
    args = ap.parse_args()
    road = curve_road()
    riders = []
    for k, (x, y, v) in enumerate([(0.0, -15.0, 5.0), (1.0, -8.0, 4.0), (-1.0, -2.0, 4.5)]):
        rider = TwoDBicycle((x, y, np.pi / 2, v, 0.0), id=f"rider{k}")
        rider.setDestinations(*road.get_destinations_from_segments())
        riders.append(rider)
    scene = SocialForceIntersection(riders, road_elements=[road])
    dt = riders[0].params.t_s
    scene.step_n(args.ticks, dense=True)
    n_last = min(args.ticks, DENSE_CHUNK)
    r = scene.clearance(args.ticks - n_last, n_last, d_event=args.near, events=True)      # road=None: the scene's own road_elements
    print(f"{len(r.ids)} riders, the last {n_last} ticks of {dt} s against {len(r.offsets) - 1} edges of {int(r.offsets[-1])} vertices, "
          f"{scene.engine.clearance_launches()} launches")
    print("rider    closest [m]  at [s]  edge  on the left [m]  on the right [m]  near samples  crossings")
    for i, name in enumerate(r.ids):
        print(f"{name:8s} {r.d_min[i]:11.3f}  {r.d_min_k[i] * dt:6.2f}  {r.d_min_edge[i]:4d}  {r.left_min[i]:15.3f}  {r.right_min[i]:16.3f}  "
              f"{r.near_samples[i]:12d}  {r.cross_n[i]:9d}")
    for e, name in zip(r.events, r.event_i_id if r.events is not None else []):
        print(f"  {name} crossed edge {e['edge']}, segment {e['seg']} at {e['t'] * dt:.2f} s ({'left to right' if e['dir'] > 0 else 'right to left'} of it)")
    if r.off_road().any():
        print(f"  off the road at the end: {[name for name, off in zip(r.ids, r.off_road()[-1]) if off]}")
    lat, width = r.lateral_position(), r.width()
    print("lateral position over tenths of the ride (0: the right kerb, 1: the left one; -: no kerb on one side), and the width met [m]")
    parts = np.array_split(np.arange(lat.shape[0]), 10)
    with np.errstate(invalid="ignore"):
        for i, name in enumerate(r.ids):
            row = [np.nanmean(lat[p, i]) if np.isfinite(lat[p, i]).any() else np.nan for p in parts]
            w = width[:, i][np.isfinite(width[:, i])]
            print(f"{name:8s} " + " ".join("  -  " if np.isnan(v) else f"{v:5.2f}" for v in row) + (f"   width {w.min():.2f} .. {w.max():.2f}" if w.size else ""))
    share = r.nearest_edge_share()
    print("share of the samples nearest to each edge: " + " ".join(f"{v:.2f}" for v in share))


if __name__ == "__main__":
    main()
