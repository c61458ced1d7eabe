#!/usr/bin/env python3
"""Force-field maps of the curve scenario (scenarios/curve-scenario.py: its road, 63-81, and the panels of its
plot_force_field, 90-125) on the MI355X engine, drawn on the Agg canvas and written to a PNG.

Left: |F| of the road elements as filled contours on the scenario's 150 x 250 grid, their direction as white arrows on the
1 m grid - RoadSegmentCollection.calcRepulsiveForce(X, Y), as the reference calls it.  Middle: |F| along y = 0.  Right: what
the first of three riders on that road would feel elsewhere - SocialForceIntersection.force_field with the other two riders'
fields, the field-of-view mask and the road term, the rider itself excluded.

    python examples/curve_force_field.py [--out curve_force_field.png] [--ticks 100]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cyclistsocialforce_amd.intersection import (CurvedRoadSegment, RoadSegmentCollection, SocialForceIntersection,  # noqa: E402
                                                 StraightRoadSegment)
from cyclistsocialforce_amd.parameters import RoadElementParameters  # noqa: E402
from cyclistsocialforce_amd.vehicle import TwoDBicycle  # noqa: E402


def curve_road():
    params = RoadElementParameters(sigma=2.0, F_0=0.15)
    width, ds = 5, 0.1
    first = StraightRoadSegment(np.array((0, -20, np.pi / 2)), width, 25, params=params, ds=ds)
    right = CurvedRoadSegment(first.x1, width, 10, np.pi / 2, "right", params=params, ds=ds)
    left = CurvedRoadSegment(right.x1, width, 10, np.pi / 2, "left", params=params, ds=ds)
    last = StraightRoadSegment(left.x1, width, 20, params=params, ds=ds)
    return RoadSegmentCollection((first, right, left, last))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="curve_force_field.png")
    ap.add_argument("--ticks", type=int, default=100, help="ticks the three riders ride before the map is taken")
    args = ap.parse_args()
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    road = curve_road()
    riders = []
    for k, (x, y, v) in enumerate([(0.0, -15.0, 5.0), (1.0, -8.0, 4.0), (-1.0, -2.0, 4.5)]):
        rider = TwoDBicycle((x, y, np.pi / 2, v, 0.0), id=f"rider{k}")
        rider.setDestinations(*road.get_destinations_from_segments())
        riders.append(rider)
    scene = SocialForceIntersection(riders, road_elements=[road])
    scene.step_n(args.ticks)

    fig, ax = plt.subplots(1, 3, figsize=(15, 6))
    X, Y = np.meshgrid(np.arange(-5, 10, 0.1), np.arange(0, 25, 0.1))
    Fx, Fy = road.calcRepulsiveForce(X, Y)
    ax[0].set_aspect("equal")
    ax[0].contourf(X, Y, np.minimum(np.hypot(Fx, Fy), 5.0))
    Xq, Yq = np.meshgrid(np.arange(-5, 10, 1.0), np.arange(0, 25, 1.0))
    Fxq, Fyq = road.calcRepulsiveForce(Xq, Yq)
    ax[0].quiver(Xq, Yq, Fxq, Fyq, color="white")
    ax[0].set_xlim(-5, 10)
    ax[0].set_ylim(0, 25)
    ax[0].set_title("road elements: |F| and direction")

    xs = np.arange(-5, 10, 0.1)
    Fxs, Fys = road.calcRepulsiveForce(xs, np.zeros_like(xs))
    ax[1].plot(xs, np.minimum(np.hypot(Fxs, Fys), 10.0))
    ax[1].set_xlabel("x at y = 0")
    ax[1].set_title("|F| across the road")

    me = riders[0]
    Xc, Yc = np.meshgrid(np.arange(-5, 10, 0.1), np.arange(-20, 25, 0.1))
    Gx, Gy = scene.force_field(Xc, Yc, psi=float(me.s[2]), crowd=True, road=True, fov=True, exclude=me)
    ax[2].set_aspect("equal")
    ax[2].contourf(Xc, Yc, np.minimum(np.hypot(Gx, Gy), 5.0))
    for r in riders:
        ax[2].plot(r.s[0], r.s[1], "o", color="red" if r is me else "white")
    ax[2].set_title(f"what {me.id} (red) would feel: riders + road, its field of view")
    fig.savefig(args.out, dpi=100)
    print(f"wrote {args.out}: road |F| up to {np.hypot(Fx, Fy).max():.3g}, {X.size} + {Xq.size} + {xs.size} + {Xc.size} probes, "
          f"{scene._engine.field_map_launches()} launches on the population's engine")


if __name__ == "__main__":
    main()
