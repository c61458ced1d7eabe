#!/usr/bin/env python3
"""Time of a force-field map (GPU box; run it under a time limit, e.g. `timeout 300 python tools/field_map_rate.py`).

Median wall time per Engine.field_map call (copies in and out included) and median time per launch (the kernels' own HIP
events, through csf_profile_enable: the crowd launch is kernel 0, the road launch kernel 1) for

    37 500 probes    x 3 riders + 1 530 road vertices     the curve scenario's own grid (scenarios/curve-scenario.py:90-125)
    1 024 x 1 024    x 1 024 riders, no road
    1 024 x 1 024    x 16 384 riders, no road

and, for the first shape, the only route the parent commit offers: one Engine.pair_force call per source, summed on the host
(it has no road route at all).  Pairs per second are set against the 157 TFLOP/s vector peak at ~100 op-equivalents per pair.
One JSON line per shape.

    python tools/field_map_rate.py [--calls 7] [--shapes curve,1k,16k] [--fov] [--out FILE]
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
from cyclistsocialforce_amd import parameters  # noqa: E402
from cyclistsocialforce_amd.engine import Engine  # noqa: E402

PEAK_PAIRS = 157e12 / 100.0          # pairs / s at the vector peak


def curve_shape():
    """the curve scenario: its road (63-81), three riders on it, the 150 x 250 grid of plot_force_field"""
    from cyclistsocialforce_amd import intersection as ci
    rp = parameters.RoadElementParameters(sigma=2.0, F_0=0.15)
    seg1 = ci.StraightRoadSegment(np.array((0, -20, np.pi / 2)), 5, 25, params=rp, ds=0.1)
    seg2 = ci.CurvedRoadSegment(seg1.x1, 5, 10, np.pi / 2, "right", params=rp, ds=0.1)
    seg3 = ci.CurvedRoadSegment(seg2.x1, 5, 10, np.pi / 2, "left", params=rp, ds=0.1)
    seg4 = ci.StraightRoadSegment(seg3.x1, 5, 20, params=rp, ds=0.1)
    road = ci.RoadSegmentCollection((seg1, seg2, seg3, seg4))
    s0 = np.array([[0.0, -15.0, np.pi / 2, 5.0, 0.0], [1.0, -5.0, np.pi / 2, 4.0, 0.0], [-1.0, 3.0, np.pi / 2, 4.5, 0.0]])
    e = Engine(parameters.default_pod("twod"), 4)
    e.add_agents(s0, 5.0)
    e.set_road(*ci.flatten_road_elements([road]))
    X, Y = np.meshgrid(np.arange(-5, 10, 0.1), np.arange(0, 25, 0.1))
    return e, s0, X, Y, sum(len(ed.vertices) for ed in road.edges())


def crowd_shape(n):
    rng = np.random.default_rng(n)
    box = 3.0 * np.sqrt(n)
    s0 = np.zeros((n, 5))
    s0[:, 0], s0[:, 1] = rng.uniform(0, box, n), rng.uniform(0, box, n)
    s0[:, 2], s0[:, 3] = rng.uniform(-np.pi, np.pi, n), rng.uniform(3, 6, n)
    e = Engine(parameters.default_pod("twod"), n)
    e.add_agents(s0, 5.0)
    X, Y = np.meshgrid(np.linspace(0, box, 1024), np.linspace(0, box, 1024))
    return e, s0, X, Y, 0


def measure(e, X, Y, psi, calls, road, fov):
    e.field_map(X, Y, psi, crowd=True, road=road, fov=fov)     # warm-up: buffers grown, code loaded
    e.profile(1)
    e.profile_kernels()
    wall = []
    for _ in range(calls):
        t0 = time.perf_counter()
        e.field_map(X, Y, psi, crowd=True, road=road, fov=fov)
        wall.append(time.perf_counter() - t0)
    crowd_us, road_us = e.profile_samples(kernel="pair"), e.profile_samples(kernel="road")
    e.profile(0)
    return float(np.median(wall)) * 1e3, float(np.median(crowd_us)), float(np.median(road_us)) if road_us.size else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--shapes", default="curve,1k,16k")
    ap.add_argument("--fov", action="store_true", help="with the field-of-view mask (the probe is a receiver)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    for shape in a.shapes.split(","):
        e, s0, X, Y, nv = curve_shape() if shape == "curve" else crowd_shape({"1k": 1024, "16k": 16384}[shape])
        psi = np.full(X.shape, 0.5 * np.pi)
        wall_ms, crowd_us, road_us = measure(e, X, Y, psi, a.calls, nv > 0, a.fov)
        pairs = X.size * s0.shape[0]
        rec = {"shape": shape, "probes": int(X.size), "sources": int(s0.shape[0]), "road_vertices": int(nv), "fov": bool(a.fov),
               "call_ms_median": round(wall_ms, 3), "crowd_launch_us_median": round(crowd_us, 2),
               "road_launch_us_median": None if road_us is None else round(road_us, 2),
               "crowd_pairs_per_s": round(pairs / (crowd_us * 1e-6), 0), "crowd_fraction_of_vector_peak": round(pairs / (crowd_us * 1e-6) / PEAK_PAIRS, 4)}
        if road_us is not None:
            rec["road_pairs_per_s"] = round(X.size * nv / (road_us * 1e-6), 0)
        if shape == "curve":                                     # the parent's route: csf_pair_force per source, summed on the host
            x, y, p = X.ravel(), Y.ravel(), psi.ravel()
            ts = []
            for _ in range(a.calls):
                t0 = time.perf_counter()
                fx, fy = np.zeros(x.size), np.zeros(x.size)
                for s in s0:
                    gx, gy = e.pair_force(s[:4], x, y, p, apply_fov=a.fov)
                    fx += gx
                    fy += gy
                ts.append(time.perf_counter() - t0)
            rec["pair_force_route_ms_median"] = round(float(np.median(ts)) * 1e3, 3)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
        e.close()


if __name__ == "__main__":
    main()
