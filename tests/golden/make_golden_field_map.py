#!/usr/bin/env python3
"""Generate tests/golden/field_map.npz by RUNNING the reference: force fields at probe points.

Test infrastructure like make_golden.py, whose import scaffolding (stand-in modules, the repaired TwoDBicycle
constructor, the curve-scenario road, the three demo riders) it reuses by importing it.  Inputs and outputs only:

(a) road_*   RoadSegmentCollection.calcRepulsiveForce(X, Y) of the curve-scenario road (scenarios/curve-scenario.py:63-81)
             on np.meshgrid(np.arange(-5, 10, 1.0), np.arange(0, 25, 1.0)) - what plot_force_field (:90-125) maps;
(b) twod_* / bicycle_*   the per-probe sum of calcRepulsiveForce of the three demo riders (vehicle.py:1560-1648 through the
             repaired subclass, :1054-1147 with the riders' speeds) on a 12 x 12 grid of probes with seeded headings, inside a
             40 m box around the riders, where the reference stays finite.

Usage:  python tests/golden/make_golden_field_map.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402


def gen_field_map():
    segs = mg.curve_road()
    X, Y = np.meshgrid(np.arange(-5, 10, 1.0), np.arange(0, 25, 1.0))
    road_Fx, road_Fy = segs.calcRepulsiveForce(X, Y)

    rng = np.random.default_rng(1207)
    px, py = np.meshgrid(np.linspace(-16.0, 24.0, 12), np.linspace(-30.0, 10.0, 12))
    ppsi = rng.uniform(-np.pi, np.pi, px.shape)
    out = {}
    for model in ("twod", "bicycle"):
        riders = mg.demo_bikes(model)
        Fx, Fy = np.zeros(px.size), np.zeros(px.size)
        for v in riders:
            if model == "twod":
                fx, fy = mg.rv.TwoDBicycle.calcRepulsiveForce(v, px.ravel().copy(), py.ravel().copy(), ppsi.ravel().copy())
            else:
                fx, fy = mg.rv.Bicycle.calcRepulsiveForce(v, px.ravel().copy(), py.ravel().copy())
            Fx += np.asarray(fx, dtype=float).ravel()
            Fy += np.asarray(fy, dtype=float).ravel()
        assert np.isfinite(Fx).all() and np.isfinite(Fy).all()
        out[model + "_s"] = np.array([np.asarray(v.s, dtype=float)[:5] for v in riders])
        out[model + "_Fx"] = Fx.reshape(px.shape)
        out[model + "_Fy"] = Fy.reshape(px.shape)
    mg.save("field_map", road_X=X, road_Y=Y, road_Fx=road_Fx, road_Fy=road_Fy, x=px, y=py, psi=ppsi, **out)


if __name__ == "__main__":
    gen_field_map()
