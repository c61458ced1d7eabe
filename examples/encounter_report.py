#!/usr/bin/env python3
"""Who came how close to whom, and when: the reference's stand-alone demo (demo/demoCSFstandalone.py:94-146: three cyclists in an
encroachment conflict in open space, 7 s of simulated time) run with every tick recorded on the device - step_n(..., dense=True) -
and its recording turned into encounter measures on the device (SocialForceIntersection.encounters; include/csf.h: csf_encounters).

For every rider: its closest approach and its smallest time to collision at constant velocity, each with the partner and the time
at which it occurred; then the pairs that came within --d-event metres or --ttc-event seconds of a collision, tick by tick.

    python examples/encounter_report.py [--model 2d] [--t-end 7.0] [--radius 0.5] [--d-event 2.0] [--ttc-event 1.5]
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
    ap.add_argument("--t-end", type=float, default=7.0)
    ap.add_argument("--radius", type=float, default=0.5, help="every rider is a disc of this radius [m]")
    ap.add_argument("--d-event", type=float, default=2.0, help="report pairs closer than this [m]")
    ap.add_argument("--ttc-event", type=float, default=1.5, help="report pairs less than this from a collision [s]")
    args = ap.parse_args()
    riders = three_cyclists(MODELS[args.model])
    scene = SocialForceIntersection(riders)
    t_s = riders[0].params.t_s
    ticks = int(round(args.t_end / t_s))
    # the ring of the dense route holds DENSE_CHUNK samples: the report is made chunk by chunk and reduced here
    best = {v.id: dict(d=(np.inf, None, None), ttc=(np.inf, None, None)) for v in riders}
    events = []
    done = 0
    while done < ticks:
        k = min(ticks - done, DENSE_CHUNK)
        scene.step_n(k, dense=True)
        r = scene.encounters(done, k, radius=args.radius, d_event=args.d_event, ttc_event=args.ttc_event, per_sample=False)
        for i, name in enumerate(r.ids):
            if r.run_d_min[i] < best[name]["d"][0]:
                best[name]["d"] = (float(r.run_d_min[i]), r.run_d_with_id[i], int(r.run_d_sample[i]))
            if r.run_ttc_min[i] < best[name]["ttc"][0]:
                best[name]["ttc"] = (float(r.run_ttc_min[i]), r.run_ttc_with_id[i], int(r.run_ttc_sample[i]))
        events.append(r.events)
        done += k
    time_of = lambda sample: (sample + 1) * t_s                  # noqa: E731  (sample k is the state after tick k + 1)
    print(f"{args.model}: {ticks} ticks of {t_s} s, riders as discs of {args.radius} m, {scene.engine.encounter_launches()} launches")
    for name, b in best.items():
        d, dw, ds = b["d"]
        t, tw, ts = b["ttc"]
        line = f"  {name}: closest approach {d:6.3f} m to {dw} at t = {time_of(ds):5.2f} s;  "
        line += f"smallest time to collision {t:6.3f} s with {tw} at t = {time_of(ts):5.2f} s" if tw is not None else "never on a course that meets anyone"
        print(line)
    ev = np.concatenate(events)
    print(f"  {len(ev)} (tick, pair) events with d < {args.d_event} m or ttc < {args.ttc_event} s")
    ids = [v.id for v in riders]
    for i in range(len(ids)):
        for j in range(i + 1, len(ids)):
            mine = ev[(ev["i"] == i) & (ev["j"] == j)]
            if len(mine):
                print(f"    {ids[i]}-{ids[j]}: {len(mine)} ticks from t = {time_of(mine['sample'].min()):.2f} s to {time_of(mine['sample'].max()):.2f} s, "
                      f"closest {mine['d'].min():.3f} m, smallest ttc {mine['ttc'].min():.3f} s")


if __name__ == "__main__":
    main()
