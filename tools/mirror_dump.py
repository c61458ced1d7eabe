#!/usr/bin/env python3
"""Everything a user can observe of SocialForceIntersections and their vehicles behind a fixed script of calls (GPU box), for
comparing two trees of the PYTHON package bit for bit on one library - what tools/small_tick_dump.py does for two builds of the
library.  The package is imported from the root given, so the same tool file runs against another checkout:

    CSF_LIB=.../libcsf_hip.so python tools/mirror_dump.py --root other/checkout --out a.npz
    CSF_LIB=.../libcsf_hip.so python tools/mirror_dump.py --out b.npz --compare a.npz     (exit status 1 on a difference)

The calls (seeded default_rng):

    mix        12 road users of four classes with their own parameter sets, one of them with saveForces; 70 random calls - join, leave by
               index and by id, parameter assignment, route reset, ticks, calc_forces() now and then - as in
               tests/test_gpu_hetero.py::test_random_mirror_calls_keep_rows_and_vehicles_together; then a rep_force_func hook is
               set on one of them and 12 more calls follow on the hooked tick
    together   four intersections of 3, 5, 9 and 16 TwoDBicycles (one vehicle.s handed out, two with saveForces) through
               step_together(..., 7) and advance_together(..., 600): more than one chunk of the dense route
    dense      a fifth one through step_n(40, dense=True) and step_n(40)

The observables: per vehicle, in the order the vehicles were made, s, traj, trajF where kept, F, znav, destpointer, i, force; per
intersection hist_n_vecs and vehicleX / Y / Theta.
"""
import argparse
import os
import sys

import numpy as np


def observe(out, name, ins, made):
    for k, v in enumerate(made):
        tag = f"{name}.v{k:02d}.{v.id}"
        out[tag + ".s"], out[tag + ".traj"], out[tag + ".znav"] = np.array(v.s), np.array(v.traj), np.array(v.znav)
        if v.saveForces:
            out[tag + ".trajF"] = np.array(v.trajF)
        out[tag + ".F"] = np.array(v.F, dtype=float)
        out[tag + ".scalars"] = np.array([v.destpointer, v.i], dtype=np.int64)
        out[tag + ".force"] = np.array(v.force, dtype=float)
    out[name + ".hist_n_vecs"] = np.array(ins.hist_n_vecs, dtype=np.int64)
    out[name + ".vehicleXYTheta"] = np.c_[ins.vehicleX, ins.vehicleY, ins.vehicleTheta]
    out[name + ".ids"] = np.array([int(v.id[1:]) for v in ins.vehicles], dtype=np.int64)


def run(pkg):
    P, V, I = pkg["parameters"], pkg["vehicle"], pkg["intersection"]
    out = {}

    # ---- mix
    rng = np.random.default_rng(1)
    made = []

    def make():
        kind = rng.choice(["twod", "invpend", "planarpoint", "bicycle"])
        k = len(made) + 1
        x, y, psi, v = rng.uniform(0, 35), rng.uniform(0, 35), rng.uniform(-np.pi, np.pi), rng.uniform(3, 4.8)
        own = rng.random() < 0.6
        save = dict(saveForces=k in (2, 15))
        if kind == "twod":
            kw = dict(hfov=float(rng.uniform(1.0, 4.0)), f_0=float(rng.uniform(4, 11))) if own else {}
            b = V.TwoDBicycle((x, y, psi, v, 0), id=f"t{k}", params=P.InvPendulumBicycleParameters(**kw), **save)
        elif kind == "invpend":
            kw = dict(hfov=float(rng.uniform(1.0, 4.0)), sigma_0=float(rng.uniform(0.4, 0.7))) if own else {}
            b = V.InvPendulumBicycle((x, y, psi, v, 0, 0), id=f"i{k}", params=P.InvPendulumBicycleParameters(**kw), **save)
        elif kind == "planarpoint":
            kw = dict(hfov=float(rng.uniform(1.0, 4.0)), f_0=float(rng.uniform(4, 11))) if own else {}
            b = V.PlanarPointBicycle((x, y, psi, v), id=f"p{k}", params=P.PlanarPointBicycleParameters(**kw), **save)
        else:
            kw = dict(hfov=float(rng.uniform(1.0, 4.0)), p_0=float(rng.uniform(20, 40))) if own else {}
            b = V.Bicycle((x, y, psi, v, 0), id=f"b{k}", params=P.BicycleParameters(**kw), **save)
        d = np.array([15.0, 29.0, 30.0])
        b.setDestinations(x + d * np.cos(psi), y + d * np.sin(psi))
        made.append(b)
        return b

    ins = I.SocialForceIntersection([make() for _ in range(12)])

    def calls(count):
        for it in range(count):
            op = str(rng.choice(["step", "step", "join", "join", "join", "join", "leave_index", "leave_id", "assign", "route"]))
            n = len(ins.vehicles)
            if op == "step":
                for _ in range(int(rng.integers(1, 4))):
                    ins.step()
            elif op == "join" and n < 40:
                ins.add_road_user(make())
            elif op == "leave_index" and n > 4:
                ins.remove_road_user(int(rng.integers(0, n)))
            elif op == "leave_id" and n > 5:
                ins.remove_road_users_by_id([ins.vehicles[int(i)].id for i in rng.choice(n, 2, replace=False)])
            elif op == "assign":
                v = ins.vehicles[int(rng.integers(0, n))]
                if type(v).__name__ != "Bicycle":
                    v.params.f_0 = float(rng.uniform(2, 12))
                else:
                    v.params.d_arrived_inter = float(rng.uniform(1.5, 3.0))
            elif op == "route":
                v = ins.vehicles[int(rng.integers(0, n))]
                d = np.array([20.0, 40.0])
                a = rng.uniform(-np.pi, np.pi)
                v.setDestinations(v.s[0] + d * np.cos(a), v.s[1] + d * np.sin(a), reset=True)
            if it % 5 == 4:
                ins.calc_forces()

    calls(70)
    observe(out, "mix.plain", ins, made)

    def half_field(v, x, y, psi):
        fx, fy = v.class_field(x, y, psi)
        return 0.5 * np.asarray(fx), 0.5 * np.asarray(fy)

    next(v for v in ins.vehicles if type(v).__name__ != "Bicycle").rep_force_func = half_field
    calls(12)
    observe(out, "mix.hooked", ins, made)

    # ---- together, dense
    def twods(n, seed, save=()):
        r = np.random.default_rng(seed)
        vs = []
        for k in range(n):
            x, y, psi = r.uniform(0, 14 + n), r.uniform(0, 14 + n), r.uniform(-np.pi, np.pi)
            v = V.TwoDBicycle((x, y, psi, r.uniform(3, 5), 0.0), id=f"t{k}", saveForces=k in save)
            d = np.array([20.0, 40.0, 80.0])
            v.setDestinations(x + d * np.cos(psi), y + d * np.sin(psi))
            vs.append(v)
        return vs

    groups = [twods(n, 50 + n, save) for n, save in ((3, (0,)), (5, ()), (9, (4,)), (16, ()))]
    many = [I.SocialForceIntersection(vs) for vs in groups]
    I.step_together(many, 7)
    groups[1][2].s[1] += 0.25                                      # (handed out and written: the watched shadow on the dense route)
    I.advance_together(many, 600)
    for k, (one, vs) in enumerate(zip(many, groups)):
        observe(out, f"together.{k}", one, vs)

    vs = twods(6, 77, save=(1,))
    fifth = I.SocialForceIntersection(vs)
    fifth.step_n(40, dense=True)
    fifth.step_n(40)
    observe(out, "dense", fifth, vs)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose package runs")
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from cyclistsocialforce_amd import intersection, parameters, vehicle
    assert os.path.abspath(intersection.__file__).startswith(os.path.abspath(a.root)), intersection.__file__
    arrays = run(dict(intersection=intersection, parameters=parameters, vehicle=vehicle))
    print(f"{os.path.abspath(a.root)}: {len(arrays)} arrays, {sum(v.size for v in arrays.values())} numbers")
    if a.out:
        np.savez(a.out, **arrays)
    if a.compare:
        other = np.load(a.compare)
        differ = sorted(set(other.files) ^ set(arrays))
        for name in differ:
            print(f"{name}: in one of the two only")
        for name in sorted(set(arrays) & set(other.files)):
            x, y = arrays[name], other[name]
            if x.shape == y.shape and np.array_equal(x, y):
                continue
            differ.append(name)
            print(f"{name}: largest |difference| {np.abs(x - y).max():.3e} in {int(np.sum(x != y))} of {x.size}" if x.shape == y.shape
                  else f"{name}: shapes {x.shape} / {y.shape}")
        both = len(set(arrays) & set(other.files))
        print(f"compared with {a.compare}: {both - len([n for n in differ if n in arrays and n in other.files])} of {both} arrays in both identical"
              + ("" if differ else ": ALL IDENTICAL"))
        if differ:
            sys.exit(1)


if __name__ == "__main__":
    main()
