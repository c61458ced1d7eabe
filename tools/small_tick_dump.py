#!/usr/bin/env python3
"""State and total forces of a fixed set of tiny populations after 60 ticks of the stepping engine's one-wave and batched tick (GPU box),
for comparing two builds of the library BIT FOR BIT - what tools/scene_eval_dump.py does for the calibration kernels, for
small_tick_kernel, small_batch_kernel, small_classes_kernel and small_classes_batch_kernel.  Everything goes through the Python Engine
API, so the tool runs unchanged from the tools/ folder of any checkout that has csf_small_classes, or on another build
of the library through CSF_LIB:

    python tools/small_tick_dump.py --out a.npz                    (the one build)
    python tools/small_tick_dump.py --out b.npz --compare a.npz    (the other: runs, writes, compares; exit status 1 on a difference)

The populations are the smallest that reach every line the two tick bodies have in common (csf_small_body.inc, csf_wide_body.inc), each one engine and 60 ticks:

    <model>.n<3|5|32>.r<0|1>   each of the six rider classes at n = 3 (P = 4: sixteen source groups), 5 and 32 (P = 32: two groups),
                               priority to the right off and on                                    small_tick_kernel
    <model>.exact              three riders: rider 0 at (10, 10) with psi = 0, riders 1 and 2 both at (15, 10) - the very same spot,
                               receiver - source = (0, 0) -, exactly on rider 0's heading line and facing it: np.sign(phi) undecided
                               in fp32, exactly 0 in fp64, the term projected on the line
    <model>.road<100|1100>     five riders beside a road edge of 100 vertices, and of 1 100: the road loop tiles by 1 024
    classes.b / classes.e      csf_small_classes on: twod, bicycle, bicycle, invpend, twod - a Bicycle source and a TwoD source in one
                               loop -, and four cyclists with a scripted UncontrolledVehicle           small_classes_kernel
    batch.<k> / cbatch.<k>     three members of 3, 5 and 32 riders through csf_step_batch (one class), and three members of several
                               classes                                             small_batch_kernel, small_classes_batch_kernel
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
os.environ.pop("CSF_PAIR_VARIANT", None)
from cyclistsocialforce_amd import _ffi, parameters  # noqa: E402
from cyclistsocialforce_amd.engine import Engine  # noqa: E402
from cyclistsocialforce_amd.engine import MODEL_IDS  # noqa: E402
from scene_calib_common import MODELS, VDES, crowd  # noqa: E402
from small_classes_common import build, case, single_population  # noqa: E402

T = 60


def population(model, n, seed, rule=0):
    """an engine that holds crowd(n) of one class, in the box the tests give a crowd of that size"""
    box = (14.0 if n <= 8 else (22.0 if n <= 16 else 30.0)) * (2.0 if model == "balancingrider" else 1.0)
    x, y, psi, v, off, dq = crowd(n, seed=seed, box=box)
    s0 = np.zeros((n, _ffi.N_STATES[MODEL_IDS[model]]))
    s0[:, 0], s0[:, 1], s0[:, 2], s0[:, 3] = x, y, psi, v
    return loaded(model, s0, off, dq, rule)


def loaded(model, s0, off, dq, rule=0):
    n = s0.shape[0]
    e = Engine(parameters.default_pod(model, priority_rule=rule), n)
    e.add_agents(s0, VDES)
    e.set_dest_queue(np.arange(n), off, dq, reset=True)
    return e


def result(e):
    """(state, total forces) behind the ticks; the engine must have taken the one-wave or the batched tick for all of them"""
    assert e.small_ticks() == T, e.small_ticks()
    s, (fx, fy) = e.state(), e.forces()
    e.close()
    assert np.isfinite(s).all()
    return s, np.c_[fx, fy]


def cases():
    """(name, function that runs the population and returns its result); a batch returns one result per member"""
    def plain(model, n, rule):
        e = population(model, n, seed=300 + 10 * n + rule, rule=rule)
        e.step(T)
        return result(e)

    def exact(model):
        # (That tick 0 takes the coincident branch and the sg == 0 projection rests on the geometry and on the conditions in the source -
        # ex == ey == 0 exactly; dy * cos - dx * sin == 0 with cos = 1, sin = 0 - and not on a counter: the kernels have none.  What was
        # seen: a build whose TwoD field contracted dx * cos + dy * sin the other way round changed every number of twod.exact.)
        _, _, _, v, off, dq = crowd(3, seed=7)
        s0 = np.zeros((3, _ffi.N_STATES[MODEL_IDS[model]]))
        s0[:, 0], s0[:, 1], s0[:, 2], s0[:, 3] = (10.0, 15.0, 15.0), (10.0, 10.0, 10.0), (0.0, -3.0, -3.1), v
        e = loaded(model, s0, off, dq)
        e.step(T)
        return result(e)

    def road(model, count):
        e = population(model, 5, seed=77)                         # (sigma: the power of rsq, and the exp2 / log2 form)
        e.set_road(np.array([0, count], dtype=np.int64), np.c_[np.linspace(-20.0, 50.0, count), np.full(count, -3.0)], np.array([0.15]),
                   np.array([2.0 if count == 100 else 2.5]))
        e.step(T)
        return result(e)

    def classes(name):
        e = build(case(name), True)
        e.step(T)
        return result(e)

    def batch(make):
        members = make()
        Engine.batch_join(members)
        Engine.step_batch(members, T, sync=True)
        assert all(e.batch_ticks() == T for e in members), [e.batch_ticks() for e in members]
        Engine.batch_leave(members)
        return [result(e) for e in members]

    out = []
    for model in MODELS:
        out += [(f"{model}.n{n}.r{rule}", lambda m=model, n=n, r=rule: plain(m, n, r)) for n in (3, 5, 32) for rule in (0, 1)]
        out.append((f"{model}.exact", lambda m=model: exact(m)))
        out += [(f"{model}.road{c}", lambda m=model, c=c: road(m, c)) for c in (100, 1100)]
    out += [(f"classes.{name}", lambda name=name: classes(name)) for name in "be"]
    out.append(("batch", lambda: batch(lambda: [population("twod", n, seed=400 + n) for n in (3, 5, 32)])))
    out.append(("cbatch", lambda: batch(lambda: [build(case("b"), True), build(case("e"), True), build(single_population(3), True)])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", default=None)
    ap.add_argument("--only", default=None, help="run the cases whose name starts with this (a first run of a new build: its smallest case alone)")
    a = ap.parse_args()
    out = {}
    for name, run in cases():
        if a.only is not None and not name.startswith(a.only):
            continue
        got = run()
        if isinstance(got, list):
            out.update({f"{name}.{k}": g for k, g in enumerate(got)})
        else:
            out[name] = got
    arrays = {}
    for name, (s, F) in out.items():
        arrays[name + ".state"], arrays[name + ".forces"] = s, F
    print(f"{len(arrays)} arrays, {sum(v.size for v in arrays.values())} numbers")
    if a.out:
        np.savez(a.out, **arrays)
    if a.compare:
        other = np.load(a.compare)
        differ = sorted(set(other.files) - set(arrays)) if a.only is None else []
        for name in differ:
            print(f"{name}: in {a.compare} only")
        for name in sorted(set(arrays) & set(other.files)):
            x, y = arrays[name], other[name]
            if x.shape == y.shape and np.array_equal(x, y):
                continue
            differ.append(name)
            print(f"{name}: largest |difference| {np.abs(x - y).max():.3e} in {int(np.sum(x != y))} of {x.size}" if x.shape == y.shape
                  else f"{name}: shapes {x.shape} / {y.shape}")
        both = len(set(arrays) & set(other.files))
        print(f"compared with {a.compare}: {both - len([n for n in differ if n in arrays])} of {both} arrays in both identical" + ("" if differ else ": ALL IDENTICAL"))
        if differ:
            sys.exit(1)


if __name__ == "__main__":
    main()
