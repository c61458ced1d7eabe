#!/usr/bin/env python3
"""Sums and sampled states of a fixed set of tiny closed-loop calibration data sets (GPU box), for comparing two builds of the library
BIT FOR BIT: the GPU tests hold the scene kernels to their twins at 2e-7, which does not see a changed rounding.  Everything goes
through the Python Engine API, so the tool runs unchanged from the tools/ folder of any checkout that has the scene calibration of
DESIGN.md 4.10 - 4.10j; run it in both, then compare:

    python tools/scene_eval_dump.py --out a.npz                    (in the one checkout)
    python tools/scene_eval_dump.py --out b.npz --compare a.npz    (in the other: evaluates, writes, compares; exit status 1 on a difference)

The data sets are the smallest that reach every piece the kernels of csf_scene.hip share - all six vehicle classes, 3 candidate sets,
60 ticks, sampled at stride 10, built with the builders of tests/scene_*_common.py:

    a    two scenes of 3 and 5 riders, the second 45 ticks long                    scene_eval_kernel<., false>
    b    a with rider 4 on its recording                                           ... the replay write-back
    c    a with presence windows, rider 2 never present; cr: and the replay        scene_eval_kernel<., true>
    d    a with a road of 100 / 101 vertices per scene, road_F0 / road_sigma per set       ... the road block of the set
    ea, ec, ed   a, c, d with the riders in two groups                             scene_groups_kernel<., false / true>
    f    a roster of 6 on 3 shared lanes, one handover at the tick the lane is left; fr: rider 3 (second on its lane) replayed and
         a road with per-set parameters                                            scene_lanes_kernel
    g    a roster of 48 on 40 wide lanes with handovers and a narrow scene of 5 in one data set, a road of 100 vertices on each with
         per-set parameters: two launches                                          scene_wide_kernel + scene_lanes_kernel
    fg, gg   fr and g with the riders in two groups (csf_scene_calib_lane_groups; left out where the library lacks the call)
                                                                                   scene_lanes_groups_kernel, scene_wide_groups_kernel
    fm, gm   fr and g with the riders alternating between two groups of two vehicle classes - the model's and the next one's
         (csf_scene_calib_lane_classes; left out where the library lacks the call: a lane changes its class at a handover)
                                                                                   scene_lanes_mixed_kernel, scene_wide_mixed_kernel
    m    a with the riders alternating between two groups of two vehicle classes - the model's and the next one's
         (csf_scene_calib_classes; left out where the library lacks the call)      scene_mixed_kernel
    mc, md   m with the windows of c and rider 4 replayed; m with the roads and the per-set road parameters of d.  (One engine, in the
         order md, m, mc: md runs with the road of d still held, mc adds to m.  Reordering the cases changes what is dumped.)
    k    csf_calib_load / csf_calib_eval of 3 sequences (the second 45 ticks long), with and without fix_speed: k1, k0
                                                                                   replay_eval_kernel
    x    a wide scene of 40 riders at once whose start reaches the two rare branches of the exact pair term (the pair loops of csf_small_body.inc / csf_wide_body.inc): riders 0
         and 1 on the very same spot (receiver - source = (0, 0): no term), and rider 3 exactly on the heading line of rider 2 - source
         at (10, 10) with psi = 0, receiver at (15, 10) looking back at it -, so the sign of phi is undecided in fp32, exactly 0 in fp64, and the term is
         projected on the line.  (The last case of every model: the dumps of the cases above stay what they were.)
                                                                                   scene_wide_kernel
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
os.environ.pop("CSF_PAIR_VARIANT", None)
from cyclistsocialforce_amd.engine import Engine  # noqa: E402
from cyclistsocialforce_amd.engine import MODEL_IDS  # noqa: E402
from calib_common import data_set, pod_sets  # noqa: E402
from scene_calib_common import MODELS, VDES, scenes  # noqa: E402
from scene_groups_common import group_sets  # noqa: E402
from scene_lanes_common import greedy_lanes, loaded_shared, roster  # noqa: E402
from scene_mixed_common import mixed_sets  # noqa: E402
from scene_wide_common import always, edge_below, loaded_wide, wide_crowd  # noqa: E402
from scene_windows_common import FEAT, one_scene, sets3  # noqa: E402

T, STRIDE = 60, 10
N_RIDERS = np.array([3, 5], dtype=np.int32)
LENGTHS = np.array([T, 45], dtype=np.int32)
R = int(N_RIDERS.sum())
ENTER = np.array([0, 7, 30, 0, 12, 0, 20, 44], dtype=np.int32)   # rider 2: never present; scene 1 ends at tick 45
EXIT = np.array([T, 41, 30, 45, 45, 33, 21, 45], dtype=np.int32)
ROAD_F0, ROAD_SIGMA = (4.0, 7.5, 0.0), (2.0, 2.5, 3.0)           # per candidate set: an integer sigma, a fractional one, F_0 = 0
REPLAYED = 4


def road_call(edges):
    """Engine.scene_calib_road's arguments for one edge (as Engine.set_road takes it) per scene"""
    off = np.r_[0, np.cumsum([e[1].shape[0] for e in edges])].astype(np.int64)
    return (np.arange(len(edges), dtype=np.int32), off, np.concatenate([e[1] for e in edges]), np.concatenate([e[2] for e in edges]),
            np.concatenate([e[3] for e in edges]))


def recording(e, sets, riders, n):
    """(x, y, psi, v) of `riders` after every tick of the loaded data set's own run with candidate 1 (0 where a rider is absent)"""
    _, st = e.scene_calib_eval(sets, states=True)
    return np.ascontiguousarray(np.nan_to_num(st[:, n + np.asarray(riders), :4]))


def next_class(model):
    """the two classes of the mixed cases: the model's and the next one's"""
    return model, MODELS[(MODELS.index(model) + 1) % len(MODELS)]


def small_cases(model, out):
    sets, gsets = sets3(model), group_sets(model, 3, 2)
    s0, off, rows, _ = scenes(model, N_RIDERS, seed=5)
    obj = np.random.default_rng(11).normal(size=(T, R, len(FEAT)))
    roads = road_call([edge_below(model, 3, count=100), edge_below(model, 5, count=101)])
    group = (np.arange(R) % 2).astype(np.uint8)
    mask = np.arange(R) == REPLAYED
    over = dict(road_F0=ROAD_F0, road_sigma=ROAD_SIGMA)
    e = Engine(sets[0], 3 * R)
    e.scene_calib_load(N_RIDERS, s0, VDES, off, rows, obj, FEAT, lengths=LENGTHS, max_sets=3)
    rec = recording(e, sets, [REPLAYED], R)
    out["a"] = e.scene_calib_eval(sets, states=True, stride=STRIDE)
    e.scene_calib_replay(mask, rec)
    out["b"] = e.scene_calib_eval(sets, states=True, stride=STRIDE)
    e.scene_calib_windows(ENTER, EXIT)
    out["cr"] = e.scene_calib_eval(sets, states=True, stride=STRIDE)
    e.scene_calib_replay(None)
    out["c"] = e.scene_calib_eval(sets, states=True, stride=STRIDE)
    e.scene_calib_groups(group, 2)
    out["ec"] = e.scene_calib_eval_groups(gsets, states=True, stride=STRIDE)
    e.scene_calib_windows(None, None)
    out["ea"] = e.scene_calib_eval_groups(gsets, states=True, stride=STRIDE)
    e.scene_calib_road(*roads)
    out["ed"] = e.scene_calib_eval_groups(gsets, states=True, stride=STRIDE, **over)
    e.scene_calib_groups(None)
    out["d"] = e.scene_calib_eval(sets, states=True, stride=STRIDE, **over)
    if hasattr(e._lib, "csf_scene_calib_classes"):               # (the road of d stays for md, then goes)
        classes = next_class(model)
        msets = mixed_sets(3, classes)
        e.scene_calib_classes(group, [MODEL_IDS[c] for c in classes], s0)
        out["md"] = e.scene_calib_eval_groups(msets, states=True, stride=STRIDE, **over)
        e.scene_calib_road(None, None, None, None, None)
        out["m"] = e.scene_calib_eval_groups(msets, states=True, stride=STRIDE)
        e.scene_calib_windows(ENTER, EXIT)
        e.scene_calib_replay(mask, rec)
        out["mc"] = e.scene_calib_eval_groups(msets, states=True, stride=STRIDE)
    e.close()


def replay_cases(model, out):
    sets = pod_sets(model, 3)
    s0, Fx, Fy = data_set(model, seed=7, n_seq=3, ticks=T)
    obj = np.random.default_rng(14).normal(size=(T, 3, len(FEAT)))
    e = Engine(sets[0], 3 * 3)
    e.calib_load(s0, Fx, Fy, obj, FEAT, lengths=np.array([T, 45, T], dtype=np.int32), max_sets=3)
    out["k1"] = e.calib_eval(sets, fix_speed=True, states=True, stride=STRIDE)
    out["k0"] = e.calib_eval(sets, fix_speed=False, states=True, stride=STRIDE)
    e.close()


def shared_cases(model, out):
    sets = sets3(model)
    part = roster(model, 6, seed=63)
    enter = np.array([0, 0, 0, 30, 25, 50], dtype=np.int32)       # rider 3 takes lane 0 over at the tick rider 0 leaves it
    exit_ = np.array([30, 25, T, T, 50, T], dtype=np.int32)
    lanes = greedy_lanes(enter, exit_)
    assert lanes[1] == 3 and lanes[0][3] == lanes[0][0]
    obj = np.random.default_rng(12).normal(size=(T, 6, len(FEAT)))
    e = loaded_shared(sets, [part], [lanes], enter, exit_, obj)
    rec = recording(e, sets, [3], 6)
    out["f"] = e.scene_calib_eval(sets, states=True, stride=STRIDE)
    e.scene_calib_replay(np.arange(6) == 3, rec)
    e.scene_calib_road(*road_call([edge_below(model, 6, count=100)]))
    out["fr"] = e.scene_calib_eval(sets, states=True, stride=STRIDE, road_F0=ROAD_F0, road_sigma=ROAD_SIGMA)
    if hasattr(e._lib, "csf_scene_calib_lane_groups"):           # (riders 0 and 3 share lane 0: its group changes at the handover)
        e.scene_calib_lane_groups((np.arange(6) % 2).astype(np.uint8), 2)
        out["fg"] = e.scene_calib_eval_groups(group_sets(model, 3, 2), states=True, stride=STRIDE, road_F0=ROAD_F0, road_sigma=ROAD_SIGMA)
    if hasattr(e._lib, "csf_scene_calib_lane_classes"):          # (riders 0 and 3 share lane 0: its class changes at the handover)
        classes = next_class(model)
        e.scene_calib_lane_classes((np.arange(6) % 2).astype(np.uint8), [MODEL_IDS[c] for c in classes], part[0])
        out["fm"] = e.scene_calib_eval_groups(mixed_sets(3, classes), states=True, stride=STRIDE, road_F0=ROAD_F0, road_sigma=ROAD_SIGMA)
    e.close()


def wide_cases(model, out):
    sets = sets3(model)
    parts = [wide_crowd(model, 48), one_scene(model, 5, seed=41)]
    enter, exit_ = np.zeros(53, dtype=np.int32), np.full(53, T, dtype=np.int32)
    exit_[:8] = 20 + 3 * np.arange(8)                             # riders 40 - 47 take the lanes of riders 0 - 7 over at those ticks
    enter[40:48] = exit_[:8]
    lanes = [greedy_lanes(enter[:48], exit_[:48]), (np.arange(5, dtype=np.int32), 5)]
    assert lanes[0][1] == 40
    obj = np.random.default_rng(13).normal(size=(T, 53, len(FEAT)))
    e = loaded_wide(sets, parts, lanes, enter, exit_, obj)
    e.scene_calib_road(*road_call([edge_below(model, 48, count=100), edge_below(model, 5, count=100)]))
    before = e.scene_calib_launches()
    out["g"] = e.scene_calib_eval(sets, states=True, stride=STRIDE, road_F0=ROAD_F0, road_sigma=ROAD_SIGMA)
    assert e.scene_calib_launches() == before + 2                 # (the narrow scene and the wide one: both kernels)
    if hasattr(e._lib, "csf_scene_calib_lane_groups"):           # (riders r and 40 + r share a lane; at two of three handovers its group changes)
        e.scene_calib_lane_groups((np.arange(53) % 3 % 2).astype(np.uint8), 2)
        out["gg"] = e.scene_calib_eval_groups(group_sets(model, 3, 2), states=True, stride=STRIDE, road_F0=ROAD_F0, road_sigma=ROAD_SIGMA)
        assert e.scene_calib_launches() == before + 4
    if hasattr(e._lib, "csf_scene_calib_lane_classes"):
        classes = next_class(model)
        at = e.scene_calib_launches()
        e.scene_calib_lane_classes((np.arange(53) % 3 % 2).astype(np.uint8), [MODEL_IDS[c] for c in classes], np.concatenate([p[0][:, :4] for p in parts]))
        out["gm"] = e.scene_calib_eval_groups(mixed_sets(3, classes), states=True, stride=STRIDE, road_F0=ROAD_F0, road_sigma=ROAD_SIGMA)
        assert e.scene_calib_launches() == at + 2
    e.close()


def exact_cases(model, out):
    # (that the start takes the two branches rests on the geometry and on the conditions in the source, not on a counter: see
    # tools/small_tick_dump.py, exact())
    sets = sets3(model)
    s0, off, dq = wide_crowd(model, 40)
    s0 = s0.copy()
    s0[1, :2] = s0[0, :2]                                         # the very same spot
    s0[2, :3] = 10.0, 10.0, 0.0                                   # cos = 1, sin = 0 exactly
    s0[3, :3] = 15.0, 10.0, -3.0                                  # 5 m straight ahead of rider 2 (phi = 0), facing it: rider 2 is in its view,
                                                                  # and to its right, so under the priority rule as well
    lanes, enter, exit_ = always(40, T)
    obj = np.random.default_rng(15).normal(size=(T, 40, len(FEAT)))
    e = loaded_wide(sets, [(s0, off, dq)], [lanes], enter, exit_, obj)
    out["x"] = e.scene_calib_eval(sets, states=True, stride=STRIDE)
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", default=None)
    ap.add_argument("--models", default=",".join(MODELS))
    a = ap.parse_args()
    arrays = {}
    for model in a.models.split(","):
        out = {}
        small_cases(model, out)
        shared_cases(model, out)
        wide_cases(model, out)
        replay_cases(model, out)
        exact_cases(model, out)
        for case, (sums, states) in out.items():
            assert np.isfinite(sums).all() and np.any(sums != 0.0) and np.isfinite(states).any(), (model, case)
            arrays[f"{model}.{case}.sums"], arrays[f"{model}.{case}.states"] = sums, states
    print(f"{len(arrays)} arrays, {sum(v.size for v in arrays.values())} numbers")
    if a.out:
        np.savez(a.out, **arrays)
    if a.compare:
        other = np.load(a.compare)
        differ = sorted(set(other.files) - set(arrays))
        for name in differ:
            print(f"{name}: in {a.compare} only")
        extra = sorted(set(arrays) - set(other.files))           # (cases the other build's library lacks the call for: nothing to compare)
        if extra:
            print(f"{len(extra)} arrays in this build only: {' '.join(sorted({n.split('.')[1] for n in extra}))}")
        for name in sorted(set(arrays) & set(other.files)):
            x, y = arrays[name], other[name]
            if x.shape == y.shape and np.array_equal(x, y, equal_nan=True):
                continue
            differ.append(name)
            if x.shape != y.shape or not np.array_equal(np.isnan(x), np.isnan(y)):
                print(f"{name}: shapes {x.shape} / {y.shape}, or another NaN pattern")
            else:
                print(f"{name}: largest |difference| {np.nanmax(np.abs(x - y)):.3e} in {int(np.sum(~((x == y) | np.isnan(x))))} of {x.size}")
        n_both = len(set(arrays) & set(other.files))
        print(f"compared with {a.compare}: {n_both + len(set(other.files) - set(arrays)) - len(differ)} of {len(other.files)} arrays identical" + ("" if differ else ": ALL IDENTICAL"))
        if differ:
            sys.exit(1)


if __name__ == "__main__":
    main()
