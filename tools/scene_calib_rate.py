#!/usr/bin/env python3
"""Time of ONE evaluation of a closed-loop calibration objective for n_sets candidate parameter sets (GPU box): (b)
csf_scene_calib_eval - the scenes resident, workgroup = (set, scene), the error summed in the launch - against (a) what a caller
had before: one engine per (set, scene) in a batch, every call their start states pushed back (csf_push_state, destination
pointers rewound), step_batch with csf_record, batch_recorded, and the NumPy error on the trajectories.  (The baseline's reset
leaves the latched navigation state and the integrators' side-state where the last call ended - it does less than a full reset
and is timed as it is.)  16 scenes of 3 - 8 riders x 1 000 ticks, TwoDBicycle and InvPendulumBicycle, n_sets in 1, 4, 16, 64, 256
(the baseline holds n_sets x 16 engines - 4 096 at 256 sets; --base-max caps it where that is too many for a box); the two paths
alternate window by window in one process, after one warm-up call of each.  One JSON line per cell, printed and appended to --out
as soon as the cell is done: medians of the windows with min / max, milliseconds per evaluation of all n_sets.

--replay adds a leg with every second rider of every scene following its recording (csf_scene_calib_replay; the recording is the
data set's own run with the base set): the same one launch per evaluation (`replay_ms`), against what the existing pieces cost -
the engines of the baseline in their batch, per tick one step_batch and per engine state() and push_state of the replayed riders,
the error in NumPy (`replay_base_ms`; --replay-base-max caps the sets it is built for, it is O(sets x scenes x ticks) host calls) -
and their ratio.  Without --replay the tool does what it did.

--road puts every scene between two road edges of --road-verts vertices each on BOTH legs - the data set gets them
through csf_scene_calib_road, every engine of the baseline through set_road before it joins its batch - and adds `road_over_ms`: the
same evaluation with road_F0 / road_sigma per candidate set (csf_scene_calib_eval_road), which the baseline has no single call for.

--presence gives every rider a random presence window of at least half the scene (csf_scene_calib_windows) and adds
`presence_ms`: the same one launch per evaluation, the instance of the kernel with the mask; the windows are dropped again before the
--replay leg.  (`--windows` was taken: it is the number of timing windows.)  The baseline has no leg for it - riders that come and go
would be add_agents / remove_agents between 1-tick calls of every engine.

--presence --share adds a cell of its own: the same number of scenes with a roster of --share-roster riders each (it fits
32) of whom --share-peak are present at a time - rider r of a scene is there for ticks x peak / roster ticks from tick r x ticks /
roster on - loaded twice on the SAME library: by csf_scene_calib_load + csf_scene_calib_windows (`unpacked_ms`, P = the power of two
that holds the roster) and by csf_scene_calib_load_shared on SceneData.lanes() (`packed_ms`, P = the one that holds the peak).  The
two legs alternate window by window after one warm-up call each; `packed_rel_gap` is the largest relative difference of their errors.

--riders 40,96 makes the scenes WIDE: scene q has riders[q % len] road users, all present throughout, in a box at the
density of 32 in 30 m; the data set is loaded by csf_scene_calib_load_wide (--wide-from, default 33) and an evaluation is one launch
per kind of scene.  The baseline leg is the tool's own: one engine per (set, scene) stepped on the engine's own path.  The option
stands alone: not with --replay, --road or --presence.

--groups G puts rider r of every scene into group r % G (G = 2: every second rider in group 1), group g carrying the
candidate's set with f_0 x (1 + 0.1 g), and adds `groups_ms`: csf_scene_calib_groups + csf_scene_calib_eval_groups, one launch per
evaluation.  Its baseline (`groups_base_ms`, built for up to --groups-base-max sets) is what a caller had before: one engine per (set,
scene) that holds the G sets as parameter classes - such an engine is on the general path and a batch steps it in turn -, per call the
start states pushed back, csf_step for all ticks with csf_record, the recorded states read back and the NumPy error.
With --riders the groups go to the wide data set through csf_scene_calib_lane_groups and the same leg and baseline
are timed there.  With --presence --share the packed data set of that cell gets them too: `packed_groups_ms`, against
`packed_groups_base_ms` - per (set, scene) one general-path engine that holds the G sets, stepped tick by tick, a rider added
(add_agents, set_agent_class, set_dest_queue) at its entry and removed at its exit, the state read back after every tick.

--mixed adds the legs of several vehicle classes in one scene on the plain data set, under "mixed":
the same scenes with rider r in group r % 2 and BOTH groups of the cell's one class, once through csf_scene_calib_groups
(`one_class_groups_ms`) and once through csf_scene_calib_classes (`one_class_classes_ms`) - the two alternate window by window, each
behind a warm-up call, and `one_class_equal` says whether their sums are array_equal: the cost of the merged kernel -, then a two-class
mix (twod, invpend: `two_classes_ms`) and a six-class mix (rider r of class r % 6: `six_classes_ms`), one launch per evaluation each.
With --riders the same legs run on the wide data set through csf_scene_calib_lane_groups / csf_scene_calib_lane_classes,
one launch per kind of scene; with --presence --share on the packed data set of that cell (under "share" -> "mixed"), where a lane changes
its class with its rider, and at 1 set `two_classes_host_stepped_ms` is what the two-class mix costs on one host-stepped general-path
engine per scene - riders added and removed between 1-tick steps - for scale.

    python tools/scene_calib_rate.py [--mixed] [--groups 2 [--groups-base-max 16]] [--sets 1,4,16,64,256] [--scenes 16] [--ticks 1000] [--windows 5] [--base-max 256] [--out FILE]
                                     [--replay [--replay-base-max 4]] [--road [--road-verts 200]] [--presence [--share [--share-roster 20] [--share-peak 6]]]
                                     [--riders 40,96 [--wide-from 33]]
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
from cyclistsocialforce_amd import _ffi, parameters  # noqa: E402
from cyclistsocialforce_amd.engine import Engine  # noqa: E402


def scene(model, n, seed, box=14.0):
    rng = np.random.default_rng(seed)
    s0 = np.zeros((n, _ffi.N_STATES[parameters.default_pod(model).model]))
    s0[:, 0], s0[:, 1] = rng.uniform(0, box, n), rng.uniform(0, box, n)
    s0[:, 2], s0[:, 3] = rng.uniform(-np.pi, np.pi, n), rng.uniform(3, 6, n)
    reach = np.array([8.0, 25.0, 60.0, 61.0])
    dq = np.zeros((n, 5, 3))
    dq[:, 0, :2] = s0[:, :2]
    dq[:, 1:, 0] = s0[:, 0:1] + reach[None, :] * np.cos(s0[:, 2:3])
    dq[:, 1:, 1] = s0[:, 1:2] + reach[None, :] * np.sin(s0[:, 2:3])
    dq[:, 4, 2] = 1.0
    return s0, np.arange(n + 1) * 5, dq.reshape(-1, 3)


def pod_sets(base, n):
    out = []
    for k in range(n):
        p = _ffi.Params.from_buffer_copy(base)
        p.f_0 = base.f_0 * (1.0 + 0.002 * k)
        p.p_0 = base.p_0 * (1.0 + 0.002 * k)
        out.append(p)
    return out


SIX = ("twod", "bicycle", "invpend", "planarpoint", "planarbike", "balancingrider")


def class_tuples(n_sets, classes):
    """candidate k: record g the default set of classes[g], its field scaled as pod_sets scales it and by 1 + 0.1 g"""
    out = []
    for k in range(n_sets):
        tup = []
        for g, m in enumerate(classes):
            c = parameters.default_pod(m)
            c.f_0, c.p_0 = c.f_0 * (1.0 + 0.002 * k) * (1.0 + 0.1 * g), c.p_0 * (1.0 + 0.002 * k) * (1.0 + 0.1 * g)
            tup.append(c)
        out.append(tuple(tup))
    return out


def ms(t):
    return dict(median=float(np.median(t)), min=min(t), max=max(t))


def mixed_legs(eng, lanes, rider, wide, n_sets, model, windows, launches):
    """the --mixed legs on the data set `eng` holds - lanes: it is on shared lanes or wide (csf_scene_calib_lane_groups / _lane_classes),
    else a plain load (csf_scene_calib_groups / _classes); rider [R]: the index of every rider in its scene; launches: per evaluation"""
    from cyclistsocialforce_amd.engine import MODEL_IDS
    groups, classes_call = (eng.scene_calib_lane_groups, eng.scene_calib_lane_classes) if lanes else (eng.scene_calib_groups, eng.scene_calib_classes)
    grp2 = (rider % 2).astype(np.uint8)
    one = class_tuples(n_sets, [model, model])
    t_grp, t_cls, equal = [], [], True
    for _ in range(windows):
        groups(grp2, 2)
        ref = eng.scene_calib_eval_groups(one)
        t0 = time.perf_counter(); eng.scene_calib_eval_groups(one); t_grp.append((time.perf_counter() - t0) * 1e3)
        classes_call(grp2, [MODEL_IDS[model]] * 2, wide)
        equal = equal and bool(np.array_equal(ref, eng.scene_calib_eval_groups(one)))
        t0 = time.perf_counter(); eng.scene_calib_eval_groups(one); t_cls.append((time.perf_counter() - t0) * 1e3)
    mixed = dict(one_class_groups_ms=ms(t_grp), one_class_classes_ms=ms(t_cls), one_class_equal=equal,
                 one_class_classes_over_groups=float(np.median(t_cls) / np.median(t_grp)))
    for name, classes in (("two_classes_ms", ("twod", "invpend")), ("six_classes_ms", SIX)):
        tups = class_tuples(n_sets, classes)
        classes_call((rider % len(classes)).astype(np.uint8), [MODEL_IDS[m] for m in classes], wide)
        before = eng.scene_calib_launches()
        eng.scene_calib_eval_groups(tups)
        assert eng.scene_calib_launches() == before + launches
        t_mix = []
        for _ in range(windows):
            t0 = time.perf_counter(); eng.scene_calib_eval_groups(tups); t_mix.append((time.perf_counter() - t0) * 1e3)
        mixed[name] = ms(t_mix)
    classes_call(None)
    return mixed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="1,4,16,64,256")
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--ticks", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--base-max", type=int, default=256)
    ap.add_argument("--models", default="twod,invpend")
    ap.add_argument("--out", default=None)
    ap.add_argument("--replay", action="store_true")
    ap.add_argument("--replay-base-max", type=int, default=4)
    ap.add_argument("--road", action="store_true")
    ap.add_argument("--road-verts", type=int, default=200)
    ap.add_argument("--presence", action="store_true")
    ap.add_argument("--share", action="store_true")
    ap.add_argument("--share-roster", type=int, default=20)
    ap.add_argument("--share-peak", type=int, default=6)
    ap.add_argument("--riders", default=None)
    ap.add_argument("--wide-from", type=int, default=33)
    ap.add_argument("--groups", type=int, default=0)
    ap.add_argument("--groups-base-max", type=int, default=16)
    ap.add_argument("--mixed", action="store_true")
    a = ap.parse_args()
    riders = [int(x) for x in a.riders.split(",")] if a.riders else None
    if riders and (a.replay or a.road or a.presence or min(riders) < 1 or max(riders) > 256):
        ap.error("--riders takes 1 .. 256 road users per scene and stands alone: not with --replay, --road or --presence")
    if a.groups and not 2 <= a.groups <= 4:
        ap.error("--groups takes 2 .. 4")
    if a.share and not (a.presence and 1 <= a.share_peak <= a.share_roster <= 32):
        ap.error("--share goes with --presence and 1 <= --share-peak <= --share-roster <= 32")
    feat = np.array([0, 1], dtype=np.int32)
    if a.out:
        open(a.out, "w").close()
    for model in a.models.split(","):
        base = parameters.default_pod(model)
        if riders:
            per = [scene(model, riders[q % len(riders)], 50 + q, box=30.0 * np.sqrt(riders[q % len(riders)] / 32.0)) for q in range(a.scenes)]
        else:
            per = [scene(model, 3 + q % 6, 50 + q) for q in range(a.scenes)]
        nr = np.array([s.shape[0] for s, _, _ in per], dtype=np.int32)
        roff = np.r_[0, np.cumsum(nr)]
        R = int(roff[-1])
        s0 = np.concatenate([s for s, _, _ in per])
        rows = np.concatenate([d for _, _, d in per])
        off = np.r_[0, np.cumsum(np.concatenate([np.diff(o) for _, o, _ in per]))]
        obj = np.random.default_rng(1).normal(size=(a.ticks, R, feat.size))
        mask = np.concatenate([np.arange(n) % 2 == 1 for n in nr])      # every second rider of a scene (>= 3 riders each)
        rec = None
        xs = np.linspace(-20.0, 34.0, a.road_verts)                 # the box is 14 m: edges 3 m below and above it
        road = (np.array([0, a.road_verts, 2 * a.road_verts]), np.r_[np.c_[xs, np.full(a.road_verts, -3.0)], np.c_[xs, np.full(a.road_verts, 17.0)]],
                np.array([0.15, 0.2]), np.array([2.0, 2.0]))
        for n_sets in [int(x) for x in a.sets.split(",")]:
            sets = pod_sets(base, n_sets)
            e = Engine(base, n_sets * R)
            if riders:                                           # every rider on a lane of its own, there throughout
                e.scene_calib_load_wide(nr, nr, np.concatenate([np.arange(n) for n in nr]), np.zeros(R, dtype=np.int32), np.full(R, a.ticks, dtype=np.int32),
                                        s0, 5.0, off, rows, obj, feat, max_sets=n_sets, wide_from=a.wide_from)
            else:
                e.scene_calib_load(nr, s0, 5.0, off, rows, obj, feat, max_sets=n_sets)
            if a.road:
                e.scene_calib_road(np.repeat(np.arange(a.scenes, dtype=np.int32), 2), np.arange(2 * a.scenes + 1) * a.road_verts,
                                   np.tile(road[1].reshape(2, -1, 2), (a.scenes, 1, 1)).reshape(-1, 2), np.tile(road[2], a.scenes), np.tile(road[3], a.scenes))
            twins = []
            if n_sets <= a.base_max:
                for pod in sets:
                    for s, o, d in per:
                        t = Engine(pod, s.shape[0])
                        t.add_agents(s, 5.0)
                        t.set_dest_queue(np.arange(s.shape[0]), o, d, reset=True)
                        if a.road:
                            t.set_road(*road)
                        t.record(stride=1, capacity=a.ticks, forces=False)
                        twins.append(t)
                Engine.batch_join(twins)

            def new():
                return e.scene_calib_eval(sets)[:, :, 0].sum(axis=1)

            def old():
                err = np.zeros(n_sets)
                for i, t in enumerate(twins):
                    s = per[i % a.scenes][0]
                    t.push_state(np.arange(s.shape[0]), s)
                    t.set_dest_pointer(np.arange(s.shape[0]), 0)
                Engine.step_batch(twins, a.ticks)
                for i, (S, _, _) in enumerate(Engine.batch_recorded(twins, a.ticks)):
                    q = i % a.scenes
                    err[i // a.scenes] += float(np.square(S[:, :, feat] - obj[:, roff[q]: roff[q + 1]]).sum())
                return err

            def replay_old():
                """the twin the replay tests compare with, for all engines of the batch: tick, read, overwrite, push"""
                err = np.zeros(n_sets)
                idx = [np.flatnonzero(mask[roff[q]: roff[q + 1]]).astype(np.int32) for q in range(a.scenes)]
                for i, t in enumerate(twins):
                    s = per[i % a.scenes][0]
                    t.push_state(np.arange(s.shape[0]), s)
                    t.set_dest_pointer(np.arange(s.shape[0]), 0)
                for tick in range(a.ticks):
                    Engine.step_batch(twins, 1)
                    for i, t in enumerate(twins):
                        q = i % a.scenes
                        s = t.state()
                        s[idx[q], :4] = rec[tick, roff[q] + idx[q], :4]
                        t.push_state(idx[q], s[idx[q]])
                        sim = np.setdiff1d(np.arange(nr[q]), idx[q])
                        err[i // a.scenes] += float(np.square(s[sim][:, feat] - obj[tick, roff[q] + sim]).sum())
                return err

            first_new = new()
            # (the first baseline call starts from fresh engines: there the two legs do the same job and their errors agree)
            first_gap = float(np.abs(old() / first_new - 1.0).max()) if twins else None
            t_new, t_old = [], []
            for _ in range(a.windows):
                t0 = time.perf_counter(); new(); t_new.append((time.perf_counter() - t0) * 1e3)
                if twins:
                    t0 = time.perf_counter(); old(); t_old.append((time.perf_counter() - t0) * 1e3)
            line = dict(model=model, n_sets=n_sets, scenes=a.scenes, riders=R, ticks=a.ticks, windows=a.windows, first_call_rel_gap=first_gap,
                        new_ms=dict(median=float(np.median(t_new)), min=min(t_new), max=max(t_new)),
                        base_ms=dict(median=float(np.median(t_old)), min=min(t_old), max=max(t_old)) if t_old else None)
            if riders:
                line.update(scene_riders=riders, wide_from=a.wide_from, launches_per_eval=e.scene_calib_launches() // (a.windows + 1))
            if a.road:
                rf, rs = 0.15 * (1.0 + 0.002 * np.arange(n_sets)), np.full(n_sets, 2.0)
                e.scene_calib_eval(sets, road_F0=rf, road_sigma=rs)          # (allocates the sets' road blocks)
                t_over = []
                for _ in range(a.windows):
                    t0 = time.perf_counter(); e.scene_calib_eval(sets, road_F0=rf, road_sigma=rs); t_over.append((time.perf_counter() - t0) * 1e3)
                line.update(road_verts=2 * a.road_verts, road_over_ms=dict(median=float(np.median(t_over)), min=min(t_over), max=max(t_over)))
            if a.presence:
                rng = np.random.default_rng(7)
                span = rng.integers((a.ticks + 1) // 2, a.ticks + 1, size=R)      # at least half the scene
                enter = rng.integers(0, a.ticks - span + 1).astype(np.int32)
                e.scene_calib_windows(enter, (enter + span).astype(np.int32))
                new()
                t_win = []
                for _ in range(a.windows):
                    t0 = time.perf_counter(); new(); t_win.append((time.perf_counter() - t0) * 1e3)
                e.scene_calib_windows(None, None)
                line["timing_windows"] = line.pop("windows")     # (in these lines "windows" would read as the presence windows)
                line.update(present_share=float(span.sum() / (a.ticks * R)), presence_ms=dict(median=float(np.median(t_win)), min=min(t_win), max=max(t_win)))
            if a.share:
                from cyclistsocialforce_amd.calibration import SceneData
                ro, pk = a.share_roster, a.share_peak
                big = [scene(model, ro, 150 + q, box=22.0) for q in range(a.scenes)]
                en1 = (np.arange(ro) * a.ticks // ro).astype(np.int32)
                ex1 = np.minimum(en1 + a.ticks * pk // ro, a.ticks).astype(np.int32)
                lane1, nl1 = SceneData(big[0][0], 5.0, big[0][1], big[0][2], np.zeros((a.ticks, ro, 4)), present=(en1, ex1)).lanes()
                nrb, Rb = np.full(a.scenes, ro, dtype=np.int32), ro * a.scenes
                sb, rb = np.concatenate([x[0] for x in big]), np.concatenate([x[2] for x in big])
                ob = np.arange(Rb + 1) * 5
                objb = np.random.default_rng(2).normal(size=(a.ticks, Rb, feat.size))
                enb, exb = np.tile(en1, a.scenes), np.tile(ex1, a.scenes)
                plain = Engine(base, n_sets * Rb)
                plain.scene_calib_load(nrb, sb, 5.0, ob, rb, objb, feat, max_sets=n_sets)
                plain.scene_calib_windows(enb, exb)
                packed = Engine(base, max(Rb, n_sets * nl1 * a.scenes))
                packed.scene_calib_load_shared(nrb, np.full(a.scenes, nl1, dtype=np.int32), np.tile(lane1, a.scenes), enb, exb, sb, 5.0, ob, rb, objb,
                                               feat, max_sets=n_sets)
                legs = [lambda: plain.scene_calib_eval(sets)[:, :, 0].sum(axis=1), lambda: packed.scene_calib_eval(sets)[:, :, 0].sum(axis=1)]
                first = [leg() for leg in legs]
                t_leg = [[], []]
                for _ in range(a.windows):
                    for k, leg in enumerate(legs):
                        t0 = time.perf_counter(); leg(); t_leg[k].append((time.perf_counter() - t0) * 1e3)
                line.update(share=dict(roster=ro, peak=pk, lanes=int(nl1), riders=Rb, packed_rel_gap=float(np.abs(first[1] / first[0] - 1.0).max()),
                                       unpacked_ms=dict(median=float(np.median(t_leg[0])), min=min(t_leg[0]), max=max(t_leg[0])),
                                       packed_ms=dict(median=float(np.median(t_leg[1])), min=min(t_leg[1]), max=max(t_leg[1]))))
                if a.groups:                                     # the packed data set with groups: a lane's set changes with its rider
                    G = a.groups
                    grpb = np.tile(np.arange(ro) % G, a.scenes).astype(np.uint8)
                    tupb = [tuple(_ffi.Params.from_buffer_copy(p) for _ in range(G)) for p in sets]
                    for tup in tupb:
                        for g, c in enumerate(tup):
                            c.f_0, c.p_0 = c.f_0 * (1.0 + 0.1 * g), c.p_0 * (1.0 + 0.1 * g)
                    packed.scene_calib_lane_groups(grpb, G)

                    def lanes_new():
                        return packed.scene_calib_eval_groups(tupb)[:, :, 0].sum(axis=1)

                    def lanes_old():
                        """the host-stepped twin: riders come and go between 1-tick steps of a general-path engine per (set, scene)"""
                        err = np.zeros(n_sets)
                        for k, tup in enumerate(tupb):
                            for q, (s, o, d) in enumerate(big):
                                t = Engine(tup[0], ro)
                                t.set_param_classes(list(tup))
                                ids = []
                                for tick in range(a.ticks):
                                    gone = [i for i, r in enumerate(ids) if ex1[r] == tick]
                                    if gone:
                                        t.remove_agents(gone)
                                        ids = [r for r in ids if ex1[r] != tick]
                                    come = [r for r in range(ro) if en1[r] == tick and ex1[r] > tick]
                                    if come:
                                        t.add_agents(s[come], 5.0)
                                        where = np.arange(len(ids), len(ids) + len(come))
                                        t.set_agent_class(where, grpb[come])
                                        t.set_dest_queue(where, np.arange(len(come) + 1) * 5, np.concatenate([d[o[r]: o[r + 1]] for r in come]), reset=True)
                                        ids += come
                                    if ids:
                                        t.step(1)
                                        st = t.state()
                                        err[k] += float(np.square(st[:, feat] - objb[tick, q * ro + np.array(ids)]).sum())
                                t.close()
                        return err

                    first_l = lanes_new()
                    with_lbase = n_sets <= a.groups_base_max
                    l_gap = float(np.abs(lanes_old() / first_l - 1.0).max()) if with_lbase else None
                    t_l, t_lold = [], []
                    for _ in range(a.windows):
                        t0 = time.perf_counter(); lanes_new(); t_l.append((time.perf_counter() - t0) * 1e3)
                        if with_lbase:
                            t0 = time.perf_counter(); lanes_old(); t_lold.append((time.perf_counter() - t0) * 1e3)
                    line["share"].update(groups=G, packed_groups_rel_gap=l_gap,
                                         packed_groups_ms=dict(median=float(np.median(t_l)), min=min(t_l), max=max(t_l)),
                                         packed_groups_base_ms=dict(median=float(np.median(t_lold)), min=min(t_lold), max=max(t_lold)) if t_lold else None)
                if a.mixed:                                      # vehicle classes on the packed data set: a lane's class changes with its rider
                    from cyclistsocialforce_amd.engine import MODEL_IDS
                    wb = np.zeros((Rb, 8))
                    wb[:, : sb.shape[1]] = sb
                    riderb = np.tile(np.arange(ro), a.scenes)
                    line["share"]["mixed"] = mixed_legs(packed, True, riderb, wb, n_sets, model, a.windows, 1)
                    if n_sets == 1:                              # for scale: the host-stepped twin of the two-class mix, one general-path engine per scene
                        two = class_tuples(1, ("twod", "invpend"))[0]
                        t0 = time.perf_counter()
                        for q, (sq, oq, dq) in enumerate(big):
                            t = Engine(two[0], ro)
                            t.set_param_classes(list(two))
                            ids = []
                            for tick in range(a.ticks):
                                gone = [i for i, r in enumerate(ids) if ex1[r] == tick]
                                if gone:
                                    t.remove_agents(gone)
                                    ids = [r for r in ids if ex1[r] != tick]
                                come = [r for r in range(ro) if en1[r] == tick and ex1[r] > tick]
                                if come:
                                    t.add_agents(wb[q * ro + np.array(come)], 5.0)
                                    where = np.arange(len(ids), len(ids) + len(come))
                                    t.set_agent_class(where, (np.array(come) % 2).astype(np.uint8))
                                    t.set_dest_queue(where, np.arange(len(come) + 1) * 5, np.concatenate([dq[oq[r]: oq[r + 1]] for r in come]), reset=True)
                                    ids += come
                                if ids:
                                    t.step(1)
                                    t.state()
                            t.close()
                        line["share"]["mixed"]["two_classes_host_stepped_ms"] = (time.perf_counter() - t0) * 1e3
                plain.close()
                packed.close()
            if a.replay:
                if rec is None:                                  # the recording: the scenes' own run with the base set
                    rec = e.scene_calib_eval([base], states=True)[1][:, :R]
                e.scene_calib_replay(mask, rec[:, mask, :4])
                first_rep = new()
                with_base = bool(twins) and n_sets <= a.replay_base_max
                gap = float(np.abs(replay_old() / first_rep - 1.0).max()) if with_base else None
                t_rep, t_rold = [], []
                for _ in range(a.windows):
                    t0 = time.perf_counter(); new(); t_rep.append((time.perf_counter() - t0) * 1e3)
                    if with_base:
                        t0 = time.perf_counter(); replay_old(); t_rold.append((time.perf_counter() - t0) * 1e3)
                line.update(replayed_riders=int(mask.sum()), replay_first_call_rel_gap=gap,
                            replay_ms=dict(median=float(np.median(t_rep)), min=min(t_rep), max=max(t_rep)),
                            replay_base_ms=dict(median=float(np.median(t_rold)), min=min(t_rold), max=max(t_rold)) if t_rold else None,
                            replay_base_over_replay=float(np.median(t_rold) / np.median(t_rep)) if t_rold else None)
            if a.groups:
                G = a.groups
                if a.replay:
                    e.scene_calib_replay(None)
                grp = np.concatenate([np.arange(n) % G for n in nr]).astype(np.uint8)
                tups = []
                for p in sets:
                    tup = []
                    for g in range(G):
                        c = _ffi.Params.from_buffer_copy(p)
                        c.f_0, c.p_0 = p.f_0 * (1.0 + 0.1 * g), p.p_0 * (1.0 + 0.1 * g)
                        tup.append(c)
                    tups.append(tuple(tup))
                (e.scene_calib_lane_groups if riders else e.scene_calib_groups)(grp, G)    # (--riders: the data set is on lanes)
                gtwins = []
                if n_sets <= a.groups_base_max:
                    for tup in tups:
                        for q, (s, o, d) in enumerate(per):
                            t = Engine(tup[0], s.shape[0])
                            t.set_param_classes(list(tup))
                            t.add_agents(s, 5.0)
                            t.set_agent_class(np.arange(s.shape[0]), grp[roff[q]: roff[q + 1]])
                            t.set_dest_queue(np.arange(s.shape[0]), o, d, reset=True)
                            if a.road:
                                t.set_road(*road)
                            t.record(stride=1, capacity=a.ticks, forces=False)
                            gtwins.append(t)

                def groups_new():
                    return e.scene_calib_eval_groups(tups)[:, :, 0].sum(axis=1)

                g_calls = [0]                                   # (csf_record numbers its samples from the engine's first tick)

                def groups_old():
                    err = np.zeros(n_sets)
                    for i, t in enumerate(gtwins):
                        s = per[i % a.scenes][0]
                        t.push_state(np.arange(s.shape[0]), s)
                        t.set_dest_pointer(np.arange(s.shape[0]), 0)
                        t.step(a.ticks)
                    for i, t in enumerate(gtwins):
                        q = i % a.scenes
                        S, _ = t.recorded(g_calls[0] * a.ticks, a.ticks)
                        err[i // a.scenes] += float(np.square(S[:, :, feat] - obj[:, roff[q]: roff[q + 1]]).sum())
                    g_calls[0] += 1
                    return err

                first_g = groups_new()
                g_gap = float(np.abs(groups_old() / first_g - 1.0).max()) if gtwins else None
                t_g, t_gold = [], []
                for _ in range(a.windows):
                    t0 = time.perf_counter(); groups_new(); t_g.append((time.perf_counter() - t0) * 1e3)
                    if gtwins:
                        t0 = time.perf_counter(); groups_old(); t_gold.append((time.perf_counter() - t0) * 1e3)
                line.update(groups=G, groups_first_call_rel_gap=g_gap,
                            groups_ms=dict(median=float(np.median(t_g)), min=min(t_g), max=max(t_g)),
                            groups_base_ms=dict(median=float(np.median(t_gold)), min=min(t_gold), max=max(t_gold)) if t_gold else None)
                for t in gtwins:
                    t.close()
            if a.mixed:                                          # (--riders: the data set is on lanes - DESIGN.md 4.10j)
                e.scene_calib_replay(None)
                wide = np.zeros((R, 8))
                wide[:, : s0.shape[1]] = s0
                rider = np.concatenate([np.arange(n) for n in nr])
                kinds = len({n >= a.wide_from for n in nr}) if riders else 1
                line["mixed"] = mixed_legs(e, bool(riders), rider, wide, n_sets, model, a.windows, kinds)
            print(json.dumps(line), flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
            for t in twins:
                t.close()
            e.close()


if __name__ == "__main__":
    main()
