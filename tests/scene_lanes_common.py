"""Shared by tests/test_gpu_scene_lanes.py, tests/test_scene_lanes_host.py and tests/scene_lanes_abi_child.py: scenes whose roster
shares the lanes of the one-wave tick - rosters, windows, the greedy lanes, a loaded engine, and the CPU oracle on a
membership that changes."""
import numpy as np

from scene_calib_common import VDES, scenes
from scene_windows_common import FEAT, TWIN_TOL, check_sums, extent, inside, sets3, sums_over_windows, window_twin  # noqa: F401

LANES_T = 120


def greedy_lanes(enter, exit):
    """(lane [n], n_lanes) as SceneData.lanes() defines them, written out a second time: in order of (enter, index) every rider with
    a non-empty window takes the lowest lane whose last occupant has left; an empty window takes nothing (lane 0)"""
    enter, exit = np.asarray(enter), np.asarray(exit)
    lane, free_at = np.zeros(enter.size, dtype=np.int32), []
    order = sorted((int(enter[i]), i) for i in range(enter.size) if exit[i] > enter[i])
    for en, i in order:
        k = next((k for k, x in enumerate(free_at) if x <= en), len(free_at))
        if k == len(free_at):
            free_at.append(0)
        lane[i], free_at[k] = k, int(exit[i])
    return lane, max(1, len(free_at))


def peak(enter, exit, ticks):
    """the largest number of riders present at one tick, by counting"""
    return int(inside(enter, exit, ticks).sum(axis=1).max()) if ticks else 0


def roster(model, n, seed, short=False):
    """(s0, off, dq) of n riders - any n - from scene_calib_common.scenes"""
    _, _, _, per = scenes(model, np.array([n]), seed=seed, short=(0,) if short else ())
    return per[0]


def windows_40():
    """40 riders, T = 120: rider r is there for 24 ticks from tick 2 r on, so 12 are present at the peak; rider 7 never is"""
    enter = (2 * np.arange(40)).astype(np.int32)
    exit = np.minimum(enter + 24, LANES_T).astype(np.int32)
    exit[7] = enter[7]
    return enter, exit


def windows_48():
    """48 riders on 32 lanes, T = 120: riders 0 - 31 enter at ticks 0 - 31, riders 0 - 15 leave at ticks 60 - 75 and riders 32 - 47 take
    their lanes over at those very ticks (no idle tick); 32 are present from tick 31 to the end"""
    enter, exit = np.zeros(48, dtype=np.int32), np.full(48, LANES_T, dtype=np.int32)
    enter[:32] = np.arange(32)
    exit[:16] = 60 + np.arange(16)
    enter[32:] = 60 + np.arange(16)
    return enter, exit


CROWDS = {40: (windows_40, 61), 48: (windows_48, 62)}            # roster -> (its windows, the seed of its riders): test 3's two scenes


def oracle_windowed(pod, s0, off, dq, enter, exit, ticks, vdes=VDES):
    """The CPU oracle on a scene whose road users enter and leave.  The oracle has no call that adds or removes a road user, so its
    population is built anew at every tick the membership changes - the present riders in roster order - and those who stay are
    carried over: state, destination pointer, navigation state, ring column and the InvPendulum's LTI side-state (not the ring's
    history and the latched navigation parameters - good enough to see whether a horizon is chaotic, not a reference for bits).
    Returns positions [ticks, n, 2] after every tick, NaN where the rider is absent."""
    from oracle import csf_oracle as orc
    from cyclistsocialforce_amd.engine import MODEL_IDS
    params = orc.Params.from_buffer_copy(bytes(pod))
    lti = params.model == MODEL_IDS["invpend"]
    n = s0.shape[0]
    out = np.full((ticks, n, 2), np.nan)
    kept, pop, ids = {}, None, []
    for t in range(ticks):
        want = [r for r in range(n) if enter[r] <= t < exit[r]]
        if want != ids:
            if pop is not None:
                s, (ptr, zn, col, _) = pop.state(), pop.nav()
                x, z = pop.lti() if lti else (None, None)
                for k, r in enumerate(ids):
                    kept[r] = (s[k], ptr[k], zn[k], col[k], x[k] if lti else None, z[k] if lti else None)
            ids, pop = want, None
            if ids:
                qoff = np.r_[0, np.cumsum([off[r + 1] - off[r] for r in ids])]
                pop = orc.Population(params, s0[ids], vdes, qoff, np.concatenate([dq[off[r]: off[r + 1]] for r in ids]))
                old = [k for k, r in enumerate(ids) if r in kept]
                if old:
                    s, (ptr, zn, col, _) = pop.state(), pop.nav()
                    zn = zn.astype(np.uint8)
                    for k in old:
                        s[k], ptr[k], zn[k], col[k] = kept[ids[k]][:4]
                    pop.push_state(s, ptr, zn, col)
                    if lti:
                        x, z = pop.lti()
                        for k in old:
                            x[k], z[k] = kept[ids[k]][4:]
                        pop.set_lti(x, z)
        if pop is not None:
            pop.step(1)
            out[t, ids] = pop.state()[:, :2]
    return out


def cat_parts(parts):
    """the riders of several scenes one after the other: (n_riders, s0, off, rows)"""
    nr = np.array([p[0].shape[0] for p in parts], dtype=np.int32)
    s0 = np.concatenate([p[0] for p in parts])
    rows = np.concatenate([p[2] for p in parts])
    off, at = [0], 0
    for p in parts:
        off.extend((p[1][1:] + at).tolist())
        at += p[2].shape[0]
    return nr, s0, np.array(off, dtype=np.int64), rows


def loaded_shared(sets, parts, lanes, enter, exit, obj, lengths=None, feat=FEAT, max_sets=None):
    """an engine that holds the scenes `parts` on shared lanes: lanes = [(lane [n], n_lanes), ...] per scene, enter / exit over all riders"""
    from cyclistsocialforce_amd.engine import Engine
    nr, s0, off, rows = cat_parts(parts)
    nl = np.array([l[1] for l in lanes], dtype=np.int32)
    K = len(sets) if max_sets is None else max_sets
    e = Engine(sets[0], max(int(nr.sum()), K * int(nl.sum())))
    e.scene_calib_load_shared(nr, nl, np.concatenate([l[0] for l in lanes]), enter, exit, s0, VDES, off, rows, obj, feat, lengths=lengths, max_sets=K)
    return e


def loaded_plain(sets, parts, obj, lengths=None, enter=None, exit=None, feat=FEAT):
    """the same scenes by csf_scene_calib_load (+ csf_scene_calib_windows): slot = set x R + rider"""
    from cyclistsocialforce_amd.engine import Engine
    nr, s0, off, rows = cat_parts(parts)
    e = Engine(sets[0], len(sets) * int(nr.sum()))
    e.scene_calib_load(nr, s0, VDES, off, rows, obj, feat, lengths=lengths, max_sets=len(sets))
    if enter is not None:
        e.scene_calib_windows(enter, exit)
    return e
