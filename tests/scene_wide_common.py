"""Shared by tests/test_gpu_scene_wide.py, tests/test_scene_wide_host.py and tests/scene_wide_abi_child.py: scenes with more than 32
road users at once - the crowds, a loaded engine, and the engine's own population path as the twin."""
import numpy as np

from scene_calib_common import VDES, crowd
from scene_lanes_common import LANES_T, cat_parts
from scene_windows_common import FEAT

from cyclistsocialforce_amd import _ffi
from cyclistsocialforce_amd.engine import MODEL_IDS

WIDE_SEED = 72                                                   # (71 is chaotic on this horizon for the BalancingRider: see the host test)
WIDE_N = (33, 65, 130)                                           # P = 64 / 128 / 256, G = 4 / 2 / 1; owners in 1 / 2 / 3 waves


def wide_crowd(model, n, seed=WIDE_SEED):
    """(s0, off, dq) of n road users at the density of scene_calib_common.scenes' 32 in a box of 30 m (the box doubled for the
    BalancingRider, as there)"""
    box = 30.0 * np.sqrt(n / 32.0) * (2.0 if model == "balancingrider" else 1.0)
    x, y, psi, v, off, dq = crowd(n, seed=seed, box=box)
    s0 = np.zeros((n, _ffi.N_STATES[MODEL_IDS[model]]))
    s0[:, 0], s0[:, 1], s0[:, 2], s0[:, 3] = x, y, psi, v
    return s0, off, dq


def always(n, ticks=LANES_T):
    """(lane, n_lanes), enter, exit of n road users that are there throughout: lane = index"""
    return (np.arange(n, dtype=np.int32), n), np.zeros(n, dtype=np.int32), np.full(n, ticks, dtype=np.int32)


def loaded_wide(sets, parts, lanes, enter, exit, obj, wide_from=33, lengths=None, feat=FEAT, max_sets=None):
    """scene_lanes_common.loaded_shared by csf_scene_calib_load_wide"""
    from cyclistsocialforce_amd.engine import Engine
    nr, s0, off, rows = cat_parts(parts)
    nl = np.array([l[1] for l in lanes], dtype=np.int32)
    K = len(sets) if max_sets is None else max_sets
    e = Engine(sets[0], max(int(nr.sum()), K * int(nl.sum())))
    e.scene_calib_load_wide(nr, nl, np.concatenate([l[0] for l in lanes]), enter, exit, s0, VDES, off, rows, obj, feat, lengths=lengths, max_sets=K,
                            wide_from=wide_from)
    return e


def pop_twin(pod, s0, off, dq, ticks, road=None, vdes=VDES):
    """the engine's own population path: a stand-alone engine created with that set holds the scene (and its road), steps `ticks` ticks
    in one csf_step call and records at stride 1; states [ticks, n, n_states]"""
    from cyclistsocialforce_amd.engine import Engine
    n = s0.shape[0]
    e = Engine(pod, n)
    e.add_agents(s0, vdes)
    e.set_dest_queue(np.arange(n), off, dq, reset=True)
    if road is not None:
        e.set_road(*road)
    e.record(stride=1, capacity=max(ticks, 1), forces=False)
    e.step(ticks)
    S, _ = e.recorded(0, ticks)
    e.close()
    return S


def edge_below(model, n, count=100, f0=6.0, sigma=2.0):
    """one road edge of `count` vertices below the box of wide_crowd(model, n), as Engine.set_road takes it"""
    box = 30.0 * np.sqrt(n / 32.0) * (2.0 if model == "balancingrider" else 1.0)
    verts = np.c_[np.linspace(-20.0, box + 20.0, count), np.full(count, -3.0)]
    return np.array([0, count], dtype=np.int64), verts, np.array([f0]), np.array([sigma])


def windows_80(ticks=LANES_T):
    """a roster of 80 whose peak is 40: rider r enters at tick r and stays 40 ticks; rider 7 is never present"""
    enter = np.arange(80, dtype=np.int32)
    exit = np.minimum(enter + 40, ticks).astype(np.int32)
    exit[7] = enter[7]
    return enter, exit
