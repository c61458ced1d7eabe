"""The optional layers of a closed-loop calibration data set (replay, roads, windows, groups, lane groups, classes) as
the caller sees them, whatever holds them on the host: a REFUSED call leaves the data set as it was, and a layer that is set and dropped
again leaves the evaluation it had before.  Both are array_equal on sums and sampled states: nothing here depends on a rounding.

TwoDBicycle; the plain data set is two scenes of 3 and 5 riders (the second 45 ticks long), the shared one a roster of 6 on 3 lanes with
a handover; 60 ticks, 3 candidate sets, states at stride 10."""
import numpy as np
import pytest

from scene_calib_common import VDES, scenes
from scene_groups_common import group_sets
from scene_lanes_common import greedy_lanes, loaded_shared, roster
from scene_mixed_common import mixed_sets
from scene_wide_common import edge_below
from scene_windows_common import FEAT, sets3

pytestmark = pytest.mark.gpu

MODEL = "twod"
T, STRIDE = 60, 10
N_RIDERS = np.array([3, 5], dtype=np.int32)
LENGTHS = np.array([T, 45], dtype=np.int32)
R = int(N_RIDERS.sum())
GROUP = (np.arange(R) % 2).astype(np.uint8)
CLASSES = ("twod", "invpend")                                   # five and six states: Engine.ns changes while they are held
ENTER = np.array([0, 7, 30, 0, 12, 0, 20, 44], dtype=np.int32)   # rider 2: never present; scene 1 ends at tick 45
EXIT = np.array([T, 41, 30, 45, 45, 33, 21, 45], dtype=np.int32)
REPLAYED = np.arange(R) == 4
S_ENTER = np.array([0, 0, 0, 30, 25, 50], dtype=np.int32)        # the shared roster: rider 3 takes lane 0 over from rider 0
S_EXIT = np.array([30, 25, T, T, 50, T], dtype=np.int32)


def _plain():
    from cyclistsocialforce_amd.engine import Engine
    sets = sets3(MODEL)
    s0, off, rows, _ = scenes(MODEL, N_RIDERS, seed=5)
    obj = np.random.default_rng(11).normal(size=(T, R, len(FEAT)))
    e = Engine(sets[0], 3 * R)
    e.scene_calib_load(N_RIDERS, s0, VDES, off, rows, obj, FEAT, lengths=LENGTHS, max_sets=3)
    return e, s0


def _shared():
    lanes = greedy_lanes(S_ENTER, S_EXIT)
    assert lanes[1] == 3
    obj = np.random.default_rng(12).normal(size=(T, 6, len(FEAT)))
    return loaded_shared(sets3(MODEL), [roster(MODEL, 6, seed=63)], [lanes], S_ENTER, S_EXIT, obj), None


def _roads(bad=False):
    edges = [edge_below(MODEL, 3, count=100), edge_below(MODEL, 5, count=101)]
    verts = np.concatenate([e[1] for e in edges])
    if bad:
        verts[150, 1] = np.inf
    return (np.arange(2, dtype=np.int32), np.array([0, 100, 201], dtype=np.int64), verts, np.concatenate([e[2] for e in edges]),
            np.concatenate([e[3] for e in edges]))


def _plain_eval(e):
    return e.scene_calib_eval(sets3(MODEL), states=True, stride=STRIDE)


def _group_eval(e):
    return e.scene_calib_eval_groups(group_sets(MODEL, 3, 2), states=True, stride=STRIDE)


def _class_eval(e):
    return e.scene_calib_eval_groups(mixed_sets(3, CLASSES), states=True, stride=STRIDE)


def _recording(e):
    _, st = e.scene_calib_eval(sets3(MODEL), states=True)
    return np.ascontiguousarray(np.nan_to_num(st[:, R + np.flatnonzero(REPLAYED), :4]))


def _bad(a, at, value):
    a = np.array(a, copy=True)
    a[at] = value
    return a


def _class_models():
    from cyclistsocialforce_amd.engine import MODEL_IDS
    return [MODEL_IDS[c] for c in CLASSES]


# layer -> (engine, set, the refused call, drop, the evaluation with the layer held); every lambda takes (engine, s0, recording)
LAYERS = {
    "road": (_plain, lambda e, s0, rec: e.scene_calib_road(*_roads()),
             lambda e, s0, rec: e.scene_calib_road(*_roads(bad=True)),                                   # a vertex that is not finite
             lambda e: e.scene_calib_road(None, None, None, None, None),
             lambda e: e.scene_calib_eval(sets3(MODEL), states=True, stride=STRIDE, road_F0=(4.0, 7.5, 0.0), road_sigma=(2.0, 2.5, 3.0))),
    "replay": (_plain, lambda e, s0, rec: e.scene_calib_replay(REPLAYED, rec),
               lambda e, s0, rec: e.scene_calib_replay(REPLAYED, _bad(rec, (20, 0, 1), np.nan)),         # a recorded row that is not finite
               lambda e: e.scene_calib_replay(None), _plain_eval),
    "windows": (_plain, lambda e, s0, rec: e.scene_calib_windows(ENTER, EXIT),
                lambda e, s0, rec: e.scene_calib_windows(ENTER, _bad(EXIT, 7, 46)),                      # a window past the end of scene 1
                lambda e: e.scene_calib_windows(None, None), _plain_eval),
    "groups": (_plain, lambda e, s0, rec: e.scene_calib_groups(GROUP, 2),
               lambda e, s0, rec: e.scene_calib_groups(_bad(GROUP, 3, 2), 2),                            # rider 3 in group 2 of 2
               lambda e: e.scene_calib_groups(None), _group_eval),
    "classes": (_plain, lambda e, s0, rec: e.scene_calib_classes(GROUP, _class_models(), s0),
                lambda e, s0, rec: e.scene_calib_classes(_bad(GROUP, 3, 2), _class_models(), s0),        # rider 3 in group 2 of 2
                lambda e: e.scene_calib_classes(None), _class_eval),
    "lane_groups": (_shared, lambda e, s0, rec: e.scene_calib_lane_groups((np.arange(6) % 2).astype(np.uint8), 2),
                    lambda e, s0, rec: e.scene_calib_lane_groups(_bad(np.arange(6) % 2, 5, 2).astype(np.uint8), 2),
                    lambda e: e.scene_calib_lane_groups(None), _group_eval),
}


def _same(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)


@pytest.mark.parametrize("layer", list(LAYERS))
def test_a_refused_call_changes_nothing_and_a_dropped_layer_leaves_none(layer):
    from cyclistsocialforce_amd.engine import EngineError
    load, set_, refused, drop, held_eval = LAYERS[layer]
    e, s0 = load()
    ns = e.ns
    rec = _recording(e) if layer == "replay" else None
    before = _plain_eval(e)
    assert np.isfinite(before[0]).all() and np.any(before[0] != 0.0)
    with pytest.raises(EngineError):                              # refused with nothing held ...
        refused(e, s0, rec)
    assert _same(before, _plain_eval(e))
    set_(e, s0, rec)
    held = held_eval(e)
    assert not _same(before, held), "the layer does not act on this data set"
    with pytest.raises(EngineError):                              # ... and with the layer held: it stays as it was set
        refused(e, s0, rec)
    assert _same(held, held_eval(e))
    if layer == "classes":
        assert e.ns == 6                                          # (the InvPendulum's six states)
    drop(e)
    assert e.ns == ns
    assert _same(before, _plain_eval(e))
    e.close()
