"""Shared by tests/test_gpu_scene_replay.py and tests/test_scene_replay_host.py: the data set of the replay tests and the oracle
stepped with replayed riders."""
import numpy as np

from scene_calib_common import ORACLE_TICKS, oracle_case, scenes

# Six scenes in one data set: every index path of the replay - a scene with one replayed rider, one that ends early, a full wave
# with both end lanes replayed, one without a replay between scenes with one, one whose riders are all replayed, an empty one.
N_RIDERS = np.array([2, 5, 32, 4, 3, 1], dtype=np.int32)
T = 40
LENGTHS = np.array([T, 25, T, T, T, 0], dtype=np.int32)
TRUE_SET = 1                                                     # the set of field_sets(model, 3) the recording is made with


# The seeds of the scenes (scene_calib_common.scenes, one scene per call).  "The replay acts" asks that every simulated rider of the
# first three scenes moves when the others are put on a recording, and a rider that never has a replayed one in its field of view
# does not: with most seeds some rider of these scenes is such a one.  The three seeds below are those of 0 .. 399 (0 .. 1 499 for the
# 32 riders) at which the CPU oracle - TwoD, 40 ticks, the first set of field_sets against a recording made with the second - moves
# the least affected simulated rider the most: 2.1e-2, 8.8e-5 and 7.2e-6 m, against a rounding of 1e-15 m.
# tests/test_scene_replay_host.py::test_every_simulated_rider_of_the_first_three_scenes_feels_the_replay holds them to 1e-6 m.
SCENE_SEEDS = (86, 66, 1286, 4, 5, 6)


def replay_scenes(model):
    """the six scenes as scene_calib_common.scenes returns a data set: (s0 [R, n_states], dest_offsets [R + 1], dest rows, per scene)"""
    s_all, rows_all, off_all, per, rows = [], [], [0], [], 0
    for n, seed in zip(N_RIDERS, SCENE_SEEDS):
        s0, off, dq, one = scenes(model, np.array([n]), seed=seed)
        per.append(one[0])
        s_all.append(s0)
        rows_all.append(dq)
        off_all.extend((off[1:] + rows).tolist())
        rows += dq.shape[0]
    return np.concatenate(s_all), np.array(off_all, dtype=np.int64), np.concatenate(rows_all), per


def masks():
    """the replayed riders of every scene, and of the data set"""
    per = [np.zeros(int(n), dtype=bool) for n in N_RIDERS]
    per[0][1] = True
    per[1][[0, 3]] = True
    per[2][::3] = True
    per[2][[0, 31]] = True
    per[4][:] = True
    per[5][:] = True
    return per, np.concatenate(per)


# ---- the oracle case: twod, 5 riders under the priority-to-the-right rule (the scene of ORACLE_CASES[1]), riders 1 and 3 replayed
ORACLE_CASE = ("twod", 5, 1, None)
ORACLE_REPLAYED = np.array([False, True, False, True, False])
ORACLE_TRUE_SET = 1                                              # the recording is an oracle run with the second of the three sets


def oracle_recording():
    """(s0, off, dq, the three sets, recording [ORACLE_TICKS, n, n_states]): the oracle free with the true set, every tick kept"""
    from oracle import csf_oracle as orc
    s, off, dq, pods = oracle_case(*ORACLE_CASE)
    pop = orc.Population(orc.Params.from_buffer_copy(bytes(pods[ORACLE_TRUE_SET])), s, 5.0, off, dq)
    rec = []
    for _ in range(ORACLE_TICKS):
        pop.step(1)
        rec.append(pop.state().copy())
    return s, off, dq, pods, np.array(rec)


def oracle_replay_run(pod, s0, off, dq, rec, replayed, ticks=ORACLE_TICKS, stride=10):
    """orc.Population stepped tick by tick, the replayed riders put on rec[t, :, :4] behind every tick with the oracle's own
    push_state (the state of the others is pushed back unchanged): positions [ticks // stride, n, 2] after every stride-th tick"""
    from oracle import csf_oracle as orc
    pop = orc.Population(orc.Params.from_buffer_copy(bytes(pod)), s0, 5.0, off, dq)
    out = []
    for t in range(ticks):
        pop.step(1)
        s = pop.state()
        s[replayed, :4] = rec[t, replayed, :4]
        pop.push_state(s)
        if (t + 1) % stride == 0:
            out.append(s[:, :2].copy())
    return np.array(out)
