"""Populations and the recorded quantities of tests/test_gpu_pair_plain_f32.py, shared with the recorder of its fixture
(tests/golden/make_golden_pair_plain_f32.py): the instantiations of pair_cull_kernel (csf_pair.hip) that
tests/test_gpu_sift_bookkeeping.py does not reach must not change by a bit either when the reach test and the field pass are issued
as plain f32 instructions instead of packed ones.

Three populations of 4 096 TwoDBicycle riders in a 100 m box, three ticks each.  At this size the engine's own choice is the
workgroup of four waves with 16 receivers on tiles of 1 024 sources (csf_engine.hip: set_chunks) - the kernel the `headline` case of
tests/sift_bookkeeping_common.py runs as well:
  p2r    priority to the right on that four-wave kernel: the P2R instantiation - keep_half<FOV, true>, the side test beside the
         field-of-view test in the sift
  seg    two parameter sets of 2 048 riders each in the class-segmented order (CSF_SEGMENTS=1): the SEG instantiation, which always
         takes the wide workgroup of eight waves - one grid for both runs, every run one tile of 2 048 sources
  rpb16  the headline population of tests/sift_bookkeeping_common.py on the wide workgroup of eight waves with 16 receivers and tiles
         of 2 048 sources, the instantiation an 8-way shard of the headline takes.  Launch-shape knobs are honoured with CSF_EXPERT=1
         only, and at 4 096 riders the wide workgroup has to be asked for: CSF_EXPERT=1 CSF_RPB=16 CSF_WIDE=1.  (Same riders as
         `headline`, other tiles: the test holds the pass counters of the two fixtures against each other to show the other kernel ran.)
The digest scheme is that of sift_bookkeeping_common.py.
"""
import os

import numpy as np

import sift_bookkeeping_common as sb

TICKS = sb.TICKS
SETS = [dict(), dict(hfov=1.2 * np.pi, f_0=10.0, sigma_0=0.6, sigma_1=5.5)]
CASES = {
    "p2r": dict(n=4096, box=100.0, seed=21, rule=1, sets=None, env={}),
    "seg": dict(n=4096, box=100.0, seed=22, rule=0, sets=SETS, env={"CSF_SEGMENTS": "1"}),
    "rpb16": dict(n=4096, box=100.0, seed=11, rule=0, sets=None, env={"CSF_EXPERT": "1", "CSF_RPB": "16", "CSF_WIDE": "1"}),
}
KNOBS = ("CSF_SEGMENTS", "CSF_EXPERT", "CSF_RPB", "CSF_WIDE", "CSF_FAR_EPS")
digest = sb.digest


def fixture_path(case):
    return os.path.join(sb.GOLDEN, f"pair_plain_f32_{case}.npz")


def population(case):
    """the populations of sift_bookkeeping_common.py: uniform positions and headings, 3 - 6 m/s, three destinations straight ahead"""
    c = CASES[case]
    n, box = c["n"], c["box"]
    rng = np.random.default_rng(c["seed"])
    s0 = np.zeros((n, 5))
    s0[:, 0] = rng.uniform(0, box, n); s0[:, 1] = rng.uniform(0, box, n)
    s0[:, 2] = rng.uniform(-np.pi, np.pi, n); s0[:, 3] = rng.uniform(3, 6, n)
    d = np.array([50.0, 99.0, 100.0])
    dq = np.zeros((n, 4, 3))
    dq[:, 0, 0] = s0[:, 0]; dq[:, 0, 1] = s0[:, 1]
    dq[:, 1:, 0] = s0[:, 0, None] + d[None, :] * np.cos(s0[:, 2])[:, None]
    dq[:, 1:, 1] = s0[:, 1, None] + d[None, :] * np.sin(s0[:, 2])[:, None]
    return s0, np.arange(n + 1) * 4, dq.reshape(-1, 3)


def classes(case):
    """parameter set of every rider (None: one set): the two sets alternate, 2 048 riders each"""
    c = CASES[case]
    return None if c["sets"] is None else (np.arange(c["n"]) % len(c["sets"])).astype(np.uint8)


def set_env(case, setenv, delenv):
    """the cull-first kernel pinned, the knobs of the case and no others"""
    setenv("CSF_PAIR_VARIANT", "0")
    for k in KNOBS:
        if k in CASES[case]["env"]:
            setenv(k, CASES[case]["env"][k])
        else:
            delenv(k)


def run(engine_cls, pod, case):
    """TICKS single ticks of the case's population (sift_bookkeeping_common.run with the case's rule and parameter sets): per tick
    the total forces, the states and the four counters of csf_count_pairs.  The environment of the case must be set (set_env)."""
    c = CASES[case]
    s0, off, dq = population(case)
    n = s0.shape[0]
    pods = [pod("twod", priority_rule=c["rule"], **kw) for kw in (c["sets"] or [dict()])]
    e = engine_cls(pods[0], n)
    e.add_agents(s0, 5.0)
    e.set_dest_queue(np.arange(n), off, dq, reset=True)
    if c["sets"] is not None:
        e.set_param_classes(pods, classes(case))
    fx, fy, st, counts = [], [], [], []
    for _ in range(TICKS):
        e.step(1)
        s, _, _, gx, gy, _ = e.tick_snapshot(forces=True)
        fx.append(gx.copy()); fy.append(gy.copy()); st.append(s.copy())
        cnt, kernel = e.count_pairs(detail=True)
        assert kernel == "pair_cull_kernel", kernel
        counts.append([cnt["evaluated"], cnt["tested"], cnt["full_passes"], cnt["partial_passes"]])
    out = dict(fx=np.array(fx), fy=np.array(fy), states=np.array(st), counts=np.array(counts, dtype=np.int64),
               near_dropped=e.near_dropped(), status_ok=bool((e.status() == 0).all()), far_radius=e.far_radius())
    e.close()
    return out
