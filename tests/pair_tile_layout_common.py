"""Populations and the recorded quantities of tests/test_gpu_pair_tile_layout.py, shared with the recorder of its fixture
(tests/golden/make_golden_pair_tile_layout.py): the paths of pair_cull_kernel (csf_pair.hip) on which a tile is filled again or
addressed differently, and which tests/test_gpu_sift_bookkeeping.py and tests/test_gpu_pair_plain_f32.py do not reach, must not
change by a bit when the tile of the plain f32 variants goes from four arrays (x | y | cos | sin) to one 16-byte record per source.

Three populations of TwoDBicycle riders built like sift_bookkeeping_common.population, three single ticks each:
  binned   4 096 in 100 m with CSF_RECV_BINNED=1: receivers in binned order (BINR) - the tile holds coordinates relative to the
           origin of the receiver group, tiles come from the candidate lists, far tiles are skipped unloaded, and a workgroup
           passes a barrier in front of a fill only once it has filled a tile (`filled`)
  wave4    4 096 in 100 m with CSF_EXPERT=1 CSF_WIDE=0: the workgroup of four waves - tiles of 1 024 sources, 16 batches,
           candidate and inside masks packed into one word.  (The engine's own choice at this size; the knob pins it.  The shape
           it is held against is the wide workgroup of eight waves, CSF_EXPERT=1 CSF_RPB=16 CSF_WIDE=1.)
  nsplit2  8 192 in 141 m with CSF_EXPERT=1 CSF_NSPLIT=2: receivers in slot order, two source chunks of 64 batches - every
           workgroup fills its tile four times between two barriers; the queue must be empty at each fill and every offset
           queued afterwards refers to the new tile
CONTRAST is the environment of the shape a case must NOT have run: the recorder runs it as well and stores its pass counters and
far-field radius, and recorder and test assert that the case's own differ (a knob that was not honoured would reproduce them).
The digest scheme is that of sift_bookkeeping_common.py.
"""
import os

import numpy as np

import sift_bookkeeping_common as sb

TICKS = sb.TICKS
CASES = {
    "binned": dict(n=4096, box=100.0, seed=31, env={"CSF_RECV_BINNED": "1"}, contrast={}),
    "wave4": dict(n=4096, box=100.0, seed=32, env={"CSF_EXPERT": "1", "CSF_WIDE": "0"},
                  contrast={"CSF_EXPERT": "1", "CSF_RPB": "16", "CSF_WIDE": "1"}),
    "nsplit2": dict(n=8192, box=141.0, seed=33, env={"CSF_EXPERT": "1", "CSF_NSPLIT": "2"}, contrast={}),
}
KNOBS = ("CSF_RECV_BINNED", "CSF_EXPERT", "CSF_WIDE", "CSF_NSPLIT", "CSF_RPB", "CSF_SEGMENTS", "CSF_FAR_EPS", "CSF_CLIST")
digest = sb.digest


def fixture_path(case):
    return os.path.join(sb.GOLDEN, f"pair_tile_layout_{case}.npz")


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


def set_env(case, setenv, delenv, contrast=False):
    """the cull-first kernel pinned, the knobs of the case (or of its contrast shape) and no others"""
    env = CASES[case]["contrast" if contrast else "env"]
    setenv("CSF_PAIR_VARIANT", "0")
    for k in KNOBS:
        if k in env:
            setenv(k, env[k])
        else:
            delenv(k)


def run(engine_cls, pod, case):
    """TICKS single ticks of the case's population: per tick the total forces, the states, the four counters of csf_count_pairs,
    the near pairs dropped so far and the name of the pair kernel.  The environment of the case must be set (set_env)."""
    s0, off, dq = population(case)
    n = s0.shape[0]
    e = engine_cls(pod("twod"), n)
    e.add_agents(s0, 5.0)
    e.set_dest_queue(np.arange(n), off, dq, reset=True)
    fx, fy, st, counts, dropped, kernels = [], [], [], [], [], []
    for _ in range(TICKS):
        e.step(1)
        s, _, _, gx, gy, _ = e.tick_snapshot(forces=True)
        fx.append(gx.copy()); fy.append(gy.copy()); st.append(s.copy())
        cnt, kernel = e.count_pairs(detail=True)
        counts.append([cnt["evaluated"], cnt["tested"], cnt["full_passes"], cnt["partial_passes"]])
        dropped.append(int(e.near_dropped()))
        kernels.append(str(kernel))
    out = dict(fx=np.array(fx), fy=np.array(fy), states=np.array(st), counts=np.array(counts, dtype=np.int64),
               near_dropped=np.array(dropped, dtype=np.int64), kernels=np.array(kernels),
               status_ok=bool((e.status() == 0).all()), far_radius=float(e.far_radius()))
    e.close()
    return out


def other_shape(counts, far_radius, contrast_counts, contrast_far_radius):
    """did these ticks run another launch shape than the contrast run?  The kernel's counters differ in every tick - other tiles:
    other passes; receivers in binned order: another rounding band, other pairs noted and evaluated again -, or the far-field
    radius does."""
    return bool((counts != contrast_counts).any(axis=1).all()) or float(far_radius) != float(contrast_far_radius)
