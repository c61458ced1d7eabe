"""Populations and the recorded quantities of tests/test_gpu_sift_bookkeeping.py, shared with the recorder of its fixture
(tests/golden/make_golden_sift_bookkeeping.py): what the sift -> queue -> field passes of pair_cull_kernel (csf_pair.hip)
produce must not change by a bit when their address and queue bookkeeping does.

Four populations of TwoDBicycle riders, the smallest at which the wide cull-first workgroup runs (tiles of 2 048 sources):
  headline  4 096 in a 100 m box, default field of view - the density of bench.py: batches wholly inside the field of view and
            partial ones side by side, and (receiver, tile) visits that keep nothing
  crowd     4 096 in 45 m with hfov = 4.0 (tests/test_gpu_chase.py) - several hundred sources kept per visit, so the queue's
            ring wraps many times; near pairs and pairs within rounding of a field-of-view edge
  ragged    4 096 + 37 in 100 m - the last tile is partial and its one batch has no partner in the packed test
  everypair the headline with CSF_FAR_EPS=0 - no reach test: the every-pair append path
"""
import hashlib
import os

import numpy as np

TICKS = 3
CASES = {
    "headline": dict(n=4096, box=100.0, seed=11, hfov=None, far_eps=None),
    "crowd": dict(n=4096, box=45.0, seed=11, hfov=4.0, far_eps=None),
    "ragged": dict(n=4096 + 37, box=100.0, seed=12, hfov=None, far_eps=None),
    "everypair": dict(n=4096, box=100.0, seed=11, hfov=None, far_eps="0"),
}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture_path(case):
    return os.path.join(GOLDEN, f"sift_bookkeeping_{case}.npz")


def population(case):
    """uniform positions and headings, 3 - 6 m/s, three destinations straight ahead (the crowd of tests/test_gpu_chase.py)"""
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


def overrides(case):
    hfov = CASES[case]["hfov"]
    return {} if hfov is None else {"hfov": hfov}


def set_env(case, setenv, delenv):
    """the cull-first kernel pinned (tests/conftest.py does the same for the suite), the far-field bound of the case"""
    setenv("CSF_PAIR_VARIANT", "0")
    if CASES[case]["far_eps"] is None:
        delenv("CSF_FAR_EPS")
    else:
        setenv("CSF_FAR_EPS", CASES[case]["far_eps"])


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run(engine_cls, pod, case):
    """TICKS single ticks of the case's population; per tick the total forces and the states csf_get_tick returns and the four
    counters of csf_count_pairs for the snapshot that tick left.  The environment of the case must be set (set_env)."""
    s0, off, dq = population(case)
    n = s0.shape[0]
    e = engine_cls(pod("twod", **overrides(case)), n)
    e.add_agents(s0, 5.0)
    e.set_dest_queue(np.arange(n), off, dq, reset=True)
    fx, fy, st, counts = [], [], [], []
    for _ in range(TICKS):
        e.step(1)
        s, _, _, gx, gy, _ = e.tick_snapshot(forces=True)
        fx.append(gx.copy()); fy.append(gy.copy()); st.append(s.copy())
        c, kernel = e.count_pairs(detail=True)
        assert kernel == "pair_cull_kernel", kernel
        counts.append([c["evaluated"], c["tested"], c["full_passes"], c["partial_passes"]])
    out = dict(fx=np.array(fx), fy=np.array(fy), states=np.array(st), counts=np.array(counts, dtype=np.int64),
               near_dropped=e.near_dropped(), status_ok=bool((e.status() == 0).all()), far_radius=e.far_radius())
    e.close()
    return out
