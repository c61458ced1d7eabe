"""Roads and members shared by tests/test_gpu_mid_road.py, tests/test_mid_road_host.py and tests/mid_road_abi_child.py.
Every edge lies at least 1 m outside the box the crowd starts in, as in the other road tests: no force is dominated by a near-singular
vertex."""
import numpy as np

from oracle import csf_oracle as orc
from test_gpu_mid import start_state
from test_gpu_small import crowd

ON_VERTEX = (12.5, -3.0)      # a vertex of every road below that fp32 holds exactly: a rider pushed there meets r = 0


def road(kind, box):
    """(offsets, vertices, F0, sigma) of a road around a crowd in [0, box]^2"""
    def line(nv, y, x0=-10.0, x1=None):
        xs = np.linspace(x0, box + 10.0 if x1 is None else x1, nv)
        return np.c_[xs, np.full(nv, y)]

    lo, hi = -3.0, box + 3.0
    if kind == "sigma2":          # one edge, sigma = 2 (NP = 3), 300 vertices: padded to 320 - a last, half-empty pass
        off, v, F0, sg = [0, 300], line(300, lo), [0.15], [2.0]
    elif kind == "two":           # two edges with the default sigma = 3 (NP = 4)
        off, v, F0, sg = [0, 400, 800], np.r_[line(400, lo), line(400, hi)], [0.15, 0.2], [3.0, 3.0]
    elif kind == "sigma2.5":      # no integer: NP = 0
        off, v, F0, sg = [0, 300], line(300, lo), [0.15], [2.5]
    elif kind == "mixed":         # two edges with different sigma: NP = 0
        off, v, F0, sg = [0, 200, 500], np.r_[line(200, lo), line(300, hi)], [0.15, 0.2], [2.0, 3.0]
    elif kind == "tiles":         # 1 100 vertices: two tiles with different origins
        off, v, F0, sg = [0, 550, 1100], np.r_[line(550, lo, -40.0, box + 40.0), line(550, hi, -40.0, box + 40.0)], [0.15, 0.2], [2.0, 2.0]
    elif kind == "cap":           # exactly 2 048 vertices
        off, v, F0, sg = [0, 1024, 2048], np.r_[line(1024, lo, -60.0, box + 60.0), line(1024, hi, -60.0, box + 60.0)], [0.15, 0.2], [3.0, 3.0]
    elif kind == "above":         # 2 049 vertices: 2 112 padded, above the cap
        off, v, F0, sg = [0, 1024, 2049], np.r_[line(1024, lo, -60.0, box + 60.0), line(1025, hi, -60.0, box + 60.0)], [0.15, 0.2], [3.0, 3.0]
    else:
        raise ValueError(kind)
    v = np.array(v)
    v[np.argmin(np.abs(v[: off[1], 0] - ON_VERTEX[0]))] = ON_VERTEX
    return np.array(off), v, np.array(F0), np.array(sg)


def box_for(n):
    return max(30.0, 3.2 * np.sqrt(n))


def member_inputs(model, n, rule, seed):
    x, y, psi, v, off, dq = crowd(n, seed=seed, box=box_for(n))
    return start_state(model, x, y, psi, v), off, dq


# ---- the oracle members: between two edges --------------------------------------------------------------------------------------------------
ORACLE_MEMBERS = [("twod", 100, 1, None, 40.0), ("invpend", 64, 0, None, 40.0), ("bicycle", 300, 1, 4.0, 60.0), ("planarpoint", 500, 1, 2.0, 70.0)]


def oracle_inputs(m):
    model, n, rule, hfov, box = m
    x, y, psi, v, off, dq = crowd(n, seed=7 * n + rule, box=box)
    over = {} if hfov is None else {"hfov": hfov}
    xs = np.linspace(-10.0, box + 10.0, 400)
    rd = (np.array([0, 400, 800]), np.r_[np.c_[xs, np.full(400, -3.0)], np.c_[xs, np.full(400, box + 3.0)]], np.array([0.15, 0.2]), np.array([3.0, 3.0]))
    return start_state(model, x, y, psi, v), off, dq, over, rd


def oracle_member(m):
    s0, off, dq, over, rd = oracle_inputs(m)
    pop = orc.Population(orc.default_params(m[0], priority_rule=m[2], **over), s0, 5.0, off, dq)
    pop.set_road(*rd)
    return pop
