"""The definitions of include/csf.h's post-encroachment time in NumPy fp64, operation for operation: the reference of
tests/test_pet_host.py and tests/test_gpu_pet.py.  It is applied to the states read back with Engine.recorded, so engine and
reference start from identical bits; every term is two products and one subtraction (NumPy forms each in a pass of its own: nothing
is contracted), the decision comes from num and den, and the quotients are formed for the crossings alone."""
import numpy as np

EVENT_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("k", np.int32), ("l", np.int32),
                        ("t_i", np.float64), ("t_j", np.float64), ("x", np.float64), ("y", np.float64)])

BLOCK_PAIRS = 1 << 21     # own x partner segments formed at a time


class Result:
    """seg_pet, seg_with, seg_t_own, seg_t_with [m, n]; run_pet, run_with, run_t_own, run_t_with, run_x, run_y, run_count [n];
    crossings: every crossing (i, j, k, l, t_i, t_j, x, y) as i reports it, for ALL ordered (i, j), in the order (k, i, j, l)"""


def _inside(num, den):
    return np.where(den > 0, (0 <= num) & (num < den), np.where(den < 0, (den < num) & (num <= 0), False))


def reference(S, limit=None):
    """the whole definition on states S [c, n, >= 2] (rows 0 and 1 are read); limit: only the first `limit` own segments (k, i) are
    formed - for timing a stated fraction of a large recording, the rows of the others stay as without a crossing"""
    S = np.asarray(S, dtype=float)
    c, n = S.shape[:2]
    m = max(c - 1, 0)
    r = Result()
    r.seg_pet, r.seg_with = np.full((m, n), np.inf), np.full((m, n), -1, np.int32)
    r.seg_t_own, r.seg_t_with = np.full((m, n), np.nan), np.full((m, n), np.nan)
    r.run_pet, r.run_with = np.full(n, np.inf), np.full(n, -1, np.int32)
    r.run_t_own, r.run_t_with, r.run_x, r.run_y = (np.full(n, np.nan) for _ in range(4))
    r.run_count = np.zeros(n, np.int32)
    r.crossings = np.zeros(0, EVENT_DTYPE)
    if m == 0 or n == 0:
        return r
    A, B = S[:-1, :, :2], S[1:, :, :2]                           # [m, n, 2]
    exists = np.isfinite(A).all(axis=2) & np.isfinite(B).all(axis=2)
    r.seg_pet[~exists] = np.nan
    with np.errstate(invalid="ignore", over="ignore"):
        R = B - A
        lo, hi = np.minimum(A, B), np.maximum(A, B)
    # own segments in the order (k, i), partners in the order (j, l)
    own = lambda a: a.reshape(m * n, *a.shape[2:])               # noqa: E731
    par = lambda a: np.swapaxes(a, 0, 1).reshape(m * n, *a.shape[2:])   # noqa: E731
    ok_o, A_o, R_o, lo_o, hi_o = own(exists), own(A), own(R), own(lo), own(hi)
    ok_p, C_p, s_p, lo_p, hi_p = par(exists), par(A), par(R), par(lo), par(hi)
    k_o, i_o = np.divmod(np.arange(m * n), n)
    j_p, l_p = np.divmod(np.arange(m * n), m)
    found = []
    step = max(1, BLOCK_PAIRS // (m * n))
    stop = m * n if limit is None else min(m * n, int(limit))
    for b0 in range(0, stop, step):
        o = slice(b0, min(stop, b0 + step))
        with np.errstate(invalid="ignore", over="ignore"):
            box = ((lo_o[o, None, 0] <= hi_p[None, :, 0]) & (hi_o[o, None, 0] >= lo_p[None, :, 0])
                   & (lo_o[o, None, 1] <= hi_p[None, :, 1]) & (hi_o[o, None, 1] >= lo_p[None, :, 1]))
            wx, wy = C_p[None, :, 0] - A_o[o, None, 0], C_p[None, :, 1] - A_o[o, None, 1]
            rx, ry, sx, sy = R_o[o, None, 0], R_o[o, None, 1], s_p[None, :, 0], s_p[None, :, 1]
            den = rx * sy - ry * sx
            ns = wx * sy - wy * sx
            nt = wx * ry - wy * rx
            cross = ok_o[o, None] & ok_p[None, :] & (i_o[o, None] != j_p[None, :]) & box & _inside(ns, den) & _inside(nt, den)
        a, p = np.nonzero(cross)                                 # row-major: per own segment the partners in (j, l) order
        if a.size == 0:
            continue
        d, u, w = den[a, p], ns[a, p], nt[a, p]
        a = a + b0
        s_own, s_with = u / d, w / d
        ev = np.zeros(a.size, EVENT_DTYPE)
        ev["i"], ev["j"], ev["k"], ev["l"] = i_o[a], j_p[p], k_o[a], l_p[p]
        ev["t_i"], ev["t_j"] = k_o[a].astype(float) + s_own, l_p[p].astype(float) + s_with
        ev["x"], ev["y"] = A_o[a, 0] + s_own * R_o[a, 0], A_o[a, 1] + s_own * R_o[a, 1]
        found.append(ev)
    if not found:
        return r
    X = r.crossings = np.concatenate(found)
    pet = np.abs(X["t_j"] - X["t_i"])
    px, py = np.full((m, n), np.nan), np.full((m, n), np.nan)     # the point of the crossing that gave the segment its minimum
    for e, d in zip(X, pet):                                     # strict `<` in the order (j, l): the first of a tie stays
        k, i = int(e["k"]), int(e["i"])
        r.run_count[i] += 1
        if d < r.seg_pet[k, i]:
            r.seg_pet[k, i], r.seg_with[k, i], r.seg_t_own[k, i], r.seg_t_with[k, i] = d, e["j"], e["t_i"], e["t_j"]
            px[k, i], py[k, i] = e["x"], e["y"]
    # the road user's minimum: the earliest k on ties
    r.run_pet, r.run_with, r.run_t_own, r.run_t_with, kk = window(r.seg_pet, r.seg_with, r.seg_t_own, r.seg_t_with)
    hit = kk >= 0
    r.run_x[hit], r.run_y[hit] = px[kk[hit], np.nonzero(hit)[0]], py[kk[hit], np.nonzero(hit)[0]]
    return r


def window(seg_pet, seg_with, seg_t_own, seg_t_with):
    """(run_pet, run_with, run_t_own, run_t_with, the k of each or -1): the minimum over k with a strict `<`, the earliest k on ties;
    NaN rows are never `<`"""
    m, n = seg_pet.shape
    bp, bw, bo, bt, bk = np.full(n, np.inf), np.full(n, -1, np.int32), np.full(n, np.nan), np.full(n, np.nan), np.full(n, -1)
    for k in range(m):
        with np.errstate(invalid="ignore"):
            less = seg_pet[k] < bp
        bp, bw = np.where(less, seg_pet[k], bp), np.where(less, seg_with[k], bw).astype(np.int32)
        bo, bt, bk = np.where(less, seg_t_own[k], bo), np.where(less, seg_t_with[k], bt), np.where(less, k, bk)
    return bp, bw, bo, bt, bk


def events(r, pet_event):
    """the crossings with i < j and pet < pet_event, sorted by (i, j, k, l)"""
    X = r.crossings
    with np.errstate(invalid="ignore"):
        keep = (X["i"] < X["j"]) & (np.abs(X["t_j"] - X["t_i"]) < pet_event)
    X = X[keep]
    return X[np.lexsort((X["l"], X["k"], X["j"], X["i"]))]


def pet_matrix(S):
    """the smallest pet of every ordered pair of road users [n, n] (+inf: their paths do not cross): the symmetry check"""
    r = reference(S)
    n = np.asarray(S).shape[1]
    M = np.full((n, n), np.inf)
    X = r.crossings
    np.minimum.at(M, (X["i"], X["j"]), np.abs(X["t_j"] - X["t_i"]))
    return M


# ---- paths given by hand -------------------------------------------------------------------------------------------------------------
def states(*paths):
    """states [c, n, 5] of road users whose positions are given sample by sample (psi, v and the rest are 0: they are not read)"""
    P = np.array(paths, dtype=float)                             # [n, c, 2]
    S = np.zeros((P.shape[1], P.shape[0], 5))
    S[:, :, :2] = np.swapaxes(P, 0, 1)
    return S


def line(start, step, c=8):
    """c samples from `start` on, `step` metres per sample"""
    return [(start[0] + k * step[0], start[1] + k * step[1]) for k in range(c)]


I_PATH = line((0.0, 0.0), (5.0, 0.0))                            # i: from (0, 0) at +5 m per sample along x
PERPENDICULAR = states(I_PATH, line((12.0, 20.0), (0.0, -4.0)))  # j comes down x = 12: at y = 0 in sample 5 exactly, i at x = 12 at 2.4
SHARED_VERTEX = states(I_PATH, line((10.0, 8.0), (0.0, -4.0)))   # j is at (10, 0) exactly in sample 2, as i is
NO_CROSSING = {
    "parallel offset paths": states(I_PATH, line((0.0, 3.0), (5.0, 0.0))),
    "collinear following": states(I_PATH, line((-7.0, 0.0), (4.0, 0.0))),
    "a stationary road user on the other's path": states(I_PATH, line((12.0, 0.0), (0.0, 0.0))),
    "a path that ends 1 m short": states(I_PATH, line((12.0, 29.0), (0.0, -4.0))),      # j ends at (12, 1)
}
# j weaves across y = 0 twice: segment 0 from (7, 4) to (8, -4) at x = 7.5 (t_j = 0.5; i is there at 1.5: PET 1.0), segment 2 from
# (18, -4) to (19, 4) at x = 18.5 (t_j = 2.5; i at 3.7: PET 1.2)
WEAVE = states(I_PATH, [(7.0, 4.0), (8.0, -4.0), (18.0, -4.0), (19.0, 4.0), (20.0, 8.0), (21.0, 12.0), (22.0, 16.0), (23.0, 20.0)])


# ---- populations of the GPU tests ----------------------------------------------------------------------------------------------------
def scatter(n, box, seed, ns=5):
    """n road users at random in a box, headings in (-pi, pi], speeds 3 ... 6 (test_gpu_encounters.crowd's)"""
    rng = np.random.default_rng(seed)
    s0 = np.zeros((n, ns))
    s0[:, 0], s0[:, 1] = rng.uniform(0, box, n), rng.uniform(0, box, n)
    s0[:, 2] = -rng.uniform(-np.pi, np.pi, n)                    # (-pi, pi]
    s0[:, 3] = rng.uniform(3, 6, n)
    return s0


def converging(n, ns=5):
    """two or three riders whose paths cross within their first second: 0 rides east along y = 0, 1 north across it, 2 south"""
    s0 = np.zeros((n, ns))
    rows = [(-3.0, 0.0, 0.0, 5.0), (1.5, -2.0, np.pi / 2, 5.0), (-1.5, 3.0, -np.pi / 2, 5.0)]
    s0[:, :4] = rows[:n]
    return s0


def with_queue(s0):
    """destinations 50, 99 and 100 m ahead of every road user: (offsets, rows) for Engine.set_dest_queue"""
    n = s0.shape[0]
    d = np.array([50.0, 99.0, 100.0])
    dq = np.zeros((n, 4, 3))
    dq[:, 0, 0], dq[:, 0, 1] = s0[:, 0], s0[:, 1]
    dq[:, 1:, 0] = s0[:, 0, None] + d[None, :] * np.cos(s0[:, 2])[:, None]
    dq[:, 1:, 1] = s0[:, 1, None] + d[None, :] * np.sin(s0[:, 2])[:, None]
    return np.arange(n + 1) * 4, dq.reshape(-1, 3)
