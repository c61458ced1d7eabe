"""The definitions of include/csf.h's encounter measures in NumPy fp64: the reference of tests/test_encounter_host.py
and tests/test_gpu_encounters.py.  It is applied to the states read back with Engine.recorded / Engine.state, so engine and reference
start from identical bits."""
import numpy as np

EVENT_DTYPE = np.dtype([("sample", np.int64), ("i", np.int32), ("j", np.int32), ("d", np.float64), ("ttc", np.float64)])


class Pairs:
    """every pair of every sample: D, T [count, n, n] (row = receiver i, column = partner j; +inf where the pair does not exist),
    the terms a, b, q, disc and which pairs exist (ok)"""


def pairs(S, radius):
    S = np.asarray(S, dtype=float)
    x, y, psi, v = S[..., 0], S[..., 1], S[..., 2], S[..., 3]
    live = np.isfinite(x) & np.isfinite(y) & np.isfinite(psi) & np.isfinite(v)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ux, uy = v * np.cos(psi), v * np.sin(psi)
        wx, wy = x[:, None, :] - x[:, :, None], y[:, None, :] - y[:, :, None]
        cx, cy = ux[:, None, :] - ux[:, :, None], uy[:, None, :] - uy[:, :, None]
        R = 2.0 * radius
        ww, a, b = wx * wx + wy * wy, cx * cx + cy * cy, wx * cx + wy * cy
        q = ww - R * R
        disc = b * b - a * q
        root = q / (-b + np.sqrt(np.where(disc >= 0, disc, 0.0)))
        T = np.where(q <= 0, 0.0, np.where((b >= 0) | (a == 0) | (disc < 0), np.inf, root))
        D = np.sqrt(ww)
    n = S.shape[1]
    p = Pairs()
    p.live = live
    p.ok = live[:, :, None] & live[:, None, :] & ~np.eye(n, dtype=bool)[None]
    p.D, p.T = np.where(p.ok, D, np.inf), np.where(p.ok, T, np.inf)
    p.a, p.b, p.q, p.disc, p.R = a, b, q, disc, R
    return p


def per_sample(S, radius, p=None):
    """d_min, d_with, ttc_min, ttc_with [count, n]: the lowest j on ties (argmin takes the first), -1 where the minimum is +inf, NaN / -1
    in the row of a road user that is not finite"""
    p = p or pairs(S, radius)
    count, n = p.live.shape
    if n == 0:
        z = np.zeros((count, 0))
        return z, z.astype(np.int32), z.copy(), z.astype(np.int32)
    d, t = p.D.min(axis=2), p.T.min(axis=2)
    dj = np.where(np.isinf(d), -1, p.D.argmin(axis=2)).astype(np.int32)
    tj = np.where(np.isinf(t), -1, p.T.argmin(axis=2)).astype(np.int32)
    d, t = np.where(p.live, d, np.nan), np.where(p.live, t, np.nan)
    dj, tj = np.where(p.live, dj, -1).astype(np.int32), np.where(p.live, tj, -1).astype(np.int32)
    return d, dj, t, tj


def fragile(S, radius, p=None):
    """the (sample, rider) cells the issue leaves out of the comparison: a pair of the cell within 1e-9 b^2 of the discriminant's zero
    while approaching, or within 1e-6 R^2 of touching, or the cell's two smallest values within 1e-9 relative without being equal"""
    p = p or pairs(S, radius)
    with np.errstate(invalid="ignore"):
        near = p.ok & (((p.b < 0) & (np.abs(p.disc) < 1e-9 * p.b * p.b)) | (np.abs(p.q) < 1e-6 * p.R * p.R))
    out = near.any(axis=2)
    for M in (p.D, p.T):
        if M.shape[2] >= 2:
            two = np.sort(M, axis=2)[:, :, :2]
            lo, hi = two[..., 0], two[..., 1]
            with np.errstate(invalid="ignore"):
                out |= np.isfinite(hi) & (hi != lo) & (hi - lo < 1e-9 * np.abs(hi))
    return out


def window(d, dj, t, tj, first):
    """the window's minima of per-sample arrays: (run_d_min, run_d_with, run_d_sample, run_ttc_min, run_ttc_with, run_ttc_sample),
    the earliest sample on ties, absolute sample indices, +inf / -1 / -1 where nothing was ever finite and below +inf"""
    count, n = d.shape
    out = []
    for v, w in ((d, dj), (t, tj)):
        bv, bw, bs = np.full(n, np.inf), np.full(n, -1, np.int32), np.full(n, -1, np.int64)
        for k in range(count):
            with np.errstate(invalid="ignore"):
                less = v[k] < bv
            bv, bw, bs = np.where(less, v[k], bv), np.where(less, w[k], bw).astype(np.int32), np.where(less, first + k if first >= 0 else -1, bs)
        out += [bv, bw, bs]
    return tuple(out)


def events(S, radius, d_event, ttc_event, first, p=None):
    """(the events sorted by (sample, i, j), the pairs within 1e-9 relative of a threshold as a set of (sample, i, j))"""
    p = p or pairs(S, radius)
    count, n = p.live.shape
    upper = np.triu(np.ones((n, n), dtype=bool), 1)[None] & p.ok
    hit = np.zeros_like(upper)
    edge = np.zeros_like(upper)
    if d_event is not None and d_event > 0:
        hit |= p.D < d_event
        edge |= np.abs(p.D - d_event) < 1e-9 * d_event
    if ttc_event is not None and ttc_event > 0:
        hit |= p.T < ttc_event
        with np.errstate(invalid="ignore"):
            edge |= np.abs(p.T - ttc_event) < 1e-9 * ttc_event
    k, i, j = np.nonzero(hit & upper)
    ev = np.zeros(k.size, EVENT_DTYPE)
    ev["sample"], ev["i"], ev["j"], ev["d"], ev["ttc"] = (first + k if first >= 0 else -1), i, j, p.D[k, i, j], p.T[k, i, j]
    ke, ie, je = np.nonzero(edge & upper)
    return ev, {(int(first + a) if first >= 0 else -1, int(b), int(c)) for a, b, c in zip(ke, ie, je)}


def scatter(n, box, seed, ns=5):
    """n road users at random in a box, headings in (-pi, pi], speeds 3 ... 6"""
    rng = np.random.default_rng(seed)
    s0 = np.zeros((n, ns))
    s0[:, 0], s0[:, 1] = rng.uniform(0, box, n), rng.uniform(0, box, n)
    s0[:, 2] = -rng.uniform(-np.pi, np.pi, n)                    # (-pi, pi]
    s0[:, 3] = rng.uniform(3, 6, n)
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


# the hand-computed cases of the issue: (name, state of i, state of j, radius, d, ttc)
KNOWN = [
    # closing speed 10 m/s over 21 - 1 = 20 m of free distance
    ("head-on", (0.0, 0.0, 0.0, 5.0), (21.0, 0.0, np.pi, 5.0), 0.5, 21.0, 2.0),
    ("parallel", (0.0, 0.0, 0.0, 5.0), (0.0, 3.0, 0.0, 5.0), 0.5, 3.0, np.inf),
    ("overlapping", (0.0, 0.0, 0.0, 5.0), (0.6, 0.0, np.pi, 5.0), 0.5, 0.6, 0.0),
    ("diverging", (0.0, 0.0, np.pi, 5.0), (10.0, 0.0, 0.0, 5.0), 0.5, 10.0, np.inf),
    # i rides along y = 0, j comes down x = 30 from y = 32.5: at t = 6 i is at (30, 0) and j at (30, 2.5) - and the distance never
    # falls below 2.5 / sqrt(2) = 1.77 m > R = 1
    ("a pass that misses", (0.0, 0.0, 0.0, 5.0), (30.0, 32.5, -np.pi / 2, 5.0), 0.5, np.hypot(30.0, 32.5), np.inf),
    # the same crossing timed to meet: j from y = 30 reaches (30, 0) with i; relative speed 5 sqrt(2) along the line of centres
    ("crossing that meets", (0.0, 0.0, 0.0, 5.0), (30.0, 30.0, -np.pi / 2, 5.0), 0.5, 30.0 * np.sqrt(2.0),
     (30.0 * np.sqrt(2.0) - 1.0) / (5.0 * np.sqrt(2.0))),
]
