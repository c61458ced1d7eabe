"""The definitions of include/csf.h's flow in NumPy fp64, operation for operation: the reference of
tests/test_flow_host.py and tests/test_gpu_flow.py.  It is applied to the states read back with Engine.recorded, so engine and
reference start from identical bits; every term is at most two products and one sum or difference (NumPy forms each in a pass of its
own: nothing is contracted), sqrt and the divisions are correctly rounded, and no transcendental is involved."""
import numpy as np

from passing_common import placed  # noqa: F401  (the populations and paths of the tests)
from pet_common import line, scatter, states, with_queue  # noqa: F401

EVENT_DTYPE = np.dtype([("i", np.int32), ("l", np.int32), ("k", np.int32), ("dir", np.int32),
                        ("t", np.float64), ("u", np.float64), ("speed", np.float64)])

ARRAYS = ("line_count", "cross_n", "first_t", "first_u", "first_speed", "first_dir", "occupancy", "in_samples", "in_first", "in_last",
          "in_dist", "grid_count")


class Result:
    """the arrays of csf_flow_out (grid_count None without a grid), n_outside, n_exist (the samples that exist), crossings: every
    crossing (i, l, k, dir, t, u, speed) in the order (k, i, l), and sign_changes [L] / refused [L]: the sign changes met at every
    line and those of them the extent test (u >= 0 && u <= 1) refused"""


def reference(S, lines=None, areas=None, grid=None, limit=None):
    """the whole definition on states S [c, n, >= 2] (columns 0 and 1 are read); lines [L, 4], areas [R, 5], grid (x0, y0, h, nx, ny) or
    None; limit: only the first `limit` road users are formed - for timing a stated fraction of a large recording"""
    S = np.asarray(S, dtype=float)
    if limit is not None:
        S = S[:, :int(limit)]
    c, n = S.shape[:2]
    lines = np.zeros((0, 4)) if lines is None else np.asarray(lines, dtype=float).reshape(-1, 4)
    areas = np.zeros((0, 5)) if areas is None else np.asarray(areas, dtype=float).reshape(-1, 5)
    L, R, m = len(lines), len(areas), max(c - 1, 0)
    r = Result()
    r.line_count, r.cross_n = np.zeros((m, L, 2), np.int32), np.zeros((n, L, 2), np.int32)
    r.first_t, r.first_u, r.first_speed = np.full((n, L), np.inf), np.full((n, L), np.nan), np.full((n, L), np.nan)
    r.first_dir = np.zeros((n, L), np.int32)
    r.occupancy, r.in_samples = np.zeros((c, R), np.int32), np.zeros((n, R), np.int32)
    r.in_first, r.in_last, r.in_dist = np.full((n, R), -1, np.int32), np.full((n, R), -1, np.int32), np.zeros((n, R))
    r.grid_count, r.n_outside = None, 0
    r.sign_changes, r.refused = np.zeros(L, np.int64), np.zeros(L, np.int64)
    P = S[:, :, :2]
    X, Y = P[..., 0], P[..., 1]
    here = np.isfinite(X) & np.isfinite(Y)                       # [c, n]
    r.n_exist = int(here.sum())
    station = here[:-1] & here[1:] if c > 0 else np.zeros((0, n), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        hx, hy = X[1:] - X[:-1], Y[1:] - Y[:-1]
        hxx, hyy = hx * hx, hy * hy
        ln = np.sqrt(hxx + hyy)                                  # [m, n]
    found = []
    for l, (ax, ay, bx, by) in enumerate(lines):
        dx, dy = bx - ax, by - ay
        dxx, dyy = dx * dx, dy * dy
        dd = dxx + dyy
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            p, q = dx * (Y - ay), dy * (X - ax)
            s = p - q                                            # [c, n]
            s0, s1 = s[:-1], s[1:]
            change = station & ((s0 > 0) != (s1 > 0))
            t = s0 / (s0 - s1)
            tx, ty = t * hx, t * hy
            cx, cy = X[:-1] + tx, Y[:-1] + ty
            e, f = (cx - ax) * dx, (cy - ay) * dy
            u = (e + f) / dd
            hit = change & (u >= 0) & (u <= 1)
        r.sign_changes[l], r.refused[l] = int(change.sum()), int((change & ~hit).sum())
        k, i = np.nonzero(hit)
        ev = np.zeros(k.size, EVENT_DTYPE)
        ev["i"], ev["l"], ev["k"] = i, l, k
        ev["dir"] = np.where(s0[k, i] > 0, 1, -1)
        ev["t"], ev["u"], ev["speed"] = k.astype(float) + t[k, i], u[k, i], ln[k, i]
        found.append(ev)
    E = np.concatenate(found) if found else np.zeros(0, EVENT_DTYPE)
    r.crossings = E = E[np.lexsort((E["l"], E["i"], E["k"]))]
    for e in E:                                                  # in the order of k: the first crossing is the lowest k
        i, l, k, col = int(e["i"]), int(e["l"]), int(e["k"]), 0 if e["dir"] > 0 else 1
        r.line_count[k, l, col] += 1
        r.cross_n[i, l, col] += 1
        if r.first_dir[i, l] == 0:
            r.first_t[i, l], r.first_u[i, l], r.first_speed[i, l], r.first_dir[i, l] = e["t"], e["u"], e["speed"], e["dir"]
    for a, (ax, ay, bx, by, hw) in enumerate(areas):
        dx, dy = bx - ax, by - ay
        dxx, dyy = dx * dx, dy * dy
        dd = dxx + dyy
        wide = hw * np.sqrt(dd)
        with np.errstate(invalid="ignore", over="ignore"):
            wx, wy = X - ax, Y - ay
            g1, g2 = wx * dx, wy * dy
            g = g1 + g2
            c1, c2 = dx * wy, dy * wx
            cr = c1 - c2
            inside = here & (g >= 0) & (g <= dd) & (np.abs(cr) <= wide)      # [c, n]
        r.occupancy[:, a] = inside.sum(axis=1)
        r.in_samples[:, a] = inside.sum(axis=0)
        for i in range(n):
            ks = np.nonzero(inside[:, i])[0]
            if ks.size:
                r.in_first[i, a], r.in_last[i, a] = ks[0], ks[-1]
        dist = np.zeros(n)                                        # from +0.0, k = 0 ... c-2 in this order
        for k in range(m):
            add = inside[k] & station[k]
            dist = np.where(add, dist + np.where(add, ln[k], 0.0), dist)
        r.in_dist[:, a] = dist
    if grid is not None:
        x0, y0, h, nx, ny = grid
        nx, ny = int(nx), int(ny)
        with np.errstate(invalid="ignore", over="ignore"):
            fx, fy = np.floor((X - x0) / h), np.floor((Y - y0) / h)
            inside = here & (fx >= 0) & (fx < nx) & (fy >= 0) & (fy < ny)    # (on the doubles, before any conversion)
        r.grid_count = np.zeros((ny, nx), np.int32)
        np.add.at(r.grid_count, (fy[inside].astype(np.int64), fx[inside].astype(np.int64)), 1)
        r.n_outside = int((here & ~inside).sum())
    return r


def events(ref):
    """every crossing, sorted by (i, l, k)"""
    E = ref.crossings
    return E[np.lexsort((E["k"], E["l"], E["i"]))]


def binned(ev, rows, L):
    """line_count [rows, L, 2] from a list of crossings"""
    out = np.zeros((rows, L, 2), np.int32)
    np.add.at(out, (ev["k"], ev["l"], np.where(ev["dir"] > 0, 0, 1)), 1)
    return out


def earliest(ev, n, L):
    """first_t, first_u, first_speed, first_dir [n, L] from a list of crossings: the lowest k of every (i, l)"""
    t, u, v, d = np.full((n, L), np.inf), np.full((n, L), np.nan), np.full((n, L), np.nan), np.zeros((n, L), np.int32)
    for e in ev[np.lexsort((ev["l"], ev["i"], ev["k"]))]:
        i, l = int(e["i"]), int(e["l"])
        if d[i, l] == 0:
            t[i, l], u[i, l], v[i, l], d[i, l] = e["t"], e["u"], e["speed"], e["dir"]
    return t, u, v, d


def layout(b):
    """the lines, areas and grid of the GPU tests, relative to the side b of the box the riders start in"""
    lines = [(b / 2, 0, b / 2, b), (b, b / 2, 0, b / 2), (0, 0, b, b), (.3 * b, .6 * b, .5 * b, .7 * b), (2 * b, 0, 2 * b, b)]
    areas = [(.25 * b, .5 * b, .75 * b, .5 * b, .15 * b), (.2 * b, .2 * b, .8 * b, .8 * b, .1 * b), (3 * b, 3 * b, 3.5 * b, 3 * b, .1 * b)]
    return np.array(lines, dtype=float), np.array(areas, dtype=float), (0.0, 0.0, b / 8, 8, 8)
