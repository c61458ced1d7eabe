"""The definitions of include/csf.h's road clearance in NumPy fp64, operation for operation: the reference of
tests/test_clearance_host.py and tests/test_gpu_clearance.py.  It is applied to the states read back with Engine.recorded, so engine
and reference start from identical bits; every term is at most two products and one sum or difference (NumPy forms each in a pass of
its own: nothing is contracted), sqrt and the divisions are correctly rounded, and no transcendental is involved."""
import numpy as np

from passing_common import placed  # noqa: F401  (the populations and paths of the tests)
from pet_common import line, scatter, states, with_queue  # noqa: F401

EVENT_DTYPE = np.dtype({"names": ["i", "k", "edge", "seg", "dir", "t", "u"], "formats": [np.int32] * 5 + [np.float64] * 2,
                        "offsets": [0, 4, 8, 12, 16, 24, 32], "itemsize": 40})

CELL = ("d", "edge", "seg", "t")
STATION = ("left", "right", "left_edge", "right_edge", "cross")
USER = ("d_min", "d_min_k", "d_min_edge", "d_min_seg", "left_min", "left_min_k", "right_min", "right_min_k", "near_samples", "near_first",
        "near_last", "cross_n")
SAMPLE = ("near_count", "cross_count")
ARRAYS = CELL + STATION + USER + SAMPLE

CHUNK = 512                       # segments a workgroup of the first launch runs against (engine.CLEARANCE_CHUNK)
BLOCK = 64                        # road users formed at a time, at most: the [c, block, S] temporaries are held to 2^21 elements


class Result:
    """the arrays of csf_clearance_out, crossings: every crossing in the order (i, k, edge, seg), and what the not-vacuous checks of
    the GPU tests read: sign_changes / refused (the sign changes met and those of them the extent test refused)"""


def segments(off, xy):
    """(ax, ay, bx, by, edge_of, seg_in) [S] of the polylines offsets [n_edges + 1] into xy [V, 2], in the order of the polylines"""
    off, xy = np.asarray(off, dtype=np.int64), np.asarray(xy, dtype=float).reshape(-1, 2)
    a = np.concatenate([np.arange(off[e], off[e + 1] - 1) for e in range(len(off) - 1)])
    edge_of = np.concatenate([np.full(off[e + 1] - off[e] - 1, e, np.int32) for e in range(len(off) - 1)])
    return xy[a, 0], xy[a, 1], xy[a + 1, 0], xy[a + 1, 1], edge_of, (a - off[edge_of]).astype(np.int32)


def _lowest(d2, names):
    """the lowest index along the last axis with the smallest value - a strict `<` from +inf, so -1 where nothing is below +inf - and
    the value; names: what to report in the index's place"""
    if d2.shape[-1] == 0:
        return np.full(d2.shape[:-1], np.inf), np.full(d2.shape[:-1], -1, np.int32)
    v = np.where(d2 != d2, np.inf, d2)                            # (a NaN fails the `<`)
    g = np.argmin(v, axis=-1)
    m = np.take_along_axis(v, g[..., None], -1)[..., 0]
    return m, np.where(m < np.inf, names[g], -1).astype(np.int32)


def reference(S, road, d_event=0.0, limit=None):
    """the whole definition on states S [c, n, >= 2] (columns 0 and 1 are read) against road = (offsets, xy); limit: only the first
    `limit` road users are formed - for timing a stated fraction of a large recording"""
    S = np.asarray(S, dtype=float)
    if limit is not None:
        S = S[:, :int(limit)]
    c, n = S.shape[:2]
    m = max(c - 1, 0)
    ax, ay, bx, by, edge_of, seg_in = segments(*road)
    G = np.arange(len(ax), dtype=np.int32)
    dx, dy = bx - ax, by - ay
    dxx, dyy = dx * dx, dy * dy
    dd = dxx + dyy
    r = Result()
    r.d, r.t = np.full((c, n), np.nan), np.full((c, n), np.nan)
    r.g = np.full((c, n), -1, np.int32)
    r.left, r.right = np.full((m, n), np.nan), np.full((m, n), np.nan)
    r.left_g, r.right_g = np.full((m, n), -1, np.int32), np.full((m, n), -1, np.int32)
    r.cross = np.zeros((m, n), np.int32)
    r.sign_changes = r.refused = 0
    found = []
    X, Y = S[:, :, 0], S[:, :, 1]
    here = np.isfinite(X) & np.isfinite(Y)                       # [c, n]
    station = here[:-1] & here[1:] if c > 0 else np.zeros((0, n), bool)
    block = max(1, min(BLOCK, (1 << 21) // max(c * len(ax), 1)))
    for i0 in range(0, n, block):
        sl = slice(i0, min(i0 + block, n))
        px, py = X[:, sl, None], Y[:, sl, None]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            rx, ry = px - ax, py - ay
            g1, g2 = rx * dx, ry * dy
            gg = g1 + g2
            t = gg / dd
            t = np.where(t > 0, t, 0.0)
            t = np.where(t > 1, 1.0, t)
            tdx, tdy = t * dx, t * dy
            qx, qy = ax + tdx, ay + tdy
            ex, ey = qx - px, qy - py
            exx, eyy = ex * ex, ey * ey
            d2 = exx + eyy                                       # [c, b, S]
            low, g = _lowest(d2, G)
            ok = here[:, sl]
            r.d[:, sl] = np.where(ok, np.sqrt(low), np.nan)
            r.g[:, sl] = np.where(ok, g, -1)
            tg = np.take_along_axis(t, np.maximum(g, 0)[..., None], -1)[..., 0]
            r.t[:, sl] = np.where(ok & (g >= 0), tg, np.nan)
            if m == 0:
                continue
            st = station[:, sl]
            wx, wy = (px[1:] - px[:-1]), (py[1:] - py[:-1])      # [m, b, 1]
            z1, z2 = wx * ey[:-1], wy * ex[:-1]
            z = z1 - z2
            for side, out, out_g in ((z > 0, r.left, r.left_g), (z < 0, r.right, r.right_g)):
                low, g = _lowest(np.where(side, d2[:-1], np.inf), G)
                out[:, sl] = np.where(st, np.sqrt(low), np.nan)
                out_g[:, sl] = np.where(st, g, -1)
            s1_, s2_ = dx * ry, dy * rx
            s = s1_ - s2_                                        # [c, b, S]
            s0, s1 = s[:-1], s[1:]
            change = st[..., None] & ((s0 > 0) != (s1 > 0))
            tt = s0 / (s0 - s1)
            ttx, tty = tt * wx, tt * wy
            cx, cy = px[:-1] + ttx, py[:-1] + tty
            e, f = (cx - ax) * dx, (cy - ay) * dy
            u = (e + f) / dd
            hit = change & (u >= 0) & (u <= 1)
        r.sign_changes += int(change.sum())
        r.refused += int((change & ~hit).sum())
        r.cross[:, sl] = hit.sum(axis=2)
        k, i, g = np.nonzero(hit)
        ev = np.zeros(k.size, EVENT_DTYPE)
        ev["i"], ev["k"], ev["edge"], ev["seg"] = i + i0, k, edge_of[g], seg_in[g]
        ev["dir"] = np.where(s0[k, i, g] > 0, 1, -1)
        ev["t"], ev["u"] = k.astype(float) + tt[k, i, g], u[k, i, g]
        found.append(ev)
    E = np.concatenate(found) if found else np.zeros(0, EVENT_DTYPE)
    r.crossings = E[np.lexsort((E["seg"], E["edge"], E["k"], E["i"]))]
    names = lambda g, table: np.where(g >= 0, table[np.maximum(g, 0)], -1).astype(np.int32) if len(table) else g   # noqa: E731
    r.edge, r.seg = names(r.g, edge_of), names(r.g, seg_in)
    r.left_edge, r.right_edge = names(r.left_g, edge_of), names(r.right_g, edge_of)
    # the walk along k: a strict `<` from +inf, so the lowest k on ties; a NaN fails it
    r.d_min, r.left_min, r.right_min = (np.full(n, np.inf) for _ in range(3))
    r.d_min_k, r.d_min_edge, r.d_min_seg, r.left_min_k, r.right_min_k, r.near_first, r.near_last = (np.full(n, -1, np.int32) for _ in range(7))
    r.near_samples = np.zeros(n, np.int32)
    with np.errstate(invalid="ignore"):
        near = r.d < d_event                                     # [c, n]
        for k in range(c):
            b = r.d[k] < r.d_min
            r.d_min = np.where(b, r.d[k], r.d_min)
            r.d_min_k, r.d_min_edge, r.d_min_seg = np.where(b, k, r.d_min_k), np.where(b, r.edge[k], r.d_min_edge), np.where(b, r.seg[k], r.d_min_seg)
            r.near_first = np.where(near[k] & (r.near_first < 0), k, r.near_first)
            r.near_last = np.where(near[k], k, r.near_last)
        for k in range(m):
            b = r.left[k] < r.left_min
            r.left_min, r.left_min_k = np.where(b, r.left[k], r.left_min), np.where(b, k, r.left_min_k)
            b = r.right[k] < r.right_min
            r.right_min, r.right_min_k = np.where(b, r.right[k], r.right_min), np.where(b, k, r.right_min_k)
    for f in ("d_min_k", "d_min_edge", "d_min_seg", "left_min_k", "right_min_k", "near_first", "near_last"):
        setattr(r, f, getattr(r, f).astype(np.int32))
    r.near_samples = near.sum(axis=0).astype(np.int32)
    r.near_count = near.sum(axis=1).astype(np.int32)
    r.cross_n = r.cross.sum(axis=0).astype(np.int32)
    r.cross_count = r.cross.sum(axis=1).astype(np.int32)
    r.n_exist = int(here.sum())
    return r


def events(ref):
    """every crossing, sorted by (i, k, edge, seg)"""
    return ref.crossings


# ---- the roads of the tests, relative to the side b of the box the riders start in ---------------------------------------------------
def polyline(a, b, segs):
    """segs segments from a to b, the vertices at equal steps: a + j * (b - a) / segs (dyadic where a, b are and segs is a power of two)"""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return a + np.arange(segs + 1)[:, None] * ((b - a) / segs)


def pack(*lines):
    """(offsets, xy) of polylines"""
    return np.r_[0, np.cumsum([len(q) for q in lines])].astype(np.int64), np.vstack(lines)


def road(b, S, shift=(0.0, 0.0)):
    """a road of S segments in all.  S >= 5: a straight two-kerb path along y = b/2 - two polylines at y = b/2 -+ b/8 from x = b/4 to
    x = 3b/4, mirrored about the midline, which the riders pass beyond the ends of, so that the clamps to 0 and 1 are met and sign
    changes beyond the extent are refused; the first takes (S - 3) // 2 segments, the second the rest -, a short polyline of two
    segments, and one segment at 3b nobody comes near.  S < 5: one polyline of S segments along the box's diagonal from (b/4, b/4) to (3b/4, 3b/4)."""
    if S < 5:
        lines = [polyline((b / 4, b / 4), (3 * b / 4, 3 * b / 4), S)]
    else:
        lo = (S - 3) // 2
        lines = [polyline((b / 4, 3 * b / 8), (3 * b / 4, 3 * b / 8), lo), polyline((b / 4, 5 * b / 8), (3 * b / 4, 5 * b / 8), S - 3 - lo),
                 np.array([(.3 * b, .6 * b), (.4 * b, .65 * b), (.5 * b, .7 * b)]), np.array([(3 * b, 3 * b), (3.5 * b, 3 * b)])]
    off, xy = pack(*lines)
    return off, xy + np.asarray(shift, dtype=float)


def mirrored(swapped=False, y=2.0, segs=640, x0=-104.0, h=0.25):
    """three chunks of segments, for a rider that runs along y = 0 from x = 0 to x = 10: two kerbs at y = -+2 with the same dyadic
    vertices x0 + j h, 640 segments each, and one segment far away.  The rider is between vertices 416 and 456, so the segment of the
    first kerb it is nearest to lies in chunk 0 (g < 512) and its mirror image (g + 640) in chunk 2 (g >= 1024): the same d2 in two
    chunks, and the lower g must be reported.  swapped: the upper kerb first."""
    lo, hi = polyline((x0, -y), (x0 + segs * h, -y), segs), polyline((x0, y), (x0 + segs * h, y), segs)
    far = np.array([(500.0, 500.0), (501.0, 500.0)])
    return pack(hi, lo, far) if swapped else pack(lo, hi, far)
