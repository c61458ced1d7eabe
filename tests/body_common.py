"""The definition of include/csf.h's body encounters in NumPy fp64, operation for operation: the reference of
tests/test_body_host.py and tests/test_gpu_body.py.  It is applied to the states read back with Engine.recorded / Engine.state, so
engine and reference start from identical bits; the only source of a difference is the last bit of the device's sincos."""
import numpy as np

EVENT_DTYPE = np.dtype([("sample", np.int64), ("i", np.int32), ("j", np.int32), ("gap", np.float64), ("ttc", np.float64)])
BIKE = (1.175, 0.825, 0.225)      # a bicycle as the reference draws it: (front, rear, half_width)
WIDE = (2.3, 2.3, 0.9)


class Pairs:
    """every pair of every sample: GAP, TTC [count, n, n] (row = receiver i, column = partner j; +inf where the pair does not exist),
    which pairs exist (ok), and what the comparisons that decide them stood on: sep, T_in, T_out, never, the rate of the axis that
    gave T_in (g_in)"""


def extents(n, every=7):
    """[n, 3]: every 7th road user (0, 7, 14, ...) has WIDE, the others a bicycle's"""
    ext = np.tile(np.array(BIKE), (n, 1))
    ext[::every] = WIDE
    return ext


def pairs(S, ext, rows=None, cols=None):
    """rows, cols: slices of the receivers and of the partners (None: all) - the arrays are then [count, rows, cols]"""
    S = np.asarray(S, dtype=float)
    count, n = S.shape[:2]
    ext = np.broadcast_to(np.asarray(ext, dtype=float), (n, 3))
    x, y, psi, v = S[..., 0], S[..., 1], S[..., 2], S[..., 3]
    live = np.isfinite(x) & np.isfinite(y) & np.isfinite(psi) & np.isfinite(v)
    front, rear, hw = ext[None, :, 0], ext[None, :, 1], ext[None, :, 2]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        cs, sn = np.cos(psi), np.sin(psi)
        L, W, o = np.broadcast_to(0.5 * (front + rear), x.shape), np.broadcast_to(hw, x.shape), 0.5 * (front - rear)
        mx, my = x + o * cs, y + o * sn
        ux, uy = v * cs, v * sn
        rows, cols = rows or slice(None), cols or slice(None)
        I, J = (slice(None), rows, None), (slice(None), None, cols)                  # [k, i, 1] the receiver, [k, 1, j] the partner
        wx, wy = mx[J] - mx[I], my[J] - my[I]
        cx, cy = ux[J] - ux[I], uy[J] - uy[I]
        cr, sr = cs[I] * cs[J] + sn[I] * sn[J], cs[I] * sn[J] - sn[I] * cs[J]
        acr, asr = np.abs(cr), np.abs(sr)
        s = [wx * cs[I] + wy * sn[I], wy * cs[I] - wx * sn[I], wx * cs[J] + wy * sn[J], wy * cs[J] - wx * sn[J]]
        g = [cx * cs[I] + cy * sn[I], cy * cs[I] - cx * sn[I], cx * cs[J] + cy * sn[J], cy * cs[J] - cx * sn[J]]
        Li, Wi, Lj, Wj = L[I], W[I], L[J], W[J]
        r = [Li + (Lj * acr + Wj * asr), Wi + (Lj * asr + Wj * acr), Lj + (Li * acr + Wi * asr), Wj + (Li * asr + Wi * acr)]
        sep = np.maximum(np.maximum(np.abs(s[0]) - r[0], np.abs(s[1]) - r[1]), np.maximum(np.abs(s[2]) - r[2], np.abs(s[3]) - r[3]))
        overlap = sep <= 0.0
        # the gap: eight corners
        d2 = np.full(sep.shape, np.inf)
        for a in (1.0, -1.0):
            for b in (1.0, -1.0):
                for s0, s1, aL, bW, srr, bl, bw in ((s[0], s[1], a * Lj, b * Wj, sr, Li, Wi), (-s[2], -s[3], a * Li, b * Wi, -sr, Lj, Wj)):
                    X, Y = s0 + (aL * cr - bW * srr), s1 + (aL * srr + bW * cr)
                    dx, dy = np.maximum(np.abs(X) - bl, 0.0), np.maximum(np.abs(Y) - bw, 0.0)
                    c = dx * dx + dy * dy
                    d2 = np.where(c < d2, c, d2)
        GAP = np.where(overlap, 0.0, np.sqrt(d2))
        # the time to contact: four slabs
        never = np.zeros(sep.shape, dtype=bool)
        T_in, T_out = np.full(sep.shape, -np.inf), np.full(sep.shape, np.inf)
        g_in = np.zeros(sep.shape)
        for k in range(4):
            still = g[k] == 0.0
            never |= still & (np.abs(s[k]) > r[k])
            gk = np.where(still, 1.0, g[k])
            ta, tb = (-r[k] - s[k]) / gk, (r[k] - s[k]) / gk
            enter, leave = np.where(ta < tb, ta, tb), np.where(ta < tb, tb, ta)
            up = ~still & (enter > T_in)
            T_in, g_in = np.where(up, enter, T_in), np.where(up, g[k], g_in)
            T_out = np.where(~still & (leave < T_out), leave, T_out)
        TTC = np.where(overlap, 0.0, np.where(never | (T_in > T_out) | (T_in < 0.0), np.inf, T_in))
    p = Pairs()
    p.live = live
    p.ok = live[I] & live[J] & ~np.eye(n, dtype=bool)[None, rows, cols]
    p.GAP, p.TTC = np.where(p.ok, GAP, np.inf), np.where(p.ok, TTC, np.inf)
    p.sep, p.overlap, p.never, p.T_in, p.T_out, p.g_in = sep, overlap, never, T_in, T_out, g_in
    return p


def per_sample(S, ext, p=None):
    """gap_min, gap_with, ttc_min, ttc_with [count, n]: the lowest j on ties (argmin takes the first), -1 where the minimum is +inf,
    NaN / -1 in the row of a road user that is not finite"""
    p = p or pairs(S, ext)
    count, n = p.live.shape
    if n == 0:
        z = np.zeros((count, 0))
        return z, z.astype(np.int32), z.copy(), z.astype(np.int32)
    d, t = p.GAP.min(axis=2), p.TTC.min(axis=2)
    dj = np.where(np.isinf(d), -1, p.GAP.argmin(axis=2)).astype(np.int32)
    tj = np.where(np.isinf(t), -1, p.TTC.argmin(axis=2)).astype(np.int32)
    d, t = np.where(p.live, d, np.nan), np.where(p.live, t, np.nan)
    dj, tj = np.where(p.live, dj, -1).astype(np.int32), np.where(p.live, tj, -1).astype(np.int32)
    return d, dj, t, tj


def shaky(p):
    """the pairs whose yes/no decisions stand within the issue's margins of flipping: |sep| < 1e-6 m; or, not overlapping and with
    a course that is not ruled out by a still axis (`approaching`, taken widely: more pairs are left out, never fewer),
    |T_in - T_out| < 1e-6 (1 + |T_in|), |T_in| < 1e-6, or a finite ttc decided by an axis with |g| < 1e-2 m/s"""
    with np.errstate(invalid="ignore"):
        app = ~p.overlap & ~p.never
        bad = np.abs(p.sep) < 1e-6
        bad |= app & (np.abs(p.T_in - p.T_out) < 1e-6 * (1.0 + np.abs(p.T_in)))
        bad |= app & (np.abs(p.T_in) < 1e-6)
        bad |= app & np.isfinite(p.TTC) & (np.abs(p.g_in) < 1e-2)
    return p.ok & bad


def fragile(S, ext, p=None):
    """the (sample, rider) cells the issue leaves out of the comparison: a pair of the cell is shaky, or the cell's two smallest
    values are within 1e-9 relative without being equal"""
    p = p or pairs(S, ext)
    out = shaky(p).any(axis=2)
    for M in (p.GAP, p.TTC):
        if M.shape[2] >= 2:
            two = np.sort(M, axis=2)[:, :, :2]
            lo, hi = two[..., 0], two[..., 1]
            with np.errstate(invalid="ignore"):
                out |= np.isfinite(hi) & (hi != lo) & (hi - lo < 1e-9 * np.abs(hi))
    return out


def window(d, dj, t, tj, first):
    """the window's minima of per-sample arrays: (run_gap_min, run_gap_with, run_gap_sample, run_ttc_min, run_ttc_with,
    run_ttc_sample, overlap_n), the earliest sample on ties, absolute sample indices, +inf / -1 / -1 where nothing was below +inf"""
    count, n = d.shape
    out = []
    for v, w in ((d, dj), (t, tj)):
        bv, bw, bs = np.full(n, np.inf), np.full(n, -1, np.int32), np.full(n, -1, np.int64)
        for k in range(count):
            with np.errstate(invalid="ignore"):
                less = v[k] < bv
            bv, bw, bs = np.where(less, v[k], bv), np.where(less, w[k], bw).astype(np.int32), np.where(less, first + k if first >= 0 else -1, bs)
        out += [bv, bw, bs]
    out.append((d == 0.0).sum(axis=0).astype(np.int64))
    return tuple(out)


def events(S, ext, gap_event, ttc_event, first, p=None):
    """(the events sorted by (sample, i, j), the pairs that may fall either side of a threshold as a set of (sample, i, j): shaky
    ones, and those within 1e-9 (1 + threshold) of one)"""
    p = p or pairs(S, ext)
    count, n = p.live.shape
    upper = np.triu(np.ones((n, n), dtype=bool), 1)[None] & p.ok
    hit = np.zeros_like(upper)
    edge = shaky(p)
    if gap_event is not None and gap_event >= 0:
        hit |= p.GAP <= gap_event
        with np.errstate(invalid="ignore"):
            edge |= (p.GAP > 0.0) & (np.abs(p.GAP - gap_event) < 1e-9 * (1.0 + gap_event))
    if ttc_event is not None and ttc_event > 0:
        hit |= p.TTC < ttc_event
        with np.errstate(invalid="ignore"):
            edge |= np.abs(p.TTC - ttc_event) < 1e-9 * (1.0 + ttc_event)
    k, i, j = np.nonzero(hit & upper)
    ev = np.zeros(k.size, EVENT_DTYPE)
    ev["sample"], ev["i"], ev["j"], ev["gap"], ev["ttc"] = (first + k if first >= 0 else -1), i, j, p.GAP[k, i, j], p.TTC[k, i, j]
    ke, ie, je = np.nonzero(edge & upper)
    return ev, {(int(first + a) if first >= 0 else -1, int(b), int(c)) for a, b, c in zip(ke, ie, je)}


# the hand-computed cases of the issue: (name, state of i, state of j, extents of i, extents of j, gap (None: not stated), ttc)
KNOWN = [
    # 21 m between the points, 1.175 m of front on either side; closing at 10 m/s
    ("head-on at 21 m", (0.0, 0.0, 0.0, 5.0), (21.0, 0.0, np.pi, 5.0), BIKE, BIKE, 18.65, 1.865),
    ("side by side at 3 m", (0.0, 0.0, 0.0, 5.0), (0.0, 3.0, 0.0, 5.0), BIKE, BIKE, 2.55, np.inf),
    ("side by side at 0.4 m", (0.0, 0.0, 0.0, 5.0), (0.0, 0.4, 0.0, 5.0), BIKE, BIKE, 0.0, 0.0),
    # a cross: no corner of either is inside the other
    ("crossed on one centre", (0.0, 0.0, 0.0, 5.0), (0.0, 0.0, np.pi / 2, 5.0), (3.0, 3.0, 0.2), (3.0, 3.0, 0.2), 0.0, 0.0),
    # 10 m less the two half lengths, the widths overlap by 0.1 m; 8 m at 5 m/s
    ("towards a standing body, offset 0.9 m", (0.0, 0.0, 0.0, 5.0), (10.0, 0.9, 0.0, 0.0), (1.0, 1.0, 0.5), (1.0, 1.0, 0.5), 8.0, 1.6),
    # 1 m of free width beside it: corner to corner sqrt(8^2 + 1^2), and it rides past
    ("towards a standing body, offset 2 m", (0.0, 0.0, 0.0, 5.0), (10.0, 2.0, 0.0, 0.0), (1.0, 1.0, 0.5), (1.0, 1.0, 0.5), np.sqrt(65.0), np.inf),
    # the centres are 29.825 m apart along both of i's axes and close at 5 m/s on each; the reach is 1 + 0.225 on both: 28.6 / 5
    ("crossing that meets", (0.0, 0.0, 0.0, 5.0), (30.0, 30.0, -np.pi / 2, 5.0), BIKE, BIKE, None, 5.72),
]
