"""The definitions of include/csf.h's following and passing in NumPy fp64, operation for operation: the reference of
tests/test_passing_host.py and tests/test_gpu_passing.py.  It is applied to the states read back with Engine.recorded, so engine and
reference start from identical bits; every term is two products and one sum or difference (NumPy forms each in a pass of its own:
nothing is contracted), sqrt and the divisions are correctly rounded, and no transcendental is involved.

`made` comes from the definition; `by_*` is derived by TRANSPOSING the made passings - the device's own evaluation of "j passes i"
in the lane of i is so checked against an independent route."""
import numpy as np

from pet_common import line, scatter, states, with_queue  # noqa: F401  (the paths and populations of the tests)

EVENT_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("k", np.int32), ("kind", np.int32),
                        ("t", np.float64), ("lat", np.float64), ("closing", np.float64), ("cosine", np.float64)])

STATION = ("gap", "gap_with", "thw")
INTERVAL = ("made_lat", "made_with", "made_t", "made_kind", "by_lat", "by_with", "by_t", "by_kind")
RUN = ("run_gap", "run_gap_with", "run_gap_k", "run_thw", "run_thw_with", "run_thw_k", "run_made_lat", "run_made_with", "run_made_t",
       "run_made_kind", "run_by_lat", "run_by_with", "run_by_t", "run_by_kind", "run_made", "run_by")


class Result:
    """gap, gap_with, thw [c-1, n]; made_*, by_* [c-2, n]; run_* [n], run_made, run_by [n, 3]; passings: every ordered passing
    (i, j, k, kind, t, lat, closing, cosine) as the passer i reports it, in the order (k, i, j)"""


def _terms(P, H, k, rows):
    """w, g, cr, dot of every ordered pair (i in rows, j) at station k: [len(rows), n] each"""
    wx, wy = P[k, None, :, 0] - P[k, rows, None, 0], P[k, None, :, 1] - P[k, rows, None, 1]     # always P_j - P_i
    hx, hy = H[k, rows, None, 0], H[k, rows, None, 1]
    g = wx * hx + wy * hy
    cr = hx * wy - hy * wx
    dot = hx * H[k, None, :, 0] + hy * H[k, None, :, 1]
    return g, cr, dot


def _first_min(value, where):
    """per row the column of the smallest value among `where`, the lowest column on ties (a strict `<` in column order), and whether
    there is one below +inf"""
    v = np.where(where, value, np.inf)
    j = np.argmin(v, axis=1)                                     # (the first occurrence of the minimum)
    return j, v[np.arange(v.shape[0]), j] < np.inf


def _kind_index(kind):
    return np.where(kind > 0, 0, np.where(kind < 0, 1, 2))


def reference(S, band=0.75, lat_max=3.0, limit=None):
    """the whole definition on states S [c, n, >= 2] (rows 0 and 1 are read); limit: only the first `limit` road users are formed as
    followers and passers - for timing a stated fraction of a large recording, the rows of the others stay as without a partner"""
    S = np.asarray(S, dtype=float)
    c, n = S.shape[:2]
    m, iv = max(c - 1, 0), max(c - 2, 0)
    r = Result()
    r.gap, r.gap_with, r.thw = np.full((m, n), np.inf), np.full((m, n), -1, np.int32), np.full((m, n), np.inf)
    for f in ("made", "by"):
        setattr(r, f + "_lat", np.full((iv, n), np.inf)), setattr(r, f + "_with", np.full((iv, n), -1, np.int32))
        setattr(r, f + "_t", np.full((iv, n), np.nan)), setattr(r, f + "_kind", np.zeros((iv, n), np.int32))
        setattr(r, "run_" + f, np.zeros((n, 3), np.int32))
    r.passings = np.zeros(0, EVENT_DTYPE)
    found = []
    if m > 0 and n > 0:
        P = S[:, :, :2]
        fin = np.isfinite(P).all(axis=2)
        exists = fin[:-1] & fin[1:]                               # [m, n]
        with np.errstate(invalid="ignore", over="ignore"):
            H = P[1:] - P[:-1]
            hh = H[..., 0] * H[..., 0] + H[..., 1] * H[..., 1]
            ln = np.sqrt(hh)
            moves = exists & (hh > 0)
        r.gap[~exists] = r.thw[~exists] = np.nan
        r.made_lat[~exists[:iv]] = np.nan
        rows = np.arange(n if limit is None else min(n, int(limit)))
        other = rows[:, None] != np.arange(n)[None, :]
        for k in range(m):
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                g0, cr0, dot0 = _terms(P, H, k, rows)
                len0 = ln[k, rows, None]
                lat0 = cr0 / len0
                ok = moves[k, rows, None] & exists[k][None, :] & other
                cand = ok & (g0 > 0) & (np.abs(lat0) <= band) & (dot0 >= 0)
                j, has = _first_min(g0, cand)
                i = rows[has]
                gap = g0[has, j[has]] / ln[k, i]
                r.gap[k, i], r.gap_with[k, i], r.thw[k, i] = gap, j[has], gap / ln[k, i]
                if k >= iv:
                    continue
                g1, cr1, _ = _terms(P, H, k + 1, rows)
                len1 = ln[k + 1, rows, None]
                a0, a1, lat1 = g0 / len0, g1 / len1, cr1 / len1
                closing = a0 - a1
                s = a0 / closing
                lat = lat0 + s * (lat1 - lat0)
                hit = ok & moves[k + 1, rows, None] & exists[k + 1][None, :] & (g0 > 0) & (g1 <= 0) & (np.abs(lat) <= lat_max)
                a, p = np.nonzero(hit)                           # row-major: per passer the passed in population order
                if a.size == 0:
                    continue
                ev = np.zeros(a.size, EVENT_DTYPE)
                ev["i"], ev["j"], ev["k"] = rows[a], p, k
                ev["kind"] = np.sign(dot0[a, p]).astype(np.int32)
                ev["t"], ev["lat"], ev["closing"] = float(k) + s[a, p], lat[a, p], closing[a, p]
                ev["cosine"] = dot0[a, p] / (ln[k, rows[a]] * ln[k, p])
                found.append(ev)
    if found:
        X = r.passings = np.concatenate(found)
        for e in X:                                              # made: the order (k, i, j), a strict `<`: the lowest j of a tie stays
            k, i = int(e["k"]), int(e["i"])
            r.run_made[i, _kind_index(e["kind"])] += 1
            if abs(e["lat"]) < abs(r.made_lat[k, i]):
                r.made_lat[k, i], r.made_with[k, i], r.made_t[k, i], r.made_kind[k, i] = e["lat"], e["j"], e["t"], e["kind"]
        for e in X[np.lexsort((X["i"], X["j"], X["k"]))]:        # received: the transposed list in the order (k, j, i): the lowest passer stays
            k, j = int(e["k"]), int(e["j"])
            r.run_by[j, _kind_index(e["kind"])] += 1
            if abs(e["lat"]) < abs(r.by_lat[k, j]):
                r.by_lat[k, j], r.by_with[k, j], r.by_t[k, j], r.by_kind[k, j] = e["lat"], e["i"], e["t"], e["kind"]
    r.run_gap, r.run_gap_with, r.run_gap_k = window(r.gap, r.gap, r.gap_with)[:3]
    r.run_thw, r.run_thw_with, r.run_thw_k = window(r.thw, r.thw, r.gap_with)[:3]
    for f in ("made", "by"):
        lat, w, _, t, kind = window(np.abs(getattr(r, f + "_lat")), getattr(r, f + "_lat"), getattr(r, f + "_with"), getattr(r, f + "_t"),
                                    getattr(r, f + "_kind"))
        setattr(r, f"run_{f}_lat", lat), setattr(r, f"run_{f}_with", w), setattr(r, f"run_{f}_t", t), setattr(r, f"run_{f}_kind", kind)
    return r


def window(key, value, with_, t=None, kind=None):
    """(value, partner, k[, t, kind]) of the smallest key over the rows k, with a strict `<`: the earliest k on ties; NaN rows are never
    `<`.  Nothing found: +inf / -1 / -1 / NaN / 0"""
    m, n = key.shape
    bk, bv, bw, bi = np.full(n, np.inf), np.full(n, np.inf), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    bt, bkind = np.full(n, np.nan), np.zeros(n, np.int32)
    for k in range(m):
        with np.errstate(invalid="ignore"):
            less = key[k] < bk
        bk, bv, bw, bi = np.where(less, key[k], bk), np.where(less, value[k], bv), np.where(less, with_[k], bw).astype(np.int32), np.where(less, k, bi).astype(np.int32)
        if t is not None:
            bt, bkind = np.where(less, t[k], bt), np.where(less, kind[k], bkind).astype(np.int32)
    return (bv, bw, bi) if t is None else (bv, bw, bi, bt, bkind)


def events(r, lat_event):
    """the ordered passings with fabs(lat) < lat_event, sorted by (i, j, k)"""
    X = r.passings
    with np.errstate(invalid="ignore"):
        X = X[np.abs(X["lat"]) < lat_event]
    return X[np.lexsort((X["k"], X["j"], X["i"]))]


def by_from_events(ev, n, intervals):
    """by_lat, by_with, by_t, by_kind [intervals, n] from a list of ordered passings: the transposed route of the GPU invariants"""
    lat, w = np.full((intervals, n), np.inf), np.full((intervals, n), -1, np.int32)
    t, kind = np.full((intervals, n), np.nan), np.zeros((intervals, n), np.int32)
    for e in ev[np.lexsort((ev["i"], ev["j"], ev["k"]))]:
        k, j = int(e["k"]), int(e["j"])
        if abs(e["lat"]) < abs(lat[k, j]):
            lat[k, j], w[k, j], t[k, j], kind[k, j] = e["lat"], e["i"], e["t"], e["kind"]
    return lat, w, t, kind


# ---- paths given by hand (metres per sample) -------------------------------------------------------------------------------------------
C_HAND = 12
OVERTAKE = states(line((0.0, 0.0), (1.2, 0.0), C_HAND), line((3.0, 1.0), (0.8, 0.0), C_HAND))      # i gains 0.4 per sample on j, 3 ahead and 1 to its left
MEETING = states(line((0.0, 0.0), (1.0, 0.0), C_HAND), line((9.0, -1.5), (-1.0, 0.0), C_HAND))     # abeam at 4.5, j 1.5 to i's right
STATIONARY = states(line((0.0, 0.0), (1.0, 0.0), C_HAND), line((4.5, 0.5), (0.0, 0.0), C_HAND))    # i passes the standing j at 4.5
TOO_WIDE = states(line((0.0, 0.0), (1.2, 0.0), C_HAND), line((3.0, 3.5), (0.8, 0.0), C_HAND))      # the overtaking, 3.5 m to the side
ABEAM = states(line((0.0, 0.0), (1.0, 0.0), C_HAND), line((2.0, 1.0), (0.5, 0.0), C_HAND))         # i at x = 4 in sample 4, as j is: g = 0 there


# ---- starts of the GPU tests' small scenes ---------------------------------------------------------------------------------------------
def placed(n, ns=5):
    """two riders head-on, 1.5 m apart laterally; the third, slow, starts 3 m ahead of rider 0 and 1 m beside it: (x, y, psi, v) and
    the rest 0"""
    s0 = np.zeros((n, ns))
    rows = [(0.0, 0.0, 0.0, 6.0), (9.0, -1.5, np.pi, 5.0), (3.0, 1.0, 0.0, 2.5)]
    s0[:, :4] = rows[:n]
    return s0
