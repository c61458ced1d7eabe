"""Array-level host API of the stepping engine: a thin, typed wrapper over the C ABI (include/csf.h).

`Engine` is what `intersection.SocialForceIntersection` drives; benchmarks and parity tests use it
directly with NumPy arrays.  Every number it returns was computed by the HIP kernels.
"""
import ctypes as C
import math

import numpy as np

from . import _ffi
from ._ffi import BICYCLE, INVPEND, N_STATES, PLANARBIKE, PLANARPOINT, TWOD, UNCONTROLLED, EngineError, Params  # noqa: F401

MODEL_IDS = {"bicycle": BICYCLE, "twod": TWOD, "invpend": INVPEND, "planarpoint": PLANARPOINT, "planarbike": PLANARBIKE,
             "uncontrolled": UNCONTROLLED, "balancingrider": _ffi.BALANCINGRIDER}


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


EVENT_DTYPE = np.dtype([("sample", np.int64), ("i", np.int32), ("j", np.int32), ("d", np.float64), ("ttc", np.float64)])   # csf_encounter_event


class Encounters:
    """What Engine.encounters returns for one engine: `first` the index of the first sample covered (-1: the current state), per
    sample d_min, d_with, ttc_min, ttc_with [count, n] (None when per_sample was off), over the window run_d_min, run_d_with,
    run_d_sample, run_ttc_min, run_ttc_with, run_ttc_sample [n], and events (EVENT_DTYPE, sorted by sample, i, j; None when no
    threshold was given) with n_events their number."""

    __slots__ = ("first", "radius", "d_min", "d_with", "ttc_min", "ttc_with", "run_d_min", "run_d_with", "run_d_sample",
                 "run_ttc_min", "run_ttc_with", "run_ttc_sample", "events", "n_events",
                 "ids", "d_with_id", "ttc_with_id", "run_d_with_id", "run_ttc_with_id")   # (SocialForceIntersection.encounters fills these)


def _events_wanted(d_event, ttc_event):
    return (d_event is not None and d_event > 0) or (ttc_event is not None and ttc_event > 0)


def _encounter_args(who, first, count, radius, d_event, ttc_event):
    """the checks of Engine.encounters / batch_encounters, before any device call: (first, count) as the C ABI takes them"""
    if not np.isscalar(radius) or not np.isfinite(radius) or radius < 0:
        raise ValueError(f"{who}: radius must be a finite number >= 0 (got {radius!r})")
    for name, v in (("d_event", d_event), ("ttc_event", ttc_event)):
        if v is not None and (not np.isscalar(v) or np.isnan(v)):
            raise ValueError(f"{who}: {name} must be None or a number (got {v!r})")
    if first is None:
        if count not in (None, 1):
            raise ValueError(f"{who}: the current state (first=None) is one sample, count={count!r}")
        return -1, 1
    if count is None:
        raise ValueError(f"{who}: count is needed with first")
    if int(first) != first or int(count) != count or first < 0 or count < 0:
        raise ValueError(f"{who}: first and count must be integers >= 0 (got {first!r}, {count!r})")
    if count > 65535:
        raise ValueError(f"{who}: at most 65535 samples in one call (got {count})")
    return int(first), int(count)


def _window_args(who, first, count, what, numbers_only=False):
    """(first, count) of a measure that needs a window of the recording, checked before any device call; what: the thing a
    window has and the current state lacks ("a path is")"""
    if first is None or count is None:
        raise ValueError(f"{who}: first and count are needed - {what} a window of the recording, the current state has none")
    if isinstance(first, bool) or isinstance(count, bool) or (numbers_only and not (_is_number(first) and _is_number(count))) \
            or int(first) != first or int(count) != count or first < 0 or count < 0:
        raise ValueError(f"{who}: first and count must be integers >= 0 (got {first!r}, {count!r})")
    if count > 65535:
        raise ValueError(f"{who}: at most 65535 samples in one call (got {count})")
    return int(first), int(count)


def _starts(*sizes):
    """where every member's part starts in an array that holds all members' parts of the given sizes, and where the last ends"""
    return tuple(np.r_[0, np.cumsum(v)] for v in sizes)


class _Pack:
    """the output arrays of a call for every member, each kind ONE array that the members' arrays are views of, and the
    records of the C ABI that point into them"""

    def _records(self, record, columns, events_col, caps, event_dtype):
        """self.events for `caps` events per member, and self.outs: the records as ONE int64 table (every member of a csf_*_out
        is 8 bytes), filled column by column - a batch of 1 024 members is written in a dozen array operations instead of 12 288
        attribute stores.  columns: (column, array or None, the members' starts in it); events_col: events, event_capacity"""
        caps = np.asarray(caps, dtype=np.int64)
        self.e0, = _starts(caps)
        self.events = np.empty(int(self.e0[-1]), event_dtype)
        tab = self._tab = np.zeros((len(caps), C.sizeof(record) // 8), dtype=np.int64)
        for col, a, start in columns:
            if a is not None:
                tab[:, col] = a.ctypes.data + a.itemsize * start[:-1]
        tab[:, events_col] = np.where(caps > 0, self.events.ctypes.data + event_dtype.itemsize * self.e0[:-1], 0)
        tab[:, events_col + 1] = caps
        self.outs = (record * len(caps)).from_buffer(tab)

    def _events_of(self, i, n_events, want_events):
        """member i's events (_FlowPack and _ClearancePack slice theirs from plain Python numbers read once: _read)"""
        return self.events[int(self.e0[i]):int(self.e0[i]) + n_events] if want_events else None


class _EncounterPack(_Pack):
    """_Pack of csf_encounter_out records (shapes: (n, count) per member)"""

    def __init__(self, shapes, per_sample, caps):
        self.shapes, self.caps = shapes, caps
        self.c0, self.n0 = _starts([n * c for n, c in shapes], [n for n, _ in shapes])
        nc, nn = (int(self.c0[-1]), int(self.n0[-1]))
        self.per = None
        if per_sample:
            self.per = (np.empty(nc), np.empty(nc, np.int32), np.empty(nc), np.empty(nc, np.int32))
        # (an empty window leaves them as they are: a minimum of +inf with nobody, at no sample)
        self.run = (np.full(nn, np.inf), np.full(nn, -1, np.int32), np.full(nn, -1, np.int64),
                    np.full(nn, np.inf), np.full(nn, -1, np.int32), np.full(nn, -1, np.int64))
        columns = [(col, a, self.c0) for col, a in enumerate(self.per or ())] + [(col, a, self.n0) for col, a in enumerate(self.run, start=4)]
        self._records(_ffi.EncounterOut, columns, 10, caps, EVENT_DTYPE)

    def result(self, i, radius, want_events):
        n, count = self.shapes[i]
        o = self.outs[i]
        r = Encounters()
        r.first, r.radius, r.n_events = int(o.first_sample), float(radius), int(o.n_events)
        r.ids = r.d_with_id = r.ttc_with_id = r.run_d_with_id = r.run_ttc_with_id = None
        c, u = int(self.c0[i]), int(self.n0[i])
        if self.per is None:
            r.d_min = r.d_with = r.ttc_min = r.ttc_with = None
        else:
            r.d_min, r.d_with, r.ttc_min, r.ttc_with = (a[c:c + n * count].reshape(count, n) for a in self.per)
        (r.run_d_min, r.run_d_with, r.run_d_sample, r.run_ttc_min, r.run_ttc_with, r.run_ttc_sample) = (a[u:u + n] for a in self.run)
        r.events = self._events_of(i, r.n_events, want_events)
        return r


PET_EVENT_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("k", np.int32), ("l", np.int32),
                            ("t_i", np.float64), ("t_j", np.float64), ("x", np.float64), ("y", np.float64)])   # csf_pet_event

_PET_TIMES = ("seg_pet", "seg_t_own", "seg_t_with", "run_pet", "run_t_own", "run_t_with")


class PostEncroachment:
    """What Engine.post_encroachment returns for one engine (csf.h: csf_post_encroachment): `first` the index of the first sample
    covered, per own segment seg_pet, seg_with, seg_t_own, seg_t_with [count - 1, n] (None when per_segment was off), per road user
    run_pet, run_with, run_t_own, run_t_with, run_x, run_y, run_count [n], and events (PET_EVENT_DTYPE, sorted by i, j, k, l; None when
    no threshold was given) with n_events their number.  Times and pet are in samples from `first`; `period` is the seconds per
    sample (stride x t_s of the recording), and in_seconds() returns the same result with them scaled by it."""

    __slots__ = ("first", "period", "seconds", "seg_pet", "seg_with", "seg_t_own", "seg_t_with", "run_pet", "run_with", "run_t_own",
                 "run_t_with", "run_x", "run_y", "run_count", "events", "n_events",
                 "ids", "seg_with_id", "run_with_id", "event_i_id", "event_j_id")   # (SocialForceIntersection.post_encroachment fills these)

    def in_seconds(self):
        """a copy whose times - seg_t_*, run_t_*, the events' t_i, t_j - and pet are seconds (from the sample `first`) instead of samples"""
        if self.seconds:
            return self
        if self.period is None:
            raise ValueError("in_seconds: the period of the recording is not known (record / enable_history were not called through this Engine)")
        r = PostEncroachment()
        for f in self.__slots__:
            setattr(r, f, getattr(self, f))
        for f in _PET_TIMES:
            if getattr(self, f) is not None:
                setattr(r, f, getattr(self, f) * self.period)
        if self.events is not None:
            r.events = self.events.copy()
            r.events["t_i"] *= self.period
            r.events["t_j"] *= self.period
        r.seconds = True
        return r


def _pet_args(who, first, count, pet_event):
    """the checks of Engine.post_encroachment / batch_post_encroachment, before any device call"""
    if pet_event is not None and (isinstance(pet_event, bool) or not np.isscalar(pet_event) or not isinstance(pet_event, (int, float, np.integer, np.floating))
                                  or np.isnan(pet_event) or pet_event == -np.inf):
        raise ValueError(f"{who}: pet_event must be None or a number, +inf for every crossing (got {pet_event!r})")
    return _window_args(who, first, count, "a path is")


def _pet_capacity_guess(segs):
    """room for events in the first call: crossings are far fewer than segments in every population looked at"""
    return min(max(64, segs), 1 << 16)


class _PetPack(_Pack):
    """_Pack of csf_pet_out records (shapes: (n, count) per member)"""

    SEG = (("seg_pet", np.float64), ("seg_with", np.int32), ("seg_t_own", np.float64), ("seg_t_with", np.float64))
    RUN = (("run_pet", np.float64), ("run_with", np.int32), ("run_t_own", np.float64), ("run_t_with", np.float64),
           ("run_x", np.float64), ("run_y", np.float64), ("run_count", np.int32))

    def __init__(self, shapes, per_segment, caps):
        self.shapes = shapes
        self.c0, self.n0 = _starts([n * max(c - 1, 0) for n, c in shapes], [n for n, _ in shapes])
        nc, nn = int(self.c0[-1]), int(self.n0[-1])
        self.seg = [np.empty(nc, dt) for _, dt in self.SEG] if per_segment else None
        self.run = [np.empty(nn, dt) for _, dt in self.RUN]
        columns = [(col, a, self.c0) for col, a in enumerate(self.seg or ())] + [(col, a, self.n0) for col, a in enumerate(self.run, start=4)]
        self._records(_ffi.PetOut, columns, 11, caps, PET_EVENT_DTYPE)

    def result(self, i, want_events, period):
        n, count = self.shapes[i]
        o = self.outs[i]
        r = PostEncroachment()
        r.first, r.n_events, r.period, r.seconds = int(o.first_sample), int(o.n_events), period, False
        r.ids = r.seg_with_id = r.run_with_id = r.event_i_id = r.event_j_id = None
        c, u, rows = int(self.c0[i]), int(self.n0[i]), max(count - 1, 0)
        for k, (name, _) in enumerate(self.SEG):
            setattr(r, name, None if self.seg is None else self.seg[k][c:c + n * rows].reshape(rows, n))
        for k, (name, _) in enumerate(self.RUN):
            setattr(r, name, self.run[k][u:u + n])
        r.events = self._events_of(i, r.n_events, want_events)
        return r


PASSING_EVENT_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("k", np.int32), ("kind", np.int32),
                                ("t", np.float64), ("lat", np.float64), ("closing", np.float64), ("cosine", np.float64)])   # csf_passing_event

_PASSING_TIMES = ("thw", "made_t", "by_t", "run_thw", "run_made_t", "run_by_t")


class Passing:
    """What Engine.passing returns for one engine (csf.h: csf_passing): `first` the index of the first sample covered; per station
    gap, gap_with, thw [count - 1, n] and per interval made_lat, made_with, made_t, made_kind, by_lat, by_with, by_t, by_kind
    [count - 2, n] (None when per_station was off); per road user run_gap, run_gap_with, run_gap_k, run_thw, run_thw_with, run_thw_k,
    run_made_lat, run_made_with, run_made_t, run_made_kind, run_by_lat, run_by_with, run_by_t, run_by_kind [n] and the counts run_made,
    run_by [n, 3] (overtakings, meetings, others); events (PASSING_EVENT_DTYPE, sorted by i, j, k; None when no threshold was given)
    with n_events their number.  t and thw are in samples (t from `first`), closing in metres per sample; `period` is the seconds
    per sample (stride x t_s of the recording), and in_seconds() returns the same result with them scaled by it."""

    STATION = (("gap", np.float64), ("gap_with", np.int32), ("thw", np.float64))
    INTERVAL = (("made_lat", np.float64), ("made_with", np.int32), ("made_t", np.float64), ("made_kind", np.int32),
                ("by_lat", np.float64), ("by_with", np.int32), ("by_t", np.float64), ("by_kind", np.int32))
    RUN = (("run_gap", np.float64), ("run_gap_with", np.int32), ("run_gap_k", np.int32),
           ("run_thw", np.float64), ("run_thw_with", np.int32), ("run_thw_k", np.int32),
           ("run_made_lat", np.float64), ("run_made_with", np.int32), ("run_made_t", np.float64), ("run_made_kind", np.int32),
           ("run_by_lat", np.float64), ("run_by_with", np.int32), ("run_by_t", np.float64), ("run_by_kind", np.int32))
    COUNT = (("run_made", np.int32), ("run_by", np.int32))

    __slots__ = (("first", "period", "seconds", "events", "n_events") + tuple(f for f, _ in STATION + INTERVAL + RUN + COUNT)
                 + ("ids", "gap_with_id", "made_with_id", "by_with_id", "run_gap_with_id", "run_thw_with_id", "run_made_with_id",
                    "run_by_with_id", "event_i_id", "event_j_id"))   # (SocialForceIntersection.passing fills these)

    def in_seconds(self):
        """a copy whose times - thw, made_t, by_t, their run_* and the events' t - are seconds (t from the sample `first`) and whose
        closing speeds are metres per second"""
        if self.seconds:
            return self
        if self.period is None:
            raise ValueError("in_seconds: the period of the recording is not known (record / enable_history were not called through this Engine)")
        r = Passing()
        for f in self.__slots__:
            setattr(r, f, getattr(self, f))
        for f in _PASSING_TIMES:
            if getattr(self, f) is not None:
                setattr(r, f, getattr(self, f) * self.period)
        if self.events is not None:
            r.events = self.events.copy()
            r.events["t"] *= self.period
            r.events["closing"] /= self.period
        r.seconds = True
        return r


def _is_number(v):
    return not isinstance(v, bool) and np.isscalar(v) and isinstance(v, (int, float, np.integer, np.floating))


def _passing_args(who, first, count, band, lat_max, lat_event):
    """the checks of Engine.passing / batch_passing, before any device call"""
    if not _is_number(band) or not band >= 0:
        raise ValueError(f"{who}: band must be a number >= 0, +inf for every road user ahead (got {band!r})")
    if not _is_number(lat_max) or not lat_max > 0:
        raise ValueError(f"{who}: lat_max must be a number > 0, +inf for every passing (got {lat_max!r})")
    if lat_event is not None and (not _is_number(lat_event) or np.isnan(lat_event) or lat_event == -np.inf):
        raise ValueError(f"{who}: lat_event must be None or a number, +inf for every passing (got {lat_event!r})")
    return _window_args(who, first, count, "a direction of travel is")


def _passing_capacity_guess(cells):
    """room for events in the first call: passings are fewer than stations in every population looked at"""
    return min(max(64, cells), 1 << 16)


class _PassingPack(_Pack):
    """_Pack of csf_passing_out records (shapes: (n, count) per member)"""

    def __init__(self, shapes, per_station, caps):
        self.shapes = shapes
        self.s0, self.i0, self.n0 = _starts([n * max(c - 1, 0) for n, c in shapes], [n * max(c - 2, 0) for n, c in shapes], [n for n, _ in shapes])
        self.station = [np.empty(int(self.s0[-1]), dt) for _, dt in Passing.STATION] if per_station else None
        self.interval = [np.empty(int(self.i0[-1]), dt) for _, dt in Passing.INTERVAL] if per_station else None
        self.run = [np.empty(int(self.n0[-1]), dt) for _, dt in Passing.RUN]
        self.count = [np.empty(3 * int(self.n0[-1]), dt) for _, dt in Passing.COUNT]
        columns, col = [], 0                                     # (in header order)
        for names, arrays, start in ((Passing.STATION, self.station, self.s0), (Passing.INTERVAL, self.interval, self.i0),
                                     (Passing.RUN, self.run, self.n0), (Passing.COUNT, self.count, 3 * self.n0)):
            columns += [(col + k, a, start) for k, a in enumerate(arrays or ())]
            col += len(names)
        self._records(_ffi.PassingOut, columns, col, caps, PASSING_EVENT_DTYPE)

    def result(self, i, want_events, period):
        n, count = self.shapes[i]
        o = self.outs[i]
        r = Passing()
        for f in Passing.__slots__:
            setattr(r, f, None)
        r.first, r.n_events, r.period, r.seconds = int(o.first_sample), int(o.n_events), period, False
        s, v, u = int(self.s0[i]), int(self.i0[i]), int(self.n0[i])
        rows_s, rows_i = max(count - 1, 0), max(count - 2, 0)
        if self.station is not None:
            for k, (name, _) in enumerate(Passing.STATION):
                setattr(r, name, self.station[k][s:s + n * rows_s].reshape(rows_s, n))
            for k, (name, _) in enumerate(Passing.INTERVAL):
                setattr(r, name, self.interval[k][v:v + n * rows_i].reshape(rows_i, n))
        for k, (name, _) in enumerate(Passing.RUN):
            setattr(r, name, self.run[k][u:u + n])
        for k, (name, _) in enumerate(Passing.COUNT):
            setattr(r, name, self.count[k][3 * u:3 * (u + n)].reshape(n, 3))
        r.events = self._events_of(i, r.n_events, want_events)
        return r


FLOW_EVENT_DTYPE = np.dtype([("i", np.int32), ("l", np.int32), ("k", np.int32), ("dir", np.int32),
                             ("t", np.float64), ("u", np.float64), ("speed", np.float64)])   # csf_flow_event

FLOW_MAX = 64             # lines, and areas, of a layout
FLOW_MAX_GRID = 1 << 20   # cells of a grid


class Flow:
    """What Engine.flow returns for one engine (csf.h: csf_flow): `first` the index of the first sample covered; line_count
    [c - 1, L, 2] the crossings of every interval by direction (index 0: left to right of A -> B, 1: right to left), cross_n [n, L, 2]
    those of every road user, first_t, first_u, first_speed, first_dir [n, L] a road user's first crossing of a line (+inf / NaN / NaN /
    0 without one); occupancy [c, R] the road users inside every area at every sample, in_samples, in_first, in_last, in_dist [n, R]
    every road user's samples inside, the first and last of them (-1: never) and the metres ridden inside; grid_count [ny, nx] the
    samples in every cell (None without a grid) and n_outside those outside the grid; events (FLOW_EVENT_DTYPE, every crossing, sorted
    by i, l, k; None when they were not asked for) with n_events their number.  lines [L, 4], areas [R, 5] and grid (x0, y0, h, nx, ny
    or None) are the layout the call was made with.  t is in samples from `first`, speed in metres per sample; `period` is the
    seconds per sample of the recording (None when it is not known), and the helpers take the dt to scale by."""

    ARRAYS = (("line_count", np.int32), ("cross_n", np.int32), ("first_t", np.float64), ("first_u", np.float64),
              ("first_speed", np.float64), ("first_dir", np.int32), ("occupancy", np.int32), ("in_samples", np.int32),
              ("in_first", np.int32), ("in_last", np.int32), ("in_dist", np.float64), ("grid_count", np.int32))

    __slots__ = (("first", "period", "events", "n_events", "n_outside", "lines", "areas", "grid") + tuple(f for f, _ in ARRAYS)
                 + ("ids", "event_i_id"))                     # (SocialForceIntersection.flow fills these)

    def _events_of(self, l, who):
        if self.events is None:
            raise ValueError(f"{who}: the events were not asked for (events=True)")
        return self.events[self.events["l"] == l]

    def flow(self, l, dt):
        """crossings of line l per second over the call, by direction: [2]"""
        rows = self.line_count.shape[0]
        total = self.line_count[:, l, :].sum(axis=0).astype(np.float64)
        return total / (rows * dt) if rows else np.full(2, np.nan)

    def cumulative(self, l):
        """line_count summed along k, by direction [c - 1, 2]: with a second line's, the N-curves of a stretch"""
        return np.cumsum(self.line_count[:, l, :], axis=0, dtype=np.int64)

    def travel_time(self, l_from, l_to, dt):
        """seconds from every road user's first crossing of line l_from to its first of l_to [n]; NaN where either is missing"""
        a, b = self.first_t[:, l_from], self.first_t[:, l_to]
        both = np.isfinite(a) & np.isfinite(b)
        out = np.full(a.shape, np.nan)
        out[both] = (b[both] - a[both]) * dt
        return out

    def speeds(self, l, dt):
        """(time-mean, harmonic = space-mean) speed in m/s of the crossings of line l, from the events; NaN without a crossing"""
        v = self._events_of(l, "speeds")["speed"] / dt
        if v.size == 0:
            return float("nan"), float("nan")
        with np.errstate(divide="ignore"):
            return math.fsum(v) / v.size, v.size / math.fsum(1.0 / v)

    def headways(self, l, dt):
        """seconds between successive crossings of line l, in either direction, from the events"""
        return np.diff(np.sort(self._events_of(l, "headways")["t"])) * dt

    def _area(self, r):
        ax, ay, bx, by, hw = (float(v) for v in self.areas[r])
        return 2.0 * hw * math.sqrt((bx - ax) * (bx - ax) + (by - ay) * (by - ay))

    def density(self, r):
        """road users per square metre inside area r at every sample [c]: occupancy / (2 * half_width * ld)"""
        return self.occupancy[:, r] / self._area(r)

    def edie(self, r, dt):
        """Edie's generalised (q, k, v) of area r over the call: the metres ridden inside and the seconds spent inside, both over
        area x T with T = the call's samples x dt - q in 1/(m s), k in 1/m^2 - and their ratio, the space-mean speed in m/s (NaN when
        nobody was inside).  Summed with math.fsum."""
        dist, time = math.fsum(self.in_dist[:, r]), math.fsum(self.in_samples[:, r] * float(dt))
        over = self._area(r) * self.occupancy.shape[0] * dt
        return dist / over, time / over, (dist / time if time > 0 else float("nan"))


def _flow_layout(who, lines, areas, grid):
    """the checks of the layout of Engine.flow / batch_flow, before any device call: (lines [L, 4], areas [R, 5], grid or None)"""
    def table(v, width, what):
        if v is None:
            return np.zeros((0, width))
        a = np.array(v, dtype=np.float64, ndmin=2) if np.size(v) else np.zeros((0, width))
        if a.ndim != 2 or a.shape[1] != width:
            raise ValueError(f"{who}: {what} must be [k, {width}] (got shape {a.shape})")
        if a.shape[0] > FLOW_MAX:
            raise ValueError(f"{who}: at most {FLOW_MAX} {what} (got {a.shape[0]})")
        if not np.isfinite(a[:, :4]).all():
            raise ValueError(f"{who}: {what} with a non-finite coordinate")
        dx, dy = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
        if not (dx * dx + dy * dy > 0).all():
            raise ValueError(f"{who}: {what} of no length (A == B)")
        return np.ascontiguousarray(a)
    lines, areas = table(lines, 4, "lines"), table(areas, 5, "areas")
    hw = areas[:, 4]
    if not (np.isfinite(hw) & (hw >= 0)).all():
        raise ValueError(f"{who}: the half widths of the areas must be finite and >= 0 (got {hw.tolist()})")
    if grid is not None:
        if len(grid) != 5:
            raise ValueError(f"{who}: grid must be (x0, y0, h, nx, ny) or None (got {grid!r})")
        x0, y0, h, nx, ny = grid
        if not all(_is_number(v) for v in (x0, y0, h, nx, ny)) or int(nx) != nx or int(ny) != ny:
            raise ValueError(f"{who}: grid must be (x0, y0, h, nx, ny) with whole nx, ny (got {grid!r})")
        if not (np.isfinite(x0) and np.isfinite(y0) and np.isfinite(h) and h > 0):
            raise ValueError(f"{who}: the grid's origin must be finite and h finite and > 0 (got {grid!r})")
        if nx < 1 or ny < 1 or nx * ny > FLOW_MAX_GRID:
            raise ValueError(f"{who}: the grid must have 1 ... 2^20 cells (got {nx} x {ny})")
        grid = (float(x0), float(y0), float(h), int(nx), int(ny))
    return lines, areas, grid


def _flow_args(who, first, count):
    return _window_args(who, first, count, "an interval is", numbers_only=True)


def _flow_capacity_guess(cells, lines):
    """room for events in the first call: on straight paths a few percent of the stations cross any one line"""
    return min(max(64, cells * min(lines, 4) // 4), 1 << 16)


class _FlowPack(_Pack):
    """_Pack of csf_flow_out records (shapes: (n, count) per member), and the csf_flow_layout they share"""

    def __init__(self, shapes, lines, areas, grid, caps):
        m = len(shapes)
        L, R = lines.shape[0], areas.shape[0]
        G = grid[3] * grid[4] if grid else 0
        self.shapes, self.lines, self.areas, self.grid = shapes, lines, areas, grid
        n = np.array([n for n, _ in shapes], dtype=np.int64)
        c = np.array([c for _, c in shapes], dtype=np.int64)
        sizes = {"line_count": np.maximum(c - 1, 0) * L * 2, "cross_n": n * L * 2, "first_t": n * L, "first_u": n * L, "first_speed": n * L,
                 "first_dir": n * L, "occupancy": c * R, "in_samples": n * R, "in_first": n * R, "in_last": n * R, "in_dist": n * R,
                 "grid_count": np.full(m, G, dtype=np.int64)}
        self.start = dict(zip(sizes, _starts(*sizes.values())))
        self.arrays = {f: np.empty(int(self.start[f][-1]), dt) for f, dt in Flow.ARRAYS}
        columns = [(col, self.arrays[f], self.start[f]) for col, (f, _) in enumerate(Flow.ARRAYS)]   # (in header order)
        self._records(_ffi.FlowOut, columns, len(Flow.ARRAYS), caps, FLOW_EVENT_DTYPE)
        self._read = None                                        # what the call wrote into the records, read once (result)
        y = self.layout = _ffi.FlowLayout()
        y.lines, y.areas, y.n_lines, y.n_areas = (lines.ctypes.data if L else None), (areas.ctypes.data if R else None), L, R
        y.x0, y.y0, y.h, y.nx, y.ny = grid if grid else (0.0, 0.0, 1.0, 0, 0)

    def result(self, i, want_events, period):
        """member i's Flow, after the call (plain Python numbers throughout: a batch builds a thousand of these)"""
        if self._read is None:
            col = len(Flow.ARRAYS)
            self._read = (self._tab[:, col + 2:col + 5].tolist(), {f: v.tolist() for f, v in self.start.items()}, self.e0.tolist())
        (n_events, n_outside, first), start, e0 = self._read[0][i], self._read[1], self._read[2]
        n, c = self.shapes[i]
        L, R = self.lines.shape[0], self.areas.shape[0]
        r = Flow()
        for f in Flow.__slots__:
            setattr(r, f, None)
        r.first, r.n_events, r.n_outside, r.period = first, n_events, n_outside, period
        r.lines, r.areas, r.grid = self.lines, self.areas, self.grid
        for f, shape in (("line_count", (max(c - 1, 0), L, 2)), ("cross_n", (n, L, 2)), ("first_t", (n, L)), ("first_u", (n, L)),
                         ("first_speed", (n, L)), ("first_dir", (n, L)), ("occupancy", (c, R)), ("in_samples", (n, R)), ("in_first", (n, R)),
                         ("in_last", (n, R)), ("in_dist", (n, R))):
            at = start[f][i]
            setattr(r, f, self.arrays[f][at:at + math.prod(shape)].reshape(shape))
        if self.grid:
            at = start["grid_count"][i]
            r.grid_count = self.arrays["grid_count"][at:at + self.grid[3] * self.grid[4]].reshape(self.grid[4], self.grid[3])
        r.events = self.events[e0[i]:e0[i] + n_events] if want_events else None
        return r


CLEARANCE_EVENT_DTYPE = np.dtype({"names": ["i", "k", "edge", "seg", "dir", "t", "u"],
                                  "formats": [np.int32] * 5 + [np.float64] * 2,
                                  "offsets": [0, 4, 8, 12, 16, 24, 32], "itemsize": 40})        # csf_clearance_event

CLEARANCE_CHUNK = 512             # segments a workgroup runs against (csf_dev.h: CLR_CHUNK)
CLEARANCE_LAUNCHES = 3
CLEARANCE_MAX_SEGMENTS = 1 << 20


class Clearance:
    """What Engine.clearance returns for one engine (csf.h: csf_clearance): `first` the index of the first sample covered; per
    sample and road user [c, n] d the distance to the nearest segment of the road (NaN where the road user has no finite position),
    edge and seg which one (-1), t the clamped place along it; per station [c - 1, n] left and right the nearest segment on either
    side of the direction of travel (+inf: none, NaN: no station) with left_edge, right_edge, and cross the segments crossed; per road
    user [n] d_min with d_min_k, d_min_edge, d_min_seg, left_min, left_min_k, right_min, right_min_k, near_samples, near_first,
    near_last (the samples with d < d_event) and cross_n; per sample near_count [c] and cross_count [c - 1]; events
    (CLEARANCE_EVENT_DTYPE, every crossing, sorted by i, k, edge, seg; None when they were not asked for) with n_events their number.
    The per-sample and per-station arrays are None with per_sample=False.  offsets [n_edges + 1] are the road's; t of an event is in
    samples from `first`, `period` the seconds per sample of the recording (None when it is not known)."""

    CELL = (("d", np.float64), ("edge", np.int32), ("seg", np.int32), ("t", np.float64))
    STATION = (("left", np.float64), ("right", np.float64), ("left_edge", np.int32), ("right_edge", np.int32), ("cross", np.int32))
    USER = (("d_min", np.float64), ("d_min_k", np.int32), ("d_min_edge", np.int32), ("d_min_seg", np.int32),
            ("left_min", np.float64), ("left_min_k", np.int32), ("right_min", np.float64), ("right_min_k", np.int32),
            ("near_samples", np.int32), ("near_first", np.int32), ("near_last", np.int32), ("cross_n", np.int32))
    SAMPLE = (("near_count", np.int32), ("cross_count", np.int32))
    ARRAYS = CELL + STATION + USER + SAMPLE

    __slots__ = (("first", "period", "events", "n_events", "offsets", "d_event") + tuple(f for f, _ in ARRAYS)
                 + ("ids", "event_i_id"))                     # (SocialForceIntersection.clearance fills these)

    def _stations(self, who):
        if self.left is None:
            raise ValueError(f"{who}: the per-station arrays were not asked for (per_sample=True)")

    def lateral_position(self):
        """where across the path every station lies, [c - 1, n]: right / (left + right) - 0 on the right edge, 1 on the left one -,
        NaN where either side is not finite"""
        self._stations("lateral_position")
        both = np.isfinite(self.left) & np.isfinite(self.right)
        out = np.full(self.left.shape, np.nan)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[both] = (self.right / (self.left + self.right))[both]
        return out

    def width(self):
        """left + right per station [c - 1, n]: the width of the path as the road user met it"""
        self._stations("width")
        return self.left + self.right

    def off_road(self):
        """[c - 1, n] bool: an odd number of crossings has been made by the end of station k - the road user that started on the
        road is off it"""
        self._stations("off_road")
        return (np.cumsum(self.cross, axis=0, dtype=np.int64) & 1).astype(bool)

    def nearest_edge_share(self):
        """the share of the existing samples whose nearest segment belongs to each edge [n_edges]; NaN without a sample"""
        if self.edge is None:
            raise ValueError("nearest_edge_share: the per-sample arrays were not asked for (per_sample=True)")
        n_edges = len(self.offsets) - 1
        e = self.edge[self.edge >= 0]
        return np.bincount(e, minlength=n_edges)[:n_edges] / e.size if e.size else np.full(n_edges, np.nan)


def _clearance_road(who, road):
    """the checks of the road of Engine.clearance / batch_clearance, before any device call: (offsets [n_edges + 1] int64,
    xy [V, 2] float64) from a list of road elements (objects with edges(), whose edges have vertices) or an (offsets, xy) pair"""
    if road is None:
        raise ValueError(f"{who}: a road is needed (a list of road elements or an (offsets, xy) pair)")
    if isinstance(road, (tuple, list)) and len(road) == 2 and not hasattr(road[0], "edges"):
        off, xy = np.asarray(road[0]), np.array(road[1], dtype=np.float64, ndmin=2)
        if off.ndim != 1 or off.size < 1 or off.dtype.kind not in "iu":
            raise ValueError(f"{who}: offsets must be whole numbers [n_edges + 1]")
        off = off.astype(np.int64)
    else:
        if hasattr(road, "edges"):
            road = [road]
        try:
            edges = [e for el in road for e in el.edges()]
            verts = [np.array(e.vertices, dtype=np.float64, ndmin=2) for e in edges]
        except (TypeError, AttributeError):
            raise ValueError(f"{who}: road must be a list of road elements or an (offsets, xy) pair") from None
        if any(v.ndim != 2 or v.shape[1] != 2 for v in verts):
            raise ValueError(f"{who}: the vertices of an edge must be [k, 2]")
        off = np.r_[0, np.cumsum([v.shape[0] for v in verts])].astype(np.int64)
        xy = np.vstack(verts) if verts else np.zeros((0, 2))
    if off.size < 2:
        raise ValueError(f"{who}: the road has no edge")
    if xy.ndim != 2 or xy.shape[1] != 2:
        raise ValueError(f"{who}: xy must be [V, 2] (got shape {xy.shape})")
    if off[0] != 0 or off[-1] != xy.shape[0] or (np.diff(off) < 2).any():
        raise ValueError(f"{who}: offsets must start at 0, end at the {xy.shape[0]} vertices, and give every edge at least 2 (got {off.tolist()[:8]} ...)")
    if xy.shape[0] - (off.size - 1) > CLEARANCE_MAX_SEGMENTS:
        raise ValueError(f"{who}: at most 2^20 segments")
    if not np.isfinite(xy).all():
        raise ValueError(f"{who}: the road has a non-finite coordinate")
    inner = np.ones(xy.shape[0] - 1, bool)
    inner[off[1:-1] - 1] = False                                 # (the step from one polyline's end to the next one's start is no segment)
    dx, dy = np.diff(xy[:, 0])[inner], np.diff(xy[:, 1])[inner]
    with np.errstate(over="ignore"):
        dd = dx * dx + dy * dy
    if not ((dd > 0) & np.isfinite(dd)).all():
        raise ValueError(f"{who}: segment {int(np.argmin((dd > 0) & np.isfinite(dd)))} of the road has no length or a non-finite one")
    return np.ascontiguousarray(off), np.ascontiguousarray(xy)


def _clearance_d_event(who, d_event):
    if isinstance(d_event, bool) or not _is_number(d_event) or not np.isfinite(d_event) or d_event < 0:
        raise ValueError(f"{who}: d_event must be finite and >= 0 (got {d_event!r})")
    return float(d_event)


def _clearance_capacity_guess(stations):
    """room for events in the first call: a road user that keeps to its path crosses no edge"""
    return min(max(64, stations // 8), 1 << 16)


class _ClearancePack(_Pack):
    """_Pack of csf_clearance_out records (shapes: (n, count) per member), and the csf_clearance_road they share"""

    def __init__(self, shapes, off, xy, caps, per_sample):
        self.shapes, self.off, self.xy, self.per_sample = shapes, off, xy, per_sample
        n = np.array([n for n, _ in shapes], dtype=np.int64)
        c = np.array([c for _, c in shapes], dtype=np.int64)
        rows = {}
        rows.update({f: c * n for f, _ in Clearance.CELL})
        rows.update({f: np.maximum(c - 1, 0) * n for f, _ in Clearance.STATION})
        rows.update({f: n for f, _ in Clearance.USER})
        rows.update(near_count=c, cross_count=np.maximum(c - 1, 0))
        wide = {f for f, _ in Clearance.CELL + Clearance.STATION}
        self.start = dict(zip(rows, _starts(*rows.values())))
        self.arrays = {f: (np.empty(int(self.start[f][-1]), dt) if per_sample or f not in wide else None) for f, dt in Clearance.ARRAYS}
        columns = [(col, self.arrays[f], self.start[f]) for col, (f, _) in enumerate(Clearance.ARRAYS)]   # (in header order)
        self._records(_ffi.ClearanceOut, columns, len(Clearance.ARRAYS), caps, CLEARANCE_EVENT_DTYPE)
        self._read = None                                        # what the call wrote into the records, read once (result)
        y = self.road = _ffi.ClearanceRoad()
        y.offsets, y.xy, y.n_edges = off.ctypes.data, xy.ctypes.data, off.size - 1

    def result(self, i, want_events, period, d_event):
        """member i's Clearance, after the call"""
        if self._read is None:
            col = len(Clearance.ARRAYS)
            self._read = (self._tab[:, col + 2:col + 4].tolist(), {f: v.tolist() for f, v in self.start.items()}, self.e0.tolist())
        (n_events, first), start, e0 = self._read[0][i], self._read[1], self._read[2]
        n, c = self.shapes[i]
        r = Clearance()
        for f in Clearance.__slots__:
            setattr(r, f, None)
        r.first, r.n_events, r.period, r.offsets, r.d_event = first, n_events, period, self.off, d_event
        shapes = [(Clearance.CELL, (c, n)), (Clearance.STATION, (max(c - 1, 0), n)), (Clearance.USER, (n,)),
                  (Clearance.SAMPLE[:1], (c,)), (Clearance.SAMPLE[1:], (max(c - 1, 0),))]
        for kind, shape in shapes:
            for f, _ in kind:
                if self.arrays[f] is not None:
                    at = start[f][i]
                    setattr(r, f, self.arrays[f][at:at + math.prod(shape)].reshape(shape))
        r.events = self.events[e0[i]:e0[i] + n_events] if want_events else None
        return r


BODY_EVENT_DTYPE = np.dtype([("sample", np.int64), ("i", np.int32), ("j", np.int32), ("gap", np.float64), ("ttc", np.float64)])   # csf_body_event


class BodyEncounters:
    """What Engine.body_encounters returns for one engine: `first` the index of the first sample covered (-1: the current state),
    `extents` [n, 3] as the call had them, per sample gap_min, gap_with, ttc_min, ttc_with [count, n] (None when per_sample was off),
    over the window run_gap_min, run_gap_with, run_gap_sample, run_ttc_min, run_ttc_with, run_ttc_sample and overlap_n [n], and
    events (BODY_EVENT_DTYPE, sorted by sample, i, j; None when no threshold was given) with n_events their number."""

    __slots__ = ("first", "extents", "gap_min", "gap_with", "ttc_min", "ttc_with", "run_gap_min", "run_gap_with", "run_gap_sample",
                 "run_ttc_min", "run_ttc_with", "run_ttc_sample", "overlap_n", "events", "n_events",
                 "ids", "gap_with_id", "ttc_with_id", "run_gap_with_id", "run_ttc_with_id")   # (SocialForceIntersection.body_encounters fills these)

    def collisions(self):
        """the events whose outlines overlap (gap 0), or None when the call fetched no events"""
        return None if self.events is None else self.events[self.events["gap"] == 0.0]


def _body_events_wanted(gap_event, ttc_event):
    return (gap_event is not None and gap_event >= 0) or (ttc_event is not None and ttc_event > 0)


def _body_thresholds(who, gap_event, ttc_event):
    """(gap_event, ttc_event) as the C ABI takes them: None is a threshold that is off"""
    for name, v in (("gap_event", gap_event), ("ttc_event", ttc_event)):
        if v is not None and (not _is_number(v) or not np.isfinite(v)):
            raise ValueError(f"{who}: {name} must be None or a finite number (got {v!r})")
    return (-1.0 if gap_event is None else float(gap_event)), (0.0 if ttc_event is None else float(ttc_event))


def _body_extents_shape(who, extents, n, member=None):
    """extents - one (front, rear, half_width) for everybody or an [n, 3] array - as a contiguous fp64 [n, 3]; values unchecked"""
    where = who if member is None else f"{who}: member {member}"
    if extents is None:
        raise ValueError(f"{where}: extents are needed: one (front, rear, half_width) or an [n, 3] array")
    try:
        a = np.asarray(extents, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{where}: extents must be numbers: one (front, rear, half_width) or an [n, 3] array") from None
    if a.shape == (3,):
        a = np.broadcast_to(a, (n, 3))
    if a.shape != (n, 3):
        raise ValueError(f"{where}: extents must be one (front, rear, half_width) or an [{n}, 3] array (got shape {a.shape})")
    return np.ascontiguousarray(a)


def _body_extents_bad(a):
    """the first row of extents [k, 3] that the C ABI would refuse, or -1"""
    bad = ~np.isfinite(a).all(axis=1) | (a[:, 0] < 0) | (a[:, 1] < 0) | ~(a[:, 0] + a[:, 1] > 0) | ~(a[:, 2] > 0)
    return int(np.flatnonzero(bad)[0]) if bad.any() else -1


_BODY_EXTENTS_RULE = "finite, front >= 0, rear >= 0, front + rear > 0, half_width > 0"


def _body_extents(who, extents, n):
    a = _body_extents_shape(who, extents, n)
    u = _body_extents_bad(a)
    if u >= 0:
        raise ValueError(f"{who}: road user {u} has the extents {tuple(float(v) for v in a[u])}: {_BODY_EXTENTS_RULE}")
    return a


def _batch_body_extents(who, extents, ns):
    """one (front, rear, half_width) for every member, or a list with a triple or an [n, 3] array per member: an [n, 3] array each
    (the values of all members are checked in one pass: a batch has a thousand members)"""
    if extents is None:
        raise ValueError(f"{who}: extents are needed: one (front, rear, half_width) or a list with one entry per member")
    single = hasattr(extents, "__len__") and len(extents) == 3 and all(_is_number(v) for v in extents)
    if not single and (isinstance(extents, np.ndarray) or not hasattr(extents, "__len__") or len(extents) != len(ns)):
        raise ValueError(f"{who}: extents must be one (front, rear, half_width) or a list with one entry for each of the {len(ns)} members")
    out = [_body_extents_shape(who, extents if single else extents[i], n, i) for i, n in enumerate(ns)]
    row = _body_extents_bad(np.concatenate(out)) if out else -1
    if row >= 0:
        i = int(np.searchsorted(np.cumsum(ns), row, side="right"))
        u = row - int(np.sum(ns[:i]))
        raise ValueError(f"{who}: member {i}: road user {u} has the extents {tuple(float(v) for v in out[i][u])}: {_BODY_EXTENTS_RULE}")
    return out


class _BodyPack(_Pack):
    """_Pack of csf_body_out records (as _EncounterPack)"""

    def __init__(self, shapes, per_sample, caps):
        self.shapes, self.caps = shapes, caps
        self.c0, self.n0 = _starts([n * c for n, c in shapes], [n for n, _ in shapes])
        nc, nn = (int(self.c0[-1]), int(self.n0[-1]))
        self.per = None
        if per_sample:
            self.per = (np.empty(nc), np.empty(nc, np.int32), np.empty(nc), np.empty(nc, np.int32))
        # (an empty window leaves them as they are: a minimum of +inf with nobody, at no sample, and no overlap)
        self.run = (np.full(nn, np.inf), np.full(nn, -1, np.int32), np.full(nn, -1, np.int64),
                    np.full(nn, np.inf), np.full(nn, -1, np.int32), np.full(nn, -1, np.int64), np.zeros(nn, np.int64))
        columns = [(col, a, self.c0) for col, a in enumerate(self.per or ())] + [(col, a, self.n0) for col, a in enumerate(self.run, start=4)]
        self._records(_ffi.BodyOut, columns, 11, caps, BODY_EVENT_DTYPE)

    def result(self, i, extents, want_events):
        n, count = self.shapes[i]
        o = self.outs[i]
        r = BodyEncounters()
        r.first, r.extents, r.n_events = int(o.first_sample), extents, int(o.n_events)
        r.ids = r.gap_with_id = r.ttc_with_id = r.run_gap_with_id = r.run_ttc_with_id = None
        c, u = int(self.c0[i]), int(self.n0[i])
        if self.per is None:
            r.gap_min = r.gap_with = r.ttc_min = r.ttc_with = None
        else:
            r.gap_min, r.gap_with, r.ttc_min, r.ttc_with = (a[c:c + n * count].reshape(count, n) for a in self.per)
        (r.run_gap_min, r.run_gap_with, r.run_gap_sample, r.run_ttc_min, r.run_ttc_with, r.run_ttc_sample, r.overlap_n) = (a[u:u + n] for a in self.run)
        r.events = self._events_of(i, r.n_events, want_events)
        return r


class Engine:
    """One population of one vehicle class on one MI355X (csf_engine)."""

    _rec_stride = None    # the stride of the state ring, as record / enable_history were last called (PostEncroachment.period)

    # what intersection.py keeps on an engine.  Declared on the class, not assigned in __init__: two more entries in every instance's
    # dictionary cost the batched calls over 256 engines 8 % of their host time (profiles/mirror_refactor_ab.txt)
    _together = None      # the engines of the batch this one was last joined to (_batch_of)
    _dense_ring = False   # it has the record ring of the dense routes (SocialForceIntersection._dense_engine)

    def __init__(self, params, capacity, device=0):
        self._lib = _ffi.load()
        self._h = None
        if not isinstance(params, Params):
            raise TypeError("params must be a cyclistsocialforce_amd._ffi.Params")
        self.params = params
        self.model = int(params.model)
        self.ns = N_STATES[self.model]
        h = self._lib.csf_create_v(C.byref(params), C.sizeof(params), _ffi.ABI_VERSION, int(capacity), int(device))
        if not h:
            raise EngineError(self._lib.csf_last_error(None).decode())
        self._h = C.c_void_p(h)
        self.capacity = int(capacity)

    # -- plumbing ---------------------------------------------------------------------------
    def _ck(self, rc):
        if rc != 0:
            raise EngineError(f"[{rc}] " + self._lib.csf_last_error(self._h).decode())

    def close(self):
        if self._h:
            self._lib.csf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def n(self):
        return int(self._lib.csf_num_agents(self._h))

    # -- population -------------------------------------------------------------------------
    def add_agents(self, s0, v_desired):
        s0 = np.asarray(s0, dtype=np.float64)
        if s0.ndim != 2 or s0.shape[1] < self.ns:
            raise ValueError(f"s0 must be [n, >={self.ns}]")
        s0 = _f64(s0[:, : self.ns])
        vd = _f64(np.broadcast_to(np.asarray(v_desired, dtype=np.float64), (s0.shape[0],)))
        self._ck(self._lib.csf_add_agents(self._h, s0.shape[0], _ptr(s0), _ptr(vd)))

    def remove_agents(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        self._ck(self._lib.csf_remove_agents(self._h, idx.size, _ptr(idx)))

    def replace_agents(self, leave, s0, v_desired, offsets, xyz_stop):
        """One traffic step (include/csf.h: csf_replace_agents): road users `leave` (indices) go, the rows of s0 join behind the rest
        with destination queues (offsets [n + 1], xyz_stop [sum, 3]).  Arrays that are already contiguous and of the right type
        are passed as they are."""
        leave = np.ascontiguousarray(leave, dtype=np.int32)
        s0 = np.asarray(s0, dtype=np.float64).reshape(-1, max(np.shape(s0)[-1] if np.ndim(s0) == 2 else self.ns, 1))
        if s0.size and s0.shape[1] < self.ns:
            raise ValueError(f"s0 must be [n, >={self.ns}]")
        s0 = _f64(s0[:, : self.ns])
        n = s0.shape[0]
        vd = _f64(np.broadcast_to(np.asarray(v_desired, dtype=np.float64), (n,)))
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        rows = _f64(xyz_stop)
        if off.size != n + 1 or rows.size != 3 * (int(off[-1]) if n else 0):
            raise ValueError("offsets [n + 1] and xyz_stop [offsets[-1], 3] must describe one queue per arrival")
        self._ck(self._lib.csf_replace_agents(self._h, leave.size, _ptr(leave), n, _ptr(s0), _ptr(vd), _ptr(off), _ptr(rows)))

    def set_dest_queue(self, agents, offsets, xyz_stop, reset=False):
        agents = np.ascontiguousarray(agents, dtype=np.int32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        xyz = _f64(xyz_stop).reshape(-1, 3)
        if offsets.shape != (agents.size + 1,) or offsets[-1] != xyz.shape[0]:
            raise ValueError("offsets must be [n+1] and end at the number of rows")
        self._ck(self._lib.csf_set_dest_queue(self._h, agents.size, _ptr(agents), _ptr(offsets), _ptr(xyz), int(reset)))  # reset: 0 append, 1 replace, 2 replace + keep pointer

    def set_script(self, agents, offsets, rows):
        """prescribed trajectories of UncontrolledVehicle road users (include/csf.h: csf_set_script): rows (x, y, psi, v)"""
        agents = np.ascontiguousarray(agents, dtype=np.int32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        rows = _f64(rows).reshape(-1, 4)
        if offsets.shape != (agents.size + 1,) or offsets[-1] != rows.shape[0]:
            raise ValueError("offsets must be [n+1] and end at the number of rows")
        self._ck(self._lib.csf_set_script(self._h, agents.size, _ptr(agents), _ptr(offsets), _ptr(rows)))

    def set_incremental(self, on=True):
        """population changes after the first tick: straight into the device arrays (True, default) or through the host
        mirror (include/csf.h: csf_set_incremental)"""
        self._ck(self._lib.csf_set_incremental(self._h, int(bool(on))))

    def set_road(self, offsets, verts, F0, sigma):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        verts = _f64(verts).reshape(-1, 2)
        F0 = _f64(F0)
        sigma = _f64(sigma)
        self._ck(self._lib.csf_set_road_vertices(self._h, offsets.size - 1, _ptr(offsets), _ptr(verts), _ptr(F0), _ptr(sigma)))

    def set_params(self, params):
        self._ck(self._lib.csf_set_params(self._h, C.byref(params)))
        self.params = params

    def set_param_classes(self, classes, cls=None, idx=None):
        """Parameter sets for a population whose vehicles own different params objects (vehicle.py:64-204) or are of
        different classes (intersection.py:797-823): `classes` a sequence of csf_params (set 0 replaces the engine's own),
        `cls[k]` the set of agent `idx[k]` (default: everyone).  With sets of several vehicle classes the state arrays
        take the widest layout (x, y, psi, v, delta, theta); install them before add_agents."""
        classes = list(classes)
        tab = (type(self.params) * len(classes))(*classes)
        rows_first = cls is not None and len(classes) < getattr(self, "_n_classes", 1)    # no row may point beyond the table
        if rows_first:
            self.set_agent_class(np.arange(self.n) if idx is None else idx, cls)
        self._ck(self._lib.csf_set_param_classes(self._h, len(classes), tab))
        self.params = classes[0]
        self._n_classes = len(classes)
        self.ns = int(self._lib.csf_num_states(self._h))         # sets of several vehicle classes: the widest state
        if cls is not None and not rows_first:
            self.set_agent_class(np.arange(self.n) if idx is None else idx, cls)

    def set_agent_class(self, idx, cls):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        cls = np.ascontiguousarray(np.broadcast_to(np.asarray(cls, dtype=np.int32), idx.shape))
        self._ck(self._lib.csf_set_agent_class(self._h, idx.size, _ptr(idx), _ptr(cls)))

    def set_v_desired(self, idx, v):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        v = _f64(np.broadcast_to(np.asarray(v, dtype=np.float64), idx.shape))
        self._ck(self._lib.csf_set_v_desired(self._h, idx.size, _ptr(idx), _ptr(v)))

    def set_priority_rule(self, rule):
        self._ck(self._lib.csf_set_priority_rule(self._h, int(rule)))

    def push_state(self, idx, s):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        s = _f64(s).reshape(idx.size, self.ns)
        self._ck(self._lib.csf_push_state(self._h, idx.size, _ptr(idx), _ptr(s)))

    def integrator_state(self):
        """(vehicle.x [n, 5] - InvPendulum: delta, ddelta, theta, dtheta, psi unwrapped, vehicle.py:1728-1733 -, the unwrapped
        yaw of the PlanarPoint / PlanarBicycle integrators [n], vehicle.zrid [n, 2]): what vehicle.s does not carry"""
        n = self.n
        x = np.zeros((n, 5)); psi = np.zeros(n); z = np.zeros((n, 2), dtype=np.uint8)
        self._ck(self._lib.csf_get_integrator_state(self._h, _ptr(x), _ptr(psi), _ptr(z)))
        return x, psi, z.astype(bool)

    def set_integrator_state(self, idx, x=None, psi_unwrapped=None, zrid=None):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        x = None if x is None else _f64(x).reshape(idx.size, 5)
        psi = None if psi_unwrapped is None else _f64(psi_unwrapped).reshape(idx.size)
        z = None if zrid is None else np.ascontiguousarray(zrid, dtype=np.uint8).reshape(idx.size, 2)
        self._ck(self._lib.csf_set_integrator_state(self._h, idx.size, _ptr(idx), *[None if a is None else _ptr(a) for a in (x, psi, z)]))

    # -- hot path ---------------------------------------------------------------------------
    def step(self, n_ticks=1, sync=False):
        self._ck(self._lib.csf_step(self._h, int(n_ticks)))
        if sync:
            self.sync()

    def sync(self):
        self._ck(self._lib.csf_sync(self._h))

    def calc_forces(self):
        self._ck(self._lib.csf_calc_forces(self._h))
        return self.forces()

    def apply_forces(self, Fx, Fy):
        Fx = _f64(Fx)
        Fy = _f64(Fy)
        if Fx.size != self.n or Fy.size != self.n:
            raise ValueError("Fx, Fy must have one entry per agent")
        self._ck(self._lib.csf_apply_forces(self._h, _ptr(Fx), _ptr(Fy)))

    def replay_forces(self, Fx, Fy, lengths=None, fix_speed=False, stride=1, return_states=True):
        """Calibration replay (calibration.py:438-460): Fx, Fy are [T, n]; returns states [T // stride, n, n_states]."""
        Fx = _f64(Fx)
        Fy = _f64(Fy)
        if Fx.ndim != 2 or Fx.shape != Fy.shape or Fx.shape[1] != self.n:
            raise ValueError("Fx, Fy must be [n_ticks, n_agents]")
        T = Fx.shape[0]
        out = np.zeros((T // stride, self.n, self.ns)) if return_states else None
        ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
        if ln is not None and ln.shape != (self.n,):
            raise ValueError("lengths must have one entry per agent")
        self._ck(self._lib.csf_replay_forces(self._h, T, _ptr(Fx), _ptr(Fy), None if ln is None else _ptr(ln),
                                             int(bool(fix_speed)), int(stride), None if out is None else _ptr(out)))
        return out

    # -- calibration (include/csf.h: csf_calib_load ...; cyclistsocialforce_amd.calibration drives it) ---------------------------
    def calib_load(self, s0, Fx, Fy, objective, feat, lengths=None, max_sets=256):
        """Make this EMPTY engine hold a calibration data set: start states s0 [n_seq, >= n_states], recorded forces Fx, Fy
        [T, n_seq], the objective [T, n_seq, n_feat] and the rows of vehicle.traj (0 .. 5) its columns are compared with;
        lengths [n_seq]: ticks of every sequence (default: T).  capacity >= max_sets * n_seq."""
        s0 = np.asarray(s0, dtype=np.float64)
        if s0.ndim != 2 or s0.shape[1] < self.ns:
            raise ValueError(f"s0 must be [n_seq, >={self.ns}]")
        s0 = _f64(s0[:, : self.ns])
        n_seq = s0.shape[0]
        Fx, Fy = _f64(Fx), _f64(Fy)
        if Fx.ndim != 2 or Fx.shape != Fy.shape or Fx.shape[1] != n_seq:
            raise ValueError("Fx, Fy must be [n_ticks, n_seq]")
        T = Fx.shape[0]
        feat = np.ascontiguousarray(feat, dtype=np.int32).reshape(-1)
        obj = _f64(objective)
        if obj.shape != (T, n_seq, feat.size):
            raise ValueError("objective must be [n_ticks, n_seq, n_feat]")
        ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
        if ln is not None and ln.shape != (n_seq,):
            raise ValueError("lengths must have one entry per sequence")
        self._ck(self._lib.csf_calib_load(self._h, n_seq, T, _ptr(s0), _ptr(Fx), _ptr(Fy), None if ln is None else _ptr(ln),
                                          _ptr(obj), feat.size, _ptr(feat), int(max_sets)))
        self._calib = (n_seq, T)

    def calib_eval(self, pods, fix_speed=True, states=False, stride=1):
        """Evaluate the parameter sets `pods` (a sequence of csf_params) on the loaded data set in one launch: sums
        [n_sets, n_seq, 2] = (sum d^2, sum |d|) per set and sequence, and with states=True the trajectories
        [T // stride, n_sets * n_seq, n_states] as well (slot = set * n_seq + seq)."""
        if getattr(self, "_calib", None) is None:
            raise EngineError("calib_eval: no calibration data set (calib_load first)")
        n_seq, T = self._calib
        pods = list(pods)
        tab = (Params * len(pods))(*pods)
        sums = np.zeros((len(pods), n_seq, 2))
        out = np.zeros((T // stride if stride >= 1 else 0, len(pods) * n_seq, self.ns)) if states else None
        self._ck(self._lib.csf_calib_eval(self._h, len(pods), tab, C.sizeof(Params), _ffi.ABI_VERSION, int(bool(fix_speed)),
                                          _ptr(sums), int(stride), None if out is None else _ptr(out)))
        return (sums, out) if states else sums

    def calib_clear(self):
        self._ck(self._lib.csf_calib_clear(self._h))
        self._calib = None

    def calib_launches(self):
        """kernel launches of calib_eval since calib_load: one per call"""
        n = C.c_int64(0)
        self._ck(self._lib.csf_calib_launches(self._h, C.byref(n)))
        return int(n.value)

    # -- calibration on closed-loop scenes (include/csf.h: csf_scene_calib_load ...; calibration.InteractionCalibration drives it) --
    def _scene_arrays(self, n_riders, s0, v_desired, dest_offsets, dest_xyz_stop, objective, feat, lengths):
        """the arguments the two scene loads share, checked and made contiguous: (nr, R, s0, vd, off, xyz, obj, feat, T, lengths)"""
        nr = np.ascontiguousarray(n_riders, dtype=np.int32).reshape(-1)
        if nr.size < 1:
            raise ValueError("n_riders must name at least one scene")
        R = int(nr.sum())
        s0 = np.asarray(s0, dtype=np.float64)
        if s0.ndim != 2 or s0.shape[0] != R or s0.shape[1] < self.ns:
            raise ValueError(f"s0 must be [sum(n_riders), >={self.ns}]")
        s0 = _f64(s0[:, : self.ns])
        vd = _f64(np.broadcast_to(np.asarray(v_desired, dtype=np.float64), (R,)))
        off = np.ascontiguousarray(dest_offsets, dtype=np.int64)
        xyz = _f64(dest_xyz_stop).reshape(-1, 3)
        if off.shape != (R + 1,) or off[0] < 0 or off[-1] > xyz.shape[0] or np.any(np.diff(off) < 1):
            raise ValueError("dest_offsets must be [sum(n_riders) + 1], ascending, with at least one row of dest_xyz_stop per rider")
        feat = np.ascontiguousarray(feat, dtype=np.int32).reshape(-1)
        obj = _f64(objective)
        if obj.ndim != 3 or obj.shape[1:] != (R, feat.size) or obj.shape[0] < 1:
            raise ValueError("objective must be [n_ticks, sum(n_riders), n_feat]")
        ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
        if ln is not None and ln.shape != (nr.size,):
            raise ValueError("lengths must have one entry per scene")
        return nr, R, s0, vd, off, xyz, obj, feat, obj.shape[0], ln

    def scene_calib_load(self, n_riders, s0, v_desired, dest_offsets, dest_xyz_stop, objective, feat, lengths=None, max_sets=256):
        """Make this EMPTY engine hold a data set of closed-loop scenes: n_riders [n_scn] road users per scene (1 .. 32, R their
        sum), start states s0 [R, >= n_states], v_desired [R] (or a scalar), the riders' destination queues in CSR form
        (dest_offsets [R + 1], dest_xyz_stop [rows, 3]), the objective [T, R, n_feat] and the rows of vehicle.traj (0 .. 5) its
        columns are compared with; lengths [n_scn]: ticks of every scene (default: T).  capacity >= max_sets * R."""
        nr, R, s0, vd, off, xyz, obj, feat, T, ln = self._scene_arrays(n_riders, s0, v_desired, dest_offsets, dest_xyz_stop, objective, feat, lengths)
        self._ck(self._lib.csf_scene_calib_load(self._h, nr.size, _ptr(nr), T, _ptr(s0), _ptr(vd), _ptr(off), _ptr(xyz),
                                                None if ln is None else _ptr(ln), _ptr(obj), feat.size, _ptr(feat), int(max_sets)))
        self._scene_calib = (R, T)

    def scene_calib_load_shared(self, n_riders, n_lanes, lane, enter, exit, s0, v_desired, dest_offsets, dest_xyz_stop, objective, feat,
                                lengths=None, max_sets=256):
        """scene_calib_load for scenes whose riders SHARE LANES: n_riders [n_scn] is the roster of every scene (>= 1, no upper bound, R
        their sum), n_lanes [n_scn] its lanes (1 .. 32), and per rider lane [R] (0 .. n_lanes - 1 of its scene) and the presence
        window enter [R], exit [R] (0 <= enter <= exit <= the length of the scene).  Riders of one lane take turns: their non-empty
        windows do not overlap.  Sums and states stay per RIDER; a row of the states is NaN wherever its rider is not present.
        capacity >= max(R, max_sets * sum(n_lanes)).  scene_calib_windows is refused on such a data set."""
        self._scene_load_lanes(self._lib.csf_scene_calib_load_shared, (), n_riders, n_lanes, lane, enter, exit, s0, v_desired, dest_offsets,
                               dest_xyz_stop, objective, feat, lengths, max_sets)

    def _scene_load_lanes(self, call, more, n_riders, n_lanes, lane, enter, exit, s0, v_desired, dest_offsets, dest_xyz_stop, objective, feat,
                          lengths, max_sets):
        """scene_calib_load_shared and scene_calib_load_wide: the same arrays, `more` the arguments behind max_sets"""
        nr, R, s0, vd, off, xyz, obj, feat, T, ln = self._scene_arrays(n_riders, s0, v_desired, dest_offsets, dest_xyz_stop, objective, feat, lengths)
        nl = np.ascontiguousarray(n_lanes, dtype=np.int32).reshape(-1)
        if nl.shape != nr.shape:
            raise ValueError("n_lanes has one entry per scene")
        ln_, en, ex = (np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (lane, enter, exit))
        if ln_.shape != (R,) or en.shape != (R,) or ex.shape != (R,):
            raise ValueError("lane, enter and exit must have one entry per rider of the data set")
        self._ck(call(self._h, nr.size, _ptr(nr), _ptr(nl), _ptr(ln_), _ptr(en), _ptr(ex), T, _ptr(s0), _ptr(vd), _ptr(off), _ptr(xyz),
                      None if ln is None else _ptr(ln), _ptr(obj), feat.size, _ptr(feat), int(max_sets), *more))
        self._scene_calib = (R, T)

    def scene_calib_load_wide(self, n_riders, n_lanes, lane, enter, exit, s0, v_desired, dest_offsets, dest_xyz_stop, objective, feat,
                              lengths=None, max_sets=256, wide_from=33):
        """scene_calib_load_shared for scenes with MORE THAN 32 ROAD USERS AT ONCE: n_lanes [n_scn] is 1 .. 256.  A scene with
        n_lanes >= wide_from (1 .. 257) is simulated by one workgroup of 256 threads for all its ticks, every other scene by the one-wave
        tick exactly as after scene_calib_load_shared; an evaluation launches one kernel per kind that the data set holds.  33 - the
        default - is the smallest scene the one-wave tick cannot take, not a measured crossover; 1 sends every scene to the wide
        kernel.  The road of a wide scene: padded vertices x P <= 16 384 with P = 64, 128 or 256.  Everything else is
        scene_calib_load_shared's."""
        self._scene_load_lanes(self._lib.csf_scene_calib_load_wide, (int(wide_from),), n_riders, n_lanes, lane, enter, exit, s0, v_desired,
                               dest_offsets, dest_xyz_stop, objective, feat, lengths, max_sets)

    def _scene_held(self, name, first="scene_calib_load"):
        """(R, T) of the loaded closed-loop data set; without one, `name` is the call that is refused"""
        if getattr(self, "_scene_calib", None) is None:
            raise EngineError(f"{name}: no closed-loop data set ({first} first)")
        return self._scene_calib

    @staticmethod
    def _scene_group8(group, R):
        """the group of every rider, checked: uint8 [R]"""
        g = np.asarray(group)
        if g.shape != (R,) or g.dtype.kind not in "iub":
            raise ValueError("group must have one integer entry per rider of the data set")
        if g.size and (g.min() < 0 or g.max() > 255):
            raise ValueError("group: entries are 0 .. n_groups - 1")
        return np.ascontiguousarray(g, dtype=np.uint8)

    @staticmethod
    def _scene_road_sets(n_sets, road_F0, road_sigma):
        """road_F0 and road_sigma per candidate set, [n_sets] each (None stays None)"""
        return tuple(None if a is None else _f64(np.broadcast_to(np.asarray(a, dtype=np.float64), (n_sets,))) for a in (road_F0, road_sigma))

    def _scene_outputs(self, n_sets, R, T, states, stride):
        """what an evaluation writes: sums [n_sets, R, 2] and, with states, the samples [T // stride, n_sets * R, n_states]"""
        return np.zeros((n_sets, R, 2)), np.zeros((T // stride if stride >= 1 else 0, n_sets * R, self.ns)) if states else None

    def scene_calib_eval(self, pods, states=False, stride=1, road_F0=None, road_sigma=None):
        """Evaluate the parameter sets `pods` (a sequence of csf_params) on the loaded scenes in one launch: sums [n_sets, R, 2] =
        (sum d^2, sum |d|) per set and RIDER (the riders of a scene are added by the caller, in rider order), and with states=True
        the trajectories [T // stride, n_sets * R, n_states] as well (slot = set * R + rider).  road_F0 / road_sigma [n_sets] (or
        scalars; both or neither): F_0 and sigma of every road vertex of the scenes' roads (scene_calib_road) for that set."""
        R, T = self._scene_held("scene_calib_eval")
        pods = list(pods)
        tab = (Params * len(pods))(*pods)
        sums, out = self._scene_outputs(len(pods), R, T, states, stride)
        if road_F0 is None and road_sigma is None:
            self._ck(self._lib.csf_scene_calib_eval(self._h, len(pods), tab, C.sizeof(Params), _ffi.ABI_VERSION, _ptr(sums), int(stride),
                                                    None if out is None else _ptr(out)))
        else:
            f0, sg = self._scene_road_sets(len(pods), road_F0, road_sigma)
            self._ck(self._lib.csf_scene_calib_eval_road(self._h, len(pods), tab, C.sizeof(Params), _ffi.ABI_VERSION,
                                                         None if f0 is None else _ptr(f0), None if sg is None else _ptr(sg), _ptr(sums),
                                                         int(stride), None if out is None else _ptr(out)))
        return (sums, out) if states else sums

    def scene_calib_road(self, edge_scene, offsets, verts, F0, sigma):
        """Road edges for scenes of the loaded data set, shared by all candidate sets: edge_scene [n_edges] the scene of every edge
        (non-decreasing), the rest as set_road takes it.  No edge (edge_scene empty or None) drops every road."""
        self._scene_held("scene_calib_road")
        es = np.ascontiguousarray([] if edge_scene is None else edge_scene, dtype=np.int32).reshape(-1)
        if es.size == 0:
            self._ck(self._lib.csf_scene_calib_road(self._h, 0, None, None, None, None, None))
            return
        offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        verts = _f64(verts).reshape(-1, 2)
        F0 = _f64(np.broadcast_to(np.asarray(F0, dtype=np.float64), (es.size,)))
        sigma = _f64(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (es.size,)))
        if offsets.shape != (es.size + 1,) or (offsets.size and offsets.max() > verts.shape[0]):
            raise ValueError("offsets must be [n_edges + 1] and stay within the vertices")
        self._ck(self._lib.csf_scene_calib_road(self._h, es.size, _ptr(es), _ptr(offsets), _ptr(verts), _ptr(F0), _ptr(sigma)))

    def scene_calib_replay(self, replayed, rows=None):
        """Riders of the loaded scenes that follow their recording: replayed [R] (bool), rows [T, n_rep, 4] = (x, y, psi, v) of the
        replayed riders, in rider order, after every tick.  They are sources of the field only; their sums are (0, 0).  None (or
        no rider marked) drops the replay."""
        R, T = self._scene_held("scene_calib_replay")
        if replayed is None:
            self._ck(self._lib.csf_scene_calib_replay(self._h, None, None))
            return
        mask = np.ascontiguousarray(np.asarray(replayed, dtype=bool), dtype=np.uint8)
        if mask.shape != (R,):
            raise ValueError("replayed must have one entry per rider of the data set")
        n_rep = int(mask.sum())
        if n_rep:
            rows = _f64(rows)
            if rows.shape != (T, n_rep, 4):
                raise ValueError("rows must be [n_ticks, replayed riders, 4]")
        self._ck(self._lib.csf_scene_calib_replay(self._h, _ptr(mask), _ptr(rows) if n_rep else None))

    def scene_calib_windows(self, enter, exit):
        """Presence windows of the riders of the loaded scenes: enter, exit [R] (int32), rider r is in its scene at the ticks
        enter[r] <= t < exit[r] (0 <= enter <= exit <= the length of its scene) and at every other tick neither a source nor a
        receiver of the field, not ticked, not put on its recording and not part of its sums.  None, None drops the windows."""
        R, _ = self._scene_held("scene_calib_windows")
        if enter is None and exit is None:
            self._ck(self._lib.csf_scene_calib_windows(self._h, None, None))
            return
        if enter is None or exit is None:
            raise ValueError("enter and exit are given together or not at all")
        en = np.ascontiguousarray(enter, dtype=np.int32)
        ex = np.ascontiguousarray(exit, dtype=np.int32)
        if en.shape != (R,) or ex.shape != (R,):
            raise ValueError("enter and exit must have one entry per rider of the data set")
        self._ck(self._lib.csf_scene_calib_windows(self._h, _ptr(en), _ptr(ex)))

    def scene_calib_groups(self, group, n_groups=None):
        """Rider GROUPS of the loaded scenes (scene_calib_load only), each with parameter sets of its own: group [R] (integers
        0 .. n_groups - 1), n_groups <= 4 (default: the largest entry + 1).  None, or n_groups <= 1, drops the groups.  With groups
        loaded an evaluation is scene_calib_eval_groups; scene_calib_eval is refused."""
        R, _ = self._scene_held("scene_calib_groups")
        if group is None:
            self._ck(self._lib.csf_scene_calib_groups(self._h, None, 0))
        else:
            g8 = self._scene_group8(group, R)
            self._ck(self._lib.csf_scene_calib_groups(self._h, _ptr(g8), int(g8.max()) + 1 if n_groups is None else int(n_groups)))
        self.ns = int(self._lib.csf_num_states(self._h))         # (the call replaces the classes of scene_calib_classes)

    def scene_calib_lane_groups(self, group, n_groups=None):
        """scene_calib_groups for a data set of scene_calib_load_shared / scene_calib_load_wide: group [R] per RIDER (integers
        0 .. n_groups - 1), n_groups <= 4 (default: the largest entry + 1); a lane's parameters are those of the rider it carries and
        change at a takeover.  None, or n_groups <= 1, drops the groups.  With groups loaded an evaluation is scene_calib_eval_groups;
        scene_calib_eval is refused.  A scene_calib_load data set takes scene_calib_groups and refuses this call."""
        R, _ = self._scene_held("scene_calib_lane_groups", "scene_calib_load_shared / scene_calib_load_wide")
        if group is None:
            self._ck(self._lib.csf_scene_calib_lane_groups(self._h, None, 0))
        else:
            g8 = self._scene_group8(group, R)
            self._ck(self._lib.csf_scene_calib_lane_groups(self._h, _ptr(g8), int(g8.max()) + 1 if n_groups is None else int(n_groups)))
        self.ns = int(self._lib.csf_num_states(self._h))         # (the call replaces the classes of scene_calib_lane_classes)

    def scene_calib_classes(self, group, models=None, s0=None):
        """Rider groups of DIFFERENT VEHICLE CLASSES on the loaded scenes (scene_calib_load only): group [R] (integers 0 .. G - 1), models
        [G] the vehicle class of every group (the constants of _ffi: BICYCLE, TWOD, INVPEND, PLANARPOINT, PLANARBIKE, BALANCINGRIDER;
        2 <= G <= 12) and s0 [R, <= 8] the start states in the widest layout (missing columns: 0).  `ns` becomes the widest state of the
        loaded classes; rows a class lacks stay 0.  An evaluation is scene_calib_eval_groups with tuple entry g of class models[g].  The
        call replaces the groups of scene_calib_groups and that call replaces these; None drops the classes."""
        self._scene_classes("scene_calib_classes", self._lib.csf_scene_calib_classes, None, group, models, s0)

    def scene_calib_lane_classes(self, group, models=None, s0=None):
        """scene_calib_classes for a data set of scene_calib_load_shared / scene_calib_load_wide: the same arguments, and the vehicle
        class is a property of the RIDER a lane carries - a lane changes its class when another rider takes it over.  An evaluation is
        scene_calib_eval_groups.  The call replaces the groups of scene_calib_lane_groups and that call replaces these; None drops the
        classes.  A scene_calib_load data set takes scene_calib_classes and refuses this call."""
        if not hasattr(self._lib, "csf_scene_calib_lane_classes"):
            raise EngineError("libcsf_hip.so has no csf_scene_calib_lane_classes: rebuild the library")
        self._scene_classes("scene_calib_lane_classes", self._lib.csf_scene_calib_lane_classes, "scene_calib_load_shared / scene_calib_load_wide",
                            group, models, s0)

    def _scene_classes(self, name, call, loader, group, models, s0):
        R, _ = self._scene_held(name, loader) if loader else self._scene_held(name)
        if group is None:
            self._ck(call(self._h, None, 0, None, None))
            self.ns = int(self._lib.csf_num_states(self._h))
            return
        g8 = self._scene_group8(group, R)
        if models is None or s0 is None:
            raise ValueError("models [n_groups] and s0 [R, <= 8] are needed with group")
        m = np.ascontiguousarray(models, dtype=np.int32).reshape(-1)
        s = np.asarray(s0, dtype=np.float64)
        if s.ndim != 2 or s.shape[0] != R or not 4 <= s.shape[1] <= 8:
            raise ValueError("s0 must be [sum(n_riders), 4 .. 8]: the start states in the widest layout")
        wide = np.zeros((R, 8))
        wide[:, : s.shape[1]] = s
        self._ck(call(self._h, _ptr(g8), int(m.size), _ptr(m), _ptr(wide)))
        self.ns = int(self._lib.csf_num_states(self._h))

    def scene_calib_eval_groups(self, pods, road_F0=None, road_sigma=None, states=False, stride=1):
        """scene_calib_eval for riders in groups: `pods` is a sequence of n_groups-tuples of csf_params, tuple k the candidate k and
        its entry g what the riders of group g carry.  A rider is simulated with its own set and acts on the others with its own
        set's field and field of view; the priority rule of a candidate is its first entry's.  Returns what scene_calib_eval returns."""
        R, T = self._scene_held("scene_calib_eval_groups")
        pods = [tuple(p) if isinstance(p, (tuple, list)) else (p,) for p in pods]
        if not pods or any(len(p) != len(pods[0]) or not p for p in pods):
            raise ValueError("pods: a non-empty sequence of tuples of one length, one csf_params per group")
        G = len(pods[0])
        tab = (Params * (len(pods) * G))(*[p for t in pods for p in t])
        sums, out = self._scene_outputs(len(pods), R, T, states, stride)
        f0, sg = self._scene_road_sets(len(pods), road_F0, road_sigma)
        self._ck(self._lib.csf_scene_calib_eval_groups(self._h, len(pods), G, tab, C.sizeof(Params), _ffi.ABI_VERSION,
                                                       None if f0 is None else _ptr(f0), None if sg is None else _ptr(sg), _ptr(sums),
                                                       int(stride), None if out is None else _ptr(out)))
        return (sums, out) if states else sums

    def scene_calib_clear(self):
        self._ck(self._lib.csf_scene_calib_clear(self._h))
        self._scene_calib = None
        self.ns = int(self._lib.csf_num_states(self._h))         # (scene_calib_classes: the engine's own width again)

    def scene_calib_launches(self):
        """kernel launches of scene_calib_eval since scene_calib_load: one per call (after scene_calib_load_wide: one per call and kind
        of scene - narrow, wide - the data set holds)"""
        n = C.c_int64(0)
        self._ck(self._lib.csf_scene_calib_launches(self._h, C.byref(n)))
        return int(n.value)

    def dest_force(self):
        fx = np.zeros(self.n)
        fy = np.zeros(self.n)
        self._ck(self._lib.csf_dest_force(self._h, _ptr(fx), _ptr(fy)))
        return fx, fy

    # -- read-back --------------------------------------------------------------------------
    def _readback_arrays(self):
        """fresh arrays of one read-back: s [n, n_states], ptr [n] int32, zn [n, 3] one-hot uint8, fx [n], fy [n]"""
        n = self.n
        return np.zeros((n, self.ns)), np.zeros(n, dtype=np.int32), np.zeros((n, 3), dtype=np.uint8), np.zeros(n), np.zeros(n)

    def _readback_ptrs(self, what, arrays):
        """the addresses of a caller's read-back arrays (s, ptr, zn, fx, fy; None where an array is None), checked"""
        n = self.n
        shapes = (((n, self.ns), np.float64), ((n,), np.int32), ((n, 3), None), ((n,), np.float64), ((n,), np.float64))
        for a, (shape, dt) in zip(arrays, shapes):
            if a is not None and not (isinstance(a, np.ndarray) and a.flags.c_contiguous and a.shape == shape
                                      and (a.dtype == dt if dt is not None else a.dtype.itemsize == 1)):
                raise ValueError(f"{what}: s [n, n_states] float64, ptr [n] int32, zn [n, 3] of one byte each, fx / fy [n] "
                                 "float64, C-contiguous")
        return [None if a is None else a.ctypes.data for a in arrays]

    def state(self, with_nav=False):
        """[n, n_states] state (and destination pointers, one-hot navigation state, tick count): one packed transfer
        (csf_get_tick; csf_get_state copies component by component)"""
        s, ptr, zn, _, _, tick = self.tick_snapshot(forces=False)
        return (s, ptr, zn, tick) if with_nav else s

    def state_by_component(self, with_nav=False):
        """the same through csf_get_state"""
        s, ptr, zn, _, _ = self._readback_arrays()
        if not with_nav:
            self._ck(self._lib.csf_get_state(self._h, _ptr(s), None, None, None))
            return s
        tick = C.c_int64(0)
        self._ck(self._lib.csf_get_state(self._h, _ptr(s), _ptr(ptr), _ptr(zn), C.byref(tick)))
        return s, ptr, zn.astype(bool), tick.value

    def tick_snapshot(self, forces=True):
        """state [n, n_states], destination pointers, one-hot navigation state, total forces and the tick count in one
        device-to-host transfer (csf_get_tick)"""
        s, ptr, zn, fx, fy = self._readback_arrays()
        tick = C.c_int64(0)
        self._ck(self._lib.csf_get_tick(self._h, _ptr(s), _ptr(ptr), _ptr(zn), _ptr(fx) if forces else None,
                                        _ptr(fy) if forces else None, C.byref(tick)))
        return s, ptr, zn.astype(bool), (fx if forces else None), (fy if forces else None), tick.value

    def step_snapshot(self, n_ticks=1, forces=True, reuse=False):
        """step(n_ticks) and tick_snapshot() in one call (csf_step_get_tick): a handful of road users then cost one launch and
        one wait per call.  reuse: the arrays returned are the engine's own buffers, overwritten by the next call (the host
        mirror copies them into its bulk arrays at once) - at three road users the allocations are a fifth of the call."""
        if reuse:
            key = (self.n, self.ns)
            if getattr(self, "_snap_key", None) != key:
                bufs = self._readback_arrays()
                self._snap_key, self._snap_bufs, self._snap_ptrs, self._snap_tick = key, bufs, [_ptr(b) for b in bufs], C.c_int64(0)
            s, ptr, zn, fx, fy = self._snap_bufs
            p = self._snap_ptrs
            self._ck(self._lib.csf_step_get_tick(self._h, int(n_ticks), p[0], p[1], p[2], p[3] if forces else None,
                                                 p[4] if forces else None, C.byref(self._snap_tick)))
            return s, ptr, zn, (fx if forces else None), (fy if forces else None), self._snap_tick.value
        s, ptr, zn, fx, fy = self._readback_arrays()
        tick = C.c_int64(0)
        self._ck(self._lib.csf_step_get_tick(self._h, int(n_ticks), _ptr(s), _ptr(ptr), _ptr(zn), _ptr(fx) if forces else None,
                                             _ptr(fy) if forces else None, C.byref(tick)))
        return s, ptr, zn.astype(bool), (fx if forces else None), (fy if forces else None), tick.value

    def step_into(self, n_ticks, s, ptr, zn, fx=None, fy=None):
        """step_snapshot straight into the caller's arrays: s [n, n_states] float64, ptr [n] int32, zn [n, 3] bool or uint8
        (one-hot), fx / fy [n] float64 or None - all C-contiguous (the host mirror's own bulk arrays: no copy in between)"""
        n = self.n
        key = (s.ctypes.data, ptr.ctypes.data, zn.ctypes.data, 0 if fx is None else fx.ctypes.data, 0 if fy is None else fy.ctypes.data, n)
        if getattr(self, "_into_key", None) != key:
            self._into_ptrs = self._readback_ptrs("step_into", (s, ptr, zn, fx, fy))
            self._into_key = key
            self._into_tick = C.c_int64(0)
        p = self._into_ptrs
        self._ck(self._lib.csf_step_get_tick(self._h, int(n_ticks), p[0], p[1], p[2], p[3], p[4], C.byref(self._into_tick)))
        return self._into_tick.value

    @property
    def tick(self):
        t = C.c_int64(0)
        self._ck(self._lib.csf_get_state(self._h, None, None, None, C.byref(t)))
        return t.value

    def forces(self):
        fx = np.zeros(self.n)
        fy = np.zeros(self.n)
        self._ck(self._lib.csf_get_forces(self._h, _ptr(fx), _ptr(fy)))
        return fx, fy

    def force_parts(self):
        a = [np.zeros(self.n) for _ in range(4)]
        self._ck(self._lib.csf_get_force_parts(self._h, *[_ptr(x) for x in a]))
        return a

    def status(self):
        st = np.zeros(self.n, dtype=np.uint32)
        self._ck(self._lib.csf_status(self._h, _ptr(st)))
        return st

    def enable_history(self, stride=1, capacity=3000):
        self._ck(self._lib.csf_enable_history(self._h, int(stride), int(capacity)))
        self._rec_stride = int(stride)

    def history(self, first, count):
        out = np.zeros((count, self.n, self.ns))
        self._ck(self._lib.csf_get_history(self._h, int(first), int(count), _ptr(out)))
        return out

    def record(self, stride=1, capacity=3000, forces=True):
        """csf_record: every `stride`-th tick's state - and total force - into device rings of `capacity` samples, written by
        whatever kernel ticks the engine: unlike enable_history it keeps the one-wave tick and the batched launch."""
        what = _ffi.REC_STATE | (_ffi.REC_FORCE if forces else 0)
        self._ck(self._lib.csf_record(self._h, int(stride), int(capacity), what))
        self._rec_forces = bool(forces)
        self._rec_stride = int(stride)

    def recorded(self, first, count):
        """samples [first, first + count) of the recording: (S [count, n, n_states], F [count, n, 2] or None) - sample k is the
        state after tick (k + 1) * stride and the total force of that tick; one gather launch and one wait (csf_get_record)"""
        n = self.n
        S = np.zeros((int(count), n, self.ns))
        F = np.zeros((int(count), n, 2)) if getattr(self, "_rec_forces", False) else None
        self._ck(self._lib.csf_get_record(self._h, int(first), int(count), _ptr(S), None if F is None else _ptr(F)))
        return S, F

    @staticmethod
    def batch_recorded(engines, n_last, only=None):
        """the last n_last samples of every recording member of a batch (the engines in join order): a list of (S, F, first) -
        S [n_last, n, n_states], F [n_last, n, 2] (None without a force ring), first the index of S[0] - and None for members
        that do not record (or are not in `only`, a collection of members to read).  One gather launch, one transfer and one wait
        for the whole batch (csf_batch_get_record).  The arrays are the caller's: new ones whenever the set of engines, their
        populations or n_last changed, else the previous call's, overwritten - the csf_record_out array is kept with them."""
        engines, arr = Engine._batch_array(engines, "batch_recorded")
        n_last = int(n_last)
        if n_last < 0:
            raise ValueError("batch_recorded: n_last must be >= 0")
        pick = None if only is None else {id(e) for e in only}
        key = (tuple(id(e) for e in engines), tuple(e.n for e in engines), n_last, None if pick is None else tuple(sorted(pick)))
        cache = getattr(engines[0], "_rec_cache", None)
        if cache is None or cache[0] != key:
            outs = (_ffi.RecordOut * len(engines))()
            firsts = (C.c_int64 * len(engines))()
            res = []
            for i, e in enumerate(engines):
                if not hasattr(e, "_rec_forces") or (pick is not None and id(e) not in pick):
                    res.append(None)
                    continue
                S = np.zeros((n_last, e.n, e.ns))
                F = np.zeros((n_last, e.n, 2)) if e._rec_forces else None
                outs[i].s = S.ctypes.data
                outs[i].F = None if F is None else F.ctypes.data
                outs[i].first_sample = C.cast(C.byref(firsts, i * C.sizeof(C.c_int64)), C.POINTER(C.c_int64))
                res.append((S, F))
            cache = engines[0]._rec_cache = (key, arr, outs, firsts, res)
        _, arr, outs, firsts, res = cache
        Engine._group_call("csf_batch_get_record", engines, arr, n_last, outs)
        return [None if r is None else (r[0], r[1], firsts[i]) for i, r in enumerate(res)]

    def pair_force(self, src, x, y, psi, apply_fov=False):
        src = _f64(src).reshape(4)
        x = _f64(x); y = _f64(y); psi = _f64(psi)
        fx = np.zeros(x.size)
        fy = np.zeros(x.size)
        self._ck(self._lib.csf_pair_force(self._h, _ptr(src), x.size, _ptr(x), _ptr(y), _ptr(psi), int(apply_fov), _ptr(fx), _ptr(fy)))
        return fx, fy

    def field_map(self, x, y, psi=None, crowd=True, road=True, fov=False, skip=-1):
        """the force field at arbitrary probe points (csf.h: csf_field_map; scenarios/curve-scenario.py:90-125): x, y (and psi, the
        heading a road user would have there) of any common shape -> (Fx, Fy) of that shape.  crowd: the sum of the live road users'
        fields, each its class's field with its own parameter set, unclamped; road: the road-edge term; fov: the probe is a receiver
        of heading psi - the mask of intersection.py:690-745 with the priority rule; skip: a road user (population order) left out as a
        source.  psi may be a scalar; it may be None only without the crowd term.  One launch per term, every pair evaluated."""
        x = np.asarray(x, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        if x.shape != y.shape:
            raise ValueError(f"field_map: x {x.shape} and y {y.shape} differ in shape")
        if not crowd and not road:
            raise ValueError("field_map: neither the crowd term nor the road term is asked for")
        if fov and not crowd:
            raise ValueError("field_map: fov masks the crowd term - it needs crowd=True")
        if psi is None:
            if crowd:
                raise ValueError("field_map: the crowd term needs the probes' headings psi")
        else:
            psi = np.asarray(psi, dtype=np.float64)
            if psi.ndim == 0:
                psi = np.full(x.shape, float(psi))
            elif psi.shape != x.shape:
                raise ValueError(f"field_map: psi {psi.shape} and x {x.shape} differ in shape")
            psi = _f64(psi)
        shape = x.shape
        x, y = _f64(x), _f64(y)
        fx, fy = np.zeros(x.size), np.zeros(x.size)
        what = (_ffi.FIELD_CROWD if crowd else 0) | (_ffi.FIELD_ROAD if road else 0) | (_ffi.FIELD_FOV if fov else 0)
        self._ck(self._lib.csf_field_map(self._h, x.size, _ptr(x), _ptr(y), None if psi is None else _ptr(psi), what, int(skip), _ptr(fx), _ptr(fy)))
        return fx.reshape(shape), fy.reshape(shape)

    def field_map_launches(self):
        """launches of field_map so far: one per requested term and call (csf.h: csf_field_map_launches)"""
        n = C.c_int64(0)
        self._ck(self._lib.csf_field_map_launches(self._h, C.byref(n)))
        return n.value

    # -- the measures of a recording: one route for a single engine, one for a batch --------------------------
    def _measure(self, make_pack, call, cap, want):
        """the pack of a single engine's call: make_pack([cap]) holds the outputs, call(pack) is the C ABI's return code.  Events
        are fetched with the capacity `cap`; when more were found, one second call with the exact capacity - only where events
        are wanted: flow and clearance count their crossings whether or not, the other measures count none without a threshold."""
        while True:
            pack = make_pack([cap])
            self._ck(call(pack))
            if not want or pack.outs[0].n_events <= cap:
                return pack
            cap = int(pack.outs[0].n_events)

    @staticmethod
    def _batch_measure(symbol, engines, arr, make_pack, args, caps, want, result):
        """the same for a batch: make_pack(caps), then the C ABI's `symbol` with args(pack) behind the engines; a list with
        result(pack, i, engine) per member, None for members that do not record (first_sample -2)"""
        while True:
            pack = make_pack(caps)
            Engine._group_call(symbol, engines, arr, *args(pack))
            found = [int(o.n_events) for o in pack.outs]
            if not want or all(f <= c for f, c in zip(found, caps)):
                return [None if pack.outs[i].first_sample == -2 else result(pack, i, e) for i, e in enumerate(engines)]
            caps = [max(f, c) for f, c in zip(found, caps)]

    def _launches(self, symbol):
        n = C.c_int64(0)
        self._ck(getattr(self._lib, symbol)(self._h, C.byref(n)))
        return n.value

    # -- encounters: closest approach and time to collision (include/csf.h: csf_encounters) ----------------------------------
    def encounters(self, first=None, count=None, radius=0.5, d_event=None, ttc_event=None, per_sample=True):
        """closest approach and time to collision of every road user (csf.h: csf_encounters; every road user a disc of `radius`):
        samples [first, first + count) of the recording (record / enable_history), or - first=None - the current state.  Returns
        an Encounters: d_min, d_with, ttc_min, ttc_with [count, n] (None without per_sample), run_* [n] over the window with the
        sample of each, and - with d_event or ttc_event - events, the pairs (sample, i < j) under a threshold, sorted.  Events
        are fetched with a guessed capacity; when more were found, one second call with the exact capacity."""
        first, count = _encounter_args("encounters", first, count, radius, d_event, ttc_event)
        n = self.n
        want = _events_wanted(d_event, ttc_event)
        cap = min(max(64, count * n), 1 << 16) if want else 0
        pack = self._measure(lambda caps: _EncounterPack([(n, count)], per_sample, caps),
                             lambda p: self._lib.csf_encounters(self._h, first, count, float(radius), float(d_event or 0.0), float(ttc_event or 0.0), p.outs),
                             cap, want)
        return pack.result(0, radius, want)

    @staticmethod
    def batch_encounters(engines, n_last, radius=0.5, d_event=None, ttc_event=None, per_sample=True):
        """encounters() over the last n_last samples of every recording member of a batch (the engines in join order), all members
        in the same two launches with one transfer and one wait (csf.h: csf_batch_encounters): a list with an Encounters per
        member, None for members that do not record"""
        n_last = _encounter_args("batch_encounters", 0, n_last, radius, d_event, ttc_event)[1]
        engines, arr = Engine._batch_array(engines, "batch_encounters")
        want = _events_wanted(d_event, ttc_event)
        shapes = [(e.n, n_last) for e in engines]
        caps = [min(max(64, n_last * n), 1 << 16) if want else 0 for n, _ in shapes]
        return Engine._batch_measure("csf_batch_encounters", engines, arr, lambda caps: _EncounterPack(shapes, per_sample, caps),
                                     lambda p: (n_last, float(radius), float(d_event or 0.0), float(ttc_event or 0.0), p.outs),
                                     caps, want, lambda p, i, e: p.result(i, radius, want))

    def encounter_launches(self):
        """launches of encounters / batch_encounters so far: two per call (csf.h: csf_encounter_launches)"""
        return self._launches("csf_encounter_launches")

    # -- post-encroachment time: path crossings of a recording (include/csf.h: csf_post_encroachment) -------------------------
    def _period(self):
        return None if self._rec_stride is None else self._rec_stride * float(self.params.t_s)

    def post_encroachment(self, first, count, pet_event=None, per_segment=True):
        """who crossed whose path, where, and how long after the other had passed (csf.h: csf_post_encroachment): the paths of
        all road users over samples [first, first + count) of the recording (record / enable_history).  Returns a
        PostEncroachment: seg_pet, seg_with, seg_t_own, seg_t_with [count - 1, n] (None without per_segment), run_* [n], and - with
        pet_event, in samples, +inf for every crossing - events, the crossings (i < j) under it, sorted by (i, j, k, l).  Times are
        in samples from `first`; in_seconds() scales them.  Events are fetched with a guessed capacity; when more were found,
        one second call with the exact capacity."""
        first, count = _pet_args("post_encroachment", first, count, pet_event)
        n = self.n
        want = pet_event is not None and pet_event > 0
        cap = _pet_capacity_guess(max(count - 1, 0) * n) if want else 0
        pack = self._measure(lambda caps: _PetPack([(n, count)], per_segment, caps),
                             lambda p: self._lib.csf_post_encroachment(self._h, first, count, float(pet_event or 0.0), p.outs), cap, want)
        return pack.result(0, want, self._period())

    @staticmethod
    def batch_post_encroachment(engines, n_last, pet_event=None, per_segment=True):
        """post_encroachment() over the last n_last samples of every recording member of a batch (the engines in join order), all
        members in the same two launches with one transfer and one wait (csf.h: csf_batch_post_encroachment): a list with a
        PostEncroachment per member, None for members that do not record"""
        n_last = _pet_args("batch_post_encroachment", 0, n_last, pet_event)[1]
        engines, arr = Engine._batch_array(engines, "batch_post_encroachment")
        want = pet_event is not None and pet_event > 0
        shapes = [(e.n, n_last) for e in engines]
        caps = [_pet_capacity_guess(max(n_last - 1, 0) * n) if want else 0 for n, _ in shapes]
        return Engine._batch_measure("csf_batch_post_encroachment", engines, arr, lambda caps: _PetPack(shapes, per_segment, caps),
                                     lambda p: (n_last, float(pet_event or 0.0), p.outs), caps, want, lambda p, i, e: p.result(i, want, e._period()))

    def pet_launches(self):
        """launches of post_encroachment / batch_post_encroachment so far: two per call (csf.h: csf_pet_launches)"""
        return self._launches("csf_pet_launches")

    # -- following and passing: gaps, overtakings and meetings of a recording (include/csf.h: csf_passing) --------------------
    def passing(self, first, count, band=0.75, lat_max=3.0, lat_event=None, per_station=True):
        """who rode behind whom, at what gap and headway, and who overtook or met whom, when and at what lateral clearance (csf.h:
        csf_passing), over samples [first, first + count) of the recording (record / enable_history).  band: half the width in metres
        of the corridor ahead in which a leader is looked for; lat_max: the largest clearance at which a passing counts.  Returns
        a Passing: per station gap, gap_with, thw [count - 1, n], per interval made_* and by_* [count - 2, n] (None without
        per_station), run_* [n], and - with lat_event, in metres, +inf for every passing - events, the ordered passings (i passes
        j) under it, sorted by (i, j, k).  Times are in samples; in_seconds() scales them.  Events are fetched with a guessed
        capacity; when more were found, one second call with the exact capacity."""
        first, count = _passing_args("passing", first, count, band, lat_max, lat_event)
        n = self.n
        want = lat_event is not None and lat_event > 0
        cap = _passing_capacity_guess(max(count - 1, 0) * n) if want else 0
        pack = self._measure(lambda caps: _PassingPack([(n, count)], per_station, caps),
                             lambda p: self._lib.csf_passing(self._h, first, count, float(band), float(lat_max), float(lat_event or 0.0), p.outs), cap, want)
        return pack.result(0, want, self._period())

    @staticmethod
    def batch_passing(engines, n_last, band=0.75, lat_max=3.0, lat_event=None, per_station=True):
        """passing() over the last n_last samples of every recording member of a batch (the engines in join order), all members in
        the same two launches with one transfer and one wait (csf.h: csf_batch_passing): a list with a Passing per member, None
        for members that do not record"""
        n_last = _passing_args("batch_passing", 0, n_last, band, lat_max, lat_event)[1]
        engines, arr = Engine._batch_array(engines, "batch_passing")
        want = lat_event is not None and lat_event > 0
        shapes = [(e.n, n_last) for e in engines]
        caps = [_passing_capacity_guess(max(n_last - 1, 0) * n) if want else 0 for n, _ in shapes]
        return Engine._batch_measure("csf_batch_passing", engines, arr, lambda caps: _PassingPack(shapes, per_station, caps),
                                     lambda p: (n_last, float(band), float(lat_max), float(lat_event or 0.0), p.outs),
                                     caps, want, lambda p, i, e: p.result(i, want, e._period()))

    def passing_launches(self):
        """launches of passing / batch_passing so far: two per call (csf.h: csf_passing_launches)"""
        return self._launches("csf_passing_launches")

    # -- flow: crossings of counting lines, occupancy of areas and of a grid (include/csf.h: csf_flow) ------------------------
    def flow(self, first, count, lines=None, areas=None, grid=None, events=False):
        """how many road users crossed which counting line, in which direction and at what speed, how many were inside which
        area at every sample and how far they rode there, and where on a grid they spent their samples (csf.h: csf_flow), over
        samples [first, first + count) of the recording (record / enable_history).  lines [L, 4] = ax, ay, bx, by; areas [R, 5] =
        ax, ay, bx, by, half_width (an oriented rectangle around the centre line A -> B); grid = (x0, y0, h, nx, ny).  Returns a
        Flow; with events=True it carries every crossing, sorted by (i, l, k).  Events are fetched with a guessed capacity; when
        more were found, one second call with the exact capacity."""
        first, count = _flow_args("flow", first, count)
        lines, areas, grid = _flow_layout("flow", lines, areas, grid)
        n = self.n
        cap = _flow_capacity_guess(max(count - 1, 0) * n, lines.shape[0]) if events else 0
        pack = self._measure(lambda caps: _FlowPack([(n, count)], lines, areas, grid, caps),
                             lambda p: self._lib.csf_flow(self._h, first, count, C.byref(p.layout), p.outs), cap, events)
        return pack.result(0, bool(events), self._period())

    @staticmethod
    def batch_flow(engines, n_last, lines=None, areas=None, grid=None, events=False):
        """flow() over the last n_last samples of every recording member of a batch (the engines in join order), all members in
        the same two launches with one transfer and one wait (csf.h: csf_batch_flow): a list with a Flow per member, None for
        members that do not record"""
        n_last = _flow_args("batch_flow", 0, n_last)[1]
        lines, areas, grid = _flow_layout("batch_flow", lines, areas, grid)
        engines, arr = Engine._batch_array(engines, "batch_flow")
        if grid and len(engines) * grid[3] * grid[4] > 1 << 24:
            raise ValueError(f"batch_flow: {len(engines)} members x {grid[3]} x {grid[4]} grid cells (at most 2^24)")
        shapes = [(e.n, n_last) for e in engines]
        caps = [_flow_capacity_guess(max(n_last - 1, 0) * n, lines.shape[0]) if events else 0 for n, _ in shapes]
        return Engine._batch_measure("csf_batch_flow", engines, arr, lambda caps: _FlowPack(shapes, lines, areas, grid, caps),
                                     lambda p: (n_last, C.byref(p.layout), p.outs), caps, events, lambda p, i, e: p.result(i, bool(events), e._period()))

    def flow_launches(self):
        """launches of flow / batch_flow so far: two per call (csf.h: csf_flow_launches)"""
        return self._launches("csf_flow_launches")

    # -- road clearance: edge distances and edge crossings of a recording (include/csf.h: csf_clearance) ----------------------
    def clearance(self, first, count, road, d_event=0.0, events=False, per_sample=True):
        """how close to the edges of a road every road user came, where across the width of the path it rode and which edges it
        crossed (csf.h: csf_clearance), over samples [first, first + count) of the recording (record / enable_history).  road is a
        list of RoadEdge / RoadSegment / RoadSegmentCollection objects or an (offsets, xy) pair as set_road takes it - given to
        the call in fp64, not taken from the engine's own road.  d_event: a sample with d below it counts as near.  Returns a
        Clearance; with events=True it carries every crossing, sorted by (i, k, edge, seg).  Events are fetched with a guessed
        capacity; when more were found, one second call with the exact capacity."""
        first, count = _flow_args("clearance", first, count)
        off, xy = _clearance_road("clearance", road)
        d_event = _clearance_d_event("clearance", d_event)
        n = self.n
        cap = _clearance_capacity_guess(max(count - 1, 0) * n) if events else 0
        pack = self._measure(lambda caps: _ClearancePack([(n, count)], off, xy, caps, bool(per_sample)),
                             lambda p: self._lib.csf_clearance(self._h, first, count, C.byref(p.road), d_event, p.outs), cap, events)
        return pack.result(0, bool(events), self._period(), d_event)

    @staticmethod
    def batch_clearance(engines, n_last, road, d_event=0.0, events=False, per_sample=True):
        """clearance() over the last n_last samples of every recording member of a batch (the engines in join order) at one road,
        all members in the same three launches with one transfer and one wait (csf.h: csf_batch_clearance): a list with a
        Clearance per member, None for members that do not record"""
        n_last = _flow_args("batch_clearance", 0, n_last)[1]
        off, xy = _clearance_road("batch_clearance", road)
        d_event = _clearance_d_event("batch_clearance", d_event)
        engines, arr = Engine._batch_array(engines, "batch_clearance")
        shapes = [(e.n, n_last) for e in engines]
        caps = [_clearance_capacity_guess(max(n_last - 1, 0) * n) if events else 0 for n, _ in shapes]
        return Engine._batch_measure("csf_batch_clearance", engines, arr, lambda caps: _ClearancePack(shapes, off, xy, caps, bool(per_sample)),
                                     lambda p: (n_last, C.byref(p.road), d_event, p.outs),
                                     caps, events, lambda p, i, e: p.result(i, bool(events), e._period(), d_event))

    def clearance_launches(self):
        """launches of clearance / batch_clearance so far: three per call (csf.h: csf_clearance_launches)"""
        return self._launches("csf_clearance_launches")

    # -- body encounters: gaps and time to contact between the outlines (include/csf.h: csf_body_encounters) ------------------
    def body_encounters(self, first=None, count=None, extents=None, gap_event=None, ttc_event=None, per_sample=True):
        """the free gap and the time to contact between the road users' outlines (csf.h: csf_body_encounters; every road user an
        oriented rectangle, `extents` one (front, rear, half_width) for everybody or an [n, 3] array): samples [first, first +
        count) of the recording (record / enable_history), or - first=None - the current state.  Returns a BodyEncounters:
        gap_min, gap_with, ttc_min, ttc_with [count, n] (None without per_sample), run_* [n] over the window with the sample of
        each, overlap_n [n], and - with gap_event (>= 0; 0 lists exactly the collisions) or ttc_event - events, the pairs (sample,
        i < j) with gap <= gap_event or ttc < ttc_event, sorted.  Events are fetched with a guessed capacity; when more were
        found, one second call with the exact capacity."""
        first, count = _encounter_args("body_encounters", first, count, 0.0, None, None)
        ge, te = _body_thresholds("body_encounters", gap_event, ttc_event)
        n = self.n
        ext = _body_extents("body_encounters", extents, n)
        want = _body_events_wanted(gap_event, ttc_event)
        cap = min(max(64, count * n), 1 << 16) if want else 0
        pack = self._measure(lambda caps: _BodyPack([(n, count)], per_sample, caps),
                             lambda p: self._lib.csf_body_encounters(self._h, first, count, _ptr(ext), ge, te, p.outs), cap, want)
        return pack.result(0, ext, want)

    @staticmethod
    def batch_body_encounters(engines, n_last, extents=None, gap_event=None, ttc_event=None, per_sample=True):
        """body_encounters() over the last n_last samples of every recording member of a batch (the engines in join order), all
        members in the same two launches with one transfer and one wait (csf.h: csf_batch_body_encounters).  extents: one (front,
        rear, half_width) for everybody, or a list with a triple or an [n, 3] array per member.  A list with a BodyEncounters per
        member, None for members that do not record"""
        n_last = _encounter_args("batch_body_encounters", 0, n_last, 0.0, None, None)[1]
        ge, te = _body_thresholds("batch_body_encounters", gap_event, ttc_event)
        engines, arr = Engine._batch_array(engines, "batch_body_encounters")
        shapes = [(e.n, n_last) for e in engines]
        exts = _batch_body_extents("batch_body_encounters", extents, [n for n, _ in shapes])
        ptrs = (C.c_void_p * len(engines))(*[a.ctypes.data for a in exts])
        want = _body_events_wanted(gap_event, ttc_event)
        caps = [min(max(64, n_last * n), 1 << 16) if want else 0 for n, _ in shapes]
        return Engine._batch_measure("csf_batch_body_encounters", engines, arr, lambda caps: _BodyPack(shapes, per_sample, caps),
                                     lambda p: (n_last, ptrs, ge, te, p.outs), caps, want, lambda p, i, e: p.result(i, exts[i], want))

    def body_encounter_launches(self):
        """launches of body_encounters / batch_body_encounters so far: two per call (csf.h: csf_body_encounter_launches)"""
        return self._launches("csf_body_encounter_launches")

    def untracked(self):
        """get_untracked_foes() (intersection.py:690-745): bool [n, n], row = source, column = receiver"""
        n = self.n
        out = np.zeros((n, n), dtype=np.uint8)
        self._ck(self._lib.csf_untracked(self._h, _ptr(out)))
        return out.astype(bool)

    def update_destination(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        self._ck(self._lib.csf_update_destination(self._h, idx.size, _ptr(idx)))

    def update_nav_state(self, idx, stop=None):
        """(vd, ddest) of Vehicle.updateNavState(stop) for the listed agents; stop None reads the queue's stop flags"""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        vd = np.zeros(idx.size)
        dd = np.zeros(idx.size)
        st = None if stop is None else np.ascontiguousarray(np.broadcast_to(np.asarray(stop, dtype=np.int32), idx.shape))
        self._ck(self._lib.csf_update_nav_state(self._h, idx.size, _ptr(idx), None if st is None else _ptr(st), _ptr(vd), _ptr(dd)))
        return vd, dd

    def set_dest_pointer(self, idx, ptr):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        ptr = np.ascontiguousarray(np.broadcast_to(np.asarray(ptr, dtype=np.int32), idx.shape))
        self._ck(self._lib.csf_set_dest_pointer(self._h, idx.size, _ptr(idx), _ptr(ptr)))

    # -- sharding ---------------------------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        lib = _ffi.load()
        buf = (C.c_uint8 * _ffi.UNIQUE_ID_BYTES)()
        rc = lib.csf_comm_unique_id(buf)
        if rc != 0:
            raise EngineError(f"[{rc}] " + lib.csf_last_error(None).decode())
        return bytes(buf)

    def comm_init(self, unique_id, rank, world):
        if unique_id is None:
            self._ck(self._lib.csf_comm_init(self._h, None, int(rank), int(world)))
            return
        buf = (C.c_uint8 * _ffi.UNIQUE_ID_BYTES).from_buffer_copy(bytes(unique_id))
        self._ck(self._lib.csf_comm_init(self._h, buf, int(rank), int(world)))

    @staticmethod
    def _group_call(symbol, engines, arr, *args, every_message=False):
        """an entry point that takes an array of handles; a refusal raises with the members' messages - every member's, or
        (batches) the distinct non-empty ones"""
        lib = _ffi.load()
        rc = getattr(lib, symbol)(arr, len(engines), *args)
        if rc != 0:
            msgs = [lib.csf_last_error(e._h).decode() for e in engines]
            raise EngineError(f"[{rc}] " + "; ".join(msgs if every_message else dict.fromkeys(m for m in msgs if m)))

    @staticmethod
    def loopback_group(engines):
        """One-device rehearsal of the sharded path (include/csf.h: csf_comm_init_loopback): the engines, all holding the
        same population, become ranks 0 .. len-1; step them together with Engine.step_group."""
        arr = (C.c_void_p * len(engines))(*[e._h for e in engines])
        Engine._group_call("csf_comm_init_loopback", engines, arr, every_message=True)

    @staticmethod
    def step_group(engines, n_ticks=1, sync=False):
        arr = (C.c_void_p * len(engines))(*[e._h for e in engines])
        Engine._group_call("csf_step_group", engines, arr, int(n_ticks), every_message=True)
        if sync:
            engines[0].sync()

    # -- batches of independent scenes (include/csf.h: csf_batch_join) ------------------------------------------------
    @staticmethod
    def _batch_array(engines, what):
        engines = list(engines)
        if not engines:
            raise ValueError(f"{what}: no engines")
        for e in engines:
            if not isinstance(e, Engine):
                raise TypeError(f"{what}: every member must be an Engine")
            if not e._h:
                raise ValueError(f"{what}: an engine is closed")
        if len({id(e) for e in engines}) != len(engines):
            raise ValueError(f"{what}: an engine is listed twice")
        return engines, (C.c_void_p * len(engines))(*[e._h for e in engines])

    @staticmethod
    def batch_join(engines):
        """The engines - independent scenes on one device - become one batch: Engine.step_batch steps them together, every
        member the one-wave tick takes in one launch per vehicle class.  Engine.batch_leave (or closing a member) dissolves it."""
        engines, arr = Engine._batch_array(engines, "batch_join")
        Engine._group_call("csf_batch_join", engines, arr)

    @staticmethod
    def batch_leave(engines):
        engines, arr = Engine._batch_array(engines, "batch_leave")
        Engine._group_call("csf_batch_leave", engines, arr)

    @staticmethod
    def step_batch(engines, n_ticks=1, sync=False):
        """csf_step_batch: every member of the batch (the engines in join order) by n_ticks, bit for bit as Engine.step on each."""
        if int(n_ticks) != n_ticks or n_ticks < 0:
            raise ValueError("step_batch: n_ticks must be an integer >= 0")
        engines, arr = Engine._batch_array(engines, "step_batch")
        Engine._group_call("csf_step_batch", engines, arr, int(n_ticks))
        if sync:
            engines[0].sync()

    @staticmethod
    def step_batch_into(engines, n_ticks, outs):
        """step_batch, then every member's read-back straight into the caller's arrays (csf_step_batch_get_tick): outs[i] is
        (s [n, n_states] float64, ptr [n] int32, zn [n, 3] of one byte each, fx [n] float64, fy [n] float64) for member i, C-contiguous;
        any of them may be None.  Returns the members' tick counts."""
        if int(n_ticks) != n_ticks or n_ticks < 0:
            raise ValueError("step_batch_into: n_ticks must be an integer >= 0")
        engines, arr = Engine._batch_array(engines, "step_batch_into")
        outs = list(outs)
        if len(outs) != len(engines):
            raise ValueError("step_batch_into: one output tuple per engine")
        tout = (_ffi.TickOut * len(engines))()
        ticks = (C.c_int64 * len(engines))()
        for i, (e, o) in enumerate(zip(engines, outs)):
            t = tout[i]
            t.s_out, t.dest_ptr, t.znav, t.Fx, t.Fy = e._readback_ptrs("step_batch_into", (tuple(o) + (None,) * 5)[:5])
            t.tick = C.cast(C.byref(ticks, i * C.sizeof(C.c_int64)), C.POINTER(C.c_int64))
        Engine._group_call("csf_step_batch_get_tick", engines, arr, int(n_ticks), tout)
        return list(ticks)

    def batch_ticks(self):
        """ticks this engine has run inside a batched launch (csf.h: csf_batch_ticks)"""
        n = C.c_int64(0)
        self._ck(self._lib.csf_batch_ticks(self._h, C.byref(n)))
        return n.value

    def batch_mid_ticks(self):
        """ticks this engine has run inside a batched one-launch tick of mid-size members (csf.h: csf_batch_mid_ticks)"""
        n = C.c_int64(0)
        self._ck(self._lib.csf_batch_mid_ticks(self._h, C.byref(n)))
        return n.value

    def batch_launches(self):
        """launches and copies enqueued for the batched members of this engine's batch since the join (csf.h: csf_batch_launches)"""
        n = C.c_int64(0)
        self._ck(self._lib.csf_batch_launches(self._h, C.byref(n)))
        return n.value

    def shard_range(self):
        lo, hi = C.c_int64(0), C.c_int64(0)
        self._ck(self._lib.csf_shard_range(self._h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def far_radius(self):
        """Radius (m) beyond which batches of sources are skipped (inf: every pair is evaluated); include/csf.h."""
        r = C.c_double(0)
        self._ck(self._lib.csf_far_radius(self._h, C.byref(r)))
        return r.value

    # -- measurement ------------------------------------------------------------------------
    def profile(self, every=1):
        """HIP events around the pair kernel on every `every`-th tick (0 / False: off)."""
        self._ck(self._lib.csf_profile_enable(self._h, int(every)))

    def profile_read(self):
        a, b, n = C.c_double(0), C.c_double(0), C.c_int64(0)
        self._ck(self._lib.csf_profile_read(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def profile_kernels(self):
        """{"pair" | "road" | "agent" | "gather": (accumulated ms, launches)} over the sampled ticks; resets the sums.
        The pair kernel is timed on every sampled tick, the others on every 8th of them."""
        ms = (C.c_double * 4)()
        cnt = (C.c_int64 * 4)()
        self._ck(self._lib.csf_profile_kernels(self._h, ms, cnt))
        return {k: (ms[i], cnt[i]) for i, k in enumerate(("pair", "road", "agent", "gather"))}

    def profile_samples(self, capacity=65536, kernel="pair"):
        """microseconds of every sampled launch of `kernel` (pair, road, agent, gather) since the last reset (does not reset)"""
        out = np.zeros(int(capacity))
        n = C.c_int64(0)
        which = {"pair": 0, "road": 1, "agent": 2, "gather": 3}[kernel]
        self._ck(self._lib.csf_profile_samples_of(self._h, which, _ptr(out), int(capacity), C.byref(n)))
        return out[: n.value].copy()

    def profile_stats(self):
        """{kernel: {"median", "min", "max", "mean", "n"}} in microseconds over the sampled launches since the last reset -
        call BEFORE profile_kernels(), which resets.  Medians: one launch that met a clock step moves a mean of forty."""
        out = {}
        for k in ("pair", "road", "agent", "gather"):
            v = self.profile_samples(kernel=k)
            out[k] = None if v.size == 0 else {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
                                               "mean": float(v.mean()), "n": int(v.size)}
        return out

    def count_pairs(self, detail=False):
        """(pair evaluations of one launch on the current snapshot or None, name of the engine's pair kernel); with
        detail=True the first item is the dict {evaluated, tested, full_passes, partial_passes}"""
        n = (C.c_int64 * 4)()
        name = C.c_char_p()
        self._ck(self._lib.csf_count_pairs(self._h, n, C.byref(name)))
        kernel = (name.value or b"").decode()
        if n[0] < 0:
            return None, kernel
        if detail:
            return dict(evaluated=n[0], tested=n[1], full_passes=n[2], partial_passes=n[3]), kernel
        return n[0], kernel

    def near_dropped(self):
        """near / field-of-view-edge pairs the pair kernels could not hand to their exact path since creation (expected 0)"""
        n = C.c_int64(0)
        self._ck(self._lib.csf_near_dropped(self._h, C.byref(n)))
        return n.value

    def small_ticks(self):
        """ticks run by the one-wave kernel of small populations (csf.h: csf_small_ticks)"""
        n = C.c_int64(0)
        self._ck(self._lib.csf_small_ticks(self._h, C.byref(n)))
        return n.value

    def small_classes(self, on=True):
        """several parameter sets, several vehicle classes or an UncontrolledVehicle population of up to 32 road users take the one-wave
        tick and the batched launch too (csf.h: csf_small_classes; off by default, or what CSF_SMALL_CLASSES said at creation)"""
        self._ck(self._lib.csf_small_classes(self._h, 1 if on else 0))

    def mid_road(self, on=True):
        """the one-launch tick of a mid-size population sums the road term of a small road (no lattice, at most 2 048 padded vertices)
        itself, alone and as a batch member, instead of a road launch in front of every tick (csf.h: csf_mid_road; off by default, or
        what CSF_MID_ROAD said at creation)"""
        self._ck(self._lib.csf_mid_road(self._h, 1 if on else 0))

    def mid_road_ticks(self):
        """ticks whose road term was summed inside the one-launch tick (csf.h: csf_mid_road_ticks; mid_ticks counts them too)"""
        v = C.c_int64()
        self._ck(self._lib.csf_mid_road_ticks(self._h, C.byref(v)))
        return v.value

    def mid_classes(self, on=True):
        """a mid-size population (33 ... 1 024 road users) of several parameter sets, of several vehicle classes or holding
        UncontrolledVehicles - no BalancingRiderBicycle - takes ONE launch per tick, alone and as a batch member, instead of a pair launch
        and a per-agent launch per class (csf.h: csf_mid_classes; off by default, or what CSF_MID_CLASSES said at creation)"""
        self._ck(self._lib.csf_mid_classes(self._h, 1 if on else 0))

    def mid_classes_ticks(self):
        """ticks taken by the one-launch tick of mixed populations (csf.h: csf_mid_classes_ticks; mid_ticks counts them too)"""
        v = C.c_int64()
        self._ck(self._lib.csf_mid_classes_ticks(self._h, C.byref(v)))
        return v.value

    def mid_ticks(self):
        """ticks run as one launch each (csf_mid.hip: mid-size populations)"""
        v = C.c_int64()
        self._ck(self._lib.csf_mid_ticks(self._h, C.byref(v)))
        return v.value

    def wg_order_tables(self):
        """(groups, chunks, ordered, cost [chunks, groups] uint32, order [chunks, groups] int32 or None) of the last tick's pair
        launch (include/csf.h: csf_wg_order_tables); None where that launch kept no tables"""
        g, c, o = C.c_int64(), C.c_int32(), C.c_int32()
        self._ck(self._lib.csf_wg_order_tables(self._h, C.byref(g), C.byref(c), C.byref(o), None, None, 0))
        if g.value == 0:
            return None
        cost = np.zeros((c.value, g.value), dtype=np.uint32)
        order = np.full((c.value, g.value), -1, dtype=np.int32)
        self._ck(self._lib.csf_wg_order_tables(self._h, C.byref(g), C.byref(c), C.byref(o), _ptr(cost), _ptr(order), cost.size))
        return g.value, c.value, bool(o.value), cost, (order if o.value else None)

    def pair_shape(self):
        """what this engine's next pair launch takes (include/csf.h: csf_pair_shape_of), as a dict: family, field, rw, p2r, classify, binr,
        ord, reach, rpb, cw, per_group, threads, tile, grid_x, order_groups, name"""
        words = (C.c_int32 * _ffi.PAIR_SHAPE_IN)()
        self._ck(self._lib.csf_pair_shape_words(self._h, words))
        return _ffi.pair_shape_of(self._lib, words)

    def chase_ticks(self):
        """ticks whose per-agent launch ran beside the pair launch (include/csf.h: csf_chase_ticks)"""
        v = C.c_int64()
        self._ck(self._lib.csf_chase_ticks(self._h, C.byref(v)))
        return v.value

    def chase_calibration(self):
        """(1 side by side / -1 in turn / 0 not measured yet, [us per tick in turn, side by side]) - include/csf.h: csf_chase_calibration"""
        st = C.c_int32()
        us = np.zeros(2)
        self._ck(self._lib.csf_chase_calibration(self._h, C.byref(st), _ptr(us)))
        return st.value, us.tolist()

    def holes_taken(self):
        """arrivals that took the slot of a road user who had left from nearby (include/csf.h: csf_holes_taken)"""
        v = C.c_int64()
        self._ck(self._lib.csf_holes_taken(self._h, C.byref(v)))
        return v.value

    def comm_stream_order(self):
        """('main' | 'second', [us per tick in stream order, on the second stream]) - where a sharded engine issues its
        all-gather, and what its communicator measured when it chose (zeros: CSF_COMM_STREAM decided, or not sharded)"""
        second = C.c_int32(0)
        us = np.zeros(2)
        self._ck(self._lib.csf_comm_stream_order(self._h, C.byref(second), _ptr(us)))
        return ("second" if second.value else "main"), [float(us[0]), float(us[1])]

    def profile_gather(self):
        """all-gather milliseconds accumulated over the launches of the last profile_read() (sharded engines)"""
        g = C.c_double(0)
        self._ck(self._lib.csf_profile_gather(self._h, C.byref(g)))
        return g.value
