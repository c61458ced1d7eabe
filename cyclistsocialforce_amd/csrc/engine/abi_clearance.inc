// engine/abi_clearance.inc - C ABI: distances to, sides of and crossings of the edges of a road, of a recording (csf_clearance.hip).
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

extern "C++" {

constexpr int64_t CLR_MAX_TESTS = 1ll << 40;   // (sample, road user) cells x segments of a call: on the order of a second of device time

using ClrAsk = MeasureAsk<csf_clearance_out>;

// the refusals that depend on the road every member shares; *S: its segments
static int clearance_road_ok(csf_engine *e, const char *who, const csf_clearance_road *y, int64_t *S) {
    if (!y) return fail(e, CSF_E_ARG, "%s: road is NULL", who);
    if (y->n_edges < 1) return fail(e, CSF_E_ARG, "%s: n_edges = %d (at least 1)", who, (int)y->n_edges);
    if (!y->offsets || !y->xy) return fail(e, CSF_E_ARG, "%s: the road's offsets or xy is NULL", who);
    if (y->offsets[0] != 0) return fail(e, CSF_E_ARG, "%s: offsets[0] = %lld (0)", who, (long long)y->offsets[0]);
    int64_t segs = 0;
    for (int32_t k = 0; k < y->n_edges; k++) {
        const int64_t v = y->offsets[k + 1] - y->offsets[k];
        if (v < 2) return fail(e, CSF_E_ARG, "%s: edge %d has %lld vertices (at least 2; the offsets must rise)", who, (int)k, (long long)v);
        segs += v - 1;
        if (segs > CLR_MAX_SEGS) return fail(e, CSF_E_ARG, "%s: more than 2^20 segments", who);
    }
    for (int32_t k = 0; k < y->n_edges; k++)
        for (int64_t v = y->offsets[k]; v < y->offsets[k + 1]; v++) {
            const double *q = y->xy + 2 * v;
            if (!std::isfinite(q[0]) || !std::isfinite(q[1]))
                return fail(e, CSF_E_ARG, "%s: edge %d, vertex %lld has a non-finite coordinate", who, (int)k, (long long)(v - y->offsets[k]));
            if (v == y->offsets[k]) continue;
            const double dx = q[0] - q[-2], dy = q[1] - q[-1];
            const double dd = dx * dx + dy * dy;
            if (!(dd > 0.0) || !std::isfinite(dd))
                return fail(e, CSF_E_ARG, "%s: edge %d, segment %lld has no length or a non-finite one (dd == 0)", who, (int)k, (long long)(v - 1 - y->offsets[k]));
        }
    *S = segs;
    return CSF_OK;
}

// ... on the threshold, and on a member's outputs
static int clearance_out_ok(csf_engine *e, const char *who, double d_event, const csf_clearance_out *o) {
    if (!(d_event >= 0.0) || !std::isfinite(d_event)) return fail(e, CSF_E_ARG, "%s: d_event = %g (finite, >= 0)", who, d_event);
    return events_ok(e, who, o);
}

// ... and on the tests of a call: `cells` (sample, road user) cells against S segments
static int clearance_tests_ok(csf_engine *e, const char *who, int64_t cells, int64_t S) {
    if (cells * S > CLR_MAX_TESTS) return fail(e, CSF_E_ARG, "%s: more than 2^40 (sample, road user) cells x segments in one call", who);
    return CSF_OK;
}

static bool clearance_event_less(const csf_clearance_event &a, const csf_clearance_event &b) {
    if (a.i != b.i) return a.i < b.i;
    if (a.k != b.k) return a.k < b.k;
    if (a.edge != b.edge) return a.edge < b.edge;
    return a.seg < b.seg;
}

static bool clearance_wants_cells(const csf_clearance_out &o) {
    return o.d || o.edge || o.seg || o.t || o.left || o.right || o.left_edge || o.right_edge || o.cross;
}

// a call that covers no sample of any road user: nobody was anywhere
static void clearance_nothing(const ClrAsk &a) {
    csf_clearance_out &o = *a.out;
    const size_t n = (size_t)a.e->d.n, c = (size_t)a.count;
    for (double *p : {o.d_min, o.left_min, o.right_min})
        if (p) std::fill_n(p, n, (double)INFINITY);
    for (int32_t *p : {o.d_min_k, o.d_min_edge, o.d_min_seg, o.left_min_k, o.right_min_k, o.near_first, o.near_last})
        if (p) std::fill_n(p, n, -1);
    if (o.near_samples) std::fill_n(o.near_samples, n, 0);
    if (o.cross_n) std::fill_n(o.cross_n, n, 0);
    if (o.near_count) std::fill_n(o.near_count, c, 0);
    if (o.cross_count && c > 1) std::fill_n(o.cross_count, c - 1, 0);
}

// CLEARANCE_LAUNCHES launches on `st` (the stream every engine asked about works on), one upload of the road, one clearing of the
// counters and added counts, one copy, one wait, then the packed buffer -> the callers' arrays.  The asks and the road (S segments)
// have been checked.  ps: the time stamps of the first launch (csf_profile_enable), or NULL.
static int clearance_run(csf_engine *e0, hipStream_t st, const ClrAsk *asks, size_t m, const csf_clearance_road &y, int64_t S, double d_event,
                         csf_engine::ProfSlot *ps) {
    const int64_t chunks = (S + CLR_CHUNK - 1) / CLR_CHUNK;
    // the packed output: the counters, every member's added counts (cleared with them), every member's block and events, then
    // every member's per-cell arrays, and behind what is transferred the chunks' parts
    const size_t counters = round32(m * sizeof(unsigned long long));
    size_t cleared = counters, rest = 0, cell_bytes = 0, scratch = 0;
    MeasureGrid grid;
    int64_t max_cells = 0;
    bool want_cells = false;
    for (size_t i = 0; i < m; i++) {
        asks[i].out->n_events = 0;
        const int64_t n = asks[i].e->d.n, c = asks[i].count;
        if (n <= 0 || c <= 0) {
            clearance_nothing(asks[i]);
            continue;
        }
        want_cells = want_cells || clearance_wants_cells(*asks[i].out);
        max_cells = std::max(max_cells, n * c);
        grid.add(n, c);
        cleared += clr_acc_bytes((size_t)c);
        rest += clr_block_bytes((size_t)n) + events_bytes<csf_clearance_event>(asks[i].out->event_capacity, true);
        cell_bytes += clr_cell_bytes((size_t)(c * n));
        scratch += sizeof(ClrPart) * (size_t)(c * n) * (size_t)chunks;
    }
    if (!grid.any()) return CSF_OK;
    const size_t small_total = cleared + rest, total = small_total + cell_bytes, moved = want_cells ? total : small_total;
    MeasureScratch<ClrDesc> &g = e0->clearance.m;
    HostBuf<unsigned char, false> &road_host = e0->clearance.road_host;
    DevBuf<unsigned char> &road = e0->clearance.road;
    // the road as the kernels read it: double seg [S][4], int32 edge_of [S], first_g [n_edges]
    const size_t road_bytes = (size_t)S * 36 + (size_t)y.n_edges * 4;
    HIPCHK(e0, road_host.reserve(road_bytes, st, 4096));
    HIPCHK(e0, road.reserve(road_bytes));
    if (int rc = measure_reserve(e0, g, st, m, total + scratch, moved)) return rc;
    {
        double *seg = (double *)road_host.p;
        int32_t *edge_of = (int32_t *)(seg + 4 * S), *first_g = edge_of + S;
        int64_t at = 0;
        for (int32_t k = 0; k < y.n_edges; k++) {
            first_g[k] = (int32_t)at;
            for (int64_t v = y.offsets[k]; v + 1 < y.offsets[k + 1]; v++, at++) {
                std::memcpy(seg + 4 * at, y.xy + 2 * v, 4 * sizeof(double));
                edge_of[at] = k;
            }
        }
    }
    size_t acc_at = counters, at = cleared, cell_at = small_total, part_at = total;
    for (size_t i = 0; i < m; i++) {
        const ClrAsk &a = asks[i];
        const int64_t n = a.e->d.n;
        ClrDesc r{};
        if (n > 0 && a.count > 0) {
            const size_t cells = (size_t)(a.count * n);
            desc_ring(r, a);
            r.acc_off = (int64_t)acc_at, acc_at += clr_acc_bytes((size_t)a.count);
            r.out_off = (int64_t)at, at += clr_block_bytes((size_t)n);
            desc_events<csf_clearance_event>(r, at, a.out->event_capacity, true);
            r.cell_off = (int64_t)cell_at, cell_at += clr_cell_bytes(cells);
            r.part_off = (int64_t)part_at, part_at += sizeof(ClrPart) * cells * (size_t)chunks;
        }
        g.desc.p[i] = r;
    }
    ClrArgs ka{};
    ka.desc = g.desc.dev, ka.out = g.dev.p, ka.count = (unsigned long long *)g.dev.p;
    ka.seg = (const double *)road.p, ka.edge_of = (const int32_t *)(ka.seg + 4 * S), ka.first_g = ka.edge_of + S;
    ka.d_event = d_event, ka.S = (int32_t)S, ka.chunks = (int32_t)chunks, ka.members = (int32_t)m;
    HIPCHK(e0, hipMemcpyAsync(road.p, road_host.p, road_bytes, hipMemcpyHostToDevice, st));
    const dim3 dim = grid.dim(m * (size_t)chunks);
    if (int rc = measure_launch(e0, g, st, cleared, moved, ps, e0->clearance_launches, CLEARANCE_LAUNCHES, [&](hipEvent_t t0, hipEvent_t t1) {
            launch_clearance(ka, dim, (int)m, max_cells, (int)grid.max_n, st, t0, t1);
        }))
        return rc;
    const unsigned long long *found = (const unsigned long long *)g.host.p;
    for (size_t i = 0; i < m; i++) {
        const ClrDesc &r = g.desc.p[i];
        csf_clearance_out &o = *asks[i].out;
        if (r.n <= 0) continue;
        const size_t n = (size_t)r.n, c = (size_t)r.count, cells = c * n, stations = (c - 1) * n;
        Cursor b{g.host.p + r.acc_off};
        b.take(o.near_count, c * 4), b.take(o.cross_count, (c - 1) * 4, c * 4);
        b = Cursor{g.host.p + r.out_off};
        b.take(o.d_min, n * 8), b.take(o.left_min, n * 8), b.take(o.right_min, n * 8);
        for (int32_t *p : {o.d_min_k, o.d_min_edge, o.d_min_seg, o.left_min_k, o.right_min_k, o.near_samples, o.near_first, o.near_last, o.cross_n}) b.take(p, n * 4);
        if (want_cells) {
            b = Cursor{g.host.p + r.cell_off};
            b.take(o.d, cells * 8), b.take(o.t, cells * 8), b.take(o.left, stations * 8, cells * 8), b.take(o.right, stations * 8, cells * 8);
            b.take(o.edge, cells * 4), b.take(o.seg, cells * 4);
            b.take(o.left_edge, stations * 4, cells * 4), b.take(o.right_edge, stations * 4, cells * 4), b.take(o.cross, stations * 4, cells * 4);
        }
        take_events(o, found[i], g.host.p + r.ev_off, clearance_event_less);
    }
    return CSF_OK;
}

}  // extern "C++"

int csf_clearance(csf_engine *e, int64_t first_sample, int64_t n_samples, const csf_clearance_road *road, double d_event, csf_clearance_out *out) try {
    static const char *const who = "csf_clearance";
    int64_t S = 0;
    int rc = measure_open(e, who, first_sample, n_samples, out, "station", [&] {
        const int rrc = clearance_road_ok(e, who, road, &S);
        return rrc ? rrc : clearance_out_ok(e, who, d_event, out);
    });
    if (rc) return rc;
    if ((rc = cells_ok(e, who, -1, e->d.n * n_samples))) return rc;
    if ((rc = clearance_tests_ok(e, who, e->d.n * n_samples, S))) return rc;
    out->first_sample = first_sample;
    ClrAsk ask{e, first_sample, n_samples, out};
    csf_engine::ProfSlot *ps = nullptr;
    if ((rc = prof_take(e, e->d.n > 0 && n_samples >= 1, &ps))) return rc;
    return clearance_run(e, e->main, &ask, 1, *road, S, d_event, ps);
} catch (...) { return csf_caught(e); }

int csf_batch_clearance(csf_engine *const *engines, int32_t count, int64_t n_last, const csf_clearance_road *road, double d_event, csf_clearance_out *outs) try {
    static const char *const who = "csf_batch_clearance";
    int rc = batch_open(engines, count, who, outs);
    if (rc) return rc;
    csf_engine *e0 = engines[0];
    int64_t S = 0;
    if ((rc = clearance_road_ok(e0, who, road, &S))) return rc;
    if ((rc = batch_n_last_ok(e0, who, n_last))) return rc;
    const int64_t chunks = (S + CLR_CHUNK - 1) / CLR_CHUNK;    // (a member takes `chunks` of the grid's z)
    if (count * chunks > 65535) return fail(e0, CSF_E_ARG, "%s: %d members x %lld chunks of %d segments (at most 65535)", who, (int)count, (long long)chunks, (int)CLR_CHUNK);
    std::vector<ClrAsk> asks;
    int64_t cells = 0;                                         // (of the members so far: the tests of the call are limited, not a member's)
    rc = batch_members(engines, count, who, n_last, outs, asks,
                       [&](csf_engine *e, int32_t i) { return clearance_out_ok(e, who, d_event, &outs[i]); },
                       [&](csf_engine *e, int32_t i) {
                           const int crc = cells_ok(e, who, i, e->d.n * n_last);
                           return crc ? crc : clearance_tests_ok(e, who, cells += e->d.n * n_last, S);
                       });
    if (rc) return rc;
    if ((rc = batch_device(e0))) return rc;
    return clearance_run(e0, e0->main, asks.data(), asks.size(), *road, S, d_event, nullptr);
} catch (...) { return csf_caught((engines && count > 0 ? engines[0] : nullptr)); }

int csf_clearance_launches(const csf_engine *e, int64_t *n_launches) try {
    return measure_launches(e, n_launches, &csf_engine::clearance_launches);
} catch (...) { return csf_caught(e); }
