// engine/abi_clearance.inc - C ABI: distances to, sides of and crossings of the edges of a road, of a recording (csf_clearance.hip).
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

extern "C++" {

constexpr int64_t CLR_MAX_TESTS = 1ll << 40;   // (sample, road user) cells x segments of a call: on the order of a second of device time

// what one engine is asked: samples [first, first + count) of its ring
struct ClrAsk {
    csf_engine *e;
    int64_t first, count;
    csf_clearance_out *out;
};

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
    if (o->event_capacity < 0) return fail(e, CSF_E_ARG, "%s: event_capacity = %lld", who, (long long)o->event_capacity);
    if (o->event_capacity > 0 && !o->events) return fail(e, CSF_E_ARG, "%s: room for %lld events is given, but events is NULL", who, (long long)o->event_capacity);
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
    for (size_t i = 0; i < m; i++) asks[i].out->n_events = 0;
    const int64_t chunks = (S + CLR_CHUNK - 1) / CLR_CHUNK;
    // the packed output: the counters, every member's added counts (cleared with them), every member's block and events, then
    // every member's per-cell arrays, and behind what is transferred the chunks' parts
    const size_t counters = (m * sizeof(unsigned long long) + 31) & ~(size_t)31;
    size_t cleared = counters, rest = 0, cell_bytes = 0, scratch = 0;
    int64_t gx = 1, gy = 1, plane = 0, max_n = 0, max_cells = 0;
    bool any = false, want_cells = false;
    for (size_t i = 0; i < m; i++) {
        const int64_t n = asks[i].e->d.n, c = asks[i].count;
        if (n <= 0 || c <= 0) {
            clearance_nothing(asks[i]);
            continue;
        }
        any = true;
        want_cells = want_cells || clearance_wants_cells(*asks[i].out);
        max_n = std::max(max_n, n), max_cells = std::max(max_cells, n * c);
        if (n <= ENC_SMALL) {
            const int64_t spw = 256 / n;
            plane = std::max(plane, (c + spw - 1) / spw);
        } else {
            gx = std::max(gx, (n + 255) / 256);
            gy = std::max(gy, c);
        }
        cleared += clr_acc_bytes((size_t)c);
        rest += clr_block_bytes((size_t)n) + (((size_t)asks[i].out->event_capacity * sizeof(csf_clearance_event) + 31) & ~(size_t)31);
        cell_bytes += clr_cell_bytes((size_t)(c * n));
        scratch += sizeof(ClrPart) * (size_t)(c * n) * (size_t)chunks;
    }
    if (!any) return CSF_OK;
    if (gx * gy < plane) {                                     // the packed members take the plane x * y (plane <= 65535 samples)
        if (gx == 1 && gy == 1) gx = plane;
        else gy = (plane + gx - 1) / gx;
    }
    const size_t small_total = cleared + rest, total = small_total + cell_bytes, moved = want_cells ? total : small_total;
    ClrScratch &g = e0->clearance;
    // the road as the kernels read it: double seg [S][4], int32 edge_of [S], first_g [n_edges]
    const size_t road_bytes = (size_t)S * 36 + (size_t)y.n_edges * 4;
    HIPCHK(e0, g.desc.reserve(m, st, 16));
    HIPCHK(e0, g.road_host.reserve(road_bytes, st, 4096));
    HIPCHK(e0, g.road.reserve(road_bytes));
    HIPCHK(e0, g.dev.reserve(total + scratch));
    HIPCHK(e0, g.host.reserve(moved, st, 4096));
    {
        double *seg = (double *)g.road_host.p;
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
        const Dev &d = a.e->d;
        ClrDesc r{};
        if (d.n > 0 && a.count > 0) {
            const size_t cells = (size_t)(a.count * d.n);
            r.n = (int32_t)d.n, r.ns = d.ns, r.count = (int32_t)a.count;
            r.s = d.hist, r.cap = d.hist_cap, r.first = (int32_t)(a.first % d.hist_cap);
            r.acc_off = (int64_t)acc_at, acc_at += clr_acc_bytes((size_t)a.count);
            r.out_off = (int64_t)at, at += clr_block_bytes((size_t)d.n);
            r.ev_off = (int64_t)at, r.ev_cap = a.out->event_capacity;
            at += ((size_t)a.out->event_capacity * sizeof(csf_clearance_event) + 31) & ~(size_t)31;
            r.cell_off = (int64_t)cell_at, cell_at += clr_cell_bytes(cells);
            r.part_off = (int64_t)part_at, part_at += sizeof(ClrPart) * cells * (size_t)chunks;
        }
        g.desc.p[i] = r;
    }
    ClrArgs ka{};
    ka.desc = g.desc.dev, ka.out = g.dev.p, ka.count = (unsigned long long *)g.dev.p;
    ka.seg = (const double *)g.road.p, ka.edge_of = (const int32_t *)(ka.seg + 4 * S), ka.first_g = ka.edge_of + S;
    ka.d_event = d_event, ka.S = (int32_t)S, ka.chunks = (int32_t)chunks, ka.members = (int32_t)m;
    HIPCHK(e0, hipMemcpyAsync(g.road.p, g.road_host.p, road_bytes, hipMemcpyHostToDevice, st));
    HIPCHK(e0, hipMemsetAsync(g.dev.p, 0, cleared, st));
    launch_clearance(ka, dim3((unsigned)gx, (unsigned)gy, (unsigned)(m * (size_t)chunks)), (int)m, max_cells, (int)max_n, st, ps ? ps->ev[0] : nullptr,
                     ps ? ps->ev[1] : nullptr);
    if (ps) ps->pair = true;
    e0->clearance_launches += CLEARANCE_LAUNCHES;
    HIPCHK(e0, hipGetLastError());
    HIPCHK(e0, hipMemcpyAsync(g.host.p, g.dev.p, moved, hipMemcpyDeviceToHost, st));
    HIPCHK(e0, hipStreamSynchronize(st));
    const unsigned long long *found = (const unsigned long long *)g.host.p;
    for (size_t i = 0; i < m; i++) {
        const ClrDesc &r = g.desc.p[i];
        csf_clearance_out &o = *asks[i].out;
        if (r.n <= 0) continue;
        const size_t n = (size_t)r.n, c = (size_t)r.count, cells = c * n, stations = (c - 1) * n;
        const unsigned char *b = g.host.p + r.acc_off;
        auto take = [&](void *dst, size_t bytes, size_t room) {   // `bytes` of the `room` the array has in the packed output
            if (dst && bytes) std::memcpy(dst, b, bytes);
            b += room;
        };
        take(o.near_count, c * 4, c * 4), take(o.cross_count, (c - 1) * 4, c * 4);
        b = g.host.p + r.out_off;
        take(o.d_min, n * 8, n * 8), take(o.left_min, n * 8, n * 8), take(o.right_min, n * 8, n * 8);
        for (int32_t *p : {o.d_min_k, o.d_min_edge, o.d_min_seg, o.left_min_k, o.right_min_k, o.near_samples, o.near_first, o.near_last, o.cross_n}) take(p, n * 4, n * 4);
        if (want_cells) {
            b = g.host.p + r.cell_off;
            take(o.d, cells * 8, cells * 8), take(o.t, cells * 8, cells * 8), take(o.left, stations * 8, cells * 8), take(o.right, stations * 8, cells * 8);
            take(o.edge, cells * 4, cells * 4), take(o.seg, cells * 4, cells * 4);
            take(o.left_edge, stations * 4, cells * 4), take(o.right_edge, stations * 4, cells * 4), take(o.cross, stations * 4, cells * 4);
        }
        o.n_events = (int64_t)found[i];
        const int64_t stored = std::min(o.n_events, o.event_capacity);
        if (stored > 0) {
            std::memcpy(o.events, g.host.p + r.ev_off, (size_t)stored * sizeof(csf_clearance_event));
            if (o.n_events <= o.event_capacity) std::sort(o.events, o.events + stored, clearance_event_less);
        }
    }
    return CSF_OK;
}

}  // extern "C++"

int csf_clearance(csf_engine *e, int64_t first_sample, int64_t n_samples, const csf_clearance_road *road, double d_event, csf_clearance_out *out) try {
    static const char *const who = "csf_clearance";
    if (!e) return CSF_E_ARG;
    if (!out) return fail(e, CSF_E_ARG, "%s: out is NULL", who);
    int64_t S = 0;
    int rc = clearance_road_ok(e, who, road, &S);
    if (rc) return rc;
    if ((rc = clearance_out_ok(e, who, d_event, out))) return rc;
    if (n_samples < 0 || n_samples > ENC_MAX_SAMPLES) return fail(e, CSF_E_ARG, "%s: n_samples = %lld (0 .. 65535)", who, (long long)n_samples);
    if (first_sample < 0)
        return fail(e, CSF_E_ARG, "%s: first_sample = %lld (the current state, -1, has no station: a window of the state ring is needed)", who, (long long)first_sample);
    if ((rc = encounter_engine_ok(e, who))) return rc;
    if (!e->d.hist) return fail(e, CSF_E_STATE, "%s: no state ring (csf_record, csf_enable_history)", who);
    HIPCHK(e, hipSetDevice(e->device));
    if ((rc = upload_all(e))) return rc;
    if ((rc = csf_sync(e))) return rc;                         // both streams (the side-by-side tick), as the read-backs wait
    if ((rc = record_range(e, first_sample, n_samples))) return rc;
    if (e->d.n * n_samples > ENC_MAX_CELLS) return fail(e, CSF_E_ARG, "%s: more than 2^31 (sample, road user) cells in one call", who);
    if (e->d.n * n_samples * S > CLR_MAX_TESTS) return fail(e, CSF_E_ARG, "%s: more than 2^40 (sample, road user) cells x segments in one call", who);
    out->first_sample = first_sample;
    ClrAsk ask{e, first_sample, n_samples, out};
    // csf_profile_enable: the first launch is timed like a tick's pair launch, as kernel 0
    csf_engine::ProfSlot *ps = nullptr;
    if (e->profile > 0 && e->d.n > 0 && n_samples >= 1) {
        if ((rc = prof_make_pool(e))) return rc;
        if (e->prof_issued - e->prof_resolved >= PROF_SLOTS && (rc = prof_resolve_one(e))) return rc;
        ps = &e->prof_pool[e->prof_issued % PROF_SLOTS];
        ps->pair = ps->road = ps->agent = ps->gather = false;
        e->prof_issued++;
    }
    return clearance_run(e, e->main, &ask, 1, *road, S, d_event, ps);
} catch (...) { return csf_caught(e); }

int csf_batch_clearance(csf_engine *const *engines, int32_t count, int64_t n_last, const csf_clearance_road *road, double d_event, csf_clearance_out *outs) try {
    static const char *const who = "csf_batch_clearance";
    int rc = batch_check(engines, count);
    if (rc) return rc;
    csf_engine *e0 = engines[0];
    if (!outs) return fail(e0, CSF_E_ARG, "%s: outs is NULL", who);
    int64_t S = 0;
    if ((rc = clearance_road_ok(e0, who, road, &S))) return rc;
    if (n_last < 0 || n_last > ENC_MAX_SAMPLES) return fail(e0, CSF_E_ARG, "%s: n_last = %lld (0 .. 65535)", who, (long long)n_last);
    const int64_t chunks = (S + CLR_CHUNK - 1) / CLR_CHUNK;
    if (count * chunks > 65535) return fail(e0, CSF_E_ARG, "%s: %d members x %lld chunks of %d segments (at most 65535)", who, (int)count, (long long)chunks, (int)CLR_CHUNK);
    std::vector<ClrAsk> asks;
    asks.reserve((size_t)count);
    int64_t cells = 0;
    for (int32_t i = 0; i < count; i++) {        // every refusal before anything is written
        csf_engine *e = engines[i];
        if ((rc = clearance_out_ok(e, who, d_event, &outs[i]))) return rc;
        if ((rc = encounter_engine_ok(e, who))) return rc;
        if (!e->d.hist) continue;
        int64_t first = 0;
        if (int rrc = record_last(e, i, n_last, &first)) return rrc;
        if (e->d.n * n_last > ENC_MAX_CELLS) return fail(e, CSF_E_ARG, "member %d: more than 2^31 (sample, road user) cells in one call", (int)i);
        cells += e->d.n * n_last;
        if (cells * S > CLR_MAX_TESTS) return fail(e, CSF_E_ARG, "%s: more than 2^40 (sample, road user) cells x segments in one call", who);
        asks.push_back(ClrAsk{e, first, n_last, &outs[i]});
    }
    for (int32_t i = 0; i < count; i++) outs[i].n_events = 0, outs[i].first_sample = -2;
    for (const ClrAsk &a : asks) a.out->first_sample = a.first;
    HIPCHK(e0, hipSetDevice(e0->device));
    // (the members share one stream, and a member stepped in turn has joined its second stream back into it: stream order is enough)
    return clearance_run(e0, e0->main, asks.data(), asks.size(), *road, S, d_event, nullptr);
} catch (...) { return csf_caught((engines && count > 0 ? engines[0] : nullptr)); }

int csf_clearance_launches(const csf_engine *e, int64_t *n_launches) try {
    if (!e || !n_launches) return CSF_E_ARG;
    *n_launches = e->clearance_launches;
    return CSF_OK;
} catch (...) { return csf_caught(e); }
