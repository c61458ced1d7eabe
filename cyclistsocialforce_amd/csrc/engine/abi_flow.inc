// engine/abi_flow.inc - C ABI: crossings of counting lines, occupancy of areas and of a grid, of a recording (csf_flow.hip).
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

extern "C++" {

constexpr int64_t FLOW_MAX_GRID = 1ll << 20;         // cells of a grid
constexpr int64_t FLOW_MAX_BATCH_GRID = 1ll << 24;   // members x cells of a batch: every member's grid is cleared and transferred

// what one engine is asked: samples [first, first + count) of its ring
struct FlowAsk {
    csf_engine *e;
    int64_t first, count;
    csf_flow_out *out;
};

// the refusals that depend on the layout every member shares ...
static int flow_layout_ok(csf_engine *e, const char *who, const csf_flow_layout *y) {
    if (!y) return fail(e, CSF_E_ARG, "%s: layout is NULL", who);
    if (y->n_lines < 0 || y->n_lines > FLOW_MAX) return fail(e, CSF_E_ARG, "%s: n_lines = %d (0 .. 64)", who, (int)y->n_lines);
    if (y->n_areas < 0 || y->n_areas > FLOW_MAX) return fail(e, CSF_E_ARG, "%s: n_areas = %d (0 .. 64)", who, (int)y->n_areas);
    if (y->n_lines > 0 && !y->lines) return fail(e, CSF_E_ARG, "%s: %d lines are given, but lines is NULL", who, (int)y->n_lines);
    if (y->n_areas > 0 && !y->areas) return fail(e, CSF_E_ARG, "%s: %d areas are given, but areas is NULL", who, (int)y->n_areas);
    auto degenerate = [](const double *q) {                    // a non-finite coordinate, or A == B (dd underflows to 0 with it)
        for (int v = 0; v < 4; v++)
            if (!std::isfinite(q[v])) return true;
        const double dx = q[2] - q[0], dy = q[3] - q[1];
        const double dd = dx * dx + dy * dy;
        return !(dd > 0.0) || !std::isfinite(dd);
    };
    for (int l = 0; l < y->n_lines; l++)
        if (degenerate(y->lines + 4 * l)) return fail(e, CSF_E_ARG, "%s: line %d has a non-finite coordinate or no length (dd == 0)", who, l);
    for (int r = 0; r < y->n_areas; r++) {
        if (degenerate(y->areas + 5 * r)) return fail(e, CSF_E_ARG, "%s: area %d has a non-finite coordinate or no length (dd == 0)", who, r);
        const double hw = y->areas[5 * r + 4];
        if (!(hw >= 0.0) || !std::isfinite(hw)) return fail(e, CSF_E_ARG, "%s: area %d: half_width = %g (finite, >= 0)", who, r, hw);
    }
    if (y->nx < 0 || y->ny < 0 || (y->nx == 0) != (y->ny == 0)) return fail(e, CSF_E_ARG, "%s: grid of %d x %d cells (both 0: no grid; else both > 0)", who, (int)y->nx, (int)y->ny);
    if ((int64_t)y->nx * y->ny > FLOW_MAX_GRID) return fail(e, CSF_E_ARG, "%s: grid of %d x %d cells (at most 2^20)", who, (int)y->nx, (int)y->ny);
    if (y->nx > 0) {
        if (!std::isfinite(y->h) || !(y->h > 0.0)) return fail(e, CSF_E_ARG, "%s: grid h = %g (finite, > 0)", who, y->h);
        if (!std::isfinite(y->x0) || !std::isfinite(y->y0)) return fail(e, CSF_E_ARG, "%s: grid origin (%g, %g) is not finite", who, y->x0, y->y0);
    }
    return CSF_OK;
}

// ... and on a member's outputs
static int flow_out_ok(csf_engine *e, const char *who, const csf_flow_out *o) {
    if (o->event_capacity < 0) return fail(e, CSF_E_ARG, "%s: event_capacity = %lld", who, (long long)o->event_capacity);
    if (o->event_capacity > 0 && !o->events) return fail(e, CSF_E_ARG, "%s: room for %lld events is given, but events is NULL", who, (long long)o->event_capacity);
    return CSF_OK;
}

static bool flow_event_less(const csf_flow_event &a, const csf_flow_event &b) {
    if (a.i != b.i) return a.i < b.i;
    if (a.l != b.l) return a.l < b.l;
    return a.k < b.k;
}

// a call that covers no sample of any road user: nobody crossed anything or was anywhere
static void flow_nothing(const FlowAsk &a, const csf_flow_layout &y) {
    csf_flow_out &o = *a.out;
    const size_t n = (size_t)a.e->d.n, c = (size_t)a.count, L = (size_t)y.n_lines, R = (size_t)y.n_areas;
    if (o.line_count && c > 1) std::fill_n(o.line_count, (c - 1) * L * 2, 0);
    if (o.occupancy) std::fill_n(o.occupancy, c * R, 0);
    if (o.grid_count) std::fill_n(o.grid_count, (size_t)y.nx * (size_t)y.ny, 0);
    if (o.cross_n) std::fill_n(o.cross_n, n * L * 2, 0);
    if (o.first_t) std::fill_n(o.first_t, n * L, (double)INFINITY);
    if (o.first_u) std::fill_n(o.first_u, n * L, (double)NAN);
    if (o.first_speed) std::fill_n(o.first_speed, n * L, (double)NAN);
    if (o.first_dir) std::fill_n(o.first_dir, n * L, 0);
    if (o.in_samples) std::fill_n(o.in_samples, n * R, 0);
    if (o.in_first) std::fill_n(o.in_first, n * R, -1);
    if (o.in_last) std::fill_n(o.in_last, n * R, -1);
    if (o.in_dist) std::fill_n(o.in_dist, n * R, 0.0);
}

// FLOW_LAUNCHES launches on `st` (the stream every engine asked about works on), one clearing of the counters and added counts, one
// copy, one wait, then the packed buffer -> the callers' arrays.  The asks and the layout have been checked.  ps: the time stamps of
// the first launch (csf_profile_enable), or NULL.
static int flow_run(csf_engine *e0, hipStream_t st, const FlowAsk *asks, size_t m, const csf_flow_layout &y, csf_engine::ProfSlot *ps) {
    for (size_t i = 0; i < m; i++) asks[i].out->n_events = 0, asks[i].out->n_outside = 0;
    const size_t L = (size_t)y.n_lines, R = (size_t)y.n_areas, G = (size_t)y.nx * (size_t)y.ny;
    // the packed output: the counters, every member's added counts (cleared with them), then every member's block and events
    size_t cleared = (2 * m * sizeof(unsigned long long) + 31) & ~(size_t)31, rest = 0, scratch = 0;
    int64_t gx = 1, gy = 1, plane = 0, max_n = 0;
    bool any = false;
    for (size_t i = 0; i < m; i++) {
        const int64_t n = asks[i].e->d.n, c = asks[i].count;
        if (n <= 0 || c <= 0) {
            flow_nothing(asks[i], y);
            continue;
        }
        any = true;
        max_n = std::max(max_n, n);
        if (n <= ENC_SMALL) {
            const int64_t spw = 256 / n;
            plane = std::max(plane, (c + spw - 1) / spw);
        } else {
            gx = std::max(gx, (n + 255) / 256);
            gy = std::max(gy, c);
        }
        cleared += flow_acc_bytes((size_t)c, L, R, G);
        rest += flow_block_bytes((size_t)n, L, R) + (((size_t)asks[i].out->event_capacity * sizeof(csf_flow_event) + 31) & ~(size_t)31);
        scratch += sizeof(FlowCell) * (size_t)(c * n);
    }
    if (!any) return CSF_OK;
    if (gx * gy < plane) {                                     // the packed members take the plane x * y (plane <= 65535 samples)
        if (gx == 1 && gy == 1) gx = plane;
        else gy = (plane + gx - 1) / gx;
    }
    const size_t total = cleared + rest;
    FlowScratch &g = e0->flow;
    HIPCHK(e0, g.desc.reserve(m, st, 16));
    HIPCHK(e0, g.layout.reserve(9 * FLOW_MAX, st));
    HIPCHK(e0, g.dev.reserve(total + scratch));
    HIPCHK(e0, g.host.reserve(total, st, 4096));
    if (L) std::memcpy(g.layout.p, y.lines, L * 4 * sizeof(double));
    if (R) std::memcpy(g.layout.p + 4 * FLOW_MAX, y.areas, R * 5 * sizeof(double));
    size_t acc_at = (2 * m * sizeof(unsigned long long) + 31) & ~(size_t)31, at = cleared, cell_at = total;
    for (size_t i = 0; i < m; i++) {
        const FlowAsk &a = asks[i];
        const Dev &d = a.e->d;
        FlowDesc r{};
        if (d.n > 0 && a.count > 0) {
            r.n = (int32_t)d.n, r.ns = d.ns, r.count = (int32_t)a.count;
            r.s = d.hist, r.cap = d.hist_cap, r.first = (int32_t)(a.first % d.hist_cap);
            r.acc_off = (int64_t)acc_at, acc_at += flow_acc_bytes((size_t)a.count, L, R, G);
            r.out_off = (int64_t)at, at += flow_block_bytes((size_t)d.n, L, R);
            r.ev_off = (int64_t)at, r.ev_cap = a.out->event_capacity;
            at += ((size_t)a.out->event_capacity * sizeof(csf_flow_event) + 31) & ~(size_t)31;
            r.cell_off = (int64_t)cell_at, cell_at += sizeof(FlowCell) * (size_t)(a.count * d.n);
        }
        g.desc.p[i] = r;
    }
    FlowArgs ka{};
    ka.desc = g.desc.dev, ka.out = g.dev.p, ka.count = (unsigned long long *)g.dev.p;
    ka.lines = g.layout.dev, ka.areas = g.layout.dev + 4 * FLOW_MAX;
    ka.x0 = y.x0, ka.y0 = y.y0, ka.h = y.h;
    ka.L = y.n_lines, ka.R = y.n_areas, ka.nx = y.nx, ka.ny = y.ny, ka.members = (int32_t)m;
    HIPCHK(e0, hipMemsetAsync(g.dev.p, 0, cleared, st));
    launch_flow(ka, dim3((unsigned)gx, (unsigned)gy, (unsigned)m), (int)m, (int)max_n, st, ps ? ps->ev[0] : nullptr, ps ? ps->ev[1] : nullptr);
    if (ps) ps->pair = true;
    e0->flow_launches += FLOW_LAUNCHES;
    HIPCHK(e0, hipGetLastError());
    HIPCHK(e0, hipMemcpyAsync(g.host.p, g.dev.p, total, hipMemcpyDeviceToHost, st));
    HIPCHK(e0, hipStreamSynchronize(st));
    const unsigned long long *found = (const unsigned long long *)g.host.p;
    for (size_t i = 0; i < m; i++) {
        const FlowDesc &r = g.desc.p[i];
        csf_flow_out &o = *asks[i].out;
        if (r.n <= 0) continue;
        const size_t n = (size_t)r.n, c = (size_t)r.count;
        const unsigned char *b = g.host.p + r.acc_off;
        auto take = [&](void *dst, size_t bytes) {
            if (dst) std::memcpy(dst, b, bytes);
            b += bytes;
        };
        take(o.line_count, (c - 1) * L * 2 * 4), take(o.occupancy, c * R * 4), take(o.grid_count, G * 4);
        b = g.host.p + r.out_off;
        take(o.first_t, n * L * 8), take(o.first_u, n * L * 8), take(o.first_speed, n * L * 8), take(o.in_dist, n * R * 8);
        take(o.cross_n, n * L * 2 * 4), take(o.first_dir, n * L * 4), take(o.in_samples, n * R * 4), take(o.in_first, n * R * 4), take(o.in_last, n * R * 4);
        o.n_events = (int64_t)found[i];
        o.n_outside = (int64_t)found[m + i];
        const int64_t stored = std::min(o.n_events, o.event_capacity);
        if (stored > 0) {
            std::memcpy(o.events, g.host.p + r.ev_off, (size_t)stored * sizeof(csf_flow_event));
            if (o.n_events <= o.event_capacity) std::sort(o.events, o.events + stored, flow_event_less);
        }
    }
    return CSF_OK;
}

}  // extern "C++"

int csf_flow(csf_engine *e, int64_t first_sample, int64_t n_samples, const csf_flow_layout *layout, csf_flow_out *out) try {
    static const char *const who = "csf_flow";
    if (!e) return CSF_E_ARG;
    if (!out) return fail(e, CSF_E_ARG, "%s: out is NULL", who);
    int rc = flow_layout_ok(e, who, layout);
    if (rc) return rc;
    if ((rc = flow_out_ok(e, who, out))) return rc;
    if (n_samples < 0 || n_samples > ENC_MAX_SAMPLES) return fail(e, CSF_E_ARG, "%s: n_samples = %lld (0 .. 65535)", who, (long long)n_samples);
    if (first_sample < 0)
        return fail(e, CSF_E_ARG, "%s: first_sample = %lld (the current state, -1, has no interval: a window of the state ring is needed)", who, (long long)first_sample);
    if ((rc = encounter_engine_ok(e, who))) return rc;
    if (!e->d.hist) return fail(e, CSF_E_STATE, "%s: no state ring (csf_record, csf_enable_history)", who);
    HIPCHK(e, hipSetDevice(e->device));
    if ((rc = upload_all(e))) return rc;
    if ((rc = csf_sync(e))) return rc;                         // both streams (the side-by-side tick), as the read-backs wait
    if ((rc = record_range(e, first_sample, n_samples))) return rc;
    if (e->d.n * n_samples > ENC_MAX_CELLS) return fail(e, CSF_E_ARG, "%s: more than 2^31 (sample, road user) cells in one call", who);
    out->first_sample = first_sample;
    FlowAsk ask{e, first_sample, n_samples, out};
    // csf_profile_enable: the first launch is timed like a tick's pair launch, as kernel 0
    csf_engine::ProfSlot *ps = nullptr;
    if (e->profile > 0 && e->d.n > 0 && n_samples >= 1) {
        if ((rc = prof_make_pool(e))) return rc;
        if (e->prof_issued - e->prof_resolved >= PROF_SLOTS && (rc = prof_resolve_one(e))) return rc;
        ps = &e->prof_pool[e->prof_issued % PROF_SLOTS];
        ps->pair = ps->road = ps->agent = ps->gather = false;
        e->prof_issued++;
    }
    return flow_run(e, e->main, &ask, 1, *layout, ps);
} catch (...) { return csf_caught(e); }

int csf_batch_flow(csf_engine *const *engines, int32_t count, int64_t n_last, const csf_flow_layout *layout, csf_flow_out *outs) try {
    static const char *const who = "csf_batch_flow";
    int rc = batch_check(engines, count);
    if (rc) return rc;
    csf_engine *e0 = engines[0];
    if (!outs) return fail(e0, CSF_E_ARG, "%s: outs is NULL", who);
    if ((rc = flow_layout_ok(e0, who, layout))) return rc;
    if (n_last < 0 || n_last > ENC_MAX_SAMPLES) return fail(e0, CSF_E_ARG, "%s: n_last = %lld (0 .. 65535)", who, (long long)n_last);
    if (count > 65535) return fail(e0, CSF_E_ARG, "%s: at most 65535 engines in one call (%d given)", who, (int)count);
    if ((int64_t)count * layout->nx * layout->ny > FLOW_MAX_BATCH_GRID)
        return fail(e0, CSF_E_ARG, "%s: %d members x %d x %d grid cells (at most 2^24)", who, (int)count, (int)layout->nx, (int)layout->ny);
    std::vector<FlowAsk> asks;
    asks.reserve((size_t)count);
    for (int32_t i = 0; i < count; i++) {        // every refusal before anything is written
        csf_engine *e = engines[i];
        if ((rc = flow_out_ok(e, who, &outs[i]))) return rc;
        if ((rc = encounter_engine_ok(e, who))) return rc;
        if (!e->d.hist) continue;
        int64_t first = 0;
        if (int rrc = record_last(e, i, n_last, &first)) return rrc;
        if (e->d.n * n_last > ENC_MAX_CELLS) return fail(e, CSF_E_ARG, "member %d: more than 2^31 (sample, road user) cells in one call", (int)i);
        asks.push_back(FlowAsk{e, first, n_last, &outs[i]});
    }
    for (int32_t i = 0; i < count; i++) outs[i].n_events = 0, outs[i].n_outside = 0, outs[i].first_sample = -2;
    for (const FlowAsk &a : asks) a.out->first_sample = a.first;
    HIPCHK(e0, hipSetDevice(e0->device));
    // (the members share one stream, and a member stepped in turn has joined its second stream back into it: stream order is enough)
    return flow_run(e0, e0->main, asks.data(), asks.size(), *layout, nullptr);
} catch (...) { return csf_caught((engines && count > 0 ? engines[0] : nullptr)); }

int csf_flow_launches(const csf_engine *e, int64_t *n_launches) try {
    if (!e || !n_launches) return CSF_E_ARG;
    *n_launches = e->flow_launches;
    return CSF_OK;
} catch (...) { return csf_caught(e); }
