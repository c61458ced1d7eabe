// engine/abi_flow.inc - C ABI: crossings of counting lines, occupancy of areas and of a grid, of a recording (csf_flow.hip).
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

extern "C++" {

constexpr int64_t FLOW_MAX_GRID = 1ll << 20;         // cells of a grid
constexpr int64_t FLOW_MAX_BATCH_GRID = 1ll << 24;   // members x cells of a batch: every member's grid is cleared and transferred

using FlowAsk = MeasureAsk<csf_flow_out>;

// the refusals that depend on the layout every member shares (a member's outputs: events_ok)
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
    const size_t L = (size_t)y.n_lines, R = (size_t)y.n_areas, G = (size_t)y.nx * (size_t)y.ny;
    // the packed output: the counters, every member's added counts (cleared with them), then every member's block and events
    const size_t counters = round32(2 * m * sizeof(unsigned long long));
    size_t cleared = counters, rest = 0, scratch = 0;
    MeasureGrid grid;
    for (size_t i = 0; i < m; i++) {
        asks[i].out->n_events = 0, asks[i].out->n_outside = 0;
        const int64_t n = asks[i].e->d.n, c = asks[i].count;
        if (n <= 0 || c <= 0) {
            flow_nothing(asks[i], y);
            continue;
        }
        grid.add(n, c);
        cleared += flow_acc_bytes((size_t)c, L, R, G);
        rest += flow_block_bytes((size_t)n, L, R) + events_bytes<csf_flow_event>(asks[i].out->event_capacity, true);
        scratch += sizeof(FlowCell) * (size_t)(c * n);
    }
    if (!grid.any()) return CSF_OK;
    const size_t total = cleared + rest;
    MeasureScratch<FlowDesc> &g = e0->flow.m;
    HostBuf<double> &layout = e0->flow.layout;
    HIPCHK(e0, layout.reserve(9 * FLOW_MAX, st));
    if (int rc = measure_reserve(e0, g, st, m, total + scratch, total)) return rc;
    if (L) std::memcpy(layout.p, y.lines, L * 4 * sizeof(double));
    if (R) std::memcpy(layout.p + 4 * FLOW_MAX, y.areas, R * 5 * sizeof(double));
    size_t acc_at = counters, at = cleared, cell_at = total;
    for (size_t i = 0; i < m; i++) {
        const FlowAsk &a = asks[i];
        const int64_t n = a.e->d.n;
        FlowDesc r{};
        if (n > 0 && a.count > 0) {
            desc_ring(r, a);
            r.acc_off = (int64_t)acc_at, acc_at += flow_acc_bytes((size_t)a.count, L, R, G);
            r.out_off = (int64_t)at, at += flow_block_bytes((size_t)n, L, R);
            desc_events<csf_flow_event>(r, at, a.out->event_capacity, true);
            r.cell_off = (int64_t)cell_at, cell_at += sizeof(FlowCell) * (size_t)(a.count * n);
        }
        g.desc.p[i] = r;
    }
    FlowArgs ka{};
    ka.desc = g.desc.dev, ka.out = g.dev.p, ka.count = (unsigned long long *)g.dev.p;
    ka.lines = layout.dev, ka.areas = layout.dev + 4 * FLOW_MAX;
    ka.x0 = y.x0, ka.y0 = y.y0, ka.h = y.h;
    ka.L = y.n_lines, ka.R = y.n_areas, ka.nx = y.nx, ka.ny = y.ny, ka.members = (int32_t)m;
    const dim3 dim = grid.dim(m);
    if (int rc = measure_launch(e0, g, st, cleared, total, ps, e0->flow_launches, FLOW_LAUNCHES, [&](hipEvent_t t0, hipEvent_t t1) {
            launch_flow(ka, dim, (int)m, (int)grid.max_n, st, t0, t1);
        }))
        return rc;
    const unsigned long long *found = (const unsigned long long *)g.host.p;
    for (size_t i = 0; i < m; i++) {
        const FlowDesc &r = g.desc.p[i];
        csf_flow_out &o = *asks[i].out;
        if (r.n <= 0) continue;
        const size_t n = (size_t)r.n, c = (size_t)r.count;
        Cursor b{g.host.p + r.acc_off};
        b.take(o.line_count, (c - 1) * L * 2 * 4), b.take(o.occupancy, c * R * 4), b.take(o.grid_count, G * 4);
        b = Cursor{g.host.p + r.out_off};
        b.take(o.first_t, n * L * 8), b.take(o.first_u, n * L * 8), b.take(o.first_speed, n * L * 8), b.take(o.in_dist, n * R * 8);
        b.take(o.cross_n, n * L * 2 * 4), b.take(o.first_dir, n * L * 4), b.take(o.in_samples, n * R * 4), b.take(o.in_first, n * R * 4), b.take(o.in_last, n * R * 4);
        o.n_outside = (int64_t)found[m + i];
        take_events(o, found[i], g.host.p + r.ev_off, flow_event_less);
    }
    return CSF_OK;
}

}  // extern "C++"

int csf_flow(csf_engine *e, int64_t first_sample, int64_t n_samples, const csf_flow_layout *layout, csf_flow_out *out) try {
    static const char *const who = "csf_flow";
    int rc = measure_open(e, who, first_sample, n_samples, out, "interval", [&] {
        const int lrc = flow_layout_ok(e, who, layout);
        return lrc ? lrc : events_ok(e, who, out);
    });
    if (rc) return rc;
    if ((rc = cells_ok(e, who, -1, e->d.n * n_samples))) return rc;
    out->first_sample = first_sample;
    FlowAsk ask{e, first_sample, n_samples, out};
    csf_engine::ProfSlot *ps = nullptr;
    if ((rc = prof_take(e, e->d.n > 0 && n_samples >= 1, &ps))) return rc;
    return flow_run(e, e->main, &ask, 1, *layout, ps);
} catch (...) { return csf_caught(e); }

int csf_batch_flow(csf_engine *const *engines, int32_t count, int64_t n_last, const csf_flow_layout *layout, csf_flow_out *outs) try {
    static const char *const who = "csf_batch_flow";
    int rc = batch_open(engines, count, who, outs);
    if (rc) return rc;
    csf_engine *e0 = engines[0];
    if ((rc = flow_layout_ok(e0, who, layout))) return rc;
    if ((rc = batch_sizes_ok(e0, who, n_last, count))) return rc;
    if ((int64_t)count * layout->nx * layout->ny > FLOW_MAX_BATCH_GRID)
        return fail(e0, CSF_E_ARG, "%s: %d members x %d x %d grid cells (at most 2^24)", who, (int)count, (int)layout->nx, (int)layout->ny);
    std::vector<FlowAsk> asks;
    rc = batch_members(engines, count, who, n_last, outs, asks,
                       [&](csf_engine *e, int32_t i) { return events_ok(e, who, &outs[i]); },
                       [&](csf_engine *e, int32_t i) { return cells_ok(e, who, i, e->d.n * n_last); });
    if (rc) return rc;
    for (int32_t i = 0; i < count; i++) outs[i].n_outside = 0;   // (a member's second counter, marked like the first)
    if ((rc = batch_device(e0))) return rc;
    return flow_run(e0, e0->main, asks.data(), asks.size(), *layout, nullptr);
} catch (...) { return csf_caught((engines && count > 0 ? engines[0] : nullptr)); }

int csf_flow_launches(const csf_engine *e, int64_t *n_launches) try {
    return measure_launches(e, n_launches, &csf_engine::flow_launches);
} catch (...) { return csf_caught(e); }
