// engine/abi_passing.inc - C ABI: gaps to the leader, overtakings and meetings of a recording (csf_passing.hip).
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

extern "C++" {

using PassAsk = MeasureAsk<csf_passing_out>;

// the refusals that depend on the arguments every member shares, and on a member's outputs
static int passing_args_ok(csf_engine *e, const char *who, double band, double lat_max, double lat_event, const csf_passing_out *o) {
    if (!(band >= 0.0)) return fail(e, CSF_E_ARG, "%s: band = %g (>= 0; +inf takes every road user ahead)", who, band);
    if (!(lat_max > 0.0)) return fail(e, CSF_E_ARG, "%s: lat_max = %g (> 0; +inf takes every passing)", who, lat_max);
    if (std::isnan(lat_event) || lat_event == -INFINITY) return fail(e, CSF_E_ARG, "%s: lat_event = %g (a number; <= 0 switches events off, +inf takes every passing)", who, lat_event);
    return events_ok(e, who, o);
}

static bool passing_event_less(const csf_passing_event &a, const csf_passing_event &b) {
    if (a.i != b.i) return a.i < b.i;
    if (a.j != b.j) return a.j < b.j;
    return a.k < b.k;
}

// a call that covers no station: nobody followed or passed anybody
static void passing_nothing(const PassAsk &a) {
    csf_passing_out &o = *a.out;
    const int64_t n = a.e->d.n;
    for (int64_t u = 0; u < n; u++) {
        if (o.run_gap) o.run_gap[u] = INFINITY;
        if (o.run_thw) o.run_thw[u] = INFINITY;
        if (o.run_made_lat) o.run_made_lat[u] = INFINITY;
        if (o.run_by_lat) o.run_by_lat[u] = INFINITY;
        if (o.run_made_t) o.run_made_t[u] = NAN;
        if (o.run_by_t) o.run_by_t[u] = NAN;
        for (int32_t *p : {o.run_gap_with, o.run_gap_k, o.run_thw_with, o.run_thw_k, o.run_made_with, o.run_by_with})
            if (p) p[u] = -1;
        for (int32_t *p : {o.run_made_kind, o.run_by_kind})
            if (p) p[u] = 0;
        for (int32_t *p : {o.run_made, o.run_by})
            if (p) p[3 * u] = p[3 * u + 1] = p[3 * u + 2] = 0;
    }
}

// PASS_LAUNCHES launches on `st` (the stream every engine asked about works on), one copy, one wait, then the packed buffer -> the
// callers' arrays.  The asks have been checked.  ps: the time stamps of the first launch (csf_profile_enable), or NULL.
static int passing_run(csf_engine *e0, hipStream_t st, const PassAsk *asks, size_t m, double band, double lat_max, double lat_event,
                       csf_engine::ProfSlot *ps) {
    const size_t header = round32(m * sizeof(unsigned long long));
    size_t total = header, scratch = 0;                        // scratch: the chunks' results, device memory behind what is transferred
    MeasureGrid grid;
    for (size_t i = 0; i < m; i++) {
        asks[i].out->n_events = 0;
        const int64_t n = asks[i].e->d.n, st_n = asks[i].count - 1;      // st_n: stations of a road user
        if (n <= 0 || st_n <= 0) {
            passing_nothing(asks[i]);
            continue;
        }
        int32_t split = 1, chunk_tiles = 1;
        if (n > ENC_SMALL) enc_split(n, st_n, split, chunk_tiles);
        grid.add(n, st_n, split);
        scratch += pass_part_bytes((size_t)(st_n * n), (size_t)split);
        total += pass_block_bytes((size_t)(st_n * n), (size_t)((st_n - 1) * n), (size_t)n) + events_bytes<csf_passing_event>(asks[i].out->event_capacity);
    }
    if (!grid.any()) return CSF_OK;
    MeasureScratch<PassDesc> &g = e0->passing;
    if (int rc = measure_reserve(e0, g, st, m, total + scratch, total)) return rc;
    size_t at = header, part_at = total;
    for (size_t i = 0; i < m; i++) {
        const PassAsk &a = asks[i];
        const int64_t n = a.e->d.n;
        PassDesc r{};
        if (n > 0 && a.count >= 2) {
            const int64_t st_n = a.count - 1, S = st_n * n, I = S - n;
            desc_ring(r, a);
            r.split = 1, r.chunk_tiles = 1;
            if (n > ENC_SMALL) enc_split(n, st_n, r.split, r.chunk_tiles);
            r.part_off = (int64_t)part_at, part_at += pass_part_bytes((size_t)S, (size_t)r.split);
            r.out_off = (int64_t)at;
            at += pass_block_bytes((size_t)S, (size_t)I, (size_t)n);
            desc_events<csf_passing_event>(r, at, a.out->event_capacity);
        }
        g.desc.p[i] = r;
    }
    PassArgs ka{};
    ka.desc = g.desc.dev, ka.out = g.dev.p, ka.count = (unsigned long long *)g.dev.p;
    ka.band = band, ka.lat_max = lat_max;
    ka.lat_event = lat_event > 0.0 ? lat_event : 0.0;
    const dim3 dim = grid.dim(m);
    if (int rc = measure_launch(e0, g, st, header, total, ps, e0->passing_launches, PASS_LAUNCHES, [&](hipEvent_t t0, hipEvent_t t1) {
            launch_passing(ka, ka.lat_event > 0.0, dim, (int)m, (int)grid.max_n, st, t0, t1);
        }))
        return rc;
    const unsigned long long *found = (const unsigned long long *)g.host.p;
    for (size_t i = 0; i < m; i++) {
        const PassDesc &r = g.desc.p[i];
        csf_passing_out &o = *asks[i].out;
        if (r.n <= 0) continue;
        const size_t n = (size_t)r.n, S = (size_t)(r.count - 1) * n, I = S - n;
        Cursor b{g.host.p + r.out_off};
        b.take(o.gap, S * 8), b.take(o.thw, S * 8), b.take(o.made_lat, I * 8), b.take(o.made_t, I * 8), b.take(o.by_lat, I * 8), b.take(o.by_t, I * 8);
        b.take(o.run_gap, n * 8), b.take(o.run_thw, n * 8), b.take(o.run_made_lat, n * 8), b.take(o.run_made_t, n * 8), b.take(o.run_by_lat, n * 8), b.take(o.run_by_t, n * 8);
        b.take(o.gap_with, S * 4), b.take(o.made_with, I * 4), b.take(o.made_kind, I * 4), b.take(o.by_with, I * 4), b.take(o.by_kind, I * 4);
        b.take(o.run_gap_with, n * 4), b.take(o.run_gap_k, n * 4), b.take(o.run_thw_with, n * 4), b.take(o.run_thw_k, n * 4);
        b.take(o.run_made_with, n * 4), b.take(o.run_made_kind, n * 4), b.take(o.run_by_with, n * 4), b.take(o.run_by_kind, n * 4);
        b.take(o.run_made, n * 12), b.take(o.run_by, n * 12);
        take_events(o, found[i], g.host.p + r.ev_off, passing_event_less);
    }
    return CSF_OK;
}

}  // extern "C++"

int csf_passing(csf_engine *e, int64_t first_sample, int64_t n_samples, double band, double lat_max, double lat_event, csf_passing_out *out) try {
    static const char *const who = "csf_passing";
    int rc = measure_open(e, who, first_sample, n_samples, out, "direction of travel", [&] { return passing_args_ok(e, who, band, lat_max, lat_event, out); });
    if (rc) return rc;
    if ((rc = cells_ok(e, who, -1, e->d.n * n_samples))) return rc;
    out->first_sample = first_sample;
    PassAsk ask{e, first_sample, n_samples, out};
    csf_engine::ProfSlot *ps = nullptr;
    if ((rc = prof_take(e, e->d.n > 0 && n_samples >= 2, &ps))) return rc;
    return passing_run(e, e->main, &ask, 1, band, lat_max, lat_event, ps);
} catch (...) { return csf_caught(e); }

int csf_batch_passing(csf_engine *const *engines, int32_t count, int64_t n_last, double band, double lat_max, double lat_event,
                      csf_passing_out *outs) try {
    static const char *const who = "csf_batch_passing";
    int rc = batch_open(engines, count, who, outs);
    if (rc) return rc;
    csf_engine *e0 = engines[0];
    if ((rc = batch_sizes_ok(e0, who, n_last, count))) return rc;
    std::vector<PassAsk> asks;
    rc = batch_members(engines, count, who, n_last, outs, asks,
                       [&](csf_engine *e, int32_t i) { return passing_args_ok(e, who, band, lat_max, lat_event, &outs[i]); },
                       [&](csf_engine *e, int32_t i) { return cells_ok(e, who, i, e->d.n * n_last); });
    if (rc) return rc;
    if ((rc = batch_device(e0))) return rc;
    return passing_run(e0, e0->main, asks.data(), asks.size(), band, lat_max, lat_event, nullptr);
} catch (...) { return csf_caught((engines && count > 0 ? engines[0] : nullptr)); }

int csf_passing_launches(const csf_engine *e, int64_t *n_launches) try {
    return measure_launches(e, n_launches, &csf_engine::passing_launches);
} catch (...) { return csf_caught(e); }
