// engine/abi_body.inc - C ABI: free gap and time to contact between the road users' outlines (csf_body.hip).
// (a section of csf_engine.hip: included there behind abi_encounter.inc, whose split of a sample's sources it shares; not a
// translation unit of its own)

extern "C++" {

// what one engine is asked: samples [first, first + count) of its ring, or the current state, and its extents
struct BodyAsk {
    MeasureAsk<csf_body_out> a;
    const double *ext;
};

// the refusals that depend on the arguments every member shares, and on a member's outputs
static int body_args_ok(csf_engine *e, const char *who, double gap_event, double ttc_event, const csf_body_out *o) {
    if (!std::isfinite(gap_event) || !std::isfinite(ttc_event))
        return fail(e, CSF_E_ARG, "%s: gap_event = %g, ttc_event = %g (finite; gap_event < 0 and ttc_event <= 0 switch a test off)", who, gap_event, ttc_event);
    return events_ok(e, who, o);
}

// ... and on a member's extents [n][3]
static int body_ext_ok(csf_engine *e, const char *who, const double *ext, int64_t n) {
    if (!ext) return fail(e, CSF_E_ARG, "%s: ext is NULL", who);
    for (int64_t u = 0; u < n; u++) {
        const double f = ext[3 * u], r = ext[3 * u + 1], w = ext[3 * u + 2];
        if (!std::isfinite(f) || !std::isfinite(r) || !std::isfinite(w))
            return fail(e, CSF_E_ARG, "%s: road user %lld has a non-finite extent (front %g, rear %g, half_width %g)", who, (long long)u, f, r, w);
        if (f < 0.0 || r < 0.0 || !(f + r > 0.0) || !(w > 0.0))
            return fail(e, CSF_E_ARG, "%s: road user %lld has the extents front %g, rear %g, half_width %g (front >= 0, rear >= 0, front + rear > 0, half_width > 0)",
                        who, (long long)u, f, r, w);
    }
    return CSF_OK;
}

static bool body_event_less(const csf_body_event &a, const csf_body_event &b) {
    if (a.sample != b.sample) return a.sample < b.sample;
    if (a.i != b.i) return a.i < b.i;
    return a.j < b.j;
}

// One upload of the extents, two launches on `st`, one copy, one wait, then the packed buffer -> the callers' arrays.  The asks
// have been checked.  ps: the time stamps of the first launch (csf_profile_enable), or NULL.
static int body_run(csf_engine *e0, hipStream_t st, const BodyAsk *asks, size_t m, double gap_event, double ttc_event, csf_engine::ProfSlot *ps) {
    const size_t header = round32(m * sizeof(unsigned long long));
    size_t total = header, scratch = 0, ext_n = 0;             // scratch: the chunks' minima, device memory behind what is transferred
    MeasureGrid grid;
    for (size_t i = 0; i < m; i++) {
        asks[i].a.out->n_events = 0;
        const int64_t n = enc_population(asks[i].a), c = asks[i].a.count;
        if (n <= 0 || c <= 0) continue;
        int32_t split = 1, chunk_tiles = 1;
        if (n > ENC_SMALL) enc_split(n, c, split, chunk_tiles);
        grid.add(n, c, split);
        if (split > 1) scratch += 24 * (size_t)split * (size_t)(c * n);
        ext_n += 3 * (size_t)n;
        total += body_block_bytes((size_t)(c * n), (size_t)n) + events_bytes<csf_body_event>(asks[i].a.out->event_capacity);
    }
    if (!grid.any()) return CSF_OK;
    MeasureScratch<BodyDesc> &g = e0->body.m;
    HostBuf<double, false> &ext_host = e0->body.ext_host;
    DevBuf<double> &ext = e0->body.ext;
    HIPCHK(e0, ext_host.reserve(ext_n, st, 512));
    HIPCHK(e0, ext.reserve(ext_n));
    if (int rc = measure_reserve(e0, g, st, m, total + scratch, total)) return rc;
    size_t at = header, part_at = total, ext_at = 0;
    for (size_t i = 0; i < m; i++) {
        const MeasureAsk<csf_body_out> &a = asks[i].a;
        const int64_t n = enc_population(a);
        BodyDesc b{};
        EncDesc &r = b.m;
        r.ns = a.e->d.ns, r.split = 1, r.chunk_tiles = 1;
        if (n > 0 && a.count > 0) {
            desc_ring_or_state(r, a, n);
            if (n > ENC_SMALL) enc_split(n, a.count, r.split, r.chunk_tiles);
            if (r.split > 1) r.part_off = (int64_t)part_at, part_at += 24 * (size_t)r.split * (size_t)(a.count * n);
            r.out_off = (int64_t)at;
            at += body_block_bytes((size_t)(a.count * n), (size_t)n);
            desc_events<csf_body_event>(r, at, a.out->event_capacity);
            std::memcpy(ext_host.p + ext_at, asks[i].ext, 3 * (size_t)n * sizeof(double));
            b.ext = ext.p + ext_at, ext_at += 3 * (size_t)n;
        }
        g.desc.p[i] = b;
    }
    BodyArgs ka{};
    ka.desc = g.desc.dev, ka.out = g.dev.p, ka.count = (unsigned long long *)g.dev.p;
    ka.gap_event = gap_event >= 0.0 ? gap_event : -1.0;
    ka.ttc_event = ttc_event > 0.0 ? ttc_event : 0.0;
    const bool events = ka.gap_event >= 0.0 || ka.ttc_event > 0.0;
    HIPCHK(e0, hipMemcpyAsync(ext.p, ext_host.p, ext_n * sizeof(double), hipMemcpyHostToDevice, st));
    const dim3 dim = grid.dim(m);
    if (int rc = measure_launch(e0, g, st, header, total, ps, e0->body_launches, 2, [&](hipEvent_t t0, hipEvent_t t1) {
            launch_body(ka, events, dim, (int)m, (int)grid.max_n, st, t0, t1);
        }))
        return rc;
    const unsigned long long *found = (const unsigned long long *)g.host.p;
    for (size_t i = 0; i < m; i++) {
        const EncDesc &r = g.desc.p[i].m;
        csf_body_out &o = *asks[i].a.out;
        if (r.n <= 0 || r.count <= 0) continue;
        const size_t n = (size_t)r.n, cells = (size_t)r.count * n;
        Cursor b{g.host.p + r.out_off};
        b.take(o.gap_min, cells * 8), b.take(o.ttc_min, cells * 8), b.take(o.run_gap_min, n * 8), b.take(o.run_ttc_min, n * 8);
        b.take(o.run_gap_sample, n * 8), b.take(o.run_ttc_sample, n * 8), b.take(o.overlap_n, n * 8);
        b.take(o.gap_with, cells * 4), b.take(o.ttc_with, cells * 4), b.take(o.run_gap_with, n * 4), b.take(o.run_ttc_with, n * 4);
        take_events(o, found[i], g.host.p + r.ev_off, body_event_less, [&](csf_body_event &ev) { event_sample_abs(ev, r.first_abs); });
    }
    return CSF_OK;
}

}  // extern "C++"

int csf_body_encounters(csf_engine *e, int64_t first_sample, int64_t n_samples, const double *ext, double gap_event, double ttc_event,
                        csf_body_out *out) try {
    static const char *const who = "csf_body_encounters";
    int rc = measure_open(e, who, first_sample, n_samples, out, nullptr, [&] { return body_args_ok(e, who, gap_event, ttc_event, out); });
    if (rc) return rc;
    BodyAsk ask{{e, first_sample, n_samples, out}, ext};
    const int64_t n = enc_population(ask.a);                   // (the population with pending arrivals brought in)
    if ((rc = body_ext_ok(e, who, ext, n))) return rc;
    if ((rc = cells_ok(e, who, -1, n * n_samples))) return rc;
    out->first_sample = first_sample;
    csf_engine::ProfSlot *ps = nullptr;
    if ((rc = prof_take(e, n > 0 && n_samples > 0, &ps))) return rc;
    return body_run(e, e->main, &ask, 1, gap_event, ttc_event, ps);
} catch (...) { return csf_caught(e); }

int csf_batch_body_encounters(csf_engine *const *engines, int32_t count, int64_t n_last, const double *const *exts, double gap_event,
                              double ttc_event, csf_body_out *outs) try {
    static const char *const who = "csf_batch_body_encounters";
    int rc = batch_open(engines, count, who, outs);
    if (rc) return rc;
    csf_engine *e0 = engines[0];
    if (!exts) return fail(e0, CSF_E_ARG, "%s: exts is NULL", who);
    if ((rc = batch_sizes_ok(e0, who, n_last, count))) return rc;
    std::vector<MeasureAsk<csf_body_out>> members;
    rc = batch_members(engines, count, who, n_last, outs, members,
                       [&](csf_engine *e, int32_t i) { return body_args_ok(e, who, gap_event, ttc_event, &outs[i]); },
                       [&](csf_engine *e, int32_t i) { return body_ext_ok(e, who, exts[i], e->d.n); },
                       [&](csf_engine *e, int32_t i) { return cells_ok(e, who, i, e->d.n * n_last); });
    if (rc) return rc;
    if ((rc = batch_device(e0))) return rc;
    std::vector<BodyAsk> asks;
    asks.reserve(members.size());
    for (const MeasureAsk<csf_body_out> &a : members) asks.push_back(BodyAsk{a, exts[a.out - outs]});
    return body_run(e0, e0->main, asks.data(), asks.size(), gap_event, ttc_event, nullptr);
} catch (...) { return csf_caught((engines && count > 0 ? engines[0] : nullptr)); }

int csf_body_encounter_launches(const csf_engine *e, int64_t *n_launches) try {
    return measure_launches(e, n_launches, &csf_engine::body_launches);
} catch (...) { return csf_caught(e); }
