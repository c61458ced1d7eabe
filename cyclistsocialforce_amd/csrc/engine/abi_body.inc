// engine/abi_body.inc - C ABI: free gap and time to contact between the road users' outlines (csf_body.hip).
// (a section of csf_engine.hip: included there behind abi_encounter.inc, whose asks, split and engine checks it shares; not a
// translation unit of its own)

extern "C++" {

// what one engine is asked: an EncAsk (samples [first, first + count) of its ring, or the current state; `out` unused) and its extents
struct BodyAsk {
    EncAsk a;
    const double *ext;
    csf_body_out *out;
};

// the refusals that depend on the arguments every member shares, and on a member's outputs
static int body_args_ok(csf_engine *e, const char *who, double gap_event, double ttc_event, const csf_body_out *o) {
    if (!std::isfinite(gap_event) || !std::isfinite(ttc_event))
        return fail(e, CSF_E_ARG, "%s: gap_event = %g, ttc_event = %g (finite; gap_event < 0 and ttc_event <= 0 switch a test off)", who, gap_event, ttc_event);
    if (o->event_capacity < 0) return fail(e, CSF_E_ARG, "%s: event_capacity = %lld", who, (long long)o->event_capacity);
    if (o->event_capacity > 0 && !o->events) return fail(e, CSF_E_ARG, "%s: room for %lld events is given, but events is NULL", who, (long long)o->event_capacity);
    return CSF_OK;
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
    for (size_t i = 0; i < m; i++) asks[i].out->n_events = 0;
    size_t total = (m * sizeof(unsigned long long) + 31) & ~(size_t)31;
    const size_t header = total;
    size_t scratch = 0, ext_n = 0;                             // the chunks' minima: device memory behind what is transferred
    int64_t gx = 1, gy = 1, plane = 0, max_n = 0;
    bool any = false;
    for (size_t i = 0; i < m; i++) {
        const int64_t n = enc_population(asks[i].a), c = asks[i].a.count;
        if (n <= 0 || c <= 0) continue;
        any = true;
        max_n = std::max(max_n, n);
        if (n <= ENC_SMALL) {
            const int64_t spw = 256 / n;
            plane = std::max(plane, (c + spw - 1) / spw);
        } else {
            int32_t split, chunk_tiles;
            enc_split(n, c, split, chunk_tiles);
            gx = std::max(gx, (n + 255) / 256);
            gy = std::max(gy, c * split);
            if (split > 1) scratch += 24 * (size_t)split * (size_t)(c * n);
        }
        ext_n += 3 * (size_t)n;
        total += body_block_bytes((size_t)(c * n), (size_t)n) + (size_t)asks[i].out->event_capacity * sizeof(csf_body_event);
    }
    if (!any) return CSF_OK;
    if (gx * gy < plane) {                                     // the packed members take the plane x * y (plane <= 65535 samples)
        if (gx == 1 && gy == 1) gx = plane;
        else gy = (plane + gx - 1) / gx;
    }
    BodyScratch &g = e0->body;
    HIPCHK(e0, g.desc.reserve(m, st, 16));
    HIPCHK(e0, g.ext_host.reserve(ext_n, st, 512));
    HIPCHK(e0, g.ext.reserve(ext_n));
    HIPCHK(e0, g.dev.reserve(total + scratch));
    HIPCHK(e0, g.host.reserve(total, st, 4096));
    size_t at = header, part_at = total, ext_at = 0;
    for (size_t i = 0; i < m; i++) {
        const EncAsk &a = asks[i].a;
        const Dev &d = a.e->d;
        const int64_t n = enc_population(a);
        BodyDesc b{};
        EncDesc &r = b.m;
        r.n = (int32_t)n, r.ns = d.ns, r.count = (int32_t)a.count;
        r.split = 1, r.chunk_tiles = 1;
        if (n > 0 && a.count > 0) {
            if (n > ENC_SMALL) enc_split(n, a.count, r.split, r.chunk_tiles);
            if (r.split > 1) r.part_off = (int64_t)part_at, part_at += 24 * (size_t)r.split * (size_t)(a.count * n);
            if (a.first < 0) {
                r.ring = 0, r.s = d.s, r.order = d.order, r.stride = d.cap, r.first_abs = -1, r.cap = 1, r.first = 0;
            } else {
                r.ring = 1, r.s = d.hist, r.cap = d.hist_cap, r.first = (int32_t)(a.first % d.hist_cap), r.first_abs = a.first;
            }
            r.out_off = (int64_t)at;
            at += body_block_bytes((size_t)(a.count * n), (size_t)n);
            r.ev_off = (int64_t)at, r.ev_cap = asks[i].out->event_capacity;
            at += (size_t)asks[i].out->event_capacity * sizeof(csf_body_event);
            std::memcpy(g.ext_host.p + ext_at, asks[i].ext, 3 * (size_t)n * sizeof(double));
            b.ext = g.ext.p + ext_at, ext_at += 3 * (size_t)n;
        } else {
            r.n = 0, r.count = 0;
        }
        g.desc.p[i] = b;
    }
    BodyArgs ka{};
    ka.desc = g.desc.dev, ka.out = g.dev.p, ka.count = (unsigned long long *)g.dev.p;
    ka.gap_event = gap_event >= 0.0 ? gap_event : -1.0;
    ka.ttc_event = ttc_event > 0.0 ? ttc_event : 0.0;
    const bool events = ka.gap_event >= 0.0 || ka.ttc_event > 0.0;
    HIPCHK(e0, hipMemcpyAsync(g.ext.p, g.ext_host.p, ext_n * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(e0, hipMemsetAsync(g.dev.p, 0, header, st));
    launch_body(ka, events, dim3((unsigned)gx, (unsigned)gy, (unsigned)m), (int)m, (int)max_n, st, ps ? ps->ev[0] : nullptr, ps ? ps->ev[1] : nullptr);
    if (ps) ps->pair = true;
    e0->body_launches += 2;
    HIPCHK(e0, hipGetLastError());
    HIPCHK(e0, hipMemcpyAsync(g.host.p, g.dev.p, total, hipMemcpyDeviceToHost, st));
    HIPCHK(e0, hipStreamSynchronize(st));
    const unsigned long long *found = (const unsigned long long *)g.host.p;
    for (size_t i = 0; i < m; i++) {
        const EncDesc &r = g.desc.p[i].m;
        csf_body_out &o = *asks[i].out;
        if (r.n <= 0 || r.count <= 0) continue;
        const size_t n = (size_t)r.n, cells = (size_t)r.count * n;
        const unsigned char *b = g.host.p + r.out_off;
        auto take = [&](void *dst, size_t bytes) {
            if (dst) std::memcpy(dst, b, bytes);
            b += bytes;
        };
        take(o.gap_min, cells * 8), take(o.ttc_min, cells * 8), take(o.run_gap_min, n * 8), take(o.run_ttc_min, n * 8);
        take(o.run_gap_sample, n * 8), take(o.run_ttc_sample, n * 8), take(o.overlap_n, n * 8);
        take(o.gap_with, cells * 4), take(o.ttc_with, cells * 4), take(o.run_gap_with, n * 4), take(o.run_ttc_with, n * 4);
        o.n_events = (int64_t)found[i];
        const int64_t stored = std::min(o.n_events, o.event_capacity);
        if (stored > 0) {
            std::memcpy(o.events, g.host.p + r.ev_off, (size_t)stored * sizeof(csf_body_event));
            for (int64_t k = 0; k < stored; k++)               // (the kernel numbers samples within the call)
                o.events[k].sample = r.first_abs < 0 ? -1 : r.first_abs + o.events[k].sample;
            if (o.n_events <= o.event_capacity) std::sort(o.events, o.events + stored, body_event_less);
        }
    }
    return CSF_OK;
}

}  // extern "C++"

int csf_body_encounters(csf_engine *e, int64_t first_sample, int64_t n_samples, const double *ext, double gap_event, double ttc_event,
                        csf_body_out *out) try {
    const char *who = "csf_body_encounters";
    if (!e) return CSF_E_ARG;
    if (!out) return fail(e, CSF_E_ARG, "%s: out is NULL", who);
    int rc = body_args_ok(e, who, gap_event, ttc_event, out);
    if (rc) return rc;
    if (n_samples < 0 || n_samples > ENC_MAX_SAMPLES) return fail(e, CSF_E_ARG, "%s: n_samples = %lld (0 .. 65535)", who, (long long)n_samples);
    if (first_sample < -1 || (first_sample == -1 && n_samples > 1))
        return fail(e, CSF_E_ARG, "%s: first_sample = %lld, n_samples = %lld (the current state is first_sample -1 with one sample)", who,
                    (long long)first_sample, (long long)n_samples);
    if ((rc = encounter_engine_ok(e, who))) return rc;
    if (first_sample >= 0 && !e->d.hist) return fail(e, CSF_E_STATE, "%s: no state ring (csf_record, csf_enable_history) - only the current state, first_sample -1, can be covered", who);
    HIPCHK(e, hipSetDevice(e->device));
    if ((rc = upload_all(e))) return rc;
    if ((rc = csf_sync(e))) return rc;                         // both streams (the side-by-side tick), as the read-backs wait
    if (first_sample >= 0 && (rc = record_range(e, first_sample, n_samples))) return rc;
    if (first_sample < 0 && (rc = sync_order(e))) return rc;
    BodyAsk ask{EncAsk{e, first_sample, n_samples, nullptr}, ext, out};
    if ((rc = body_ext_ok(e, who, ext, enc_population(ask.a)))) return rc;   // (the population with pending arrivals brought in)
    if (enc_population(ask.a) * n_samples > ENC_MAX_CELLS) return fail(e, CSF_E_ARG, "%s: more than 2^31 (sample, road user) cells in one call", who);
    out->first_sample = first_sample;
    // csf_profile_enable: the first launch is timed like a tick's pair launch, as kernel 0
    csf_engine::ProfSlot *ps = nullptr;
    if (e->profile > 0 && enc_population(ask.a) > 0 && n_samples > 0) {
        if ((rc = prof_make_pool(e))) return rc;
        if (e->prof_issued - e->prof_resolved >= PROF_SLOTS && (rc = prof_resolve_one(e))) return rc;
        ps = &e->prof_pool[e->prof_issued % PROF_SLOTS];
        ps->pair = ps->road = ps->agent = ps->gather = false;
        e->prof_issued++;
    }
    return body_run(e, e->main, &ask, 1, gap_event, ttc_event, ps);
} catch (...) { return csf_caught(e); }

int csf_batch_body_encounters(csf_engine *const *engines, int32_t count, int64_t n_last, const double *const *exts, double gap_event,
                              double ttc_event, csf_body_out *outs) try {
    const char *who = "csf_batch_body_encounters";
    int rc = batch_check(engines, count);
    if (rc) return rc;
    csf_engine *e0 = engines[0];
    if (!outs) return fail(e0, CSF_E_ARG, "%s: outs is NULL", who);
    if (!exts) return fail(e0, CSF_E_ARG, "%s: exts is NULL", who);
    if (n_last < 0 || n_last > ENC_MAX_SAMPLES) return fail(e0, CSF_E_ARG, "%s: n_last = %lld (0 .. 65535)", who, (long long)n_last);
    if (count > 65535) return fail(e0, CSF_E_ARG, "%s: at most 65535 engines in one call (%d given)", who, (int)count);
    std::vector<BodyAsk> asks;
    asks.reserve((size_t)count);
    for (int32_t i = 0; i < count; i++) {        // every refusal before anything is written
        csf_engine *e = engines[i];
        if ((rc = body_args_ok(e, who, gap_event, ttc_event, &outs[i]))) return rc;
        if ((rc = encounter_engine_ok(e, who))) return rc;
        if (!e->d.hist) continue;
        if ((rc = body_ext_ok(e, who, exts[i], e->d.n))) return rc;
        int64_t first = 0;
        if (int rrc = record_last(e, i, n_last, &first)) return rrc;
        if (e->d.n * n_last > ENC_MAX_CELLS) return fail(e, CSF_E_ARG, "member %d: more than 2^31 (sample, road user) cells in one call", (int)i);
        asks.push_back(BodyAsk{EncAsk{e, first, n_last, nullptr}, exts[i], &outs[i]});
    }
    for (int32_t i = 0; i < count; i++) outs[i].n_events = 0, outs[i].first_sample = -2;
    for (const BodyAsk &a : asks) a.out->first_sample = a.a.first;
    HIPCHK(e0, hipSetDevice(e0->device));
    // (the members share one stream, and a member stepped in turn has joined its second stream back into it: stream order is enough)
    return body_run(e0, e0->main, asks.data(), asks.size(), gap_event, ttc_event, nullptr);
} catch (...) { return csf_caught((engines && count > 0 ? engines[0] : nullptr)); }

int csf_body_encounter_launches(const csf_engine *e, int64_t *n_launches) try {
    if (!e || !n_launches) return CSF_E_ARG;
    *n_launches = e->body_launches;
    return CSF_OK;
} catch (...) { return csf_caught(e); }
