// engine/abi_passing.inc - C ABI: gaps to the leader, overtakings and meetings of a recording (csf_passing.hip).
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

extern "C++" {

// what one engine is asked: samples [first, first + count) of its ring
struct PassAsk {
    csf_engine *e;
    int64_t first, count;
    csf_passing_out *out;
};

// the refusals that depend on the arguments every member shares, and on a member's outputs
static int passing_args_ok(csf_engine *e, const char *who, double band, double lat_max, double lat_event, const csf_passing_out *o) {
    if (!(band >= 0.0)) return fail(e, CSF_E_ARG, "%s: band = %g (>= 0; +inf takes every road user ahead)", who, band);
    if (!(lat_max > 0.0)) return fail(e, CSF_E_ARG, "%s: lat_max = %g (> 0; +inf takes every passing)", who, lat_max);
    if (std::isnan(lat_event) || lat_event == -INFINITY) return fail(e, CSF_E_ARG, "%s: lat_event = %g (a number; <= 0 switches events off, +inf takes every passing)", who, lat_event);
    if (o->event_capacity < 0) return fail(e, CSF_E_ARG, "%s: event_capacity = %lld", who, (long long)o->event_capacity);
    if (o->event_capacity > 0 && !o->events) return fail(e, CSF_E_ARG, "%s: room for %lld events is given, but events is NULL", who, (long long)o->event_capacity);
    return CSF_OK;
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
    for (size_t i = 0; i < m; i++) asks[i].out->n_events = 0;
    size_t total = (m * sizeof(unsigned long long) + 31) & ~(size_t)31;
    const size_t header = total;
    size_t scratch = 0;                                        // the chunks' results: device memory behind what is transferred
    int64_t gx = 1, gy = 1, plane = 0, max_n = 0;
    bool any = false;
    for (size_t i = 0; i < m; i++) {
        const int64_t n = asks[i].e->d.n, st_n = asks[i].count - 1;      // st_n: stations of a road user
        if (n <= 0 || st_n <= 0) {
            passing_nothing(asks[i]);
            continue;
        }
        any = true;
        max_n = std::max(max_n, n);
        int32_t split = 1, chunk_tiles = 1;
        if (n <= ENC_SMALL) {
            const int64_t spw = 256 / n;
            plane = std::max(plane, (st_n + spw - 1) / spw);
        } else {
            enc_split(n, st_n, split, chunk_tiles);
            gx = std::max(gx, (n + 255) / 256);
            gy = std::max(gy, st_n * split);
        }
        scratch += pass_part_bytes((size_t)(st_n * n), (size_t)split);
        total += pass_block_bytes((size_t)(st_n * n), (size_t)((st_n - 1) * n), (size_t)n) + (size_t)asks[i].out->event_capacity * sizeof(csf_passing_event);
    }
    if (!any) return CSF_OK;
    if (gx * gy < plane) {                                     // the packed members take the plane x * y (plane <= 65535 stations)
        if (gx == 1 && gy == 1) gx = plane;
        else gy = (plane + gx - 1) / gx;
    }
    PassScratch &g = e0->passing;
    HIPCHK(e0, g.desc.reserve(m, st, 16));
    HIPCHK(e0, g.dev.reserve(total + scratch));
    HIPCHK(e0, g.host.reserve(total, st, 4096));
    size_t at = header, part_at = total;
    for (size_t i = 0; i < m; i++) {
        const PassAsk &a = asks[i];
        const Dev &d = a.e->d;
        PassDesc r{};
        if (d.n > 0 && a.count >= 2) {
            const int64_t st_n = a.count - 1, S = st_n * d.n, I = S - d.n;
            r.n = (int32_t)d.n, r.ns = d.ns, r.count = (int32_t)a.count;
            r.split = 1, r.chunk_tiles = 1;
            if (d.n > ENC_SMALL) enc_split(d.n, st_n, r.split, r.chunk_tiles);
            r.part_off = (int64_t)part_at, part_at += pass_part_bytes((size_t)S, (size_t)r.split);
            r.s = d.hist, r.cap = d.hist_cap, r.first = (int32_t)(a.first % d.hist_cap);
            r.out_off = (int64_t)at;
            at += pass_block_bytes((size_t)S, (size_t)I, (size_t)d.n);
            r.ev_off = (int64_t)at, r.ev_cap = a.out->event_capacity;
            at += (size_t)a.out->event_capacity * sizeof(csf_passing_event);
        }
        g.desc.p[i] = r;
    }
    PassArgs ka{};
    ka.desc = g.desc.dev, ka.out = g.dev.p, ka.count = (unsigned long long *)g.dev.p;
    ka.band = band, ka.lat_max = lat_max;
    ka.lat_event = lat_event > 0.0 ? lat_event : 0.0;
    HIPCHK(e0, hipMemsetAsync(g.dev.p, 0, header, st));
    launch_passing(ka, ka.lat_event > 0.0, dim3((unsigned)gx, (unsigned)gy, (unsigned)m), (int)m, (int)max_n, st, ps ? ps->ev[0] : nullptr, ps ? ps->ev[1] : nullptr);
    if (ps) ps->pair = true;
    e0->passing_launches += PASS_LAUNCHES;
    HIPCHK(e0, hipGetLastError());
    HIPCHK(e0, hipMemcpyAsync(g.host.p, g.dev.p, total, hipMemcpyDeviceToHost, st));
    HIPCHK(e0, hipStreamSynchronize(st));
    const unsigned long long *found = (const unsigned long long *)g.host.p;
    for (size_t i = 0; i < m; i++) {
        const PassDesc &r = g.desc.p[i];
        csf_passing_out &o = *asks[i].out;
        if (r.n <= 0) continue;
        const size_t n = (size_t)r.n, S = (size_t)(r.count - 1) * n, I = S - n;
        const unsigned char *b = g.host.p + r.out_off;
        auto take = [&](void *dst, size_t bytes) {
            if (dst) std::memcpy(dst, b, bytes);
            b += bytes;
        };
        take(o.gap, S * 8), take(o.thw, S * 8), take(o.made_lat, I * 8), take(o.made_t, I * 8), take(o.by_lat, I * 8), take(o.by_t, I * 8);
        take(o.run_gap, n * 8), take(o.run_thw, n * 8), take(o.run_made_lat, n * 8), take(o.run_made_t, n * 8), take(o.run_by_lat, n * 8), take(o.run_by_t, n * 8);
        take(o.gap_with, S * 4), take(o.made_with, I * 4), take(o.made_kind, I * 4), take(o.by_with, I * 4), take(o.by_kind, I * 4);
        take(o.run_gap_with, n * 4), take(o.run_gap_k, n * 4), take(o.run_thw_with, n * 4), take(o.run_thw_k, n * 4);
        take(o.run_made_with, n * 4), take(o.run_made_kind, n * 4), take(o.run_by_with, n * 4), take(o.run_by_kind, n * 4);
        take(o.run_made, n * 12), take(o.run_by, n * 12);
        o.n_events = (int64_t)found[i];
        const int64_t stored = std::min(o.n_events, o.event_capacity);
        if (stored > 0) {
            std::memcpy(o.events, g.host.p + r.ev_off, (size_t)stored * sizeof(csf_passing_event));
            if (o.n_events <= o.event_capacity) std::sort(o.events, o.events + stored, passing_event_less);
        }
    }
    return CSF_OK;
}

}  // extern "C++"

int csf_passing(csf_engine *e, int64_t first_sample, int64_t n_samples, double band, double lat_max, double lat_event, csf_passing_out *out) try {
    static const char *const who = "csf_passing";
    if (!e) return CSF_E_ARG;
    if (!out) return fail(e, CSF_E_ARG, "%s: out is NULL", who);
    int rc = passing_args_ok(e, who, band, lat_max, lat_event, out);
    if (rc) return rc;
    if (n_samples < 0 || n_samples > ENC_MAX_SAMPLES) return fail(e, CSF_E_ARG, "%s: n_samples = %lld (0 .. 65535)", who, (long long)n_samples);
    if (first_sample < 0)
        return fail(e, CSF_E_ARG, "%s: first_sample = %lld (the current state, -1, has no direction of travel: a window of the state ring is needed)", who, (long long)first_sample);
    if ((rc = encounter_engine_ok(e, who))) return rc;
    if (!e->d.hist) return fail(e, CSF_E_STATE, "%s: no state ring (csf_record, csf_enable_history)", who);
    HIPCHK(e, hipSetDevice(e->device));
    if ((rc = upload_all(e))) return rc;
    if ((rc = csf_sync(e))) return rc;                         // both streams (the side-by-side tick), as the read-backs wait
    if ((rc = record_range(e, first_sample, n_samples))) return rc;
    if (e->d.n * n_samples > ENC_MAX_CELLS) return fail(e, CSF_E_ARG, "%s: more than 2^31 (sample, road user) cells in one call", who);
    out->first_sample = first_sample;
    PassAsk ask{e, first_sample, n_samples, out};
    // csf_profile_enable: the first launch is timed like a tick's pair launch, as kernel 0
    csf_engine::ProfSlot *ps = nullptr;
    if (e->profile > 0 && e->d.n > 0 && n_samples >= 2) {
        if ((rc = prof_make_pool(e))) return rc;
        if (e->prof_issued - e->prof_resolved >= PROF_SLOTS && (rc = prof_resolve_one(e))) return rc;
        ps = &e->prof_pool[e->prof_issued % PROF_SLOTS];
        ps->pair = ps->road = ps->agent = ps->gather = false;
        e->prof_issued++;
    }
    return passing_run(e, e->main, &ask, 1, band, lat_max, lat_event, ps);
} catch (...) { return csf_caught(e); }

int csf_batch_passing(csf_engine *const *engines, int32_t count, int64_t n_last, double band, double lat_max, double lat_event,
                      csf_passing_out *outs) try {
    static const char *const who = "csf_batch_passing";
    int rc = batch_check(engines, count);
    if (rc) return rc;
    csf_engine *e0 = engines[0];
    if (!outs) return fail(e0, CSF_E_ARG, "%s: outs is NULL", who);
    if (n_last < 0 || n_last > ENC_MAX_SAMPLES) return fail(e0, CSF_E_ARG, "%s: n_last = %lld (0 .. 65535)", who, (long long)n_last);
    if (count > 65535) return fail(e0, CSF_E_ARG, "%s: at most 65535 engines in one call (%d given)", who, (int)count);
    std::vector<PassAsk> asks;
    asks.reserve((size_t)count);
    for (int32_t i = 0; i < count; i++) {        // every refusal before anything is written
        csf_engine *e = engines[i];
        if ((rc = passing_args_ok(e, who, band, lat_max, lat_event, &outs[i]))) return rc;
        if ((rc = encounter_engine_ok(e, who))) return rc;
        if (!e->d.hist) continue;
        int64_t first = 0;
        if (int rrc = record_last(e, i, n_last, &first)) return rrc;
        if (e->d.n * n_last > ENC_MAX_CELLS) return fail(e, CSF_E_ARG, "member %d: more than 2^31 (sample, road user) cells in one call", (int)i);
        asks.push_back(PassAsk{e, first, n_last, &outs[i]});
    }
    for (int32_t i = 0; i < count; i++) outs[i].n_events = 0, outs[i].first_sample = -2;
    for (const PassAsk &a : asks) a.out->first_sample = a.first;
    HIPCHK(e0, hipSetDevice(e0->device));
    // (the members share one stream, and a member stepped in turn has joined its second stream back into it: stream order is enough)
    return passing_run(e0, e0->main, asks.data(), asks.size(), band, lat_max, lat_event, nullptr);
} catch (...) { return csf_caught((engines && count > 0 ? engines[0] : nullptr)); }

int csf_passing_launches(const csf_engine *e, int64_t *n_launches) try {
    if (!e || !n_launches) return CSF_E_ARG;
    *n_launches = e->passing_launches;
    return CSF_OK;
} catch (...) { return csf_caught(e); }
