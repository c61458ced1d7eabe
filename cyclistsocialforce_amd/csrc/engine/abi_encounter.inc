// engine/abi_encounter.inc - C ABI: closest approach and time to collision of a recording (csf_encounter.hip).
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

extern "C++" {

constexpr int64_t ENC_MAX_SAMPLES = 65535;      // samples per call (the grid's y extent)
constexpr int64_t ENC_MAX_CELLS = 1ll << 31;    // (sample, road user) cells per member

// what one engine is asked: samples [first, first + count) of its ring, or (first == -1) its current state
struct EncAsk {
    csf_engine *e;
    int64_t first, count;
    csf_encounter_out *out;
};

static int64_t enc_population(const EncAsk &a) { return a.first < 0 ? (int64_t)a.e->order.size() : a.e->d.n; }

// Workgroups per receiver tile that share a sample's sources (EncDesc::split).  One receiver per lane makes tiles x samples workgroups:
// 64 for a 16 384-rider sample, on 256 CUs.  Below ENC_FILL workgroups - four waves per SIMD - the sources are split, over at most
// ENC_MAX_SPLIT chunks of whole tiles; the second pass puts the chunks together, the same bits as one chunk gives.
constexpr int64_t ENC_FILL = 1024, ENC_MAX_SPLIT = 16;
static void enc_split(int64_t n, int64_t count, int32_t &split, int32_t &chunk_tiles) {
    const int64_t tiles = (n + 255) / 256, blocks = tiles * count;
    int64_t want = blocks >= ENC_FILL ? 1 : std::min({(ENC_FILL + blocks - 1) / blocks, tiles, ENC_MAX_SPLIT, ENC_MAX_SAMPLES / count});
    want = std::max<int64_t>(want, 1);
    chunk_tiles = (int32_t)((tiles + want - 1) / want);
    split = (int32_t)((tiles + chunk_tiles - 1) / chunk_tiles);
}

// the refusals that depend on the engine alone
static int encounter_engine_ok(csf_engine *e, const char *who) {
    if (int crc = calib_refuses(e, who)) return crc;
    if (e->world > 1 || e->loopback || e->nccl != nullptr || !e->state_all_current)
        return fail(e, CSF_E_STATE, "%s: the engine is a rank of a sharded run or a member of a loopback group - the other ranks' road users have no fp64 state here", who);
    return CSF_OK;
}

// ... and on the arguments every member shares, and on its outputs
static int encounter_args_ok(csf_engine *e, const char *who, double radius, const csf_encounter_out *o) {
    if (!(radius >= 0.0) || !std::isfinite(radius)) return fail(e, CSF_E_ARG, "%s: radius = %g (finite, >= 0)", who, radius);
    if (o->event_capacity < 0) return fail(e, CSF_E_ARG, "%s: event_capacity = %lld", who, (long long)o->event_capacity);
    if (o->event_capacity > 0 && !o->events) return fail(e, CSF_E_ARG, "%s: room for %lld events is given, but events is NULL", who, (long long)o->event_capacity);
    return CSF_OK;
}

static bool enc_event_less(const csf_encounter_event &a, const csf_encounter_event &b) {
    if (a.sample != b.sample) return a.sample < b.sample;
    if (a.i != b.i) return a.i < b.i;
    return a.j < b.j;
}

// Two launches on `st` (the stream every engine asked about works on), one copy, one wait, then the packed buffer -> the callers'
// arrays.  The asks have been checked.  ps: the time stamps of the first launch (csf_profile_enable), or NULL.
static int encounters_run(csf_engine *e0, hipStream_t st, const EncAsk *asks, size_t m, double radius, double d_event, double ttc_event,
                          csf_engine::ProfSlot *ps) {
    for (size_t i = 0; i < m; i++) asks[i].out->n_events = 0;
    size_t total = (m * sizeof(unsigned long long) + 31) & ~(size_t)31;
    const size_t header = total;
    size_t scratch = 0;                                        // the chunks' minima: device memory behind what is transferred
    int64_t gx = 1, gy = 1, plane = 0, max_n = 0;
    bool any = false;
    for (size_t i = 0; i < m; i++) {
        const int64_t n = enc_population(asks[i]), c = asks[i].count;
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
        total += enc_block_bytes((size_t)(c * n), (size_t)n) + (size_t)asks[i].out->event_capacity * sizeof(csf_encounter_event);
    }
    if (!any) return CSF_OK;
    if (gx * gy < plane) {                                     // the packed members take the plane x * y (plane <= 65535 samples)
        if (gx == 1 && gy == 1) gx = plane;
        else gy = (plane + gx - 1) / gx;
    }
    EncScratch &g = e0->enc;
    HIPCHK(e0, g.desc.reserve(m, st, 16));
    HIPCHK(e0, g.dev.reserve(total + scratch));
    HIPCHK(e0, g.host.reserve(total, st, 4096));
    size_t at = header, part_at = total;
    for (size_t i = 0; i < m; i++) {
        const EncAsk &a = asks[i];
        const Dev &d = a.e->d;
        const int64_t n = enc_population(a);
        EncDesc r{};
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
            at += enc_block_bytes((size_t)(a.count * n), (size_t)n);
            r.ev_off = (int64_t)at, r.ev_cap = a.out->event_capacity;
            at += (size_t)a.out->event_capacity * sizeof(csf_encounter_event);
        } else {
            r.n = 0, r.count = 0;
        }
        g.desc.p[i] = r;
    }
    EncArgs ka{};
    ka.desc = g.desc.dev, ka.out = g.dev.p, ka.count = (unsigned long long *)g.dev.p;
    const double R = 2.0 * radius;
    ka.R2 = R * R;
    ka.d_event = d_event > 0.0 ? d_event : 0.0;
    ka.ttc_event = ttc_event > 0.0 ? ttc_event : 0.0;
    ka.de2_hi = ka.d_event * ka.d_event * (1.0 + 1e-15);
    const bool events = ka.d_event > 0.0 || ka.ttc_event > 0.0;
    HIPCHK(e0, hipMemsetAsync(g.dev.p, 0, header, st));
    launch_encounters(ka, events, dim3((unsigned)gx, (unsigned)gy, (unsigned)m), (int)m, (int)max_n, st, ps ? ps->ev[0] : nullptr, ps ? ps->ev[1] : nullptr);
    if (ps) ps->pair = true;
    e0->encounter_launches += 2;
    HIPCHK(e0, hipGetLastError());
    HIPCHK(e0, hipMemcpyAsync(g.host.p, g.dev.p, total, hipMemcpyDeviceToHost, st));
    HIPCHK(e0, hipStreamSynchronize(st));
    const unsigned long long *found = (const unsigned long long *)g.host.p;
    for (size_t i = 0; i < m; i++) {
        const EncDesc &r = g.desc.p[i];
        csf_encounter_out &o = *asks[i].out;
        if (r.n <= 0 || r.count <= 0) continue;
        const size_t n = (size_t)r.n, cells = (size_t)r.count * n;
        const unsigned char *b = g.host.p + r.out_off;
        auto take = [&](void *dst, size_t bytes) {
            if (dst) std::memcpy(dst, b, bytes);
            b += bytes;
        };
        take(o.d_min, cells * 8), take(o.ttc_min, cells * 8), take(o.run_d_min, n * 8), take(o.run_ttc_min, n * 8);
        take(o.run_d_sample, n * 8), take(o.run_ttc_sample, n * 8);
        take(o.d_with, cells * 4), take(o.ttc_with, cells * 4), take(o.run_d_with, n * 4), take(o.run_ttc_with, n * 4);
        o.n_events = (int64_t)found[i];
        const int64_t stored = std::min(o.n_events, o.event_capacity);
        if (stored > 0) {
            std::memcpy(o.events, g.host.p + r.ev_off, (size_t)stored * sizeof(csf_encounter_event));
            for (int64_t k = 0; k < stored; k++)               // (the kernel numbers samples within the call)
                o.events[k].sample = r.first_abs < 0 ? -1 : r.first_abs + o.events[k].sample;
            if (o.n_events <= o.event_capacity) std::sort(o.events, o.events + stored, enc_event_less);
        }
    }
    return CSF_OK;
}

}  // extern "C++"

int csf_encounters(csf_engine *e, int64_t first_sample, int64_t n_samples, double radius, double d_event, double ttc_event,
                   csf_encounter_out *out) try {
    if (!e) return CSF_E_ARG;
    if (!out) return fail(e, CSF_E_ARG, "csf_encounters: out is NULL");
    int rc = encounter_args_ok(e, "csf_encounters", radius, out);
    if (rc) return rc;
    if (n_samples < 0 || n_samples > ENC_MAX_SAMPLES) return fail(e, CSF_E_ARG, "csf_encounters: n_samples = %lld (0 .. 65535)", (long long)n_samples);
    if (first_sample < -1 || (first_sample == -1 && n_samples > 1))
        return fail(e, CSF_E_ARG, "csf_encounters: first_sample = %lld, n_samples = %lld (the current state is first_sample -1 with one sample)",
                    (long long)first_sample, (long long)n_samples);
    if ((rc = encounter_engine_ok(e, "csf_encounters"))) return rc;
    if (first_sample >= 0 && !e->d.hist) return fail(e, CSF_E_STATE, "csf_encounters: no state ring (csf_record, csf_enable_history) - only the current state, first_sample -1, can be covered");
    HIPCHK(e, hipSetDevice(e->device));
    if ((rc = upload_all(e))) return rc;
    if ((rc = csf_sync(e))) return rc;                         // both streams (the side-by-side tick), as the read-backs wait
    if (first_sample >= 0 && (rc = record_range(e, first_sample, n_samples))) return rc;
    if (first_sample < 0 && (rc = sync_order(e))) return rc;
    EncAsk ask{e, first_sample, n_samples, out};
    if (enc_population(ask) * n_samples > ENC_MAX_CELLS) return fail(e, CSF_E_ARG, "csf_encounters: more than 2^31 (sample, road user) cells in one call");
    out->first_sample = first_sample;
    // csf_profile_enable: the first launch is timed like a tick's pair launch, as kernel 0
    csf_engine::ProfSlot *ps = nullptr;
    if (e->profile > 0 && enc_population(ask) > 0 && n_samples > 0) {
        if ((rc = prof_make_pool(e))) return rc;
        if (e->prof_issued - e->prof_resolved >= PROF_SLOTS && (rc = prof_resolve_one(e))) return rc;
        ps = &e->prof_pool[e->prof_issued % PROF_SLOTS];
        ps->pair = ps->road = ps->agent = ps->gather = false;
        e->prof_issued++;
    }
    return encounters_run(e, e->main, &ask, 1, radius, d_event, ttc_event, ps);
} catch (...) { return csf_caught(e); }

int csf_batch_encounters(csf_engine *const *engines, int32_t count, int64_t n_last, double radius, double d_event, double ttc_event,
                         csf_encounter_out *outs) try {
    int rc = batch_check(engines, count);
    if (rc) return rc;
    csf_engine *e0 = engines[0];
    if (!outs) return fail(e0, CSF_E_ARG, "csf_batch_encounters: outs is NULL");
    if (n_last < 0 || n_last > ENC_MAX_SAMPLES) return fail(e0, CSF_E_ARG, "csf_batch_encounters: n_last = %lld (0 .. 65535)", (long long)n_last);
    if (count > 65535) return fail(e0, CSF_E_ARG, "csf_batch_encounters: at most 65535 engines in one call (%d given)", (int)count);
    std::vector<EncAsk> asks;
    asks.reserve((size_t)count);
    for (int32_t i = 0; i < count; i++) {        // every refusal before anything is written
        csf_engine *e = engines[i];
        if ((rc = encounter_args_ok(e, "csf_batch_encounters", radius, &outs[i]))) return rc;
        if ((rc = encounter_engine_ok(e, "csf_batch_encounters"))) return rc;
        if (!e->d.hist) continue;
        int64_t first = 0;
        if (int rrc = record_last(e, i, n_last, &first)) return rrc;
        if (e->d.n * n_last > ENC_MAX_CELLS) return fail(e, CSF_E_ARG, "member %d: more than 2^31 (sample, road user) cells in one call", (int)i);
        asks.push_back(EncAsk{e, first, n_last, &outs[i]});
    }
    for (int32_t i = 0; i < count; i++) outs[i].n_events = 0, outs[i].first_sample = -2;
    for (const EncAsk &a : asks) a.out->first_sample = a.first;
    HIPCHK(e0, hipSetDevice(e0->device));
    // (the members share one stream, and a member stepped in turn has joined its second stream back into it: stream order is enough)
    return encounters_run(e0, e0->main, asks.data(), asks.size(), radius, d_event, ttc_event, nullptr);
} catch (...) { return csf_caught((engines && count > 0 ? engines[0] : nullptr)); }

int csf_encounter_launches(const csf_engine *e, int64_t *n_launches) try {
    if (!e || !n_launches) return CSF_E_ARG;
    *n_launches = e->encounter_launches;
    return CSF_OK;
} catch (...) { return csf_caught(e); }
