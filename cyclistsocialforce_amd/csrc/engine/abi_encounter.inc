// engine/abi_encounter.inc - C ABI: closest approach and time to collision of a recording (csf_encounter.hip).
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

extern "C++" {

using EncAsk = MeasureAsk<csf_encounter_out>;

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

// the refusals that depend on the arguments every member shares, and on a member's outputs
static int encounter_args_ok(csf_engine *e, const char *who, double radius, const csf_encounter_out *o) {
    if (!(radius >= 0.0) || !std::isfinite(radius)) return fail(e, CSF_E_ARG, "%s: radius = %g (finite, >= 0)", who, radius);
    return events_ok(e, who, o);
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
    const size_t header = round32(m * sizeof(unsigned long long));
    size_t total = header, scratch = 0;                        // scratch: the chunks' minima, device memory behind what is transferred
    MeasureGrid grid;
    for (size_t i = 0; i < m; i++) {
        asks[i].out->n_events = 0;
        const int64_t n = enc_population(asks[i]), c = asks[i].count;
        if (n <= 0 || c <= 0) continue;
        int32_t split = 1, chunk_tiles = 1;
        if (n > ENC_SMALL) enc_split(n, c, split, chunk_tiles);
        grid.add(n, c, split);
        if (split > 1) scratch += 24 * (size_t)split * (size_t)(c * n);
        total += enc_block_bytes((size_t)(c * n), (size_t)n) + events_bytes<csf_encounter_event>(asks[i].out->event_capacity);
    }
    if (!grid.any()) return CSF_OK;
    MeasureScratch<EncDesc> &g = e0->enc;
    if (int rc = measure_reserve(e0, g, st, m, total + scratch, total)) return rc;
    size_t at = header, part_at = total;
    for (size_t i = 0; i < m; i++) {
        const EncAsk &a = asks[i];
        const int64_t n = enc_population(a);
        EncDesc r{};
        r.ns = a.e->d.ns, r.split = 1, r.chunk_tiles = 1;
        if (n > 0 && a.count > 0) {
            desc_ring_or_state(r, a, n);
            if (n > ENC_SMALL) enc_split(n, a.count, r.split, r.chunk_tiles);
            if (r.split > 1) r.part_off = (int64_t)part_at, part_at += 24 * (size_t)r.split * (size_t)(a.count * n);
            r.out_off = (int64_t)at;
            at += enc_block_bytes((size_t)(a.count * n), (size_t)n);
            desc_events<csf_encounter_event>(r, at, a.out->event_capacity);
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
    const dim3 dim = grid.dim(m);
    if (int rc = measure_launch(e0, g, st, header, total, ps, e0->encounter_launches, 2, [&](hipEvent_t t0, hipEvent_t t1) {
            launch_encounters(ka, events, dim, (int)m, (int)grid.max_n, st, t0, t1);
        }))
        return rc;
    const unsigned long long *found = (const unsigned long long *)g.host.p;
    for (size_t i = 0; i < m; i++) {
        const EncDesc &r = g.desc.p[i];
        csf_encounter_out &o = *asks[i].out;
        if (r.n <= 0 || r.count <= 0) continue;
        const size_t n = (size_t)r.n, cells = (size_t)r.count * n;
        Cursor b{g.host.p + r.out_off};
        b.take(o.d_min, cells * 8), b.take(o.ttc_min, cells * 8), b.take(o.run_d_min, n * 8), b.take(o.run_ttc_min, n * 8);
        b.take(o.run_d_sample, n * 8), b.take(o.run_ttc_sample, n * 8);
        b.take(o.d_with, cells * 4), b.take(o.ttc_with, cells * 4), b.take(o.run_d_with, n * 4), b.take(o.run_ttc_with, n * 4);
        take_events(o, found[i], g.host.p + r.ev_off, enc_event_less, [&](csf_encounter_event &ev) { event_sample_abs(ev, r.first_abs); });
    }
    return CSF_OK;
}

}  // extern "C++"

int csf_encounters(csf_engine *e, int64_t first_sample, int64_t n_samples, double radius, double d_event, double ttc_event,
                   csf_encounter_out *out) try {
    static const char *const who = "csf_encounters";
    int rc = measure_open(e, who, first_sample, n_samples, out, nullptr, [&] { return encounter_args_ok(e, who, radius, out); });
    if (rc) return rc;
    EncAsk ask{e, first_sample, n_samples, out};
    const int64_t n = enc_population(ask);                     // (the population with pending arrivals brought in)
    if ((rc = cells_ok(e, who, -1, n * n_samples))) return rc;
    out->first_sample = first_sample;
    csf_engine::ProfSlot *ps = nullptr;
    if ((rc = prof_take(e, n > 0 && n_samples > 0, &ps))) return rc;
    return encounters_run(e, e->main, &ask, 1, radius, d_event, ttc_event, ps);
} catch (...) { return csf_caught(e); }

int csf_batch_encounters(csf_engine *const *engines, int32_t count, int64_t n_last, double radius, double d_event, double ttc_event,
                         csf_encounter_out *outs) try {
    static const char *const who = "csf_batch_encounters";
    int rc = batch_open(engines, count, who, outs);
    if (rc) return rc;
    csf_engine *e0 = engines[0];
    if ((rc = batch_sizes_ok(e0, who, n_last, count))) return rc;
    std::vector<EncAsk> asks;
    rc = batch_members(engines, count, who, n_last, outs, asks,
                       [&](csf_engine *e, int32_t i) { return encounter_args_ok(e, who, radius, &outs[i]); },
                       [&](csf_engine *e, int32_t i) { return cells_ok(e, who, i, e->d.n * n_last); });
    if (rc) return rc;
    if ((rc = batch_device(e0))) return rc;
    return encounters_run(e0, e0->main, asks.data(), asks.size(), radius, d_event, ttc_event, nullptr);
} catch (...) { return csf_caught((engines && count > 0 ? engines[0] : nullptr)); }

int csf_encounter_launches(const csf_engine *e, int64_t *n_launches) try {
    return measure_launches(e, n_launches, &csf_engine::encounter_launches);
} catch (...) { return csf_caught(e); }
