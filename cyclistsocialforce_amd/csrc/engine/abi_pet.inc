// engine/abi_pet.inc - C ABI: path crossings of a recording and their post-encroachment time (csf_pet.hip).
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

extern "C++" {

constexpr int64_t PET_MAX_SEGS = 1ll << 30;     // own segments per member

// what one engine is asked: samples [first, first + count) of its ring
struct PetAsk {
    csf_engine *e;
    int64_t first, count;
    csf_pet_out *out;
};

// Workgroups per tile of own segments that share its partners (PetDesc::split).  One own segment per lane makes segs / 256 workgroups:
// 396 for 1 024 riders x 99 segments, on 256 CUs.  Below PET_FILL workgroups - four waves per SIMD - the partners are split, over at
// most PET_MAX_SPLIT chunks of whole tiles; the window pass puts the chunks together, the same bits as one chunk gives.
constexpr int64_t PET_FILL = 1024, PET_MAX_SPLIT = 16;
static void pet_split(int64_t segs, int32_t &split, int32_t &chunk_tiles) {
    const int64_t tiles = (segs + PET_TILE - 1) / PET_TILE;
    int64_t want = tiles >= PET_FILL ? 1 : std::min({(PET_FILL + tiles - 1) / tiles, tiles, PET_MAX_SPLIT});
    want = std::max<int64_t>(want, 1);
    chunk_tiles = (int32_t)((tiles + want - 1) / want);
    split = (int32_t)((tiles + chunk_tiles - 1) / chunk_tiles);
}

// the refusals that depend on the arguments every member shares, and on a member's outputs
static int pet_args_ok(csf_engine *e, const char *who, double pet_event, const csf_pet_out *o) {
    if (std::isnan(pet_event) || pet_event == -INFINITY) return fail(e, CSF_E_ARG, "%s: pet_event = %g (a number; <= 0 switches events off, +inf takes every crossing)", who, pet_event);
    if (o->event_capacity < 0) return fail(e, CSF_E_ARG, "%s: event_capacity = %lld", who, (long long)o->event_capacity);
    if (o->event_capacity > 0 && !o->events) return fail(e, CSF_E_ARG, "%s: room for %lld events is given, but events is NULL", who, (long long)o->event_capacity);
    return CSF_OK;
}

static bool pet_event_less(const csf_pet_event &a, const csf_pet_event &b) {
    if (a.i != b.i) return a.i < b.i;
    if (a.j != b.j) return a.j < b.j;
    if (a.k != b.k) return a.k < b.k;
    return a.l < b.l;
}

// a call that covers no segment: nobody crossed anybody
static void pet_nothing(const PetAsk &a) {
    csf_pet_out &o = *a.out;
    const int64_t n = a.e->d.n;
    for (int64_t u = 0; u < n; u++) {
        if (o.run_pet) o.run_pet[u] = INFINITY;
        if (o.run_with) o.run_with[u] = -1;
        if (o.run_t_own) o.run_t_own[u] = NAN;
        if (o.run_t_with) o.run_t_with[u] = NAN;
        if (o.run_x) o.run_x[u] = NAN;
        if (o.run_y) o.run_y[u] = NAN;
        if (o.run_count) o.run_count[u] = 0;
    }
}

// PET_LAUNCHES launches on `st` (the stream every engine asked about works on), one copy, one wait, then the packed buffer -> the
// callers' arrays.  The asks have been checked.  ps: the time stamps of the first launch (csf_profile_enable), or NULL.
static int pet_run(csf_engine *e0, hipStream_t st, const PetAsk *asks, size_t m, double pet_event, csf_engine::ProfSlot *ps) {
    for (size_t i = 0; i < m; i++) asks[i].out->n_events = 0;
    size_t total = (m * sizeof(unsigned long long) + 31) & ~(size_t)31;
    const size_t header = total;
    size_t scratch = 0;                                        // the chunks' results: device memory behind what is transferred
    int64_t gx = 1, gy = 1, max_n = 0;
    bool any = false;
    for (size_t i = 0; i < m; i++) {
        const int64_t n = asks[i].e->d.n, c = asks[i].count;
        if (n <= 0 || c < 2) {
            pet_nothing(asks[i]);
            continue;
        }
        any = true;
        max_n = std::max(max_n, n);
        const int64_t segs = (c - 1) * n;
        int32_t split, chunk_tiles;
        pet_split(segs, split, chunk_tiles);
        gx = std::max(gx, (segs + PET_TILE - 1) / PET_TILE);
        gy = std::max<int64_t>(gy, split);
        scratch += pet_part_bytes((size_t)segs, (size_t)split);
        total += pet_block_bytes((size_t)segs, (size_t)n) + (size_t)asks[i].out->event_capacity * sizeof(csf_pet_event);
    }
    if (!any) return CSF_OK;
    PetScratch &g = e0->pet;
    HIPCHK(e0, g.desc.reserve(m, st, 16));
    HIPCHK(e0, g.dev.reserve(total + scratch));
    HIPCHK(e0, g.host.reserve(total, st, 4096));
    size_t at = header, part_at = total;
    for (size_t i = 0; i < m; i++) {
        const PetAsk &a = asks[i];
        const Dev &d = a.e->d;
        PetDesc r{};
        if (d.n > 0 && a.count >= 2) {
            const int64_t segs = (a.count - 1) * d.n;
            r.n = (int32_t)d.n, r.ns = d.ns, r.count = (int32_t)a.count;
            pet_split(segs, r.split, r.chunk_tiles);
            r.part_off = (int64_t)part_at, part_at += pet_part_bytes((size_t)segs, (size_t)r.split);
            r.s = d.hist, r.cap = d.hist_cap, r.first = (int32_t)(a.first % d.hist_cap);
            r.out_off = (int64_t)at;
            at += pet_block_bytes((size_t)segs, (size_t)d.n);
            r.ev_off = (int64_t)at, r.ev_cap = a.out->event_capacity;
            at += (size_t)a.out->event_capacity * sizeof(csf_pet_event);
        }
        g.desc.p[i] = r;
    }
    PetArgs ka{};
    ka.desc = g.desc.dev, ka.out = g.dev.p, ka.count = (unsigned long long *)g.dev.p;
    ka.pet_event = pet_event > 0.0 ? pet_event : 0.0;
    HIPCHK(e0, hipMemsetAsync(g.dev.p, 0, header, st));
    launch_pet(ka, ka.pet_event > 0.0, dim3((unsigned)gx, (unsigned)gy, (unsigned)m), (int)m, (int)max_n, st, ps ? ps->ev[0] : nullptr, ps ? ps->ev[1] : nullptr);
    if (ps) ps->pair = true;
    e0->pet_launches += PET_LAUNCHES;
    HIPCHK(e0, hipGetLastError());
    HIPCHK(e0, hipMemcpyAsync(g.host.p, g.dev.p, total, hipMemcpyDeviceToHost, st));
    HIPCHK(e0, hipStreamSynchronize(st));
    const unsigned long long *found = (const unsigned long long *)g.host.p;
    for (size_t i = 0; i < m; i++) {
        const PetDesc &r = g.desc.p[i];
        csf_pet_out &o = *asks[i].out;
        if (r.n <= 0) continue;
        const size_t n = (size_t)r.n, segs = (size_t)(r.count - 1) * n;
        const unsigned char *b = g.host.p + r.out_off;
        auto take = [&](void *dst, size_t bytes) {
            if (dst) std::memcpy(dst, b, bytes);
            b += bytes;
        };
        take(o.seg_pet, segs * 8), take(o.seg_t_own, segs * 8), take(o.seg_t_with, segs * 8);
        take(o.run_pet, n * 8), take(o.run_t_own, n * 8), take(o.run_t_with, n * 8), take(o.run_x, n * 8), take(o.run_y, n * 8);
        take(o.seg_with, segs * 4), take(o.run_with, n * 4), take(o.run_count, n * 4);
        o.n_events = (int64_t)found[i];
        const int64_t stored = std::min(o.n_events, o.event_capacity);
        if (stored > 0) {
            std::memcpy(o.events, g.host.p + r.ev_off, (size_t)stored * sizeof(csf_pet_event));
            if (o.n_events <= o.event_capacity) std::sort(o.events, o.events + stored, pet_event_less);
        }
    }
    return CSF_OK;
}

}  // extern "C++"

int csf_post_encroachment(csf_engine *e, int64_t first_sample, int64_t n_samples, double pet_event, csf_pet_out *out) try {
    static const char *const who = "csf_post_encroachment";
    if (!e) return CSF_E_ARG;
    if (!out) return fail(e, CSF_E_ARG, "%s: out is NULL", who);
    int rc = pet_args_ok(e, who, pet_event, out);
    if (rc) return rc;
    if (n_samples < 0 || n_samples > ENC_MAX_SAMPLES) return fail(e, CSF_E_ARG, "%s: n_samples = %lld (0 .. 65535)", who, (long long)n_samples);
    if (first_sample < 0)
        return fail(e, CSF_E_ARG, "%s: first_sample = %lld (the current state, -1, has no path: a window of the state ring is needed)", who, (long long)first_sample);
    if ((rc = encounter_engine_ok(e, who))) return rc;
    if (!e->d.hist) return fail(e, CSF_E_STATE, "%s: no state ring (csf_record, csf_enable_history)", who);
    HIPCHK(e, hipSetDevice(e->device));
    if ((rc = upload_all(e))) return rc;
    if ((rc = csf_sync(e))) return rc;                         // both streams (the side-by-side tick), as the read-backs wait
    if ((rc = record_range(e, first_sample, n_samples))) return rc;
    if (n_samples >= 2 && e->d.n * (n_samples - 1) > PET_MAX_SEGS) return fail(e, CSF_E_ARG, "%s: more than 2^30 segments in one call", who);
    out->first_sample = first_sample;
    PetAsk ask{e, first_sample, n_samples, out};
    // csf_profile_enable: the first launch is timed like a tick's pair launch, as kernel 0
    csf_engine::ProfSlot *ps = nullptr;
    if (e->profile > 0 && e->d.n > 0 && n_samples >= 2) {
        if ((rc = prof_make_pool(e))) return rc;
        if (e->prof_issued - e->prof_resolved >= PROF_SLOTS && (rc = prof_resolve_one(e))) return rc;
        ps = &e->prof_pool[e->prof_issued % PROF_SLOTS];
        ps->pair = ps->road = ps->agent = ps->gather = false;
        e->prof_issued++;
    }
    return pet_run(e, e->main, &ask, 1, pet_event, ps);
} catch (...) { return csf_caught(e); }

int csf_batch_post_encroachment(csf_engine *const *engines, int32_t count, int64_t n_last, double pet_event, csf_pet_out *outs) try {
    static const char *const who = "csf_batch_post_encroachment";
    int rc = batch_check(engines, count);
    if (rc) return rc;
    csf_engine *e0 = engines[0];
    if (!outs) return fail(e0, CSF_E_ARG, "%s: outs is NULL", who);
    if (n_last < 0 || n_last > ENC_MAX_SAMPLES) return fail(e0, CSF_E_ARG, "%s: n_last = %lld (0 .. 65535)", who, (long long)n_last);
    if (count > 65535) return fail(e0, CSF_E_ARG, "%s: at most 65535 engines in one call (%d given)", who, (int)count);
    std::vector<PetAsk> asks;
    asks.reserve((size_t)count);
    for (int32_t i = 0; i < count; i++) {        // every refusal before anything is written
        csf_engine *e = engines[i];
        if ((rc = pet_args_ok(e, who, pet_event, &outs[i]))) return rc;
        if ((rc = encounter_engine_ok(e, who))) return rc;
        if (!e->d.hist) continue;
        int64_t first = 0;
        if (int rrc = record_last(e, i, n_last, &first)) return rrc;
        if (n_last >= 2 && e->d.n * (n_last - 1) > PET_MAX_SEGS) return fail(e, CSF_E_ARG, "member %d: more than 2^30 segments in one call", (int)i);
        asks.push_back(PetAsk{e, first, n_last, &outs[i]});
    }
    for (int32_t i = 0; i < count; i++) outs[i].n_events = 0, outs[i].first_sample = -2;
    for (const PetAsk &a : asks) a.out->first_sample = a.first;
    HIPCHK(e0, hipSetDevice(e0->device));
    // (the members share one stream, and a member stepped in turn has joined its second stream back into it: stream order is enough)
    return pet_run(e0, e0->main, asks.data(), asks.size(), pet_event, nullptr);
} catch (...) { return csf_caught((engines && count > 0 ? engines[0] : nullptr)); }

int csf_pet_launches(const csf_engine *e, int64_t *n_launches) try {
    if (!e || !n_launches) return CSF_E_ARG;
    *n_launches = e->pet_launches;
    return CSF_OK;
} catch (...) { return csf_caught(e); }
