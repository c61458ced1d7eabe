// engine/abi_pet.inc - C ABI: path crossings of a recording and their post-encroachment time (csf_pet.hip).
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

extern "C++" {

constexpr int64_t PET_MAX_SEGS = 1ll << 30;     // own segments per member

using PetAsk = MeasureAsk<csf_pet_out>;

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
    return events_ok(e, who, o);
}

// ... and on a member's own segments (member < 0: the call is one engine's)
static int pet_segs_ok(csf_engine *e, const char *who, int32_t member, int64_t n_samples) {
    if (n_samples < 2 || e->d.n * (n_samples - 1) <= PET_MAX_SEGS) return CSF_OK;
    if (member < 0) return fail(e, CSF_E_ARG, "%s: more than 2^30 segments in one call", who);
    return fail(e, CSF_E_ARG, "member %d: more than 2^30 segments in one call", (int)member);
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
    const size_t header = round32(m * sizeof(unsigned long long));
    size_t total = header, scratch = 0;                        // scratch: the chunks' results, device memory behind what is transferred
    MeasureGrid grid;
    for (size_t i = 0; i < m; i++) {
        asks[i].out->n_events = 0;
        const int64_t n = asks[i].e->d.n, c = asks[i].count;
        if (n <= 0 || c < 2) {
            pet_nothing(asks[i]);
            continue;
        }
        const int64_t segs = (c - 1) * n;
        int32_t split, chunk_tiles;
        pet_split(segs, split, chunk_tiles);
        grid.add_tiles(n, (segs + PET_TILE - 1) / PET_TILE, split);
        scratch += pet_part_bytes((size_t)segs, (size_t)split);
        total += pet_block_bytes((size_t)segs, (size_t)n) + events_bytes<csf_pet_event>(asks[i].out->event_capacity);
    }
    if (!grid.any()) return CSF_OK;
    MeasureScratch<PetDesc> &g = e0->pet;
    if (int rc = measure_reserve(e0, g, st, m, total + scratch, total)) return rc;
    size_t at = header, part_at = total;
    for (size_t i = 0; i < m; i++) {
        const PetAsk &a = asks[i];
        const int64_t n = a.e->d.n;
        PetDesc r{};
        if (n > 0 && a.count >= 2) {
            const int64_t segs = (a.count - 1) * n;
            desc_ring(r, a);
            pet_split(segs, r.split, r.chunk_tiles);
            r.part_off = (int64_t)part_at, part_at += pet_part_bytes((size_t)segs, (size_t)r.split);
            r.out_off = (int64_t)at;
            at += pet_block_bytes((size_t)segs, (size_t)n);
            desc_events<csf_pet_event>(r, at, a.out->event_capacity);
        }
        g.desc.p[i] = r;
    }
    PetArgs ka{};
    ka.desc = g.desc.dev, ka.out = g.dev.p, ka.count = (unsigned long long *)g.dev.p;
    ka.pet_event = pet_event > 0.0 ? pet_event : 0.0;
    const dim3 dim = grid.dim(m);                              // (no packed members: x, y as they were added)
    if (int rc = measure_launch(e0, g, st, header, total, ps, e0->pet_launches, PET_LAUNCHES, [&](hipEvent_t t0, hipEvent_t t1) {
            launch_pet(ka, ka.pet_event > 0.0, dim, (int)m, (int)grid.max_n, st, t0, t1);
        }))
        return rc;
    const unsigned long long *found = (const unsigned long long *)g.host.p;
    for (size_t i = 0; i < m; i++) {
        const PetDesc &r = g.desc.p[i];
        csf_pet_out &o = *asks[i].out;
        if (r.n <= 0) continue;
        const size_t n = (size_t)r.n, segs = (size_t)(r.count - 1) * n;
        Cursor b{g.host.p + r.out_off};
        b.take(o.seg_pet, segs * 8), b.take(o.seg_t_own, segs * 8), b.take(o.seg_t_with, segs * 8);
        b.take(o.run_pet, n * 8), b.take(o.run_t_own, n * 8), b.take(o.run_t_with, n * 8), b.take(o.run_x, n * 8), b.take(o.run_y, n * 8);
        b.take(o.seg_with, segs * 4), b.take(o.run_with, n * 4), b.take(o.run_count, n * 4);
        take_events(o, found[i], g.host.p + r.ev_off, pet_event_less);
    }
    return CSF_OK;
}

}  // extern "C++"

int csf_post_encroachment(csf_engine *e, int64_t first_sample, int64_t n_samples, double pet_event, csf_pet_out *out) try {
    static const char *const who = "csf_post_encroachment";
    int rc = measure_open(e, who, first_sample, n_samples, out, "path", [&] { return pet_args_ok(e, who, pet_event, out); });
    if (rc) return rc;
    if ((rc = pet_segs_ok(e, who, -1, n_samples))) return rc;
    out->first_sample = first_sample;
    PetAsk ask{e, first_sample, n_samples, out};
    csf_engine::ProfSlot *ps = nullptr;
    if ((rc = prof_take(e, e->d.n > 0 && n_samples >= 2, &ps))) return rc;
    return pet_run(e, e->main, &ask, 1, pet_event, ps);
} catch (...) { return csf_caught(e); }

int csf_batch_post_encroachment(csf_engine *const *engines, int32_t count, int64_t n_last, double pet_event, csf_pet_out *outs) try {
    static const char *const who = "csf_batch_post_encroachment";
    int rc = batch_open(engines, count, who, outs);
    if (rc) return rc;
    csf_engine *e0 = engines[0];
    if ((rc = batch_sizes_ok(e0, who, n_last, count))) return rc;
    std::vector<PetAsk> asks;
    rc = batch_members(engines, count, who, n_last, outs, asks,
                       [&](csf_engine *e, int32_t i) { return pet_args_ok(e, who, pet_event, &outs[i]); },
                       [&](csf_engine *e, int32_t i) { return pet_segs_ok(e, who, i, n_last); });
    if (rc) return rc;
    if ((rc = batch_device(e0))) return rc;
    return pet_run(e0, e0->main, asks.data(), asks.size(), pet_event, nullptr);
} catch (...) { return csf_caught((engines && count > 0 ? engines[0] : nullptr)); }

int csf_pet_launches(const csf_engine *e, int64_t *n_launches) try {
    return measure_launches(e, n_launches, &csf_engine::pet_launches);
} catch (...) { return csf_caught(e); }
