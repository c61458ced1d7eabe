// engine/measure.inc - what the measures of a recording share on the host: the route of a call from the ask to the caller's arrays.
// (a section of csf_engine.hip: included there, in this order, ahead of the abi_*.inc of the measures; not a translation unit of its own)
//
// A call checks (measure_open, or batch_open .. batch_members: every refusal before anything is written), plans the packed output
// and the grid (MeasureGrid), reserves (measure_reserve), fills one descriptor per member (desc_ring, desc_events), clears, launches,
// copies and waits once (measure_launch), and unpacks (Cursor, take_events).  A measure's own file holds what it alone has.

extern "C++" {

constexpr int64_t ENC_MAX_SAMPLES = 65535;      // samples per call (the grid's y extent)
constexpr int64_t ENC_MAX_CELLS = 1ll << 31;    // (sample, road user) cells per member

// what one engine is asked: samples [first, first + count) of its ring, or (first == -1; encounters and body only) its current state
template <class Out>
struct MeasureAsk {
    csf_engine *e;
    int64_t first, count;
    Out *out;
};

template <class Out>
static int64_t enc_population(const MeasureAsk<Out> &a) { return a.first < 0 ? (int64_t)a.e->order.size() : a.e->d.n; }

static size_t round32(size_t bytes) { return (bytes + 31) & ~(size_t)31; }

// the refusals that depend on the engine alone
static int encounter_engine_ok(csf_engine *e, const char *who) {
    if (int crc = calib_refuses(e, who)) return crc;
    if (e->world > 1 || e->loopback || e->nccl != nullptr || !e->state_all_current)
        return fail(e, CSF_E_STATE, "%s: the engine is a rank of a sharded run or a member of a loopback group - the other ranks' road users have no fp64 state here", who);
    return CSF_OK;
}

// ... and on the room a member gives for events
template <class Out>
static int events_ok(csf_engine *e, const char *who, const Out *o) {
    if (o->event_capacity < 0) return fail(e, CSF_E_ARG, "%s: event_capacity = %lld", who, (long long)o->event_capacity);
    if (o->event_capacity > 0 && !o->events) return fail(e, CSF_E_ARG, "%s: room for %lld events is given, but events is NULL", who, (long long)o->event_capacity);
    return CSF_OK;
}

// ... and on the cells of a member (member < 0: the call is one engine's)
static int cells_ok(csf_engine *e, const char *who, int32_t member, int64_t cells) {
    if (cells <= ENC_MAX_CELLS) return CSF_OK;
    if (member < 0) return fail(e, CSF_E_ARG, "%s: more than 2^31 (sample, road user) cells in one call", who);
    return fail(e, CSF_E_ARG, "member %d: more than 2^31 (sample, road user) cells in one call", (int)member);
}

// The opening of a single engine's call: the refusals in their order - args_ok() the measure's own -, then the engine brought up to
// date and the samples found in the ring.  lacks: what the current state lacks for this measure ("path", ...); NULL: the current state,
// first_sample -1 with one sample, can be covered too (encounters, body), in the population order with pending arrivals brought in.
template <class Out, class Check>
static int measure_open(csf_engine *e, const char *who, int64_t first_sample, int64_t n_samples, const Out *out, const char *lacks, Check args_ok) {
    if (!e) return CSF_E_ARG;
    if (!out) return fail(e, CSF_E_ARG, "%s: out is NULL", who);
    int rc = args_ok();
    if (rc) return rc;
    if (n_samples < 0 || n_samples > ENC_MAX_SAMPLES) return fail(e, CSF_E_ARG, "%s: n_samples = %lld (0 .. 65535)", who, (long long)n_samples);
    if (lacks && first_sample < 0)
        return fail(e, CSF_E_ARG, "%s: first_sample = %lld (the current state, -1, has no %s: a window of the state ring is needed)", who, (long long)first_sample, lacks);
    if (first_sample < -1 || (first_sample == -1 && n_samples > 1))
        return fail(e, CSF_E_ARG, "%s: first_sample = %lld, n_samples = %lld (the current state is first_sample -1 with one sample)", who,
                    (long long)first_sample, (long long)n_samples);
    if ((rc = encounter_engine_ok(e, who))) return rc;
    if (first_sample >= 0 && !e->d.hist)
        return fail(e, CSF_E_STATE, "%s: no state ring (csf_record, csf_enable_history)%s", who, lacks ? "" : " - only the current state, first_sample -1, can be covered");
    HIPCHK(e, hipSetDevice(e->device));
    if ((rc = upload_all(e))) return rc;
    if ((rc = csf_sync(e))) return rc;                         // both streams (the side-by-side tick), as the read-backs wait
    return first_sample >= 0 ? record_range(e, first_sample, n_samples) : sync_order(e);
}

// The opening of a batch's call, in three steps between which a measure puts the checks of what its members share.  First the engines
// and the outputs ...
template <class Out>
static int batch_open(csf_engine *const *engines, int32_t count, const char *who, const Out *outs) {
    if (int rc = batch_check(engines, count)) return rc;
    if (!outs) return fail(engines[0], CSF_E_ARG, "%s: outs is NULL", who);
    return CSF_OK;
}

// ... then the samples and the members (the grid's y and z extents; clearance, whose members take several z each, has its own second half) ...
static int batch_n_last_ok(csf_engine *e0, const char *who, int64_t n_last) {
    if (n_last < 0 || n_last > ENC_MAX_SAMPLES) return fail(e0, CSF_E_ARG, "%s: n_last = %lld (0 .. 65535)", who, (long long)n_last);
    return CSF_OK;
}
static int batch_sizes_ok(csf_engine *e0, const char *who, int64_t n_last, int32_t count) {
    if (int rc = batch_n_last_ok(e0, who, n_last)) return rc;
    if (count > 65535) return fail(e0, CSF_E_ARG, "%s: at most 65535 engines in one call (%d given)", who, (int)count);
    return CSF_OK;
}

// ... then member by member: out_ok(e, i) the measure's check of the member's outputs, ring_ok(e, i) of what else it reads of a member
// that records, fits(e, i) its limit on the member's size.  A member without a ring is no ask: its first_sample stays -2.  Every
// refusal comes before anything is written; the caller then marks what else its outputs count and takes the device (batch_device).
template <class Out, class OutOk, class RingOk, class Fits>
static int batch_members(csf_engine *const *engines, int32_t count, const char *who, int64_t n_last, Out *outs, std::vector<MeasureAsk<Out>> &asks,
                         OutOk out_ok, RingOk ring_ok, Fits fits) {
    asks.reserve((size_t)count);
    for (int32_t i = 0; i < count; i++) {
        csf_engine *e = engines[i];
        int rc = out_ok(e, i);
        if (rc) return rc;
        if ((rc = encounter_engine_ok(e, who))) return rc;
        if (!e->d.hist) continue;
        if ((rc = ring_ok(e, i))) return rc;
        int64_t first = 0;
        if ((rc = record_last(e, i, n_last, &first))) return rc;
        if ((rc = fits(e, i))) return rc;
        asks.push_back(MeasureAsk<Out>{e, first, n_last, &outs[i]});
    }
    for (int32_t i = 0; i < count; i++) outs[i].n_events = 0, outs[i].first_sample = -2;
    for (const MeasureAsk<Out> &a : asks) a.out->first_sample = a.first;
    return CSF_OK;
}
template <class Out, class OutOk, class Fits>
static int batch_members(csf_engine *const *engines, int32_t count, const char *who, int64_t n_last, Out *outs, std::vector<MeasureAsk<Out>> &asks,
                         OutOk out_ok, Fits fits) {
    return batch_members(engines, count, who, n_last, outs, asks, out_ok, [](csf_engine *, int32_t) { return CSF_OK; }, fits);
}

// the device of a batch's first member, whose stream the launches go to
// (the members share one stream, and a member stepped in turn has joined its second stream back into it: stream order is enough)
static int batch_device(csf_engine *e0) {
    HIPCHK(e0, hipSetDevice(e0->device));
    return CSF_OK;
}

// The grid of a measure's first launch: x, y the largest member's, z = members.  A member of n > ENC_SMALL road users takes tiles of 256
// of them in x and its rows (samples or stations, times the workgroups that share a row's partners) in y; a smaller one packs
// 256 / n rows into a workgroup, and the packed members take the plane x * y.
struct MeasureGrid {
    int64_t gx = 1, gy = 1, plane = 0, max_n = 0;
    void add(int64_t n, int64_t rows, int64_t split = 1) {
        max_n = std::max(max_n, n);
        if (n <= ENC_SMALL) {
            const int64_t spw = 256 / n;
            plane = std::max(plane, (rows + spw - 1) / spw);
        } else {
            gx = std::max(gx, (n + 255) / 256);
            gy = std::max(gy, rows * split);
        }
    }
    // a member that has its own shape (PET: tiles of own segments, the workgroups that share a tile's partners)
    void add_tiles(int64_t n, int64_t tiles, int64_t split) { max_n = std::max(max_n, n), gx = std::max(gx, tiles), gy = std::max(gy, split); }
    bool any() const { return max_n > 0; }                     // (a member is added only with n > 0)
    dim3 dim(size_t z) {
        if (gx * gy < plane) {                                 // the packed members take the plane x * y (plane <= 65535 rows)
            if (gx == 1 && gy == 1) gx = plane;
            else gy = (plane + gx - 1) / gx;
        }
        return dim3((unsigned)gx, (unsigned)gy, (unsigned)z);
    }
};

// room for m descriptors, dev_bytes on the device (the packed output, and the scratch behind it) and host_bytes of it on the host
template <class Desc>
static int measure_reserve(csf_engine *e0, MeasureScratch<Desc> &g, hipStream_t st, size_t m, size_t dev_bytes, size_t host_bytes) {
    HIPCHK(e0, g.desc.reserve(m, st, 16));
    HIPCHK(e0, g.dev.reserve(dev_bytes));
    HIPCHK(e0, g.host.reserve(host_bytes, st, 4096));
    return CSF_OK;
}

// a member's samples in its ring, for its descriptor
template <class Desc, class Out>
static void desc_ring(Desc &r, const MeasureAsk<Out> &a) {
    const Dev &d = a.e->d;
    r.n = (int32_t)d.n, r.ns = d.ns, r.count = (int32_t)a.count;
    r.s = d.hist, r.cap = d.hist_cap, r.first = (int32_t)(a.first % d.hist_cap);
}

// ... or its current state (encounters, body)
template <class Out>
static void desc_ring_or_state(EncDesc &r, const MeasureAsk<Out> &a, int64_t n) {
    const Dev &d = a.e->d;
    if (a.first >= 0) desc_ring(r, a), r.ring = 1, r.first_abs = a.first;
    else r.n = (int32_t)n, r.ns = d.ns, r.count = (int32_t)a.count, r.ring = 0, r.s = d.s, r.order = d.order, r.stride = d.cap, r.first_abs = -1, r.cap = 1, r.first = 0;
}

// ... and its events at `at`, which moves behind them; whole: the area is rounded up to 32 bytes (flow, clearance)
template <class Event>
static size_t events_bytes(int64_t capacity, bool whole = false) {
    const size_t bytes = (size_t)capacity * sizeof(Event);
    return whole ? round32(bytes) : bytes;
}
template <class Event, class Desc>
static void desc_events(Desc &r, size_t &at, int64_t capacity, bool whole = false) {
    r.ev_off = (int64_t)at, r.ev_cap = capacity;
    at += events_bytes<Event>(capacity, whole);
}

// The first `cleared` bytes of the packed output zeroed (the counters lead it), the measure's `launches` launches - launch(t0, t1), with
// the events of the profile slot around the first -, then `moved` bytes copied to the host and one wait.
template <class Desc, class Launch>
static int measure_launch(csf_engine *e0, MeasureScratch<Desc> &g, hipStream_t st, size_t cleared, size_t moved, csf_engine::ProfSlot *ps,
                          int64_t &counter, int launches, Launch launch) {
    HIPCHK(e0, hipMemsetAsync(g.dev.p, 0, cleared, st));
    launch(ps ? ps->ev[0] : nullptr, ps ? ps->ev[1] : nullptr);
    if (ps) ps->pair = true;
    counter += launches;
    HIPCHK(e0, hipGetLastError());
    HIPCHK(e0, hipMemcpyAsync(g.host.p, g.dev.p, moved, hipMemcpyDeviceToHost, st));
    HIPCHK(e0, hipStreamSynchronize(st));
    return CSF_OK;
}

// a walk over a block of the packed output: array after array into the caller's, where the caller wants it
struct Cursor {
    const unsigned char *b;
    void take(void *dst, size_t bytes, size_t room) {          // `bytes` of the `room` the array has in the block
        if (dst && bytes) std::memcpy(dst, b, bytes);
        b += room;
    }
    void take(void *dst, size_t bytes) { take(dst, bytes, bytes); }
};

// A member's events: `found` of them, of which the first event_capacity were stored at src; fix(event) puts right what the kernel
// could not know.  They are sorted only when all of them fitted (else the caller asks again with room for all).
template <class Out, class Less, class Fix>
static void take_events(Out &o, unsigned long long found, const unsigned char *src, Less less, Fix fix) {
    o.n_events = (int64_t)found;
    const int64_t stored = std::min(o.n_events, o.event_capacity);
    if (stored <= 0) return;
    std::memcpy(o.events, src, (size_t)stored * sizeof(*o.events));
    for (int64_t k = 0; k < stored; k++) fix(o.events[k]);
    if (o.n_events <= o.event_capacity) std::sort(o.events, o.events + stored, less);
}
template <class Out, class Less>
static void take_events(Out &o, unsigned long long found, const unsigned char *src, Less less) {
    take_events(o, found, src, less, [](decltype(*o.events) &) {});
}

// the kernel numbers samples within the call: as csf_get_record numbers them (encounters, body; -1: the current state)
template <class Event>
static void event_sample_abs(Event &ev, int64_t first_abs) { ev.sample = first_abs < 0 ? -1 : first_abs + ev.sample; }

static int measure_launches(const csf_engine *e, int64_t *n_launches, int64_t csf_engine::*counter) {
    if (!e || !n_launches) return CSF_E_ARG;
    *n_launches = e->*counter;
    return CSF_OK;
}

}  // extern "C++"
