// engine/abi_batch.inc - C ABI: batches of independent scenes (csf_batch_join, csf_step_batch, csf_step_batch_get_tick).
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)
//
// A junction of a SUMO network or one run of a parameter sweep is a handful of road users: one wave of the one-wave tick
// (csf_agent.hip: small_tick_kernel), and its launch is nearly all latency.  The members of a batch that this tick takes
// (small_fused_ok) are stepped by small_batch_kernel instead - one launch per vehicle class present, workgroup b ticking the scene
// of table[b], and with csf_small_classes on one further launch of small_classes_batch_kernel (csf_small_classes.hip) for all members
// of several parameter sets or classes - and every other member by step_impl in turn.  The table holds the members' Dev records in
// device memory; it is renewed in stream order, and only where a member's Dev changed since it was last copied (a host shadow, memcmp).  Per-call
// values stay out of it: whether the read-back is packed is a kernel argument, and Dev::tick - what the samples of a recording
// (csf_record) are numbered from - is 0 in the table: a recording member's count is a word of its own in device memory
// (Dev::rec_tick) that the launch reads and moves on itself.  The host knows what the word holds (csf_engine::rec_tick_dev) and
// writes it in stream order only where the engine has ticked outside the batched launch since.
//
// Mid-size members - those the one-launch tick takes (tick.inc: mid_fused_ok), without a road or with one that the launch sums itself
// (tick.inc: mid_road_ok - csf_mid_road on, no lattice, at most MID_ROAD_MAX vertices; any other road is a launch of its own per tick:
// such members stay in turn), without wave traces, with nothing pending, and at least two of them - are stepped together too: tick by
// tick, one launch of mid_batch_kernel (csf_mid.hip) per vehicle class, priority rule and with / without road present.  Their
// Dev differs on every tick (the halves of the double buffers trade places, tick, stamp, rounding bands), so a second table holds
// each member's Dev in a form that does not (mid_canon), renewed like the first one, and the kernel composes the tick's Dev from
// it and the member's MidTick (csf_dev.h: 48 bytes).  The host knows these records in advance: it writes them for a STRETCH of
// ticks - up to MID_STRETCH, ending in front of the next tick on which some member re-bins or measures its coordinate bound
// again - into pinned staging, copies them in one go and enqueues the stretch's launches.  Per tick that is O(members) host
// work and 48 bytes per member.  The periodic work of the stretch's first tick - the re-binning on the plain order, the copy into
// the other halves - runs for all members that are due in one launch each (csf_bin.hip: rebase_batch_kernel ...); its host side
// stays per member (binning.inc: rebin).  A member that stops qualifying behind a re-binning finishes the call in turn.
// The host books the ticks of a stretch (halves traded, counters, tick) BEFORE the stretch is enqueued.  An error return in
// between - a failed HIP call - therefore leaves the mid-size members of the batch ahead of the device by up to a stretch: such
// an error is not a refusal, and the members' states are not a simulation after it; they are to be uploaded again (csf_push_state)
// or destroyed.

extern "C++" {

struct BatchState {
    int device = 0;
    std::vector<csf_engine *> members;           // join order
    DevBuf<Dev> table;                           // the one-wave members' Dev records, grouped by vehicle class
    HostBuf<Dev, false> stage;                   // what the copies into `table` read
    std::vector<Dev> shadow;                     // what `table` holds, slot by slot (valid where `held`)
    std::vector<uint8_t> held;
    hipEvent_t copied = nullptr;                 // recorded behind the last copy from `stage`
    bool copy_pending = false;
    // per call (kept to spare the allocations)
    std::vector<int32_t> small, rest;            // members the one-wave launch takes / that are stepped in turn
    std::vector<uint8_t> snapped;                // per member: its read-back is in its mapped snapshot buffer (1: packed by the
                                                 // batched launch, 2: by its own one-wave launch), 0: not
    std::vector<int32_t> slot_member;            // table slot -> member
    // mid-size members: their Dev records in canonical form (table slot = place in `mid` at the call's start), the workgroups of a
    // tick (slot, group within the member) sorted by launch, the tick records of a stretch
    std::vector<int32_t> mid;                    // members the batched one-launch tick takes, by launch (class, priority rule)
    std::vector<uint8_t> mid_out;                // per slot: the member left the batched tick in mid-call
    DevBuf<Dev> mtable;
    HostBuf<Dev, false> mstage;
    std::vector<Dev> mshadow;
    std::vector<uint8_t> mheld;
    hipEvent_t mcopied = nullptr;
    bool mcopy_pending = false;
    DevBuf<int2> mgroups;
    HostBuf<int2, false> mgroups_stage;
    std::vector<int2> mgroups_now, mgroups_dev;  // what this call wants / what the device holds
    struct MidLaunch { int model, p2r, road, beg, end; };    // (road: the ROAD instance - members without a road keep their kernel)
    std::vector<MidLaunch> mlaunch;
    DevBuf<MidTick> mticks;                      // [MID_STRETCH][members]
    HostBuf<MidTick, false> mticks_stage;        // two of them, used in turn
    hipEvent_t mticked[2] = {nullptr, nullptr};
    bool mticked_pending[2] = {false, false};
    unsigned mstretch = 0;
    int64_t launches = 0;                        // csf_batch_launches
    RecGather rgather;                           // csf_batch_get_record
    std::vector<RecAsk> asks;
    ~BatchState() {   // (the last copy from `stage` has ended before the members below go, `stage` among them)
        (void)hipSetDevice(device);
        if (copy_pending && copied) (void)hipEventSynchronize(copied);
        if (copied) (void)hipEventDestroy(copied);
        if (mcopy_pending && mcopied) (void)hipEventSynchronize(mcopied);
        if (mcopied) (void)hipEventDestroy(mcopied);
        for (int h = 0; h < 2; h++) {
            if (mticked_pending[h] && mticked[h]) (void)hipEventSynchronize(mticked[h]);
            if (mticked[h]) (void)hipEventDestroy(mticked[h]);
        }
    }
};
constexpr int MID_STRETCH = 64;   // ticks whose records one copy carries at most (CSF_REBIN_TICKS' default: a stretch per re-binning)

// Every member goes back to its own stream, and the batch's table, staging and event go with the last reference to it.
static int batch_dissolve(csf_engine *e) {
    std::shared_ptr<BatchState> b = e->batch;
    if (!b) return CSF_OK;
    (void)hipSetDevice(b->device);
    int rc = CSF_OK;
    if (e->main && hipStreamSynchronize(e->main) != hipSuccess) rc = fail(e, CSF_E_DEVICE, "hipStreamSynchronize failed while the batch was dissolved");
    for (csf_engine *m : b->members) {
        if (m->own_hold) {
            m->main_hold = m->own_hold;
            m->main = m->main_hold->s;
            m->own_hold.reset();
        }
        m->batch.reset();
    }
    return rc;
}

// `engines` is exactly a batch, in join order
static int batch_check(csf_engine *const *engines, int32_t count) {
    if (!engines || count < 1) return CSF_E_ARG;
    for (int32_t i = 0; i < count; i++)
        if (!engines[i]) return CSF_E_ARG;
    csf_engine *e0 = engines[0];
    for (int32_t i = 0; i < count; i++)
        if (!engines[i]->batch) return fail(engines[i], CSF_E_STATE, "engine is not in a batch (csf_batch_join)");
    const std::vector<csf_engine *> &m = e0->batch->members;
    if ((size_t)count != m.size()) return fail(e0, CSF_E_ARG, "the batch has %zu members, %d were given", m.size(), (int)count);
    for (int32_t i = 0; i < count; i++)
        if (engines[i] != m[(size_t)i]) return fail(engines[i], CSF_E_ARG, "the engines must be the batch's members in join order");
    return CSF_OK;
}

// The table <- the Dev records of the one-wave members, grouped by class; copied in stream order where they changed.
static int batch_table(BatchState &b, hipStream_t st) {
    const size_t k = b.slot_member.size();                      // (<= members: the table, staging and shadow were sized at the join)
    size_t run0 = 0, runs = 0;
    bool waited = false;
    auto flush = [&](size_t end) -> int {
        if (end > run0) {
            HIPCHK(b.members[0], hipMemcpyAsync(b.table.p + run0, b.stage.p + run0, (end - run0) * sizeof(Dev), hipMemcpyHostToDevice, st));
            runs++;
            b.launches++;
        }
        return CSF_OK;
    };
    bool in_run = false;
    for (size_t j = 0; j < k; j++) {
        const csf_engine *e = b.members[(size_t)b.slot_member[j]];
        Dev dd;
        std::memcpy((void *)&dd, (const void *)&e->d, sizeof(Dev));
        dd.tick = 0;                                              // (per call; a recording counts in Dev::rec_tick)
        dd.snap = (e->d.order == nullptr && e->snap.dev != nullptr && e->snap.n >= snap_need(e)) ? (double *)e->snap.dev : nullptr;
        const bool same = b.held[j] && std::memcmp((const void *)&b.shadow[j], (const void *)&dd, sizeof(Dev)) == 0;
        if (same) {
            if (in_run) {
                int rc = flush(j);
                if (rc) return rc;
                in_run = false;
            }
            continue;
        }
        if (!waited && b.copy_pending) {                          // (an earlier copy may still read the staging memory)
            HIPCHK(b.members[0], hipEventSynchronize(b.copied));
            b.copy_pending = false;
        }
        waited = true;
        std::memcpy((void *)&b.stage.p[j], (const void *)&dd, sizeof(Dev));
        std::memcpy((void *)&b.shadow[j], (const void *)&dd, sizeof(Dev));
        b.held[j] = 1;
        if (!in_run) run0 = j, in_run = true;
    }
    if (in_run) {
        int rc = flush(k);
        if (rc) return rc;
    }
    if (runs > 0) {
        HIPCHK(b.members[0], hipEventRecord(b.copied, st));
        b.copy_pending = true;
    }
    return CSF_OK;
}

// ---- mid-size members ---------------------------------------------------------------------------------------------------------
// could the batched one-launch tick take this member (behind upload_all and the calibration)?
static bool batch_mid_ok(const csf_engine *e) {
    return e->knobs.batch_mid != 0 && mid_fused_ok(e) && (e->d.nv == 0 || mid_road_ok(e)) && e->d.atrace == nullptr && e->pend.empty() && !e->dirty;
}

// The launch a member belongs to, beside its priority rule and with / without road: its vehicle class, or 7 - "classes kernel" - for
// a member of several sets or classes (mid_classes_batch_kernel: ONE launch whatever the members' classes, as the one-wave members'
// small_takes_classes ? 7 : model below).
static int mid_launch_key(const csf_engine *e) { return mid_takes_classes(e) ? 7 : e->d.p.model; }

// A member's Dev as the table holds it: what enqueue_mid_tick's launch sees, but for what changes from tick to tick - the halves
// by name, not by role; tick, stamp and bands zero (csf_dev.h: mid_compose puts them in) - and the flags that say which halves
// this tick reads.
static uint32_t mid_canon(const csf_engine *e, Dev &dd) {
    std::memcpy((void *)&dd, (const void *)&e->d, sizeof(Dev));
    uint32_t fl = 0;
    if (e->d.rec != e->rec.p) fl |= MID_SWAP_REC;
    if (e->d.recg != e->recg.p) fl |= MID_SWAP_RECG;
    if (e->d.rec2 != e->rec2.p) fl |= MID_SWAP_REC2;
    if (!e->mid_cur_is_a) fl |= MID_SWAP_SRC64;
    dd.rec = e->rec.p, dd.rec_w = e->rec_alt.p;
    dd.recg = e->recg.p, dd.recg_w = e->recg_alt.p;
    dd.rec2 = e->rec2.p, dd.rec2_w = e->rec2_alt.p;
    dd.src64 = e->src64_a.p, dd.src64_w = e->src64_b.p;
    dd.mid_group = mid_group_for(e);
    dd.tick = 0;
    dd.edge_stamp = 0;
    dd.pc.fovA = dd.pc.fovB = dd.pc.sideA = dd.pc.sideB = dd.pc.fovT0 = dd.pc.fovT1 = 0.0f;
    return fl;
}

// the table's slot j <- member's Dev where it changed (one copy per slot: members change one at a time, at their re-binnings)
static int mid_table_slot(BatchState &b, size_t j, const Dev &dd, bool *waited, bool *copied) {
    if (b.mheld[j] && std::memcmp((const void *)&b.mshadow[j], (const void *)&dd, sizeof(Dev)) == 0) return CSF_OK;
    if (!*waited && b.mcopy_pending) {                            // (an earlier copy may still read the staging memory)
        HIPCHK(b.members[0], hipEventSynchronize(b.mcopied));
        b.mcopy_pending = false;
    }
    *waited = true;
    std::memcpy((void *)&b.mstage.p[j], (const void *)&dd, sizeof(Dev));
    std::memcpy((void *)&b.mshadow[j], (const void *)&dd, sizeof(Dev));
    b.mheld[j] = 1;
    *copied = true;
    return CSF_OK;
}

// ... and the copies: one per run of changed slots
static int mid_table_flush(BatchState &b, const std::vector<uint8_t> &changed, hipStream_t st) {
    const size_t k = changed.size();
    bool any = false;
    for (size_t j = 0; j < k;) {
        if (!changed[j]) {
            j++;
            continue;
        }
        size_t end = j;
        while (end < k && changed[end]) end++;
        HIPCHK(b.members[0], hipMemcpyAsync(b.mtable.p + j, b.mstage.p + j, (end - j) * sizeof(Dev), hipMemcpyHostToDevice, st));
        b.launches++;
        any = true;
        j = end;
    }
    if (any) {
        HIPCHK(b.members[0], hipEventRecord(b.mcopied, st));
        b.mcopy_pending = true;
    }
    return CSF_OK;
}

// the workgroups of a tick, launch by launch: (slot, group) of every group of every member that is still in; copied where the
// list differs from what the device holds
static int mid_groups(BatchState &b, csf_engine *const *engines, hipStream_t st) {
    csf_engine *e0 = b.members[0];
    b.mgroups_now.clear();
    b.mlaunch.clear();
    for (size_t j = 0; j < b.mid.size(); j++) {
        if (b.mid_out[j]) continue;
        const csf_engine *e = engines[b.mid[j]];
        const int model = mid_launch_key(e), p2r = e->d.p.priority_rule == CSF_P2R ? 1 : 0, road = e->d.nv > 0 ? 1 : 0;
        if (b.mlaunch.empty() || b.mlaunch.back().model != model || b.mlaunch.back().p2r != p2r || b.mlaunch.back().road != road)
            b.mlaunch.push_back({model, p2r, road, (int)b.mgroups_now.size(), (int)b.mgroups_now.size()});
        const int G = mid_group_for(e), groups = (int)((e->d.hi - e->d.lo + G - 1) / G);
        for (int g = 0; g < groups; g++) b.mgroups_now.push_back(make_int2((int)j, g));
        b.mlaunch.back().end = (int)b.mgroups_now.size();
    }
    const size_t n = b.mgroups_now.size();
    if (n == b.mgroups_dev.size() && (n == 0 || std::memcmp(b.mgroups_now.data(), b.mgroups_dev.data(), n * sizeof(int2)) == 0)) return CSF_OK;
    if (b.mgroups.n < n || b.mgroups_stage.n < n) {              // (allocations synchronise: membership changed)
        HIPCHK(e0, hipStreamSynchronize(st));
        HIPCHK(e0, b.mgroups.alloc(2 * n));
        HIPCHK(e0, b.mgroups_stage.alloc(2 * n));
    } else {
        HIPCHK(e0, hipStreamSynchronize(st));                     // (the last copy from the staging memory; once per change of membership)
    }
    std::memcpy(b.mgroups_stage.p, b.mgroups_now.data(), n * sizeof(int2));
    HIPCHK(e0, hipMemcpyAsync(b.mgroups.p, b.mgroups_stage.p, n * sizeof(int2), hipMemcpyHostToDevice, st));
    b.launches++;
    b.mgroups_dev = b.mgroups_now;
    return CSF_OK;
}

// a member that the batched tick no longer takes (behind mid_prelude: this tick's bounds are in place): what was deferred is
// enqueued for it alone, and it finishes the call in turn
static int mid_leave(csf_engine *e, int64_t ticks_left) {
    e->mid_defer = false;
    if (e->mid_deferred & MID_DUE_REBIN) {
        launch_identity_perm(e->d, e->main);
        launch_rebase(e->d, e->main);
    }
    if (e->mid_deferred & MID_DUE_SYNC) e->mid_synced = false;
    e->mid_deferred = 0;
    int rc = enqueue_two_launch_tick(e, true);
    for (int64_t t = 1; t < ticks_left && !rc; t++) rc = enqueue_tick(e, ticks_left - t);
    if (!rc) rc = chase_join(e);
    if (e->cal_phase >= 1 && e->cal_phase <= 3) e->cal_phase = 0;  // (as step_impl: a measurement does not span calls)
    e->device_ahead = true;                                        // (it has ticked, whatever the batch does with the others)
    return rc;
}

// n_ticks ticks of the members in b.mid (at least two; batch_mid_ok held for each when the call began)
static int step_batch_mid(BatchState &b, csf_engine *const *engines, int64_t n_ticks) {
    csf_engine *e0 = b.members[0];
    hipStream_t st = e0->main;
    const size_t k = b.mid.size(), cap = b.members.size();
    int rc;
    // everything that allocates (and so synchronises) in front of the tick loop
    if (b.mtable.n < cap) {
        HIPCHK(e0, b.mtable.alloc(cap));
        HIPCHK(e0, b.mstage.alloc(cap));
        HIPCHK(e0, b.mticks.alloc(cap * MID_STRETCH));
        HIPCHK(e0, b.mticks_stage.alloc(2 * cap * MID_STRETCH));
        HIPCHK(e0, hipEventCreateWithFlags(&b.mcopied, hipEventDisableTiming));
        for (hipEvent_t &ev : b.mticked) HIPCHK(e0, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        b.mshadow.resize(cap);
        b.mheld.assign(cap, 0);
    }
    for (int32_t i : b.mid) {
        csf_engine *e = engines[i];
        if ((rc = chase_join(e))) return rc;
        if ((rc = alt_alloc(e))) return rc;
    }
    // by launch: vehicle class, then priority rule, then without / with a road (batch_mid_ok: a road here is one the launch sums);
    // join order within
    std::stable_sort(b.mid.begin(), b.mid.end(), [&](int32_t x, int32_t y) {
        const Dev &dx = engines[x]->d, &dy = engines[y]->d;
        const int px = dx.p.priority_rule == CSF_P2R, py = dy.p.priority_rule == CSF_P2R;
        const int rx = dx.nv > 0, ry = dy.nv > 0;
        const int kx = mid_launch_key(engines[x]), ky = mid_launch_key(engines[y]);
        return kx != ky ? kx < ky : px != py ? px < py : rx < ry;
    });
    b.mid_out.assign(k, 0);
    struct Defer {   // (the members go back to enqueueing their own periodic launches on every way out)
        BatchState &b;
        csf_engine *const *engines;
        ~Defer() {
            for (int32_t i : b.mid) engines[i]->mid_defer = false;
        }
    } guard{b, engines};
    for (int32_t i : b.mid) engines[i]->mid_defer = true, engines[i]->mid_deferred = 0;
    bool regroup = true;
    std::vector<uint8_t> changed(k, 0);
    std::vector<OtherHalves> halves(k);
    for (int64_t t = 0; t < n_ticks;) {
        // the stretch's first tick: whatever is periodic - re-binning, a coordinate bound measured again, halves made equal
        std::fill(changed.begin(), changed.end(), 0);
        const unsigned h = b.mstretch++ & 1u;
        if (b.mticked_pending[h]) {                               // (the copy of the stretch before last read this staging half)
            HIPCHK(e0, hipEventSynchronize(b.mticked[h]));
            b.mticked_pending[h] = false;
        }
        MidTick *const stage = b.mticks_stage.p + (size_t)h * cap * MID_STRETCH;
        bool waited = false;
        uint32_t due = 0;
        int64_t max_n_pad = 0, max_sync = 0;
        size_t in = 0;
        auto tick_of = [&](size_t j, int64_t row, bool head) -> int {
            csf_engine *e = engines[b.mid[j]];
            bool take = false;
            int rc2 = mid_prelude(e, &take);
            if (rc2) return rc2;
            Dev dd;
            uint32_t fl = 0;
            if (take) {
                fl = mid_canon(e, dd);
                take = mid_shape_ok(dd);
            }
            if (!take && !head) return fail(e, CSF_E_STATE, "a member of the batched one-launch tick changed inside a stretch of ticks");
            if (!take) {                                          // (only ever on a stretch's first tick: nothing else changes a Dev)
                b.mid_out[j] = 1;
                regroup = true;
                stage[(size_t)row * k + j] = MidTick{};
                return mid_leave(e, n_ticks - t);
            }
            if (!head && std::memcmp((const void *)&b.mshadow[j], (const void *)&dd, sizeof(Dev)) != 0)
                return fail(e, CSF_E_STATE, "a member of the batched one-launch tick changed inside a stretch of ticks");
            if (head) {
                bool cp = false;
                if ((rc2 = mid_table_slot(b, j, dd, &waited, &cp))) return rc2;
                changed[j] = cp;
            }
            MidTick &m = stage[(size_t)row * k + j];
            m.tick = e->d.tick;
            m.edge_stamp = e->d.edge_stamp;
            m.flags = fl | e->mid_deferred;
            const PairConsts &pc = e->d.pc;
            m.fovA = pc.fovA, m.fovB = pc.fovB, m.sideA = pc.sideA, m.sideB = pc.sideB, m.fovT0 = pc.fovT0, m.fovT1 = pc.fovT1;
            m.nrecg = (int32_t)std::min((size_t)e->d.n_pad, e->recg.n);
            m.pad = 0;
            if (e->mid_deferred) {
                due |= e->mid_deferred;
                max_n_pad = std::max(max_n_pad, e->d.n_pad);
                max_sync = std::max(max_sync, std::max<int64_t>(e->d.n_pad, 3 * e->d.cap));
                e->mid_deferred = 0;
            }
            mid_ticked(e, other_halves(e), true, e->d.nv > 0, mid_takes_classes(e));
            e->device_ahead = true;
            return CSF_OK;
        };
        for (size_t j = 0; j < k; j++) {
            if (b.mid_out[j]) {                                   // (its slot asks for nothing)
                stage[j] = MidTick{};
                continue;
            }
            if ((rc = tick_of(j, 0, true))) return rc;
            if (!b.mid_out[j]) in++;
        }
        if (in == 0) return CSF_OK;                               // (every member left: each has finished the call in turn)
        // ... and the ticks behind it, up to the next one on which a member has periodic work
        int64_t T = 1;
        for (; T < MID_STRETCH && t + T < n_ticks; T++) {
            bool quiet = true;
            for (size_t j = 0; j < k && quiet; j++) {
                if (b.mid_out[j]) continue;
                const csf_engine *e = engines[b.mid[j]];
                quiet = !rebin_due(e) && e->mid_synced && !e->bound_stale;
            }
            if (!quiet) break;
            for (size_t j = 0; j < k; j++) {
                if (b.mid_out[j]) continue;
                if ((rc = tick_of(j, T, false))) return rc;
            }
        }
        if ((rc = mid_table_flush(b, changed, st))) return rc;
        if (regroup && (rc = mid_groups(b, engines, st))) return rc;
        regroup = false;
        HIPCHK(e0, hipMemcpyAsync(b.mticks.p, stage, (size_t)T * k * sizeof(MidTick), hipMemcpyHostToDevice, st));
        HIPCHK(e0, hipEventRecord(b.mticked[h], st));
        b.mticked_pending[h] = true;
        b.launches++;
        if (due & MID_DUE_REBIN) {
            launch_mid_batch_rebin(b.mtable.p, b.mticks.p, (int)k, max_n_pad, st);
            b.launches += 2;
        }
        if (due & MID_DUE_SYNC) {
            launch_mid_batch_sync(b.mtable.p, b.mticks.p, (int)k, max_sync, st);
            b.launches++;
        }
        for (int64_t r = 0; r < T; r++)
            for (const BatchState::MidLaunch &l : b.mlaunch) {
                if (l.model == 7) launch_mid_classes_batch(l.p2r != 0, l.road != 0, b.mtable.p, b.mticks.p + (size_t)r * k, b.mgroups.p + l.beg, l.end - l.beg, st);
                else launch_mid_batch(l.model, l.p2r != 0, l.road != 0, b.mtable.p, b.mticks.p + (size_t)r * k, b.mgroups.p + l.beg, l.end - l.beg, st);
                b.launches++;
            }
        HIPCHK(e0, hipGetLastError());
        t += T;
    }
    return CSF_OK;
}

static int step_batch_impl(csf_engine *const *engines, int32_t count, int64_t n_ticks, const csf_tick_out *out) {
    int rc = batch_check(engines, count);
    if (rc) return rc;
    csf_engine *e0 = engines[0];
    if (n_ticks < 0) return fail(e0, CSF_E_ARG, "n_ticks must be >= 0");
    BatchState &b = *e0->batch;
    HIPCHK(e0, hipSetDevice(e0->device));
    const bool want_snap = out != nullptr;
    b.small.clear();
    b.rest.clear();
    b.mid.clear();
    b.snapped.assign((size_t)count, 0);
    // the members the one-wave launch takes get step_impl's prelude; the others are stepped by step_impl itself
    for (int32_t i = 0; i < count; i++) {
        csf_engine *e = engines[i];
        if ((rc = upload_all(e))) return rc;
        const bool take = n_ticks > 0 && !e->order.empty() && (e->comm_calibrated || (rc = calibrate_comm_stream(e)) == CSF_OK) && small_fused_ok(e);
        if (rc) return rc;
        if (!take) {
            // (small_fused_ok is false, so the calibration ran - or failed - above, where n_ticks > 0 and the member has road users)
            if (n_ticks > 0 && !e->order.empty() && e->comm_calibrated && batch_mid_ok(e)) {
                b.mid.push_back(i);
                continue;
            }
            bool snapped = false;
            if ((rc = step_impl(e, n_ticks, want_snap, &snapped))) return rc;
            b.snapped[(size_t)i] = snapped ? 2 : 0;
            b.rest.push_back(i);
            continue;
        }
        bool pack = false;
        if ((rc = small_prelude(e, want_snap, &pack))) return rc;
        b.snapped[(size_t)i] = pack;
        b.small.push_back(i);
    }
    if (b.mid.size() == 1) {                                      // a single mid-size member: stepped as it is alone
        bool snapped = false;
        if ((rc = step_impl(engines[b.mid[0]], n_ticks, want_snap, &snapped))) return rc;
        b.snapped[(size_t)b.mid[0]] = snapped ? 2 : 0;
        b.rest.push_back(b.mid[0]);
        b.mid.clear();
    }
    if (b.mid.size() >= 2 && (rc = step_batch_mid(b, engines, n_ticks))) return rc;
    if (!b.small.empty()) {
        // table slots: the one-wave members by vehicle class, in join order within a class - one launch per class
        b.slot_member.clear();
        // (... and behind them the members of several sets or classes, csf_small_classes: ONE further launch whatever their classes)
        int cls_beg[9] = {0}, cls_nv[8] = {0};
        for (int m = 0; m < 8; m++) {
            cls_beg[m] = (int)b.slot_member.size();
            for (int32_t i : b.small) {
                const Dev &d = engines[i]->d;
                if ((small_takes_classes(engines[i]) ? 7 : d.p.model) != m) continue;
                b.slot_member.push_back(i);
                if (d.nv > 0) cls_nv[m] = std::max(cls_nv[m], (int)d.nv_pad);
            }
        }
        cls_beg[8] = (int)b.slot_member.size();
        if ((rc = batch_table(b, e0->main))) return rc;
        for (int32_t i : b.small) {                               // a recording member's tick word, where it is not current
            csf_engine *e = engines[i];
            if (e->d.rec_tick == nullptr || e->rec_tick_dev == e->d.tick) continue;
            HIPCHK(e, hipMemsetD32Async((hipDeviceptr_t)e->d.rec_tick, (int)(uint32_t)((uint64_t)e->d.tick & 0xffffffffu), 1, e0->main));
            HIPCHK(e, hipMemsetD32Async((hipDeviceptr_t)((uint32_t *)e->d.rec_tick + 1), (int)(uint32_t)((uint64_t)e->d.tick >> 32), 1, e0->main));
            e->rec_tick_dev = e->d.tick;
            b.launches += 2;
        }
        for (int64_t t = 0; t < n_ticks;) {
            const int k = small_launch_ticks(n_ticks - t);
            const bool pack = want_snap && t + k == n_ticks;
            for (int m = 0; m < 8; m++) {
                const int cnt = cls_beg[m + 1] - cls_beg[m];
                if (cnt == 0) continue;
                if (m == 7) launch_small_classes_batch(b.table.p + cls_beg[m], cnt, cls_nv[m], k, pack, e0->main);
                else launch_small_batch(m, b.table.p + cls_beg[m], cnt, cls_nv[m], k, pack, e0->main);
                b.launches++;
                HIPCHK(e0, hipGetLastError());
            }
            for (int32_t i : b.small) small_ticked(engines[i], k, true);
            t += k;
        }
        for (int32_t i : b.small) engines[i]->device_ahead = true;
    }
    if (!want_snap) return CSF_OK;
    // one wait for every member whose read-back the launches packed; the others are read back as csf_get_tick does
    HIPCHK(e0, hipStreamSynchronize(e0->main));
    for (int32_t i = 0; i < count; i++) {
        csf_engine *e = engines[i];
        const csf_tick_out &o = out[i];
        if (!b.snapped[(size_t)i]) {
            if ((rc = csf_get_tick(e, o.s_out, o.dest_ptr, o.znav, o.Fx, o.Fy, o.tick))) return rc;
            continue;
        }
        if (b.snapped[(size_t)i] == 2 && (rc = csf_sync(e))) return rc;   // (as csf_step_get_tick: its second stream, its error word)
        if (o.tick) *o.tick = e->d.tick;
        if ((rc = snap_unpack(e, o.s_out, o.dest_ptr, o.znav, o.Fx, o.Fy))) return rc;
    }
    return CSF_OK;
}

}  // extern "C++"

int csf_batch_join(csf_engine *const *engines, int32_t count) try {
    if (!engines || count < 1) return CSF_E_ARG;
    for (int32_t i = 0; i < count; i++) {
        csf_engine *e = engines[i];
        if (!e) return CSF_E_ARG;
        for (int32_t q = 0; q < i; q++)
            if (engines[q] == e) return fail(e, CSF_E_ARG, "engine listed twice");
        if (e->device != engines[0]->device) return fail(e, CSF_E_ARG, "the members of a batch are on one device");
        if (e->batch) return fail(e, CSF_E_STATE, "engine already belongs to a batch");
        if (int crc = calib_refuses(e, "csf_batch_join")) return crc;
        if (e->loopback) return fail(e, CSF_E_STATE, "members of a loopback group cannot join a batch");
        if (e->nccl || e->world > 1) return fail(e, CSF_E_STATE, "a sharded engine cannot join a batch");
    }
    csf_engine *e0 = engines[0];
    HIPCHK(e0, hipSetDevice(e0->device));
    // everything that can fail first: a refused call changes nothing
    auto b = std::make_shared<BatchState>();
    b->device = e0->device;
    b->members.assign(engines, engines + count);
    HIPCHK(e0, b->table.alloc((size_t)count));
    HIPCHK(e0, b->stage.alloc((size_t)count));
    HIPCHK(e0, hipEventCreateWithFlags(&b->copied, hipEventDisableTiming));
    b->shadow.resize((size_t)count);
    b->held.assign((size_t)count, 0);
    for (int32_t i = 0; i < count; i++) HIPCHK(engines[i], hipStreamSynchronize(engines[i]->main));
    for (int32_t i = 0; i < count; i++) {       // one stream for the whole batch: the first member's
        csf_engine *e = engines[i];
        e->batch = b;
        if (i > 0) {
            e->own_hold = e->main_hold;
            e->main_hold = e0->main_hold;
            e->main = e->main_hold->s;
        }
    }
    return CSF_OK;
} catch (...) { return csf_caught((engines && count > 0 ? engines[0] : nullptr)); }

int csf_batch_leave(csf_engine *const *engines, int32_t count) try {
    int rc = batch_check(engines, count);
    if (rc) return rc;
    return batch_dissolve(engines[0]);
} catch (...) { return csf_caught((engines && count > 0 ? engines[0] : nullptr)); }

int csf_step_batch(csf_engine *const *engines, int32_t count, int64_t n_ticks) try {
    return step_batch_impl(engines, count, n_ticks, nullptr);
} catch (...) { return csf_caught((engines && count > 0 ? engines[0] : nullptr)); }

int csf_step_batch_get_tick(csf_engine *const *engines, int32_t count, int64_t n_ticks, const csf_tick_out *out) try {
    if (!out) return engines && count > 0 && engines[0] ? fail(engines[0], CSF_E_ARG, "csf_step_batch_get_tick: out is NULL") : CSF_E_ARG;
    return step_batch_impl(engines, count, n_ticks, out);
} catch (...) { return csf_caught((engines && count > 0 ? engines[0] : nullptr)); }

int csf_batch_get_record(csf_engine *const *engines, int32_t count, int64_t n_last, const csf_record_out *out) try {
    int rc = batch_check(engines, count);
    if (rc) return rc;
    csf_engine *e0 = engines[0];
    if (!out) return fail(e0, CSF_E_ARG, "csf_batch_get_record: out is NULL");
    if (n_last < 0) return fail(e0, CSF_E_ARG, "csf_batch_get_record: n_last must be >= 0");
    BatchState &b = *e0->batch;
    b.asks.clear();
    for (int32_t i = 0; i < count; i++) {        // every refusal before anything is written
        csf_engine *e = engines[i];
        const csf_record_out &o = out[i];
        if (!o.s && !o.F) continue;
        if (!e->d.hist) return fail(e, CSF_E_STATE, "member %d: history is not enabled (csf_record)", (int)i);
        if (o.F && !e->d.hist_F) return fail(e, CSF_E_STATE, "member %d: forces are not recorded (csf_record with CSF_REC_FORCE)", (int)i);
        int64_t first = 0;
        if (int rrc = record_last(e, i, n_last, &first)) return rrc;
        b.asks.push_back(RecAsk{e, first, n_last, o.s, o.F});
    }
    HIPCHK(e0, hipSetDevice(e0->device));
    // (the members share one stream, and a member stepped in turn has joined its second stream back into it: stream order is enough)
    if ((rc = record_gather(e0, b.rgather, e0->main, b.asks.data(), b.asks.size()))) return rc;
    for (int32_t i = 0; i < count; i++)
        if ((out[i].s || out[i].F) && out[i].first_sample) *out[i].first_sample = engines[i]->d.tick / engines[i]->d.hist_stride - n_last;
    return CSF_OK;
} catch (...) { return csf_caught((engines && count > 0 ? engines[0] : nullptr)); }

int csf_batch_ticks(const csf_engine *e, int64_t *n_ticks) try {
    if (!e || !n_ticks) return CSF_E_ARG;
    *n_ticks = e->batch_ticks;
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_batch_mid_ticks(const csf_engine *e, int64_t *n_ticks) try {
    if (!e || !n_ticks) return CSF_E_ARG;
    *n_ticks = e->batch_mid_ticks;
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_batch_launches(const csf_engine *e, int64_t *n_launches) try {
    if (!e || !n_launches) return CSF_E_ARG;
    if (!e->batch) return CSF_E_STATE;           // (not a member; no message is written: the call changes nothing)
    *n_launches = e->batch->launches;
    return CSF_OK;
} catch (...) { return csf_caught(e); }
