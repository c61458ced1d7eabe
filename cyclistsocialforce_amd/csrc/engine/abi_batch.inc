// engine/abi_batch.inc - C ABI: batches of independent scenes (csf_batch_join, csf_step_batch, csf_step_batch_get_tick).
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)
//
// A junction of a SUMO network or one run of a parameter sweep is a handful of road users: one wave of the one-wave tick
// (csf_agent.hip: small_tick_kernel), and its launch is nearly all latency.  The members of a batch that this tick takes
// (small_fused_ok) are stepped by small_batch_kernel instead - one launch per vehicle class present, workgroup b ticking the scene
// of table[b] - and every other member by step_impl in turn.  The table holds the members' Dev records in device memory; it is
// renewed in stream order, and only where a member's Dev changed since it was last copied (a host shadow, memcmp).  Per-call
// values stay out of it: whether the read-back is packed is a kernel argument, and Dev::tick - what the samples of a recording
// (csf_record) are numbered from - is 0 in the table: a recording member's count is a word of its own in device memory
// (Dev::rec_tick) that the launch reads and moves on itself.  The host knows what the word holds (csf_engine::rec_tick_dev) and
// writes it in stream order only where the engine has ticked outside the batched launch since.

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
    RecGather rgather;                           // csf_batch_get_record
    std::vector<RecAsk> asks;
    ~BatchState() {   // (the last copy from `stage` has ended before the members below go, `stage` among them)
        (void)hipSetDevice(device);
        if (copy_pending && copied) (void)hipEventSynchronize(copied);
        if (copied) (void)hipEventDestroy(copied);
    }
};

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
    b.snapped.assign((size_t)count, 0);
    // the members the one-wave launch takes get step_impl's prelude; the others are stepped by step_impl itself
    for (int32_t i = 0; i < count; i++) {
        csf_engine *e = engines[i];
        if ((rc = upload_all(e))) return rc;
        const bool take = n_ticks > 0 && !e->order.empty() && (e->comm_calibrated || (rc = calibrate_comm_stream(e)) == CSF_OK) && small_fused_ok(e);
        if (rc) return rc;
        if (!take) {
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
    if (!b.small.empty()) {
        // table slots: the one-wave members by vehicle class, in join order within a class - one launch per class
        b.slot_member.clear();
        int cls_beg[8] = {0}, cls_nv[7] = {0};
        for (int m = 0; m < 7; m++) {
            cls_beg[m] = (int)b.slot_member.size();
            for (int32_t i : b.small) {
                const Dev &d = engines[i]->d;
                if (d.p.model != m) continue;
                b.slot_member.push_back(i);
                if (d.nv > 0) cls_nv[m] = std::max(cls_nv[m], (int)d.nv_pad);
            }
        }
        cls_beg[7] = (int)b.slot_member.size();
        if ((rc = batch_table(b, e0->main))) return rc;
        for (int32_t i : b.small) {                               // a recording member's tick word, where it is not current
            csf_engine *e = engines[i];
            if (e->d.rec_tick == nullptr || e->rec_tick_dev == e->d.tick) continue;
            HIPCHK(e, hipMemsetD32Async((hipDeviceptr_t)e->d.rec_tick, (int)(uint32_t)((uint64_t)e->d.tick & 0xffffffffu), 1, e0->main));
            HIPCHK(e, hipMemsetD32Async((hipDeviceptr_t)((uint32_t *)e->d.rec_tick + 1), (int)(uint32_t)((uint64_t)e->d.tick >> 32), 1, e0->main));
            e->rec_tick_dev = e->d.tick;
        }
        for (int64_t t = 0; t < n_ticks;) {
            const int k = small_launch_ticks(n_ticks - t);
            const bool pack = want_snap && t + k == n_ticks;
            for (int m = 0; m < 7; m++) {
                const int cnt = cls_beg[m + 1] - cls_beg[m];
                if (cnt == 0) continue;
                launch_small_batch(m, b.table.p + cls_beg[m], cnt, cls_nv[m], k, pack, e0->main);
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
        const int64_t have = e->d.tick / e->d.hist_stride;
        if (n_last > have || n_last > e->d.hist_cap)
            return fail(e, CSF_E_ARG, "member %d: the last %lld samples are not in the ring (have %lld, capacity %d)", (int)i, (long long)n_last,
                        (long long)have, e->d.hist_cap);
        b.asks.push_back(RecAsk{e, have - n_last, n_last, o.s, o.F});
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
