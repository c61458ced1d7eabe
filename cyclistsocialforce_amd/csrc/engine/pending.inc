// engine/pending.inc - population changes collected for the device (patch_kernel), order and row read-backs.
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

// Population changes between ticks go straight to the device arrays (spawn / retire / requeue kernels of csf_agent.hip)
// when the device copy is current: no download, no upload, no re-sort.  Sharded engines, engines with the opt-in
// history ring and CSF_INCREMENTAL=0 take the round trip through the host mirror (prepare_mutation / upload_all).
bool can_patch_device(const csf_engine *e) {
    return e->knobs.incremental && e->incremental && !e->dirty && e->world == 1 && !e->nccl && !e->loopback && e->d.hist == nullptr;
}

// a pinned, device-visible host buffer of `bytes` from the ring; waits only if the ring of four is exhausted
int stage_acquire(csf_engine *e, size_t bytes, csf_engine::PinnedSlot **out) {
    csf_engine::PinnedSlot &sl = e->pinned[e->pinned_next];
    e->pinned_next = (e->pinned_next + 1) % 4;
    if (sl.busy) {
        HIPCHK(e, hipEventSynchronize(sl.done));
        sl.busy = false;
    }
    if (bytes > sl.buf.n) HIPCHK(e, sl.buf.alloc(std::max<size_t>(2 * bytes, 1 << 16)));   // (not busy: nothing reads it any more)
    if (!sl.done) HIPCHK(e, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    *out = &sl;
    return CSF_OK;
}

// The collected retirements, spawns and queue replacements -> one patch_kernel launch (csf_agent.hip), which also renews
// the circles of the tail batches the arrivals went to; the binned order is renewed when ticks x arrivals since the last
// re-binning says so (bounds_before_pair).
int flush_pending(csf_engine *e) {
    csf_engine::Pending &pd = e->pend;
    if (pd.empty()) return CSF_OK;
    Dev &d = e->d;
    e->mid_synced = false;
    const size_t b_ret = pd.retire.size() * sizeof(int32_t), b_sp = pd.spawn.size() * sizeof(SpawnRec),
                 b_rq = pd.requeue.size() * sizeof(QueueRec), b_rows = pd.rows.size() * sizeof(double);
    auto up8 = [](size_t x) { return (x + 7) & ~(size_t)7; };
    PatchHeader h;
    h.n_retire = (int64_t)pd.retire.size();
    h.n_spawn = (int64_t)pd.spawn.size();
    h.n_requeue = (int64_t)pd.requeue.size();
    h.n_rows = (int64_t)(pd.rows.size() / 3);
    h.off_retire = (int64_t)up8(sizeof(PatchHeader));
    h.off_spawn = h.off_retire + (int64_t)up8(b_ret);
    h.off_requeue = h.off_spawn + (int64_t)up8(b_sp);
    h.off_rows = h.off_requeue + (int64_t)up8(b_rq);
    h.q_top = e->q_top;
    for (SpawnRec &r : pd.spawn) r.qbeg += e->q_top;          // relative to this batch's rows until now
    for (QueueRec &r : pd.requeue) r.qbeg += e->q_top;
    csf_engine::PinnedSlot *pin = nullptr;
    int rc = stage_acquire(e, (size_t)h.off_rows + b_rows, &pin);
    if (rc) return rc;
    char *base = pin->buf.p;
    memcpy(base, &h, sizeof h);
    if (b_ret) memcpy(base + h.off_retire, pd.retire.data(), b_ret);
    if (b_sp) memcpy(base + h.off_spawn, pd.spawn.data(), b_sp);
    if (b_rq) memcpy(base + h.off_requeue, pd.requeue.data(), b_rq);
    if (b_rows) memcpy(base + h.off_rows, pd.rows.data(), b_rows);
    // The arrivals went to known places of the sentinel tail (rebin): the launch itself renews the circles of those few
    // batches, and the circles the last pair launch emitted for this tick stay good for all others (a retirement only
    // leaves a circle larger than necessary).  Otherwise every circle is recomputed before the next pair launch.
    int b0 = 0, b1 = 0;
    bool circles_here = e->bounds_fresh && e->tail_tracked && d.classify && !e->pend_inplace;
    if (circles_here && h.n_spawn > 0) {
        b0 = (int)((e->live_at_rebin + e->tail_flushed) / 64);
        b1 = (int)((e->live_at_rebin + e->tail_used + 63) / 64);
        if (b1 - b0 > 32 || (int64_t)b1 * 64 > d.n_src) circles_here = false, b0 = b1 = 0;
    }
    launch_patch(d, h, pin->buf.dev, e->ticket.p, b0, b1, h.n_retire + h.n_spawn + h.n_requeue + 3 * h.n_rows, e->main);
    e->tail_flushed = e->tail_used;
    e->pend_inplace = false;
    // The class-segmented order has no tail for arrivals: an arrival belongs into its set's run, which only a re-binning
    // can give it (the sort reads every slot's record and set) - so the order is renewed before the next pair launch
    // (~50 us, against 5 ms for the way through the host mirror).  Departures leave sentinel records in their runs.
    if (!e->segs.empty() && h.n_spawn > 0) e->ticks_since_rebin = std::max<int64_t>(e->ticks_since_rebin, e->knobs.rebin_ticks);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipEventRecord(pin->done, e->main));
    pin->busy = true;
    e->q_top += h.n_rows;
    for (int32_t a : pd.retire) e->sidx[(size_t)a].retire = -1, e->dev_alive[(size_t)a] = 0;
    for (const SpawnRec &r : pd.spawn) e->sidx[(size_t)r.slot].spawn = -1, e->dev_alive[(size_t)r.slot] = 1;
    for (const QueueRec &r : pd.requeue) e->sidx[(size_t)r.slot].requeue = -1;
    e->churn += e->pend_tail_spawns;                          // (an arrival in a leaver's slot adds nothing to the tail)
    e->pend_tail_spawns = 0;
    pd.retire.clear();
    pd.spawn.clear();
    pd.requeue.clear();
    pd.rows.clear();
    if (!circles_here) e->bounds_fresh = false;
    e->device_ahead = true;                                    // the host mirror of the patched slots was not kept up
    d.n_live = (int64_t)e->order.size();
    if (e->knobs.fake_world <= 1) d.hi = d.n;                 // (unsharded: the receiver block is every slot)
    update_far_radius(e);
    return CSF_OK;
}

// the queue replacement collected for slot a, if any, is void (the slot is retired or spawned into anew)
void drop_pending_requeue(csf_engine *e, size_t a) {
    const int32_t at = e->sidx[a].requeue;
    if (at < 0) return;
    const QueueRec last = e->pend.requeue.back();
    e->pend.requeue[(size_t)at] = last;
    e->sidx[(size_t)last.slot].requeue = at;
    e->pend.requeue.pop_back();
    e->sidx[a].requeue = -1;
}

int sync_order(csf_engine *e) {                         // the device copy of the population order (read-back kernels)
    Dev &d = e->d;
    bool identity = (int64_t)e->order.size() == d.n;
    for (size_t i = 0; identity && i < e->order.size(); i++) identity = e->order[i] == (int32_t)i;
    if (identity) {
        d.order = nullptr;
    } else {
        if (e->order_dirty)
            HIPCHK(e, hipMemcpyAsync(e->order_dev.p, e->order.data(), e->order.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->main));
        d.order = e->order_dev.p;
    }
    e->order_dirty = false;
    return CSF_OK;
}

// slot-indexed device array (component c at [c * cap + slot]) -> caller's array in population order
template <class T>
int read_rows(csf_engine *e, const T *dev, int comps, T *out, bool row_major) {
    const int64_t n = (int64_t)e->order.size(), ns = e->d.n, cap = e->cap;
    std::vector<T> tmp((size_t)ns);
    for (int c = 0; c < comps; c++) {
        HIPCHK(e, hipMemcpy(tmp.data(), dev + (size_t)c * cap, (size_t)ns * sizeof(T), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; i++) out[row_major ? i * comps + c : c * n + i] = tmp[(size_t)e->order[(size_t)i]];
    }
    return CSF_OK;
}

// entry points that index the device arrays by road user (replay, history, sharding) want slots == population order
int ensure_compact(csf_engine *e) {
    bool identity = e->free_tail.empty() && e->free_recent.empty() && (int64_t)e->order.size() == e->d.n;
    for (size_t i = 0; identity && i < e->order.size(); i++) identity = e->order[i] == (int32_t)i;
    if (identity) return CSF_OK;
    int rc = download_all(e);
    if (rc) return rc;
    e->dirty = true;
    return upload_all(e);
}
