// engine/comm_prof.inc - the tick's all-gather, per-kernel time stamps.
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

// CSF_COMM_STREAM=second puts the all-gather on a second HIP stream, so that the destination-force phase of the
// next tick (launched before the wait) overlaps it.  Measured with a 1-rank communicator the two cross-stream
// event waits per tick and the extra launch cost 26 us against 8 us in stream order, more than the ~6 us of
// destination-force work they can hide, so the default keeps the collective in stream order on the main stream.
bool comm_second_stream(const csf_engine *e) { return e->comm_second; }

int all_gather_records(csf_engine *e) {
    Dev &d = e->d;
    size_t shard = (size_t)(d.n_pad / e->world);
    const bool second = comm_second_stream(e);
    hipStream_t cs = second ? e->comm : e->main;
    if (second) HIPCHK(e, hipStreamWaitEvent(e->comm, e->ev_integ, 0));
    // ONE collective on the exchange records (csf_dev.h: xbuf; 32 B per slot: the record, what its position left over in
    // fp32, the Bicycle field's second record) - until round 5 a group of two or three all-gathers on rec / reclo / rec2
    if (d.xbuf == nullptr) return fail(e, CSF_E_DEVICE, "no exchange buffer (allocation failed when the shard layout was set)");
    NCCLCHK(e, g_rccl.AllGather(d.xbuf + 2 * (size_t)e->rank * shard, d.xbuf, shard * 8, ncclFloat32, e->nccl, cs));
    e->xbuf_fresh = true;
    if (second) {
        HIPCHK(e, hipEventRecord(e->ev_gather, e->comm));
        e->gather_pending = true;
    }
    return CSF_OK;
}

constexpr size_t PROF_SLOTS = 256, PROF_KEEP = 1 << 16;

// oldest outstanding slot -> running sums (waits for its last event)
int prof_resolve_one(csf_engine *e) {
    csf_engine::ProfSlot &sl = e->prof_pool[e->prof_resolved % PROF_SLOTS];
    const int last = sl.gather ? 7 : sl.agent ? 5 : sl.road ? 3 : sl.pair ? 1 : -1;
    if (last >= 0) HIPCHK(e, hipEventSynchronize(sl.ev[last]));
    const bool have[4] = {sl.pair, sl.road, sl.agent, sl.gather};
    for (int k = 0; k < 4; k++) {
        if (!have[k]) continue;
        float ms = 0;
        HIPCHK(e, hipEventElapsedTime(&ms, sl.ev[2 * k], sl.ev[2 * k + 1]));
        e->prof_ms[k] += ms;
        e->prof_cnt[k]++;
        if (e->prof_us[k].size() < PROF_KEEP) e->prof_us[k].push_back(ms * 1e3f);
    }
    // CSF_CHASE_CLOCK (measurement aid, every tick sampled): the dispatch time stamps of consecutive ticks against each other - pair end ->
    // per-agent start / end, per-agent end -> the next tick's pair start (the previous slot of the pool is still intact)
    if (!e->knobs.chase_clock.empty() && sl.pair && sl.agent && e->prof_resolved > 0) {
        csf_engine::ProfSlot &pv = e->prof_pool[(e->prof_resolved - 1) % PROF_SLOTS];
        float a = 0, b = 0, c = 0, d2 = 0;
        if (pv.pair && pv.agent && hipEventElapsedTime(&a, pv.ev[1], pv.ev[4]) == hipSuccess && hipEventElapsedTime(&b, pv.ev[1], pv.ev[5]) == hipSuccess &&
            hipEventElapsedTime(&c, pv.ev[5], sl.ev[0]) == hipSuccess && hipEventElapsedTime(&d2, pv.ev[0], sl.ev[0]) == hipSuccess)
            fprintf(stderr, "CHASE_EVENTS agent_start_after_pair_end %.2f agent_end_after_pair_end %.2f next_pair_start_after_agent_end %.2f period %.2f\n",
                    a * 1e3, b * 1e3, c * 1e3, d2 * 1e3);
        (void)hipGetLastError();
    }
    e->prof_resolved++;
    return CSF_OK;
}

int prof_make_pool(csf_engine *e) {
    if (!e->prof_pool.empty()) return CSF_OK;
    e->prof_pool.resize(PROF_SLOTS);
    for (auto &sl : e->prof_pool)
        for (auto &ev : sl.ev) HIPCHK(e, hipEventCreate(&ev));
    return CSF_OK;
}

// a free slot for a call outside the ticks (csf_profile_enable: its first launch is timed like a tick's pair launch, as kernel 0), if
// the call launches anything; *sl stays NULL where profiling is off
int prof_take(csf_engine *e, bool launches, csf_engine::ProfSlot **sl) {
    *sl = nullptr;
    if (e->profile <= 0 || !launches) return CSF_OK;
    if (int rc = prof_make_pool(e)) return rc;
    if (e->prof_issued - e->prof_resolved >= PROF_SLOTS)
        if (int rc = prof_resolve_one(e)) return rc;
    *sl = &e->prof_pool[e->prof_issued % PROF_SLOTS];
    (*sl)->pair = (*sl)->road = (*sl)->agent = (*sl)->gather = false;
    e->prof_issued++;
    return CSF_OK;
}

// ... and for this tick (NULL with *rc == 0: profiling is off for it)
csf_engine::ProfSlot *prof_slot(csf_engine *e, int *rc) {
    csf_engine::ProfSlot *sl = nullptr;
    *rc = prof_take(e, e->profile > 0 && e->d.tick % e->profile == 0, &sl);
    return sl;
}

int wait_gather(csf_engine *e) {
    if (e->gather_pending) {
        HIPCHK(e, hipStreamWaitEvent(e->main, e->ev_gather, 0));
        e->gather_pending = false;
    }
    return CSF_OK;
}

}  // namespace
