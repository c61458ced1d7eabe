// engine/abi_measurement.inc - C ABI: far-field radius, time stamps, counters.
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

int csf_far_radius(const csf_engine *e, double *radius_m) try {
    if (!e || !radius_m) return CSF_E_ARG;
    // (a population that has not been uploaded yet: the kernel the upload's re-binning will choose)
    const int32_t pv = e->dirty ? pair_variant_for(e, (int64_t)e->order.size()) : e->d.pair_variant;
    const bool binned = pv == 0 && e->d.p.model != CSF_BICYCLE && e->d.n >= BIN_MIN_AGENTS;
    // (computed here rather than read back: the kernel's copy is refreshed with the next upload of the population)
    *radius_m = binned ? (double)(float)far_radius(e->far_kappa, e->d.n, e->knobs.far_eps) : (double)INFINITY;  // no circles, no cull
    // (large populations: the radius in use since the last re-binning, from the sources a receiver can meet - rebin)
    if (binned && e->far_T > 0.0 && e->far_kappa > 0.0) *radius_m = (double)(float)(e->far_T / e->far_kappa);
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_profile_enable(csf_engine *e, int32_t on) try {
    if (!e) return CSF_E_ARG;
    e->profile = on > 0 ? on : 0;
    if (e->profile) {                    // the event pool is created here, not inside the first sampled tick
        HIPCHK(e, hipSetDevice(e->device));
        return prof_make_pool(e);
    }
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_profile_kernels(csf_engine *e, double ms[4], int64_t launches[4]) try {
    if (!e) return CSF_E_ARG;
    int rc = csf_sync(e);
    if (rc) return rc;
    while (e->prof_resolved < e->prof_issued)
        if ((rc = prof_resolve_one(e))) return rc;
    for (int k = 0; k < 4; k++) {
        if (ms) ms[k] = e->prof_ms[k];
        if (launches) launches[k] = e->prof_cnt[k];
    }
    e->last_gather_ms = e->prof_ms[3];
    for (int k = 0; k < 4; k++) e->prof_ms[k] = 0, e->prof_cnt[k] = 0;
    e->prof_ticks = 0;
    for (auto &v : e->prof_us) v.clear();
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_profile_read(csf_engine *e, double *pair_ms, double *agent_ms, int64_t *launches) try {
    double ms[4];
    int64_t cnt[4];
    int rc = csf_profile_kernels(e, ms, cnt);
    if (rc) return rc;
    if (pair_ms) *pair_ms = ms[0];
    if (agent_ms) *agent_ms = cnt[2] > 0 ? ms[2] * (double)cnt[0] / (double)cnt[2] : 0.0;   // scaled to the pair kernel's count
    if (launches) *launches = cnt[0];
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_profile_samples_of(csf_engine *e, int32_t kernel, double *us, int64_t capacity, int64_t *n_samples) try {
    if (!e || !n_samples || capacity < 0 || (capacity > 0 && !us) || kernel < 0 || kernel > 3)
        return e ? fail(e, CSF_E_ARG, "csf_profile_samples_of: bad arguments") : CSF_E_ARG;
    int rc = csf_sync(e);
    if (rc) return rc;
    while (e->prof_resolved < e->prof_issued)
        if ((rc = prof_resolve_one(e))) return rc;
    const std::vector<float> &v = e->prof_us[kernel];
    const int64_t n = std::min<int64_t>(capacity, (int64_t)v.size());
    for (int64_t k = 0; k < n; k++) us[k] = v[(size_t)k];
    *n_samples = n;
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_profile_samples(csf_engine *e, double *pair_us, int64_t capacity, int64_t *n_samples) try {
    return csf_profile_samples_of(e, 0, pair_us, capacity, n_samples);
} catch (...) { return csf_caught(e); }

int csf_count_pairs(csf_engine *e, int64_t counts[4], const char **kernel_name) try {
    if (!e || !counts) return e ? fail(e, CSF_E_ARG, "csf_count_pairs: NULL output") : CSF_E_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    int rc = upload_all(e);
    if (rc) return rc;
    Dev &d = e->d;
    const char *name = pair_kernel_name(d);
    if (!e->segs.empty()) {                                      // one launch per parameter set: the kernel of the first
        Dev d0 = d;
        d0.p = e->classes[(size_t)e->segs[0].cls];
        d0.n_classes = 1;
        name = pair_kernel_name(d0);
    }
    if (kernel_name) *kernel_name = name;
    for (int k = 0; k < 4; k++) counts[k] = -1;
    if (std::string(name) != "pair_cull_kernel") return CSF_OK;   // only the cull-first kernel counts
    for (int k = 0; k < 4; k++) counts[k] = 0;
    if (d.n_live <= 1 || d.hi <= d.lo) return CSF_OK;
    if ((rc = wait_gather(e))) return rc;
    if (!e->segs.empty() && e->ticks_since_rebin >= e->knobs.rebin_ticks && (rc = rebin(e))) return rc;   // (arrivals since: flush_pending)
    if (d.classify && !e->bounds_fresh) launch_bounds(d, e->main);
    if ((e->world > 1 || e->nccl != nullptr || e->loopback) && d.recs_valid && e->ticks_since_rebin > 1) {
        launch_sorted_copy(d, e->main, e->xbuf_fresh);
        e->xbuf_fresh = false;
    }
    DevBuf<unsigned long long> &cnt = e->scratch_cnt;
    HIPCHK(e, cnt.reserve(4));
    HIPCHK(e, hipMemsetAsync(cnt.p, 0, 4 * sizeof(unsigned long long), e->main));
    if ((rc = set_fov_band(e))) return rc;
    Dev dd = d;                 // this tick's records and circles; the circles of the next tick are not touched
    dd.pair_count = cnt.p;
    dd.bnd_next = nullptr;
    dd.edge = nullptr;          // (no per-agent launch follows that would take undecided pairs over)
    launch_pair_all(e, dd);                                      // (the Bicycle-field launches of a mixed population do not count)
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(e->main));
    unsigned long long h[4] = {0, 0, 0, 0};
    HIPCHK(e, hipMemcpy(h, cnt.p, sizeof h, hipMemcpyDeviceToHost));
    for (int k = 0; k < 4; k++) counts[k] = (int64_t)h[k];
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_near_dropped(csf_engine *e, int64_t *n_dropped) try {
    if (!e || !n_dropped) return e ? fail(e, CSF_E_ARG, "csf_near_dropped: NULL output") : CSF_E_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->main));
    unsigned h = 0;
    HIPCHK(e, hipMemcpy(&h, e->edge_n.p + 1, sizeof h, hipMemcpyDeviceToHost));
    *n_dropped = (int64_t)h;
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_handout_ranks(const uint32_t *cand, const uint32_t *inside, int32_t n, int32_t *rank, int32_t *weight) try {
    if (!cand || !inside || !rank || n < 0 || n > 64) return -1;
    if (weight)
        for (int r = 0; r < n; r++) weight[r] = (int32_t)csf::handout_weight(cand[r], inside[r] & cand[r]);
    return csf::handout_ranks(cand, inside, n, rank);
} catch (...) { return -1; }

int csf_wg_order_ranks(const uint32_t *cost, int32_t n, int32_t *order) try {
    if (!cost || !order || n < 0) return -1;
    csf::wg_order_host(cost, n, order);
    return n;
} catch (...) { return -1; }

// pair_shape on bare words (tests/test_pair_shape_host.py: the whole lattice against the recorded table, no device)
static Dev pair_shape_dev(const int32_t *in) {
    Dev d{};
    d.pc.p2r = in[0], d.n_classes = in[1], d.has_bike = in[2], d.model_mask = in[3], d.p.model = in[4], d.classify = in[5], d.recs_valid = in[6];
    d.pair_variant = in[7], d.recv_binned = in[8], d.rpb = in[9], d.wide = in[10], d.pc.reach = in[11];
    static uint32_t given;
    d.wg_cost = in[12] ? &given : nullptr;      // (compared with NULL, never read)
    d.hi = in[14];
    return d;
}

int csf_pair_shape_of(const int32_t *in, int32_t *out, const char **name) try {
    if (!in || !out) return -1;
    const Dev d = pair_shape_dev(in);
    const PairShape s = pair_shape(d, in[13] != 0);
    const int32_t w[CSF_PAIR_SHAPE_OUT] = {s.family, s.field, s.rw, s.p2r, s.classify, s.binr, s.ord, s.reach, s.rpb, s.cw, s.per_group, s.threads,
                                           s.tile(), (int32_t)s.groups(d.hi - d.lo), (int32_t)pair_order_groups(d)};
    std::copy(w, w + CSF_PAIR_SHAPE_OUT, out);
    if (name) *name = s.name;
    return CSF_PAIR_SHAPE_OUT;
} catch (...) { return -1; }

int csf_pair_shape_words(csf_engine *e, int32_t *in) try {
    if (!e || !in) return e ? fail(e, CSF_E_ARG, "csf_pair_shape_words: NULL output") : CSF_E_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    int rc = upload_all(e);
    if (rc) return rc;
    Dev d = e->d;
    const bool one_grid = !e->segs.empty() && e->seg_total_by > 0 && e->knobs.seg_grid != 0;
    if (!e->segs.empty()) {                      // the first launch of launch_pair_all: the grid of all runs, or the first set's run
        d.n_classes = 1, d.recv_binned = 0;
        if (!one_grid) d.p = e->classes[(size_t)e->segs[0].cls], d.pc = e->segs[0].pc;
    }
    const int32_t w[CSF_PAIR_SHAPE_IN] = {d.pc.p2r != 0, d.n_classes, d.has_bike, d.model_mask, d.p.model, d.classify, d.recs_valid, d.pair_variant,
                                          d.recv_binned, d.rpb, d.wide, d.pc.reach, e->wgo.last >= 0, one_grid,
                                          (int32_t)std::min<int64_t>(d.hi - d.lo, INT32_MAX), 0};
    std::copy(w, w + CSF_PAIR_SHAPE_IN, in);
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_wg_order_tables(csf_engine *e, int64_t *groups, int32_t *chunks, int32_t *ordered, uint32_t *cost, int32_t *order, int64_t capacity) try {
    if (!e || !groups || !chunks || !ordered || capacity < 0) return e ? fail(e, CSF_E_ARG, "csf_wg_order_tables: bad arguments") : CSF_E_ARG;
    int rc = csf_sync(e);
    if (rc) return rc;
    const csf_engine::WgOrder &w = e->wgo;
    *groups = 0, *chunks = 0, *ordered = 0;
    if (w.last < 0) return CSF_OK;
    const int64_t words = w.groups * w.chunks;
    if ((cost || order) && words > capacity) return fail(e, CSF_E_ARG, "csf_wg_order_tables: %lld words, room for %lld", (long long)words, (long long)capacity);
    *groups = w.groups, *chunks = w.chunks, *ordered = w.last_ordered ? 1 : 0;
    if (cost) HIPCHK(e, hipMemcpy(cost, w.cost[w.last].p, (size_t)words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (order && w.last_ordered) HIPCHK(e, hipMemcpy(order, w.order[w.last].p, (size_t)words * sizeof(int32_t), hipMemcpyDeviceToHost));
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_comm_stream_order(const csf_engine *e, int32_t *second_stream, double us_per_tick[2]) try {
    if (!e || !second_stream) return CSF_E_ARG;
    *second_stream = e->comm_second ? 1 : 0;
    if (us_per_tick) us_per_tick[0] = e->comm_cal_us[0], us_per_tick[1] = e->comm_cal_us[1];
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_small_ticks(const csf_engine *e, int64_t *n_ticks) try {
    if (!e || !n_ticks) return CSF_E_ARG;
    *n_ticks = e->small_ticks;
    return CSF_OK;
} catch (...) { return csf_caught(e); }

// (refused like csf_step while a calibration data set is held; a refused call changes nothing)
int csf_small_classes(csf_engine *e, int32_t on) try {
    if (!e || (on != 0 && on != 1)) return CSF_E_ARG;
    if (int crc = calib_refuses(e, "csf_small_classes")) return crc;
    e->small_classes = on == 1;
    return CSF_OK;
} catch (...) { return csf_caught(e); }

// (refused like csf_small_classes; the next tick asks mid_road_ok, and a batch asks it at the start of every call)
int csf_mid_road(csf_engine *e, int32_t on) try {
    if (!e || (on != 0 && on != 1)) return CSF_E_ARG;
    if (int crc = calib_refuses(e, "csf_mid_road")) return crc;
    e->mid_road = on == 1;
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_mid_road_ticks(const csf_engine *e, int64_t *n_ticks) try {
    if (!e || !n_ticks) return CSF_E_ARG;
    *n_ticks = e->mid_road_ticks;
    return CSF_OK;
} catch (...) { return csf_caught(e); }

// (refused like csf_small_classes; the next tick asks mid_takes_classes, and a batch asks it at the start of every call)
int csf_mid_classes(csf_engine *e, int32_t on) try {
    if (!e || (on != 0 && on != 1)) return CSF_E_ARG;
    if (int crc = calib_refuses(e, "csf_mid_classes")) return crc;
    e->mid_classes = on == 1;
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_mid_classes_ticks(const csf_engine *e, int64_t *n_ticks) try {
    if (!e || !n_ticks) return CSF_E_ARG;
    *n_ticks = e->mid_classes_ticks;
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_mid_ticks(const csf_engine *e, int64_t *n_ticks) try {
    if (!e || !n_ticks) return CSF_E_ARG;
    *n_ticks = e->mid_ticks;
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_holes_taken(const csf_engine *e, int64_t *n) try {
    if (!e || !n) return CSF_E_ARG;
    *n = e->holes.taken;
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_profile_gather(const csf_engine *e, double *gather_ms) try {
    if (!e || !gather_ms) return CSF_E_ARG;
    *gather_ms = e->last_gather_ms;
    return CSF_OK;
} catch (...) { return csf_caught(e); }

}  // extern "C"
