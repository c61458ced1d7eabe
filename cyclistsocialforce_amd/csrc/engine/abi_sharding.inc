// engine/abi_sharding.inc - C ABI: communicators, loopback groups.
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

int csf_comm_unique_id(uint8_t id_out[CSF_UNIQUE_ID_BYTES]) try {
    if (!id_out) return CSF_E_ARG;
    if (!g_rccl.load()) return fail(nullptr, CSF_E_COMM, "%s", g_rccl.err.c_str());
    static_assert(sizeof(ncclUniqueId) == CSF_UNIQUE_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    ncclResult_t r = g_rccl.GetUniqueId(&id);
    if (r != ncclSuccess) return fail(nullptr, CSF_E_COMM, "ncclGetUniqueId: %s", g_rccl.GetErrorString(r));
    memcpy(id_out, &id, sizeof id);
    return CSF_OK;
} catch (...) { return csf_caught(nullptr); }

int csf_comm_init(csf_engine *e, const uint8_t id[CSF_UNIQUE_ID_BYTES], int32_t rank, int32_t world) try {
    if (!e) return CSF_E_ARG;
    if (world < 1 || rank < 0 || rank >= world) return fail(e, CSF_E_ARG, "bad rank %d / world %d", rank, world);
    if (world > 64) return fail(e, CSF_E_ARG, "world > 64 is not supported");
    if (e->nccl) return fail(e, CSF_E_STATE, "communicator already initialised");
    if (int crc = calib_refuses(e, "csf_comm_init")) return crc;
    if (e->batch) return fail(e, CSF_E_STATE, "engine belongs to a batch (csf_batch_leave first)");
    if (!id && world > 1) return fail(e, CSF_E_ARG, "unique id is NULL");       // (before anything changes: a refused call leaves the engine as it was)
    if (id && !g_rccl.load()) return fail(e, CSF_E_COMM, "%s", g_rccl.err.c_str());
    HIPCHK(e, hipSetDevice(e->device));
    int rc = download_all(e);
    if (rc) return rc;
    const int32_t rank_was = e->rank, world_was = e->world;
    e->rank = rank;
    e->world = world;
    e->dirty = true;
    set_shard(e);
    if (!id) return CSF_OK;                                                      // (a world of one without a communicator)
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof uid);
    const ncclResult_t nrc = g_rccl.CommInitRank(&e->nccl, world, uid, rank);
    if (nrc != ncclSuccess) {                                                              // no communicator: the engine owns every receiver again
        e->nccl = nullptr;
        e->rank = rank_was;
        e->world = world_was;
        set_shard(e);
        return fail(e, CSF_E_COMM, "ncclCommInitRank failed: %s", g_rccl.GetErrorString(nrc));
    }
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_comm_init_loopback(csf_engine *const *engines, int32_t world) try {
    if (!engines || world < 1 || world > 64) return CSF_E_ARG;
    for (int r = 0; r < world; r++) {
        csf_engine *e = engines[r];
        if (!e) return CSF_E_ARG;
        if (e->nccl || e->loopback || e->world > 1) return fail(e, CSF_E_STATE, "engine already belongs to a communicator");
        if (int crc = calib_refuses(e, "csf_comm_init_loopback")) return crc;
        if (e->batch) return fail(e, CSF_E_STATE, "engine belongs to a batch (csf_batch_leave first)");
        if (e->device != engines[0]->device || e->order.size() != engines[0]->order.size() || e->d.p.model != engines[0]->d.p.model)
            return fail(e, CSF_E_ARG, "loopback members hold the same population on the same device");
        for (int q = 0; q < r; q++)
            if (engines[q] == e) return fail(e, CSF_E_ARG, "engine listed twice");
    }
    HIPCHK(engines[0], hipSetDevice(engines[0]->device));
    for (int r = 0; r < world; r++) {
        csf_engine *e = engines[r];
        int rc = download_all(e);
        if (rc) return rc;
        e->rank = r;
        e->world = world;
        e->loopback = true;
        e->dirty = true;
        e->group.assign(engines, engines + world);
        if (r > 0) {                                  // one stream for the whole group: ticks and exchanges in order
            HIPCHK(e, hipStreamSynchronize(e->main));
            e->main_hold = engines[0]->main_hold;     // (the member's own stream goes with its last holder: now)
            e->main = e->main_hold->s;
        }
        set_shard(e);
    }
    return CSF_OK;
} catch (...) { return csf_caught((engines ? engines[0] : nullptr)); }

int csf_step_group(csf_engine *const *engines, int32_t world, int64_t n_ticks) try {
    if (!engines || world < 1 || !engines[0]) return CSF_E_ARG;
    csf_engine *e0 = engines[0];
    if (n_ticks < 0) return fail(e0, CSF_E_ARG, "n_ticks must be >= 0");
    if (!e0->loopback || (int)e0->group.size() != world) return fail(e0, CSF_E_STATE, "not a loopback group of %d engines", world);
    for (int r = 0; r < world; r++)
        if (engines[r] != e0->group[(size_t)r]) return fail(e0, CSF_E_ARG, "members must be passed in rank order");
    HIPCHK(e0, hipSetDevice(e0->device));
    for (int r = 0; r < world; r++) {
        int rc = upload_all(engines[r]);
        if (rc) return rc;
    }
    for (int64_t t = 0; t < n_ticks; t++) {
        for (int r = 0; r < world; r++) {
            int rc = !e0->order.empty() ? enqueue_tick(engines[r]) : (engines[r]->d.tick++, CSF_OK);
            if (rc) return rc;
        }
        if (!e0->order.empty()) {
            int rc = loopback_exchange(engines, world);
            if (rc) return rc;
        }
    }
    if (n_ticks > 0 && !e0->order.empty())
        for (int r = 0; r < world; r++) engines[r]->device_ahead = true;
    return CSF_OK;
} catch (...) { return csf_caught((engines ? engines[0] : nullptr)); }

int csf_shard_range(const csf_engine *e, int64_t *lo, int64_t *hi) try {
    if (!e) return CSF_E_ARG;
    if (lo) *lo = e->d.lo;
    if (hi) *hi = e->d.hi;
    return CSF_OK;
} catch (...) { return csf_caught(e); }
