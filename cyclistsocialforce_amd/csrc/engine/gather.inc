// engine/gather.inc - a sharded run's blocks brought together before the population changes.
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

// A rank of a sharded run integrates only its own block of slots: its fp64 copy of the other blocks goes stale with the first
// tick.  Before the host may change the population - the road users of SUMO co-simulation arrive and leave on every rank's copy
// alike, intersection.py:458-634 - every rank needs every block's state as it is now: one all-gather per array on packed blocks
// (gather_population; a rare call); the members of a loopback group copy them from each other.  Every rank has to make the same population calls in the same order (they are collective from here on).
template <class F>
static int each_slot_array(csf_engine *e, F &&f) {                // f(base pointer, bytes per element, rows): the arrays download_all reads
    const int hl = e->d.hist_len;
    int rc;
#define ARR(buf, rows) if ((rc = f((char *)e->buf.p, sizeof(*e->buf.p), (int)(rows)))) return rc;
    ARR(s, STATE_ROWS) ARR(znp, 3) ARR(hx, hl) ARR(hy, hl) ARR(lti, 5) ARR(ppsi, 1) ARR(F, 6)
    ARR(ptr, 1) ARR(ti, 1) ARR(dgood, 1) ARR(znav, 1) ARR(zrid, 1) ARR(status, 1)
#undef ARR
    return CSF_OK;
}

static int gather_population(csf_engine *e) {
    // One exchange per ARRAY (thirteen in all), on equal blocks: a rank packs the rows of its own block - strided by the capacity -
    // into its place of a staging buffer ([rank][row][shard]: the in-place layout of ncclAllGather, the collective every tick
    // already uses), and unpacks the others' behind the call.  The members of a loopback group pack and unpack with the same code
    // and copy the packed blocks from each other where a real run calls the collective; a communicator of ONE rank takes the path
    // too (its all-gather is a copy onto itself) - so what the tests on one device cannot reach is the collective call alone.
    // (Until round 6: one ncclBroadcast per rank, array and ROW in one group - ~2 300 calls at 8 ranks with the ring's 128
    // columns - on a branch no test could enter.)
    const bool rehearse = e->nccl && e->world == 1 && !e->loopback;
    if (e->state_all_current && !rehearse) return CSF_OK;
    std::vector<csf_engine *> mem;
    if (e->loopback) mem.assign(e->group.begin(), e->group.end());
    else if (e->nccl) mem.push_back(e);
    if (mem.empty()) {                                             // (one device, no communicator: every block is its own)
        e->state_all_current = true;
        return CSF_OK;
    }
    const int world = e->loopback ? (int)mem.size() : e->world;
    const size_t cap = (size_t)e->cap;
    const int64_t shard = e->d.n_pad / world;
    if (shard <= 0 || shard * world != e->d.n_pad) return fail(e, CSF_E_STATE, "shard layout: %lld slots do not split over %d ranks", (long long)e->d.n_pad, world);
    for (csf_engine *m : mem) {
        if (m->cap != e->cap || m->d.n_pad != e->d.n_pad || m->d.n != e->d.n) return fail(e, CSF_E_STATE, "the ranks of a group hold different populations");
        HIPCHK(m, hipStreamSynchronize(m->main));
        if (m->comm) HIPCHK(m, hipStreamSynchronize(m->comm));
    }
    struct Arr { char *p; size_t el; int rows; };
    std::vector<std::vector<Arr>> arrs(mem.size());
    for (size_t i = 0; i < mem.size(); i++)
        each_slot_array(mem[i], [&](char *p, size_t el, int rows) -> int { arrs[i].push_back({p, el, rows}); return CSF_OK; });
    std::vector<DevBuf<char>> stage(mem.size());
    auto block = [&](int r, int64_t &lo, int64_t &hi) { lo = std::min<int64_t>(e->d.n, (int64_t)r * shard), hi = std::min<int64_t>(e->d.n, lo + shard); };
    int rc = CSF_OK;
    auto body = [&]() -> int {
        for (size_t k = 0; k < arrs[0].size(); k++) {
            const size_t el = arrs[0][k].el;
            const int rows = arrs[0][k].rows;
            if (rows <= 0) continue;
            const size_t blk = (size_t)rows * (size_t)shard * el;  // bytes of one rank's packed block
            int64_t lo, hi;
            for (size_t i = 0; i < mem.size(); i++) {              // pack: own block, rows made contiguous
                csf_engine *m = mem[i];
                HIPCHK(m, stage[i].reserve(blk * (size_t)world));
                block(m->rank, lo, hi);
                if (hi > lo)
                    HIPCHK(m, hipMemcpy2DAsync(stage[i].p + (size_t)m->rank * blk, (size_t)shard * el, arrs[i][k].p + (size_t)lo * el, cap * el,
                                               (size_t)(hi - lo) * el, (size_t)rows, hipMemcpyDeviceToDevice, m->main));
            }
            if (e->loopback) {                                     // the "all-gather" of a group on one device
                for (size_t i = 0; i < mem.size(); i++)
                    for (size_t j = 0; j < mem.size(); j++)
                        if (i != j)
                            HIPCHK(mem[i], hipMemcpyAsync(stage[i].p + (size_t)mem[j]->rank * blk, stage[j].p + (size_t)mem[j]->rank * blk, blk,
                                                          hipMemcpyDeviceToDevice, e->main));
            } else {
                NCCLCHK(e, g_rccl.AllGather(stage[0].p + (size_t)e->rank * blk, stage[0].p, blk, ncclChar, e->nccl, e->main));
            }
            for (size_t i = 0; i < mem.size(); i++) {              // unpack: everybody else's block
                csf_engine *m = mem[i];
                for (int r = 0; r < world; r++) {
                    if (r == m->rank) continue;
                    block(r, lo, hi);
                    if (hi > lo)
                        HIPCHK(m, hipMemcpy2DAsync(arrs[i][k].p + (size_t)lo * el, cap * el, stage[i].p + (size_t)r * blk, (size_t)shard * el,
                                                   (size_t)(hi - lo) * el, (size_t)rows, hipMemcpyDeviceToDevice, m->main));
                }
            }
        }
        return CSF_OK;
    };
    rc = body();
    hipError_t sr = hipSuccess;
    for (csf_engine *m : mem) {                                    // (before the staging buffers go)
        hipError_t r1 = hipStreamSynchronize(m->main);
        if (sr == hipSuccess) sr = r1;
    }
    if (rc) return rc;
    HIPCHK(e, sr);
    for (csf_engine *m : mem) m->state_all_current = true;
    return CSF_OK;
}

// calib_ok: the caller is one of the calls a loaded calibration engine takes (csf_set_dest_queue)
int prepare_mutation(csf_engine *e, bool calib_ok = false) {
    // a rank integrates only its own block: its fp64 copy of the other blocks goes stale with the first tick, and an
    // upload would rebuild their records from it - so the blocks are gathered first (gather_population)
    int rc;
    if (!calib_ok && (rc = calib_refuses(e, "a change of the population"))) return rc;
    if ((e->world > 1 || e->loopback || e->nccl) && e->device_ahead) {
        if ((rc = flush_pending(e))) return rc;
        if ((rc = gather_population(e))) return rc;
    }
    rc = download_all(e);
    if (rc) return rc;
    e->dirty = true;
    e->wgo.forget();
    return CSF_OK;
}
