// engine/layout.inc - allocation, shard bounds, source chunks, the pair kernel by population size.
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

int alloc_all(csf_engine *e) {
    const size_t cap = (size_t)e->cap;
    const size_t hl = (size_t)e->d.hist_len;
    HIPCHK(e, e->s.alloc(STATE_ROWS * cap));
    HIPCHK(e, e->vdes.alloc(cap));
    HIPCHK(e, e->qbeg.alloc(cap));
    HIPCHK(e, e->qlen.alloc(cap));
    HIPCHK(e, e->alive.alloc(cap));
    HIPCHK(e, e->order_dev.alloc(cap));
    HIPCHK(e, e->ptr.alloc(cap));
    HIPCHK(e, e->znav.alloc(cap));
    HIPCHK(e, e->znp.alloc(3 * cap));
    HIPCHK(e, e->ti.alloc(cap));
    HIPCHK(e, e->hx.alloc(hl * cap));
    HIPCHK(e, e->hy.alloc(hl * cap));
    HIPCHK(e, e->lti.alloc(5 * cap));
    HIPCHK(e, e->zrid.alloc(cap));
    HIPCHK(e, e->dgood.alloc(cap));
    HIPCHK(e, e->ppsi.alloc(cap));
    HIPCHK(e, e->F.alloc(6 * cap));
    HIPCHK(e, e->status.alloc(cap));
    HIPCHK(e, e->part.alloc((size_t)MAX_SPLIT * cap));
    HIPCHK(e, e->froad.alloc(cap));
    // records: room for the per-rank padding of an 8-way shard
    size_t nrec = (cap + 64 * 64 + 63) / 64 * 64;
    HIPCHK(e, e->rec.alloc(nrec));
    HIPCHK(e, e->rec2.alloc(nrec));
    {   // the last record of the arrays is no slot's: a sentinel for ever (padding of the class-segmented order)
        const float4 sent = make_float4(1e15f, 1e15f, 1.0f, 0.0f);
        const float2 sent2 = make_float2(0.0f, 1.0f);
        HIPCHK(e, hipMemcpy(e->rec.p + nrec - 1, &sent, sizeof sent, hipMemcpyHostToDevice));
        HIPCHK(e, hipMemcpy(e->rec2.p + nrec - 1, &sent2, sizeof sent2, hipMemcpyHostToDevice));
        e->sent_slot = (int32_t)(nrec - 1);
    }
    HIPCHK(e, e->recs2.alloc(nrec));
    HIPCHK(e, e->perm.alloc(nrec));
    HIPCHK(e, e->pos.alloc(nrec));
    HIPCHK(e, e->recs.alloc(nrec));
    HIPCHK(e, e->recg.alloc(nrec));
    HIPCHK(e, e->recb.alloc(nrec));
    if (g_poison) {   // records that no slot owns: NaN instead of (0, 0, 0, 0), which is a road user at the scene's origin
        const float4 sent = make_float4(1e15f, 1e15f, 1.0f, 0.0f);
        const float2 sent2 = make_float2(0.0f, 1.0f);
        HIPCHK(e, e->rec.poison_from(0)); HIPCHK(e, e->rec2.poison_from(0)); HIPCHK(e, e->recs.poison_from(0));
        HIPCHK(e, e->recs2.poison_from(0)); HIPCHK(e, e->recg.poison_from(0)); HIPCHK(e, e->recb.poison_from(0));
        HIPCHK(e, hipMemcpy(e->rec.p + nrec - 1, &sent, sizeof sent, hipMemcpyHostToDevice));
        HIPCHK(e, hipMemcpy(e->rec2.p + nrec - 1, &sent2, sizeof sent2, hipMemcpyHostToDevice));
    }
    HIPCHK(e, e->borg.alloc(nrec / 64 + 1));
    HIPCHK(e, e->bnd.alloc(nrec / 64));
    HIPCHK(e, e->bnd2.alloc(nrec / 64));
    HIPCHK(e, e->rorg.alloc(nrec));
    HIPCHK(e, e->reclo.alloc(nrec));
    HIPCHK(e, e->sort_vals.alloc(nrec));
    HIPCHK(e, e->rlist.alloc(nrec));
    HIPCHK(e, e->sort_keys.alloc(nrec));
    HIPCHK(e, e->sort_keys_out.alloc(nrec));
    HIPCHK(e, e->sort_tmp.alloc(bin_temp_bytes((int64_t)nrec) + 256));
    e->h_s.assign(STATE_ROWS * cap, 0.0);
    e->h_vdes.assign(cap, 0.0);
    e->h_znp.assign(3 * cap, 0.0);
    e->h_hx.assign(hl * cap, 0.0);
    e->h_hy.assign(hl * cap, 0.0);
    e->h_lti.assign(5 * cap, 0.0);
    e->h_ppsi.assign(cap, 0.0);
    e->h_F.assign(6 * cap, 0.0);
    e->h_ptr.assign(cap, 0);
    e->h_ti.assign(cap, 0);
    e->h_dgood.assign(cap, 0);
    e->h_znav.assign(cap, 0);
    e->h_zrid.assign(cap, 0);
    e->h_status.assign(cap, 0);
    e->h_q.assign(cap, {});
    e->h_script.assign(cap, {});
    HIPCHK(e, e->sbeg.alloc(cap));
    HIPCHK(e, e->slen.alloc(cap));
    e->h_alive.assign(cap, 0);
    e->h_cls.assign(cap, 0);
    HIPCHK(e, e->cls.alloc(cap));
    HIPCHK(e, e->ticket.alloc(1));
    HIPCHK(e, e->edge.alloc(EDGE_CAP));
    HIPCHK(e, e->edge_n.alloc(2));
    HIPCHK(e, e->edge_head.alloc(cap));
    e->sidx.assign(cap, csf_engine::SlotIdx());
    HIPCHK(e, e->bound_pin.alloc(2 * cap));
    e->dev_alive.assign(cap, 0);
    Dev &d = e->d;
    d.cap = (int64_t)cap;
    d.s = e->s.p;
    d.vdes = e->vdes.p;
    d.qbeg = e->qbeg.p;
    d.qlen = e->qlen.p;
    d.alive = e->alive.p;
    d.order = nullptr;
    d.ptr = e->ptr.p;
    d.znav = e->znav.p;
    d.znp = e->znp.p;
    d.ti = e->ti.p;
    d.hx = e->hx.p;
    d.hy = e->hy.p;
    d.lti = e->lti.p;
    d.zrid = e->zrid.p;
    d.dgood = e->dgood.p;
    d.ppsi = e->ppsi.p;
    d.F = e->F.p;
    d.F_rows = 6;
    d.status = e->status.p;
    d.part = e->part.p;
    d.froad = e->froad.p;
    d.rec = e->rec.p;
    d.rec2 = e->rec2.p;
    d.recs2 = e->recs2.p;
    d.perm = e->perm.p;
    d.pos = e->pos.p;
    d.recs = e->recs.p;
    d.recg = e->recg.p;
    d.rec_w = d.rec;
    d.recg_w = d.recg;
    d.rec2_w = d.rec2;
    d.recs_w = d.recs;
    d.chase_misc = nullptr;
    d.chase_err = nullptr;
    d.chase_round = 0;
    d.chase_gate = 0;
    d.part4 = nullptr;
    d.chase_tag = 0;
    d.chase_clock = nullptr;
    d.chase_slot = 0;
    d.src64 = e->s.p;
    d.src64_w = nullptr;
    d.mid_group = 0;
    d.recb = e->recb.p;
    d.borg = e->borg.p;
    d.bnd = e->bnd.p;
    d.bnd_next = e->bnd2.p;
    d.rorg = e->rorg.p;
    d.reclo = e->reclo.p;
    d.edge = e->edge.p;
    d.edge_n = e->edge_n.p;
    d.near_dropped = e->edge_n.p + 1;
    d.edge_head = e->edge_head.p;
    d.atrace = nullptr;
    d.snap = nullptr;
    if (!e->knobs.trace_agent.empty()) {   // 8 words per wave of 64 road users
        HIPCHK(e, e->atrace.alloc(8 * ((size_t)cap / 64 + 2) + 16 * ((size_t)cap / 4 + 2)));   // (csf_mid.hip: 16 words per workgroup)
        d.atrace = e->atrace.p;
    }
    d.index_order = e->knobs.handout_index;
    d.wg_order = nullptr;   // (set around a tick's own pair launch only: tick.inc wg_order_apply)
    d.wg_cost = nullptr;
    d.wg_groups = 0;
    d.trace = nullptr;
    if (!e->knobs.trace_blocks.empty()) {  // 3 words per wave: the grid is at most (cap/16) x MAX_SPLIT workgroups of 4 waves
        e->trace_words = 3 * 4 * ((size_t)cap / 16 + 1) * MAX_SPLIT;
        HIPCHK(e, e->trace.alloc(e->trace_words));
        HIPCHK(e, hipMemset(e->trace.p, 0, e->trace_words * sizeof(uint64_t)));
        d.trace = e->trace.p;
    }
    return CSF_OK;
}

constexpr int64_t TAIL_SLOTS = 4096;   // sentinel slots kept behind a binned population (csf_create adds them to the capacity)
void set_chunks(csf_engine *e);

void set_shard(csf_engine *e) {
    Dev &d = e->d;
    d.keep_lo = (e->world > 1 || e->loopback || e->nccl != nullptr) ? 1 : 0;   // (csf_dev.h: reclo)
    d.xbuf = nullptr;
    if (d.keep_lo) {
        // (set_shard has no error path: a failed allocation leaves the pointer NULL, and the exchange itself reports it)
        if (e->xbuf.n < 2 * e->rec.n && e->xbuf.alloc(2 * e->rec.n) != hipSuccess) e->xbuf.release();
        d.xbuf = e->xbuf.p;
    }
    if (e->world <= 1) {
        d.lo = 0;
        d.hi = d.n;
        // (sentinel slots behind the population take the arrivals between two re-binnings, csf_add_agents)
        d.n_pad = (std::min<int64_t>(e->cap, d.n + (e->loopback ? 0 : TAIL_SLOTS)) + 63) / 64 * 64;
    } else {
        // (several parameter sets: the class-segmented order starts every set's run at a multiple of 64 - room for that)
        const int64_t nk = (int64_t)e->classes.size(), seg_pad = nk > 1 && nk <= 16 ? 64 * nk : 0;
        int64_t shard = (d.n + seg_pad + e->world - 1) / e->world;
        shard = (shard + 63) / 64 * 64;
        d.lo = std::min<int64_t>(d.n, (int64_t)e->rank * shard);
        d.hi = std::min<int64_t>(d.n, d.lo + shard);
        d.n_pad = shard * e->world;
    }
    if (e->knobs.fake_world > 1) {  // timing aid (CSF_FAKE_SHARD=r/w): only rank r's receiver block of w is computed
        const int fr = e->knobs.fake_rank, fw = e->knobs.fake_world;   // (no communicator, other blocks' records go stale)
        int64_t shard = ((d.n + fw - 1) / fw + 63) / 64 * 64;
        d.lo = std::min<int64_t>(d.n, (int64_t)fr * shard);
        d.hi = std::min<int64_t>(d.n, d.lo + shard);
    }
    d.n_src = d.n_pad;          // every place of the source order may hold a road user (rebin() knows better)
    e->tail_tracked = false;
    set_chunks(e);
}

// the source chunks of the pair kernel's grid, for the d.n_src places of the source order that can hold road users
void set_chunks(csf_engine *e) {
    Dev &d = e->d;
    e->wgo.forget();
    int64_t nloc = d.hi - d.lo;
    int64_t blocks = (nloc + 15) / 16;
    int64_t units = std::max<int64_t>(1, d.n_src / 64);
    // Many more workgroups than the chip holds at once: receivers see very different numbers of sources (field
    // of view, position in the scene), so the hardware's dynamic workgroup dispatch is the load balancer.  Chunks
    // of one LDS tile (1024 sources) measured best for 1-, 2-, 4- and 8-way shards of N = 16 384 (DESIGN.md).
    int64_t split;
    if (d.n_src >= 16384) {
        split = blocks > 0 ? (16384 + blocks - 1) / blocks : 1;
        split = std::min<int64_t>(split, d.n_src / 1024);
    } else {
        split = blocks > 0 ? (1024 + blocks - 1) / blocks : 1;
    }
    split = std::max<int64_t>(1, std::min<int64_t>({split, (int64_t)MAX_SPLIT, units}));
    // large populations run the far-tile-skipping variant (rebin: recv_binned): most tiles of a chunk are
    // skipped unloaded, and longer chunks amortise the workgroup's start-up (config 4: 7.3 ms at 64 chunks, 6.2 at 8-16)
    if (d.n_src >= 65536 && d.p.model != CSF_BICYCLE) split = std::min<int64_t>(split, 16);
    if (e->knobs.nsplit > 0) split = std::max<int64_t>(1, std::min<int64_t>({(int64_t)e->knobs.nsplit, (int64_t)MAX_SPLIT, units}));
    // no empty chunk: with per = ceil(units / split) units per chunk only ceil(units / per) chunks hold sources (n = 1040:
    // 17 units, split 16 -> per 2 -> 9 chunks).  A workgroup of an empty chunk would leave its slot of d.part untouched,
    // and the combine phase would add whatever an earlier population layout left there.
    int64_t per = (units + split - 1) / split;
    // a chunk just over one LDS tile (16 batches) would load a second, nearly empty tile in every workgroup: the few
    // batches of arrivals behind a population that filled whole tiles get a chunk - and workgroups - of their own
    if (per > 16 && per < 32 && (units + 15) / 16 <= MAX_SPLIT && e->knobs.nsplit <= 0) per = 16;
    // 32 receivers per workgroup where that still leaves thousands of workgroups (N = 16 384 unsharded: 8192): measured
    // better from 8192 receivers up, worse for the few workgroups of small populations and 4-way shards
    d.rpb = (nloc >= 8192 || (nloc >= 4096 && d.n_src >= 16384)) ? 32 : 16;   // (4-way shard of 16 384: 38.9 -> 36.6 us with the wide workgroups below)
    if (e->knobs.rpb > 0) d.rpb = e->knobs.rpb == 32 ? 32 : 16;
    // ... and then workgroups of 8 waves on tiles of 2048 sources (csf_pair.hip: CW); below 65 536 places in chunks of 32 batches
    // (with 16 receivers for the shards of a large population: 8-way shard of 16 384 26.3 -> 25.1 us; unsharded 115 against 101)
    d.wide = (d.rpb == 32 || (d.rpb == 16 && (e->knobs.wide > 0 || d.n_src >= 16384))) && d.p.model != CSF_BICYCLE &&
             (e->knobs.nsplit <= 0 || d.n_src >= 65536) && (e->knobs.wide >= 0 ? e->knobs.wide != 0 : true);
    if (d.wide && d.n_src < 65536) per = 32;
    split = (units + per - 1) / per;
    d.n_split = (int32_t)split;
    d.chunk_units = (int32_t)per;
}

constexpr int64_t BIN_MIN_AGENTS = 1024;

// Which pair kernel (csf_pair.hip: launch_pair): 0 the cull-first kernel (binned records from BIN_MIN_AGENTS road users),
// 1 the plain all-pairs kernel, 2 cull-first without binning.  Below ~3 000 road users the plain kernel is the faster
// one - no classification, no queue, no re-binning launches: 14.1 against 20.7 us per tick at 1 024 TwoDBicycle, 11.1
// against 13.2 at 64, level at ~3 000, 41 against 32 at 4 096 (tools/variant_by_n.py; the Bicycle field crosses over at
// the same size) - and small populations are what the reference itself runs.  CSF_PAIR_VARIANT overrides.
constexpr int64_t PLAIN_BELOW = 3072;
int32_t pair_variant_for(const csf_engine *e, int64_t n) {
    return e->knobs.pair_variant >= 0 ? e->knobs.pair_variant : (n < PLAIN_BELOW ? 1 : 0);
}
