// engine/tick.inc - one tick enqueued: two launches in turn, one launch (mid-size), side by side (large), one wave (a handful); csf_step, csf_sync.
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

// One tick, all on the main stream (dependent launches in one stream cost ~2 us; a cross-stream event wait was
// measured at ~11 us here, more than running the destination-force phase beside the pair kernel saves):
//   main:  bounds - pair - road - agent(DEST|COMBINE|INTEGRATE) - [all-gather(records)]       (world > 1: RCCL)
// CSF_COMM_STREAM=second moves the collective to a second stream and issues the destination-force phase of the
// next tick (it needs only the agent's own state) before the wait on it:
// The pair term of a tick: one launch, or - class-segmented order, several parameter sets - one launch of the culling kernel
// per set's run of places, with that set's constants, field (vehicle class) and far-field radius; `base` carries what the
// caller wants of every launch (counters, next tick's circles or not).  The optional time stamps bracket the first launch.
// Heaviest group first (csf_wg_order.h; csf_engine::WgOrder has the hand-off): the tables of a tick's own pair launch on stream `st`,
// k the parity that picks them.  The order is formed again every CSF_WG_ORDER_TICKS ticks and as soon as a launch of this grid and
// these tiles has left its costs - the order kernel sits directly in front of the launch, in its stream; until then the launch
// takes the groups in index order (NULL).  Every other launch of the pair kernel (the warm launch, csf_count_pairs, calibration,
// the copies of Dev the scene and measurement calls make) leaves both pointers NULL: Dev holds them only from here to wg_order_done.
static int wg_order_apply(csf_engine *e, Dev &dd, int k, hipStream_t st) {
    dd.wg_order = nullptr;
    dd.wg_cost = nullptr;
    dd.wg_groups = 0;
    e->wgo.last = -1;
    if (e->knobs.wg_order == 0 || !e->segs.empty()) return CSF_OK;
    const int64_t groups = pair_order_groups(dd);
    const int chunks = (int)dd.n_split;
    if (groups <= 0 || chunks <= 0 || groups * chunks < e->knobs.wg_order_min) return CSF_OK;
    csf_engine::WgOrder &w = e->wgo;
    const size_t words = (size_t)groups * (size_t)chunks;
    if (w.groups != groups || w.chunks != chunks || w.cost[0].n < words) {   // another grid: nothing known about it
        w.forget();
        w.groups = groups, w.chunks = chunks;
        for (int t = 0; t < 2; t++) {   // (grow-only; an allocation waits for the device: no launch still reads what is freed)
            HIPCHK(e, w.cost[t].reserve(words));
            HIPCHK(e, w.order[t].reserve(words));
        }
    }
    if (w.cost_ok[k] && (!w.order_ok[k] || 2 * w.used[k] >= e->knobs.wg_order_ticks)) {
        launch_wg_order(w.cost[k].p, w.order[k].p, groups, chunks, st);
        w.order_ok[k] = true;
        w.used[k] = 0;
    }
    if (w.order_ok[k] && e->knobs.wg_order == 1) dd.wg_order = w.order[k].p;
    // (a workgroup whose source chunk is empty stores no cost: the first launch after the costs were forgotten starts from zeros,
    // so that no word of another grid or of older tiles is left in the table)
    if (!w.cost_ok[k]) HIPCHK(e, hipMemsetAsync(w.cost[k].p, 0, words * sizeof(uint32_t), st));
    dd.wg_cost = w.cost[k].p;
    dd.wg_groups = (int32_t)groups;
    w.cost_ok[k] = true;          // (for whatever follows this launch in its stream)
    w.used[k]++;
    w.last = k, w.last_ordered = dd.wg_order != nullptr;
    return CSF_OK;
}
static void wg_order_done(Dev &dd) { dd.wg_order = nullptr, dd.wg_cost = nullptr, dd.wg_groups = 0; }

static void launch_pair_all(csf_engine *e, const Dev &base, hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr) {
    if (e->segs.empty()) {
        launch_pair(base, e->main, t0, t1);
        return;
    }
    const bool one_grid = e->seg_total_by > 0 && base.pair_count == nullptr && e->knobs.seg_grid != 0;
    if (one_grid) {      // the runs of all TwoD-field sets in one grid
        Dev dd = base;
        dd.n_classes = 1;
        dd.recv_binned = 0;
        dd.segtab = e->segtab.p;
        dd.n_seg = (int32_t)e->h_segtab.size();
        launch_pair_segments(dd, e->seg_total_by, e->main, t0, t1);
        t0 = t1 = nullptr;
    }
    for (const csf_engine::Segment &sg : e->segs) {
        if (one_grid && e->classes[(size_t)sg.cls].model != CSF_BICYCLE) continue;   // (done above; the Bicycle field has a kernel of its own)
        Dev dd = base;
        dd.p = e->classes[(size_t)sg.cls];
        dd.p.priority_rule = base.p.priority_rule;
        dd.pc = sg.pc;
        dd.n_classes = 1;
        dd.src_beg = sg.beg;
        dd.n_src = sg.end;
        dd.chunk_units = sg.chunk_units;
        dd.n_split = sg.n_split;
        dd.part_base = sg.part_base;
        dd.recv_binned = 0;
        launch_pair(dd, e->main, t0, t1);
        t0 = t1 = nullptr;
    }
}

// Which order for the collective?  Timed on the communicator as it is - its ranks, its links - with launches that change
// nothing: the pair kernel on the records as they are (it writes partial sums and nothing else here) followed by the
// all-gather of the records (in place: what arrives is what was there), 8 + 32 times in stream order and 8 + 32 times with
// the collective on the second stream behind an event and a small kernel of the next tick in front of the wait.  The two
// times are max-reduced over the ranks, so that every rank keeps the same order.
static int calibrate_comm_stream_body(csf_engine *e) {
    if (!e->nccl || e->loopback) {
        e->comm_second = e->knobs.comm_second > 0;
        return CSF_OK;
    }
    {   // CSF_COMM_STREAM decides which collectives a rank issues below: every rank must have read the same value, or the
        // ranks that measure wait for the ones that do not.  Agree on it before branching (max and min over the ranks).
        float v[2] = {(float)e->knobs.comm_second, -(float)e->knobs.comm_second};
        DevBuf<float> t;
        HIPCHK(e, t.alloc(2));
        HIPCHK(e, hipMemcpy(t.p, v, sizeof v, hipMemcpyHostToDevice));
        NCCLCHK(e, g_rccl.AllReduce(t.p, t.p, 2, ncclFloat32, ncclMax, e->nccl, e->main));
        HIPCHK(e, hipStreamSynchronize(e->main));
        HIPCHK(e, hipMemcpy(v, t.p, sizeof v, hipMemcpyDeviceToHost));
        if (v[0] != -v[1]) return fail(e, CSF_E_STATE, "CSF_COMM_STREAM differs between the ranks of this communicator: set it on all of them or on none");
    }
    if (e->knobs.comm_second >= 0) {
        e->comm_second = e->knobs.comm_second > 0;
        return CSF_OK;
    }
    {
        int rc = set_fov_band(e);
        if (rc) return rc;
    }
    Dev dd = e->d;
    dd.edge = nullptr;          // (no per-agent launch follows that would take undecided pairs over)
    dd.bnd_next = nullptr;      // (the circles stay as they are)
    struct Events {   // (destroyed on every way out)
        hipEvent_t a = nullptr, b = nullptr;
        ~Events() {
            if (a) (void)hipEventDestroy(a);
            if (b) (void)hipEventDestroy(b);
        }
    } evs;
    HIPCHK(e, hipEventCreate(&evs.a));
    HIPCHK(e, hipEventCreate(&evs.b));
    const hipEvent_t a = evs.a, b = evs.b;
    float us[2] = {0.f, 0.f};
    for (int mode = 0; mode < 2; mode++) {
        e->comm_second = mode == 1;
        for (int it = 0; it < 40; it++) {
            if (it == 8) HIPCHK(e, hipEventRecord(a, e->main));
            if (mode == 1) {
                if (dd.recs_valid) launch_sorted_copy(dd, e->main);   // (stands for the destination-force phase of the next tick)
                int rc = wait_gather(e);
                if (rc) return rc;
            }
            if (dd.n_live > 1 && dd.hi > dd.lo) launch_pair_all(e, dd, nullptr, nullptr);
            if (mode == 1) HIPCHK(e, hipEventRecord(e->ev_integ, e->main));
            int rc = all_gather_records(e);
            if (rc) return rc;
        }
        int rc = wait_gather(e);
        if (rc) return rc;
        HIPCHK(e, hipEventRecord(b, e->main));
        HIPCHK(e, hipStreamSynchronize(e->main));
        if (e->comm) HIPCHK(e, hipStreamSynchronize(e->comm));
        float ms = 0.f;
        HIPCHK(e, hipEventElapsedTime(&ms, a, b));
        us[mode] = ms * 1e3f / 32.f;
    }
    {   // the slowest rank's figures, on every rank
        DevBuf<float> t;
        HIPCHK(e, t.alloc(2));
        HIPCHK(e, hipMemcpy(t.p, us, sizeof us, hipMemcpyHostToDevice));
        NCCLCHK(e, g_rccl.AllReduce(t.p, t.p, 2, ncclFloat32, ncclMax, e->nccl, e->main));
        HIPCHK(e, hipStreamSynchronize(e->main));
        HIPCHK(e, hipMemcpy(us, t.p, sizeof us, hipMemcpyDeviceToHost));
    }
    e->comm_cal_us[0] = us[0];
    e->comm_cal_us[1] = us[1];
    e->comm_second = us[1] < us[0];
    return CSF_OK;
}

// (the flag is set only when the measurement went through: after an error the order is the plain one - collective in stream
// order - and the next csf_step tries again)
int calibrate_comm_stream(csf_engine *e) {
    const int rc = calibrate_comm_stream_body(e);
    if (rc) e->comm_second = false;
    else e->comm_calibrated = true;
    return rc;
}

// ---- mid-size populations: the whole tick in one launch (csf_mid.hip) --------------------------------------------------
// One device, one parameter set, the plain all-pairs kernel's range (below PLAIN_BELOW road users; up to SMALL_MAX the one-wave
// kernel is faster still), nothing that wants the two kernels apart (time stamps per kernel, wave traces, pair counters).
// Where two launches take over again (tools/mid_rate.py, profiles/r5_v2_models_mid_rate.jsonl; microseconds per tick, one launch /
// two): the classes with twelve waves per workgroup and the cull-first pair sums win up to ~2 100 road users (2 048: TwoD 20.9 /
// 22.0, PlanarPoint 20.6 / 21.7), the InvPendulum (eight waves) and the Bicycle field (four receivers per item, no cull) only
// to ~1 300 (1 024: 18.2 / 19.2 and 13.7 / 14.0; 2 048: 29.2 / 26.0 and 20.0 / 17.5).

// A population of several parameter sets (any classes), or of the UncontrolledVehicle's class: mid_tick_kernel does not take it.
static bool mid_is_classes(const csf_engine *e) { return e->classes.size() > 1 || e->d.p.model == CSF_UNCONTROLLED; }

// mid_classes_kernel (csf_mid_classes.hip) has plain items and eight waves.  Where it was measured faster than the general path
// (tools/mid_classes_rate.py, profiles/mid_classes_rate.jsonl; DESIGN.md 4.7c has the table; the median of five windows below the general
// path's minimum): every composition up to 1 024 road users - at 1 279 the populations of one class lose (two TwoD sets 22.7 against 21.4 us,
// 32 sets 23.1 against 22.4) -, but for a population of ONE vehicle class whose road term is not summed inside the launch, which wins by
// 6 ... 11 % up to 256 road users (one pass of the per-agent phases: the launch saved is all there is to gain), loses at 600 (two sets 14.7
// against 14.2) and wins again at 1 024 (15.9 against 18.5): between the two it keeps the general path.
constexpr int64_t MID_CLASSES_BELOW = 1025;
constexpr int64_t MID_CLASSES_ONE_CLASS_UPTO = 256, MID_CLASSES_ONE_CLASS_FROM = 1024;
static int64_t mid_below_for(const csf_engine *e) {
    if (e->knobs.mid_below > 0) return e->knobs.mid_below;
    if (mid_is_classes(e)) return MID_CLASSES_BELOW;
    return e->d.p.model == CSF_INVPEND || e->d.p.model == CSF_BICYCLE ? 1280 : 2176;
}

// what the one-launch tick asks whatever its kernel
static bool mid_common_ok(const csf_engine *e) {
    const Dev &d = e->d;
    return e->knobs.fused_mid != 0 && e->knobs.pair_variant < 0 && d.pair_variant == 1 && d.n_live > 1 && d.n_live < mid_below_for(e) &&
           e->world == 1 && !e->nccl && !e->loopback && e->knobs.fake_world <= 1 && e->profile <= 0 &&
           d.trace == nullptr && d.pair_count == nullptr && d.lo == 0 && d.hi == d.n && e->segs.empty() && e->state_all_current &&
           d.src_beg == 0 && d.n_src / 64 * 8 <= 384;                  // (csf_mid.hip: MID_ITEMS_MAX items of the largest group)
}

// ... and does mid_classes_kernel take this population?  The switch of csf_mid_classes on, several sets or the UncontrolledVehicle's
// class, no set of a BalancingRiderBicycle (its one-launch tick was measured slower than two launches: csf_mid.hip), the table within
// what the kernel stages - and everything mid_tick_kernel asks.  A single set of a rider class keeps mid_tick_kernel, switch or no switch.
static bool mid_road_ok(const csf_engine *e);
static bool mid_takes_classes(const csf_engine *e) {
    if (!e->mid_classes || !mid_is_classes(e) || (e->d.model_mask & (1 << CSF_BALANCINGRIDER)) != 0 || e->classes.size() > 256) return false;
    const int64_t n = e->d.n_live;
    // (no trace of the workgroups' phases - tools/mid_timeline.py reads mid_tick_kernel's stamps, this kernel leaves none -, and more road
    // users than the one-wave tick's range: the smallest measured cell is 64, and 33 is where the one-launch tick begins)
    if (e->d.atrace != nullptr || n <= SMALL_MAX) return false;
    // (Dev::model_mask is formed from the TABLE of sets, derive_consts: a table that lists a second class no road user belongs to counts as
    // several classes here - it is admitted between 257 and 1 023 road users too, and wave 0 runs an empty pass per phase for that class)
    const bool one_class = (e->d.model_mask & (e->d.model_mask - 1)) == 0;
    if (one_class && !mid_road_ok(e) && n > MID_CLASSES_ONE_CLASS_UPTO && n < MID_CLASSES_ONE_CLASS_FROM) return false;   // (measured slower: above)
    return mid_common_ok(e);
}

static bool mid_fused_ok(const csf_engine *e) {
    if (mid_is_classes(e)) return mid_takes_classes(e);
    return mid_common_ok(e) && e->d.p.model != CSF_BALANCINGRIDER;
}

// ... and does its launch sum the road term too (csf_mid.hip: the ROAD instances; DESIGN.md 4.7b)?  The switch of csf_mid_road on, a
// road, no lattice (csf_road.hip sums a lattice its own way), and no more padded vertices than MID_ROAD_MAX.  False: launch_road goes
// in front of the plain instance, as before there was a switch - and inside a batch the member is stepped in turn.
static bool mid_road_ok(const csf_engine *e) {
    const Dev &d = e->d;
    return e->mid_road && d.nv > 0 && d.rg_nx == 0 && d.nv_pad <= MID_ROAD_MAX;
}

// the second halves of the double buffers (allocations synchronise: never inside something that is being timed)
static int alt_alloc(csf_engine *e) {
    const size_t nrec = e->rec.n;
    if (e->rec_alt.n >= nrec) return CSF_OK;
    HIPCHK(e, e->rec_alt.alloc(nrec));
    HIPCHK(e, e->recg_alt.alloc(e->recg.n));
    HIPCHK(e, e->rec2_alt.alloc(e->rec2.n));
    HIPCHK(e, e->src64_a.alloc(3 * (size_t)e->cap));
    HIPCHK(e, e->src64_b.alloc(3 * (size_t)e->cap));
    HIPCHK(e, e->recs_alt.alloc(e->recs.n));
    // the permanent sentinel (alloc_all: the last record, no slot's; the padding of the class-segmented order points at it)
    // exists in BOTH halves: after an odd number of one-launch ticks d.rec is the other half, and a population that then
    // outgrows this path would read (0, 0, 0, 0) - a road user at the origin - where its order is padded
    HIPCHK(e, hipMemcpyAsync(e->rec_alt.p + e->sent_slot, e->rec.p + e->sent_slot, sizeof(float4), hipMemcpyDeviceToDevice, e->main));
    HIPCHK(e, hipMemcpyAsync(e->rec2_alt.p + e->sent_slot, e->rec2.p + e->sent_slot, sizeof(float2), hipMemcpyDeviceToDevice, e->main));
    if ((size_t)e->sent_slot < e->recg.n)
        HIPCHK(e, hipMemcpyAsync(e->recg_alt.p + e->sent_slot, e->recg.p + e->sent_slot, sizeof(float4), hipMemcpyDeviceToDevice, e->main));
    return CSF_OK;
}

// The halves of the double buffers that the engine's Dev does not read this tick - a one-launch or side-by-side tick writes next
// tick's records there -, and the fp64 snapshots of (x, y, psi): `cur` holds the state of the tick's start, `nxt` takes its end.
struct OtherHalves {
    float4 *rec, *recg, *recs;
    float2 *rec2;
    double *cur, *nxt;
};

static OtherHalves other_halves(const csf_engine *e) {
    const Dev &d = e->d;
    return {d.rec == e->rec.p ? e->rec_alt.p : e->rec.p,     d.recg == e->recg.p ? e->recg_alt.p : e->recg.p,
            d.recs == e->recs.p ? e->recs_alt.p : e->recs.p, d.rec2 == e->rec2.p ? e->rec2_alt.p : e->rec2.p,
            e->mid_cur_is_a ? e->src64_a.p : e->src64_b.p,   e->mid_cur_is_a ? e->src64_b.p : e->src64_a.p};
}

// a launch's view writes them (with_recs: the binned copy too - the side-by-side tick; the one-launch tick keeps none)
static void write_other_halves(Dev &dd, const OtherHalves &o, bool with_recs) {
    dd.rec_w = o.rec;
    dd.recg_w = o.recg;
    dd.rec2_w = o.rec2;
    if (with_recs) dd.recs_w = o.recs;
    dd.src64 = o.cur;
    dd.src64_w = o.nxt;
}

// the halves trade places: what the launch wrote is what every later launch reads
static void trade_halves(csf_engine *e, const OtherHalves &o, bool with_recs) {
    Dev &d = e->d;
    d.rec = d.rec_w = o.rec;
    d.recg = d.recg_w = o.recg;
    d.rec2 = d.rec2_w = o.rec2;
    if (with_recs) d.recs = d.recs_w = o.recs;
    e->mid_cur_is_a = !e->mid_cur_is_a;
}

// the other halves <- this tick's records (sentinels of free and padding slots included) and state
static int mid_sync(csf_engine *e, unsigned *through = nullptr) {
    Dev &d = e->d;
    {
        int rca = alt_alloc(e);
        if (rca) return rca;
    }
    const OtherHalves o = other_halves(e);
    // (one launch: six copy / fill calls cost a launch and its gap each, once per re-binning)
    launch_chase_sync(d, o.rec, o.recg, o.recs, o.rec2, o.cur, (int64_t)std::min((size_t)d.n_pad, e->recg.n), through, e->main);
    HIPCHK(e, hipGetLastError());
    if (through == nullptr) e->chase_resume = false;              // (the one-launch tick's call: the gate's counter is as it was)
    e->mid_synced = true;
    return CSF_OK;
}

// The one-launch tick in three parts, which csf_step (below) and the mid-size members of a batch (abi_batch.inc) both run: what
// comes in front of the launch, the launch's view of the engine, and the book-keeping behind it.
//
// In front: the re-binning where it is due (new origins of the precise records, and a new d.n_src, which the gate reads: *take
// false - the bounds are in place, the caller carries on with two launches), the rounding bands, the other halves made equal.
// With csf_engine::mid_defer the launches of a re-binning on the plain order and of the copy are noted in mid_deferred instead.
static int mid_prelude(csf_engine *e, bool *take) {
    *take = false;
    int rc;
    if ((rc = bounds_before_pair(e))) return rc;
    if (!mid_fused_ok(e)) return CSF_OK;
    if ((rc = set_fov_band(e))) return rc;
    if (!e->mid_synced) {
        if (e->mid_defer && !e->d.recs_valid && e->rec_alt.n >= e->rec.n) {
            e->mid_deferred |= MID_DUE_SYNC;
            e->chase_resume = false;
            e->mid_synced = true;
        } else if ((rc = mid_sync(e))) return rc;
    }
    *take = true;
    return CSF_OK;
}

// road users per workgroup: about one workgroup (of eight waves, at the per-agent code's 255 registers a CU holds one) per CU
static int mid_group_for(const csf_engine *e) {
    int G = e->knobs.mid_group;
    if (G != 4 && G != 8 && G != 16 && G != 32) {
        G = 4;
        while (G < 32 && (e->d.hi - e->d.lo + G - 1) / G > 256) G *= 2;
    }
    return G;
}

// behind the launch: the halves trade places, the counters move on
static void mid_ticked(csf_engine *e, const OtherHalves &o, bool batched, bool road, bool classes) {
    trade_halves(e, o, false);
    bounds_after_pair(e, true);
    e->moves++;
    e->mid_ticks++;
    if (road) e->mid_road_ticks++;
    if (classes) e->mid_classes_ticks++;
    if (batched) e->batch_mid_ticks++;
    e->d.tick++;
}

// (behind mid_prelude)
static int enqueue_mid_tick(csf_engine *e) {
    Dev &d = e->d;
    const bool road = mid_road_ok(e);                             // (the launch below sums the road term itself)
    if (d.nv > 0 && !road) launch_road(d, e->main);
    const OtherHalves o = other_halves(e);
    Dev dd = d;
    write_other_halves(dd, o, false);                             // (this tick writes no binned copy)
    dd.mid_group = mid_group_for(e);
    // (nothing has traded places yet: a refused launch leaves the engine where it was)
    const bool classes = mid_takes_classes(e);                    // (several sets or classes: csf_mid_classes.hip in place of the pair launch and the launches per class)
    if (!(classes ? launch_mid_classes(dd, road, e->main) : launch_mid_tick(dd, road, e->main)))
        return fail(e, CSF_E_STATE, "the one-launch tick does not take this population (%lld sources, groups of %d)", (long long)d.n_src, dd.mid_group);
    HIPCHK(e, hipGetLastError());
    mid_ticked(e, o, false, road, classes);
    return CSF_OK;
}

// ---- the per-agent launch inside the pair launch's drain (csf_dev.h: part4) ---------------------------------------------------
// At the headline size the pair launch idles most CUs for its last ~24 us while the per-agent launch (8 us + two launch gaps) waits
// behind it.  Here the two run side by side on the engine's two streams, which trade places every tick:
//   tick t:      P: pair(t)                      Q: gate(t) - agent(t)     [agent(t) waits, per 64 slots, for pair(t)'s arrivals]
//   tick t + 1:  Q: pair(t + 1)  (behind agent(t): every record is in place)      P: gate(t + 1) - agent(t + 1)  (behind pair(t))
// No event between the streams in steady state: a kernel only ever waits (on the device) for one that was enqueued BEFORE it, on
// a stream whose earlier work does not wait for it - so whatever the runtime maps the streams to, the grid drains (mapped to one
// hardware queue the launches simply serialise).  Next tick's records go to the other halves of the double buffers, hand-overs
// read the fp64 snapshot of the tick's start (as in csf_mid.hip).  The streams meet (two events) when the path is left.
static bool rebin_due(const csf_engine *e) {   // (bounds_before_pair's condition: this tick renews the binned order, on the main stream)
    return e->ticks_since_rebin + e->moved_unbinned >= e->knobs.rebin_ticks || e->ticks_since_rebin * e->churn >= e->knobs.rebin_churn;
}

// could ticks of this engine take the path at all (what does not change from tick to tick)?
static bool chase_shape(const csf_engine *e) {
    const Dev &d = e->d;
    const int m = d.p.model;
    return e->knobs.chase != 0 && (m == CSF_TWOD || m == CSF_INVPEND || m == CSF_PLANARPOINT) && e->classes.size() == 1 && d.pair_variant == 0 && d.classify &&
           !d.recv_binned && e->world == 1 && !e->nccl && !e->loopback && d.nv == 0 && d.hist == nullptr && e->comm != nullptr;   // (CSF_FAKE_SHARD: a rank's block of receivers, for tools/fake_shard.py)
}

// ... and what does: everything but "no re-binning this tick".  The receiver range is asked about here only: chase_shape says yes
// to a rank's block whatever CSF_FAKE_SHARD is (the upload then makes the path's buffers, which harms nobody), a tick takes a
// partial block only under CSF_FAKE_SHARD.
static bool chase_eligible(const csf_engine *e, int64_t ticks_left) {
    const Dev &d = e->d;
    return chase_shape(e) && d.n_classes == 1 && d.recs_valid && pair_shape(d).family == PairShape::CULL && d.n_split <= 16 &&
           d.part_base == 0 && d.pair_count == nullptr && e->segs.empty() && e->state_all_current &&   // (wave traces allowed: tools/chase_timeline.py)
           e->pend.empty() && !e->bound_stale && e->bounds_fresh && d.n_live > 1 && d.hi > d.lo && (d.lo & 63) == 0 && d.replay_len == nullptr &&
           ((d.lo == 0 && d.hi == d.n) || e->knobs.fake_world > 1) && (e->chase_prev || ticks_left >= 4);
}

static bool chase_ok(const csf_engine *e, int64_t ticks_left) { return !rebin_due(e) && chase_eligible(e, ticks_left); }

// the two streams meet: whatever follows runs on the main stream alone
static int chase_join(csf_engine *e) {
    if (!e->chase_prev) return CSF_OK;
    // (one event: the main stream behind the second; the second stream is put behind the main one when the path is entered again)
    HIPCHK(e, hipEventRecord(e->ev_gather, e->comm));
    HIPCHK(e, hipStreamWaitEvent(e->main, e->ev_gather, 0));
    e->chase_prev = false;
    return CSF_OK;
}

// what the side-by-side tick needs beside the engine's arrays (allocations synchronise: before a measurement, not inside it)
static int chase_alloc(csf_engine *e) {
    if (e->part4.n < (size_t)16 * (size_t)e->cap) HIPCHK(e, e->part4.alloc((size_t)16 * (size_t)e->cap));   // (zero: no tick's tag)
    if (e->chase_misc.n == 0) {
        HIPCHK(e, e->chase_misc.reserve(64));
        // once per engine: the runtime makes a stream's hardware queue when the stream is first used, and loads a kernel's code when it
        // is first asked for - a hundred microseconds and more each, which would land in the first side-by-side tick (and, for a
        // caller who times twenty ticks, in the figure)
        HIPCHK(e, hipMemsetAsync(e->chase_misc.p, 0, 64 * sizeof(unsigned), e->comm));
        if (!e->chase_err.p) {   // (the word a wait that gives up sets: mapped host memory, so that csf_sync need not copy anything)
            HIPCHK(e, e->chase_err.alloc(16));
            std::memset(e->chase_err.p, 0, 64);
        }
        preload_chase_kernels();
        // ... and a queue gets its scratch memory when a kernel that spills is first dispatched on it: one pair launch that hands
        // nothing over (as csf_count_pairs's: partial sums and next tick's circles are written again by the tick's own launch)
        // and a kernel that asks for the per-agent kernels' bytes per lane, on the second stream
        if (e->d.n_live > 1 && e->d.hi > e->d.lo && !e->dirty_layout_for_warm()) {
            // This launch writes the live partial sums, next tick's circles and the near-pair counter, and reads the records the
            // per-agent kernel rewrites in place.  Where the upload did not run it (chase_shape was false then), it may come with
            // hundreds of ticks queued on the main stream (chase_take: the measurement's first period starts at tick 256 or later of
            // a long call), and nothing else orders the second stream behind them: so the second stream waits for everything
            // enqueued on the main one, and the synchronisation below waits for those ticks as well.  No live tick can overlap it
            // (once per engine, before the measurement's first event).
            HIPCHK(e, hipEventRecord(e->ev_integ, e->main));
            HIPCHK(e, hipStreamWaitEvent(e->comm, e->ev_integ, 0));
            Dev dw = e->d;
            dw.edge = nullptr;
            dw.pair_count = nullptr;
            dw.trace = nullptr;
            launch_pair(dw, e->comm);
        }
        launch_chase_scratch_warm(e->chase_misc.p, e->comm);
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipStreamSynchronize(e->comm));
    }
    return alt_alloc(e);
}

// What an engine measured holds for the next engine of the same kind in this process (same device, same rider class, same size to a
// factor of two): bench.py's timed engine takes over what its scratch engine found, and a caller that steps a few ticks per call
// - too few for a measurement of its own - is served by an earlier one.  0: nothing measured yet.
static std::atomic<int> g_chase_found[8][8][32];
static std::atomic<int> *chase_found_slot(const csf_engine *e) {
    int b = 0;
    for (int64_t n = std::max<int64_t>(e->d.n, 1); n > 1 && b < 31; n >>= 1) b++;
    return &g_chase_found[e->device & 7][e->d.p.model & 7][b];
}

// the measurement's last event has been reached: decide
static void chase_cal_resolve(csf_engine *e, bool wait) {
    if (e->cal_phase != 4) return;
    if (wait ? hipEventSynchronize(e->cal_ev[3]) != hipSuccess : hipEventQuery(e->cal_ev[3]) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    float t[3] = {0, 0, 0};
    bool ok = true;
    for (int k = 0; k < 3; k++) ok = ok && hipEventElapsedTime(&t[k], e->cal_ev[k], e->cal_ev[k + 1]) == hipSuccess && e->cal_ticks[k] > 0;
    if (ok) {
        for (int k = 0; k < 3; k++) t[k] = t[k] * 1e3f / (float)e->cal_ticks[k];        // microseconds per tick of every period
        e->chase_cal_us[0] = 0.5 * (double)(t[0] + t[2]);
        e->chase_cal_us[1] = (double)t[1];
        // (the side-by-side period against the MEAN of the in-turn periods on either side of it: a clock that is still ramping up
        // cancels; by a per cent, so that noise does not decide)
        e->chase_state = t[1] < 0.99f * 0.5f * (t[0] + t[2]) ? 1 : -1;
        chase_found_slot(e)->store(e->chase_state);
    }
    (void)hipGetLastError();
    e->cal_phase = 0;
}

// This tick beside the pair launch?  CSF_CHASE=1 drives the one-off measurement: three whole periods between re-binnings - in turn, side
// by side, in turn -, each from its re-binning tick to the next, so that what entering and leaving the side-by-side path costs once
// per period (the halves made equal, the streams meeting) is part of what is compared.
static bool chase_take(csf_engine *e, int64_t ticks_left) {
    const bool ok = chase_ok(e, ticks_left);
    if (e->knobs.chase != 1 || e->chase_state != 0) return ok && (e->knobs.chase >= 2 || e->chase_state == 1);
    if (e->cal_phase == 0) {
        const int found = chase_found_slot(e)->load();                     // an earlier engine of this kind has measured
        if (found != 0) {
            e->chase_state = found;
            return ok && found == 1;
        }
    }
    if (e->cal_phase == 4) {
        chase_cal_resolve(e, false);
        return ok && e->chase_state == 1;
    }
    if (rebin_due(e) && chase_eligible(e, ticks_left)) {                   // a period ends, the next begins (this tick: the launches in turn)
        if (e->cal_phase == 0) {
            // three periods inside this call, on clocks that have had time to come up (a fresh process finds the device in a low
            // power state: its first few hundred ticks run up to 1.7 x slower and speed up as they go), nothing else sampled
            if (ticks_left < 3 * e->knobs.rebin_ticks + 2 || e->d.tick < 256 || e->profile > 0) return false;
            for (hipEvent_t &ev : e->cal_ev)
                if (!ev && hipEventCreate(&ev) != hipSuccess) return false;
            if (chase_alloc(e) != CSF_OK) return false;                     // (now, not inside the side-by-side period)
            if (hipEventRecord(e->cal_ev[0], e->main) != hipSuccess) return false;
            e->cal_phase = 1;
            for (int64_t &c : e->cal_ticks) c = 0;
        } else {
            if ((e->cal_phase == 2 && chase_join(e) != CSF_OK) || hipEventRecord(e->cal_ev[e->cal_phase], e->main) != hipSuccess) {
                e->cal_phase = 0;
                return false;
            }
            e->cal_phase++;
        }
        if (e->cal_phase <= 3) e->cal_ticks[e->cal_phase - 1]++;
        return false;
    }
    if (e->cal_phase >= 1 && e->cal_phase <= 3) {
        if (!ok) {                                                          // (something else got in the way: start over later)
            e->cal_phase = 0;
            return false;
        }
        e->cal_ticks[e->cal_phase - 1]++;
        return e->cal_phase == 2;
    }
    return false;
}

static int enqueue_chase_tick(csf_engine *e, csf_engine::ProfSlot *ps, csf_engine::ProfSlot *po) {
    Dev &d = e->d;
    int rc;
    if ((rc = bounds_before_pair(e))) return rc;                 // (chase_ok: no re-binning, circles in place - nothing is launched)
    if ((rc = set_fov_band(e))) return rc;
    if (!e->chase_prev) {                                         // entering: the second stream behind everything so far
        if ((rc = chase_alloc(e))) return rc;
        // Nothing but side-by-side ticks since the halves were made equal (the last call ended with such ticks and nothing ran in
        // between): the gate's counter, round and stream parity carry on, and entering costs one event.  Else one launch makes
        // the halves equal and clears the gate's counter (the error word stays).
        if (!e->mid_synced || !e->chase_resume) {
            if ((rc = mid_sync(e, e->chase_misc.p))) return rc;
            e->chase_round = 0;
            e->chase_parity = 0;
        }
        e->chase_resume = true;
        HIPCHK(e, hipEventRecord(e->ev_integ, e->main));
        HIPCHK(e, hipStreamWaitEvent(e->comm, e->ev_integ, 0));
    }
    hipStream_t P = e->chase_parity ? e->comm : e->main, Q = e->chase_parity ? e->main : e->comm;
    const OtherHalves o = other_halves(e);
    const int64_t groups = pair_shape(d).groups(d.hi - d.lo), wgs = groups * d.n_split;   // (the grid launch_pair takes below)
    e->chase_round++;
    Dev dd = d;
    write_other_halves(dd, o, true);
    dd.chase_misc = e->chase_misc.p;
    dd.chase_err = e->chase_err.dev;
    dd.chase_round = e->chase_round;
    dd.part4 = e->part4.p;
    dd.chase_tag = (uint32_t)(e->chase_ticks + 1) | 0x40000000u;   // (never 0, never a tag an older granule carries)
    dd.chase_clock = nullptr;
    if (!e->knobs.chase_clock.empty()) {   // (a ring of 128 ticks, initialised once: the tool reads fewer than that)
        if (e->chase_clock.n == 0) {
            HIPCHK(e, e->chase_clock.alloc(128 * 8));
            std::vector<unsigned long long> init(128 * 8, 0ull);
            for (int r = 0; r < 128; r++) init[8 * r + 0] = init[8 * r + 4] = ~0ull;       // (minima start high)
            HIPCHK(e, hipMemcpy(e->chase_clock.p, init.data(), init.size() * sizeof(init[0]), hipMemcpyHostToDevice));
        }
        dd.chase_clock = e->chase_clock.p;
        dd.chase_slot = (uint32_t)(e->chase_ticks & 127);
    }
    // (cumulative: the counter is cleared when the path is entered.  At least ONE workgroup of THIS launch: the launch sits behind the
    // previous tick's per-agent kernel in its stream, so a workgroup of it through means that kernel has ended - whose state this
    // tick's per-agent kernel reads from its first instruction on)
    dd.chase_gate = (uint32_t)((int64_t)(e->chase_round - 1) * wgs + std::max<int64_t>(1, wgs * e->knobs.chase_gate_pct / 100));
    if ((rc = wg_order_apply(e, dd, e->chase_parity ? 1 : 0, P))) return rc;
    launch_pair(dd, P, ps ? ps->ev[0] : nullptr, ps ? ps->ev[1] : nullptr);
    wg_order_done(dd);
    if (ps) ps->pair = true;
    bounds_after_pair(e, true);
    if (!launch_agent_chase(dd, Q, po ? po->ev[4] : nullptr, po ? po->ev[5] : nullptr))
        return fail(e, CSF_E_STATE, "the per-agent kernel beside the pair launch is not built for vehicle class %d", (int)d.p.model);
    if (po) po->agent = true;
    HIPCHK(e, hipGetLastError());
    trade_halves(e, o, true);
    e->chase_parity ^= 1;
    e->chase_prev = true;
    e->chase_ticks++;
    e->moves++;
    d.tick++;
    return CSF_OK;
}

//   main:  agent(DEST) - wait(ev_gather) - bounds - pair - road - agent(COMBINE|INTEGRATE) - record(ev_integ)
//   comm:  wait(ev_integ) - all-gather(records) - record(ev_gather)
static int enqueue_two_launch_tick(csf_engine *e, bool bounds_done);

static int enqueue_tick(csf_engine *e, int64_t ticks_left = 1) {
    if (chase_take(e, ticks_left)) {                              // the per-agent launch beside the pair launch (large populations)
        int rcp = CSF_OK;
        csf_engine::ProfSlot *ps = prof_slot(e, &rcp);
        if (rcp) return rcp;
        return enqueue_chase_tick(e, ps, (ps && ((e->prof_ticks++ % 8 == 0) || !e->knobs.chase_clock.empty())) ? ps : nullptr);
    }
    {
        int rcj = chase_join(e);
        if (rcj) return rcj;
    }
    bool bounds_done = false;
    if (mid_fused_ok(e)) {
        // the re-binning inside may move d.n_src past what the one-launch tick takes: mid_prelude asks again behind it, and the
        // tick carries on with two launches (the bounds are in place) rather than be lost
        bool take = false;
        int rcb = mid_prelude(e, &take);
        if (rcb) return rcb;
        bounds_done = true;
        if (take) return enqueue_mid_tick(e);
    }
    return enqueue_two_launch_tick(e, bounds_done);
}

// the pair launch and the per-agent launch in turn (bounds_done: bounds_before_pair has run for this tick)
static int enqueue_two_launch_tick(csf_engine *e, bool bounds_done) {
    Dev &d = e->d;
    e->mid_synced = false;
    const bool sharded = e->world > 1 || e->nccl != nullptr || e->loopback;  // a 1-rank communicator rehearses the sharded path
    int rc = CSF_OK;
    csf_engine::ProfSlot *ps = prof_slot(e, &rc);
    if (rc) return rc;
    // time stamps cost a few microseconds of launch gap per kernel: the pair kernel (what the roofline is computed from)
    // takes them on every sampled tick, the other kernels on every 8th of those
    csf_engine::ProfSlot *po = (ps && (e->prof_ticks++ % 8 == 0)) ? ps : nullptr;
    const bool overlap = sharded && !e->loopback && comm_second_stream(e);
    if (overlap) {
        launch_agent(d, PH_DEST, e->main);
        if ((rc = wait_gather(e))) return rc;
    }
    if (!bounds_done && (rc = bounds_before_pair(e))) return rc;
    // sharded: the other ranks' records arrived in index order; a coalesced tile fill from the binned copy saves the
    // pair kernel 5 - 7 us at every shard size, the copy costs ~3 us
    if (sharded && d.recs_valid && e->ticks_since_rebin > 1) {
        launch_sorted_copy(d, e->main, e->xbuf_fresh);
        e->xbuf_fresh = false;
    }
    if ((rc = set_fov_band(e))) return rc;
    if (d.n_live > 1 && d.hi > d.lo) {
        if ((rc = wg_order_apply(e, d, (int)(d.tick & 1), e->main))) return rc;
        launch_pair_all(e, d, ps ? ps->ev[0] : nullptr, ps ? ps->ev[1] : nullptr);
        wg_order_done(d);
        if (ps) ps->pair = true;
    }
    bounds_after_pair(e, true);
    if (d.nv > 0 && d.hi > d.lo) {
        launch_road(d, e->main, po ? po->ev[2] : nullptr, po ? po->ev[3] : nullptr);
        if (po) po->road = true;
    }
    launch_agent(d, overlap ? (PH_COMBINE | PH_INTEGRATE) : (PH_DEST | PH_COMBINE | PH_INTEGRATE), e->main,
                 po ? po->ev[4] : nullptr, po ? po->ev[5] : nullptr);
    // a rank integrates its own block only: the others' fp64 state is stale from now on (a 1-rank communicator owns every block)
    if (e->world > 1 || e->loopback) e->state_all_current = false;
    e->moves++;
    if (po) po->agent = true;
    HIPCHK(e, hipGetLastError());
    d.tick++;
    if (sharded && !e->loopback) {
        if (overlap) HIPCHK(e, hipEventRecord(e->ev_integ, e->main));
        hipStream_t cs = overlap ? e->comm : e->main;
        if (po) HIPCHK(e, hipEventRecord(po->ev[6], cs));
        if ((rc = all_gather_records(e))) return rc;
        if (po) {
            HIPCHK(e, hipEventRecord(po->ev[7], cs));
            po->gather = true;
        }
    }
    return CSF_OK;
}

// the loopback "all-gather": every member's own record block is copied into the record arrays of the others
static int loopback_exchange(csf_engine *const *g, int world) {
    for (int r = 0; r < world; r++) {
        csf_engine *src = g[r];
        const size_t shard = (size_t)(src->d.n_pad / world);
        for (int p = 0; p < world; p++) {
            if (p == r) continue;
            // (one block of exchange records per peer, where a real run has one collective: csf_dev.h xbuf)
            if (!g[p]->xbuf.p || !src->xbuf.p) return fail(g[p], CSF_E_DEVICE, "no exchange buffer (allocation failed when the shard layout was set)");
            HIPCHK(g[p], hipMemcpyAsync(g[p]->xbuf.p + 2 * r * shard, src->xbuf.p + 2 * r * shard, 2 * shard * sizeof(float4),
                                        hipMemcpyDeviceToDevice, src->main));
            g[p]->xbuf_fresh = true;
        }
    }
    return CSF_OK;
}

// A handful of road users of one class (not the UncontrolledVehicle's; with csf_small_classes on: of any sets and classes) on one
// device, nothing sampled per tick and no history ring but
// csf_record's (the engine's rec_fast; the ring of csf_enable_history keeps the general path): the whole tick in one
// wave, all ticks of the call in one launch (csf_agent.hip: small_tick_kernel).  A pinned pair-kernel variant (the test suite's
// CSF_PAIR_VARIANT) keeps the general path.
static bool small_road_ok(const Dev &d) {   // no road, or a small one: staged in LDS, at most 256 vertices per lane and tick
    if (d.nv == 0) return true;
    int64_t P = 1;
    while (P < d.n) P <<= 1;
    return d.rg_nx == 0 && d.nv_pad <= SMALL_ROAD_MAX && d.nv_pad * P <= 256 * WAVE;
}

// A population of several parameter sets (any classes), or of the UncontrolledVehicle's class: small_tick_kernel does not take it.
static bool small_is_classes(const csf_engine *e) { return e->classes.size() > 1 || e->d.p.model == CSF_UNCONTROLLED; }

static bool small_fused_ok(const csf_engine *e) {
    const Dev &d = e->d;
    return e->knobs.fused_small != 0 && e->knobs.pair_variant < 0 && d.n >= 1 && d.n <= SMALL_MAX && d.n_live == d.n &&
           (!small_is_classes(e) || e->small_classes) && small_road_ok(d) &&
           e->world == 1 && !e->nccl && !e->loopback && e->knobs.fake_world <= 1 && (d.hist == nullptr || e->rec_fast) && e->profile <= 0 &&
           d.atrace == nullptr && d.lo == 0 && d.hi == d.n && e->pend.empty() && !e->dirty;
}

// ... and which of the two kernels a population that small_fused_ok admits takes: small_classes_kernel (csf_small_classes.hip; DESIGN.md
// 4.6e) with the switch of csf_small_classes on; a single set of a rider class keeps small_tick_kernel, switch or no switch.
static bool small_takes_classes(const csf_engine *e) { return e->small_classes && small_is_classes(e); }

// the bytes of the packed read-back (csf_get_tick: state rows, Fx, Fy, destination pointers, one-hot navigation state)
static size_t snap_need(const csf_engine *e) {
    return e->order.size() * ((size_t)(e->d.ns + 2) * sizeof(double) + sizeof(int32_t) + 3);
}

// ... and its mapped host buffer (csf_get_tick, csf_step_get_tick, csf_step_batch_get_tick), large enough for the population
static int snap_reserve(csf_engine *e) {
    HIPCHK(e, e->snap.reserve(snap_need(e), e->main, 4096));
    return CSF_OK;
}

// In front of a launch of one-wave ticks (small_fused_ok holds): the bands of the fp32 decisions (tracked_precise, side_undecided)
// and, for a read-back, its buffer.  *pack: the kernel may pack the read-back itself behind its last tick - slots are the
// population order and the buffer is there.
static int small_prelude(csf_engine *e, bool want_snap, bool *pack) {
    *pack = false;
    int rc = set_fov_band(e);
    if (rc || !want_snap) return rc;
    if ((rc = sync_order(e))) return rc;
    *pack = e->d.order == nullptr && snap_reserve(e) == CSF_OK;
    return CSF_OK;
}

// one launch takes at most 2^16 ticks: a second or less
static int small_launch_ticks(int64_t ticks_left) { return (int)std::min<int64_t>(ticks_left, 65536); }

// behind a launch of k one-wave ticks (batched: small_batch_kernel's, which also moved a recording member's tick word on)
static void small_ticked(csf_engine *e, int64_t k, bool batched) {
    e->mid_synced = false;
    e->d.tick += k;
    e->moves += k;
    e->small_ticks += k;
    if (!batched) return;
    e->batch_ticks += k;
    if (e->d.rec_tick != nullptr) e->rec_tick_dev = e->d.tick;
}

static int step_impl(csf_engine *e, int64_t n_ticks, bool want_snap, bool *snapped) {
    if (snapped) *snapped = false;
    if (!e) return CSF_E_ARG;
    if (n_ticks < 0) return fail(e, CSF_E_ARG, "n_ticks must be >= 0");
    if (int crc = calib_refuses(e, "csf_step")) return crc;
    HIPCHK(e, hipSetDevice(e->device));
    if (e->loopback) return fail(e, CSF_E_STATE, "members of a loopback group are stepped with csf_step_group");
    if (e->world > 1 && !e->nccl) return fail(e, CSF_E_STATE, "csf_comm_init must run before csf_step when world > 1");
    int rc = upload_all(e);
    if (rc) return rc;
    if (e->order.empty()) {  // intersection.py:888: nothing to do, time still advances
        e->d.tick += n_ticks;
        return CSF_OK;
    }
    if (n_ticks > 0 && !e->comm_calibrated && (rc = calibrate_comm_stream(e))) return rc;
    if (n_ticks > 0 && small_fused_ok(e)) {
        bool snap = false;                                     // csf_step_get_tick: the kernel packs the read-back
        if ((rc = small_prelude(e, want_snap, &snap))) return rc;
        for (int64_t t = 0; t < n_ticks;) {
            const int k = small_launch_ticks(n_ticks - t);
            Dev dd = e->d;
            dd.snap = (snap && t + k == n_ticks) ? (double *)e->snap.dev : nullptr;
            if (small_takes_classes(e)) launch_small_classes(dd, k, e->main);
            else launch_small_tick(dd, k, e->main);
            HIPCHK(e, hipGetLastError());
            small_ticked(e, k, false);
            t += k;
        }
        e->device_ahead = true;
        if (snapped) *snapped = snap;
        return CSF_OK;
    }
    for (int64_t t = 0; t < n_ticks; t++) {
        rc = enqueue_tick(e, n_ticks - t);
        if (rc) {
            // the streams meet on this way out too (every other entry point works on the main stream alone), best-effort: the
            // message of the first error stays, and a join that fails is tried again by the next csf_step
            if (e->chase_prev && hipEventRecord(e->ev_gather, e->comm) == hipSuccess && hipStreamWaitEvent(e->main, e->ev_gather, 0) == hipSuccess)
                e->chase_prev = false;
            (void)hipGetLastError();
            if (e->cal_phase >= 1 && e->cal_phase <= 3) e->cal_phase = 0;
            return rc;
        }
    }
    if ((rc = chase_join(e))) return rc;                          // (every other entry point works on the main stream alone)
    if (e->cal_phase >= 1 && e->cal_phase <= 3) e->cal_phase = 0;  // (a measurement does not span calls)
    if (n_ticks > 0) e->device_ahead = true;
    return CSF_OK;
}

int csf_step(csf_engine *e, int64_t n_ticks) try { return step_impl(e, n_ticks, false, nullptr); } catch (...) { return csf_caught(e); }

int csf_sync(csf_engine *e) try {
    if (!e) return CSF_E_ARG;
    if (e->knobs.debug_throw == 1) throw std::bad_alloc();
    if (e->knobs.debug_throw == 2) throw std::runtime_error("CSF_DEBUG_THROW=2");
    HIPCHK(e, hipSetDevice(e->device));
    {
        int rc = flush_pending(e);
        if (rc) return rc;
    }
    // (polling hipStreamQuery before sleeping in the runtime was tried again in round 5, with the group's stream lifetime put
    // right: no abort any more, and no gain - SocialForceIntersection.step() 37 / 54 us per tick at N = 3 / 1 024 against 32 / 48)
    HIPCHK(e, hipStreamSynchronize(e->main));
    HIPCHK(e, hipStreamSynchronize(e->comm));
    chase_cal_resolve(e, true);
    // did a wait of the side-by-side tick give up? (csf_dev.h: CHASE_SPIN_LIMIT - it never has.)  The kernels set a word of mapped host
    // memory: read here behind the streams' end, no copy (a 4-byte hipMemcpyAsync + wait per csf_sync was ~20 us of every timed call)
    if (e->chase_err.p && *(volatile unsigned *)e->chase_err.p != 0)
        return fail(e, CSF_E_DEVICE, "a wait of the per-agent kernel beside the pair launch gave up: the states since are not a simulation (CSF_CHASE=0 takes the two launches in turn)");
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_chase_ticks(const csf_engine *e, int64_t *n_ticks) try {
    if (!e || !n_ticks) return CSF_E_ARG;
    *n_ticks = e->chase_ticks;
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_chase_calibration(const csf_engine *e, int32_t *side_by_side, double us_per_tick[2]) try {
    if (!e) return CSF_E_ARG;
    if (side_by_side) *side_by_side = e->knobs.chase >= 2 ? 1 : e->knobs.chase == 0 ? -1 : e->chase_state;
    if (us_per_tick) us_per_tick[0] = e->chase_cal_us[0], us_per_tick[1] = e->chase_cal_us[1];
    return CSF_OK;
} catch (...) { return csf_caught(e); }
