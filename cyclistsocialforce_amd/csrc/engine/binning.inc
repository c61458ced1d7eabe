// engine/binning.inc - holes left by departures, the re-binning, bounding circles around a pair launch.
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

// ---- holes (csf_engine::HoleIndex) -----------------------------------------------------------------------------------
// after a re-binning: ask for the places and the circles (two copies and an event behind the re-binning's launches)
static int holes_request(csf_engine *e) {
    csf_engine::HoleIndex &h = e->holes;
    const Dev &d = e->d;
    h.ready = h.pending = false;
    for (auto &c : h.cell_tab) c.n = 0;
    if (!e->knobs.hole_reuse || !e->tail_tracked || !d.classify || d.n_pad <= 0) return CSF_OK;
    // Only where road users come and go: a population that saw no arrival or departure since the last re-binning is not asked for
    // its places and circles (two copies to the host and what surrounds them: ~25 us of every re-binning of a static crowd).  The
    // first period of traffic then has no lattice - its arrivals take places of the tail, as they did before round 5 - and the
    // re-binning that ends it asks.
    const bool traffic = e->pop_calls_in_period;
    e->pop_calls_in_period = false;
    if (!traffic && e->knobs.hole_lazy) return CSF_OK;
    const size_t np = (size_t)d.n_pad, nb = np / 64;
    if (h.pos.n < np) HIPCHK(e, h.pos.alloc(np));     // (the last read-back has landed, or nobody will look at it: no wait)
    if (h.bnd.n < nb) HIPCHK(e, h.bnd.alloc(nb));
    if (!h.ev) HIPCHK(e, hipEventCreateWithFlags(&h.ev, hipEventDisableTiming));
    // (a KERNEL writes them into mapped host memory: two hipMemcpyAsync to the host in the middle of a run cost the tick loop far more
    // than their 7 us on the device - 2.6 us per tick at the headline with a re-binning every 64 ticks, profiles/r6_hole_readback_ab.txt)
    if (e->knobs.hole_export_kernel) {
        launch_export_places(d, h.pos.dev, h.bnd.dev, (int64_t)np, (int64_t)nb, e->main);
        HIPCHK(e, hipGetLastError());
    } else {
        HIPCHK(e, hipMemcpyAsync(h.pos.p, d.pos, np * sizeof(int32_t), hipMemcpyDeviceToHost, e->main));
        HIPCHK(e, hipMemcpyAsync(h.bnd.p, d.bnd, nb * sizeof(float4), hipMemcpyDeviceToHost, e->main));
    }
    HIPCHK(e, hipEventRecord(h.ev, e->main));
    h.places = (e->live_at_rebin + 63) / 64 * 64;
    h.ox = d.ox, h.oy = d.oy;
    h.pending = true;
    return CSF_OK;
}

// the lattice, once the read-back has landed (the first population call after a re-binning waits for it, if at all)
static bool holes_ready(csf_engine *e) {
    csf_engine::HoleIndex &h = e->holes;
    if (h.ready) return true;
    if (!h.pending) return false;
    if (hipEventSynchronize(h.ev) != hipSuccess) return h.pending = false;
    h.pending = false;
    const int64_t nb = h.places / 64;
    h.hpos.assign(h.pos.p, h.pos.p + h.pos.n);
    h.hbnd.assign(h.bnd.p, h.bnd.p + h.bnd.n);
    std::vector<float> radii;
    double x0 = 1e300, x1 = -1e300, y0 = 1e300, y1 = -1e300;
    for (int64_t b = 0; b < nb; b++) {
        const float4 c = h.hbnd[(size_t)b];
        if (!(c.z < 1e6f) || !std::isfinite(c.x) || !std::isfinite(c.y)) continue;       // (a batch of sentinels)
        radii.push_back(c.z);
        x0 = std::min(x0, (double)c.x), x1 = std::max(x1, (double)c.x), y0 = std::min(y0, (double)c.y), y1 = std::max(y1, (double)c.y);
    }
    if (radii.size() < 4) return false;
    std::nth_element(radii.begin(), radii.begin() + radii.size() / 2, radii.end());
    const double reach = e->knobs.hole_dist * (double)radii[radii.size() / 2];
    if (!(reach > 0.0)) return false;
    h.reach2 = reach * reach;
    h.cell = reach;
    h.x0 = x0 - reach, h.y0 = y0 - reach;
    h.nx = (int)std::min(512.0, std::ceil((x1 - x0 + 2 * reach) / h.cell) + 1);
    h.ny = (int)std::min(512.0, std::ceil((y1 - y0 + 2 * reach) / h.cell) + 1);
    h.cell = std::max({h.cell, (x1 - x0 + 2 * reach) / (h.nx - 1), (y1 - y0 + 2 * reach) / (h.ny - 1)});
    h.inv_cell = 1.0 / h.cell;
    h.cell_tab.assign((size_t)h.nx * (size_t)h.ny, csf_engine::HoleIndex::Cell{});
    return h.ready = true;
}

// a road user has left slot a: if the slot had a place in a real batch, its hole can be found by the batch's centre
static void holes_add(csf_engine *e, int32_t a) {
    csf_engine::HoleIndex &h = e->holes;
    if (!holes_ready(e) || (size_t)a >= h.hpos.size()) return;
    const int64_t place = h.hpos[(size_t)a];
    if (place < 0 || place >= h.places) return;                    // (it arrived after the re-binning: a place of the tail)
    const float4 c = h.hbnd[(size_t)(place >> 6)];
    if (!(c.z < 1e6f)) return;
    const int ix = (int)(((double)c.x - h.x0) * h.inv_cell), iy = (int)(((double)c.y - h.y0) * h.inv_cell);
    if (ix < 0 || iy < 0 || ix >= h.nx || iy >= h.ny) return;
    csf_engine::HoleIndex::Cell &cl = h.cell_tab[(size_t)iy * h.nx + ix];
    if (cl.n >= csf_engine::HoleIndex::CELL_CAP) return;          // (a crowded cell: this one is found by the re-binning only)
    cl.e[cl.n++] = {a, c.x, c.y};
}

// the hole nearest to (x, y) whose batch's centre is within reach; -1: none
static int32_t holes_take(csf_engine *e, double x, double y) {
    csf_engine::HoleIndex &h = e->holes;
    if (!h.ready || e->free_recent.empty() || !std::isfinite(x) || !std::isfinite(y)) return -1;
    const float sx = (float)(x - h.ox), sy = (float)(y - h.oy);    // scene coordinates, as the circles
    const int ix = (int)std::floor(((double)sx - h.x0) * h.inv_cell), iy = (int)std::floor(((double)sy - h.y0) * h.inv_cell);
    const int jx0 = std::max(0, ix - 1), jx1 = std::min(h.nx - 1, ix + 1), jy0 = std::max(0, iy - 1), jy1 = std::min(h.ny - 1, iy + 1);
    for (;;) {
        float best = (float)h.reach2;
        csf_engine::HoleIndex::Cell *bc = nullptr;
        int bi = -1;
        auto look = [&](csf_engine::HoleIndex::Cell &cl) {
            for (int i = 0; i < cl.n; i++) {
                const float dx = cl.e[i].x - sx, dy = cl.e[i].y - sy, d2 = dx * dx + dy * dy;
                if (d2 < best) best = d2, bc = &cl, bi = i;
            }
        };
        // its own cell first: a hole within reach there is as good as any (its batch's circle holds the arrival, or nearly)
        if (ix >= 0 && iy >= 0 && ix < h.nx && iy < h.ny) look(h.cell_tab[(size_t)iy * h.nx + ix]);
        if (bi < 0)                                                // (nobody there: the eight cells around)
            for (int jy = jy0; jy <= jy1; jy++)
                for (int jx = jx0; jx <= jx1; jx++)
                    if (jx != ix || jy != iy) look(h.cell_tab[(size_t)jy * h.nx + jx]);
        if (bi < 0) return -1;
        const int32_t a = bc->e[bi].slot;
        bc->e[bi] = bc->e[--bc->n];
        const int32_t at = e->sidx[(size_t)a].recent;
        if (at < 0) continue;                                      // (handed out some other way since: look again)
        const int32_t last = e->free_recent.back();                // out of free_recent as well
        e->free_recent[(size_t)at] = last;
        e->sidx[(size_t)last].recent = at;
        e->free_recent.pop_back();
        e->sidx[(size_t)a].recent = -1;
        h.taken++;
        return a;
    }
}

// (re)build the spatially binned order of the records; decides whether batches are classified this tick
int rebin(csf_engine *e) {
    Dev &d = e->d;
    e->mid_synced = false;     // (records re-expressed, perhaps a new sentinel tail: csf_mid.hip's other halves are stale)
    if (e->world <= 1 && !e->loopback && d.n_pad < e->cap && d.n + TAIL_SLOTS / 2 > d.n_pad) {   // fresh slots are running out
        set_shard(e);
        launch_records(d, e->main);     // sentinels in the new tail (the records of the road users are rewritten as they are)
    }
    d.pair_variant = pair_variant_for(e, d.n_live);
    // Several parameter sets: up to 16 of them get the class-segmented order (a rank of a sharded run too: the order is one of
    // the SOURCES, which every rank holds in full, and the same on every rank) - the set leads the
    // sort key, every set becomes a run of places that starts at a multiple of 64, and the pair term is one launch of the
    // culling kernel per run with that set's constants, far-field radius and field (launch_pair_all).  Otherwise the
    // plain kernel looks every source's set up (csf_pair.hip: HET).
    e->segs.clear();
    e->h_segtab.clear();
    e->seg_total_by = 0;
    d.seg_keys = 0;
    d.src_beg = 0;
    d.part_base = 0;
    // It pays from ~2 048 road users per set (a launch per set has its own start-up): four sets at N = 16 384 199 us per
    // tick against 387 us, at 8 192 104 against 119, at 4 096 68 against 41 (tools/hetero_rate.py; CSF_SEGMENTS=1 forces
    // it from 1 024 road users, 0 switches it off).
    const int seg_env = e->knobs.segments;
    bool seg = d.n_classes > 1 && d.n_classes <= 16 && d.pair_variant == 0 && d.n >= BIN_MIN_AGENTS &&
               e->class_kappa.size() == e->classes.size() &&
               (seg_env >= 0 ? seg_env != 0 : d.n_live >= 2048 * (int64_t)d.n_classes);
    SegTable tab{};
    if (seg) {
        std::vector<int64_t> count((size_t)d.n_classes, 0);
        for (int32_t a : e->order) count[e->h_cls[(size_t)a]]++;
        int64_t sorted = 0, place = 0, units_total = 0;
        tab.n = d.n_classes;
        tab.sent_slot = e->sent_slot;
        for (int c = 0; c < d.n_classes; c++) {
            tab.sorted_beg[c] = sorted;
            tab.place_beg[c] = place;
            sorted += count[(size_t)c];
            place += (count[(size_t)c] + 63) / 64 * 64;
        }
        tab.sorted_beg[d.n_classes] = sorted;
        units_total = place / 64;
        if (place > d.n_pad || sorted != d.n_live) seg = false;      // (no room for the padding: the plain kernel)
        if (seg) {
            const int64_t per_min = std::max<int64_t>(d.wide ? 32 : 16, (units_total + (MAX_SPLIT - d.n_classes) - 1) / std::max(1, MAX_SPLIT - d.n_classes));
            int32_t slots = 0;
            for (int c = 0; c < d.n_classes; c++) {
                const int64_t units = (count[(size_t)c] + 63) / 64;
                PairConsts pc;
                derive_pair_consts(e->classes[(size_t)c], pc, e->knobs.rnear);
                pc.p2r = d.pc.p2r;
                set_far_consts(e->knobs, e->classes[(size_t)c], e->class_kappa[(size_t)c], d.n, pc);
                if (units == 0 || pc.f0_zero) continue;              // nobody of this set, or a set whose field is zero
                const int64_t chunks = (units + per_min - 1) / per_min;
                csf_engine::Segment sg;
                sg.cls = c;
                sg.beg = tab.place_beg[c];
                sg.end = sg.beg + units * 64;
                sg.chunk_units = (int32_t)((units + chunks - 1) / chunks);
                sg.n_split = (int32_t)((units + sg.chunk_units - 1) / sg.chunk_units);
                sg.part_base = slots;
                sg.pc = pc;
                slots += sg.n_split;
                e->segs.push_back(sg);
            }
            if (slots > MAX_SPLIT) seg = false, e->segs.clear();
            else {
                d.seg_keys = 1;
                d.n_split = std::max(1, slots);                       // what the per-agent kernel sums
                d.n_src = place;
            }
            // the runs whose field is the TwoD one, as the segmented grid reads them
            e->h_segtab.clear();
            e->seg_total_by = 0;
            for (const csf_engine::Segment &sg : e->segs) {
                if (e->classes[(size_t)sg.cls].model == CSF_BICYCLE) continue;
                SegDev t{};
                t.pc = sg.pc;
                t.hfov = e->classes[(size_t)sg.cls].hfov;
                t.src_beg = sg.beg;
                t.n_src = sg.end;
                t.chunk_units = sg.chunk_units;
                t.n_split = sg.n_split;
                t.part_base = sg.part_base;
                t.first_by = e->seg_total_by;
                e->seg_total_by += sg.n_split;
                e->h_segtab.push_back(t);
            }
            bool same_reach = true;
            for (const SegDev &t : e->h_segtab) same_reach = same_reach && t.pc.reach != 0;
            if (e->h_segtab.size() < 2 || !same_reach || e->h_segtab.size() > 16) e->seg_total_by = 0;   // (one run: nothing to merge)
            else {
                HIPCHK(e, e->segtab.reserve(16));
                HIPCHK(e, hipMemcpyAsync(e->segtab.p, e->h_segtab.data(), e->h_segtab.size() * sizeof(SegDev), hipMemcpyHostToDevice, e->main));
            }
        }
    }
    const bool binned = d.pair_variant == 0 && d.n >= BIN_MIN_AGENTS && (d.n_classes == 1 || seg);
    d.classify = binned;
    update_far_radius(e);
    const bool track = binned && !seg && e->world <= 1 && !e->loopback;
    // (a mid-size member of a batch on the plain order: the batch runs the two launches for all members that are due - abi_batch.inc)
    const bool defer = e->mid_defer && !seg && !binned;
    if (defer) e->mid_deferred |= MID_DUE_REBIN;
    if (seg) {
        Dev ds = d;
        ds.perm = e->rlist.p;                                        // the sorted slots, before the runs are moved apart
        int rc = launch_rebin(ds, e->sort_keys.p, e->sort_keys_out.p, e->sort_vals.p, e->sort_tmp.p, e->sort_tmp.n, e->main);
        if (rc != 0) return fail(e, CSF_E_DEVICE, "radix sort of the record bins failed (%d)", rc);
        launch_segment_perm(d, e->rlist.p, tab, e->main);
    } else if (binned) {
        int rc = launch_rebin(d, e->sort_keys.p, e->sort_keys_out.p, e->sort_vals.p, e->sort_tmp.p, e->sort_tmp.n, e->main);
        if (rc != 0) return fail(e, CSF_E_DEVICE, "radix sort of the record bins failed (%d)", rc);
    } else if (!defer) {
        launch_identity_perm(d, e->main);
    }
    // Every precise record gets a new origin - where the road user is now - and is re-expressed relative to it; pos[],
    // the binned copy of the records in scene coordinates and the circles (csf_bin.hip: rebase_kernel).  The binned
    // copy is maintained by the agent kernel where every record is local, rebuilt from the gathered records before every
    // pair launch of a sharded run (enqueue_tick).
    d.recs_valid = binned;
    d.rebase_from_state = e->state_all_current;
    if (!defer) launch_rebase(d, e->main);
    {   // receivers in binned order + far-tile skipping, where there are enough tiles for it to pay.  A rank that owns
        // an index block [lo, hi) takes ITS receivers in binned order: their positions, sorted
        const int ov = e->knobs.recv_binned;
        const bool whole = d.lo == 0 && d.hi == d.n;
        d.recv_binned = binned && d.recs_valid && std::isfinite(d.pc.rfar) && (ov >= 0 ? ov != 0 : d.n_pad >= 65536);
        d.rlist = nullptr;
        if (d.recv_binned && !whole) {
            int rc = launch_receiver_list(d, e->sort_keys.p, e->rlist.p, e->sort_tmp.p, e->sort_tmp.n, e->main);
            if (rc != 0) return fail(e, CSF_E_DEVICE, "radix sort of the receiver positions failed (%d)", rc);
            d.rlist = e->rlist.p;
        }
    }
    // Where the sentinels went: the sort is stable and their key is the largest, so the road users fill the places
    // [0, n_live) and the free slots follow in ascending slot order.  Handing the free slots out in that order
    // (csf_add_agents) keeps the places that can hold a road user a prefix of the order, and the pair kernel's source
    // chunks end there (d.n_src) instead of at n_pad.  Slots retired since the last re-binning are sentinels from now on.
    e->tail_tracked = track;
    for (int32_t a : e->free_recent) e->sidx[(size_t)a].recent = -1;   // (every hole goes to the tail: the order has none)
    e->free_tail.insert(e->free_tail.end(), e->free_recent.begin(), e->free_recent.end());
    e->free_recent.clear();
    std::sort(e->free_tail.begin(), e->free_tail.end(), std::greater<int32_t>());
    e->live_at_rebin = d.n_live;
    e->tail_used = 0;
    e->tail_flushed = 0;
    if (!seg) {
        const int64_t n_src = e->tail_tracked ? std::max<int64_t>(64, (e->live_at_rebin + 63) / 64 * 64)
                              : (e->world <= 1 && !e->loopback && !binned ? std::max<int64_t>(64, (d.n + 63) / 64 * 64) : d.n_pad);
        d.n_src = std::min(n_src, d.n_pad);
        set_chunks(e);                                               // (also after a segmented period: n_split was the segments')
    }
    d.clist = nullptr;
    d.ccount = nullptr;
    if (d.recv_binned && e->knobs.clist != 0) {   // which tiles can matter to which receiver group until the next re-binning
        const PairShape sh = pair_shape(d);           // (the instance that reads the lists checks both words against its own)
        d.clist_tile = sh.tile();
        d.clist_rpb = sh.rpb;
        const int64_t nloc = d.hi - d.lo, groups = (nloc + sh.rpb - 1) / sh.rpb;
        const int64_t ntiles = (d.n_src + d.clist_tile - 1) / d.clist_tile;
        if (groups > 0 && ntiles > 0 && ntiles < 65536) {
            HIPCHK(e, e->tcirc.reserve((size_t)ntiles + 1));
            HIPCHK(e, e->clist.reserve((size_t)groups * CLIST_MAX));
            HIPCHK(e, e->ccount.reserve((size_t)groups));
            // tiles that hold road users as of now are listed; the tile the population ends in and the sentinel tail behind it
            // (where arrivals appear) are always visited
            d.ctail = (int32_t)(e->tail_tracked ? e->live_at_rebin / d.clist_tile : ntiles);
            // both sides move until the lists are rebuilt (REBIN_TICKS ticks; a churn-triggered re-binning comes sooner)
            const float move = (float)(e->knobs.rebin_ticks + 2) * d.bnd_margin + 5e-3f;   // what either side can move until then
            const float reach = d.pc.rfar + 2.0f * move;
            // The far-field bound from the tiles within reach (large populations): R = ln(n / eps) / kappa prices every one of
            // the n sources at the cut - a million road users pay for a radius that holds a few ten thousand.  With the lists
            // in hand: a receiver meets at most m sources (the places of its group's listed tiles and of the tiles always
            // visited), and every source of a tile it does not list is at least the circles' separation away and adds at
            // most f_0 exp(-kappa separation) - `tail` in all.  Leaving out the pairs with rho q / sigma > T among the m
            // omits at most m exp(-T) f_0 more: T = ln(m / (eps - tail)) keeps the total below eps f_0, the same promise
            // (include/csf.h: csf_far_radius) at a smaller radius.  m and tail are maxima over the groups of this device,
            // measured at every re-binning; one read-back of two words, where a tick takes milliseconds.
            const bool tighten = e->knobs.far_tight != 0 && d.pc.reach && e->classes.size() == 1 && e->far_kappa > 0;
            if (tighten) {
                HIPCHK(e, e->far_stat.reserve(2));
                HIPCHK(e, hipMemsetAsync(e->far_stat.p, 0, 2 * sizeof(unsigned), e->main));
            }
            launch_candidate_lists(d, e->tcirc.p, e->clist.p, e->ccount.p, reach, e->main, tighten ? e->far_stat.p : nullptr, (float)e->far_kappa, move);
            d.clist = e->clist.p;
            d.ccount = e->ccount.p;
            if (tighten) {
                // (into the pinned buffer csf_create made for the coordinate bound - cap >= 64 doubles; the stream is waited for
                // right below, so the two uses cannot meet: a runtime's first copy into PAGEABLE memory cost 9 ms in mid-run)
                unsigned st[2] = {0u, 0u};
                HIPCHK(e, hipMemcpyAsync(e->bound_pin.p, e->far_stat.p, sizeof st, hipMemcpyDeviceToHost, e->main));
                HIPCHK(e, hipStreamSynchronize(e->main));
                std::memcpy(st, e->bound_pin.p, sizeof st);
                float tail;
                std::memcpy(&tail, &st[1], sizeof tail);
                const double eps = e->knobs.far_eps, met = std::min<double>((double)st[0], (double)d.n) + (double)TAIL_SLOTS;   // (+ arrivals until then)
                e->far_met = met;
                e->far_tail = tail;
                if (st[0] > 0 && std::isfinite(tail) && tail < 0.5 * eps) {
                    const double T = std::log(met / (eps - (double)tail)), T0 = std::log((double)d.n / eps);
                    if (T < T0) {                                    // (the lists were built for the larger radius: still complete)
                        set_far_consts_T(d.p, e->far_kappa, T, d.pc);
                        e->far_T = T;
                    }
                }
            }
        }
    }
    // set_fov_band bounds the coordinates by "where they were at the last upload + a speed clamp's worth per step since": over
    // 1e5 ticks that bound - and with it every rounding band - grows far beyond the scene.  Measure again now and then
    // (one read-back of the positions; where every slot's state is on this device).
    if (e->moves >= 4096 && e->world <= 1 && !e->loopback) e->bound_stale = true;
    e->ticks_since_rebin = 0;
    e->wgo.forget();            // (new tiles: what a group cost against the old ones says little)
    e->moved_unbinned = 0;
    e->churn = 0;
    e->bounds_fresh = true;                                          // (rebase_kernel wrote the circles of the records as they are)
    return holes_request(e);                                         // (places and circles of this order, for arrivals that take a leaver's slot)
}

// bounding circles for the pair launch that follows; afterwards the circles emitted by that launch become current
int bounds_before_pair(csf_engine *e) {
    Dev &d = e->d;
    // Road users that arrived since the last re-binning sit in the tail batches of the binned order, among each other
    // and far from sorted: every receiver tests those batches lane by lane (measured ~1.3 us per batch and tick at
    // N = 16 384), against ~35 us for the kernels of a re-binning.  With r arrivals per tick the cheapest period is about
    // sqrt(2 * 35 * 64 / (1.3 r)) ticks, i.e. re-bin when ticks x arrivals since the last one reaches ~3500; 3000 to 6000
    // measured alike (profiles/r2_churn_rate.txt; CSF_REBIN_CHURN overrides the constant).
    const int64_t churn_k = e->knobs.rebin_churn;
    const bool rebin_now = e->ticks_since_rebin + e->moved_unbinned >= e->knobs.rebin_ticks || e->ticks_since_rebin * e->churn >= churn_k;
    // Exchange records that arrived behind the last tick (a rank of a sharded run): spread to rec / reclo / rec2 by the copy into
    // binned order that follows the circles - unless this call re-bins (the re-binning reads the records) or no such copy will
    // run (records not binned; the first tick of a binned order, whose copy the re-binning made itself)
    if (e->xbuf_fresh && (rebin_now || !d.recs_valid || e->ticks_since_rebin < 1)) {
        launch_unpack_exchange(d, e->main);
        e->xbuf_fresh = false;
    }
    if (rebin_now) {
        int rc = rebin(e);
        if (rc) return rc;
    }
    if (d.classify && !e->bounds_fresh) launch_bounds(d, e->main);
    e->ticks_since_rebin++;
    e->pair_since_move = true;
    return CSF_OK;
}

void bounds_after_pair(csf_engine *e, bool records_will_move_one_tick) {
    Dev &d = e->d;
    if (!d.classify || d.n_live <= 1) {
        e->bounds_fresh = false;
        return;
    }
    std::swap(d.bnd, d.bnd_next);                   // the launch wrote the next tick's circles
    e->bounds_fresh = records_will_move_one_tick;   // valid only if exactly one integrate follows
}
