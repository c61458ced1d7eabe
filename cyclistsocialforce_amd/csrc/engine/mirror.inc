// engine/mirror.inc - host mirror <-> device: download, compaction, queue slab, parameter table, upload.
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

int flush_pending(csf_engine *e);   // collected population changes -> the device (defined with the population entry points)

// device -> host mirror (needed before a structural change once ticks have run)
int download_all(csf_engine *e) {
    int frc = flush_pending(e);
    if (frc) return frc;
    if (!e->device_ahead) return CSF_OK;
    HIPCHK(e, hipStreamSynchronize(e->main));
    if (e->comm) HIPCHK(e, hipStreamSynchronize(e->comm));
#define D2H(vec, buf) HIPCHK(e, hipMemcpy(vec.data(), buf.p, vec.size() * sizeof(vec[0]), hipMemcpyDeviceToHost))
    D2H(e->h_s, e->s);
    D2H(e->h_znp, e->znp);
    D2H(e->h_hx, e->hx);
    D2H(e->h_hy, e->hy);
    D2H(e->h_lti, e->lti);
    D2H(e->h_ppsi, e->ppsi);
    D2H(e->h_F, e->F);
    D2H(e->h_ptr, e->ptr);
    D2H(e->h_ti, e->ti);
    D2H(e->h_dgood, e->dgood);
    D2H(e->h_znav, e->znav);
    D2H(e->h_zrid, e->zrid);
    D2H(e->h_status, e->status);
#undef D2H
    e->device_ahead = false;
    return CSF_OK;
}

// slots -> population order on the host mirror (a full upload starts from a population without holes)
void compact_host(csf_engine *e) {
    const int64_t n = (int64_t)e->order.size(), cap = e->cap, hl = e->d.hist_len;
    bool identity = e->free_tail.empty() && e->free_recent.empty() && n == e->d.n;
    for (int64_t i = 0; identity && i < n; i++) identity = e->order[(size_t)i] == i;
    if (!identity) {
        auto gather = [&](auto &vec, int64_t comps) {
            auto old = vec;
            for (int64_t c = 0; c < comps; c++)
                for (int64_t i = 0; i < n; i++) vec[(size_t)(c * cap + i)] = old[(size_t)(c * cap + e->order[(size_t)i])];
        };
        gather(e->h_s, STATE_ROWS); gather(e->h_F, 6); gather(e->h_znp, 3); gather(e->h_lti, 5);
        gather(e->h_hx, hl); gather(e->h_hy, hl);
        gather(e->h_vdes, 1); gather(e->h_ppsi, 1); gather(e->h_ptr, 1); gather(e->h_ti, 1); gather(e->h_dgood, 1);
        gather(e->h_znav, 1); gather(e->h_zrid, 1); gather(e->h_status, 1); gather(e->h_cls, 1);
        std::vector<std::vector<double>> q((size_t)cap), sc((size_t)cap);
        for (int64_t i = 0; i < n; i++) q[(size_t)i] = std::move(e->h_q[(size_t)e->order[(size_t)i]]);
        for (int64_t i = 0; i < n; i++) sc[(size_t)i] = std::move(e->h_script[(size_t)e->order[(size_t)i]]);
        e->h_q.swap(q);
        e->h_script.swap(sc);
        for (int64_t i = 0; i < n; i++) e->order[(size_t)i] = (int32_t)i;
        e->free_tail.clear();
        e->free_recent.clear();
        for (csf_engine::SlotIdx &x : e->sidx) x.recent = -1;
    }
    std::fill(e->h_alive.begin(), e->h_alive.end(), (uint8_t)0);
    std::fill(e->h_alive.begin(), e->h_alive.begin() + n, (uint8_t)1);
    std::fill(e->h_cls.begin() + n, e->h_cls.end(), (uint8_t)0);
    e->d.n = n;
    e->d.n_live = n;
    e->order_dirty = true;
}

// destination queues of the live slots -> one slab of rows, every queue contiguous, with room behind them for the queues
// of road users that arrive and for queues that are replaced (those are appended, flush_pending), `extra` rows at least
int upload_queues(csf_engine *e, int64_t extra) {
    Dev &d = e->d;
    std::vector<int64_t> beg((size_t)e->cap, 0);
    std::vector<int32_t> len((size_t)e->cap, 0);
    int64_t rows = 0;
    for (int64_t a = 0; a < d.n; a++) {
        if (!e->h_alive[(size_t)a]) continue;
        beg[(size_t)a] = rows;
        len[(size_t)a] = (int32_t)(e->h_q[(size_t)a].size() / 3);
        rows += len[(size_t)a];
    }
    if ((size_t)(3 * (rows + extra)) > e->q.n || e->q.n == 0) {
        size_t want = (size_t)std::max<int64_t>(3 * (rows + extra) * 2, 3 * 4096);
        HIPCHK(e, e->q.alloc(want));
    }
    // A slab that is rewritten often (compact_slab: arrivals and new routes every tick - each such rewrite waits for the ticks in
    // flight and uploads every live queue, ~1 ms at N = 16 384, and at 5 % of the population replaced per tick it came every 17
    // ticks: 59 us per tick, most of the host's time in csf_set_dest_queue) grows to eight times what is alive: a rewrite every
    // ~140 such ticks.  (Up to 96 MB; beyond, twice the live rows as before.)
    if (e->slab_rewrites >= 2 && (size_t)(3 * (rows + extra)) * 8 > e->q.n && (size_t)(3 * (rows + extra)) * 8 * sizeof(double) <= (96u << 20))
        HIPCHK(e, e->q.alloc((size_t)(3 * (rows + extra)) * 8));
    d.q = e->q.p;
    d.qcap = (int64_t)(e->q.n / 3);
    e->q_top = rows;
    std::vector<double> flat((size_t)(3 * rows), 0.0);
    for (int64_t a = 0; a < d.n; a++) {
        if (!e->h_alive[(size_t)a]) continue;
        const std::vector<double> &qa = e->h_q[(size_t)a];
        std::copy(qa.begin(), qa.end(), flat.begin() + 3 * beg[(size_t)a]);
    }
    if (!flat.empty()) HIPCHK(e, hipMemcpy(e->q.p, flat.data(), flat.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(e->qbeg.p, beg.data(), beg.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(e->qlen.p, len.data(), len.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return CSF_OK;
}

// The slab is full of queues that were replaced or whose road users left: write the live queues afresh (the host holds
// every queue as it was last set; the pointers into them live on the device and stay as they are).
int compact_slab(csf_engine *e, int64_t extra) {
    e->slab_rewrites++;
    int rc = flush_pending(e);
    if (rc) return rc;
    HIPCHK(e, hipStreamSynchronize(e->main));                  // ticks in flight read the old slab
    return upload_queues(e, extra);
}

// the table of parameter sets, what the kernels derive from each row, and the row of every slot
int upload_classes(csf_engine *e) {
    Dev &d = e->d;
    const size_t K = e->classes.size();
    if (e->ptab.n < K) {
        HIPCHK(e, e->ptab.alloc(K));
        HIPCHK(e, e->pctab.alloc(K));
        HIPCHK(e, e->pbtab.alloc(7 * K));
    }
    std::vector<PairConsts> pc(K);
    std::vector<double> pb(7 * K, 0.0);
    e->class_kappa.assign(K, 0.0);
    for (size_t c = 0; c < K; c++) {
        derive_pair_consts(e->classes[c], pc[c], e->knobs.rnear);
        if (K > 1 && K <= 16) e->class_kappa[c] = far_kappa(e->classes[c]);   // (for the launches per set: rebin)
        pc[c].p2r = d.pc.p2r;                                    // (the rule belongs to the intersection: intersection.py:324)
        if (e->classes[c].model == CSF_PLANARBIKE) derive_planarbike(e->classes[c], &pb[7 * c]);
    }
    HIPCHK(e, hipStreamSynchronize(e->main));                  // ticks in flight read the old rows
    HIPCHK(e, hipMemcpy(e->ptab.p, e->classes.data(), K * sizeof(csf_params), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(e->pctab.p, pc.data(), K * sizeof(PairConsts), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(e->pbtab.p, pb.data(), pb.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(e->cls.p, e->h_cls.data(), e->h_cls.size(), hipMemcpyHostToDevice));
    d.ptab = e->ptab.p;
    d.pctab = e->pctab.p;
    d.pbtab = e->pbtab.p;
    d.cls = e->cls.p;
    d.n_classes = (int32_t)K;
    e->classes_dirty = false;
    return CSF_OK;
}

// Dev::road_np of a road [nv] rows (x, y, F0, sigma): one integer sigma for every edge gives r^-(sigma+1) as a power of rsq(r^2)
static int32_t road_np_of(const double *road, int64_t nv) {
    if (nv <= 0) return 0;
    const double sg = road[3];
    bool same = sg == std::floor(sg) && sg >= 1 && sg <= 5;
    for (int64_t k = 1; same && k < nv; k++) same = road[4 * k + 3] == sg;
    return same ? (int32_t)sg + 1 : 0;
}

// Road vertices (x, y, -F0, -(sigma+1)/2), padded with inert vertices.  Positions are offsets from the origin of
// their tile of 1024 consecutive vertices (the centre of its box, rounded to 1/4 m): consecutive vertices of a
// polyline are neighbours, so a vertex resolves to 2^-24 of ~50 m whatever the extent of the scene, and the road
// kernel forms receiver - vertex relative to the tile (csf_pair.hip: road_kernel).
// road: [nv] rows (x, y, F0, sigma); (ox, oy) the origin of the scene.  Fills rv [nv padded to 64] and rvo [tiles] and returns
// Dev::road_np.  Shared by upload_all and the scene roads of csf_scene_calib_road (engine/abi_scene.inc): a view's road is packed
// as the road of a stand-alone engine that holds the scene.
static int32_t pack_road(const double *road, int64_t nv, double ox, double oy, std::vector<float4> &rv, std::vector<float2> &rvo) {
    const int64_t nv_pad = (nv + 63) / 64 * 64;
    rv.clear(), rvo.clear();
    if (nv > 0) {
        const int64_t tiles = (nv_pad + 1023) / 1024;
        rv.assign((size_t)nv_pad, make_float4(1e15f, 1e15f, 0.f, -1.f));
        rvo.assign((size_t)tiles, make_float2(0.f, 0.f));
        for (int64_t t = 0; t < tiles; t++) {
            const int64_t k0 = t * 1024, k1 = std::min<int64_t>(nv, k0 + 1024);
            double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
            for (int64_t k = k0; k < k1; k++) {
                x0 = std::min(x0, road[4 * k]), x1 = std::max(x1, road[4 * k]);
                y0 = std::min(y0, road[4 * k + 1]), y1 = std::max(y1, road[4 * k + 1]);
            }
            if (!(k1 > k0)) continue;
            const double tx = 0.25 * std::nearbyint(4.0 * (0.5 * (x0 + x1) - ox)), ty = 0.25 * std::nearbyint(4.0 * (0.5 * (y0 + y1) - oy));
            rvo[(size_t)t] = make_float2((float)tx, (float)ty);
            for (int64_t k = k0; k < k1; k++)
                rv[(size_t)k] = make_float4((float)((road[4 * k] - ox) - tx), (float)((road[4 * k + 1] - oy) - ty),
                                            (float)(-road[4 * k + 2]), (float)(-0.5 * (road[4 * k + 3] + 1.0)));
        }
    }
    return road_np_of(road, nv);
}

int upload_all(csf_engine *e) {
    if (e->classes_dirty) {
        int rc = upload_classes(e);
        if (rc) return rc;
    }
    if (!e->dirty) return flush_pending(e);
    Dev &d = e->d;
    e->mid_synced = false;
    compact_host(e);
    if (e->classes.size() > 1) HIPCHK(e, hipMemcpy(e->cls.p, e->h_cls.data(), e->h_cls.size(), hipMemcpyHostToDevice));   // (slots moved)
    const int64_t n = d.n;
    int qrc = upload_queues(e, 0);
    if (qrc) return qrc;
    {   // the prescribed trajectories of UncontrolledVehicle road users (vehicle.py:958-960): one slab of rows
        std::vector<int64_t> beg((size_t)e->cap, 0);
        std::vector<int32_t> len((size_t)e->cap, 0);
        std::vector<double> flat;
        for (int64_t a = 0; a < n; a++) {
            beg[(size_t)a] = (int64_t)(flat.size() / 4);
            len[(size_t)a] = (int32_t)(e->h_script[(size_t)a].size() / 4);
            flat.insert(flat.end(), e->h_script[(size_t)a].begin(), e->h_script[(size_t)a].end());
        }
        if (flat.size() > e->script.n) HIPCHK(e, e->script.alloc(flat.size()));
        if (!flat.empty()) HIPCHK(e, hipMemcpy(e->script.p, flat.data(), flat.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(e, hipMemcpy(e->sbeg.p, beg.data(), beg.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        HIPCHK(e, hipMemcpy(e->slen.p, len.data(), len.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        d.script = e->script.p;
        d.sbeg = e->sbeg.p;
        d.slen = e->slen.p;
    }
    HIPCHK(e, hipMemcpy(e->alive.p, e->h_alive.data(), e->h_alive.size(), hipMemcpyHostToDevice));
    e->dev_alive = e->h_alive;
    if (g_poison) {   // the slots behind the population (no road user, no sentinel duty but the record): NaN, not zero
        const double qnan = std::numeric_limits<double>::quiet_NaN();
        auto fill = [&](std::vector<double> &v) {
            const size_t rows = v.size() / (size_t)e->cap;
            for (size_t r = 0; r < rows; r++) std::fill(v.begin() + r * e->cap + n, v.begin() + (r + 1) * e->cap, qnan);
        };
        fill(e->h_s); fill(e->h_vdes); fill(e->h_znp); fill(e->h_hx); fill(e->h_hy); fill(e->h_lti); fill(e->h_ppsi); fill(e->h_F);
    }
#define H2D(vec, buf) HIPCHK(e, hipMemcpy(buf.p, vec.data(), vec.size() * sizeof(vec[0]), hipMemcpyHostToDevice))
    H2D(e->h_s, e->s);
    H2D(e->h_vdes, e->vdes);
    H2D(e->h_znp, e->znp);
    H2D(e->h_hx, e->hx);
    H2D(e->h_hy, e->hy);
    H2D(e->h_lti, e->lti);
    H2D(e->h_ppsi, e->ppsi);
    H2D(e->h_F, e->F);
    H2D(e->h_ptr, e->ptr);
    H2D(e->h_ti, e->ti);
    H2D(e->h_dgood, e->dgood);
    H2D(e->h_znav, e->znav);
    H2D(e->h_zrid, e->zrid);
    H2D(e->h_status, e->status);
#undef H2D
    // origin of the fp32 records: centre of the bounding box of the population (and road)
    if (n > 0) {
        double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
        for (int64_t a = 0; a < n; a++) {
            x0 = std::min(x0, e->h_s[a]);
            x1 = std::max(x1, e->h_s[a]);
            y0 = std::min(y0, e->h_s[e->cap + a]);
            y1 = std::max(y1, e->h_s[e->cap + a]);
        }
        d.ox = 0.5 * (x0 + x1);
        d.oy = 0.5 * (y0 + y1);
        if (!std::isfinite(d.ox)) d.ox = 0;
        if (!std::isfinite(d.oy)) d.oy = 0;
    }
    double rbox[4];
    const bool road_grid = road_grid_wanted(e, rbox);
    if (road_grid) {   // a lattice over the road network (csf_road.hip) is anchored at the origin: the network's centre, which stays
        d.ox = std::nearbyint(0.5 * (rbox[0] + rbox[1]));
        d.oy = std::nearbyint(0.5 * (rbox[2] + rbox[3]));
    }
    {   // the largest coordinate a record can take, relative to that origin (set_fov_band): road users and the prescribed
        // trajectories of UncontrolledVehicles now; arrivals and motion are added as they come
        double cb = 0;
        for (int64_t a = 0; a < n; a++) {
            cb = std::max({cb, std::fabs(e->h_s[a] - d.ox), std::fabs(e->h_s[e->cap + a] - d.oy)});
            const std::vector<double> &sc = e->h_script[(size_t)a];
            for (size_t r = 0; r + 3 < sc.size(); r += 4) cb = std::max({cb, std::fabs(sc[r] - d.ox), std::fabs(sc[r + 1] - d.oy)});
        }
        e->coord_bound0 = std::isfinite(cb) ? cb : 0.0;
        e->moves = 0;
    }
    d.nv = (int64_t)e->h_road.size() / 4;
    d.nv_pad = (d.nv + 63) / 64 * 64;
    {
        std::vector<float4> rv;
        std::vector<float2> rvo;
        d.road_np = pack_road(e->h_road.data(), d.nv, d.ox, d.oy, rv, rvo);
        if (d.nv > 0) {
            if (rv.size() > e->rv.n) HIPCHK(e, e->rv.alloc(rv.size()));
            if (rvo.size() > e->rvo.n) HIPCHK(e, e->rvo.alloc(rvo.size()));
            HIPCHK(e, hipMemcpy(e->rv.p, rv.data(), rv.size() * sizeof(float4), hipMemcpyHostToDevice));
            HIPCHK(e, hipMemcpy(e->rvo.p, rvo.data(), rvo.size() * sizeof(float2), hipMemcpyHostToDevice));
        }
    }
    d.rvo = e->rvo.p;
    d.rv = e->rv.p;
    d.rg_nx = d.rg_ny = 0;
    if (road_grid) {
        const int rc = build_road_grid(e, rbox);
        if (rc) return rc;
    }
    set_shard(e);
    if ((size_t)d.n_pad > e->rec.n) return fail(e, CSF_E_CAPACITY, "record buffer too small for this shard layout");
    HIPCHK(e, hipMemsetAsync(e->part.p, 0, e->part.n * sizeof(float2), e->main));   // a new layout starts from clean partial sums
    // records as offsets from the scene origin first (what the sort keys are made of); the re-binning then gives every
    // record its own origin and rewrites it from the fp64 state just uploaded
    HIPCHK(e, hipMemsetAsync(e->rorg.p, 0, e->rorg.n * sizeof(float2), e->main));
    e->state_all_current = true;
    e->xbuf_fresh = false;                                       // (exchange records of the population as it was: every record is rewritten from the state)
    launch_records(d, e->main);
    int rrc = rebin(e);
    if (rrc) return rrc;
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(e->main));
    e->gather_pending = false;
    e->dirty = false;
    // what the side-by-side tick needs beside these arrays (enqueue_chase_tick): allocated here, where the host waits anyway - an
    // allocation synchronises, and the first such tick may lie inside a region somebody is timing
    if (chase_shape(e)) {
        int rcc = chase_alloc(e);
        if (rcc) return rcc;
    }
    return CSF_OK;
}
