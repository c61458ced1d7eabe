// engine/abi_scene.inc - C ABI: calibration on closed-loop scenes.  A data set of small scenes resident on the device, workgroup = (parameter set, scene), the error against the recorded trajectories summed in the launch.
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)
//
// csf_calib_eval (engine/abi_calib.inc) replays recorded forces, which couples no two vehicles: the parameters of the social-force
// field cannot be fitted with it.  Here every candidate set simulates every scene of the data set with its riders together - the
// one-wave tick of csf_step for up to 32 road users (csf_small_body.inc) - and the kernel sums the error against the recorded
// trajectories per rider (csf_scene.hip: scene_eval_kernel).  One copy of the call's table of sets, one launch, one wait per call.
//
// On the host: the load's core (SceneCalibState) and one LAYER per optional feature, each with held() and fill(SceneDev &); a setter
// validates, builds a fresh layer - everything that can fail - and moves it in (DESIGN.md 4.10, The host layers).

extern "C++" {

// The reset image (csf_scene.h: SceneDev), by rider: an array is declared here and named once in each of alloc, capture and fill.
// vdes, qbeg, qlen: shared lanes only - what a slot kept for good while it had one rider
struct SceneImage {
    DevBuf<double> s, lti, ppsi, znp, hx0, hy0, vdes;
    DevBuf<int32_t> ti, ptr, qlen;
    DevBuf<uint32_t> status;
    DevBuf<uint8_t> znav;
    DevBuf<int64_t> qbeg;
    hipError_t alloc(size_t R, bool shared) {
        hipError_t r = s.alloc(STATE_ROWS * R);
        if (r == hipSuccess) r = lti.alloc(5 * R);
        if (r == hipSuccess) r = ppsi.alloc(R);
        if (r == hipSuccess) r = znp.alloc(3 * R);
        if (r == hipSuccess) r = hx0.alloc(R);
        if (r == hipSuccess) r = hy0.alloc(R);
        if (r == hipSuccess) r = ti.alloc(R);
        if (r == hipSuccess) r = ptr.alloc(R);
        if (r == hipSuccess) r = status.alloc(R);
        if (r == hipSuccess) r = znav.alloc(R);
        if (r == hipSuccess && shared) r = vdes.alloc(R);
        if (r == hipSuccess && shared) r = qbeg.alloc(R);
        if (r == hipSuccess && shared) r = qlen.alloc(R);
        return r;
    }
    // what csf_add_agents made of the first R slots (the caller has waited for the stream)
    hipError_t capture(const csf_engine *e, size_t R, bool shared) {
        const size_t cap = (size_t)e->cap;
        hipError_t c = s.copy_rows(e->s, R, cap, STATE_ROWS);
        if (c == hipSuccess) c = lti.copy_rows(e->lti, R, cap, 5);
        if (c == hipSuccess) c = znp.copy_rows(e->znp, R, cap, 3);
        if (c == hipSuccess) c = ppsi.copy_rows(e->ppsi, R, cap);
        if (c == hipSuccess) c = hx0.copy_rows(e->hx, R, cap);         // (row 0 of the ring: csf_scene.h)
        if (c == hipSuccess) c = hy0.copy_rows(e->hy, R, cap);
        if (c == hipSuccess) c = ti.copy_rows(e->ti, R, cap);
        if (c == hipSuccess) c = ptr.copy_rows(e->ptr, R, cap);
        if (c == hipSuccess) c = status.copy_rows(e->status, R, cap);
        if (c == hipSuccess) c = znav.copy_rows(e->znav, R, cap);
        if (c == hipSuccess && shared) c = vdes.copy_rows(e->vdes, R, cap);
        if (c == hipSuccess && shared) c = qbeg.copy_rows(e->qbeg, R, cap);
        if (c == hipSuccess && shared) c = qlen.copy_rows(e->qlen, R, cap);
        return c;
    }
    void fill(SceneDev &c) const {
        c.img_s = s.p, c.img_lti = lti.p, c.img_ppsi = ppsi.p, c.img_znp = znp.p, c.img_hx0 = hx0.p, c.img_hy0 = hy0.p;
        c.img_ti = ti.p, c.img_ptr = ptr.p, c.img_status = status.p, c.img_znav = znav.p;
        c.img_vdes = vdes.p, c.img_qbeg = qbeg.p, c.img_qlen = qlen.p;
    }
};

// csf_scene_calib_replay: the riders that follow their recording (csf_scene.h).  Absent: the kernel's path without a replay
struct SceneReplay {
    DevBuf<int32_t> index;                   // [R]
    DevBuf<double> rows;                     // [n_ticks][n][4]
    int32_t n = 0;
    double bound = 0.0;                      // largest |coordinate| of a replayed row, relative to the scene origin
    bool held() const { return n > 0; }
    void fill(SceneDev &c) const { c.n_rep = n, c.rep_index = held() ? index.p : nullptr, c.rep = held() ? rows.p : nullptr; }
};

// csf_scene_calib_road: a road per scene, shared by all candidate sets (DESIGN.md 4.10c).  Absent: every view has nv = nv_pad = 0 and
// a launch asks for no dynamic LDS.  (The views that point into rv / rvo are the core's: `table`.)
struct SceneRoad {
    DevBuf<float4> rv;                       // [stride] the packed roads of the scenes, one after the other
    DevBuf<float2> rvo;                      // their tile origins
    DevBuf<float4> blk;                      // [sets][stride] the roads as a set's parameters make them: allocated by the first evaluation that overrides them
    int64_t stride = 0;
    int32_t max_pad = 0;                     // largest nv_pad of a scene
    bool held() const { return stride > 0; }
    void fill(SceneDev &c) const {
        c.road_rv = held() ? rv.p : nullptr, c.road_blk = nullptr;
        c.road_stride = stride;
        c.road_lds = (uint32_t)max_pad * (uint32_t)sizeof(float4);
    }
};

// csf_scene_calib_windows, or the windows a load on shared lanes came with (DESIGN.md 4.10d).  Absent: the kernel instance without a mask
struct SceneWindows {
    DevBuf<int32_t> enter, exit;             // [R]
    bool held() const { return enter.n > 0; }
    void fill(SceneDev &c) const { c.win_enter = held() ? enter.p : nullptr, c.win_exit = held() ? exit.p : nullptr; }
};

// csf_scene_calib_load_shared (DESIGN.md 4.10e).  Absent: slot = set * R + rider.  Else slot = set * Lsum + lane_off[scene] + lane, the
// windows came with the load, and the image holds vdes, qbeg and qlen.  csf_scene_calib_load_wide (4.10f): wide_from > 0, the scenes with
// n_lanes >= wide_from are WIDE - scn_w, their views in table_w -, `table` holds the narrow ones alone (csf_scene.h: SceneWideDev)
struct SceneLanes {
    int32_t Lsum = 0, wide_from = 0;
    std::vector<int32_t> h_nl;               // [n_scn] lanes of every scene
    DevBuf<int32_t> lane_off, lane_first, rider_next;   // [n_scn + 1], [Lsum], [R]: the chains (csf_scene.h)
    std::vector<int32_t> h_scn_w, h_scn_n;   // the wide scenes and the narrow ones, ascending
    DevBuf<Dev> table_w;                     // [max_sets][n_wide]
    DevBuf<int32_t> scn_w, len_n, roff_n, lane_off_n;
    bool held() const { return Lsum > 0; }
    bool wide() const { return wide_from > 0; }
    bool is_wide(size_t q) const { return wide() && h_nl[q] >= wide_from; }
    void fill(SceneDev &c) const { c.lane_off = lane_off.p, c.lane_first = lane_first.p, c.rider_next = rider_next.p; }
    void fill(SceneWideDev &w) const {
        w.table_w = table_w.p, w.scn_w = scn_w.p;
        w.n_wide = (int32_t)h_scn_w.size(), w.n_narrow = (int32_t)h_scn_n.size();
        w.len_n = len_n.p, w.roff_n = roff_n.p, w.lane_off_n = lane_off_n.p;
    }
};

// csf_scene_calib_groups / _lane_groups (DESIGN.md 4.10g, 4.10h): rider groups with parameter sets of their own; the call's table is
// [n_sets][n] records in `sets`.  csf_scene_calib_classes / _lane_classes (4.10i, 4.10j): class_models [n] the vehicle class of every group.  Dev::ns of the engine
// is the widest of them while they are held - ns_own is what it was -, and an evaluation restores from the class image: state rows, side
// state and first ring row as a fresh vehicle of the rider's OWN class has them (abi_population.inc: add_agents_impl, side_state)
struct SceneGroups {
    int32_t n = 0;
    DevBuf<uint8_t> group;                   // [R]
    DevBuf<SceneSet> sets;                   // [max_sets][n]
    std::unique_ptr<HostBuf<SceneSet, false>> pin;   // ... and where the host composes them
    std::vector<int32_t> class_models;
    int32_t ns_own = 0;
    DevBuf<double> cimg_s, cimg_lti, cimg_ppsi, cimg_hx0, cimg_hy0;
    bool held() const { return n > 0; }
    bool mixed() const { return !class_models.empty(); }
    // (behind SceneImage::fill: the class image overrides five of its pointers)
    void fill(SceneDev &c) const {
        if (held()) c.group = group.p, c.n_groups = n;
        if (mixed()) c.img_s = cimg_s.p, c.img_lti = cimg_lti.p, c.img_ppsi = cimg_ppsi.p, c.img_hx0 = cimg_hx0.p, c.img_hy0 = cimg_hy0.p;
    }
};

struct SceneCalibState {
    int32_t n_scn = 0, n_feat = 0, max_sets = 0, R = 0;
    int64_t n_ticks = 0;
    int32_t feat[CALIB_MAX_FEAT] = {0, 0, 0, 0, 0, 0};
    double coord_bound = 0.0;                // largest |coordinate| of a start position, relative to the scene origin
    DevBuf<double> obj, states;
    DevBuf<int32_t> len, roff;
    std::vector<int32_t> h_len, h_roff;      // the scenes' lengths and first riders, as on the device
    DevBuf<Dev> table;                       // [max_sets][n_scn] the views of the slot blocks (csf_scene_calib_road: with the roads)
    std::vector<Dev> h_table;                // the table as the load built it: no roads, the engine's origin
    std::vector<double> h_ox, h_oy;          // [n_scn] the origin a stand-alone engine that holds the scene would have (mirror.inc)
    DevBuf<SceneSet> sets;                   // [max_sets] the call's candidate sets ...
    HostBuf<SceneSet, false> sets_pin;       // ... and where the host composes them: one copy per call
    HostBuf<double2> sums;                   // [max_sets * R] written by the kernel (mapped)
    int64_t launches = 0;                    // csf_scene_calib_launches
    SceneImage image;
    SceneReplay replay;
    SceneRoad road;
    SceneWindows windows;
    SceneLanes lanes;
    SceneGroups groups;
};

// the classes of csf_scene_calib_classes go: the state width is the engine's own again
static void scene_drop_classes(csf_engine *e, const SceneCalibState &cs) {
    if (cs.groups.mixed()) e->d.ns = cs.groups.ns_own;
}

// "no closed-loop data set"; `calib_tail`: what the call says instead to an engine that holds the data set of csf_calib_load
static int scene_none(csf_engine *e, const char *fn, const char *calib_tail = nullptr) {
    if (e->calib && calib_tail) return fail(e, CSF_E_STATE, "%s: the engine holds the data set of csf_calib_load, %s", fn, calib_tail);
    return fail(e, CSF_E_STATE, "%s: no closed-loop data set (csf_scene_calib_load first)", fn);
}

// The views on the device from the whole table [max_sets][n_scn] on the host: all of it in `table`, or - a wide load - the narrow
// scenes' in `table` and the wide scenes' in `table_w`, both [max_sets][their scenes].  Allocates; the caller waits for the device.
static hipError_t scene_upload_tables(const SceneCalibState &cs, const std::vector<Dev> &tab, DevBuf<Dev> &table, DevBuf<Dev> &table_w) {
    const size_t n_scn = (size_t)cs.n_scn, sets = (size_t)cs.max_sets;
    if (!cs.lanes.wide()) return table.upload(tab);
    hipError_t r = hipSuccess;
    const std::vector<int32_t> *part[2] = {&cs.lanes.h_scn_n, &cs.lanes.h_scn_w};
    DevBuf<Dev> *dst[2] = {&table, &table_w};
    for (int w = 0; w < 2 && r == hipSuccess; w++) {
        const size_t m = part[w]->size();
        std::vector<Dev> sub;
        sub.reserve(sets * m);
        for (size_t k = 0; k < sets; k++)
            for (size_t j = 0; j < m; j++) sub.push_back(tab[k * n_scn + (size_t)(*part[w])[j]]);
        r = dst[w]->upload(sub);
    }
    return r;
}

// Shared lanes, host only: the occupants of a lane one after the other - lo [n_scn + 1] the first lane of every scene, lfirst [Lsum],
// rnext [R] (csf_scene.h).  A chain holds the lane's riders with a non-empty window in entry order; names the first offending rider
static int scene_lane_chains(csf_engine *e, const char *fn, int32_t n_scn, const int32_t *n_riders, const int32_t *n_lanes, const int32_t *lane,
                             const int32_t *enter, const int32_t *exit, const int32_t *lengths, int64_t n_ticks, int32_t R, int32_t Lsum,
                             std::vector<int32_t> &lo, std::vector<int32_t> &lfirst, std::vector<int32_t> &rnext) {
    lo.assign((size_t)n_scn + 1, 0), lfirst.assign((size_t)Lsum, -1), rnext.assign((size_t)R, -1);
    std::vector<int32_t> idx;
    for (int32_t q = 0, r0 = 0; q < n_scn; r0 += n_riders[q], q++) {
        lo[(size_t)q + 1] = lo[(size_t)q] + n_lanes[q];
        const int32_t ticks = lengths ? lengths[q] : (int32_t)n_ticks;
        idx.clear();
        for (int32_t r = r0; r < r0 + n_riders[q]; r++) {
            if (lane[r] < 0 || lane[r] >= n_lanes[q]) return fail(e, CSF_E_ARG, "%s: rider %d is on lane %d, scene %d has %d lanes", fn, (int)r, (int)lane[r], (int)q, (int)n_lanes[q]);
            if (enter[r] < 0 || enter[r] > exit[r] || exit[r] > ticks)
                return fail(e, CSF_E_ARG, "%s: rider %d has the window [%d, %d), scene %d has %d ticks (0 <= enter <= exit <= ticks)", fn, (int)r, (int)enter[r], (int)exit[r], (int)q, (int)ticks);
            if (enter[r] < exit[r]) idx.push_back(r);
        }
        std::stable_sort(idx.begin(), idx.end(), [&](int32_t a, int32_t b) { return lane[a] != lane[b] ? lane[a] < lane[b] : enter[a] < enter[b]; });
        for (size_t i = 0; i < idx.size(); i++) {
            const int32_t r = idx[i];
            if (i > 0 && lane[idx[i - 1]] == lane[r]) {
                const int32_t before = idx[i - 1];
                if (exit[before] > enter[r])
                    return fail(e, CSF_E_ARG, "%s: riders %d [%d, %d) and %d [%d, %d) overlap on lane %d of scene %d", fn, (int)before, (int)enter[before], (int)exit[before], (int)r, (int)enter[r], (int)exit[r], (int)lane[r], (int)q);
                rnext[(size_t)before] = r;
            } else {
                lfirst[(size_t)lo[(size_t)q] + (size_t)lane[r]] = r;
            }
        }
    }
    return CSF_OK;
}

// The n vehicles handed to add_agents_impl.  Without shared lanes slot set * R + rider: every set starts every scene from its start states,
// with its queues.  With them the R riders once, then spare slots up to those that are run: rider 0 with the first row of its queue
static int scene_add_population(csf_engine *e, bool sh, int32_t R, int64_t n, const double *s0, const double *v_desired, const int64_t *dest_offsets,
                                const double *dest_xyz_stop) {
    const size_t ns = (size_t)e->d.ns;
    std::vector<double> s_all((size_t)n * ns), vd((size_t)n), rows_all;
    std::vector<int64_t> off_all((size_t)n + 1, 0);
    const int64_t q_rows = dest_offsets[R] - dest_offsets[0];
    rows_all.reserve(3 * (size_t)(sh ? q_rows + (n - R) : n / R * q_rows));
    for (int64_t i = 0; i < n; i++) {
        const bool spare = sh && i >= R;
        const size_t r = spare ? 0 : (size_t)(i % R);
        std::memcpy(&s_all[(size_t)i * ns], s0 + r * ns, ns * sizeof(double));
        vd[(size_t)i] = v_desired[r];
        const double *rows = dest_xyz_stop + 3 * dest_offsets[r];
        rows_all.insert(rows_all.end(), rows, rows + 3 * (spare ? 1 : dest_offsets[r + 1] - dest_offsets[r]));
        off_all[(size_t)i + 1] = (int64_t)(rows_all.size() / 3);
    }
    return add_agents_impl(e, n, s_all.data(), vd.data(), off_all.data(), rows_all.data());
}

// The views: the engine's Dev with every per-slot array shifted to the block of (set, scene) and the population the scene's.  What the
// one-wave tick does not touch - the binned order, the exchange records, the rings of a recording - is switched off.
static std::vector<Dev> scene_views(const Dev &d0, int32_t max_sets, int32_t n_scn, const int32_t *n_riders, const int32_t *n_lanes, int32_t R,
                                    int32_t Lsum, const std::vector<int32_t> &lo, const std::vector<int32_t> &ro) {
    const bool sh = n_lanes != nullptr;
    std::vector<Dev> tab((size_t)max_sets * (size_t)n_scn, d0);
    for (int32_t k = 0; k < max_sets; k++)
        for (int32_t q = 0; q < n_scn; q++) {
            Dev &v = tab[(size_t)k * (size_t)n_scn + (size_t)q];
            const int64_t b = sh ? (int64_t)k * Lsum + lo[(size_t)q] : (int64_t)k * R + ro[(size_t)q];
            v.n = v.n_live = v.hi = sh ? n_lanes[q] : n_riders[q];
            v.lo = 0;
            v.n_classes = 1;
            v.s = d0.s + b, v.vdes = d0.vdes + b, v.qbeg = d0.qbeg + b, v.qlen = d0.qlen + b, v.ptr = d0.ptr + b, v.znav = d0.znav + b;
            v.znp = d0.znp + b, v.ti = d0.ti + b, v.hx = d0.hx + b, v.hy = d0.hy + b, v.lti = d0.lti + b, v.zrid = d0.zrid + b;
            v.dgood = d0.dgood + b, v.ppsi = d0.ppsi + b, v.F = d0.F + b, v.status = d0.status + b, v.froad = d0.froad + b;
            v.alive = d0.alive + b;
            v.rorg = d0.rorg + b;
            v.rec = v.rec_w = d0.rec + b;
            v.recg = v.recg_w = d0.recg + b;
            v.rec2 = v.rec2_w = d0.rec2 ? d0.rec2 + b : nullptr;
            v.F_rows = 6;
            v.recs_valid = 0, v.recv_binned = 0, v.keep_lo = 0, v.classify = 0;
            v.xbuf = nullptr, v.src64_w = nullptr, v.order = nullptr;
            v.nv = v.nv_pad = 0;
            v.replay_len = nullptr, v.replay_tick = 0, v.tick = 0;
            v.hist = nullptr, v.hist_F = nullptr, v.rec_tick = nullptr, v.hist_stride = 1, v.hist_cap = 1;
            v.snap = nullptr, v.atrace = nullptr, v.trace = nullptr, v.pair_count = nullptr;
        }
    return tab;
}

// coord_bound, and the origin of a stand-alone engine that holds scene q: the centre of the box of its start positions (mirror.inc: upload_all)
static void scene_origins(SceneCalibState &cs, const Dev &d0, const double *s0, const std::vector<int32_t> &ro) {
    const size_t ns = (size_t)d0.ns;
    double cb = 0.0;
    for (int32_t i = 0; i < cs.R; i++) cb = std::max({cb, std::fabs(s0[(size_t)i * ns] - d0.ox), std::fabs(s0[(size_t)i * ns + 1] - d0.oy)});
    cs.coord_bound = cb;
    cs.h_ox.assign((size_t)cs.n_scn, 0.0), cs.h_oy.assign((size_t)cs.n_scn, 0.0);
    for (int32_t q = 0; q < cs.n_scn; q++) {
        double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
        for (int32_t i = ro[(size_t)q]; i < ro[(size_t)q + 1]; i++) {
            x0 = std::min(x0, s0[(size_t)i * ns]), x1 = std::max(x1, s0[(size_t)i * ns]);
            y0 = std::min(y0, s0[(size_t)i * ns + 1]), y1 = std::max(y1, s0[(size_t)i * ns + 1]);
        }
        const double ox = 0.5 * (x0 + x1), oy = 0.5 * (y0 + y1);
        cs.h_ox[(size_t)q] = std::isfinite(ox) ? ox : 0.0;
        cs.h_oy[(size_t)q] = std::isfinite(oy) ? oy : 0.0;
    }
}

}  // extern "C++"

// csf_scene_calib_load (n_lanes == NULL), csf_scene_calib_load_shared and csf_scene_calib_load_wide: `fn` names the call in the messages,
// lane_max is the most lanes a scene may have, wide_from == 0 no wide load (else: scenes with n_lanes >= wide_from are wide)
static int scene_load_impl(csf_engine *e, const char *fn, int32_t n_scn, const int32_t *n_riders, const int32_t *n_lanes, const int32_t *lane,
                           const int32_t *enter, const int32_t *exit, int64_t n_ticks, const double *s0, const double *v_desired,
                           const int64_t *dest_offsets, const double *dest_xyz_stop, const int32_t *lengths, const double *objective,
                           int32_t n_feat, const int32_t *feat, int32_t max_sets, int32_t lane_max = SMALL_MAX, int32_t wide_from = 0) {
    // the arguments and the engine
    const bool sh = n_lanes != nullptr;
    if (!n_riders || !s0 || !v_desired || !dest_offsets || !dest_xyz_stop || !objective || !feat) return fail(e, CSF_E_ARG, "%s: NULL array", fn);
    if (sh && (!lane || !enter || !exit)) return fail(e, CSF_E_ARG, "%s: NULL array", fn);
    if (n_scn < 1 || n_scn > (1 << 20) || n_ticks < 1 || n_ticks > 2000000000 || n_feat < 1 || n_feat > CALIB_MAX_FEAT || max_sets < 1 || max_sets > 256)
        return fail(e, CSF_E_ARG, "%s: 1 <= n_scn <= 2^20, 1 <= n_ticks <= 2e9, 1 <= n_feat <= %d, 1 <= max_sets <= 256", fn, CALIB_MAX_FEAT);
    if (e->scene_calib) return fail(e, CSF_E_STATE, "%s: the engine holds a closed-loop data set already (csf_scene_calib_clear first)", fn);
    if (e->calib) return fail(e, CSF_E_STATE, "%s: the engine holds a calibration data set (csf_calib_clear first)", fn);
    if (int irc = calib_load_refuses(e, fn)) return irc;
    if (e->world > 1 || e->nccl) return fail(e, CSF_E_STATE, "%s: a sharded engine holds no scenes", fn);
    if (!e->h_road.empty()) return fail(e, CSF_E_STATE, "%s: the engine has a road of its own (csf_set_road_vertices); the roads of scenes are given by csf_scene_calib_road", fn);
    if (e->d.hist != nullptr) return fail(e, CSF_E_STATE, "%s: the engine records (csf_record / csf_enable_history); an evaluation writes its own samples", fn);
    if (e->classes.size() != 1) return fail(e, CSF_E_STATE, "%s: the engine has %d parameter sets; the candidates of an evaluation replace ONE", fn, (int)e->classes.size());
    if (e->d.p.model == CSF_UNCONTROLLED) return fail(e, CSF_E_ARG, "%s: an UncontrolledVehicle follows its trajectory whatever the field", fn);
    int64_t R64 = 0, L64 = 0;
    for (int32_t q = 0; q < n_scn; q++) {
        // (a shared roster has no bound of its own: what is bounded is its lanes)
        if (n_riders[q] < 1 || (!sh && n_riders[q] > SMALL_MAX)) return fail(e, CSF_E_ARG, "%s: scene %d has %d road users (1 .. %d)", fn, (int)q, (int)n_riders[q], SMALL_MAX);
        if (sh && (n_lanes[q] < 1 || n_lanes[q] > lane_max)) return fail(e, CSF_E_ARG, "%s: scene %d has %d lanes (1 .. %d)", fn, (int)q, (int)n_lanes[q], (int)lane_max);
        if (sh && wide_from > 0 && n_lanes[q] > SMALL_MAX && n_lanes[q] < wide_from)
            return fail(e, CSF_E_ARG, "%s: scene %d has %d lanes and wide_from is %d: the one-wave tick takes 1 .. %d", fn, (int)q, (int)n_lanes[q], (int)wide_from, SMALL_MAX);
        R64 += n_riders[q];
        L64 += sh ? n_lanes[q] : 0;
    }
    if (sh && R64 > (1 << 24)) return fail(e, CSF_E_ARG, "%s: %lld road users in all (at most 2^24)", fn, (long long)R64);
    // the slots: max_sets x R without shared lanes.  With them the engine holds every rider once - the fresh vehicles the image is
    // taken from, and their queues, which stay where they are - and max_sets x Lsum slots are run: the larger of the two
    const int64_t n = sh ? std::max(R64, (int64_t)max_sets * L64) : (int64_t)max_sets * R64;
    if (n > e->cap_user) {
        if (sh) return fail(e, CSF_E_CAPACITY, "%s: max(riders, max_sets x lanes) = %lld road users, capacity %lld", fn, (long long)n, (long long)e->cap_user);
        return fail(e, CSF_E_CAPACITY, "%s: max_sets x riders = %lld road users, capacity %lld", fn, (long long)n, (long long)e->cap_user);
    }
    const int32_t R = (int32_t)R64, Lsum = (int32_t)L64;
    for (int32_t q = 0; lengths && q < n_scn; q++)
        if (lengths[q] < 0 || lengths[q] > n_ticks) return fail(e, CSF_E_ARG, "%s: lengths[%d] = %d outside 0 .. %lld", fn, (int)q, (int)lengths[q], (long long)n_ticks);
    for (int32_t k = 0; k < n_feat; k++)
        if (feat[k] < 0 || feat[k] >= CALIB_MAX_FEAT) return fail(e, CSF_E_ARG, "%s: feature %d names no row of vehicle.traj (0 .. %d)", fn, (int)feat[k], CALIB_MAX_FEAT - 1);
    for (int32_t r = 0; r < R; r++) {
        const int64_t rows = dest_offsets[r + 1] - dest_offsets[r];
        if (dest_offsets[r] < 0 || rows < 1 || rows > MAX_QUEUE_ROWS) return fail(e, CSF_E_ARG, "%s: the destination queue of rider %d has %lld rows (1 .. %lld)", fn, (int)r, (long long)rows, (long long)MAX_QUEUE_ROWS);
    }
    std::vector<int32_t> lo, lfirst, rnext;
    if (sh)
        if (int rc = scene_lane_chains(e, fn, n_scn, n_riders, n_lanes, lane, enter, exit, lengths, n_ticks, R, Lsum, lo, lfirst, rnext)) return rc;
    HIPCHK(e, hipSetDevice(e->device));
    // everything that can fail first: a refused call changes nothing
    auto cs = std::make_shared<SceneCalibState>();
    SceneLanes &ln = cs->lanes;
    ln.Lsum = Lsum;
    ln.wide_from = sh ? wide_from : 0;
    if (sh) ln.h_nl.assign(n_lanes, n_lanes + n_scn);
    for (int32_t q = 0; ln.wide() && q < n_scn; q++) (ln.is_wide((size_t)q) ? ln.h_scn_w : ln.h_scn_n).push_back(q);
    cs->n_scn = n_scn, cs->n_feat = n_feat, cs->max_sets = max_sets, cs->n_ticks = n_ticks, cs->R = R;
    for (int32_t k = 0; k < n_feat; k++) cs->feat[k] = feat[k];
    const size_t Rs = (size_t)R;
    std::vector<int32_t> ls((size_t)n_scn), ro((size_t)n_scn + 1, 0);
    for (int32_t q = 0; q < n_scn; q++) ls[(size_t)q] = lengths ? lengths[q] : (int32_t)n_ticks, ro[(size_t)q + 1] = ro[(size_t)q] + n_riders[q];
    hipError_t r = cs->obj.upload(objective, (size_t)n_ticks * Rs * (size_t)n_feat);
    if (r == hipSuccess) r = cs->image.alloc(Rs, sh);
    if (r == hipSuccess) r = cs->len.upload(ls);
    if (r == hipSuccess) r = cs->roff.upload(ro);
    // (the table itself is allocated where it is filled: scene_upload_tables)
    if (r == hipSuccess) r = cs->sets.alloc((size_t)max_sets);
    if (r == hipSuccess) r = cs->sets_pin.alloc((size_t)max_sets);
    if (r == hipSuccess) r = cs->sums.alloc((size_t)max_sets * Rs);
    if (sh) {
        if (r == hipSuccess) r = ln.lane_off.upload(lo);
        if (r == hipSuccess) r = ln.lane_first.upload(lfirst);
        if (r == hipSuccess) r = ln.rider_next.upload(rnext);
        if (r == hipSuccess) r = cs->windows.enter.upload(enter, Rs);
        if (r == hipSuccess) r = cs->windows.exit.upload(exit, Rs);
    }
    if (ln.wide()) {   // what scene_lanes_kernel reads per scene, for the narrow scenes alone (csf_scene.h: SceneWideDev)
        const size_t m = ln.h_scn_n.size();
        std::vector<int32_t> lnn(m), rn(m + 1, R), on(m);
        for (size_t j = 0; j < m; j++) {
            const size_t q = (size_t)ln.h_scn_n[j];
            lnn[j] = ls[q], rn[j] = ro[q], on[j] = lo[q];
        }
        if (m > 0) rn[m] = ro[(size_t)ln.h_scn_n[m - 1] + 1];
        if (r == hipSuccess) r = ln.scn_w.upload(ln.h_scn_w);
        if (r == hipSuccess) r = ln.len_n.upload(lnn);
        if (r == hipSuccess) r = ln.roff_n.upload(rn);
        if (r == hipSuccess) r = ln.lane_off_n.upload(on);
    }
    if (r != hipSuccess) return fail(e, CSF_E_DEVICE, "%s: no memory for the data set: %s", fn, hipGetErrorString(r));
    std::memset(cs->sets_pin.p, 0, (size_t)max_sets * sizeof(SceneSet));
    int rc = scene_add_population(e, sh, R, n, s0, v_desired, dest_offsets, dest_xyz_stop);
    if (rc) return rc;
    if ((rc = upload_all(e))) return calib_undo_load(e, rc);
    if ((rc = ensure_compact(e))) return calib_undo_load(e, rc);             // slot == place in the population order: slot a is (a / R, a % R)
    // the image: what csf_add_agents made of the first set's slots (the stream is idle: upload_all has waited)
    hipError_t c = hipStreamSynchronize(e->main);
    if (c == hipSuccess) c = cs->image.capture(e, Rs, sh);
    if (c != hipSuccess) return calib_undo_load(e, fail(e, CSF_E_DEVICE, "%s: the reset image: %s", fn, hipGetErrorString(c)));
    std::vector<Dev> tab = scene_views(e->d, max_sets, n_scn, n_riders, n_lanes, R, Lsum, lo, ro);
    c = scene_upload_tables(*cs, tab, cs->table, ln.table_w);
    if (c == hipSuccess) c = hipDeviceSynchronize();
    if (c != hipSuccess) return calib_undo_load(e, fail(e, CSF_E_DEVICE, "%s: the table of views: %s", fn, hipGetErrorString(c)));
    scene_origins(*cs, e->d, s0, ro);
    cs->h_table = std::move(tab);
    cs->h_len = std::move(ls), cs->h_roff = std::move(ro);
    e->scene_calib = std::move(cs);
    return CSF_OK;
}

int csf_scene_calib_load(csf_engine *e, int32_t n_scn, const int32_t *n_riders, int64_t n_ticks, const double *s0, const double *v_desired,
                         const int64_t *dest_offsets, const double *dest_xyz_stop, const int32_t *lengths, const double *objective,
                         int32_t n_feat, const int32_t *feat, int32_t max_sets) try {
    if (!e) return CSF_E_ARG;
    return scene_load_impl(e, "csf_scene_calib_load", n_scn, n_riders, nullptr, nullptr, nullptr, nullptr, n_ticks, s0, v_desired, dest_offsets,
                           dest_xyz_stop, lengths, objective, n_feat, feat, max_sets);
} catch (...) { return csf_caught(e); }

int csf_scene_calib_load_shared(csf_engine *e, int32_t n_scn, const int32_t *n_riders, const int32_t *n_lanes, const int32_t *lane,
                                const int32_t *enter, const int32_t *exit, int64_t n_ticks, const double *s0, const double *v_desired,
                                const int64_t *dest_offsets, const double *dest_xyz_stop, const int32_t *lengths, const double *objective,
                                int32_t n_feat, const int32_t *feat, int32_t max_sets) try {
    if (!e) return CSF_E_ARG;
    if (!n_lanes) return fail(e, CSF_E_ARG, "csf_scene_calib_load_shared: NULL array");
    return scene_load_impl(e, "csf_scene_calib_load_shared", n_scn, n_riders, n_lanes, lane, enter, exit, n_ticks, s0, v_desired, dest_offsets,
                           dest_xyz_stop, lengths, objective, n_feat, feat, max_sets);
} catch (...) { return csf_caught(e); }

int csf_scene_calib_load_wide(csf_engine *e, int32_t n_scn, const int32_t *n_riders, const int32_t *n_lanes, const int32_t *lane,
                              const int32_t *enter, const int32_t *exit, int64_t n_ticks, const double *s0, const double *v_desired,
                              const int64_t *dest_offsets, const double *dest_xyz_stop, const int32_t *lengths, const double *objective,
                              int32_t n_feat, const int32_t *feat, int32_t max_sets, int32_t wide_from) try {
    if (!e) return CSF_E_ARG;
    if (!n_lanes) return fail(e, CSF_E_ARG, "csf_scene_calib_load_wide: NULL array");
    if (wide_from < 1 || wide_from > WIDE_MAX + 1) return fail(e, CSF_E_ARG, "csf_scene_calib_load_wide: wide_from = %d outside 1 .. %d", (int)wide_from, WIDE_MAX + 1);
    return scene_load_impl(e, "csf_scene_calib_load_wide", n_scn, n_riders, n_lanes, lane, enter, exit, n_ticks, s0, v_desired, dest_offsets,
                           dest_xyz_stop, lengths, objective, n_feat, feat, max_sets, WIDE_MAX, wide_from);
} catch (...) { return csf_caught(e); }

int csf_scene_calib_eval(csf_engine *e, int32_t n_sets, const csf_params *params, size_t params_size, int32_t abi_version, double *sums_out,
                         int32_t stride, double *states_out) {
    return csf_scene_calib_eval_road(e, n_sets, params, params_size, abi_version, nullptr, nullptr, sums_out, stride, states_out);
}

// Dev::road_np of one sigma, as road_np_of decides it for a road whose edges share it
static int32_t road_np_sigma(double sg) { return sg == std::floor(sg) && sg >= 1 && sg <= 5 ? (int32_t)sg + 1 : 0; }

// the checks of an evaluation: csf_scene_calib_eval_road (one record per set) and csf_scene_calib_eval_groups (params is [n_sets][groups held])
static int scene_eval_check(csf_engine *e, int32_t n_sets, const csf_params *params, size_t params_size, int32_t abi_version, const double *road_F0,
                            const double *road_sigma, const double *sums_out, int32_t stride) {
    if (!e->scene_calib) return scene_none(e, "csf_scene_calib_eval");
    // before anything is read from `params` (csf_create_v)
    if (params_size != sizeof(csf_params) || abi_version != CSF_ABI_VERSION)
        return fail(e, CSF_E_ABI, "csf_scene_calib_eval: the caller's csf_params has %zu bytes and ABI %d, this library's has %zu bytes and ABI %d",
                    params_size, (int)abi_version, sizeof(csf_params), (int)CSF_ABI_VERSION);
    const SceneCalibState &cs = *e->scene_calib;
    if (!params || !sums_out) return fail(e, CSF_E_ARG, "csf_scene_calib_eval: NULL array");
    if (n_sets < 1 || n_sets > cs.max_sets) return fail(e, CSF_E_ARG, "csf_scene_calib_eval: %d parameter sets, the data set was loaded for 1 .. %d", (int)n_sets, (int)cs.max_sets);
    if (stride < 1) return fail(e, CSF_E_ARG, "csf_scene_calib_eval: stride must be >= 1");
    const int32_t G = std::max(cs.groups.n, 1);
    for (int32_t k = 0; k < n_sets * G; k++) {
        int rc = check_params(e, params + k);
        if (rc) return rc;
        if (cs.groups.mixed()) {                               // (csf_scene_calib_classes: record (set, g) is of the class loaded for group g)
            if (params[k].model != cs.groups.class_models[(size_t)(k % G)])
                return fail(e, CSF_E_ARG, "csf_scene_calib_eval_groups: the record of set %d, group %d is of vehicle class %d, the group was loaded with class %d (csf_scene_calib_classes)",
                            (int)(k / G), (int)(k % G), (int)params[k].model, (int)cs.groups.class_models[(size_t)(k % G)]);
        } else if (params[k].model != e->d.p.model) return fail(e, CSF_E_ARG, "csf_scene_calib_eval: parameter set %d is of vehicle class %d, the data set was loaded for class %d", (int)k, (int)params[k].model, (int)e->d.p.model);
        if (params[k].t_s != e->d.p.t_s || params[k].traj_len != e->d.p.traj_len)
            return fail(e, CSF_E_ARG, "csf_scene_calib_eval: parameter set %d: t_s and traj_len are the engine's (parameters.py:516-528)", (int)k);
    }
    const bool road_over = road_F0 != nullptr || road_sigma != nullptr;
    // road parameters per candidate set: both arrays or neither.  csf_set_road_vertices places no limit on sigma; a value that is
    // not finite is refused here as it is by csf_scene_calib_road
    if (road_over) {
        if (!road_F0 || !road_sigma) return fail(e, CSF_E_ARG, "csf_scene_calib_eval_road: road_F0 and road_sigma are given together or not at all");
        if (!cs.road.held()) return fail(e, CSF_E_STATE, "csf_scene_calib_eval_road: road parameters and no scene has a road (csf_scene_calib_road first)");
        for (int32_t k = 0; k < n_sets; k++) {
            if (!std::isfinite(road_F0[k]) || road_F0[k] < 0.0) return fail(e, CSF_E_ARG, "csf_scene_calib_eval_road: road_F0[%d] = %g is not a finite value >= 0", (int)k, road_F0[k]);
            if (!std::isfinite(road_sigma[k])) return fail(e, CSF_E_ARG, "csf_scene_calib_eval_road: road_sigma[%d] is not finite", (int)k);
        }
    }
    return CSF_OK;
}

// The table of this call, composed in pinned memory (the last call has been waited for): n_sets x G records at `pin`.  The bands of the
// fp32 field-of-view and side decisions (consts.inc: fov_band_consts) are those of the largest coordinate any rider can reach in n_ticks
// from the start of its scene with the set's speed clamp: conservative for every tick, and inside a band the kernel decides by the
// reference's fp64 chain, so its width changes no result.
static void scene_compose_sets(const csf_engine *e, const SceneCalibState &cs, int32_t n_sets, const csf_params *params, const double *road_F0,
                               const double *road_sigma, SceneSet *pin) {
    const bool groups = cs.groups.held(), road_over = road_F0 != nullptr;
    const int32_t G = std::max(cs.groups.n, 1);
    for (int32_t k = 0; k < n_sets * G; k++) {
        SceneSet &ss = pin[k];
        std::memset(&ss, 0, sizeof ss);
        ss.p = params[k];
        // (groups: the rule belongs to the intersection - the candidate's first record has it, as csf_set_param_classes gives every set
        // the engine's)
        if (groups) ss.p.priority_rule = params[k - k % G].priority_rule;
        // (derive_consts without update_far_radius: rfar, reach and tA0 .. tB1 stay 0.  They are the cull of the pair kernels
        // (csf_field.h: keep_x2) and depend on the population size, which differs from scene to scene; the one-wave tick culls
        // nothing and reads none of them.  A tick that does must get them per (set, scene), not from this record.)
        derive_pair_consts(ss.p, ss.pc, e->knobs.rnear);
        if (ss.p.model == CSF_PLANARBIKE) derive_planarbike(ss.p, ss.pb);
        double vmax = 0.0;                                      // (groups: the largest clamp among the candidate's records)
        for (int32_t g = k - k % G; g < k - k % G + G; g++)
            vmax = std::max({vmax, std::fabs(params[g].v_max_riding[0]), std::fabs(params[g].v_max_riding[1]), std::fabs(params[g].v_max_walk)});
        const double step = ss.p.t_s * vmax * 1.01 + 1e-4;
        // (a replayed rider is not bound by the set's clamp: it goes where its recording goes)
        fov_band_consts(e->knobs, step, std::max(cs.coord_bound + step * (double)(cs.n_ticks + 2), cs.replay.bound) + 1.0, ss.pc);
        if (road_over) {   // (the roundings of pack_road)
            ss.road_z = (float)(-road_F0[k / G]);
            ss.road_w = (float)(-0.5 * (road_sigma[k / G] + 1.0));
            ss.road_np = road_np_sigma(road_sigma[k / G]);
        }
    }
}

static int scene_eval_impl(csf_engine *e, int32_t n_sets, const csf_params *params, size_t params_size, int32_t abi_version, const double *road_F0,
                           const double *road_sigma, double *sums_out, int32_t stride, double *states_out) {
    if (int rc = scene_eval_check(e, n_sets, params, params_size, abi_version, road_F0, road_sigma, sums_out, stride)) return rc;
    SceneCalibState &cs = *e->scene_calib;
    const int32_t G = std::max(cs.groups.n, 1);
    const bool road_over = road_F0 != nullptr || road_sigma != nullptr;
    HIPCHK(e, hipSetDevice(e->device));
    int rc = upload_all(e);
    if (rc) return rc;
    if (road_over && (size_t)n_sets * (size_t)cs.road.stride > cs.road.blk.n) {
        HIPCHK(e, hipStreamSynchronize(e->main));
        const hipError_t r = cs.road.blk.alloc((size_t)n_sets * (size_t)cs.road.stride);
        if (r != hipSuccess) {
            cs.road.blk.release();
            return fail(e, CSF_E_DEVICE, "csf_scene_calib_eval_road: no memory for the roads of %d parameter sets: %s", (int)n_sets, hipGetErrorString(r));
        }
    }
    const int64_t n = (int64_t)n_sets * cs.R;
    const int64_t n_samples = states_out ? cs.n_ticks / stride : 0;
    const size_t n_states = (size_t)n_samples * (size_t)n * (size_t)e->d.ns;
    if (n_states > cs.states.n) {
        HIPCHK(e, hipStreamSynchronize(e->main));
        HIPCHK(e, cs.states.alloc(n_states));
    }
    SceneSet *const pin = cs.groups.held() ? cs.groups.pin->p : cs.sets_pin.p;
    SceneSet *const d_sets = cs.groups.held() ? cs.groups.sets.p : cs.sets.p;
    scene_compose_sets(e, cs, n_sets, params, road_F0, road_sigma, pin);
    // what the kernel is handed: the core's part, then every layer's
    SceneDev c{};
    c.obj = cs.obj.p, c.len = cs.len.p, c.roff = cs.roff.p;
    c.n_scn = cs.n_scn, c.n_ticks = (int32_t)cs.n_ticks, c.n_feat = cs.n_feat, c.R = cs.R;
    for (int k = 0; k < CALIB_MAX_FEAT; k++) c.feat[k] = cs.feat[k];
    c.img_cap = cs.R;
    c.sums = cs.sums.dev;
    c.states = n_states > 0 ? cs.states.p : nullptr;
    c.stride = states_out ? stride : 1;
    c.n_samples = (int32_t)n_samples;
    c.n_sets = n_sets;
    cs.image.fill(c);
    cs.replay.fill(c);
    cs.road.fill(c);
    if (road_over) c.road_blk = cs.road.blk.p;
    cs.windows.fill(c);
    if (cs.lanes.held()) {
        cs.lanes.fill(c);
        // a lane writes the sample rows of the rider it carries at the ticks that rider is present: every other row is NaN
        if (n_states > 0) HIPCHK(e, hipMemsetAsync(cs.states.p, 0xff, n_states * sizeof(double), e->main));
    }
    cs.groups.fill(c);
    // one copy of the table, one or two launches, one wait
    HIPCHK(e, hipMemcpyAsync(d_sets, pin, (size_t)n_sets * (size_t)G * sizeof(SceneSet), hipMemcpyHostToDevice, e->main));
    if (cs.groups.mixed() && cs.lanes.wide()) {   // (csf_scene_calib_lane_classes: scene_lanes_mixed_kernel, then scene_wide_mixed_kernel)
        SceneWideDev w{};
        cs.lanes.fill(w);
        cs.launches += launch_scene_mixed(cs.table.p, d_sets, c, e->d.ns, e->main, &w);
    } else if (cs.lanes.wide()) {   // the narrow scenes on scene_lanes_kernel, the wide ones on scene_wide_kernel: one stream, one wait
        SceneWideDev w{};
        cs.lanes.fill(w);
        cs.launches += launch_scene_eval(e->d.p.model, cs.table.p, d_sets, c, e->main, &w);
    } else if (cs.groups.mixed()) {   // several vehicle classes: scene_mixed_kernel (shared lanes: scene_lanes_mixed_kernel), the views' state width the widest of them
        cs.launches += launch_scene_mixed(cs.table.p, d_sets, c, e->d.ns, e->main);
    } else {
        cs.launches += launch_scene_eval(e->d.p.model, cs.table.p, d_sets, c, e->main);
    }
    HIPCHK(e, hipGetLastError());
    if (n_states > 0) HIPCHK(e, hipMemcpyAsync(states_out, cs.states.p, n_states * sizeof(double), hipMemcpyDeviceToHost, e->main));
    HIPCHK(e, hipStreamSynchronize(e->main));
    std::memcpy(sums_out, cs.sums.p, (size_t)n * sizeof(double2));
    // the slots hold the end of this evaluation (the read-backs show it); nothing of it enters the next one
    e->device_ahead = true;
    e->mid_synced = false;
    e->bounds_fresh = false;
    return CSF_OK;
}

int csf_scene_calib_eval_road(csf_engine *e, int32_t n_sets, const csf_params *params, size_t params_size, int32_t abi_version,
                              const double *road_F0, const double *road_sigma, double *sums_out, int32_t stride, double *states_out) try {
    if (!e) return CSF_E_ARG;
    if (e->scene_calib && e->scene_calib->groups.mixed())
        return fail(e, CSF_E_STATE, "csf_scene_calib_eval: the riders are in %d groups of several vehicle classes (csf_scene_calib_classes) and one set cannot say what group 1 carries: csf_scene_calib_eval_groups",
                    (int)e->scene_calib->groups.n);
    if (e->scene_calib && e->scene_calib->groups.held())
        return fail(e, CSF_E_STATE, "csf_scene_calib_eval: the riders are in %d groups (csf_scene_calib_groups / _lane_groups) and one set cannot say what group 1 carries: csf_scene_calib_eval_groups",
                    (int)e->scene_calib->groups.n);
    return scene_eval_impl(e, n_sets, params, params_size, abi_version, road_F0, road_sigma, sums_out, stride, states_out);
} catch (...) { return csf_caught(e); }

int csf_scene_calib_eval_groups(csf_engine *e, int32_t n_sets, int32_t n_groups, const csf_params *params, size_t params_size, int32_t abi_version,
                                const double *road_F0, const double *road_sigma, double *sums_out, int32_t stride, double *states_out) try {
    if (!e) return CSF_E_ARG;
    if (!e->scene_calib) return scene_none(e, "csf_scene_calib_eval_groups");
    const int32_t held = std::max(e->scene_calib->groups.n, 1);
    if (n_groups != held) return fail(e, CSF_E_ARG, "csf_scene_calib_eval_groups: %d groups, the data set holds %d (csf_scene_calib_groups)", (int)n_groups, (int)held);
    // (no groups loaded: one record per set, the call is csf_scene_calib_eval_road)
    return scene_eval_impl(e, n_sets, params, params_size, abi_version, road_F0, road_sigma, sums_out, stride, states_out);
} catch (...) { return csf_caught(e); }

// what the three calls that load groups share: "rider r is in group g of n" ...
static int scene_check_groups(csf_engine *e, const char *fn, const SceneCalibState &cs, const uint8_t *group, int32_t n_groups) {
    for (int32_t r = 0; r < cs.R; r++)
        if (group[r] >= n_groups) return fail(e, CSF_E_ARG, "%s: rider %d is in group %d of %d", fn, (int)r, (int)group[r], (int)n_groups);
    return CSF_OK;
}

// ... and the staging of group / sets / pin in a fresh layer
static hipError_t scene_stage_groups(const SceneCalibState &cs, const uint8_t *group, int32_t n_groups, SceneGroups &g) {
    const size_t recs = (size_t)cs.max_sets * (size_t)n_groups;
    g.pin.reset(new HostBuf<SceneSet, false>());
    hipError_t r = g.group.upload(group, (size_t)cs.R);
    if (r == hipSuccess) r = g.sets.alloc(recs);
    if (r == hipSuccess) r = g.pin->alloc(recs);
    if (r != hipSuccess) return r;
    std::memset(g.pin->p, 0, recs * sizeof(SceneSet));
    g.n = n_groups;
    return hipSuccess;
}

// csf_scene_calib_groups (lanes == false: a csf_scene_calib_load data set, one slot per rider) and csf_scene_calib_lane_groups (lanes ==
// true: a data set of csf_scene_calib_load_shared / _load_wide, the group goes with the rider a lane carries).  `fn` names the call in
// the messages
static int scene_groups_impl(csf_engine *e, const char *fn, bool lanes, const uint8_t *group, int32_t n_groups) {
    if (!e->scene_calib) return scene_none(e, fn, "whose candidate sets are whole populations already");
    SceneCalibState &cs = *e->scene_calib;
    if (!lanes && cs.lanes.held())
        return fail(e, CSF_E_STATE, "csf_scene_calib_groups: the data set shares its lanes (csf_scene_calib_load_shared / _load_wide): a lane's parameters would change with its rider; groups need csf_scene_calib_load, or csf_scene_calib_lane_groups on this data set");
    if (lanes && !cs.lanes.held())
        return fail(e, CSF_E_STATE, "csf_scene_calib_lane_groups: the data set has one slot per rider (csf_scene_calib_load): its groups are loaded by csf_scene_calib_groups");
    const bool drop = group == nullptr || n_groups <= 1;
    if (!drop) {
        if (n_groups > SCENE_GROUPS_MAX) return fail(e, CSF_E_ARG, "%s: %d groups (at most %d)", fn, (int)n_groups, SCENE_GROUPS_MAX);
        if (int rc = scene_check_groups(e, fn, cs, group, n_groups)) return rc;
    }
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->main));
    SceneGroups fresh;
    if (!drop) {
        const hipError_t r = scene_stage_groups(cs, group, n_groups, fresh);
        if (r != hipSuccess) return fail(e, CSF_E_DEVICE, "%s: no memory for the groups: %s", fn, hipGetErrorString(r));
    }
    scene_drop_classes(e, cs);                                 // (these groups replace the classes of csf_scene_calib_classes)
    cs.groups = std::move(fresh);
    return CSF_OK;
}

// csf_scene_calib_classes (lanes == false: a csf_scene_calib_load data set, one slot per rider) and csf_scene_calib_lane_classes (lanes ==
// true: a data set of csf_scene_calib_load_shared / _load_wide, the class goes with the rider a lane carries; DESIGN.md 4.10j).  `fn` names
// the call in the messages
static int scene_classes_impl(csf_engine *e, const char *fn, bool lanes, const uint8_t *group, int32_t n_groups, const int32_t *models,
                              const double *s0) {
    if (!e->scene_calib) return scene_none(e, fn, "whose candidate sets are whole populations already");
    SceneCalibState &cs = *e->scene_calib;
    if (!lanes && cs.lanes.held())
        return fail(e, CSF_E_STATE, "%s: the data set shares its lanes (csf_scene_calib_load_shared / _load_wide): mixed classes need csf_scene_calib_load - one slot per rider, at most %d riders per scene", fn, SMALL_MAX);
    if (lanes && !cs.lanes.held())
        return fail(e, CSF_E_STATE, "%s: the data set has one slot per rider (csf_scene_calib_load): its classes are loaded by csf_scene_calib_classes", fn);
    const bool drop = group == nullptr && n_groups == 0 && models == nullptr && s0 == nullptr;
    HIPCHK(e, hipSetDevice(e->device));
    if (drop) {                                                // the data set is what it was after the load (groups of either call go)
        HIPCHK(e, hipStreamSynchronize(e->main));
        scene_drop_classes(e, cs);
        cs.groups = SceneGroups();
        return CSF_OK;
    }
    if (n_groups < 2 || n_groups > SCENE_CLASS_GROUPS_MAX) return fail(e, CSF_E_ARG, "%s: %d groups (2 .. %d)", fn, (int)n_groups, SCENE_CLASS_GROUPS_MAX);
    if (!group || !models) return fail(e, CSF_E_ARG, "%s: NULL array", fn);
    if (!s0) return fail(e, CSF_E_ARG, "%s: s0 is NULL: the start states in the widest layout, [R][%d]", fn, STATE_ROWS);
    for (int32_t g = 0; g < n_groups; g++)
        if (models[g] < 0 || models[g] > CSF_BALANCINGRIDER || models[g] == CSF_UNCONTROLLED)
            return fail(e, CSF_E_ARG, "%s: group %d is of vehicle class %d: not one of the six simulated classes", fn, (int)g, (int)models[g]);
    if (int rc = scene_check_groups(e, fn, cs, group, n_groups)) return rc;
    // the image per rider and class: what csf_add_agents and side_state make of a fresh vehicle of that class (vehicle.py:64-204, 1728-1736;
    // dynamics.py:306-307, 350-371 for the BalancingRider's mirrored layout).  zrid and dgood follow in the kernel from the rider's own record
    const size_t Rs = (size_t)cs.R;
    std::vector<double> is(STATE_ROWS * Rs, 0.0), il(5 * Rs, 0.0), ip(Rs, 0.0), hx(Rs), hy(Rs);
    int32_t ns = 0;
    for (int32_t g = 0; g < n_groups; g++) ns = std::max(ns, (int32_t)NS_OF[models[g]]);
    for (size_t r = 0; r < Rs; r++) {
        const int m = models[group[r]];
        const double *s = s0 + r * STATE_ROWS;
        double v[STATE_ROWS];
        for (int c = 0; c < STATE_ROWS; c++) v[c] = c < NS_OF[m] ? s[c] : 0.0;
        v[2] = limit_angle_h(s[2]);                            // vehicle.py:154-155
        for (int c = 0; c < STATE_ROWS; c++) is[(size_t)c * Rs + r] = v[c];
        hx[r] = s[0], hy[r] = s[1];                            // traj[:, 0] = s  (vehicle.py:159-160)
        if (m == CSF_BALANCINGRIDER) {
            il[0 * Rs + r] = v[5], il[1 * Rs + r] = -v[4], il[2 * Rs + r] = v[7], il[3 * Rs + r] = -v[6], il[4 * Rs + r] = -v[2];
            ip[r] = v[3];
        } else {
            il[0 * Rs + r] = v[4], il[2 * Rs + r] = v[5], il[4 * Rs + r] = v[2];
            ip[r] = v[2];
        }
    }
    HIPCHK(e, hipStreamSynchronize(e->main));
    SceneGroups fresh;
    hipError_t r = scene_stage_groups(cs, group, n_groups, fresh);
    if (r == hipSuccess) r = fresh.cimg_s.upload(is);
    if (r == hipSuccess) r = fresh.cimg_lti.upload(il);
    if (r == hipSuccess) r = fresh.cimg_ppsi.upload(ip);
    if (r == hipSuccess) r = fresh.cimg_hx0.upload(hx);
    if (r == hipSuccess) r = fresh.cimg_hy0.upload(hy);
    if (r != hipSuccess) return fail(e, CSF_E_DEVICE, "%s: no memory for the classes: %s", fn, hipGetErrorString(r));
    fresh.class_models.assign(models, models + n_groups);
    fresh.ns_own = cs.groups.mixed() ? cs.groups.ns_own : e->d.ns;
    scene_drop_classes(e, cs);
    cs.groups = std::move(fresh);
    e->d.ns = ns;                                              // csf_num_states: the widest class while the classes are held
    return CSF_OK;
}

int csf_scene_calib_classes(csf_engine *e, const uint8_t *group, int32_t n_groups, const int32_t *models, const double *s0) try {
    if (!e) return CSF_E_ARG;
    return scene_classes_impl(e, "csf_scene_calib_classes", false, group, n_groups, models, s0);
} catch (...) { return csf_caught(e); }

int csf_scene_calib_lane_classes(csf_engine *e, const uint8_t *group, int32_t n_groups, const int32_t *models, const double *s0) try {
    if (!e) return CSF_E_ARG;
    return scene_classes_impl(e, "csf_scene_calib_lane_classes", true, group, n_groups, models, s0);
} catch (...) { return csf_caught(e); }

int csf_scene_calib_groups(csf_engine *e, const uint8_t *group, int32_t n_groups) try {
    if (!e) return CSF_E_ARG;
    return scene_groups_impl(e, "csf_scene_calib_groups", false, group, n_groups);
} catch (...) { return csf_caught(e); }

int csf_scene_calib_lane_groups(csf_engine *e, const uint8_t *group, int32_t n_groups) try {
    if (!e) return CSF_E_ARG;
    return scene_groups_impl(e, "csf_scene_calib_lane_groups", true, group, n_groups);
} catch (...) { return csf_caught(e); }

int csf_scene_calib_road(csf_engine *e, int32_t n_edges, const int32_t *edge_scene, const int64_t *offsets, const double *xy, const double *F0,
                         const double *sigma) try {
    if (!e) return CSF_E_ARG;
    if (!e->scene_calib) return scene_none(e, "csf_scene_calib_road", "whose vehicles are not coupled and feel no road");
    SceneCalibState &cs = *e->scene_calib;
    if (n_edges < 0) return fail(e, CSF_E_ARG, "csf_scene_calib_road: n_edges must be >= 0");
    if (n_edges > 0 && (!edge_scene || !offsets || !xy || !F0 || !sigma)) return fail(e, CSF_E_ARG, "csf_scene_calib_road: NULL array");
    for (int32_t k = 0; k < n_edges; k++) {
        if (edge_scene[k] < 0 || edge_scene[k] >= cs.n_scn) return fail(e, CSF_E_ARG, "csf_scene_calib_road: edge %d names scene %d, the data set has %d", (int)k, (int)edge_scene[k], (int)cs.n_scn);
        if (k > 0 && edge_scene[k] < edge_scene[k - 1]) return fail(e, CSF_E_ARG, "csf_scene_calib_road: edge_scene[%d .. %d] decreases", (int)k - 1, (int)k);
        if (offsets[k] < 0 || offsets[k + 1] < offsets[k]) return fail(e, CSF_E_ARG, "csf_scene_calib_road: offsets[%d .. %d] run backwards", (int)k, (int)k + 1);
        if (!std::isfinite(F0[k]) || !std::isfinite(sigma[k])) return fail(e, CSF_E_ARG, "csf_scene_calib_road: F0 or sigma of edge %d is not finite", (int)k);
        for (int64_t v = offsets[k]; v < offsets[k + 1]; v++)
            if (!std::isfinite(xy[2 * v]) || !std::isfinite(xy[2 * v + 1])) return fail(e, CSF_E_ARG, "csf_scene_calib_road: vertex %lld of edge %d is not finite", (long long)v, (int)k);
    }
    // the road of every scene as csf_set_road_vertices keeps it - rows (x, y, F0, sigma), the edges one after the other - held to what
    // the one-wave tick stages (tick.inc: small_road_ok) and packed as upload_all packs the road of an engine that holds the scene
    const size_t n_scn = (size_t)cs.n_scn;
    std::vector<int64_t> nv(n_scn, 0), at(n_scn, 0), tile_at(n_scn, 0);
    std::vector<int32_t> np(n_scn, 0);
    std::vector<float4> rv_all;
    std::vector<float2> rvo_all;
    int64_t max_pad = 0;
    {
        std::vector<double> road;
        std::vector<float4> rv;
        std::vector<float2> rvo;
        int32_t k = 0;
        for (size_t q = 0; q < n_scn; q++) {
            road.clear();
            for (; k < n_edges && (size_t)edge_scene[k] == q; k++)
                for (int64_t v = offsets[k]; v < offsets[k + 1]; v++) {
                    road.push_back(xy[2 * v]);
                    road.push_back(xy[2 * v + 1]);
                    road.push_back(F0[k]);
                    road.push_back(sigma[k]);
                    if (road.size() / 4 > (size_t)SMALL_ROAD_MAX)
                        return fail(e, CSF_E_ARG, "csf_scene_calib_road: the road of scene %d has more than %d vertices", (int)q, SMALL_ROAD_MAX);
                }
            nv[q] = (int64_t)road.size() / 4;
            // (shared lanes: the one-wave tick runs the scene's lanes, not its roster)
            const int64_t nv_pad = (nv[q] + 63) / 64 * 64, n = cs.lanes.held() ? cs.lanes.h_nl[q] : cs.h_roff[q + 1] - cs.h_roff[q];
            int64_t P = cs.lanes.is_wide(q) ? WAVE : 1;        // (a wide scene: the workgroup's P is 64, 128 or 256)
            while (P < n) P <<= 1;
            if (nv_pad * P > 256 * WAVE)
                return fail(e, CSF_E_ARG, "csf_scene_calib_road: the road of scene %d has %lld vertices, a scene of %lld road users takes %lld", (int)q,
                            (long long)nv[q], (long long)n, (long long)(256 * WAVE / P));
            at[q] = (int64_t)rv_all.size(), tile_at[q] = (int64_t)rvo_all.size();
            np[q] = pack_road(road.data(), nv[q], cs.h_ox[q], cs.h_oy[q], rv, rvo);
            rv_all.insert(rv_all.end(), rv.begin(), rv.end());
            rvo_all.insert(rvo_all.end(), rvo.begin(), rvo.end());
            max_pad = std::max(max_pad, nv_pad);
        }
    }
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->main));
    // a fresh road, and the views that point into it
    SceneRoad fresh;
    DevBuf<Dev> d_table, d_table_w;
    std::vector<Dev> tab = cs.h_table;
    hipError_t r = fresh.rv.upload(rv_all);
    if (r == hipSuccess) r = fresh.rvo.upload(rvo_all);
    if (r == hipSuccess) {
        for (int32_t k = 0; k < cs.max_sets; k++)
            for (size_t q = 0; q < n_scn; q++) {
                if (nv[q] == 0) continue;
                Dev &v = tab[(size_t)k * n_scn + q];
                v.nv = nv[q], v.nv_pad = (nv[q] + 63) / 64 * 64;
                v.rv = fresh.rv.p + at[q], v.rvo = fresh.rvo.p + tile_at[q];
                v.road_np = np[q];
                v.ox = cs.h_ox[q], v.oy = cs.h_oy[q];
                v.rg_nx = v.rg_ny = 0;
            }
        r = scene_upload_tables(cs, tab, d_table, d_table_w);
    }
    if (r == hipSuccess) r = hipDeviceSynchronize();
    if (r != hipSuccess) return fail(e, CSF_E_DEVICE, "csf_scene_calib_road: no memory for the roads: %s", hipGetErrorString(r));
    fresh.stride = (int64_t)rv_all.size();
    fresh.max_pad = (int32_t)max_pad;
    cs.table = std::move(d_table);
    cs.lanes.table_w = std::move(d_table_w);
    cs.road = std::move(fresh);
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_scene_calib_replay(csf_engine *e, const uint8_t *replayed, const double *rows) try {
    if (!e) return CSF_E_ARG;
    if (!e->scene_calib) return scene_none(e, "csf_scene_calib_replay");
    SceneCalibState &cs = *e->scene_calib;
    const int32_t R = cs.R;
    std::vector<int32_t> index((size_t)R, -1);
    SceneReplay fresh;
    for (int32_t r = 0; replayed && r < R; r++)
        if (replayed[r]) index[(size_t)r] = fresh.n++;
    const int32_t n_rep = fresh.n;
    if (n_rep > 0 && !rows) return fail(e, CSF_E_ARG, "csf_scene_calib_replay: %d riders are replayed and rows is NULL", (int)n_rep);
    // the rows a tick reads - t < the length of the rider's scene - are finite; the largest coordinate among them sizes the bands
    for (int32_t q = 0; n_rep > 0 && q < cs.n_scn; q++)
        for (int32_t r = cs.h_roff[(size_t)q]; r < cs.h_roff[(size_t)q + 1]; r++) {
            const int32_t k = index[(size_t)r];
            if (k < 0) continue;
            for (int64_t t = 0; t < cs.h_len[(size_t)q]; t++) {
                const double *v = rows + ((size_t)t * (size_t)n_rep + (size_t)k) * 4;
                if (!(std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]) && std::isfinite(v[3])))
                    return fail(e, CSF_E_ARG, "csf_scene_calib_replay: the recorded state of rider %d after tick %lld is not finite", (int)r, (long long)t);
                fresh.bound = std::max({fresh.bound, std::fabs(v[0] - e->d.ox), std::fabs(v[1] - e->d.oy)});
            }
        }
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->main));
    if (n_rep > 0) {
        hipError_t r = fresh.index.upload(index);
        if (r == hipSuccess) r = fresh.rows.upload(rows, (size_t)cs.n_ticks * (size_t)n_rep * 4);
        if (r != hipSuccess) return fail(e, CSF_E_DEVICE, "csf_scene_calib_replay: no memory for the recorded states: %s", hipGetErrorString(r));
    }
    cs.replay = std::move(fresh);
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_scene_calib_windows(csf_engine *e, const int32_t *enter, const int32_t *exit) try {
    if (!e) return CSF_E_ARG;
    if (!e->scene_calib) return scene_none(e, "csf_scene_calib_windows", "whose samples are single vehicles that are there throughout");
    SceneCalibState &cs = *e->scene_calib;
    if (cs.lanes.held()) return fail(e, CSF_E_STATE, "csf_scene_calib_windows: the data set shares its lanes: the windows came with csf_scene_calib_load_shared and decide who sits where");
    if ((enter == nullptr) != (exit == nullptr)) return fail(e, CSF_E_ARG, "csf_scene_calib_windows: enter and exit are given together or not at all");
    for (int32_t q = 0; enter && q < cs.n_scn; q++)
        for (int32_t r = cs.h_roff[(size_t)q]; r < cs.h_roff[(size_t)q + 1]; r++)
            if (enter[r] < 0 || enter[r] > exit[r] || exit[r] > cs.h_len[(size_t)q])
                return fail(e, CSF_E_ARG, "csf_scene_calib_windows: rider %d has the window [%d, %d), scene %d has %d ticks (0 <= enter <= exit <= ticks)",
                            (int)r, (int)enter[r], (int)exit[r], (int)q, (int)cs.h_len[(size_t)q]);
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->main));
    SceneWindows fresh;
    if (enter) {
        hipError_t r = fresh.enter.upload(enter, (size_t)cs.R);
        if (r == hipSuccess) r = fresh.exit.upload(exit, (size_t)cs.R);
        if (r != hipSuccess) return fail(e, CSF_E_DEVICE, "csf_scene_calib_windows: no memory for the windows: %s", hipGetErrorString(r));
    }
    cs.windows = std::move(fresh);
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_scene_calib_launches(const csf_engine *e, int64_t *n_launches) try {
    if (!e || !n_launches) return CSF_E_ARG;
    if (!e->scene_calib) return CSF_E_STATE;       // (no data set; no message is written: the call changes nothing)
    *n_launches = e->scene_calib->launches;
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_scene_calib_clear(csf_engine *e) try {
    if (!e) return CSF_E_ARG;
    if (!e->scene_calib) return fail(e, CSF_E_STATE, "csf_scene_calib_clear: no closed-loop data set");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->main));
    // The removal goes through the host mirror, which closes the holes (compact_host): patched on the device it would leave
    // max_sets x R dead slots behind, and a small population added next would find d.n > n_live and miss the one-wave tick.
    // What can fail - the download into the mirror - comes first, with the data set still held: a refused call changes nothing.
    int rc = prepare_mutation(e, true);
    if (rc) return rc;
    std::shared_ptr<SceneCalibState> cs = std::move(e->scene_calib);   // (csf_remove_agents takes the engine again)
    e->scene_calib.reset();
    rc = remove_everybody(e);
    if (rc) e->scene_calib = std::move(cs);                            // (refused before it touched the mirror: the data set stays)
    else scene_drop_classes(e, *cs);                                   // (csf_scene_calib_classes: the state width is the engine's own again)
    return rc;                                                         // the buffers go with cs
} catch (...) { return csf_caught(e); }
