// engine/abi_scene.inc - C ABI: calibration on closed-loop scenes.  A data set of small scenes resident on the device, workgroup = (parameter set, scene), the error against the recorded trajectories summed in the launch.
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)
//
// csf_calib_eval (engine/abi_calib.inc) replays recorded forces, which couples no two vehicles: the parameters of the social-force
// field cannot be fitted with it.  Here every candidate set simulates every scene of the data set with its riders together - the
// one-wave tick of csf_step for up to 32 road users (csf_small_body.inc) - and the kernel sums the error against the recorded
// trajectories per rider (csf_scene.hip: scene_eval_kernel).  One copy of the call's table of sets, one launch, one wait per call.

extern "C++" {

struct SceneCalibState {
    int32_t n_scn = 0, n_feat = 0, max_sets = 0, R = 0;
    int64_t n_ticks = 0;
    int32_t feat[CALIB_MAX_FEAT] = {0, 0, 0, 0, 0, 0};
    double coord_bound = 0.0;                // largest |coordinate| of a start position, relative to the scene origin
    DevBuf<double> obj, img_s, img_lti, img_ppsi, img_znp, img_hx0, img_hy0, states;
    DevBuf<int32_t> len, roff, img_ti, img_ptr;
    DevBuf<uint32_t> img_status;
    DevBuf<uint8_t> img_znav;
    DevBuf<Dev> table;                       // [max_sets][n_scn] the views of the slot blocks, built once
    DevBuf<SceneSet> sets;                   // [max_sets] the call's candidate sets ...
    HostBuf<SceneSet, false> sets_pin;       // ... and where the host composes them: one copy per call
    HostBuf<double2> sums;                   // [max_sets * R] written by the kernel (mapped)
    int64_t launches = 0;                    // csf_scene_calib_launches
    // csf_scene_calib_replay: the riders that follow their recording (csf_scene.h).  n_rep == 0: none, and an evaluation is
    // handed rep == NULL - the kernel's path without a replay
    std::vector<int32_t> h_len, h_roff;      // the scenes' lengths and first riders, as on the device
    DevBuf<int32_t> rep_index;               // [R]
    DevBuf<double> rep;                      // [n_ticks][n_rep][4]
    int32_t n_rep = 0;
    double rep_bound = 0.0;                  // largest |coordinate| of a replayed row, relative to the scene origin
    // csf_scene_calib_road: a road per scene, shared by all candidate sets (DESIGN.md 4.10c).  road_stride == 0: no scene has one,
    // every view has nv = nv_pad = 0 and a launch asks for no dynamic LDS
    std::vector<Dev> h_table;                // the table as csf_scene_calib_load built it: no roads, the engine's origin
    std::vector<double> h_ox, h_oy;          // [n_scn] the origin a stand-alone engine that holds the scene would have (mirror.inc)
    DevBuf<float4> road_rv;                  // [road_stride] the packed roads of the scenes, one after the other
    DevBuf<float2> road_rvo;                 // their tile origins
    DevBuf<float4> road_blk;                 // [sets][road_stride] the roads as a candidate set's parameters make them: allocated by
                                             // the first evaluation that overrides them
    int64_t road_stride = 0;
    int32_t road_max_pad = 0;                // largest nv_pad of a scene
    // csf_scene_calib_windows: a presence window per rider (DESIGN.md 4.10d).  Empty buffers: no windows, and an evaluation is
    // handed win_enter == NULL - the kernel instance without a mask
    DevBuf<int32_t> win_enter, win_exit;     // [R]
    // csf_scene_calib_load_shared: rosters that share the lanes of their scene (DESIGN.md 4.10e).  Lsum == 0: not shared - slot =
    // set * R + rider.  Else slot = set * Lsum + lane_off[scene] + lane, the windows above came with the load, and the image holds
    // what was constant per slot before: the desired speed and the destination queue of every rider
    int32_t Lsum = 0;
    std::vector<int32_t> h_nl;               // [n_scn] lanes of every scene
    DevBuf<int32_t> lane_off, lane_first, rider_next, img_qlen;   // [n_scn + 1], [Lsum], [R], [R]
    DevBuf<int64_t> img_qbeg;                // [R]
    DevBuf<double> img_vdes;                 // [R]
    // csf_scene_calib_load_wide: scenes with up to WIDE_MAX lanes (DESIGN.md 4.10f).  wide_from == 0: not such a load.  Else the scenes
    // with n_lanes >= wide_from are WIDE - scn_w, their views in table_w - and `table` holds the views of the narrow scenes alone, with
    // the compacted lengths, first riders and lane offsets scene_lanes_kernel reads (csf_scene.h: SceneWideDev)
    int32_t wide_from = 0;
    std::vector<int32_t> h_scn_w, h_scn_n;   // the wide scenes and the narrow ones, ascending
    DevBuf<Dev> table_w;                     // [max_sets][n_wide]
    DevBuf<int32_t> scn_w, len_n, roff_n, lane_off_n;
    bool is_wide(size_t q) const { return wide_from > 0 && h_nl[q] >= wide_from; }
    // csf_scene_calib_groups, and on shared lanes csf_scene_calib_lane_groups (DESIGN.md 4.10g, 4.10h): rider groups with parameter sets of their own.  n_groups == 0: none, an evaluation is
    // handed group == NULL and launches what it launched before.  Else the call's table is [n_sets][n_groups] records in sets_g
    int32_t n_groups = 0;
    DevBuf<uint8_t> group;                   // [R]
    DevBuf<SceneSet> sets_g;                 // [max_sets][n_groups]
    std::unique_ptr<HostBuf<SceneSet, false>> sets_g_pin;
    // csf_scene_calib_classes (DESIGN.md 4.10i): the groups are of different vehicle classes.  Empty: none.  Else n_groups, group, sets_g are
    // those of this call, class_models [n_groups] the class of every group, the engine's state width (Dev::ns, csf_num_states) is the widest
    // of them while they are held - ns_own is what it was -, and an evaluation restores from cimg_*: the image's state rows, side state and
    // first ring row as a fresh vehicle of the rider's OWN class has them (abi_population.inc: add_agents_impl, side_state)
    std::vector<int32_t> class_models;
    int32_t ns_own = 0;
    DevBuf<double> cimg_s, cimg_lti, cimg_ppsi, cimg_hx0, cimg_hy0;
    bool mixed() const { return !class_models.empty(); }
};

// the classes of csf_scene_calib_classes go: the state width is the engine's own again, the image the load's
static void scene_drop_classes(csf_engine *e, SceneCalibState &cs) {
    if (!cs.mixed()) return;
    e->d.ns = cs.ns_own;
    cs.class_models.clear();
    cs.cimg_s = DevBuf<double>(), cs.cimg_lti = DevBuf<double>(), cs.cimg_ppsi = DevBuf<double>();
    cs.cimg_hx0 = DevBuf<double>(), cs.cimg_hy0 = DevBuf<double>();
}

// The views on the device from the whole table [max_sets][n_scn] on the host: all of it in `table`, or - a wide load - the narrow
// scenes' in `table` and the wide scenes' in `table_w`, both [max_sets][their scenes].  Allocates; the caller waits for the device.
static hipError_t scene_upload_tables(const SceneCalibState &cs, const std::vector<Dev> &tab, DevBuf<Dev> &table, DevBuf<Dev> &table_w) {
    const size_t n_scn = (size_t)cs.n_scn, sets = (size_t)cs.max_sets;
    if (cs.wide_from == 0) {
        hipError_t r = table.alloc(tab.size());
        if (r == hipSuccess) r = hipMemcpy(table.p, tab.data(), tab.size() * sizeof(Dev), hipMemcpyHostToDevice);
        return r;
    }
    hipError_t r = hipSuccess;
    const std::vector<int32_t> *part[2] = {&cs.h_scn_n, &cs.h_scn_w};
    DevBuf<Dev> *dst[2] = {&table, &table_w};
    for (int w = 0; w < 2 && r == hipSuccess; w++) {
        const size_t m = part[w]->size();
        std::vector<Dev> sub;
        sub.reserve(sets * m);
        for (size_t k = 0; k < sets; k++)
            for (size_t j = 0; j < m; j++) sub.push_back(tab[k * n_scn + (size_t)(*part[w])[j]]);
        r = dst[w]->alloc(sub.size());
        if (r == hipSuccess && !sub.empty()) r = hipMemcpy(dst[w]->p, sub.data(), sub.size() * sizeof(Dev), hipMemcpyHostToDevice);
    }
    return r;
}

}  // extern "C++"

// csf_scene_calib_load (n_lanes == NULL), csf_scene_calib_load_shared and csf_scene_calib_load_wide: `fn` names the call in the messages,
// lane_max is the most lanes a scene may have, wide_from == 0 no wide load (else: scenes with n_lanes >= wide_from are wide)
static int scene_load_impl(csf_engine *e, const char *fn, int32_t n_scn, const int32_t *n_riders, const int32_t *n_lanes, const int32_t *lane,
                           const int32_t *enter, const int32_t *exit, int64_t n_ticks, const double *s0, const double *v_desired,
                           const int64_t *dest_offsets, const double *dest_xyz_stop, const int32_t *lengths, const double *objective,
                           int32_t n_feat, const int32_t *feat, int32_t max_sets, int32_t lane_max = SMALL_MAX, int32_t wide_from = 0) {
    const bool sh = n_lanes != nullptr;
    if (!n_riders || !s0 || !v_desired || !dest_offsets || !dest_xyz_stop || !objective || !feat) return fail(e, CSF_E_ARG, "%s: NULL array", fn);
    if (sh && (!lane || !enter || !exit)) return fail(e, CSF_E_ARG, "%s: NULL array", fn);
    if (n_scn < 1 || n_scn > (1 << 20) || n_ticks < 1 || n_ticks > 2000000000 || n_feat < 1 || n_feat > CALIB_MAX_FEAT || max_sets < 1 || max_sets > 256)
        return fail(e, CSF_E_ARG, "%s: 1 <= n_scn <= 2^20, 1 <= n_ticks <= 2e9, 1 <= n_feat <= %d, 1 <= max_sets <= 256", fn, CALIB_MAX_FEAT);
    if (e->scene_calib) return fail(e, CSF_E_STATE, "%s: the engine holds a closed-loop data set already (csf_scene_calib_clear first)", fn);
    if (e->calib) return fail(e, CSF_E_STATE, "%s: the engine holds a calibration data set (csf_calib_clear first)", fn);
    if (!e->order.empty()) return fail(e, CSF_E_STATE, "%s: the engine is not empty (%lld road users)", fn, (long long)e->order.size());
    if (e->batch) return fail(e, CSF_E_STATE, "%s: the engine belongs to a batch (csf_batch_leave first)", fn);
    if (e->loopback) return fail(e, CSF_E_STATE, "%s: the engine is a member of a loopback group", fn);
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
    // shared lanes: every rider's lane and window, and the occupants of a lane one after the other.  The chain of a lane holds its
    // riders with a non-empty window in entry order; a rider that is never present sits on no lane (its lane is checked all the same)
    std::vector<int32_t> lo, lfirst, rnext;
    if (sh) {
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
    }
    HIPCHK(e, hipSetDevice(e->device));
    // everything that can fail first: a refused call changes nothing
    auto cs = std::make_shared<SceneCalibState>();
    cs->Lsum = Lsum;
    cs->wide_from = sh ? wide_from : 0;
    if (sh) cs->h_nl.assign(n_lanes, n_lanes + n_scn);
    for (int32_t q = 0; cs->wide_from > 0 && q < n_scn; q++) (cs->is_wide((size_t)q) ? cs->h_scn_w : cs->h_scn_n).push_back(q);
    cs->n_scn = n_scn, cs->n_feat = n_feat, cs->max_sets = max_sets, cs->n_ticks = n_ticks, cs->R = R;
    for (int32_t k = 0; k < n_feat; k++) cs->feat[k] = feat[k];
    const size_t Rs = (size_t)R, tn = (size_t)n_ticks * Rs * (size_t)n_feat, views = (size_t)max_sets * (size_t)n_scn;
    hipError_t r = cs->obj.alloc(tn);
    if (r == hipSuccess) r = cs->img_s.alloc(STATE_ROWS * Rs);
    if (r == hipSuccess) r = cs->img_lti.alloc(5 * Rs);
    if (r == hipSuccess) r = cs->img_ppsi.alloc(Rs);
    if (r == hipSuccess) r = cs->img_znp.alloc(3 * Rs);
    if (r == hipSuccess) r = cs->img_hx0.alloc(Rs);
    if (r == hipSuccess) r = cs->img_hy0.alloc(Rs);
    if (r == hipSuccess) r = cs->img_ti.alloc(Rs);
    if (r == hipSuccess) r = cs->img_ptr.alloc(Rs);
    if (r == hipSuccess) r = cs->img_status.alloc(Rs);
    if (r == hipSuccess) r = cs->img_znav.alloc(Rs);
    if (r == hipSuccess) r = cs->len.alloc((size_t)n_scn);
    if (r == hipSuccess) r = cs->roff.alloc((size_t)n_scn + 1);
    // (the table itself is allocated where it is filled: scene_upload_tables)
    if (r == hipSuccess) r = cs->sets.alloc((size_t)max_sets);
    if (r == hipSuccess) r = cs->sets_pin.alloc((size_t)max_sets);
    if (r == hipSuccess) r = cs->sums.alloc((size_t)max_sets * Rs);
    if (sh) {
        if (r == hipSuccess) r = cs->lane_off.alloc((size_t)n_scn + 1);
        if (r == hipSuccess) r = cs->lane_first.alloc((size_t)Lsum);
        if (r == hipSuccess) r = cs->rider_next.alloc(Rs);
        if (r == hipSuccess) r = cs->win_enter.alloc(Rs);
        if (r == hipSuccess) r = cs->win_exit.alloc(Rs);
        if (r == hipSuccess) r = cs->img_vdes.alloc(Rs);
        if (r == hipSuccess) r = cs->img_qbeg.alloc(Rs);
        if (r == hipSuccess) r = cs->img_qlen.alloc(Rs);
    }
    if (cs->wide_from > 0) {
        if (r == hipSuccess) r = cs->scn_w.alloc(cs->h_scn_w.size());
        if (r == hipSuccess) r = cs->len_n.alloc(cs->h_scn_n.size());
        if (r == hipSuccess) r = cs->roff_n.alloc(cs->h_scn_n.size() + 1);
        if (r == hipSuccess) r = cs->lane_off_n.alloc(cs->h_scn_n.size());
    }
    if (r != hipSuccess) return fail(e, CSF_E_DEVICE, "%s: no memory for the data set: %s", fn, hipGetErrorString(r));
    std::memset(cs->sets_pin.p, 0, (size_t)max_sets * sizeof(SceneSet));
    std::vector<int32_t> ls((size_t)n_scn), ro((size_t)n_scn + 1, 0);
    for (int32_t q = 0; q < n_scn; q++) ls[(size_t)q] = lengths ? lengths[q] : (int32_t)n_ticks, ro[(size_t)q + 1] = ro[(size_t)q] + n_riders[q];
    HIPCHK(e, hipMemcpy(cs->obj.p, objective, tn * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(cs->len.p, ls.data(), ls.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(cs->roff.p, ro.data(), ro.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (sh) {
        HIPCHK(e, hipMemcpy(cs->lane_off.p, lo.data(), lo.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(e, hipMemcpy(cs->lane_first.p, lfirst.data(), lfirst.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(e, hipMemcpy(cs->rider_next.p, rnext.data(), rnext.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(e, hipMemcpy(cs->win_enter.p, enter, Rs * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(e, hipMemcpy(cs->win_exit.p, exit, Rs * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    if (cs->wide_from > 0) {   // what scene_lanes_kernel reads per scene, for the narrow scenes alone (csf_scene.h: SceneWideDev)
        const size_t m = cs->h_scn_n.size();
        std::vector<int32_t> ln(m), rn(m + 1, R), on(m);
        for (size_t j = 0; j < m; j++) {
            const size_t q = (size_t)cs->h_scn_n[j];
            ln[j] = ls[q], rn[j] = ro[q], on[j] = lo[q];
        }
        if (m > 0) {
            rn[m] = ro[(size_t)cs->h_scn_n[m - 1] + 1];
            HIPCHK(e, hipMemcpy(cs->len_n.p, ln.data(), m * sizeof(int32_t), hipMemcpyHostToDevice));
            HIPCHK(e, hipMemcpy(cs->lane_off_n.p, on.data(), m * sizeof(int32_t), hipMemcpyHostToDevice));
        }
        HIPCHK(e, hipMemcpy(cs->roff_n.p, rn.data(), rn.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        if (!cs->h_scn_w.empty()) HIPCHK(e, hipMemcpy(cs->scn_w.p, cs->h_scn_w.data(), cs->h_scn_w.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    // the max_sets x R vehicles, slot set * R + rider: every set starts every scene from the scene's start states, with its queues
    const int ns = e->d.ns;
    const int64_t q0 = dest_offsets[0], q_rows = dest_offsets[R] - q0;
    // (shared lanes: the R riders once, then copies of rider 0 with the first row of its queue up to the slots that are run)
    const int64_t q_all = sh ? q_rows + (n - R) : (int64_t)max_sets * q_rows;
    std::vector<double> s_all((size_t)n * (size_t)ns), vd((size_t)n), rows_all((size_t)q_all * 3);
    std::vector<int64_t> off_all((size_t)n + 1);
    if (sh) {
        std::memcpy(s_all.data(), s0, Rs * (size_t)ns * sizeof(double));
        std::memcpy(vd.data(), v_desired, Rs * sizeof(double));
        std::memcpy(rows_all.data(), dest_xyz_stop + 3 * q0, (size_t)q_rows * 3 * sizeof(double));
        for (int32_t i = 0; i < R; i++) off_all[(size_t)i] = dest_offsets[i] - q0;
        for (int64_t i = R; i < n; i++) {
            std::memcpy(&s_all[(size_t)i * (size_t)ns], s0, (size_t)ns * sizeof(double));
            vd[(size_t)i] = v_desired[0];
            std::memcpy(&rows_all[(size_t)(q_rows + (i - R)) * 3], dest_xyz_stop + 3 * dest_offsets[0], 3 * sizeof(double));
            off_all[(size_t)i] = q_rows + (i - R);
        }
    }
    for (int32_t k = 0; !sh && k < max_sets; k++) {
        std::memcpy(&s_all[(size_t)k * Rs * (size_t)ns], s0, Rs * (size_t)ns * sizeof(double));
        std::memcpy(&vd[(size_t)k * Rs], v_desired, Rs * sizeof(double));
        std::memcpy(&rows_all[(size_t)k * (size_t)q_rows * 3], dest_xyz_stop + 3 * q0, (size_t)q_rows * 3 * sizeof(double));
        for (int32_t i = 0; i < R; i++) off_all[(size_t)k * Rs + (size_t)i] = (int64_t)k * q_rows + (dest_offsets[i] - q0);
    }
    off_all[(size_t)n] = q_all;
    int rc = add_agents_impl(e, n, s_all.data(), vd.data(), off_all.data(), rows_all.data());
    auto undo = [&](int code) {       // (the engine was empty: what has been added goes again)
        std::vector<int32_t> all((size_t)e->order.size());
        for (size_t i = 0; i < all.size(); i++) all[i] = (int32_t)i;
        const std::string msg = e->err;
        if (!all.empty()) (void)csf_remove_agents(e, (int64_t)all.size(), all.data());
        e->err = msg;
        return code;
    };
    if (rc) return rc;
    if ((rc = upload_all(e))) return undo(rc);
    if ((rc = ensure_compact(e))) return undo(rc);             // slot == place in the population order: slot a is (a / R, a % R)
    // the image: what csf_add_agents made of the first set's slots (the stream is idle: upload_all has waited)
    const size_t cap = (size_t)e->cap;
    hipError_t c = hipStreamSynchronize(e->main);
    for (size_t k = 0; c == hipSuccess && k < STATE_ROWS; k++) c = hipMemcpy(cs->img_s.p + k * Rs, e->s.p + k * cap, Rs * sizeof(double), hipMemcpyDeviceToDevice);
    for (size_t k = 0; c == hipSuccess && k < 5; k++) c = hipMemcpy(cs->img_lti.p + k * Rs, e->lti.p + k * cap, Rs * sizeof(double), hipMemcpyDeviceToDevice);
    for (size_t k = 0; c == hipSuccess && k < 3; k++) c = hipMemcpy(cs->img_znp.p + k * Rs, e->znp.p + k * cap, Rs * sizeof(double), hipMemcpyDeviceToDevice);
    if (c == hipSuccess) c = hipMemcpy(cs->img_ppsi.p, e->ppsi.p, Rs * sizeof(double), hipMemcpyDeviceToDevice);
    if (c == hipSuccess) c = hipMemcpy(cs->img_hx0.p, e->hx.p, Rs * sizeof(double), hipMemcpyDeviceToDevice);      // (row 0 of the ring: csf_scene.h)
    if (c == hipSuccess) c = hipMemcpy(cs->img_hy0.p, e->hy.p, Rs * sizeof(double), hipMemcpyDeviceToDevice);
    if (c == hipSuccess) c = hipMemcpy(cs->img_ti.p, e->ti.p, Rs * sizeof(int32_t), hipMemcpyDeviceToDevice);
    if (c == hipSuccess) c = hipMemcpy(cs->img_ptr.p, e->ptr.p, Rs * sizeof(int32_t), hipMemcpyDeviceToDevice);
    if (c == hipSuccess) c = hipMemcpy(cs->img_status.p, e->status.p, Rs * sizeof(uint32_t), hipMemcpyDeviceToDevice);
    if (c == hipSuccess) c = hipMemcpy(cs->img_znav.p, e->znav.p, Rs, hipMemcpyDeviceToDevice);
    if (sh) {   // what a slot kept for good while it had one rider
        if (c == hipSuccess) c = hipMemcpy(cs->img_vdes.p, e->vdes.p, Rs * sizeof(double), hipMemcpyDeviceToDevice);
        if (c == hipSuccess) c = hipMemcpy(cs->img_qbeg.p, e->qbeg.p, Rs * sizeof(int64_t), hipMemcpyDeviceToDevice);
        if (c == hipSuccess) c = hipMemcpy(cs->img_qlen.p, e->qlen.p, Rs * sizeof(int32_t), hipMemcpyDeviceToDevice);
    }
    if (c != hipSuccess) return undo(fail(e, CSF_E_DEVICE, "%s: the reset image: %s", fn, hipGetErrorString(c)));
    // the views: the engine's Dev with every per-slot array shifted to the block of (set, scene) and the population the scene's.  What
    // the one-wave tick does not touch - the binned order, the exchange records, the rings of a recording - is switched off.
    {
        const Dev &d0 = e->d;
        std::vector<Dev> tab(views, d0);
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
        c = scene_upload_tables(*cs, tab, cs->table, cs->table_w);
        if (c == hipSuccess) c = hipDeviceSynchronize();
        if (c != hipSuccess) return undo(fail(e, CSF_E_DEVICE, "%s: the table of views: %s", fn, hipGetErrorString(c)));
        double cb = 0.0;
        for (int32_t i = 0; i < R; i++) cb = std::max({cb, std::fabs(s0[(size_t)i * ns] - d0.ox), std::fabs(s0[(size_t)i * ns + 1] - d0.oy)});
        cs->coord_bound = cb;
        // the origin of a stand-alone engine that holds scene q: the centre of the box of its start positions (mirror.inc: upload_all)
        cs->h_ox.assign((size_t)n_scn, 0.0), cs->h_oy.assign((size_t)n_scn, 0.0);
        for (int32_t q = 0; q < n_scn; q++) {
            double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
            for (int32_t i = ro[(size_t)q]; i < ro[(size_t)q + 1]; i++) {
                x0 = std::min(x0, s0[(size_t)i * ns]), x1 = std::max(x1, s0[(size_t)i * ns]);
                y0 = std::min(y0, s0[(size_t)i * ns + 1]), y1 = std::max(y1, s0[(size_t)i * ns + 1]);
            }
            const double ox = 0.5 * (x0 + x1), oy = 0.5 * (y0 + y1);
            cs->h_ox[(size_t)q] = std::isfinite(ox) ? ox : 0.0;
            cs->h_oy[(size_t)q] = std::isfinite(oy) ? oy : 0.0;
        }
        cs->h_table = std::move(tab);
    }
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

// csf_scene_calib_eval_road (n_groups == 0: one record per set) and csf_scene_calib_eval_groups (params is [n_sets][n_groups])
static int scene_eval_impl(csf_engine *e, int32_t n_sets, int32_t n_groups, const csf_params *params, size_t params_size, int32_t abi_version,
                           const double *road_F0, const double *road_sigma, double *sums_out, int32_t stride, double *states_out);

int csf_scene_calib_eval_road(csf_engine *e, int32_t n_sets, const csf_params *params, size_t params_size, int32_t abi_version,
                              const double *road_F0, const double *road_sigma, double *sums_out, int32_t stride, double *states_out) try {
    if (!e) return CSF_E_ARG;
    if (e->scene_calib && e->scene_calib->mixed())
        return fail(e, CSF_E_STATE, "csf_scene_calib_eval: the riders are in %d groups of several vehicle classes (csf_scene_calib_classes) and one set cannot say what group 1 carries: csf_scene_calib_eval_groups",
                    (int)e->scene_calib->n_groups);
    if (e->scene_calib && e->scene_calib->n_groups > 0)
        return fail(e, CSF_E_STATE, "csf_scene_calib_eval: the riders are in %d groups (csf_scene_calib_groups / _lane_groups) and one set cannot say what group 1 carries: csf_scene_calib_eval_groups",
                    (int)e->scene_calib->n_groups);
    return scene_eval_impl(e, n_sets, 0, params, params_size, abi_version, road_F0, road_sigma, sums_out, stride, states_out);
} catch (...) { return csf_caught(e); }

int csf_scene_calib_eval_groups(csf_engine *e, int32_t n_sets, int32_t n_groups, const csf_params *params, size_t params_size, int32_t abi_version,
                                const double *road_F0, const double *road_sigma, double *sums_out, int32_t stride, double *states_out) try {
    if (!e) return CSF_E_ARG;
    if (!e->scene_calib) return fail(e, CSF_E_STATE, "csf_scene_calib_eval_groups: no closed-loop data set (csf_scene_calib_load first)");
    const int32_t held = e->scene_calib->n_groups > 0 ? e->scene_calib->n_groups : 1;
    if (n_groups != held) return fail(e, CSF_E_ARG, "csf_scene_calib_eval_groups: %d groups, the data set holds %d (csf_scene_calib_groups)", (int)n_groups, (int)held);
    // (no groups loaded: one record per set, the call is csf_scene_calib_eval_road)
    return scene_eval_impl(e, n_sets, e->scene_calib->n_groups, params, params_size, abi_version, road_F0, road_sigma, sums_out, stride, states_out);
} catch (...) { return csf_caught(e); }

// csf_scene_calib_groups (lanes == false: a csf_scene_calib_load data set, one slot per rider) and csf_scene_calib_lane_groups (lanes ==
// true: a data set of csf_scene_calib_load_shared / _load_wide, the group goes with the rider a lane carries).  `fn` names the call in
// the messages; the checks, the allocate-before-replace order and the drop are one.
static int scene_groups_impl(csf_engine *e, const char *fn, bool lanes, const uint8_t *group, int32_t n_groups) {
    if (!e->scene_calib) {
        if (e->calib) return fail(e, CSF_E_STATE, "%s: the engine holds the data set of csf_calib_load, whose candidate sets are whole populations already", fn);
        return fail(e, CSF_E_STATE, "%s: no closed-loop data set (csf_scene_calib_load first)", fn);
    }
    SceneCalibState &cs = *e->scene_calib;
    if (!lanes && cs.Lsum > 0)
        return fail(e, CSF_E_STATE, "csf_scene_calib_groups: the data set shares its lanes (csf_scene_calib_load_shared / _load_wide): a lane's parameters would change with its rider; groups need csf_scene_calib_load, or csf_scene_calib_lane_groups on this data set");
    if (lanes && cs.Lsum == 0)
        return fail(e, CSF_E_STATE, "csf_scene_calib_lane_groups: the data set has one slot per rider (csf_scene_calib_load): its groups are loaded by csf_scene_calib_groups");
    const bool drop = group == nullptr || n_groups <= 1;
    if (!drop) {
        if (n_groups > SCENE_GROUPS_MAX) return fail(e, CSF_E_ARG, "%s: %d groups (at most %d)", fn, (int)n_groups, SCENE_GROUPS_MAX);
        for (int32_t r = 0; r < cs.R; r++)
            if (group[r] >= n_groups) return fail(e, CSF_E_ARG, "%s: rider %d is in group %d of %d", fn, (int)r, (int)group[r], (int)n_groups);
    }
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->main));
    // everything that can fail first: a refused call changes nothing
    DevBuf<uint8_t> d_group;
    DevBuf<SceneSet> d_sets;
    std::unique_ptr<HostBuf<SceneSet, false>> pin;
    if (!drop) {
        const size_t recs = (size_t)cs.max_sets * (size_t)n_groups;
        pin.reset(new HostBuf<SceneSet, false>());
        hipError_t r = d_group.alloc((size_t)cs.R);
        if (r == hipSuccess) r = d_sets.alloc(recs);
        if (r == hipSuccess) r = pin->alloc(recs);
        if (r == hipSuccess) r = hipMemcpy(d_group.p, group, (size_t)cs.R, hipMemcpyHostToDevice);
        if (r != hipSuccess) return fail(e, CSF_E_DEVICE, "%s: no memory for the groups: %s", fn, hipGetErrorString(r));
        std::memset(pin->p, 0, recs * sizeof(SceneSet));
    }
    scene_drop_classes(e, cs);                                 // (these groups replace the classes of csf_scene_calib_classes)
    cs.group = std::move(d_group);
    cs.sets_g = std::move(d_sets);
    cs.sets_g_pin = std::move(pin);
    cs.n_groups = drop ? 0 : n_groups;
    return CSF_OK;
}

int csf_scene_calib_classes(csf_engine *e, const uint8_t *group, int32_t n_groups, const int32_t *models, const double *s0) try {
    if (!e) return CSF_E_ARG;
    const char *fn = "csf_scene_calib_classes";
    if (!e->scene_calib) {
        if (e->calib) return fail(e, CSF_E_STATE, "%s: the engine holds the data set of csf_calib_load, whose candidate sets are whole populations already", fn);
        return fail(e, CSF_E_STATE, "%s: no closed-loop data set (csf_scene_calib_load first)", fn);
    }
    SceneCalibState &cs = *e->scene_calib;
    if (cs.Lsum > 0)
        return fail(e, CSF_E_STATE, "%s: the data set shares its lanes (csf_scene_calib_load_shared / _load_wide): mixed classes need csf_scene_calib_load - one slot per rider, at most %d riders per scene", fn, SMALL_MAX);
    const bool drop = group == nullptr && n_groups == 0 && models == nullptr && s0 == nullptr;
    HIPCHK(e, hipSetDevice(e->device));
    if (drop) {                                                // the data set is what it was after the load (groups of either call go)
        HIPCHK(e, hipStreamSynchronize(e->main));
        scene_drop_classes(e, cs);
        cs.group = DevBuf<uint8_t>();
        cs.sets_g = DevBuf<SceneSet>();
        cs.sets_g_pin.reset();
        cs.n_groups = 0;
        return CSF_OK;
    }
    if (n_groups < 2 || n_groups > SCENE_CLASS_GROUPS_MAX) return fail(e, CSF_E_ARG, "%s: %d groups (2 .. %d)", fn, (int)n_groups, SCENE_CLASS_GROUPS_MAX);
    if (!group || !models) return fail(e, CSF_E_ARG, "%s: NULL array", fn);
    if (!s0) return fail(e, CSF_E_ARG, "%s: s0 is NULL: the start states in the widest layout, [R][%d]", fn, STATE_ROWS);
    for (int32_t g = 0; g < n_groups; g++)
        if (models[g] < 0 || models[g] > CSF_BALANCINGRIDER || models[g] == CSF_UNCONTROLLED)
            return fail(e, CSF_E_ARG, "%s: group %d is of vehicle class %d: not one of the six simulated classes", fn, (int)g, (int)models[g]);
    for (int32_t r = 0; r < cs.R; r++)
        if (group[r] >= n_groups) return fail(e, CSF_E_ARG, "%s: rider %d is in group %d of %d", fn, (int)r, (int)group[r], (int)n_groups);
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
    // everything that can fail first: a refused call changes nothing
    DevBuf<uint8_t> d_group;
    DevBuf<SceneSet> d_sets;
    DevBuf<double> d_s, d_l, d_p, d_hx, d_hy;
    std::unique_ptr<HostBuf<SceneSet, false>> pin(new HostBuf<SceneSet, false>());
    const size_t recs = (size_t)cs.max_sets * (size_t)n_groups;
    hipError_t r = d_group.alloc(Rs);
    if (r == hipSuccess) r = d_sets.alloc(recs);
    if (r == hipSuccess) r = pin->alloc(recs);
    if (r == hipSuccess) r = d_s.alloc(is.size());
    if (r == hipSuccess) r = d_l.alloc(il.size());
    if (r == hipSuccess) r = d_p.alloc(Rs);
    if (r == hipSuccess) r = d_hx.alloc(Rs);
    if (r == hipSuccess) r = d_hy.alloc(Rs);
    if (r == hipSuccess) r = hipMemcpy(d_group.p, group, Rs, hipMemcpyHostToDevice);
    if (r == hipSuccess) r = hipMemcpy(d_s.p, is.data(), is.size() * sizeof(double), hipMemcpyHostToDevice);
    if (r == hipSuccess) r = hipMemcpy(d_l.p, il.data(), il.size() * sizeof(double), hipMemcpyHostToDevice);
    if (r == hipSuccess) r = hipMemcpy(d_p.p, ip.data(), Rs * sizeof(double), hipMemcpyHostToDevice);
    if (r == hipSuccess) r = hipMemcpy(d_hx.p, hx.data(), Rs * sizeof(double), hipMemcpyHostToDevice);
    if (r == hipSuccess) r = hipMemcpy(d_hy.p, hy.data(), Rs * sizeof(double), hipMemcpyHostToDevice);
    if (r != hipSuccess) return fail(e, CSF_E_DEVICE, "%s: no memory for the classes: %s", fn, hipGetErrorString(r));
    std::memset(pin->p, 0, recs * sizeof(SceneSet));
    if (!cs.mixed()) cs.ns_own = e->d.ns;
    cs.group = std::move(d_group);
    cs.sets_g = std::move(d_sets);
    cs.sets_g_pin = std::move(pin);
    cs.n_groups = n_groups;
    cs.class_models.assign(models, models + n_groups);
    cs.cimg_s = std::move(d_s), cs.cimg_lti = std::move(d_l), cs.cimg_ppsi = std::move(d_p), cs.cimg_hx0 = std::move(d_hx), cs.cimg_hy0 = std::move(d_hy);
    e->d.ns = ns;                                              // csf_num_states: the widest class while the classes are held
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_scene_calib_groups(csf_engine *e, const uint8_t *group, int32_t n_groups) try {
    if (!e) return CSF_E_ARG;
    return scene_groups_impl(e, "csf_scene_calib_groups", false, group, n_groups);
} catch (...) { return csf_caught(e); }

int csf_scene_calib_lane_groups(csf_engine *e, const uint8_t *group, int32_t n_groups) try {
    if (!e) return CSF_E_ARG;
    return scene_groups_impl(e, "csf_scene_calib_lane_groups", true, group, n_groups);
} catch (...) { return csf_caught(e); }

static int scene_eval_impl(csf_engine *e, int32_t n_sets, int32_t n_groups, const csf_params *params, size_t params_size, int32_t abi_version,
                           const double *road_F0, const double *road_sigma, double *sums_out, int32_t stride, double *states_out) {
    if (!e->scene_calib) return fail(e, CSF_E_STATE, "csf_scene_calib_eval: no closed-loop data set (csf_scene_calib_load first)");
    // before anything is read from `params` (csf_create_v)
    if (params_size != sizeof(csf_params) || abi_version != CSF_ABI_VERSION)
        return fail(e, CSF_E_ABI, "csf_scene_calib_eval: the caller's csf_params has %zu bytes and ABI %d, this library's has %zu bytes and ABI %d",
                    params_size, (int)abi_version, sizeof(csf_params), (int)CSF_ABI_VERSION);
    SceneCalibState &cs = *e->scene_calib;
    if (!params || !sums_out) return fail(e, CSF_E_ARG, "csf_scene_calib_eval: NULL array");
    if (n_sets < 1 || n_sets > cs.max_sets) return fail(e, CSF_E_ARG, "csf_scene_calib_eval: %d parameter sets, the data set was loaded for 1 .. %d", (int)n_sets, (int)cs.max_sets);
    if (stride < 1) return fail(e, CSF_E_ARG, "csf_scene_calib_eval: stride must be >= 1");
    const int32_t G = n_groups > 0 ? n_groups : 1;            // records per candidate set
    for (int32_t k = 0; k < n_sets * G; k++) {
        int rc = check_params(e, params + k);
        if (rc) return rc;
        if (cs.mixed()) {                                      // (csf_scene_calib_classes: record (set, g) is of the class loaded for group g)
            if (params[k].model != cs.class_models[(size_t)(k % G)])
                return fail(e, CSF_E_ARG, "csf_scene_calib_eval_groups: the record of set %d, group %d is of vehicle class %d, the group was loaded with class %d (csf_scene_calib_classes)",
                            (int)(k / G), (int)(k % G), (int)params[k].model, (int)cs.class_models[(size_t)(k % G)]);
        } else if (params[k].model != e->d.p.model) return fail(e, CSF_E_ARG, "csf_scene_calib_eval: parameter set %d is of vehicle class %d, the data set was loaded for class %d", (int)k, (int)params[k].model, (int)e->d.p.model);
        if (params[k].t_s != e->d.p.t_s || params[k].traj_len != e->d.p.traj_len)
            return fail(e, CSF_E_ARG, "csf_scene_calib_eval: parameter set %d: t_s and traj_len are the engine's (parameters.py:516-528)", (int)k);
    }
    // road parameters per candidate set: both arrays or neither.  csf_set_road_vertices places no limit on sigma; a value that is
    // not finite is refused here as it is by csf_scene_calib_road
    const bool road_over = road_F0 != nullptr || road_sigma != nullptr;
    if (road_over) {
        if (!road_F0 || !road_sigma) return fail(e, CSF_E_ARG, "csf_scene_calib_eval_road: road_F0 and road_sigma are given together or not at all");
        if (cs.road_stride == 0) return fail(e, CSF_E_STATE, "csf_scene_calib_eval_road: road parameters and no scene has a road (csf_scene_calib_road first)");
        for (int32_t k = 0; k < n_sets; k++) {
            if (!std::isfinite(road_F0[k]) || road_F0[k] < 0.0) return fail(e, CSF_E_ARG, "csf_scene_calib_eval_road: road_F0[%d] = %g is not a finite value >= 0", (int)k, road_F0[k]);
            if (!std::isfinite(road_sigma[k])) return fail(e, CSF_E_ARG, "csf_scene_calib_eval_road: road_sigma[%d] is not finite", (int)k);
        }
    }
    HIPCHK(e, hipSetDevice(e->device));
    int rc = upload_all(e);
    if (rc) return rc;
    if (road_over && (size_t)n_sets * (size_t)cs.road_stride > cs.road_blk.n) {
        HIPCHK(e, hipStreamSynchronize(e->main));
        const hipError_t r = cs.road_blk.alloc((size_t)n_sets * (size_t)cs.road_stride);
        if (r != hipSuccess) {
            cs.road_blk.release();
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
    // the table of this call, composed in pinned memory (the last call has been waited for).  The bands of the fp32 field-of-view
    // and side decisions (consts.inc: fov_band_consts) are those of the largest coordinate any rider can reach in n_ticks from the
    // start of its scene with the set's speed clamp: conservative for every tick, and inside a band the kernel decides by the
    // reference's fp64 chain, so its width changes no result.
    SceneSet *const pin = n_groups > 0 ? cs.sets_g_pin->p : cs.sets_pin.p;
    for (int32_t k = 0; k < n_sets * G; k++) {
        SceneSet &ss = pin[k];
        std::memset(&ss, 0, sizeof ss);
        ss.p = params[k];
        // (groups: the rule belongs to the intersection - the candidate's first record has it, as csf_set_param_classes gives every set
        // the engine's)
        if (n_groups > 0) ss.p.priority_rule = params[k - k % G].priority_rule;
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
        fov_band_consts(e->knobs, step, std::max(cs.coord_bound + step * (double)(cs.n_ticks + 2), cs.rep_bound) + 1.0, ss.pc);
        if (road_over) {   // (the roundings of pack_road)
            ss.road_z = (float)(-road_F0[k / G]);
            ss.road_w = (float)(-0.5 * (road_sigma[k / G] + 1.0));
            ss.road_np = road_np_sigma(road_sigma[k / G]);
        }
    }
    SceneDev c{};
    c.obj = cs.obj.p, c.len = cs.len.p, c.roff = cs.roff.p;
    c.n_scn = cs.n_scn, c.n_ticks = (int32_t)cs.n_ticks, c.n_feat = cs.n_feat, c.R = cs.R;
    for (int k = 0; k < CALIB_MAX_FEAT; k++) c.feat[k] = cs.feat[k];
    c.img_cap = cs.R;
    c.img_s = cs.img_s.p, c.img_lti = cs.img_lti.p, c.img_ppsi = cs.img_ppsi.p, c.img_znp = cs.img_znp.p, c.img_hx0 = cs.img_hx0.p, c.img_hy0 = cs.img_hy0.p;
    c.img_ti = cs.img_ti.p, c.img_ptr = cs.img_ptr.p, c.img_status = cs.img_status.p, c.img_znav = cs.img_znav.p;
    c.sums = cs.sums.dev;
    c.states = n_states > 0 ? cs.states.p : nullptr;
    c.stride = states_out ? stride : 1;
    c.n_samples = (int32_t)n_samples;
    c.n_sets = n_sets;
    c.n_rep = cs.n_rep;
    c.rep_index = cs.n_rep > 0 ? cs.rep_index.p : nullptr;
    c.rep = cs.n_rep > 0 ? cs.rep.p : nullptr;
    c.road_rv = cs.road_stride > 0 ? cs.road_rv.p : nullptr;
    c.road_blk = road_over ? cs.road_blk.p : nullptr;
    c.road_stride = cs.road_stride;
    c.road_lds = (uint32_t)cs.road_max_pad * (uint32_t)sizeof(float4);
    c.win_enter = cs.win_enter.n > 0 ? cs.win_enter.p : nullptr;
    c.win_exit = cs.win_exit.n > 0 ? cs.win_exit.p : nullptr;
    if (cs.Lsum > 0) {
        c.lane_off = cs.lane_off.p, c.lane_first = cs.lane_first.p, c.rider_next = cs.rider_next.p;
        c.img_vdes = cs.img_vdes.p, c.img_qbeg = cs.img_qbeg.p, c.img_qlen = cs.img_qlen.p;
        // a lane writes the sample rows of the rider it carries at the ticks that rider is present: every other row is NaN
        if (n_states > 0) HIPCHK(e, hipMemsetAsync(cs.states.p, 0xff, n_states * sizeof(double), e->main));
    }
    SceneSet *const d_sets = n_groups > 0 ? cs.sets_g.p : cs.sets.p;
    if (n_groups > 0) c.group = cs.group.p, c.n_groups = n_groups;
    if (cs.mixed()) c.img_s = cs.cimg_s.p, c.img_lti = cs.cimg_lti.p, c.img_ppsi = cs.cimg_ppsi.p, c.img_hx0 = cs.cimg_hx0.p, c.img_hy0 = cs.cimg_hy0.p;
    HIPCHK(e, hipMemcpyAsync(d_sets, pin, (size_t)n_sets * (size_t)G * sizeof(SceneSet), hipMemcpyHostToDevice, e->main));
    if (cs.wide_from > 0) {   // the narrow scenes on scene_lanes_kernel, the wide ones on scene_wide_kernel: one stream, one wait
        SceneWideDev w{};
        w.table_w = cs.table_w.p, w.scn_w = cs.scn_w.p;
        w.n_wide = (int32_t)cs.h_scn_w.size(), w.n_narrow = (int32_t)cs.h_scn_n.size();
        w.len_n = cs.len_n.p, w.roff_n = cs.roff_n.p, w.lane_off_n = cs.lane_off_n.p;
        cs.launches += launch_scene_eval(e->d.p.model, cs.table.p, d_sets, c, e->main, &w);
    } else if (cs.mixed()) {   // several vehicle classes: scene_mixed_kernel, the views' state width the widest of them
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

int csf_scene_calib_road(csf_engine *e, int32_t n_edges, const int32_t *edge_scene, const int64_t *offsets, const double *xy, const double *F0,
                         const double *sigma) try {
    if (!e) return CSF_E_ARG;
    if (!e->scene_calib) {
        if (e->calib) return fail(e, CSF_E_STATE, "csf_scene_calib_road: the engine holds the data set of csf_calib_load, whose vehicles are not coupled and feel no road");
        return fail(e, CSF_E_STATE, "csf_scene_calib_road: no closed-loop data set (csf_scene_calib_load first)");
    }
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
            const int64_t nv_pad = (nv[q] + 63) / 64 * 64, n = cs.Lsum > 0 ? cs.h_nl[q] : cs.h_roff[q + 1] - cs.h_roff[q];
            int64_t P = cs.is_wide(q) ? WAVE : 1;              // (a wide scene: the workgroup's P is 64, 128 or 256)
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
    // everything that can fail first: a refused call changes nothing
    DevBuf<float4> d_rv;
    DevBuf<float2> d_rvo;
    DevBuf<Dev> d_table, d_table_w;
    std::vector<Dev> tab = cs.h_table;
    hipError_t r = hipSuccess;
    if (!rv_all.empty()) {
        if (r == hipSuccess) r = d_rv.alloc(rv_all.size());
        if (r == hipSuccess) r = d_rvo.alloc(rvo_all.size());
        if (r == hipSuccess) r = hipMemcpy(d_rv.p, rv_all.data(), rv_all.size() * sizeof(float4), hipMemcpyHostToDevice);
        if (r == hipSuccess) r = hipMemcpy(d_rvo.p, rvo_all.data(), rvo_all.size() * sizeof(float2), hipMemcpyHostToDevice);
    }
    if (r == hipSuccess) {
        for (int32_t k = 0; k < cs.max_sets; k++)
            for (size_t q = 0; q < n_scn; q++) {
                if (nv[q] == 0) continue;
                Dev &v = tab[(size_t)k * n_scn + q];
                v.nv = nv[q], v.nv_pad = (nv[q] + 63) / 64 * 64;
                v.rv = d_rv.p + at[q], v.rvo = d_rvo.p + tile_at[q];
                v.road_np = np[q];
                v.ox = cs.h_ox[q], v.oy = cs.h_oy[q];
                v.rg_nx = v.rg_ny = 0;
            }
        r = scene_upload_tables(cs, tab, d_table, d_table_w);
    }
    if (r == hipSuccess) r = hipDeviceSynchronize();
    if (r != hipSuccess) return fail(e, CSF_E_DEVICE, "csf_scene_calib_road: no memory for the roads: %s", hipGetErrorString(r));
    cs.table = std::move(d_table);
    cs.table_w = std::move(d_table_w);
    cs.road_rv = std::move(d_rv);
    cs.road_rvo = std::move(d_rvo);
    cs.road_blk = DevBuf<float4>();
    cs.road_stride = (int64_t)rv_all.size();
    cs.road_max_pad = (int32_t)max_pad;
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_scene_calib_replay(csf_engine *e, const uint8_t *replayed, const double *rows) try {
    if (!e) return CSF_E_ARG;
    if (!e->scene_calib) return fail(e, CSF_E_STATE, "csf_scene_calib_replay: no closed-loop data set (csf_scene_calib_load first)");
    SceneCalibState &cs = *e->scene_calib;
    const int32_t R = cs.R;
    std::vector<int32_t> index((size_t)R, -1);
    int32_t n_rep = 0;
    for (int32_t r = 0; replayed && r < R; r++)
        if (replayed[r]) index[(size_t)r] = n_rep++;
    if (n_rep > 0 && !rows) return fail(e, CSF_E_ARG, "csf_scene_calib_replay: %d riders are replayed and rows is NULL", (int)n_rep);
    // the rows a tick reads - t < the length of the rider's scene - are finite; the largest coordinate among them sizes the bands
    double bound = 0.0;
    for (int32_t q = 0; n_rep > 0 && q < cs.n_scn; q++)
        for (int32_t r = cs.h_roff[(size_t)q]; r < cs.h_roff[(size_t)q + 1]; r++) {
            const int32_t k = index[(size_t)r];
            if (k < 0) continue;
            for (int64_t t = 0; t < cs.h_len[(size_t)q]; t++) {
                const double *v = rows + ((size_t)t * (size_t)n_rep + (size_t)k) * 4;
                if (!(std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]) && std::isfinite(v[3])))
                    return fail(e, CSF_E_ARG, "csf_scene_calib_replay: the recorded state of rider %d after tick %lld is not finite", (int)r, (long long)t);
                bound = std::max({bound, std::fabs(v[0] - e->d.ox), std::fabs(v[1] - e->d.oy)});
            }
        }
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->main));
    // everything that can fail first: a refused call changes nothing
    DevBuf<int32_t> d_index;
    DevBuf<double> d_rows;
    if (n_rep > 0) {
        const size_t count = (size_t)cs.n_ticks * (size_t)n_rep * 4;
        hipError_t r = d_index.alloc((size_t)R);
        if (r == hipSuccess) r = d_rows.alloc(count);
        if (r == hipSuccess) r = hipMemcpy(d_index.p, index.data(), (size_t)R * sizeof(int32_t), hipMemcpyHostToDevice);
        if (r == hipSuccess) r = hipMemcpy(d_rows.p, rows, count * sizeof(double), hipMemcpyHostToDevice);
        if (r != hipSuccess) return fail(e, CSF_E_DEVICE, "csf_scene_calib_replay: no memory for the recorded states: %s", hipGetErrorString(r));
    }
    cs.rep_index = std::move(d_index);
    cs.rep = std::move(d_rows);
    cs.n_rep = n_rep;
    cs.rep_bound = bound;
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_scene_calib_windows(csf_engine *e, const int32_t *enter, const int32_t *exit) try {
    if (!e) return CSF_E_ARG;
    if (!e->scene_calib) {
        if (e->calib) return fail(e, CSF_E_STATE, "csf_scene_calib_windows: the engine holds the data set of csf_calib_load, whose samples are single vehicles that are there throughout");
        return fail(e, CSF_E_STATE, "csf_scene_calib_windows: no closed-loop data set (csf_scene_calib_load first)");
    }
    SceneCalibState &cs = *e->scene_calib;
    if (cs.Lsum > 0) return fail(e, CSF_E_STATE, "csf_scene_calib_windows: the data set shares its lanes: the windows came with csf_scene_calib_load_shared and decide who sits where");
    if ((enter == nullptr) != (exit == nullptr)) return fail(e, CSF_E_ARG, "csf_scene_calib_windows: enter and exit are given together or not at all");
    const int32_t R = cs.R;
    for (int32_t q = 0; enter && q < cs.n_scn; q++)
        for (int32_t r = cs.h_roff[(size_t)q]; r < cs.h_roff[(size_t)q + 1]; r++)
            if (enter[r] < 0 || enter[r] > exit[r] || exit[r] > cs.h_len[(size_t)q])
                return fail(e, CSF_E_ARG, "csf_scene_calib_windows: rider %d has the window [%d, %d), scene %d has %d ticks (0 <= enter <= exit <= ticks)",
                            (int)r, (int)enter[r], (int)exit[r], (int)q, (int)cs.h_len[(size_t)q]);
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->main));
    // everything that can fail first: a refused call changes nothing
    DevBuf<int32_t> d_enter, d_exit;
    if (enter) {
        hipError_t r = d_enter.alloc((size_t)R);
        if (r == hipSuccess) r = d_exit.alloc((size_t)R);
        if (r == hipSuccess) r = hipMemcpy(d_enter.p, enter, (size_t)R * sizeof(int32_t), hipMemcpyHostToDevice);
        if (r == hipSuccess) r = hipMemcpy(d_exit.p, exit, (size_t)R * sizeof(int32_t), hipMemcpyHostToDevice);
        if (r != hipSuccess) return fail(e, CSF_E_DEVICE, "csf_scene_calib_windows: no memory for the windows: %s", hipGetErrorString(r));
    }
    cs.win_enter = std::move(d_enter);
    cs.win_exit = std::move(d_exit);
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
    std::vector<int32_t> all(e->order.size());
    for (size_t i = 0; i < all.size(); i++) all[i] = (int32_t)i;
    std::shared_ptr<SceneCalibState> cs = std::move(e->scene_calib);   // (csf_remove_agents takes the engine again)
    e->scene_calib.reset();
    rc = all.empty() ? CSF_OK : csf_remove_agents(e, (int64_t)all.size(), all.data());
    if (rc) e->scene_calib = std::move(cs);                            // (refused before it touched the mirror: the data set stays)
    else if (cs->mixed()) e->d.ns = cs->ns_own;                        // (csf_scene_calib_classes: the state width is the engine's own again)
    return rc;                                                         // the buffers go with cs
} catch (...) { return csf_caught(e); }
