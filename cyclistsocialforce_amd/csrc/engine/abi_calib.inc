// engine/abi_calib.inc - C ABI: calibration.  A data set resident on the device, many parameter sets evaluated per launch, the error summed there.
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)
//
// DownhillSimplexCalibration (calibration.py:243-526) calls its objective hundreds of times; every call replays every recorded
// sequence with one candidate parameter set (:438-460) and sums an error over the trajectories (:27-77).  csf_replay_forces restates
// that inner loop for ONE replay - it allocates, uploads the forces, launches once per tick and copies every state back.  Here the
// data set is uploaded once (csf_calib_load), and one call evaluates up to 256 candidate sets on all sequences in one launch
// (csf_calib.hip: replay_eval_kernel) and returns two sums per (set, sequence), from which both error functions follow.
// Also here, for this data set and the closed-loop one (engine/abi_scene.inc): remove_everybody, calib_undo_load, calib_load_refuses.

extern "C++" {

struct CalibState {
    int32_t n_seq = 0, n_feat = 0, max_sets = 0;
    int64_t n_ticks = 0;
    int32_t feat[CALIB_MAX_FEAT] = {0, 0, 0, 0, 0, 0};
    DevBuf<double> Fx, Fy, obj, img_s, img_lti, img_ppsi, states;
    DevBuf<int32_t> len_seq, len_slot, img_ti;
    DevBuf<uint32_t> img_status;
    DevBuf<uint8_t> cls;                 // [cap] slot -> row of `tab`: slot / n_seq
    // the evaluation's own class table - [max_sets] csf_params, then [max_sets][7] PlanarBicycle step matrices - and where the host
    // composes it: one copy per call, whatever the number of sets
    DevBuf<char> tab;
    HostBuf<char, false> tab_pin;
    HostBuf<double2> sums;               // [max_sets * n_seq] written by the kernel (mapped)
    int64_t launches = 0;                // csf_calib_launches
    size_t pb_off() const { return (size_t)max_sets * sizeof(csf_params); }
    size_t tab_bytes() const { return pb_off() + (size_t)max_sets * 7 * sizeof(double); }
};

// every road user of the engine leaves: what the two data sets' loads take back when they fail, and their _clear calls
static int remove_everybody(csf_engine *e) {
    std::vector<int32_t> all(e->order.size());
    for (size_t i = 0; i < all.size(); i++) all[i] = (int32_t)i;
    return all.empty() ? CSF_OK : csf_remove_agents(e, (int64_t)all.size(), all.data());
}

// a load that fails behind add_agents_impl: the engine was empty, so what has been added goes again; the call's message and code stay
static int calib_undo_load(csf_engine *e, int code) {
    const std::string msg = e->err;
    (void)remove_everybody(e);
    e->err = msg;
    return code;
}

// the engine states both loads refuse in the same words; what they say differently stays with them
static int calib_load_refuses(csf_engine *e, const char *fn) {
    if (!e->order.empty()) return fail(e, CSF_E_STATE, "%s: the engine is not empty (%lld road users)", fn, (long long)e->order.size());
    if (e->batch) return fail(e, CSF_E_STATE, "%s: the engine belongs to a batch (csf_batch_leave first)", fn);
    if (e->loopback) return fail(e, CSF_E_STATE, "%s: the engine is a member of a loopback group", fn);
    return CSF_OK;
}

}  // extern "C++"

int csf_calib_load(csf_engine *e, int32_t n_seq, int64_t n_ticks, const double *s0, const double *Fx, const double *Fy, const int32_t *lengths,
                   const double *objective, int32_t n_feat, const int32_t *feat, int32_t max_sets) try {
    if (!e) return CSF_E_ARG;
    if (!s0 || !Fx || !Fy || !objective || !feat) return fail(e, CSF_E_ARG, "csf_calib_load: NULL array");
    if (n_seq < 1 || n_ticks < 1 || n_ticks > 2000000000 || n_feat < 1 || n_feat > CALIB_MAX_FEAT || max_sets < 1 || max_sets > 256)
        return fail(e, CSF_E_ARG, "csf_calib_load: n_seq >= 1, 1 <= n_ticks <= 2e9, 1 <= n_feat <= %d, 1 <= max_sets <= 256", CALIB_MAX_FEAT);
    if (e->calib) return fail(e, CSF_E_STATE, "csf_calib_load: the engine holds a calibration data set already (csf_calib_clear first)");
    if (int crc = calib_refuses(e, "csf_calib_load")) return crc;      // (a closed-loop data set: engine/abi_scene.inc)
    if (int irc = calib_load_refuses(e, "csf_calib_load")) return irc;
    if (e->world > 1 || e->nccl) return fail(e, CSF_E_STATE, "csf_calib_load: a sharded engine replays nothing");
    if (!e->h_road.empty()) return fail(e, CSF_E_STATE, "csf_calib_load: the engine has a road (a replay takes its forces from the data set)");
    if (e->d.hist != nullptr) return fail(e, CSF_E_STATE, "csf_calib_load: the engine records (csf_record / csf_enable_history); a replay writes its own samples");
    if (e->classes.size() != 1) return fail(e, CSF_E_STATE, "csf_calib_load: the engine has %d parameter sets; the candidates of an evaluation replace ONE", (int)e->classes.size());
    if (e->d.p.model == CSF_UNCONTROLLED) return fail(e, CSF_E_ARG, "csf_calib_load: an UncontrolledVehicle follows its trajectory whatever the forces");
    const int64_t n = (int64_t)max_sets * n_seq;
    if (n > e->cap_user) return fail(e, CSF_E_CAPACITY, "csf_calib_load: max_sets x n_seq = %lld road users, capacity %lld", (long long)n, (long long)e->cap_user);
    for (int32_t i = 0; lengths && i < n_seq; i++)
        if (lengths[i] < 0 || lengths[i] > n_ticks) return fail(e, CSF_E_ARG, "csf_calib_load: lengths[%d] = %d outside 0 .. %lld", i, lengths[i], (long long)n_ticks);
    for (int32_t k = 0; k < n_feat; k++)
        if (feat[k] < 0 || feat[k] >= CALIB_MAX_FEAT) return fail(e, CSF_E_ARG, "csf_calib_load: feature %d names no row of vehicle.traj (0 .. %d)", feat[k], CALIB_MAX_FEAT - 1);
    HIPCHK(e, hipSetDevice(e->device));
    // everything that can fail first: a refused call changes nothing
    auto cs = std::make_shared<CalibState>();
    cs->n_seq = n_seq, cs->n_feat = n_feat, cs->max_sets = max_sets, cs->n_ticks = n_ticks;
    for (int32_t k = 0; k < n_feat; k++) cs->feat[k] = feat[k];
    const size_t cap = (size_t)e->cap, tn = (size_t)n_ticks * (size_t)n_seq;
    std::vector<int32_t> ls((size_t)n_seq), la(cap, 0);
    std::vector<uint8_t> cl(cap, 0);
    for (int32_t i = 0; i < n_seq; i++) ls[(size_t)i] = lengths ? lengths[i] : (int32_t)n_ticks;
    for (int64_t a = 0; a < n; a++) la[(size_t)a] = ls[(size_t)(a % n_seq)], cl[(size_t)a] = (uint8_t)(a / n_seq);
    hipError_t r = cs->Fx.upload(Fx, tn);
    if (r == hipSuccess) r = cs->Fy.upload(Fy, tn);
    if (r == hipSuccess) r = cs->obj.upload(objective, tn * (size_t)n_feat);
    if (r == hipSuccess) r = cs->img_s.alloc(STATE_ROWS * cap);
    if (r == hipSuccess) r = cs->img_lti.alloc(5 * cap);
    if (r == hipSuccess) r = cs->img_ppsi.alloc(cap);
    if (r == hipSuccess) r = cs->img_ti.alloc(cap);
    if (r == hipSuccess) r = cs->img_status.alloc(cap);
    if (r == hipSuccess) r = cs->len_seq.upload(ls);
    if (r == hipSuccess) r = cs->len_slot.upload(la);
    if (r == hipSuccess) r = cs->cls.upload(cl);
    if (r == hipSuccess) r = cs->tab.alloc(cs->tab_bytes());
    if (r == hipSuccess) r = cs->tab_pin.alloc(cs->tab_bytes());
    if (r == hipSuccess) r = cs->sums.alloc((size_t)n);
    if (r != hipSuccess) return fail(e, CSF_E_DEVICE, "csf_calib_load: no memory for the data set: %s", hipGetErrorString(r));
    std::memset(cs->tab_pin.p, 0, cs->tab_bytes());
    // the max_sets x n_seq vehicles: every set starts every sequence from the sequence's first state (calibration.py:443-448)
    const int ns = e->d.ns;
    std::vector<double> s_all((size_t)n * (size_t)ns), vd((size_t)n, 0.0);
    for (int64_t a = 0; a < n; a++) std::memcpy(&s_all[(size_t)a * ns], s0 + (a % n_seq) * ns, (size_t)ns * sizeof(double));
    int rc = add_agents_impl(e, n, s_all.data(), vd.data(), nullptr, nullptr);
    if (rc) return rc;
    if ((rc = upload_all(e))) return calib_undo_load(e, rc);
    if ((rc = ensure_compact(e))) return calib_undo_load(e, rc);             // slot == place in the population order: slot a is (a / n_seq, a % n_seq)
    // the image: what csf_add_agents made of the start states (the stream is idle: upload_all has waited)
    hipError_t c = hipStreamSynchronize(e->main);
    if (c == hipSuccess) c = hipMemcpy(cs->img_s.p, e->s.p, STATE_ROWS * cap * sizeof(double), hipMemcpyDeviceToDevice);
    if (c == hipSuccess) c = hipMemcpy(cs->img_lti.p, e->lti.p, 5 * cap * sizeof(double), hipMemcpyDeviceToDevice);
    if (c == hipSuccess) c = hipMemcpy(cs->img_ppsi.p, e->ppsi.p, cap * sizeof(double), hipMemcpyDeviceToDevice);
    if (c == hipSuccess) c = hipMemcpy(cs->img_ti.p, e->ti.p, cap * sizeof(int32_t), hipMemcpyDeviceToDevice);
    if (c == hipSuccess) c = hipMemcpy(cs->img_status.p, e->status.p, cap * sizeof(uint32_t), hipMemcpyDeviceToDevice);
    if (c == hipSuccess) c = hipDeviceSynchronize();
    if (c != hipSuccess) return calib_undo_load(e, fail(e, CSF_E_DEVICE, "csf_calib_load: the reset image: %s", hipGetErrorString(c)));
    e->calib = std::move(cs);
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_calib_eval(csf_engine *e, int32_t n_sets, const csf_params *params, size_t params_size, int32_t abi_version, int32_t fix_speed,
                   double *sums_out, int32_t stride, double *states_out) try {
    if (!e) return CSF_E_ARG;
    if (!e->calib) return fail(e, CSF_E_STATE, "csf_calib_eval: no calibration data set (csf_calib_load first)");
    // before anything is read from `params` (csf_create_v)
    if (params_size != sizeof(csf_params) || abi_version != CSF_ABI_VERSION)
        return fail(e, CSF_E_ABI, "csf_calib_eval: the caller's csf_params has %zu bytes and ABI %d, this library's has %zu bytes and ABI %d",
                    params_size, (int)abi_version, sizeof(csf_params), (int)CSF_ABI_VERSION);
    CalibState &cs = *e->calib;
    if (!params || !sums_out) return fail(e, CSF_E_ARG, "csf_calib_eval: NULL array");
    if (n_sets < 1 || n_sets > cs.max_sets) return fail(e, CSF_E_ARG, "csf_calib_eval: %d parameter sets, the data set was loaded for 1 .. %d", (int)n_sets, (int)cs.max_sets);
    if (states_out && stride < 1) return fail(e, CSF_E_ARG, "csf_calib_eval: stride must be >= 1");
    for (int32_t k = 0; k < n_sets; k++) {
        int rc = check_params(e, params + k);
        if (rc) return rc;
        if (params[k].model != e->d.p.model) return fail(e, CSF_E_ARG, "csf_calib_eval: parameter set %d is of vehicle class %d, the data set was loaded for class %d", (int)k, (int)params[k].model, (int)e->d.p.model);
        if (params[k].t_s != e->d.p.t_s || params[k].traj_len != e->d.p.traj_len)
            return fail(e, CSF_E_ARG, "csf_calib_eval: parameter set %d: t_s and traj_len are the engine's (parameters.py:516-528)", (int)k);
    }
    HIPCHK(e, hipSetDevice(e->device));
    int rc = upload_all(e);
    if (rc) return rc;
    const int64_t n = (int64_t)n_sets * cs.n_seq;
    const int64_t n_samples = states_out ? cs.n_ticks / stride : 0;
    const size_t n_states = (size_t)n_samples * (size_t)n * (size_t)e->d.ns;
    if (n_states > cs.states.n) {
        HIPCHK(e, hipStreamSynchronize(e->main));
        HIPCHK(e, cs.states.alloc(n_states));
    }
    // the table of this call, composed in pinned memory (the last call has been waited for)
    csf_params *pt = (csf_params *)cs.tab_pin.p;
    double *pb = (double *)(cs.tab_pin.p + cs.pb_off());
    for (int32_t k = 0; k < n_sets; k++) {
        pt[k] = params[k];
        pt[k].priority_rule = e->d.p.priority_rule;             // (the rule belongs to the intersection: intersection.py:324)
        for (int j = 0; j < 7; j++) pb[7 * k + j] = 0.0;
        if (pt[k].model == CSF_PLANARBIKE) derive_planarbike(pt[k], pb + 7 * k);
    }
    Dev dd = e->d;                       // a view of the engine: the call's table, its first n slots, a private sample buffer
    dd.ptab = (const csf_params *)cs.tab.p;
    dd.pbtab = (const double *)(cs.tab.p + cs.pb_off());
    dd.cls = cs.cls.p;
    dd.n_classes = n_sets;
    dd.n = dd.n_live = n;                // (the samples are rows of n road users)
    dd.lo = 0;
    dd.hi = n;
    dd.F = e->F.p;
    dd.F_rows = 6;
    dd.replay_len = cs.len_slot.p;
    dd.replay_tick = 0;
    dd.tick = 0;
    dd.hist = n_states > 0 ? cs.states.p : nullptr;
    dd.hist_F = nullptr;
    dd.hist_stride = states_out ? stride : 1;
    dd.hist_cap = (int32_t)std::max<int64_t>(n_samples, 1);
    dd.rec_tick = nullptr;
    dd.atrace = nullptr;
    dd.snap = nullptr;
    CalibDev c{};
    c.Fx = cs.Fx.p, c.Fy = cs.Fy.p, c.obj = cs.obj.p, c.len = cs.len_seq.p;
    c.n_seq = cs.n_seq, c.n_ticks = (int32_t)cs.n_ticks, c.n_feat = cs.n_feat;
    for (int k = 0; k < CALIB_MAX_FEAT; k++) c.feat[k] = cs.feat[k];
    c.img_s = cs.img_s.p, c.img_lti = cs.img_lti.p, c.img_ppsi = cs.img_ppsi.p, c.img_ti = cs.img_ti.p, c.img_status = cs.img_status.p;
    c.sums = cs.sums.dev;
    HIPCHK(e, hipMemcpyAsync(cs.tab.p, cs.tab_pin.p, cs.tab_bytes(), hipMemcpyHostToDevice, e->main));
    launch_replay_eval(dd, PH_INTEGRATE | (fix_speed ? PH_FIXSPEED : 0), c, e->main);
    HIPCHK(e, hipGetLastError());
    cs.launches++;
    if (n_states > 0) HIPCHK(e, hipMemcpyAsync(states_out, cs.states.p, n_states * sizeof(double), hipMemcpyDeviceToHost, e->main));
    HIPCHK(e, hipStreamSynchronize(e->main));
    std::memcpy(sums_out, cs.sums.p, (size_t)n * sizeof(double2));
    // the slots hold the end of this evaluation (the read-backs show it); nothing of it enters the next one
    e->device_ahead = true;
    e->mid_synced = false;
    e->bounds_fresh = false;
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_calib_launches(const csf_engine *e, int64_t *n_launches) try {
    if (!e || !n_launches) return CSF_E_ARG;
    if (!e->calib) return CSF_E_STATE;             // (no data set; no message is written: the call changes nothing)
    *n_launches = e->calib->launches;
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_calib_clear(csf_engine *e) try {
    if (!e) return CSF_E_ARG;
    if (!e->calib) return fail(e, CSF_E_STATE, "csf_calib_clear: no calibration data set");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->main));
    std::shared_ptr<CalibState> cs = std::move(e->calib);      // (the population calls take the engine again; the buffers go with cs)
    e->calib.reset();
    return remove_everybody(e);
} catch (...) { return csf_caught(e); }
