// engine/abi_forces_readback.inc - C ABI: forces on their own, replay, read-backs, the single-function entry points.
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

int csf_calc_forces(csf_engine *e) try {
    if (!e) return CSF_E_ARG;
    if (int crc = calib_refuses(e, "csf_calc_forces")) return crc;
    HIPCHK(e, hipSetDevice(e->device));
    int rc = upload_all(e);
    if (rc) return rc;
    if (e->order.empty()) return CSF_OK;
    rc = wait_gather(e);
    if (rc) return rc;
    rc = bounds_before_pair(e);
    if (rc) return rc;
    if ((e->world > 1 || e->nccl != nullptr || e->loopback) && e->d.recs_valid && e->ticks_since_rebin > 1) {
        launch_sorted_copy(e->d, e->main, e->xbuf_fresh);
        e->xbuf_fresh = false;
    }
    if ((rc = set_fov_band(e))) return rc;
    if (e->d.n_live > 1) launch_pair_all(e, e->d);
    bounds_after_pair(e, false);                     // the records do not move: recompute next time
    launch_road(e->d, e->main);
    launch_agent(e->d, PH_DEST | PH_COMBINE, e->main);
    HIPCHK(e, hipGetLastError());
    e->device_ahead = true;
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_apply_forces(csf_engine *e, const double *Fx, const double *Fy) try {
    if (!e) return CSF_E_ARG;
    if (int crc = calib_refuses(e, "csf_apply_forces")) return crc;
    if (!Fx || !Fy) return fail(e, CSF_E_ARG, "csf_apply_forces: NULL force array");
    HIPCHK(e, hipSetDevice(e->device));
    if (e->world > 1) return fail(e, CSF_E_STATE, "csf_apply_forces is a single-device entry point");
    int rc = upload_all(e);
    if (rc) return rc;
    if (e->order.empty()) return CSF_OK;
    HIPCHK(e, hipStreamSynchronize(e->main));
    {   // Fx, Fy are in population order, the device array is indexed by slot
        std::vector<double> fx((size_t)e->d.n, 0.0), fy((size_t)e->d.n, 0.0);
        for (size_t i = 0; i < e->order.size(); i++) {
            fx[(size_t)e->order[i]] = Fx[i];
            fy[(size_t)e->order[i]] = Fy[i];
        }
        HIPCHK(e, hipMemcpy(e->F.p, fx.data(), fx.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(e, hipMemcpy(e->F.p + e->cap, fy.data(), fy.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    launch_agent(e->d, PH_INTEGRATE, e->main);
    HIPCHK(e, hipGetLastError());
    e->mid_synced = false;
    e->bounds_fresh = false;
    if (!e->pair_since_move) e->moved_unbinned++;              // (csf_calc_forces before it has counted this tick already)
    e->pair_since_move = false;
    e->moves++;
    e->d.tick++;
    e->device_ahead = true;
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_replay_forces(csf_engine *e, int64_t n_ticks, const double *Fx, const double *Fy, const int32_t *lengths,
                      int32_t fix_speed, int32_t stride, double *states_out) try {
    if (!e) return CSF_E_ARG;
    if (int crc = calib_refuses(e, "csf_replay_forces")) return crc;
    if (n_ticks < 0 || stride < 1 || (n_ticks > 0 && (!Fx || !Fy))) return fail(e, CSF_E_ARG, "csf_replay_forces: bad arguments");
    if (e->world > 1) return fail(e, CSF_E_STATE, "csf_replay_forces is a single-device entry point");
    if (lengths)
        for (size_t a = 0; a < e->order.size(); a++)
            if (lengths[a] < 0) return fail(e, CSF_E_ARG, "csf_replay_forces: lengths[%d] is negative", (int)a);
    HIPCHK(e, hipSetDevice(e->device));
    int rc = upload_all(e);
    if (rc) return rc;
    if ((rc = ensure_compact(e))) return rc;
    const int64_t n = e->d.n, cap = e->cap;
    if (n == 0 || n_ticks == 0) return CSF_OK;
    HIPCHK(e, hipStreamSynchronize(e->main));
    const int64_t chunk = std::min<int64_t>(n_ticks, 256);
    DevBuf<double> fbuf, hbuf;
    DevBuf<int32_t> lbuf;
    // (the per-agent kernel asks for the destination-force rows F[2], F[3] of its view unconditionally - a guarded load would be
    // a branch with its own wait; the view says how many rows it has, Dev::F_rows, and the kernel clamps the row: no padding)
    HIPCHK(e, fbuf.alloc((size_t)chunk * 2 * (size_t)cap));
    const int64_t n_samples = n_ticks / stride;
    if (states_out && n_samples > 0) HIPCHK(e, hbuf.alloc((size_t)n_samples * (size_t)n * (size_t)e->d.ns));
    if (lengths) {
        HIPCHK(e, lbuf.alloc((size_t)n));
        HIPCHK(e, hipMemcpy(lbuf.p, lengths, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    Dev dd = e->d;                       // a view of the engine with replay forces and a private history ring
    dd.F_rows = 2;                       // (the view holds Fx, Fy of one tick: the kernel clamps its row index - csf_dev.h)
    dd.replay_len = lengths ? lbuf.p : nullptr;
    dd.hist = (states_out && n_samples > 0) ? hbuf.p : nullptr;
    dd.hist_F = nullptr;                 // (the engine's own recording does not see the replay)
    dd.hist_stride = stride;
    dd.hist_cap = (int32_t)std::max<int64_t>(n_samples, 1);
    std::vector<double> host((size_t)chunk * 2 * (size_t)cap, 0.0);
    for (int64_t t0 = 0; t0 < n_ticks; t0 += chunk) {
        const int64_t cnt = std::min<int64_t>(chunk, n_ticks - t0);
        for (int64_t t = 0; t < cnt; t++) {
            memcpy(&host[(size_t)(t * 2) * cap], Fx + (t0 + t) * n, (size_t)n * sizeof(double));
            memcpy(&host[(size_t)(t * 2 + 1) * cap], Fy + (t0 + t) * n, (size_t)n * sizeof(double));
        }
        HIPCHK(e, hipMemcpy(fbuf.p, host.data(), (size_t)cnt * 2 * cap * sizeof(double), hipMemcpyHostToDevice));
        for (int64_t t = 0; t < cnt; t++) {
            dd.F = fbuf.p + (size_t)(t * 2) * cap;   // PH_INTEGRATE alone reads only Fx = F[0][.], Fy = F[1][.]
            dd.replay_tick = t0 + t;
            dd.tick = t0 + t;                        // history sample index counts from the start of the replay
            launch_agent(dd, PH_INTEGRATE | (fix_speed ? PH_FIXSPEED : 0), e->main);
        }
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipStreamSynchronize(e->main));
    }
    e->d.tick += n_ticks;
    e->moves += n_ticks;
    e->mid_synced = false;
    e->moved_unbinned += n_ticks;
    e->pair_since_move = false;
    if (fix_speed) {                         // (calibration.py:454-458 sets the speed to |F|: no clamp bounds the step)
        e->bound_stale = true;
        e->moved_unbinned = 1 << 20;         // (nor what the candidate lists and the circles allow for: re-bin before the next pair launch)
    }
    e->device_ahead = true;
    e->bounds_fresh = false;
    if (dd.hist)
        HIPCHK(e, hipMemcpy(states_out, hbuf.p, (size_t)n_samples * n * e->d.ns * sizeof(double), hipMemcpyDeviceToHost));
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_dest_force(csf_engine *e, double *Fx, double *Fy) try {
    if (!e) return CSF_E_ARG;
    if (!Fx || !Fy) return fail(e, CSF_E_ARG, "csf_dest_force: NULL output");
    if (int crc = calib_refuses(e, "csf_dest_force")) return crc;
    HIPCHK(e, hipSetDevice(e->device));
    int rc = upload_all(e);
    if (rc) return rc;
    if (e->order.empty()) return CSF_OK;
    launch_agent(e->d, PH_DEST, e->main);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(e->main));
    e->device_ahead = true;
    if ((rc = read_rows(e, e->F.p + 2 * e->cap, 1, Fx, false))) return rc;
    return read_rows(e, e->F.p + 3 * e->cap, 1, Fy, false);
} catch (...) { return csf_caught(e); }

int csf_get_state(csf_engine *e, double *s_out, int32_t *dest_ptr, uint8_t *znav, int64_t *tick) try {
    if (!e) return CSF_E_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    int rc = upload_all(e);  // a never-stepped engine still answers from a consistent device copy
    if (rc) return rc;
    rc = csf_sync(e);
    if (rc) return rc;
    const int64_t n = (int64_t)e->order.size();
    const int ns = e->d.ns;
    if (tick) *tick = e->d.tick;
    if (n == 0) return CSF_OK;
    if (s_out && (rc = read_rows(e, e->s.p, ns, s_out, true))) return rc;
    if (dest_ptr && (rc = read_rows(e, e->ptr.p, 1, dest_ptr, false))) return rc;
    if (znav) {
        std::vector<uint8_t> z((size_t)n);
        if ((rc = read_rows(e, e->znav.p, 1, z.data(), false))) return rc;
        for (int64_t a = 0; a < n; a++) {
            znav[3 * a + 0] = (z[(size_t)a] & 3) == 0;
            znav[3 * a + 1] = (z[(size_t)a] & 3) == 1;
            znav[3 * a + 2] = (z[(size_t)a] & 3) == 2;
        }
    }
    return CSF_OK;
} catch (...) { return csf_caught(e); }

static int get_F(csf_engine *e, int comp, double *out) {
    if (!out) return CSF_OK;
    return read_rows(e, e->F.p + (size_t)comp * e->cap, 1, out, false);
}

// the packed read-back in the mapped host buffer -> the caller's arrays
static int snap_unpack(csf_engine *e, double *s_out, int32_t *dest_ptr, uint8_t *znav, double *Fx, double *Fy) {
    const int64_t n = (int64_t)e->order.size();
    const int ns = e->d.ns;
    const double *S = (const double *)e->snap.p;
    const double *F = S + (size_t)n * ns;
    const int32_t *P = (const int32_t *)(F + 2 * (size_t)n);
    const uint8_t *Z = (const uint8_t *)(P + n);
    if (s_out) std::memcpy(s_out, S, (size_t)n * ns * sizeof(double));
    if (Fx) std::memcpy(Fx, F, (size_t)n * sizeof(double));
    if (Fy) std::memcpy(Fy, F + n, (size_t)n * sizeof(double));
    if (dest_ptr) std::memcpy(dest_ptr, P, (size_t)n * sizeof(int32_t));
    if (znav) std::memcpy(znav, Z, (size_t)n * 3);
    return CSF_OK;
}

int csf_get_tick(csf_engine *e, double *s_out, int32_t *dest_ptr, uint8_t *znav, double *Fx, double *Fy, int64_t *tick) try {
    if (!e) return CSF_E_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    int rc = upload_all(e);  // a never-stepped engine still answers from a consistent device copy
    if (rc) return rc;
    if (tick) *tick = e->d.tick;
    if (e->order.empty()) return csf_sync(e);
    if ((rc = sync_order(e))) return rc;
    if ((rc = snap_reserve(e))) return rc;
    launch_snapshot(e->d, (double *)e->snap.dev, e->main);
    HIPCHK(e, hipGetLastError());
    rc = csf_sync(e);
    if (rc) return rc;
    return snap_unpack(e, s_out, dest_ptr, znav, Fx, Fy);
} catch (...) { return csf_caught(e); }

// csf_step(e, n_ticks) + csf_get_tick in one call: what a caller that looks at every tick does (SocialForceIntersection.step(),
// intersection.py:866-896 - the host mirror refreshes vehicle.s, znav, force after each tick).  On the one-wave path the kernel
// packs the read-back itself: one launch and one wait per call.
int csf_step_get_tick(csf_engine *e, int64_t n_ticks, double *s_out, int32_t *dest_ptr, uint8_t *znav, double *Fx, double *Fy,
                      int64_t *tick) try {
    bool snapped = false;
    int rc = step_impl(e, n_ticks, true, &snapped);
    if (rc) return rc;
    if (!snapped) return csf_get_tick(e, s_out, dest_ptr, znav, Fx, Fy, tick);
    if (tick) *tick = e->d.tick;
    if ((rc = csf_sync(e))) return rc;
    return snap_unpack(e, s_out, dest_ptr, znav, Fx, Fy);
} catch (...) { return csf_caught(e); }

int csf_get_forces(csf_engine *e, double *Fx, double *Fy) try {
    if (!e) return CSF_E_ARG;
    int rc = csf_sync(e);
    if (rc) return rc;
    if (e->dirty && !e->device_ahead) {
        rc = upload_all(e);
        if (rc) return rc;
    }
    if (e->order.empty()) return CSF_OK;
    if ((rc = get_F(e, 0, Fx))) return rc;
    return get_F(e, 1, Fy);
} catch (...) { return csf_caught(e); }

int csf_get_force_parts(csf_engine *e, double *Fdest_x, double *Fdest_y, double *Frep_x, double *Frep_y) try {
    if (!e) return CSF_E_ARG;
    int rc = csf_sync(e);
    if (rc) return rc;
    if (e->order.empty()) return CSF_OK;
    if ((rc = get_F(e, 2, Fdest_x))) return rc;
    if ((rc = get_F(e, 3, Fdest_y))) return rc;
    if ((rc = get_F(e, 4, Frep_x))) return rc;
    return get_F(e, 5, Frep_y);
} catch (...) { return csf_caught(e); }

int csf_status(csf_engine *e, uint32_t *per_agent_flags) try {
    if (!e) return CSF_E_ARG;
    if (!per_agent_flags) return fail(e, CSF_E_ARG, "csf_status: NULL output");
    int rc = upload_all(e);
    if (rc) return rc;
    rc = csf_sync(e);
    if (rc) return rc;
    if (e->order.empty()) return CSF_OK;
    rc = read_rows(e, e->status.p, 1, per_agent_flags, false);
    for (size_t i = 0; rc == CSF_OK && i < e->order.size(); i++) per_agent_flags[i] &= ~CSF_ST_EDGE;   // (internal: csf_dev.h)
    return rc;
} catch (...) { return csf_caught(e); }

// (re)allocates the rings; everything that can fail first, then the old rings go: a refused call changes nothing
static int rings_setup(csf_engine *e, int32_t stride, int32_t capacity, bool forces, bool fast) {
    if (int crc = calib_refuses(e, "csf_record / csf_enable_history")) return crc;
    HIPCHK(e, hipSetDevice(e->device));
    int rc = csf_sync(e);
    if (rc) return rc;
    if ((rc = ensure_compact(e))) return rc;              // the ring is indexed by road user: slots == population order
    DevBuf<double> hs, hf;
    DevBuf<int64_t> tk;
    const size_t rows = (size_t)capacity * (size_t)e->cap;
    hipError_t r = hs.alloc(rows * (size_t)e->d.ns);
    if (r == hipSuccess && forces) r = hf.alloc(rows * 2);
    if (r == hipSuccess && fast) r = tk.alloc(1);
    if (r != hipSuccess)
        return fail(e, CSF_E_DEVICE, "no device memory for a ring of %d samples: %s", (int)capacity, hipGetErrorString(r));
    std::swap(e->hist, hs); std::swap(e->hist_F, hf); std::swap(e->rec_tick, tk);   // (the old rings go with hs, hf, tk)
    e->d.hist = e->hist.p;
    e->d.hist_F = e->hist_F.p;
    e->d.rec_tick = e->rec_tick.p;
    e->d.hist_stride = stride;
    e->d.hist_cap = capacity;
    e->rec_tick_dev = -1;
    e->rec_k0 = e->d.tick / stride;                       // sample k is the state after tick (k + 1) * stride: k >= tick / stride are this ring's
    e->rec_fast = fast;
    return CSF_OK;
}

int csf_enable_history(csf_engine *e, int32_t stride, int32_t capacity) try {
    if (!e) return CSF_E_ARG;
    if (stride < 1 || capacity < 1) return fail(e, CSF_E_ARG, "stride and capacity must be >= 1");
    return rings_setup(e, stride, capacity, false, false);
} catch (...) { return csf_caught(e); }

int csf_record(csf_engine *e, int32_t stride, int32_t capacity, uint32_t what) try {
    if (!e) return CSF_E_ARG;
    if (stride < 1 || capacity < 1) return fail(e, CSF_E_ARG, "stride and capacity must be >= 1");
    if (what == 0 || (what & ~(CSF_REC_STATE | CSF_REC_FORCE)) != 0)
        return fail(e, CSF_E_ARG, "csf_record: what must be CSF_REC_STATE, CSF_REC_FORCE or both (got 0x%x)", (unsigned)what);
    return rings_setup(e, stride, capacity, (what & CSF_REC_FORCE) != 0, true);
} catch (...) { return csf_caught(e); }

extern "C++" {

// samples [first, first + count) of one engine's rings, for the caller's arrays (either may be NULL)
struct RecAsk {
    csf_engine *e;
    int64_t first, count;
    double *s_out, *F_out;
};

// samples [first, first + count) are in the ring, and written since it was started or the roster last changed (rec_k0): the
// message of csf_get_history
static int record_range(csf_engine *e, int64_t first, int64_t count) {
    const int64_t have = e->d.tick / e->d.hist_stride;
    if (first < 0 || count < 0 || first + count > have || have - first > e->d.hist_cap || first < e->rec_k0)
        return fail(e, CSF_E_ARG, "samples [%lld, %lld) are not in the ring (have %lld, capacity %d, first readable sample %lld)",
                    (long long)first, (long long)(first + count), (long long)have, e->d.hist_cap,
                    (long long)std::max(e->rec_k0, have - e->d.hist_cap));
    return CSF_OK;
}

// the same for the last n_last samples of member i of a batch (n_last >= 0): *first is the first of them
static int record_last(csf_engine *e, int32_t i, int64_t n_last, int64_t *first) {
    const int64_t have = e->d.tick / e->d.hist_stride;
    if (n_last > have || n_last > e->d.hist_cap || n_last > have - e->rec_k0)
        return fail(e, CSF_E_ARG, "member %d: the last %lld samples are not in the ring (have %lld, capacity %d, first readable sample %lld)",
                    (int)i, (long long)n_last, (long long)have, e->d.hist_cap, (long long)std::max(e->rec_k0, have - e->d.hist_cap));
    *first = have - n_last;
    return CSF_OK;
}

// One gather launch on `st` (the stream every engine asked about works on), one wait, then the packed buffer -> the callers' arrays.
// The asks have been checked (record_range; rings present where an output is given).
static int record_gather(csf_engine *e0, RecGather &g, hipStream_t st, const RecAsk *asks, size_t m) {
    if (m == 0) return CSF_OK;
    if (m > 65535) return fail(e0, CSF_E_ARG, "at most 65535 engines in one read-back of rings (%zu given)", m);
    size_t total = 0;
    int64_t most = 0;
    for (size_t i = 0; i < m; i++) {
        const RecAsk &a = asks[i];
        const size_t n = (size_t)a.e->d.n, ns = (size_t)a.e->d.ns, c = (size_t)a.count;
        if (a.s_out) total += (c * n * ns + 1) & ~(size_t)1, most = std::max<int64_t>(most, (int64_t)(c * n * ns));
        if (a.F_out) total += c * n * 2, most = std::max<int64_t>(most, (int64_t)(c * n * 2));
    }
    if (total == 0) return CSF_OK;
    HIPCHK(e0, g.reserve(m, total, st));
    size_t at = 0;
    for (size_t i = 0; i < m; i++) {
        const RecAsk &a = asks[i];
        const Dev &d = a.e->d;
        const size_t n = (size_t)d.n, ns = (size_t)d.ns, c = (size_t)a.count;
        RecDesc r{};
        r.n = (int32_t)d.n, r.ns = d.ns, r.cap = d.hist_cap;
        r.first = (int32_t)(a.first % d.hist_cap), r.count = (int32_t)a.count;
        if (a.s_out && c * n > 0) r.s = d.hist, r.s_off = (int64_t)at, at += (c * n * ns + 1) & ~(size_t)1;
        if (a.F_out && c * n > 0) r.F = d.hist_F, r.F_off = (int64_t)at, at += c * n * 2;
        g.desc.p[i] = r;
    }
    launch_record_gather(g.desc.dev, (int)m, most, g.out.dev, st);
    HIPCHK(e0, hipGetLastError());
    HIPCHK(e0, hipStreamSynchronize(st));
    for (size_t i = 0; i < m; i++) {
        const RecAsk &a = asks[i];
        const RecDesc &r = g.desc.p[i];
        const size_t n = (size_t)r.n, c = (size_t)r.count;
        if (r.s) std::memcpy(a.s_out, g.out.p + r.s_off, c * n * (size_t)r.ns * sizeof(double));
        if (r.F) std::memcpy(a.F_out, g.out.p + r.F_off, c * n * 2 * sizeof(double));
    }
    return CSF_OK;
}

}  // extern "C++"

int csf_get_history(csf_engine *e, int64_t first_sample, int64_t n_samples, double *out) try {
    if (!e) return CSF_E_ARG;
    if (!e->d.hist) return fail(e, CSF_E_STATE, "history is not enabled");
    if (!out || first_sample < 0 || n_samples < 0) return fail(e, CSF_E_ARG, "csf_get_history: bad arguments");
    HIPCHK(e, hipSetDevice(e->device));
    int rc = csf_sync(e);
    if (rc) return rc;
    if ((rc = record_range(e, first_sample, n_samples))) return rc;
    const RecAsk ask{e, first_sample, n_samples, out, nullptr};
    return record_gather(e, e->rgather, e->main, &ask, 1);
} catch (...) { return csf_caught(e); }

int csf_get_record(csf_engine *e, int64_t first_sample, int64_t n_samples, double *s_out, double *F_out) try {
    if (!e) return CSF_E_ARG;
    if (!e->d.hist) return fail(e, CSF_E_STATE, "history is not enabled (csf_record)");
    if ((!s_out && !F_out) || first_sample < 0 || n_samples < 0) return fail(e, CSF_E_ARG, "csf_get_record: bad arguments");
    if (F_out && !e->d.hist_F) return fail(e, CSF_E_STATE, "forces are not recorded (csf_record with CSF_REC_FORCE)");
    HIPCHK(e, hipSetDevice(e->device));
    int rc = csf_sync(e);
    if (rc) return rc;
    if ((rc = record_range(e, first_sample, n_samples))) return rc;
    const RecAsk ask{e, first_sample, n_samples, s_out, F_out};
    return record_gather(e, e->rgather, e->main, &ask, 1);
} catch (...) { return csf_caught(e); }

int csf_pair_force(csf_engine *e, const double *src, int64_t m, const double *x, const double *y,
                   const double *psi, int32_t apply_fov, double *Fx, double *Fy) try {
    if (!e) return CSF_E_ARG;
    if (m < 0 || !src || (m > 0 && (!x || !y || !psi || !Fx || !Fy))) return fail(e, CSF_E_ARG, "csf_pair_force: bad arguments");
    if (m == 0) return CSF_OK;
    HIPCHK(e, hipSetDevice(e->device));
    const csf_params &p = e->d.p;
    std::vector<float4> hs((size_t)m), hr((size_t)m);
    std::vector<float2> h2((size_t)m), ho((size_t)m);
    double ev = 0.0;  // vehicle.py:1062-1064
    if (src[3] > 0.0) ev = std::min(std::pow(src[3] / p.v_max_riding[1], 0.1), 0.7);
    for (int64_t k = 0; k < m; k++) {
        hs[(size_t)k] = make_float4(0.f, 0.f, (float)std::cos(src[2]), (float)std::sin(src[2]));
        hr[(size_t)k] = make_float4((float)(x[k] - src[0]), (float)(y[k] - src[1]), (float)std::cos(psi[k]), (float)std::sin(psi[k]));
        h2[(size_t)k] = make_float2((float)ev, (float)(1.0 / std::sqrt(1.0 - ev * ev)));
    }
    if (e->kat4.n < (size_t)(2 * m)) HIPCHK(e, e->kat4.alloc((size_t)(2 * m)));
    if (e->kat2.n < (size_t)(2 * m)) HIPCHK(e, e->kat2.alloc((size_t)(2 * m)));
    HIPCHK(e, hipMemcpy(e->kat4.p, hs.data(), (size_t)m * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(e->kat4.p + m, hr.data(), (size_t)m * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(e->kat2.p, h2.data(), (size_t)m * sizeof(float2), hipMemcpyHostToDevice));
    launch_pair_kat(e->d, e->kat4.p, e->kat2.p, e->kat4.p + m, m, apply_fov, e->kat2.p + m, e->main);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(e->main));
    HIPCHK(e, hipMemcpy(ho.data(), e->kat2.p + m, (size_t)m * sizeof(float2), hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < m; k++) {
        Fx[k] = ho[(size_t)k].x;
        Fy[k] = ho[(size_t)k].y;
    }
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_untracked(csf_engine *e, uint8_t *out) try {
    if (!e) return CSF_E_ARG;
    if (!out) return fail(e, CSF_E_ARG, "csf_untracked: NULL output");
    HIPCHK(e, hipSetDevice(e->device));
    int rc = upload_all(e);
    if (rc) return rc;
    const int64_t n = (int64_t)e->order.size();
    if (n == 0) return CSF_OK;
    if (n > 46340) return fail(e, CSF_E_ARG, "csf_untracked: the n x n matrix is limited to n <= 46340");
    if ((rc = wait_gather(e))) return rc;
    if ((rc = sync_order(e))) return rc;
    HIPCHK(e, e->scratch_u8.reserve((size_t)(n * n)));         // (every byte of the matrix is written by the kernel)
    e->d.state_current = e->state_all_current ? 1 : 0;        // (then every pair is decided on the fp64 state, as the reference does)
    launch_untracked(e->d, e->scratch_u8.p, e->main);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(e->main));
    HIPCHK(e, hipMemcpy(out, e->scratch_u8.p, (size_t)(n * n), hipMemcpyDeviceToHost));
    return CSF_OK;
} catch (...) { return csf_caught(e); }

static int nav_kat(csf_engine *e, int64_t n, const int32_t *idx, int what, const int32_t *stop, double *vd, double *ddest) {
    if (n < 0 || (n > 0 && !idx)) return fail(e, CSF_E_ARG, "bad agent list");
    if (int crc = calib_refuses(e, "csf_update_destination / csf_update_nav_state")) return crc;
    for (int64_t k = 0; k < n; k++)
        if (idx[k] < 0 || idx[k] >= (int64_t)e->order.size()) return fail(e, CSF_E_ARG, "agent index %d out of range", idx[k]);
    HIPCHK(e, hipSetDevice(e->device));
    int rc = upload_all(e);
    if (rc) return rc;
    if (n == 0) return CSF_OK;
    HIPCHK(e, hipStreamSynchronize(e->main));                  // (the scratch buffers may still be read by an earlier call)
    HIPCHK(e, e->scratch_i32.reserve((size_t)(2 * n)));
    HIPCHK(e, e->scratch_f64.reserve((size_t)(2 * n)));
    int32_t *di = e->scratch_i32.p, *ds = e->scratch_i32.p + n;
    double *out = e->scratch_f64.p;
    std::vector<int32_t> slots((size_t)n);
    for (int64_t k = 0; k < n; k++) slots[(size_t)k] = e->order[(size_t)idx[k]];
    HIPCHK(e, hipMemcpy(di, slots.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    if (stop) HIPCHK(e, hipMemcpy(ds, stop, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    launch_nav_kat(e->d, di, n, what, stop ? ds : nullptr, out, out + n, e->main);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(e->main));
    e->device_ahead = true;
    if (vd) HIPCHK(e, hipMemcpy(vd, out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    if (ddest) HIPCHK(e, hipMemcpy(ddest, out + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return CSF_OK;
}

int csf_update_destination(csf_engine *e, int64_t n, const int32_t *idx) try {
    if (!e) return CSF_E_ARG;
    return nav_kat(e, n, idx, 1, nullptr, nullptr, nullptr);
} catch (...) { return csf_caught(e); }

int csf_update_nav_state(csf_engine *e, int64_t n, const int32_t *idx, const int32_t *stop, double *vd, double *ddest) try {
    if (!e) return CSF_E_ARG;
    if (n > 0 && (!vd || !ddest)) return fail(e, CSF_E_ARG, "csf_update_nav_state: NULL output");
    return nav_kat(e, n, idx, 2, stop, vd, ddest);
} catch (...) { return csf_caught(e); }

int csf_set_dest_pointer(csf_engine *e, int64_t n, const int32_t *idx, const int32_t *ptr) try {
    if (!e) return CSF_E_ARG;
    if (n < 0 || (n > 0 && (!idx || !ptr))) return fail(e, CSF_E_ARG, "csf_set_dest_pointer: bad arguments");
    for (int64_t k = 0; k < n; k++) {
        if (idx[k] < 0 || idx[k] >= (int64_t)e->order.size()) return fail(e, CSF_E_ARG, "agent index %d out of range", idx[k]);
        const int32_t rows = (int32_t)(e->h_q[(size_t)e->order[(size_t)idx[k]]].size() / 3);
        if (ptr[k] < 0 || ptr[k] >= rows) return fail(e, CSF_E_ARG, "destination pointer %d outside the queue of agent %d (%d rows)", ptr[k], idx[k], rows);
    }
    HIPCHK(e, hipSetDevice(e->device));
    int rc = prepare_mutation(e);
    if (rc) return rc;
    for (int64_t k = 0; k < n; k++) e->h_ptr[(size_t)e->order[(size_t)idx[k]]] = ptr[k];
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_set_script(csf_engine *e, int64_t n, const int32_t *agent, const int64_t *offsets, const double *rows) try {
    if (!e) return CSF_E_ARG;
    if (n < 0 || (n > 0 && (!agent || !offsets))) return fail(e, CSF_E_ARG, "csf_set_script: bad arguments");
    for (int64_t k = 0; k < n; k++) {
        if (agent[k] < 0 || agent[k] >= (int64_t)e->order.size()) return fail(e, CSF_E_ARG, "agent index %d out of range", agent[k]);
        if (offsets[k + 1] < offsets[k]) return fail(e, CSF_E_ARG, "offsets must be non-decreasing");
        if (offsets[k + 1] > offsets[k] && !rows) return fail(e, CSF_E_ARG, "csf_set_script: NULL rows");
        if (offsets[k + 1] - offsets[k] > 2000000000) return fail(e, CSF_E_ARG, "a prescribed trajectory holds at most 2e9 states");
    }
    {   // (a road user may get its trajectory before it is given its parameter set - the mirror does: add, script, then the rows of
        // the table - so what is asked is that the engine HAS such a set)
        bool any = false;
        for (const csf_params &c : e->classes) any = any || c.model == CSF_UNCONTROLLED;
        if (n > 0 && !any) return fail(e, CSF_E_ARG, "csf_set_script: no parameter set of this engine is an UncontrolledVehicle's - nobody would follow the trajectory");
    }
    if (n == 0) return CSF_OK;
    HIPCHK(e, hipSetDevice(e->device));
    int rc = prepare_mutation(e);                              // (through the host mirror: scripts are set once, before the run)
    if (rc) return rc;
    for (int64_t k = 0; k < n; k++) {
        std::vector<double> &sc = e->h_script[(size_t)e->order[(size_t)agent[k]]];
        sc.assign(rows + 4 * offsets[k], rows + 4 * offsets[k + 1]);
    }
    return CSF_OK;
} catch (...) { return csf_caught(e); }
