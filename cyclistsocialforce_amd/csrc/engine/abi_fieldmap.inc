// engine/abi_fieldmap.inc - C ABI: the force field at arbitrary probe points (csf_fieldmap.hip).
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

extern "C++" {

// The rounding bands of the map's field-of-view and np.sign(phi) tests (consts.inc: fov_band_consts has the tick's).  With u = 2^-24:
// (dx, dy) is an fp64 difference rounded once - off by u |dx|, u |dy|, whatever the extent of the scene -, a heading (cos, sin) by u
// per component.  t = rho cos(bearing) is then off by < 6 u rho and g = t|t| + chs rho^2 by < 20 u rho^2; rho sin(bearing), and
// rho sin(phi) of the TwoD field, by < 5 u rho.  Twice that each; tracked_m takes the side band as sideA r2 + sideB (rho <= r2 / 16 + 4).
static void field_map_bands(const Knobs &kn, FieldMapArgs &a) {
    const double u = 5.9604644775390625e-8, sc = kn.fov_band;
    a.fovA = (float)(sc * 64 * u);
    a.fovB = 0.0f;
    a.sideA = (float)(sc * 0.625 * u);
    a.sideB = (float)(sc * 40 * u);
    a.sideP0 = 0.0f;
    a.sideP1 = (float)(sc * 10 * u);
}

constexpr int64_t FIELD_MAP_CHUNK = 1 << 20;    // probes per copy
constexpr int64_t FIELD_MAP_MAX = 1ll << 31;    // probes per call (the grid: 2^23 workgroups)

// host -> device (to == true) or back, FIELD_MAP_CHUNK probes at a time
static int field_map_copy(csf_engine *e, double *dev, const double *in, double *out, int64_t m, bool to) {
    for (int64_t at = 0; at < m; at += FIELD_MAP_CHUNK) {
        const size_t cnt = (size_t)std::min(FIELD_MAP_CHUNK, m - at) * sizeof(double);
        if (to) HIPCHK(e, hipMemcpy(dev + at, in + at, cnt, hipMemcpyHostToDevice));
        else HIPCHK(e, hipMemcpy(out + at, dev + at, cnt, hipMemcpyDeviceToHost));
    }
    return CSF_OK;
}

}  // extern "C++"

int csf_field_map(csf_engine *e, int64_t m, const double *x, const double *y, const double *psi, uint32_t what, int32_t skip,
                  double *Fx, double *Fy) try {
    if (!e) return CSF_E_ARG;
    if (what == 0 || (what & ~(CSF_FIELD_CROWD | CSF_FIELD_ROAD | CSF_FIELD_FOV)) != 0)
        return fail(e, CSF_E_ARG, "csf_field_map: what must be a combination of CSF_FIELD_CROWD, CSF_FIELD_ROAD and CSF_FIELD_FOV (got 0x%x)", (unsigned)what);
    const bool crowd = (what & CSF_FIELD_CROWD) != 0, road = (what & CSF_FIELD_ROAD) != 0, fov = (what & CSF_FIELD_FOV) != 0;
    if (fov && !crowd) return fail(e, CSF_E_ARG, "csf_field_map: CSF_FIELD_FOV masks the crowd term - it needs CSF_FIELD_CROWD");
    if (m < 0 || m > FIELD_MAP_MAX) return fail(e, CSF_E_ARG, "csf_field_map: m = %lld probes (0 .. 2^31)", (long long)m);
    if (m > 0 && (!x || !y || !Fx || !Fy)) return fail(e, CSF_E_ARG, "csf_field_map: NULL probe or output array");
    if (m > 0 && crowd && !psi) return fail(e, CSF_E_ARG, "csf_field_map: the crowd term needs the probes' headings (psi is NULL)");
    if (skip < -1 || skip >= (int64_t)e->order.size())
        return fail(e, CSF_E_ARG, "csf_field_map: skip = %d is no road user (population of %lld)", skip, (long long)e->order.size());
    if (int crc = calib_refuses(e, "csf_field_map")) return crc;
    // (a foreign source has no fp64 state on a rank, and the map decides on fp64 positions: Dev::state_current)
    if (e->world > 1 || e->loopback || e->nccl != nullptr || !e->state_all_current)
        return fail(e, CSF_E_STATE, "csf_field_map: the engine is a rank of a sharded run or a member of a loopback group - the other ranks' road users have no fp64 state here");
    if (m == 0) return CSF_OK;
    HIPCHK(e, hipSetDevice(e->device));
    int rc = upload_all(e);
    if (rc) return rc;
    if ((rc = csf_sync(e))) return rc;                         // both streams (the side-by-side tick), as the read-backs wait
    if ((rc = sync_order(e))) return rc;
    HIPCHK(e, e->scratch_f64.reserve((size_t)(5 * m)));
    double *const dx = e->scratch_f64.p, *const dy = dx + m, *const dp = dy + m, *const dFx = dp + m, *const dFy = dFx + m;
    if ((rc = field_map_copy(e, dx, x, nullptr, m, true))) return rc;
    if ((rc = field_map_copy(e, dy, y, nullptr, m, true))) return rc;
    if (crowd && (rc = field_map_copy(e, dp, psi, nullptr, m, true))) return rc;
    Dev dd = e->d;                                             // a view: the engine's own Dev is not touched
    dd.state_current = 1;
    FieldMapArgs a{};
    a.x = dx, a.y = dy, a.psi = dp, a.Fx = dFx, a.Fy = dFy, a.m = m;
    a.skip = skip, a.fov = fov ? 1 : 0;
    field_map_bands(e->knobs, a);
    // csf_profile_enable: the launches are timed like a tick's - the crowd launch as kernel 0 (pair), the road launch as kernel 1
    csf_engine::ProfSlot *ps = nullptr;
    if ((rc = prof_take(e, true, &ps))) return rc;
    if (crowd) {
        launch_field_map_crowd(dd, a, e->main, ps ? ps->ev[0] : nullptr, ps ? ps->ev[1] : nullptr);
        if (ps) ps->pair = true;
        e->field_map_launches++;
    }
    if (road) {
        a.accumulate = crowd ? 1 : 0;
        launch_field_map_road(dd, a, e->main, ps ? ps->ev[2] : nullptr, ps ? ps->ev[3] : nullptr);
        if (ps) ps->road = true;
        e->field_map_launches++;
    }
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(e->main));
    if ((rc = field_map_copy(e, dFx, nullptr, Fx, m, false))) return rc;
    return field_map_copy(e, dFy, nullptr, Fy, m, false);
} catch (...) { return csf_caught(e); }

int csf_field_map_launches(const csf_engine *e, int64_t *n_launches) try {
    if (!e || !n_launches) return CSF_E_ARG;
    *n_launches = e->field_map_launches;
    return CSF_OK;
} catch (...) { return csf_caught(e); }
