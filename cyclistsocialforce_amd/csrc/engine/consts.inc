// engine/consts.inc - errors, parameter checks, the far-field radius, the rounding bands of a tick, what the kernels derive from a parameter set.
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

namespace {

int fail(csf_engine *e, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (e) e->err = buf;
    else g_create_error = buf;
    return code;
}

// an engine that holds a calibration data set (csf_calib_load, csf_scene_calib_load) is evaluated, read, given destination queues and cleared - nothing else
int calib_refuses(csf_engine *e, const char *what) {
    if (!e || (!e->calib && !e->scene_calib)) return CSF_OK;
    if (e->scene_calib) return fail(e, CSF_E_STATE, "%s: the engine holds a closed-loop calibration data set (csf_scene_calib_clear first)", what);
    return fail(e, CSF_E_STATE, "%s: the engine holds a calibration data set (csf_calib_clear first)", what);
}

constexpr int64_t MAX_QUEUE_ROWS = 1 << 24;   // destinations of ONE road user (row numbers are 32-bit; a route has a few dozen)

// Every extern "C" entry point is a function-try-block that ends here: no C++ exception (a std::bad_alloc of the host mirror's
// vectors, a std::length_error) crosses the C boundary - the caller gets CSF_E_HOST and a sentence.  What the call had
// already changed stays changed: after CSF_E_HOST an engine is good for csf_last_error and csf_destroy only.
int csf_caught(const csf_engine *e) noexcept {
    char msg[256] = "an exception that is no std::exception";
    try {
        throw;
    } catch (const std::bad_alloc &) {
        snprintf(msg, sizeof msg, "the host ran out of memory (std::bad_alloc)");
    } catch (const std::exception &ex) {
        snprintf(msg, sizeof msg, "%s", ex.what());
    } catch (...) {
    }
    try {
        return fail(const_cast<csf_engine *>(e), CSF_E_HOST, "C++ exception at the C boundary: %s", msg);
    } catch (...) {       // (the message itself could not be stored)
        return CSF_E_HOST;
    }
}

#define HIPCHK(e, call)                                                                           \
    do {                                                                                          \
        hipError_t _r = (call);                                                                   \
        if (_r != hipSuccess)                                                                     \
            return fail(e, CSF_E_DEVICE, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_r), __FILE__, __LINE__); \
    } while (0)

#define NCCLCHK(e, call)                                                                          \
    do {                                                                                          \
        ncclResult_t _r = (call);                                                                 \
        if (_r != ncclSuccess)                                                                    \
            return fail(e, CSF_E_COMM, "%s failed: %s", #call, g_rccl.GetErrorString(_r));        \
    } while (0)

const int NS_OF[7] = {5, 5, 6, 4, 5, 4, 8};
// Ticks between two re-binnings.  The circles of the batches are renewed EVERY tick from the positions as they are (the pair
// kernel emits them), so a stale order costs only what the batches' members drift apart: the pair kernel takes the same
// 105 us with 32, 48 and 64 ticks and 0.3 - 0.5 us more with 96 / 128, while the re-binning itself (~40 us of sort, rebase
// and launch gaps) is paid half as often: 64 (round 4: +0.5 % over 32; profiles/r4_rebin_period_ab.txt).
constexpr int64_t REBIN_TICKS = 64;     // (default of Knobs::rebin_ticks)
int32_t pair_variant_for(const csf_engine *e, int64_t n);   // (with rebin, below)

double limit_angle_h(double th) {  // utils.py:124-139 (host: Vehicle.__init__, vehicle.py:154-155)
    const double PI = 3.141592653589793238462643383279502884;
    th = std::floor(th / (2 * PI)) * (-2 * PI) + th;
    if (th > PI) th -= 2 * PI;
    else if (th < -PI) th += 2 * PI;
    return th;
}

int check_params(csf_engine *e, const csf_params *p) {
    if (!p) return fail(e, CSF_E_ARG, "params is NULL");
    if (p->model < 0 || p->model > 6) return fail(e, CSF_E_ARG, "unknown model %d", p->model);
    {   // a NaN in any number of the parameter set (the doubles lead the struct: include/csf.h): never meant, and it would pass every
        // range check below as well as the far-field bound's
        const double *v = (const double *)p;
        for (size_t k = 0; k < offsetof(csf_params, model) / sizeof(double); k++)
            if (std::isnan(v[k])) return fail(e, CSF_E_ARG, "csf_params: number %d of the struct is NaN", (int)k);
    }
    if (p->model == CSF_PLANARBIKE) {
        const double sum_im = p->pb_poles[1] + p->pb_poles[3], prod_im = p->pb_poles[0] * p->pb_poles[3] + p->pb_poles[1] * p->pb_poles[2];
        if (std::fabs(sum_im) > 1e-12 || std::fabs(prod_im) > 1e-12 || !(p->pb_poles[0] < 0) || !(p->pb_poles[2] < 0))
            return fail(e, CSF_E_ARG, "PlanarBicycle needs two stable poles, real or a conjugate pair");
        if (!(p->l > 0)) return fail(e, CSF_E_ARG, "PlanarBicycle needs a wheelbase l > 0");
    }
    if (!(p->t_s > 0)) return fail(e, CSF_E_ARG, "t_s must be > 0");
    if (p->traj_len < 2) return fail(e, CSF_E_ARG, "traj_len must be >= 2 (int(30/t_s) in the reference)");
    if (p->priority_rule < 0 || p->priority_rule > 1) return fail(e, CSF_E_ARG, "unknown priority rule");
    if (!(p->hfov >= 0)) return fail(e, CSF_E_ARG, "hfov must be >= 0");
    return CSF_OK;
}

// Far-field radius of the TwoD field (vehicle.py:1560-1648).  |F| = f_0 exp(-rho q / sigma) with
// q = sqrt(1 - e^2 cos^2 phi), sigma = sga - sgb |sin(phi/2)|, all functions of s2 = sin^2(psi0 - psi) in [0, 1] and of
// phi: kappa = min q / sigma bounds the decay from below, so every source beyond
//     R = ln(n / far_eps) / kappa
// adds less than far_eps f_0 / n, and all of them together less than far_eps f_0, to a receiver's column sum.
// far_eps defaults to 2^-24 (half an fp32 ulp of f_0; CSF_FAR_EPS overrides, 0 switches the cull off): what is
// left out is below the rounding of the fp32 sum it would have been added to.  Batches of binned records
// whose bounding circle lies entirely beyond R are skipped by the pair kernel (DESIGN.md, D8).
double far_kappa(const csf_params &p) {
    if (p.model == CSF_BICYCLE) return 0.0;
    double kappa = INFINITY;
    for (int i = 0; i <= 256; i++) {
        const double s2 = i / 256.0;
        const double e = p.e_0 - p.e_1 * s2, sga = p.sigma_0 + p.sigma_1 * s2, sgb = p.sigma_2 + p.sigma_3 * s2;
        for (int j = 0; j <= 512; j++) {
            const double phi = 3.141592653589793 * j / 512.0;
            const double q2 = 1.0 - e * e * std::cos(phi) * std::cos(phi), sigma = sga - sgb * std::sin(0.5 * phi);
            if (!(sigma > 0) || !(q2 > 0)) return 0.0;   // degenerate parameters: no usable bound
            kappa = std::min(kappa, std::sqrt(q2) / sigma);
        }
    }
    return std::isfinite(kappa) ? 0.98 * kappa : 0.0;  // the grid is fine but finite
}

double far_radius(double kappa, int64_t n, double far_eps) {
    if (!(far_eps > 0) || !(kappa > 0) || n < 1) return INFINITY;
    return std::log((double)n / far_eps) / kappa;
}

// Per-pair form of the same bound.  A pair adds f_0 exp(-x), x = rho q / sigma (vehicle.py:1628), and may be left out
// when x > T = ln(n / far_eps): then it is below far_eps f_0 / n like every source beyond the far-field radius.  With
// X = rho cos(phi) (the receiver along the source's heading), rho^2 q^2 = rho^2 - e^2 X^2 exactly, and
// sigma = sigma_a - sigma_b |sin(phi/2)| <= sigma_a - sigma_b (1 - cos phi) / 2 because |sin(phi/2)| <= 1; so
//     rho^2 - e^2 X^2 > T^2 (sigma_a - sigma_b / 2 + (sigma_b / 2) X / rho)^2   implies   x > T.
// The kernel evaluates this with one rsq per pair (csf_pair.hip: keep_x2); T carries a 0.2 % margin against the fp32
// rounding of the two sides.  At N = 16 384 in 200 m the test removes three of four pairs that pass the field of view.
// far-field radius and reach-test constants of one parameter set in a population of n road users
void set_far_consts(const Knobs &kn, const csf_params &p, double kappa, int64_t n, PairConsts &k) {
    const double eps = kn.far_eps;
    k.rfar = (float)far_radius(kappa, n, eps);
    // (sigma_b >= 0 is what the bound sigma <= sigma_a - sigma_b (1 - cos phi) / 2 rests on; the reference's setters enforce
    // it, the C ABI does not: a set with a negative sigma_2 / sigma_3 keeps the radius-only cull)
    const bool on = std::isfinite(k.rfar) && p.model != CSF_BICYCLE && n >= 1 && p.sigma_2 < p.sigma_0 && p.sigma_3 < p.sigma_1 &&
                    p.sigma_2 >= 0 && p.sigma_3 >= 0 && p.sigma_2 + p.sigma_3 >= 0 && kn.reach;
    k.reach = on;
    if (on) {
        const double T = std::log((double)n / eps) * 1.002;
        k.tA0 = (float)(T * (p.sigma_0 - 0.5 * p.sigma_2));
        k.tA1 = (float)(T * (p.sigma_1 - 0.5 * p.sigma_3));
        k.tB0 = (float)(T * 0.5 * p.sigma_2);
        k.tB1 = (float)(T * 0.5 * p.sigma_3);
    } else {
        k.tA0 = k.tA1 = k.tB0 = k.tB1 = 0.f;
    }
}

// set_far_consts with ln(n / eps) replaced by T
static void set_far_consts_T(const csf_params &p, double kappa, double T, PairConsts &k) {
    k.rfar = (float)(T / kappa);
    if (k.reach) {
        const double Tm = T * 1.002;
        k.tA0 = (float)(Tm * (p.sigma_0 - 0.5 * p.sigma_2));
        k.tA1 = (float)(Tm * (p.sigma_1 - 0.5 * p.sigma_3));
        k.tB0 = (float)(Tm * 0.5 * p.sigma_2);
        k.tB1 = (float)(Tm * 0.5 * p.sigma_3);
    }
}

void update_far_radius(csf_engine *e) {   // depends on the parameters and on the population size
    e->far_T = 0.0;
    PairConsts &k = e->d.pc;
    if (e->classes.size() > 1) {          // several parameter sets: the plain kernel, or one launch per set with its own
        k.rfar = INFINITY;                // constants (Segment::pc)
        k.reach = 0;
        k.tA0 = k.tA1 = k.tB0 = k.tB1 = 0.f;
        return;
    }
    set_far_consts(e->knobs, e->d.p, e->far_kappa, e->d.n, k);
}

// The rounding band of the fp32 field-of-view test (csf_dev.h: PairConsts::fovA ...; csf_field.h: keep_x2, tracked_m), for the
// pair launches that follow.  With u = 2^-24: a position in a tile is off by eps_p = u * (largest |coordinate|) per
// component (offset + origin rounded once), a heading (cos, sin) by u per component; t = rho cos(bearing) is then off by
// < 3 eps_p + 5 u rho and g = t|t| + chs rho^2 by < 12 eps_p rho + 18 u rho^2.  Twice that, with rho <= r2 / 16 + 4:
//     band = (36 u + 1.5 eps_p) r2 + 96 eps_p;   side test (priority to the right): 0.625 u r2 + 6 eps_p + 40 u
// (tracked_m: the plain kernels).  The packed test of the cull-first kernel (keep_x2) compares cos(bearing) = t rsq(rho^2)
// with cos(hfov / 2): off by < 3 eps_p / rho + 8 u (the rsq included); twice that is its band, and that of sin(bearing).
// A pair formed from the precise records (offsets of at most a few metres from origins whose difference is exact) has
// eps_p = u * (largest offset), and its band is evaluated with rho itself: 24 eps_p rho + 36 u r2; 6 eps_p + 10 u rho.
// the bands themselves, for positions whose coordinates stay below cmax and road users that move at most `step` per tick
void fov_band_consts(const Knobs &kn, double step, double cmax, PairConsts &k) {
    const double u = 5.9604644775390625e-8;
    const double eps_p = u * cmax * 1.01 + 4 * u;
    // (full circle: chs = 4, g > 3 r2 - never inside a band that small)
    const double sc = kn.fov_band;
    k.fovA = (float)(sc * (36 * u + 1.5 * eps_p));
    k.fovB = (float)(sc * 96 * eps_p);
    k.sideA = (float)(sc * 0.625 * u);
    k.sideB = (float)(sc * (6 * eps_p + 40 * u));
    k.fovT0 = (float)(sc * 16 * u);
    k.fovT1 = (float)(sc * 6 * eps_p);
    // whole batches are classified against the field-of-view cone with a margin of 1e-4 in the cosine (csf_pair.hip:
    // classify_batch): the bearing of a source nearer than 2.9 u (coordinates) / 5e-5 is not known that well in fp32, so a
    // batch whose circle comes closer goes to the per-lane test
    k.clsk = (float)(2.9 * u * 1.01 / 5e-5);
    // offsets: a quarter-metre grid of origins + what a road user covers between two re-binnings (REBIN_TICKS steps + a few;
    // arrivals take their position as their origin)
    const double off = 0.25 + step * (double)(kn.rebin_ticks + 8);
    const double eps_o = u * off * 1.5;
    k.fovP1 = (float)(sc * 24 * eps_o);
    k.fovP2 = (float)(sc * 36 * u);
    k.sideP0 = (float)(sc * 6 * eps_o);
    k.sideP1 = (float)(sc * 10 * u);
}

int set_fov_band(csf_engine *e) {
    Dev &d = e->d;
    if (e->bound_stale) {   // (single device: every slot's state is here)
        // (through a pinned buffer: the first copy into pageable memory of a process costs ~9 ms - the runtime sets its staging
        // path up - and a population that is only ever stepped met it here, in the middle of a run: tick 4 096 of config 2)
        // (csf_create made it: alloc_all)
        HIPCHK(e, hipMemcpyAsync(e->bound_pin.p, e->s.p, 2 * (size_t)e->cap * sizeof(double), hipMemcpyDeviceToHost, e->main));
        HIPCHK(e, hipStreamSynchronize(e->main));
        const double *xy = e->bound_pin.p;
        double cb = e->coord_bound0;
        for (int32_t a : e->order) {
            const double bx = std::fabs(xy[(size_t)a] - d.ox), by = std::fabs(xy[(size_t)e->cap + (size_t)a] - d.oy);
            if (std::isfinite(bx) && std::isfinite(by)) cb = std::max({cb, bx, by});
        }
        e->coord_bound0 = cb;
        e->moves = 0;
        e->bound_stale = false;
    }
    double vmax = 0;
    for (const csf_params &c : e->classes)
        vmax = std::max({vmax, std::fabs(c.v_max_riding[0]), std::fabs(c.v_max_riding[1]), std::fabs(c.v_max_walk)});
    const double step = d.p.t_s * vmax * 1.01 + 1e-4;
    // receivers in binned order work relative to the origin of their group: up to twice the bound from the scene origin
    double cmax = e->coord_bound0 + step * (double)(e->moves + 2) + 1.0;
    // receivers in binned order work relative to the origin of their group: at most twice the bound from the scene origin
    // (a tighter one - far-field radius + the extent of a group and of a batch - would need the circles, which only the
    // device knows; the band only decides how many pairs take the exact path, a few per thousand receivers either way)
    if (d.recv_binned) cmax *= 2.0;
    PairConsts &k = d.pc;
    fov_band_consts(e->knobs, step, cmax, k);
    for (csf_engine::Segment &sg : e->segs) {
        sg.pc.fovA = k.fovA, sg.pc.fovB = k.fovB, sg.pc.sideA = k.sideA, sg.pc.sideB = k.sideB;
        sg.pc.fovT0 = k.fovT0, sg.pc.fovT1 = k.fovT1, sg.pc.clsk = k.clsk;
        sg.pc.fovP1 = k.fovP1, sg.pc.fovP2 = k.fovP2, sg.pc.sideP0 = k.sideP0, sg.pc.sideP1 = k.sideP1;
    }
    d.state_current = e->state_all_current ? 1 : 0;
    d.edge = e->edge.p;
    d.edge_stamp = ++e->edge_stamp;
    d.keep_lo = (e->world > 1 || e->loopback || e->nccl != nullptr) ? 1 : 0;
    return CSF_OK;
}

// exp(A) of a small dense matrix (n <= 4, row major): scaling and squaring of a degree-18 Taylor polynomial
void expm_small(int n, const double *A, double *E) {
    double nrm = 0;
    for (int i = 0; i < n * n; i++) nrm = std::max(nrm, std::fabs(A[i]));
    int sq = 0;
    while (nrm * n > 0.25 && sq < 60) nrm *= 0.5, sq++;
    const double sc = std::ldexp(1.0, -sq);
    double M[16], T[16], P[16];
    for (int i = 0; i < n * n; i++) M[i] = A[i] * sc;
    for (int i = 0; i < n * n; i++) E[i] = (i / n == i % n) ? 1.0 : 0.0, P[i] = E[i];
    for (int k = 1; k <= 18; k++) {
        for (int r = 0; r < n; r++)
            for (int c = 0; c < n; c++) {
                double acc = 0;
                for (int q = 0; q < n; q++) acc += P[r * n + q] * M[q * n + c];
                T[r * n + c] = acc / k;
            }
        for (int i = 0; i < n * n; i++) P[i] = T[i], E[i] += T[i];
    }
    for (int it = 0; it < sq; it++) {
        for (int r = 0; r < n; r++)
            for (int c = 0; c < n; c++) {
                double acc = 0;
                for (int q = 0; q < n; q++) acc += E[r * n + q] * E[q * n + c];
                T[r * n + c] = acc;
            }
        for (int i = 0; i < n * n; i++) E[i] = T[i];
    }
}

// PlanarBicycle (dynamics.py:178-258, 1167-1226).  x = (delta, psi), A(v) = [[0, 0], [a, 0]] with a = v / l, B = (1, 0)^T,
// K_x = (k1, k2) places the class's poles p1, p2: s^2 + k1 s + k2 a = (s - p1)(s - p2), so k1 = -(p1 + p2), k2 = p1 p2 / a.
// With z = (a delta, psi) the closed loop reads z' = M z + (a, 0)^T u, M = [[-k1, -p1 p2], [1, 0]] - no speed in M.
// The reference sets K_u = 1 / psi_sim(T), psi_sim the yaw at the end of a simulated response (T = 0 .. 9.99 in steps of
// 0.01, input 0 for ten samples then 1, first-order hold) of the loop with K_u = 1: psi_sim = a G with G the same response
// of z' = M z + (1, 0)^T u.  Hence a K_u = 1 / G and the controlled loop is z' = M z + (1 / G, 0)^T psi_d at EVERY speed:
// one exact step z+ = E z + Gamma psi_d is derived here once; the kernel scales delta by a on the way in and out.
void derive_planarbike(const csf_params &p, double pb[7]) {
    const double k1 = -(p.pb_poles[0] + p.pb_poles[2]), w2 = p.pb_poles[0] * p.pb_poles[2] - p.pb_poles[1] * p.pb_poles[3];
    auto step_matrices = [&](double dt, double Ad[4], double Bd0[2], double Bd1[2]) {   // first-order hold, input (1, 0)^T
        double Mx[16] = {0}, Ex[16];
        Mx[0] = -k1 * dt; Mx[1] = -w2 * dt; Mx[2] = dt;
        Mx[4] = dt;
        Mx[11] = 1.0;
        expm_small(4, Mx, Ex);
        Ad[0] = Ex[0]; Ad[1] = Ex[1]; Ad[2] = Ex[4]; Ad[3] = Ex[5];
        Bd1[0] = Ex[3]; Bd1[1] = Ex[7];
        Bd0[0] = Ex[2] - Bd1[0]; Bd0[1] = Ex[6] - Bd1[1];
    };
    double Ad[4], Bd0[2], Bd1[2];
    step_matrices(0.01, Ad, Bd0, Bd1);                         // from_pole_placement's own t_s = 0.01, t_end = 10
    double z0 = 0, z1 = 0;
    for (int i = 1; i < 1000; i++) {
        const double u0 = (i - 1) >= 10 ? 1.0 : 0.0, u1 = i >= 10 ? 1.0 : 0.0;
        const double n0 = Ad[0] * z0 + Ad[1] * z1 + Bd0[0] * u0 + Bd1[0] * u1;
        const double n1 = Ad[2] * z0 + Ad[3] * z1 + Bd0[1] * u0 + Bd1[1] * u1;
        z0 = n0, z1 = n1;
    }
    const double G = z1;
    step_matrices(p.t_s, Ad, Bd0, Bd1);                        // forced_response over [0, t_s], input psi_d at both ends
    for (int i = 0; i < 4; i++) pb[i] = Ad[i];
    pb[4] = (Bd0[0] + Bd1[0]) / G;
    pb[5] = (Bd0[1] + Bd1[1]) / G;
    pb[6] = std::exp(-p.k_p_v * p.t_s);                        // dynamics.py:156
}

// what the pair kernels need of one parameter set
void derive_pair_consts(const csf_params &p, PairConsts &k, double rnear) {
    k.sg0 = (float)p.sigma_0;
    k.sg1 = (float)p.sigma_1;
    k.sg2 = (float)p.sigma_2;
    k.sg3 = (float)p.sigma_3;
    k.e0 = (float)p.e_0;
    k.e1 = (float)p.e_1;
    k.kexp = 1.4426950408889634f;
    const double PI_ = 3.141592653589793;
    double ch = std::cos(0.5 * std::min(p.hfov, 2 * PI_));
    k.chs = (float)(p.hfov <= PI_ ? -ch * ch : ch * ch);
    if (p.hfov >= 2 * PI_) k.chs = 4.0f;  // full circle: every bearing is inside (t|t| + 4 rho^2 > 0)
    k.ch = (float)ch;
    k.chm = k.ch - 1e-4f;
    k.chp = k.ch + 1e-4f;
    k.chk = p.hfov >= 2 * PI_ ? -2.0f : (float)ch;      // (keep_x2: cos(bearing) > chk)
    k.p2r = p.priority_rule == CSF_P2R;
    if (p.model == CSF_BICYCLE) {
        k.lf0 = (float)std::log2(p.p_0 / p.p_decay);
        k.ipd = (float)(1.0 / p.p_decay);
        k.f0_zero = 0;
    } else {
        k.lf0 = p.f_0 > 0 ? (float)std::log2(p.f_0) : -INFINITY;
        k.ipd = 0.f;
        k.f0_zero = p.f_0 == 0.0;
    }
    k.full_circle = p.hfov >= 2 * PI_;
    k.fov_classify = 1;   // any field of view: csf_pair.hip guards the wide ones (set to 0 to fall back to exact tests)
    k.rfar = INFINITY;
    k.tA0 = k.tA1 = k.tB0 = k.tB1 = 0.f;
    k.reach = 0;
    k.rnear = (float)std::max(0.0, rnear);
    k.rnear2 = k.rnear * k.rnear;
    k.rn2big = 1e20f * k.rnear2;
}

void derive_consts(csf_engine *e) {
    const csf_params &p = e->d.p;
    if (p.model == CSF_PLANARBIKE) derive_planarbike(p, e->d.pb);
    derive_pair_consts(p, e->d.pc, e->knobs.rnear);
    e->far_kappa = far_kappa(p);
    update_far_radius(e);
    if (e->classes.empty()) e->classes.push_back(p);
    e->classes[0] = p;
    e->d.n_classes = (int32_t)e->classes.size();
    e->classes_dirty = true;
    e->d.pair_variant = pair_variant_for(e, e->d.n_live);
    {   // no rider model moves faster than its speed clamp (vehicle.py:1258, 1876, 1905; dynamics.py:1025)
        double vmax = 0;
        for (const csf_params &c : e->classes)
            vmax = std::max({vmax, std::fabs(c.v_max_riding[0]), std::fabs(c.v_max_riding[1]), std::fabs(c.v_max_walk)});
        e->d.bnd_margin = (float)(p.t_s * vmax * 1.01 + 1e-4);
    }
    e->d.back = (int32_t)(1.0 / p.t_s);
    int hl = 4;
    while (hl < e->d.back + 2) hl *= 2;
    e->d.hist_len = hl;
    e->d.ns = 0;
    e->d.model_mask = 0;
    for (const csf_params &c : e->classes) {
        e->d.ns = std::max(e->d.ns, NS_OF[c.model]);            // (several vehicle classes: the widest state; unused ones stay 0)
        e->d.model_mask |= 1 << c.model;
    }
    e->d.has_bike = e->d.model_mask & 1;
}
