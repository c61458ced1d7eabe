// csf_body.hip — body encounters of a recording (csf_body_encounters, csf_batch_body_encounters): the free gap and the constant-velocity
// time to contact between the road users' OUTLINES, every road user an oriented rectangle of its own extents (front, rear, half
// width), where csf_encounter.hip has discs of one radius.  The definitions are include/csf.h's, operation for operation.
//
// The mapping is encounter_kernel's: ONE RECEIVER PER LANE, its centre, velocity, heading and half extents in registers, the sources of
// the same sample in LDS tiles of 256 that every lane of a wave reads at the same address at the same time (a broadcast).  A source is
// staged once per sample by one thread - centre, velocity, (cos, sin), (L, W), the bounding radius sqrt(L L + W W), a live flag: one
// sincos and one sqrt per source, not per pair.  A lane forms its minima in population order with a strict `<` and no cross-lane
// reduction: its row is the same bits whatever else is in the launch.  Everything is fp64, nothing is contracted.
//
// body_kernel<EVENTS>   grid (x, y, members), 256 threads; BodyDesc::m says where the samples are and where the results go, exactly
//     as EncDesc does for encounter_kernel: n > 32 a tile of 256 receivers x (sample, chunk of sources), n <= 32 the cells (sample,
//     rider) packed into the lanes of a workgroup.
//     The pair by the definition costs four axes, eight corners and eight divisions; it sits behind two filters on the bounding discs
//     (radius rad_i + rad_j around the centres, which hold the outlines), each 20-odd operations:
//       gap:  the outlines are at least |w| - (rad_i + rad_j) apart, so a pair with |w|^2 above (best + rad_i + rad_j)^2, widened by
//             2e-9, cannot have the smaller gap - and once the best gap is 0 nothing can;
//       ttc:  the outlines meet no sooner than the discs, and the discs no sooner than q / (-2 b) (enc_pair's bound), so a pair whose
//             discs never meet, or not before the best ttc, cannot have the smaller ttc.  q is formed from |w|^2 narrowed by 2e-9 and the
//             discriminant is let be negative by 1e-9 b^2, so that a pair the discs decide by a rounding error passes.
//     With events a pair (i < j) is also tested against the thresholds.  A filter changes no bit: a pair that passes any of them is
//     decided by the definition itself, both values, compared with `<`; a pair that fails all of them is larger than the minimum so
//     far on both counts and under no threshold.
//     EVENTS: a pair (i < j) under a threshold is stored by the lane of i; a wave reserves its slots with ballot, popcount, one
//     atomicAdd by its first such lane and a broadcast of the base; slots past the capacity are counted, not written.
// body_window_kernel    the second launch: thread = rider, the samples in order with a strict `<` - the earliest sample wins a tie -,
//     the chunks of a split sample combined first, in chunk order, and the samples with gap_min == 0 counted.
#include "csf_dev.h"

namespace csf {

constexpr int BODY_BLOCK = 256;
constexpr int BODY_TILE = 256;     // sources per LDS tile: one per thread of the fill
constexpr int BODY_WBLOCK = 64;    // riders per workgroup of the window pass

struct BodySrc {
    double mx, my, ux, uy, cs, sn, L, W, rad;
    bool live;
};

struct BodyHead {
    double cs, sn;
    bool live;
};

// (cos, sin) of a heading; live: x, y, psi, v are all finite.  A CALL, once per source and sample, as enc_source is (inlined, its
// sincos sets the kernel's scalar register count); it returns in registers, which the whole BodySrc would not
__device__ __attribute__((noinline)) BodyHead body_heading(double x, double y, double psi, double v) {
    BodyHead r;
    r.live = isfinite(x) && isfinite(y) && isfinite(psi) && isfinite(v);
    r.sn = 0.0, r.cs = 1.0;
    if (r.live) sincos(psi, &r.sn, &r.cs);
    return r;
}

// include/csf.h "Outline": centre, velocity, heading and half extents from a state's rows 0 - 3 and the extents
__device__ __forceinline__ BodySrc body_source(double x, double y, double psi, double v, double front, double rear, double hw) {
#pragma clang fp contract(off)
    const BodyHead h = body_heading(x, y, psi, v);
    BodySrc r;
    r.live = h.live;
    const double o = 0.5 * (front - rear);
    r.cs = h.cs, r.sn = h.sn;
    r.L = 0.5 * (front + rear), r.W = hw;
    r.mx = x + o * h.cs, r.my = y + o * h.sn;
    r.ux = v * h.cs, r.uy = v * h.sn;
    r.rad = sqrt(r.L * r.L + r.W * r.W);
    return r;
}

// road user u in sample k of the member
__device__ __forceinline__ BodySrc body_load(const BodyDesc &b, int k, int u) {
    const EncDesc &m = b.m;
    double x, y, psi, v;
    if (m.ring) {
        int slot = m.first + k;
        if (slot >= m.cap) slot -= m.cap;
        const double *p = m.s + ((int64_t)slot * m.n + u) * m.ns;
        x = p[0], y = p[1], psi = p[2], v = p[3];
    } else {
        const int64_t slot = m.order ? (int64_t)m.order[u] : (int64_t)u;
        x = m.s[slot], y = m.s[m.stride + slot], psi = m.s[2 * m.stride + slot], v = m.s[3 * m.stride + slot];
    }
    const double *e = b.ext + 3 * (int64_t)u;
    return body_source(x, y, psi, v, e[0], e[1], e[2]);
}

// include/csf.h "Gap": one corner (a L, b W) of the other body, given in the frame of the box (bl, bw) whose centre is (-s0, -s1) away
__device__ __forceinline__ double body_corner(double s0, double s1, double aL, double bW, double cr, double sr, double bl, double bw) {
#pragma clang fp contract(off)
    const double X = s0 + (aL * cr - bW * sr), Y = s1 + (aL * sr + bW * cr);
    const double dx = fmax(fabs(X) - bl, 0.0), dy = fmax(fabs(Y) - bw, 0.0);
    return dx * dx + dy * dy;
}

// include/csf.h "Time to contact": one axis
__device__ __forceinline__ void body_axis(double s, double g, double r, bool &never, double &t_in, double &t_out) {
#pragma clang fp contract(off)
    if (g == 0.0) {
        if (fabs(s) > r) never = true;
    } else {
        const double ta = (-r - s) / g, tb = (r - s) / g;
        const double enter = ta < tb ? ta : tb, leave = ta < tb ? tb : ta;
        if (enter > t_in) t_in = enter;
        if (leave < t_out) t_out = leave;
    }
}

// include/csf.h "Pair (i, j)": gap and ttc of receiver p (= i) and source s (= j); w = m_j - m_i, c = u_j - u_i
__device__ __forceinline__ void body_exact(const BodySrc &p, const double2 sh, const double2 sl, double wx, double wy, double cx, double cy,
                                           double &gap, double &ttc) {
#pragma clang fp contract(off)
    const double cr = p.cs * sh.x + p.sn * sh.y, sr = p.cs * sh.y - p.sn * sh.x;
    const double acr = fabs(cr), asr = fabs(sr);
    const double s0 = wx * p.cs + wy * p.sn, s1 = wy * p.cs - wx * p.sn, s2 = wx * sh.x + wy * sh.y, s3 = wy * sh.x - wx * sh.y;
    const double Li = p.L, Wi = p.W, Lj = sl.x, Wj = sl.y;
    const double r0 = Li + (Lj * acr + Wj * asr), r1 = Wi + (Lj * asr + Wj * acr);
    const double r2 = Lj + (Li * acr + Wi * asr), r3 = Wj + (Li * asr + Wi * acr);
    const double sep = fmax(fmax(fabs(s0) - r0, fabs(s1) - r1), fmax(fabs(s2) - r2, fabs(s3) - r3));
    if (sep <= 0.0) {
        gap = 0.0, ttc = 0.0;
        return;
    }
    double d2 = INFINITY;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const double a = (c & 2) ? -1.0 : 1.0, b = (c & 1) ? -1.0 : 1.0;
        const double dj = body_corner(s0, s1, a * Lj, b * Wj, cr, sr, Li, Wi);        // a corner of j in the frame of i
        const double di = body_corner(-s2, -s3, a * Li, b * Wi, cr, -sr, Lj, Wj);     // a corner of i in the frame of j
        if (dj < d2) d2 = dj;
        if (di < d2) d2 = di;
    }
    gap = sqrt(d2);
    const double g0 = cx * p.cs + cy * p.sn, g1 = cy * p.cs - cx * p.sn, g2 = cx * sh.x + cy * sh.y, g3 = cy * sh.x - cx * sh.y;
    bool never = false;
    double t_in = -INFINITY, t_out = INFINITY;
    body_axis(s0, g0, r0, never, t_in, t_out);
    body_axis(s1, g1, r1, never, t_in, t_out);
    body_axis(s2, g2, r2, never, t_in, t_out);
    body_axis(s3, g3, r3, never, t_in, t_out);
    ttc = (never || t_in > t_out || t_in < 0.0) ? INFINITY : t_in;
}

struct BodyBest {
    double g, t;
    int32_t gj, tj;
};

// where the events of the workgroup's member go
struct BodyEv {
    csf_body_event *ev;
    unsigned long long *count;
    unsigned long long cap;
};

// One pair: receiver p = road user `me` of sample `k`, source = slot of the tile = road user uj.
template <bool EVENTS>
__device__ __forceinline__ void body_pair(const BodyArgs &a, const BodyEv &e, const double2 sm, const double2 su, const double2 sh, const double2 sl,
                                          const double srad, const bool ok, const BodySrc &p, const int me, const int uj, const int k, BodyBest &best) {
#pragma clang fp contract(off)
    const double wx = sm.x - p.mx, wy = sm.y - p.my, cx = su.x - p.ux, cy = su.y - p.uy;
    const double ww = wx * wx + wy * wy, ca = cx * cx + cy * cy, cb = wx * cx + wy * cy;
    const double rr = p.rad + srad;
    // the gap: |w| - rr bounds it from below
    const double bg = best.g + rr;
    bool pass = ok & (best.g > 0.0) & (ww <= bg * bg * 1.000000002);
    // the ttc: the bounding discs' (enc_pair), with q narrowed
    const double q = ww * 0.999999998 - rr * rr;
    const double bb = cb * cb;
    const bool meets = ok & ((q <= 0.0) | ((cb < 0.0) & (bb - ca * q >= -1e-9 * bb)));
    double tlim = best.t;
    if (EVENTS) {
        if (uj > me) {
            tlim = fmax(tlim, a.ttc_event);
            const double be = a.gap_event + rr;                // (gap_event < 0: off)
            pass |= ok & (a.gap_event >= 0.0) & (ww <= be * be * 1.000000002);
        }
    }
    pass |= meets & (tlim > 0.0) & ((q <= 0.0) | (q * 0.999999 <= tlim * (-2.0 * cb)));
    if (pass) {
        double g, t;
        body_exact(p, sh, sl, wx, wy, cx, cy, g, t);
        if (g < best.g) best.g = g, best.gj = uj;
        if (t < best.t) best.t = t, best.tj = uj;
        if (EVENTS) {
            const bool hit = (uj > me) & (((a.gap_event >= 0.0) & (g <= a.gap_event)) | (t < a.ttc_event));
            const unsigned long long mask = __ballot(hit);
            if (mask) {
                const int lane = (int)(threadIdx.x & 63);
                const int leader = __ffsll((long long)mask) - 1;
                unsigned long long base = 0;
                if (lane == leader) base = atomicAdd(e.count, (unsigned long long)__popcll(mask));
                base = __shfl(base, leader, 64);
                if (hit) {
                    const unsigned long long at = base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
                    if (at < e.cap) {
                        csf_body_event ev;
                        ev.sample = k;                         // (within the call: the host adds the index of the first sample)
                        ev.i = me, ev.j = uj, ev.gap = g, ev.ttc = t;
                        e.ev[at] = ev;
                    }
                }
            }
        }
    }
}

template <bool EVENTS>
__global__ __launch_bounds__(BODY_BLOCK) void body_kernel(const BodyArgs a) {
    __shared__ double2 sm[BODY_TILE], su[BODY_TILE], sh[BODY_TILE], sl[BODY_TILE];
    __shared__ double srad[BODY_TILE];
    __shared__ uint8_t slive[BODY_TILE];
    const BodyDesc bd = a.desc[blockIdx.z];
    const EncDesc &m = bd.m;
    const int n = m.n, t = (int)threadIdx.x;
    if (n <= 0 || m.count <= 0) return;
    const int64_t cells = (int64_t)m.count * n;
    double *const o_g = (double *)(a.out + m.out_off), *const o_t = o_g + cells;
    int32_t *const o_gj = (int32_t *)(o_t + cells + 5 * (int64_t)n), *const o_tj = o_gj + cells;   // (behind the window arrays: BodyDesc)
    BodyBest best{INFINITY, INFINITY, -1, -1};
    const BodyEv ev{(csf_body_event *)(a.out + m.ev_off), a.count + blockIdx.z, (unsigned long long)m.ev_cap};
    if (n <= ENC_SMALL) {
        const int spw = BODY_BLOCK / n;                        // samples per workgroup
        const int64_t b = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        const int64_t k0 = b * spw;
        if (k0 >= m.count) return;                             // (uniform)
        const int ls = t / n, u = t - ls * n;
        const int64_t k = k0 + ls;
        const bool have = ls < spw && k < m.count;
        BodySrc me{0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 1.0, 1.0, false};
        if (have) me = body_load(bd, (int)k, u);
        sm[t] = make_double2(me.mx, me.my);
        su[t] = make_double2(me.ux, me.uy);
        sh[t] = make_double2(me.cs, me.sn);
        sl[t] = make_double2(me.L, me.W);
        srad[t] = me.rad;
        slive[t] = me.live ? 1 : 0;
        __syncthreads();
        if (!have) return;
        if (me.live) {
            const int s0 = ls * n;
            for (int j = 0; j < n; j++)
                body_pair<EVENTS>(a, ev, sm[s0 + j], su[s0 + j], sh[s0 + j], sl[s0 + j], srad[s0 + j], (slive[s0 + j] != 0) & (j != u), me, u, j, (int)k, best);
        }
        const int64_t c = k * n + u;
        o_g[c] = me.live ? best.g : NAN;
        o_t[c] = me.live ? best.t : NAN;
        o_gj[c] = best.gj;
        o_tj[c] = best.tj;
        return;
    }
    // blockIdx.y = (sample, chunk of the sample's sources), as in encounter_kernel
    const int k = (int)blockIdx.y / m.split, chunk = (int)blockIdx.y - k * m.split;
    const int64_t i = (int64_t)blockIdx.x * BODY_BLOCK + t;
    if (k >= m.count || (int64_t)blockIdx.x * BODY_BLOCK >= n) return;   // (uniform: the grid is the largest member's)
    const bool have = i < n;
    const BodySrc me = body_load(bd, k, (int)(have ? i : n - 1));   // (clamped: every thread fills tiles and meets the barriers)
    const int src0 = chunk * m.chunk_tiles * BODY_TILE;
    const int src1 = n - src0 < m.chunk_tiles * BODY_TILE ? n : src0 + m.chunk_tiles * BODY_TILE;
    for (int base = src0; base < src1; base += BODY_TILE) {
        const int cnt = src1 - base < BODY_TILE ? src1 - base : BODY_TILE;
        __syncthreads();
        if (t < cnt) {
            const BodySrc s = body_load(bd, k, base + t);
            sm[t] = make_double2(s.mx, s.my);
            su[t] = make_double2(s.ux, s.uy);
            sh[t] = make_double2(s.cs, s.sn);
            sl[t] = make_double2(s.L, s.W);
            srad[t] = s.rad;
            slive[t] = s.live ? 1 : 0;
        }
        __syncthreads();
        if (!me.live) continue;
        for (int j = 0; j < cnt; j++) {                        // (every lane of a wave reads the same source: LDS broadcasts)
            if (!slive[j]) continue;                           // (uniform)
            body_pair<EVENTS>(a, ev, sm[j], su[j], sh[j], sl[j], srad[j], (int64_t)(base + j) != i, me, (int)i, base + j, k, best);
        }
    }
    if (have) {
        int64_t c = (int64_t)k * n + i;
        double *w_g = o_g, *w_t = o_t;
        int32_t *w_gj = o_gj, *w_tj = o_tj;
        if (m.split > 1) {                                     // the chunk's own arrays (EncDesc::part_off)
            const int64_t all = cells * m.split;
            w_g = (double *)(a.out + m.part_off), w_t = w_g + all, w_gj = (int32_t *)(w_t + all), w_tj = w_gj + all;
            c += chunk * cells;
        }
        w_g[c] = me.live ? best.g : NAN;
        w_t[c] = me.live ? best.t : NAN;
        w_gj[c] = best.gj;
        w_tj[c] = best.tj;
    }
}

__global__ __launch_bounds__(BODY_WBLOCK) void body_window_kernel(const BodyArgs a) {
    const EncDesc m = a.desc[blockIdx.z].m;
    const int n = m.n;
    const int64_t u = (int64_t)blockIdx.x * BODY_WBLOCK + threadIdx.x;
    if (u >= n || m.count <= 0) return;
    const int64_t cells = (int64_t)m.count * n;
    double *const o_g = (double *)(a.out + m.out_off), *const o_t = o_g + cells;
    double *const r_g = (double *)(o_t + cells), *const r_t = r_g + n;
    int64_t *const r_gs = (int64_t *)(r_t + n), *const r_ts = r_gs + n, *const r_ov = r_ts + n;
    int32_t *const o_gj = (int32_t *)(r_ov + n), *const o_tj = o_gj + cells;
    int32_t *const r_gj = (int32_t *)(o_tj + cells), *const r_tj = r_gj + n;
    const int64_t all = cells * m.split;
    const double *const p_g = (const double *)(a.out + m.part_off), *const p_t = p_g + all;
    const int32_t *const p_gj = (const int32_t *)(p_t + all), *const p_tj = p_gj + all;
    double bg = INFINITY, bt = INFINITY;
    int32_t gj = -1, tj = -1;
    int64_t gs = -1, ts = -1, ov = 0;
    for (int k = 0; k < m.count; k++) {                        // (a NaN row - the rider was not finite in that sample - is never `<`)
        const int64_t c = (int64_t)k * n + u;
        double g, tt;
        int32_t wg, wt;
        if (m.split > 1) {                                     // the chunks of the sample's sources, in order: the lowest j keeps a tie
            g = p_g[c], tt = p_t[c], wg = p_gj[c], wt = p_tj[c];
            for (int q = 1; q < m.split; q++) {
                const int64_t cq = c + q * cells;
                const double gq = p_g[cq], tq = p_t[cq];
                if (gq < g) g = gq, wg = p_gj[cq];
                if (tq < tt) tt = tq, wt = p_tj[cq];
            }
            o_g[c] = g, o_t[c] = tt, o_gj[c] = wg, o_tj[c] = wt;
        } else {
            g = o_g[c], tt = o_t[c], wg = o_gj[c], wt = o_tj[c];
        }
        if (g < bg) bg = g, gj = wg, gs = k;
        if (tt < bt) bt = tt, tj = wt, ts = k;
        if (g == 0.0) ov++;
    }
    r_g[u] = bg, r_t[u] = bt, r_gj[u] = gj, r_tj[u] = tj, r_ov[u] = ov;
    r_gs[u] = (gs < 0 || m.first_abs < 0) ? -1 : m.first_abs + gs;   // (the current state is sample -1)
    r_ts[u] = (ts < 0 || m.first_abs < 0) ? -1 : m.first_abs + ts;
}

void launch_body(const BodyArgs &a, bool events, dim3 grid, int members, int max_n, hipStream_t st, hipEvent_t t0, hipEvent_t t1) {
    if (members <= 0 || max_n <= 0) return;
    if (events) hipExtLaunchKernelGGL(body_kernel<true>, grid, dim3(BODY_BLOCK), 0, st, t0, t1, 0, a);
    else hipExtLaunchKernelGGL(body_kernel<false>, grid, dim3(BODY_BLOCK), 0, st, t0, t1, 0, a);
    hipLaunchKernelGGL(body_window_kernel, dim3((unsigned)((max_n + BODY_WBLOCK - 1) / BODY_WBLOCK), 1, (unsigned)members), dim3(BODY_WBLOCK), 0, st, a);
}

}  // namespace csf
