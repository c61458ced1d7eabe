// csf_fieldmap.hip — the force field at arbitrary probe points (csf_field_map): what a road user WOULD feel there.
//
// The reference inspects a scene by evaluating calcRepulsiveForce on a meshgrid (scenarios/curve-scenario.py:90-125): the road
// elements' term (intersection.py:226-242) and every road user's field (vehicle.py:1054-1147, 1560-1648).  A map has up to
// millions of probes and often three sources, so the mapping is the opposite of plain_pair_sums (csf_pair_dev.h): ONE PROBE PER
// LANE, its fp64 (x, y, psi) in registers, the sources / vertices in LDS tiles that every lane of a wave reads at the same
// address at the same time (a broadcast: no bank conflicts).  Workgroups of 256 threads, grid = ceil(m / 256), one launch per term.
//
// A probe's sum is formed by its own lane in a fixed order - population order for the crowd, vertex order for the road - with no
// cross-lane reduction: its result is the same bits whatever else is in the call.
//
// field_map_crowd_kernel<P2R>   sum of the live road users' fields, each the field of ITS class with ITS parameter set (the table
//     of PairConsts in LDS, as plain_pair_sums<.., HET> holds it).  (dx, dy) = probe - source is formed in fp64 from the fp64 state
//     and rounded once to fp32.  EVERY pair is evaluated: there is no far-field cull here - the map is a diagnostic, and the bound
//     of D8 is per receiver of a tick.  D1 / D2 hold: the guarded normalisation of csf_field.h, and r2 == 0 adds nothing.
//     With `fov` the probe is a receiver of heading psi: the mask of intersection.py:690-745 with the priority rule, through
//     tracked_m with the band of THIS delta's rounding; a pair the band flags (kept & lt) is decided on the spot by the reference's
//     own fp64 chain (csf_dev.h: untracked_exact_xy), and a TwoD pair within rounding of the line ahead of its source
//     (side_undecided) takes np.sign(phi) from sign_phi_exact - both fp64 positions are in hand, nobody is handed anything, no ring.
// field_map_road_kernel<NP>     sum over EVERY vertex of d.rv, the arithmetic of road_kernel (csf_pair.hip) - never the lattice or
//     the Chebyshev far field of csf_road.hip.  The probe's offset from a vertex tile's origin is formed in fp64 once per tile of
//     1024 and used in fp32.  A probe exactly on a vertex gets nothing from that vertex.
// Both write fp64 (Fx, Fy) per probe; the road launch adds to what the crowd launch left when both are asked for.
#include "csf_field.h"

namespace csf {

#include "csf_tick_terms.h"

constexpr int FM_BLOCK = 256;
constexpr int FM_TILE = 256;      // sources per LDS tile: one per thread of the fill
constexpr int FM_RTILE = 1024;    // vertices per LDS tile: the tiles of d.rvo

// The two fp64 chains of the reference's own decisions (csf_dev.h), as CALLS: a pair in a million takes one, and inlined they set the
// kernel's register count - 227 VGPRs, 2 waves / SIMD, 56.2 ms for 1 024 x 1 024 probes x 16 384 sources; as calls 128 VGPRs, 4 waves / SIMD,
// 36.0 ms (profiles/field_map_rate.txt).
__device__ __attribute__((noinline)) bool fm_untracked_exact(double xi, double yi, double xj, double yj, double psij, double hfov, bool p2r) {
    return untracked_exact_xy(xi, yi, xj, yj, psij, hfov, p2r);
}
__device__ __attribute__((noinline)) int fm_sign_phi_exact(double xi, double yi, double psii, double xj, double yj) {
    return sign_phi_exact(xi, yi, psii, xj, yj);
}

// intersection.py:690-745 + vehicle.py:1054-1147 / 1560-1648 for one probe (px, py, ppsi; r holds its heading) and one source
template <bool P2R>
__device__ __forceinline__ void field_map_pair(const Dev &d, const PairConsts &kb, const PairConsts &ks, const bool fov, const Recv &r,
                                               const double px, const double py, const double ppsi, const double xs, const double ys,
                                               const float4 q, const int32_t slot, const int cls, double &rx, double &ry) {
    const double ex = px - xs, ey = py - ys;                   // vehicle.py:1615-1616
    const float dx = (float)ex, dy = (float)ey, r2raw = dx * dx + dy * dy;
    if (!(r2raw > 0.0f)) return;                               // D2: a probe on the very spot of a source (and a non-finite one)
    const float r2 = fmaxf(r2raw, 1e-30f);
    if (fov) {
        bool kept, lt;
        bool in = tracked_m<P2R>(kb, ks.chs, r, dx, dy, r2raw, kept, lt);
        if (kept & lt) in = !fm_untracked_exact(xs, ys, px, py, ppsi, d.ptab[cls].hfov, P2R);   // (one pair in a million)
        if (!in) return;
    }
    int sg = 1;
    float F, gx, gy;
    if (ks.ipd != 0.0f) {                                      // vehicle.py:1054-1147: no jump at phi = 0
        field_bicycle(ks, q, make_float2(q.x, q.y), dx, dy, r2, F, gx, gy);
    } else {
        float sgf = 0.0f;                                      // 0: the sign of the fp32 sine
        if (side_undecided(kb, q, dx, dy, r2)) {
            sg = fm_sign_phi_exact(xs, ys, d.s[2 * d.cap + slot], px, py);
            sgf = sg < 0 ? -1.0f : 1.0f;
        }
        field_twod(ks, r, q, dx, dy, r2, F, gx, gy, sgf);
    }
    double wx = (double)(F * gx), wy = (double)(F * gy);
    if (sg == 0) {                                             // phi = 0 exactly: no tangential part, |F| = P along the line
        const double Pm = sqrt(wx * wx + wy * wy), il = 1.0 / sqrt(ex * ex + ey * ey);
        wx = Pm * ex * il;
        wy = Pm * ey * il;
    }
    rx += wx;
    ry += wy;
}

template <bool P2R>
__global__ __launch_bounds__(FM_BLOCK) void field_map_crowd_kernel(const Dev d, const FieldMapArgs a) {
    // a source of the tile: fp64 position, (e, 1 / sqrt(1 - e^2), cos psi, sin psi) - the first two the Bicycle field's alone -, its
    // slot (-1: not a source - the skipped road user, f_0 == 0: vehicle.py:1592-1593) and its parameter set
    __shared__ double sx[FM_TILE], sy[FM_TILE];
    __shared__ float4 sq[FM_TILE];
    __shared__ int32_t sslot[FM_TILE];
    __shared__ uint8_t scls[FM_TILE];
    extern __shared__ __align__(16) unsigned char fm_dyn[];   // [d.n_classes] PairConsts
    PairConsts *const ctab = (PairConsts *)fm_dyn;
    {
        const int words = d.n_classes * (int)(sizeof(PairConsts) / 4);
        for (int w = threadIdx.x; w < words; w += FM_BLOCK) ((uint32_t *)ctab)[w] = ((const uint32_t *)d.pctab)[w];
    }
    PairConsts kb = d.pc;                                      // the bands of this kernel's own rounding (engine/abi_fieldmap.inc)
    kb.fovA = a.fovA, kb.fovB = a.fovB, kb.sideA = a.sideA, kb.sideB = a.sideB, kb.sideP0 = a.sideP0, kb.sideP1 = a.sideP1;
    const int64_t i = (int64_t)blockIdx.x * FM_BLOCK + threadIdx.x;
    const bool have = i < a.m;
    const int64_t ii = have ? i : a.m - 1;                     // (clamped: every thread fills tiles and meets the barriers)
    const double px = a.x[ii], py = a.y[ii], ppsi = a.psi[ii];
    const bool finite = isfinite(px) && isfinite(py) && isfinite(ppsi);
    double sp = 0.0, cp = 1.0;
    if (finite) sincos(ppsi, &sp, &cp);
    const Recv r{0.f, 0.f, (float)cp, (float)sp};
    const bool fov = a.fov != 0;
    const int64_t cap = d.cap, n = d.n_live;
    double rx = 0.0, ry = 0.0;
    for (int64_t base = 0; base < n; base += FM_TILE) {
        const int cnt = (int)((n - base) < FM_TILE ? (n - base) : FM_TILE);
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            const int t = (int)threadIdx.x;
            const int64_t u = base + t;
            const int32_t slot = d.order ? d.order[u] : (int32_t)u;
            const int c = d.n_classes > 1 ? (int)d.cls[slot] : 0;
            const csf_params &ps = d.ptab[c];
            const bool bike = ps.model == CSF_BICYCLE;
            double ss, cs;
            sincos(d.s[2 * cap + slot], &ss, &cs);
            float2 se = make_float2(0.f, 1.f);
            if (bike) se = bicycle_se(d.s[3 * cap + slot], ps.v_max_riding[1]);
            sx[t] = d.s[slot];
            sy[t] = d.s[cap + slot];
            sq[t] = make_float4(se.x, se.y, (float)cs, (float)ss);
            scls[t] = (uint8_t)c;
            sslot[t] = (u == (int64_t)a.skip || (!bike && ps.f_0 == 0.0)) ? -1 : slot;
        }
        __syncthreads();
        if (!finite) continue;
        for (int j = 0; j < cnt; j++) {                        // (every lane of a wave reads the same source: LDS broadcasts)
            const int32_t slot = sslot[j];
            if (slot < 0) continue;                            // (uniform)
            const int c = scls[j];
            field_map_pair<P2R>(d, kb, ctab[c], fov, r, px, py, ppsi, sx[j], sy[j], sq[j], slot, c, rx, ry);
        }
    }
    if (have) {
        a.Fx[i] = finite ? rx : NAN;
        a.Fy[i] = finite ? ry : NAN;
    }
}

template <int NP>
__global__ __launch_bounds__(FM_BLOCK) void field_map_road_kernel(const Dev d, const FieldMapArgs a) {
    __shared__ float4 tv[FM_RTILE];                            // (x, y, -F0, -(sigma + 1) / 2); padding has F0 = 0
    static_assert(FM_RTILE == 1024, "the origins of the road vertices are per tile of 1024");
    const int64_t i = (int64_t)blockIdx.x * FM_BLOCK + threadIdx.x;
    const bool have = i < a.m;
    const int64_t ii = have ? i : a.m - 1;
    const double px = a.x[ii], py = a.y[ii];
    const bool finite = isfinite(px) && isfinite(py);
    const double bx = px - d.ox, by = py - d.oy;
    double fx = 0.0, fy = 0.0;
    for (int64_t base = 0; base < d.nv_pad; base += FM_RTILE) {
        const int cnt = (int)((d.nv_pad - base) < FM_RTILE ? (d.nv_pad - base) : FM_RTILE);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt; t += FM_BLOCK) tv[t] = d.rv[base + t];
        __syncthreads();
        if (!finite) continue;
        const float2 ot = d.rvo[base >> 10];
        const float rxo = (float)(bx - (double)ot.x), ryo = (float)(by - (double)ot.y);
        for (int u = 0; u < cnt; u++) {                        // (the same vertex in every lane: LDS broadcasts)
            const float4 v = tv[u];
            const float ex = v.x - rxo, ey = v.y - ryo, r2 = ex * ex + ey * ey;   // intersection.py:231-236
            float m;
            if (NP) {
                const float inv = fminf(fast_rsq(r2), 1e6f), i2 = inv * inv;      // r = 0: finite, times ex = ey = 0
                m = NP == 2 ? i2 : NP == 3 ? i2 * inv : NP == 4 ? i2 * i2 : NP == 5 ? i2 * i2 * inv : i2 * i2 * i2;
            } else {
                m = fast_exp2(fminf(v.w * fast_log2(r2), 120.f));
            }
            m *= v.z;                                          // -F0 r^-(sigma+1)    :238
            fx += (double)(m * ex);                            // :239-240
            fy += (double)(m * ey);
        }
    }
    if (have) {
        const double ax = a.accumulate ? a.Fx[i] : 0.0, ay = a.accumulate ? a.Fy[i] : 0.0;   // the crowd term first
        a.Fx[i] = finite ? ax + fx : NAN;
        a.Fy[i] = finite ? ay + fy : NAN;
    }
}

void launch_field_map_crowd(const Dev &d, const FieldMapArgs &a, hipStream_t st, hipEvent_t t0, hipEvent_t t1) {
    if (a.m <= 0) return;
    const dim3 g((unsigned)((a.m + FM_BLOCK - 1) / FM_BLOCK));
    const unsigned lds = (unsigned)((size_t)d.n_classes * sizeof(PairConsts));
    if (d.pc.p2r) hipExtLaunchKernelGGL(field_map_crowd_kernel<true>, g, dim3(FM_BLOCK), lds, st, t0, t1, 0, d, a);
    else hipExtLaunchKernelGGL(field_map_crowd_kernel<false>, g, dim3(FM_BLOCK), lds, st, t0, t1, 0, d, a);
}

template <int NP>
static void field_map_road_launch(const Dev &d, const FieldMapArgs &a, hipStream_t st, hipEvent_t t0, hipEvent_t t1) {
    hipExtLaunchKernelGGL(field_map_road_kernel<NP>, dim3((unsigned)((a.m + FM_BLOCK - 1) / FM_BLOCK)), dim3(FM_BLOCK), 0, st, t0, t1, 0, d, a);
}

void launch_field_map_road(const Dev &d, const FieldMapArgs &a, hipStream_t st, hipEvent_t t0, hipEvent_t t1) {
    if (a.m <= 0) return;
    switch (d.road_np) {
    case 2: field_map_road_launch<2>(d, a, st, t0, t1); break;
    case 3: field_map_road_launch<3>(d, a, st, t0, t1); break;
    case 4: field_map_road_launch<4>(d, a, st, t0, t1); break;
    case 5: field_map_road_launch<5>(d, a, st, t0, t1); break;
    case 6: field_map_road_launch<6>(d, a, st, t0, t1); break;
    default: field_map_road_launch<0>(d, a, st, t0, t1); break;
    }
}

}  // namespace csf
