// csf_clearance.hip — road clearance of a recording (csf_clearance, csf_batch_clearance): how close to the segments of a road every
// road user came at every sample, which segment was the nearest, the nearest on the left and on the right of the direction of travel,
// and which segments it crossed.  The definitions are include/csf.h's.
//
// Every value belongs to ONE road user, so the mapping is ONE CELL (k, i) PER LANE, as in csf_flow.hip - but the road has thousands of
// segments where a layout has at most 64 lines, so a workgroup runs against one CHUNK of CLR_CHUNK segments, staged in LDS as a = A,
// d = B - A and dd (40 B a segment, formed once per workgroup), which every lane of a wave reads at the same address at the same time
// (a broadcast).  Everything is fp64 - no fp32, no fast-math function, and no contraction of a * b + c.
//
// clearance_kernel     grid (x, y, members x chunks), 256 threads: x, y the two grids of flow_kernel (n > 32: a tile of 256 road users
//     x the sample; n <= 32: the cells of a member packed, 256 / n samples to a workgroup), z / chunks the member and z % chunks the
//     chunk.  A lane keeps P(k), P(k+1), w and its three running minima in registers.  A segment costs a lane the foot of the
//     perpendicular (the division only where 0 < gg < dd: elsewhere the clamps give 0.0 or 1.0 whatever the quotient is), d2, and at
//     a station z and the two side values with their sign test; tt, the crossing point, u and the append sit behind the test, which
//     almost always fails.  A crossing is appended as flow_kernel appends one: ballot, popcount, one returning atomicAdd by the wave's
//     first finding lane, the base broadcast; slots past the capacity are counted, not written.  Every lane leaves a ClrPart.
// clearance_combine_kernel   a lane per cell: the chunks in the order of their index with the same strict `<` - the lowest g still
//     wins, whatever the chunk size -, then d, t (formed again with the function the first launch used: the same bits), the sides and
//     the per-cell arrays; near_count and cross_count are integer atomics, one per wave and sample where a wave shares its sample.
// clearance_walk_kernel      a lane per road user, a loop over k in order: d_min, left_min, right_min, near_* and cross_n.
#include "csf_dev.h"

// every product below is rounded before it is added: the whole file, the kernels' bodies included
#pragma clang fp contract(off)

namespace csf {

constexpr int CLR_BLOCK = 256;

// (x, y) of road user u in sample k of the call; NaN outside the window
__device__ __forceinline__ double2 clr_pos(const ClrDesc &m, int k, int u) {
    if (k >= m.count) return make_double2(NAN, NAN);
    int slot = m.first + k;
    if (slot >= m.cap) slot -= m.cap;
    const double *p = m.s + ((int64_t)slot * m.n + u) * m.ns;
    return make_double2(p[0], p[1]);
}

// the foot of the perpendicular from p on the segment A + t d, clamped: t, e = Q - p, and r = p - A for the side value
__device__ __forceinline__ void clr_foot(const double2 A, const double2 d, const double dd, const double2 p, double &t, double2 &e, double2 &r) {
#pragma clang fp contract(off)
    r = make_double2(p.x - A.x, p.y - A.y);
    const double gg = r.x * d.x + r.y * d.y;
    // t = gg / dd, t = t > 0 ? t : 0.0, t = t > 1 ? 1.0 : t - with dd > 0: gg <= 0 or NaN ends at 0.0, gg >= dd at 1.0, and a
    // quotient of 0 < gg < dd lies in [0, 1], where the clamps leave it alone
    t = 0.0;
    if (gg >= dd) t = 1.0;
    else if (gg > 0.0) t = gg / dd;
    const double qx = A.x + t * d.x, qy = A.y + t * d.y;
    e = make_double2(qx - p.x, qy - p.y);
}

__global__ __launch_bounds__(CLR_BLOCK) void clearance_kernel(const ClrArgs a) {
    __shared__ double2 s_a[CLR_CHUNK], s_d[CLR_CHUNK];
    __shared__ double s_dd[CLR_CHUNK];
    const int member = (int)blockIdx.z / a.chunks, chunk = (int)blockIdx.z - member * a.chunks;
    const ClrDesc m = a.desc[member];
    const int n = m.n, t = (int)threadIdx.x, c = m.count;
    if (n <= 0 || c <= 0) return;
    int k, u;
    bool have;
    if (n <= ENC_SMALL) {
        const int spw = CLR_BLOCK / n;                         // samples per workgroup
        const int64_t b = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        const int64_t k0 = b * spw;
        if (k0 >= c) return;                                   // (uniform)
        const int ls = t / n;
        u = t - ls * n;
        k = (int)(k0 + ls);
        have = ls < spw && k < c;
    } else {
        k = (int)blockIdx.y;
        const int64_t i = (int64_t)blockIdx.x * CLR_BLOCK + t;
        if (k >= c || (int64_t)blockIdx.x * CLR_BLOCK >= n) return;   // (uniform: the grid is the largest member's)
        have = i < n;
        u = (int)(have ? i : n - 1);
    }
    // the chunk, once per workgroup
    const int g0 = chunk * CLR_CHUNK, gn = min(CLR_CHUNK, a.S - g0);
    for (int j = t; j < gn; j += CLR_BLOCK) {
        const double *q = a.seg + 4 * (int64_t)(g0 + j);
        const double dx = q[2] - q[0], dy = q[3] - q[1];
        s_a[j] = make_double2(q[0], q[1]), s_d[j] = make_double2(dx, dy), s_dd[j] = dx * dx + dy * dy;
    }
    __syncthreads();
    const int lane = t & 63;
    double2 p0 = make_double2(NAN, NAN), p1 = p0;
    if (have) p0 = clr_pos(m, k, u), p1 = clr_pos(m, k + 1, u);
    const bool here = have && isfinite(p0.x) && isfinite(p0.y);             // cell (k, u) exists
    const bool station = here && isfinite(p1.x) && isfinite(p1.y);          // station (k, u) exists (k + 1 < c: p1 is NaN past the window)
    const double2 w = make_double2(p1.x - p0.x, p1.y - p0.y);
    ClrPart part;
    part.d2 = part.l2 = part.r2 = INFINITY;
    part.g = part.lg = part.rg = -1, part.cross = 0;
    if (here) {
        csf_clearance_event *const evs = (csf_clearance_event *)(a.out + m.ev_off);
        for (int j = 0; j < gn; j++) {                         // (every lane of a wave reads the same segment: LDS broadcasts)
            const double2 A = s_a[j], d = s_d[j];
            const double dd = s_dd[j];
            const int g = g0 + j;
            double tc;
            double2 e, r;
            clr_foot(A, d, dd, p0, tc, e, r);
            const double d2 = e.x * e.x + e.y * e.y;
            if (d2 < part.d2) part.d2 = d2, part.g = g;
            if (!station) continue;
            const double z = w.x * e.y - w.y * e.x;
            if (z > 0.0 && d2 < part.l2) part.l2 = d2, part.lg = g;
            if (z < 0.0 && d2 < part.r2) part.r2 = d2, part.rg = g;
            const double s0 = d.x * r.y - d.y * r.x, s1 = d.x * (p1.y - A.y) - d.y * (p1.x - A.x);
            if ((s0 > 0.0) == (s1 > 0.0)) continue;            // (almost always)
            const double tt = s0 / (s0 - s1);
            const double cx = p0.x + tt * w.x, cy = p0.y + tt * w.y;
            const double uc = ((cx - A.x) * d.x + (cy - A.y) * d.y) / dd;
            const bool hit = uc >= 0.0 && uc <= 1.0;
            const unsigned long long mask = __ballot(hit);    // (the lanes that met a sign change on this segment)
            if (!mask) continue;
            const int leader = __ffsll((long long)mask) - 1;
            unsigned long long base = 0;
            if (lane == leader) base = atomicAdd(a.count + member, (unsigned long long)__popcll(mask));
            base = __shfl(base, leader, 64);
            if (!hit) continue;
            part.cross++;
            const unsigned long long at = base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
            if (at < (unsigned long long)m.ev_cap) {
                csf_clearance_event ev;
                ev.i = u, ev.k = k, ev.edge = a.edge_of[g], ev.seg = g - a.first_g[ev.edge], ev.dir = s0 > 0.0 ? 1 : -1;
                ev.t = (double)k + tt, ev.u = uc;
                evs[at] = ev;
            }
        }
    }
    if (have) ((ClrPart *)(a.out + m.part_off))[(int64_t)chunk * c * n + (int64_t)k * n + u] = part;
}

__global__ __launch_bounds__(CLR_BLOCK) void clearance_combine_kernel(const ClrArgs a) {
    const ClrDesc m = a.desc[blockIdx.z];
    const int n = m.n, c = m.count;
    const int64_t cells = (int64_t)c * n, idx = (int64_t)blockIdx.x * CLR_BLOCK + threadIdx.x;
    if (n <= 0 || c <= 0 || idx >= cells) return;
    const int k = (int)(idx / n), u = (int)(idx - (int64_t)k * n), lane = (int)threadIdx.x & 63;
    const double2 p0 = clr_pos(m, k, u), p1 = clr_pos(m, k + 1, u);
    const bool here = isfinite(p0.x) && isfinite(p0.y);
    const bool station = here && isfinite(p1.x) && isfinite(p1.y);
    const ClrPart *const parts = (const ClrPart *)(a.out + m.part_off);
    ClrPart best = parts[idx];
    for (int ch = 1; ch < a.chunks; ch++) {                    // in the order of the chunks, a strict `<`: the lowest g wins a tie
        const ClrPart q = parts[(int64_t)ch * cells + idx];
        if (q.d2 < best.d2) best.d2 = q.d2, best.g = q.g;
        if (q.l2 < best.l2) best.l2 = q.l2, best.lg = q.lg;
        if (q.r2 < best.r2) best.r2 = q.r2, best.rg = q.rg;
        best.cross += q.cross;
    }
    double *const cd = (double *)(a.out + m.cell_off);
    int32_t *const ci = (int32_t *)(cd + 4 * cells);
    double d = NAN, tc = NAN;
    int32_t edge = -1, seg = -1;
    if (here) d = sqrt(best.d2);
    if (here && best.g >= 0) {                                 // (no segment is below +inf only where every d2 overflowed)
        const double *q = a.seg + 4 * (int64_t)best.g;
        const double dx = q[2] - q[0], dy = q[3] - q[1];
        double2 e, r;
        clr_foot(make_double2(q[0], q[1]), make_double2(dx, dy), dx * dx + dy * dy, p0, tc, e, r);
        edge = a.edge_of[best.g], seg = best.g - a.first_g[edge];
    }
    cd[idx] = d, cd[cells + idx] = tc;
    cd[2 * cells + idx] = station ? sqrt(best.l2) : NAN, cd[3 * cells + idx] = station ? sqrt(best.r2) : NAN;
    ci[idx] = edge, ci[cells + idx] = seg;
    ci[2 * cells + idx] = station && best.lg >= 0 ? a.edge_of[best.lg] : -1;
    ci[3 * cells + idx] = station && best.rg >= 0 ? a.edge_of[best.rg] : -1;
    ci[4 * cells + idx] = best.cross;
    int32_t *const near_count = (int32_t *)(a.out + m.acc_off), *const cross_count = near_count + c;
    if (best.cross > 0) atomicAdd(cross_count + k, best.cross);
    const bool near = d < a.d_event;                           // (NaN: no cell)
    const unsigned long long mask = __ballot(near);
    if (mask) {                                                // (uniform)
        const int leader = __ffsll((long long)mask) - 1;
        const int kl = __shfl(k, leader, 64);
        if (__all(!near || k == kl)) {
            if (lane == leader) atomicAdd(near_count + k, __popcll(mask));
        } else if (near) {
            atomicAdd(near_count + k, 1);
        }
    }
}

__global__ __launch_bounds__(CLR_BLOCK) void clearance_walk_kernel(const ClrArgs a) {
    const ClrDesc m = a.desc[blockIdx.z];
    const int n = m.n, c = m.count;
    const int64_t u = (int64_t)blockIdx.x * CLR_BLOCK + threadIdx.x;
    if (n <= 0 || c <= 0 || u >= n) return;
    const int64_t cells = (int64_t)c * n;
    const double *const cd = (const double *)(a.out + m.cell_off);
    const int32_t *const ci = (const int32_t *)(cd + 4 * cells);
    double d_min = INFINITY, l_min = INFINITY, r_min = INFINITY;
    int32_t d_k = -1, d_edge = -1, d_seg = -1, l_k = -1, r_k = -1, near = 0, first = -1, last = -1, crossed = 0;
    for (int k = 0; k < c; k++) {
        const int64_t at = (int64_t)k * n + u;
        const double d = cd[at], l = cd[2 * cells + at], r = cd[3 * cells + at];
        if (d < d_min) d_min = d, d_k = k, d_edge = ci[at], d_seg = ci[cells + at];
        if (l < l_min) l_min = l, l_k = k;
        if (r < r_min) r_min = r, r_k = k;
        if (d < a.d_event) {
            near++;
            if (first < 0) first = k;
            last = k;
        }
        crossed += ci[4 * cells + at];
    }
    double *const od = (double *)(a.out + m.out_off);
    int32_t *const oi = (int32_t *)(od + 3 * (int64_t)n);
    od[u] = d_min, od[n + u] = l_min, od[2 * (int64_t)n + u] = r_min;
    const int64_t N = n;
    oi[u] = d_k, oi[N + u] = d_edge, oi[2 * N + u] = d_seg, oi[3 * N + u] = l_k, oi[4 * N + u] = r_k;
    oi[5 * N + u] = near, oi[6 * N + u] = first, oi[7 * N + u] = last, oi[8 * N + u] = crossed;
}

void launch_clearance(const ClrArgs &a, dim3 grid, int members, int64_t max_cells, int max_n, hipStream_t st, hipEvent_t t0, hipEvent_t t1) {
    if (members <= 0 || max_n <= 0 || max_cells <= 0) return;
    hipExtLaunchKernelGGL(clearance_kernel, grid, dim3(CLR_BLOCK), 0, st, t0, t1, 0, a);
    hipLaunchKernelGGL(clearance_combine_kernel, dim3((unsigned)((max_cells + CLR_BLOCK - 1) / CLR_BLOCK), 1, (unsigned)members), dim3(CLR_BLOCK), 0, st, a);
    hipLaunchKernelGGL(clearance_walk_kernel, dim3((unsigned)((max_n + CLR_BLOCK - 1) / CLR_BLOCK), 1, (unsigned)members), dim3(CLR_BLOCK), 0, st, a);
}

}  // namespace csf
