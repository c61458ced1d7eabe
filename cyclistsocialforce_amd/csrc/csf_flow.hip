// csf_flow.hip — flow, density and speed of a recording at counting lines and areas (csf_flow, csf_batch_flow): who crossed which
// cross-section, in which direction and at what speed, who was inside which stretch of path at each sample and how far they rode
// there, and in which cell of a grid everybody spent their samples.  The definitions are include/csf.h's.
//
// Nothing here is a pair: every value belongs to ONE road user, so the mapping is ONE CELL (k, i) PER LANE - the sample P_i(k) for the
// areas and the grid, the station P_i(k), P_i(k+1) for the lines - and the layout (at most 64 lines and 64 areas, with d = B - A, dd
// and half_width * ld formed once per workgroup) in LDS, which every lane of a wave reads at the same address at the same time (a
// broadcast).  Everything is fp64 - no fp32, no fast-math function, and no contraction of a * b + c.
//
// flow_kernel          grid (x, y, members), 256 threads, the two grids of passing_kernel with samples in the place of stations.
//     n > 32:  blockIdx.x = a tile of 256 road users, blockIdx.y = the sample: the workgroup shares k, so occupancy [k][r] - the one
//              word every tile of a sample adds to - is counted in LDS and costs one global atomic per workgroup and area that
//              found anybody.
//     n <= 32: the cells of a member are packed: workgroup b takes the 256 / n samples from b * (256 / n) on, thread t the road user
//              t % n of sample t / n.  At most n lanes meet in a word of occupancy: they add to it directly.
//     A line costs a lane two side values (four differences, four products, two differences) and their sign test; t, the crossing
//     point, u and the append sit behind the test, which almost always fails.  Crossings and grid cells are spread out and add
//     directly (integer atomics: no order is involved).  A crossing is appended as passing_kernel appends a passing: ballot,
//     popcount, one returning atomicAdd by the wave's first finding lane, the base broadcast; slots past the capacity are counted,
//     not written.  The samples outside the grid are counted per wave the same way.  Every lane leaves a FlowCell: the masks of the
//     areas it is inside and of the lines it crosses, the direction of each, and its len (NaN: no station).
// flow_walk_kernel     the second pass, a launch of its own behind the first: thread = (road user, line or area), a loop over k in
//     order over the cells of its road user.  A line's thread counts the crossings by direction and forms the first one again from
//     the ring with the function the first launch used - the same bits; an area's thread counts the samples inside, keeps the first
//     and the last, and forms in_dist as the stated sequential sum.
#include "csf_dev.h"

// every product below is rounded before it is added: the whole file, the kernels' bodies included
#pragma clang fp contract(off)

namespace csf {

constexpr int FLOW_BLOCK = 256;
constexpr int FLOW_WBLOCK = 256;   // (road user, line or area) lanes per workgroup of the walk

// (x, y) of road user u in sample k of the call; NaN outside the window
__device__ __forceinline__ double2 flow_pos(const FlowDesc &m, int k, int u) {
    if (k >= m.count) return make_double2(NAN, NAN);
    int slot = m.first + k;
    if (slot >= m.cap) slot -= m.cap;
    const double *p = m.s + ((int64_t)slot * m.n + u) * m.ns;
    return make_double2(p[0], p[1]);
}

// a line or the centre line of an area as the lanes read it
struct FlowLine {
    double2 a, d;
    double dd;
};

__device__ __forceinline__ FlowLine flow_line(const double *q) {
#pragma clang fp contract(off)
    FlowLine f;
    f.a = make_double2(q[0], q[1]);
    f.d = make_double2(q[2] - q[0], q[3] - q[1]);
    f.dd = f.d.x * f.d.x + f.d.y * f.d.y;
    return f;
}

// s(P): positive on the left of A -> B
__device__ __forceinline__ double flow_side(const FlowLine &f, const double2 p) {
#pragma clang fp contract(off)
    return f.d.x * (p.y - f.a.y) - f.d.y * (p.x - f.a.x);
}

// behind a sign change: t and u of the crossing point; true: it lies within the line's extent
__device__ __forceinline__ bool flow_cross(const FlowLine &f, const double2 p0, const double2 h, const double s0, const double s1, double &t, double &u) {
#pragma clang fp contract(off)
    t = s0 / (s0 - s1);
    const double xx = p0.x + t * h.x, xy = p0.y + t * h.y;
    u = ((xx - f.a.x) * f.d.x + (xy - f.a.y) * f.d.y) / f.dd;
    return u >= 0.0 && u <= 1.0;
}

__global__ __launch_bounds__(FLOW_BLOCK) void flow_kernel(const FlowArgs a) {
    __shared__ double2 s_la[FLOW_MAX], s_ld[FLOW_MAX], s_aa[FLOW_MAX], s_ad[FLOW_MAX];
    __shared__ double s_ldd[FLOW_MAX], s_add[FLOW_MAX], s_aw[FLOW_MAX];
    __shared__ int s_occ[FLOW_MAX];
    const FlowDesc m = a.desc[blockIdx.z];
    const int n = m.n, t = (int)threadIdx.x, c = m.count, L = a.L, R = a.R;
    if (n <= 0 || c <= 0) return;
    int k, u;
    bool have;
    const bool packed = n <= ENC_SMALL;
    if (packed) {
        const int spw = FLOW_BLOCK / n;                        // samples per workgroup
        const int64_t b = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        const int64_t k0 = b * spw;
        if (k0 >= c) return;                                   // (uniform)
        const int ls = t / n;
        u = t - ls * n;
        k = (int)(k0 + ls);
        have = ls < spw && k < c;
    } else {
        k = (int)blockIdx.y;
        const int64_t i = (int64_t)blockIdx.x * FLOW_BLOCK + t;
        if (k >= c || (int64_t)blockIdx.x * FLOW_BLOCK >= n) return;   // (uniform: the grid is the largest member's)
        have = i < n;
        u = (int)(have ? i : n - 1);
    }
    // the layout, once per workgroup
    if (t < L) {
        const FlowLine f = flow_line(a.lines + 4 * t);
        s_la[t] = f.a, s_ld[t] = f.d, s_ldd[t] = f.dd;
    }
    if (t >= FLOW_MAX && t - FLOW_MAX < R) {
        const int r = t - FLOW_MAX;
        const double *q = a.areas + 5 * r;
        const FlowLine f = flow_line(q);
        s_aa[r] = f.a, s_ad[r] = f.d, s_add[r] = f.dd, s_aw[r] = q[4] * sqrt(f.dd);
    }
    if (t < FLOW_MAX) s_occ[t] = 0;
    __syncthreads();
    int32_t *const acc = (int32_t *)(a.out + m.acc_off);       // line_count [c-1][L][2], occupancy [c][R], grid_count [ny][nx]
    int32_t *const occ = acc + (int64_t)(c - 1) * L * 2;
    int32_t *const cells = occ + (int64_t)c * R;
    const int lane = t & 63;
    double2 p0 = make_double2(NAN, NAN), p1 = p0;
    if (have) p0 = flow_pos(m, k, u), p1 = flow_pos(m, k + 1, u);
    const bool here = have && isfinite(p0.x) && isfinite(p0.y);             // sample (u, k) exists
    const bool station = here && isfinite(p1.x) && isfinite(p1.y);          // station (u, k) exists (k + 1 < c: p1 is NaN past the window)
    const double2 h = make_double2(p1.x - p0.x, p1.y - p0.y);
    FlowCell cell;
    cell.inside = cell.cross = cell.left = 0ull;
    cell.len = station ? sqrt(h.x * h.x + h.y * h.y) : NAN;
    // areas
    if (here) {
        for (int r = 0; r < R; r++) {                          // (every lane of a wave reads the same area: LDS broadcasts)
            const double2 A = s_aa[r], d = s_ad[r];
            const double wx = p0.x - A.x, wy = p0.y - A.y;
            const double g = wx * d.x + wy * d.y, cr = d.x * wy - d.y * wx;
            if (g >= 0.0 && g <= s_add[r] && fabs(cr) <= s_aw[r]) {
                cell.inside |= 1ull << r;
                if (packed) atomicAdd(occ + (int64_t)k * R + r, 1);
                else atomicAdd(&s_occ[r], 1);
            }
        }
    }
    // grid
    if (a.nx > 0) {
        bool out = false;
        if (here) {
            const double fx = floor((p0.x - a.x0) / a.h), fy = floor((p0.y - a.y0) / a.h);
            if (fx >= 0.0 && fx < (double)a.nx && fy >= 0.0 && fy < (double)a.ny) atomicAdd(cells + (int64_t)fy * a.nx + (int64_t)fx, 1);
            else out = true;
        }
        const unsigned long long mask = __ballot(out);
        if (mask && lane == __ffsll((long long)mask) - 1) atomicAdd(a.count + a.members + blockIdx.z, (unsigned long long)__popcll(mask));
    }
    // lines
    if (station) {
        csf_flow_event *const evs = (csf_flow_event *)(a.out + m.ev_off);
        for (int l = 0; l < L; l++) {
            FlowLine f;
            f.a = s_la[l], f.d = s_ld[l], f.dd = s_ldd[l];
            const double s0 = flow_side(f, p0), s1 = flow_side(f, p1);
            if ((s0 > 0.0) == (s1 > 0.0)) continue;            // (almost always)
            double tc, uc;
            const bool hit = flow_cross(f, p0, h, s0, s1, tc, uc);
            const unsigned long long mask = __ballot(hit);    // (the lanes that met a sign change on this line)
            if (!mask) continue;
            const int leader = __ffsll((long long)mask) - 1;
            unsigned long long base = 0;
            if (lane == leader) base = atomicAdd(a.count + blockIdx.z, (unsigned long long)__popcll(mask));
            base = __shfl(base, leader, 64);
            if (!hit) continue;
            const bool left = s0 > 0.0;
            cell.cross |= 1ull << l;
            if (left) cell.left |= 1ull << l;
            atomicAdd(acc + ((int64_t)k * L + l) * 2 + (left ? 0 : 1), 1);
            const unsigned long long at = base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
            if (at < (unsigned long long)m.ev_cap) {
                csf_flow_event ev;
                ev.i = u, ev.l = l, ev.k = k, ev.dir = left ? 1 : -1;
                ev.t = (double)k + tc, ev.u = uc, ev.speed = cell.len;
                evs[at] = ev;
            }
        }
    }
    if (have) ((FlowCell *)(a.out + m.cell_off))[(int64_t)k * n + u] = cell;
    if (!packed) {
        __syncthreads();
        if (t < R && s_occ[t] != 0) atomicAdd(occ + (int64_t)k * R + t, s_occ[t]);
    }
}

__global__ __launch_bounds__(FLOW_WBLOCK) void flow_walk_kernel(const FlowArgs a) {
    const FlowDesc m = a.desc[blockIdx.z];
    const int n = m.n, c = m.count, L = a.L, R = a.R, J = L + R;
    const int64_t g = (int64_t)blockIdx.x * FLOW_WBLOCK + threadIdx.x;
    if (n <= 0 || c <= 0 || J <= 0 || g >= (int64_t)n * J) return;
    const int u = (int)(g / J), j = (int)(g - (int64_t)u * J);
    const FlowCell *const cells = (const FlowCell *)(a.out + m.cell_off);
    // the member's block (FlowDesc): the doubles, then the int32 arrays
    double *const od = (double *)(a.out + m.out_off);
    const int64_t nL = (int64_t)n * L, nR = (int64_t)n * R;
    int32_t *const oi = (int32_t *)(od + 3 * nL + nR);
    if (j < L) {
        const unsigned long long bit = 1ull << j;
        int32_t c0 = 0, c1 = 0, dir = 0;
        double ft = INFINITY, fu = NAN, fs = NAN;
        for (int k = 0; k + 1 < c; k++) {
            const FlowCell &q = cells[(int64_t)k * n + u];
            if (!(q.cross & bit)) continue;
            const bool left = (q.left & bit) != 0;
            c0 += left, c1 += !left;
            if (dir != 0) continue;
            dir = left ? 1 : -1;
            const FlowLine f = flow_line(a.lines + 4 * j);
            const double2 p0 = flow_pos(m, k, u), p1 = flow_pos(m, k + 1, u);
            const double2 h = make_double2(p1.x - p0.x, p1.y - p0.y);
            double tc, uc;
            flow_cross(f, p0, h, flow_side(f, p0), flow_side(f, p1), tc, uc);
            ft = (double)k + tc, fu = uc, fs = q.len;
        }
        const int64_t at = (int64_t)u * L + j;
        od[at] = ft, od[nL + at] = fu, od[2 * nL + at] = fs;
        oi[2 * at] = c0, oi[2 * at + 1] = c1, oi[2 * nL + at] = dir;
        return;
    }
    const int r = j - L;
    const unsigned long long bit = 1ull << r;
    int32_t samples = 0, first = -1, last = -1;
    double dist = 0.0;
    for (int k = 0; k < c; k++) {
        const FlowCell &q = cells[(int64_t)k * n + u];
        if (!(q.inside & bit)) continue;
        samples++;
        if (first < 0) first = k;
        last = k;
        if (q.len == q.len) dist = dist + q.len;               // (NaN: no station begins here)
    }
    const int64_t at = (int64_t)u * R + r;
    od[3 * nL + at] = dist;
    int32_t *const ia = oi + 3 * nL;
    ia[at] = samples, ia[nR + at] = first, ia[2 * nR + at] = last;
}

void launch_flow(const FlowArgs &a, dim3 grid, int members, int max_n, hipStream_t st, hipEvent_t t0, hipEvent_t t1) {
    if (members <= 0 || max_n <= 0) return;
    hipExtLaunchKernelGGL(flow_kernel, grid, dim3(FLOW_BLOCK), 0, st, t0, t1, 0, a);
    const int64_t lanes = (int64_t)max_n * (a.L + a.R);
    if (lanes > 0) hipLaunchKernelGGL(flow_walk_kernel, dim3((unsigned)((lanes + FLOW_WBLOCK - 1) / FLOW_WBLOCK), 1, (unsigned)members), dim3(FLOW_WBLOCK), 0, st, a);
}

}  // namespace csf
