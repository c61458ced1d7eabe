// csf_encounter.hip — proximity and time-to-collision measures of a recording (csf_encounters, csf_batch_encounters): how close the
// road users came, to whom and when, and how many seconds from a collision they were.  The definitions are include/csf.h's.
//
// The mapping is field_map_crowd_kernel's (csf_fieldmap.hip): ONE RECEIVER PER LANE, its fp64 (x, y, ux, uy) in registers, the
// sources of the same sample in LDS tiles of 256 - (x, y), (ux, uy) as two 16-byte words and a live flag - that every lane of a
// wave reads at the same address at the same time (a broadcast).  A tile slot is filled by one thread: one sincos per source and
// sample, not per pair.  A lane forms its minima in population order with a strict `<` and no cross-lane reduction: its row is the
// same bits whatever else is in the launch.  Everything is fp64 - no fp32, no fast-math function, and no contraction of a * b + c,
// so that a product is the same number wherever it is formed.
//
// encounter_kernel<EVENTS>   grid (x, y, members), 256 threads; a member's descriptor (EncDesc) says where its samples are - a
//     ring that may wrap, or the current state in slot order - and where its results go.
//     n > 32:  blockIdx.x = a tile of 256 receivers, blockIdx.y = (sample, chunk of sources); the workgroup walks its sources tile by
//              tile.  One chunk per sample, unless tiles x samples leave CUs idle (EncDesc::split: 16 384 riders x 1 sample are 64
//              workgroups): then a receiver tile's sources are split over up to 16 workgroups, each with its own minima.
//     n <= 32: a 256-thread workgroup per 3-rider sample would idle 253 lanes, so the cells (sample, rider) of a member are packed:
//              workgroup b (= blockIdx.y * gridDim.x + blockIdx.x) takes the 256 / n samples from b * (256 / n) on, thread t the
//              rider t % n of sample t / n; the one tile holds all of them, and a lane loops over the n slots of ITS sample.
//     The pair costs 17 fp64 operations and six compares where nothing is near: sqrt, the division and the event test sit behind
//     tests that almost always fail - ww against the best so far widened by 2^-50 (sqrt is monotone: a pair that fails cannot have
//     the smaller d), and q against best * (-2 b) (ttc >= q / (-2 b), because sqrt(b^2 - a q) <= |b|) narrowed by 1e-6.  A pair that
//     passes is decided by the definition itself: d = sqrt(ww) and ttc from the root without cancellation, compared with `<`.
//     EVENTS: a pair (i < j) under a threshold is stored by the lane of i.  Each wave makes one reservation per pass that found
//     any: ballot, popcount, one atomicAdd by its first such lane, the base broadcast; slots past the capacity are counted, not written.
// encounter_window_kernel    the second pass, a launch of its own behind the first: thread = rider, a loop over the samples of the
//     per-sample arrays in order, strict `<` - the earliest sample wins a tie -, absolute sample indices.  It reads what the first
//     launch wrote, in stream order: nothing depends on the order of workgroups.  Where the sources of a sample were split it first
//     takes the chunks' minima in order with the same `<` - the minimum of (value, j) in dictionary order, which does not depend on
//     where the chunks were cut - and writes the per-sample arrays itself.
#include "csf_dev.h"

namespace csf {

constexpr int ENC_BLOCK = 256;
constexpr int ENC_TILE = 256;     // sources per LDS tile: one per thread of the fill
constexpr int ENC_WBLOCK = 64;    // riders per workgroup of the window pass

struct EncSrc {
    double x, y, ux, uy;
    bool live;
};

// (x, y, ux, uy) of a state's rows 0 - 3; live: all four are finite.  A CALL: once per source and sample, and inlined three times its
// sincos sets the kernel's scalar register count (106, two of them spilled to lanes; as a call 66 and none)
__device__ __attribute__((noinline)) EncSrc enc_source(double x, double y, double psi, double v) {
    EncSrc r;
    r.live = isfinite(x) && isfinite(y) && isfinite(psi) && isfinite(v);
    double sn = 0.0, cs = 1.0;
    if (r.live) sincos(psi, &sn, &cs);
    r.x = x, r.y = y, r.ux = v * cs, r.uy = v * sn;
    return r;
}

// road user u in sample k of the member
__device__ __forceinline__ EncSrc enc_load(const EncDesc &m, int k, int u) {
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
    return enc_source(x, y, psi, v);
}

// include/csf.h: the four cases of ttc_ij
__device__ __forceinline__ double enc_ttc(double a, double b, double q) {
#pragma clang fp contract(off)
    if (q <= 0.0) return 0.0;
    if (b >= 0.0 || a == 0.0) return INFINITY;
    const double disc = b * b - a * q;
    if (disc < 0.0) return INFINITY;
    return q / (-b + sqrt(disc));
}

struct EncBest {
    double d, d_hi, t;     // the minima so far; d_hi = ww of the best d, widened: what a smaller d has to be under
    int32_t dj, tj;
};

// where the events of the workgroup's member go
struct EncEv {
    csf_encounter_event *ev;
    unsigned long long *count;
    unsigned long long cap;
};

// One pair: receiver (px, py, pu, pv) = road user `me` of sample `k`, source = slot j of the tile = road user uj.
template <bool EVENTS>
__device__ __forceinline__ void enc_pair(const EncArgs &a, const EncEv &e, const double2 sxy, const double2 suv, const bool ok, const double px,
                                         const double py, const double pu, const double pv, const int me, const int uj, const int k, EncBest &best) {
#pragma clang fp contract(off)
    const double wx = sxy.x - px, wy = sxy.y - py, cx = suv.x - pu, cy = suv.y - pv;
    const double ww = wx * wx + wy * wy, ca = cx * cx + cy * cy, cb = wx * cx + wy * cy, q = ww - a.R2;
    const bool near_d = ok & (ww < best.d_hi);
    // a candidate for the smaller ttc: overlapping, or approaching on a course that meets and not later than the best by the bound
    const bool meets = ok & ((q <= 0.0) | ((cb < 0.0) & (cb * cb - ca * q >= 0.0)));
    double tlim = best.t;
    bool ev_d = false;
    if (EVENTS) {
        if (uj > me) tlim = fmax(tlim, a.ttc_event);
        ev_d = ok & (uj > me) & (ww < a.de2_hi);
    }
    const bool near_t = meets & ((q <= 0.0) | (q * 0.999999 <= tlim * (-2.0 * cb)));
    if (near_d | near_t | ev_d) {                              // (seldom: a handful of passes per lane and sample)
        const double d = sqrt(ww);
        const double t = meets ? enc_ttc(ca, cb, q) : INFINITY;
        if (near_d && d < best.d) best.d = d, best.dj = uj, best.d_hi = ww * 1.0000000000000009;   // (1 + 2^-50)
        if (near_t && t < best.t) best.t = t, best.tj = uj;
        if (EVENTS) {
            const bool hit = ok & (uj > me) & ((d < a.d_event) | (t < a.ttc_event));
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
                        csf_encounter_event ev;
                        ev.sample = k;                         // (within the call: the host adds the index of the first sample)
                        ev.i = me, ev.j = uj, ev.d = d, ev.ttc = t;
                        e.ev[at] = ev;
                    }
                }
            }
        }
    }
}

template <bool EVENTS>
__global__ __launch_bounds__(ENC_BLOCK) void encounter_kernel(const EncArgs a) {
    __shared__ double2 sxy[ENC_TILE], suv[ENC_TILE];
    __shared__ uint8_t slive[ENC_TILE];
    const EncDesc m = a.desc[blockIdx.z];
    const int n = m.n, t = (int)threadIdx.x;
    if (n <= 0 || m.count <= 0) return;
    const int64_t cells = (int64_t)m.count * n;
    double *const o_d = (double *)(a.out + m.out_off), *const o_t = o_d + cells;
    int32_t *const o_dj = (int32_t *)(o_t + cells + 4 * (int64_t)n), *const o_tj = o_dj + cells;   // (behind the window arrays: EncDesc)
    EncBest best{INFINITY, INFINITY, INFINITY, -1, -1};
    const EncEv ev{(csf_encounter_event *)(a.out + m.ev_off), a.count + blockIdx.z, (unsigned long long)m.ev_cap};
    if (n <= ENC_SMALL) {
        const int spw = ENC_BLOCK / n;                         // samples per workgroup
        const int64_t b = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        const int64_t k0 = b * spw;
        if (k0 >= m.count) return;                             // (uniform)
        const int ls = t / n, u = t - ls * n;
        const int64_t k = k0 + ls;
        const bool have = ls < spw && k < m.count;
        EncSrc me{0.0, 0.0, 0.0, 0.0, false};
        if (have) me = enc_load(m, (int)k, u);
        sxy[t] = make_double2(me.x, me.y);
        suv[t] = make_double2(me.ux, me.uy);
        slive[t] = me.live ? 1 : 0;
        __syncthreads();
        if (!have) return;
        if (me.live) {
            const int s0 = ls * n;
            for (int j = 0; j < n; j++)
                enc_pair<EVENTS>(a, ev, sxy[s0 + j], suv[s0 + j], (slive[s0 + j] != 0) & (j != u), me.x, me.y, me.ux, me.uy, u, j, (int)k, best);
        }
        const int64_t c = k * n + u;
        o_d[c] = me.live ? best.d : NAN;
        o_t[c] = me.live ? best.t : NAN;
        o_dj[c] = best.dj;
        o_tj[c] = best.tj;
        return;
    }
    // blockIdx.y = (sample, chunk of the sample's sources): a member whose receivers and samples alone would leave CUs idle has its
    // sources split over m.split workgroups per receiver tile, each with the minima of ITS sources; the second pass takes the
    // chunks in order with the same strict `<`, which is the minimum of (value, j) in dictionary order - the same bits as one loop
    const int k = (int)blockIdx.y / m.split, chunk = (int)blockIdx.y - k * m.split;
    const int64_t i = (int64_t)blockIdx.x * ENC_BLOCK + t;
    if (k >= m.count || (int64_t)blockIdx.x * ENC_BLOCK >= n) return;   // (uniform: the grid is the largest member's)
    const bool have = i < n;
    const EncSrc me = enc_load(m, k, (int)(have ? i : n - 1));  // (clamped: every thread fills tiles and meets the barriers)
    const int src0 = chunk * m.chunk_tiles * ENC_TILE;
    const int src1 = n - src0 < m.chunk_tiles * ENC_TILE ? n : src0 + m.chunk_tiles * ENC_TILE;
    for (int base = src0; base < src1; base += ENC_TILE) {
        const int cnt = src1 - base < ENC_TILE ? src1 - base : ENC_TILE;
        __syncthreads();
        if (t < cnt) {
            const EncSrc s = enc_load(m, k, base + t);
            sxy[t] = make_double2(s.x, s.y);
            suv[t] = make_double2(s.ux, s.uy);
            slive[t] = s.live ? 1 : 0;
        }
        __syncthreads();
        if (!me.live) continue;
        for (int j = 0; j < cnt; j++) {                        // (every lane of a wave reads the same source: LDS broadcasts)
            if (!slive[j]) continue;                           // (uniform)
            enc_pair<EVENTS>(a, ev, sxy[j], suv[j], (int64_t)(base + j) != i, me.x, me.y, me.ux, me.uy, (int)i, base + j, k, best);
        }
    }
    if (have) {
        int64_t c = (int64_t)k * n + i;
        double *w_d = o_d, *w_t = o_t;
        int32_t *w_dj = o_dj, *w_tj = o_tj;
        if (m.split > 1) {                                     // the chunk's own arrays (EncDesc::part_off)
            const int64_t all = cells * m.split;
            w_d = (double *)(a.out + m.part_off), w_t = w_d + all, w_dj = (int32_t *)(w_t + all), w_tj = w_dj + all;
            c += chunk * cells;
        }
        w_d[c] = me.live ? best.d : NAN;
        w_t[c] = me.live ? best.t : NAN;
        w_dj[c] = best.dj;
        w_tj[c] = best.tj;
    }
}

__global__ __launch_bounds__(ENC_WBLOCK) void encounter_window_kernel(const EncArgs a) {
    const EncDesc m = a.desc[blockIdx.z];
    const int n = m.n;
    const int64_t u = (int64_t)blockIdx.x * ENC_WBLOCK + threadIdx.x;
    if (u >= n) return;
    const int64_t cells = (int64_t)m.count * n;
    double *const o_d = (double *)(a.out + m.out_off), *const o_t = o_d + cells;
    double *const r_d = (double *)(o_t + cells), *const r_t = r_d + n;
    int64_t *const r_ds = (int64_t *)(r_t + n), *const r_ts = r_ds + n;
    int32_t *const o_dj = (int32_t *)(r_ts + n), *const o_tj = o_dj + cells;
    int32_t *const r_dj = (int32_t *)(o_tj + cells), *const r_tj = r_dj + n;
    const int64_t all = cells * m.split;
    const double *const p_d = (const double *)(a.out + m.part_off), *const p_t = p_d + all;
    const int32_t *const p_dj = (const int32_t *)(p_t + all), *const p_tj = p_dj + all;
    double bd = INFINITY, bt = INFINITY;
    int32_t dj = -1, tj = -1;
    int64_t ds = -1, ts = -1;
    for (int k = 0; k < m.count; k++) {                        // (a NaN row - the rider was not finite in that sample - is never `<`)
        const int64_t c = (int64_t)k * n + u;
        double d, tt;
        int32_t wd, wt;
        if (m.split > 1) {                                     // the chunks of the sample's sources, in order: the lowest j keeps a tie
            d = p_d[c], tt = p_t[c], wd = p_dj[c], wt = p_tj[c];
            for (int q = 1; q < m.split; q++) {
                const int64_t cq = c + q * cells;
                const double dq = p_d[cq], tq = p_t[cq];
                if (dq < d) d = dq, wd = p_dj[cq];
                if (tq < tt) tt = tq, wt = p_tj[cq];
            }
            o_d[c] = d, o_t[c] = tt, o_dj[c] = wd, o_tj[c] = wt;
        } else {
            d = o_d[c], tt = o_t[c], wd = o_dj[c], wt = o_tj[c];
        }
        if (d < bd) bd = d, dj = wd, ds = k;
        if (tt < bt) bt = tt, tj = wt, ts = k;
    }
    r_d[u] = bd, r_t[u] = bt, r_dj[u] = dj, r_tj[u] = tj;
    r_ds[u] = (ds < 0 || m.first_abs < 0) ? -1 : m.first_abs + ds;   // (the current state is sample -1)
    r_ts[u] = (ts < 0 || m.first_abs < 0) ? -1 : m.first_abs + ts;
}

void launch_encounters(const EncArgs &a, bool events, dim3 grid, int members, int max_n, hipStream_t st, hipEvent_t t0, hipEvent_t t1) {
    if (members <= 0 || max_n <= 0) return;
    if (events) hipExtLaunchKernelGGL(encounter_kernel<true>, grid, dim3(ENC_BLOCK), 0, st, t0, t1, 0, a);
    else hipExtLaunchKernelGGL(encounter_kernel<false>, grid, dim3(ENC_BLOCK), 0, st, t0, t1, 0, a);
    hipLaunchKernelGGL(encounter_window_kernel, dim3((unsigned)((max_n + ENC_WBLOCK - 1) / ENC_WBLOCK), 1, (unsigned)members), dim3(ENC_WBLOCK), 0, st, a);
}

}  // namespace csf
