// csf_passing.hip — following and passing in a recording (csf_passing, csf_batch_passing): who rode behind whom, at what gap and time
// headway, and who overtook or met whom, when, and with how much lateral clearance.  The definitions are include/csf.h's.
//
// The mapping is encounter_kernel's (csf_encounter.hip), because partners come from the same sample: ONE OWN STATION (k, i) PER LANE,
// P_i(k), P_i(k+1), the two directions of travel h_i(k), h_i(k+1) and their lengths in registers; the partners of station k in LDS
// tiles of 256 that every lane of a wave reads at the same address at the same time (a broadcast).  A tile slot is filled by one
// thread from P_j(k ... k+2): P_j(k), h_j(k), P_j(k+1), h_j(k+1) - four 16-byte words, 16 384 B of LDS -, NaN where a sample is absent
// or outside the window: station (j, k) that does not exist is all NaN, station (j, k+1) that does not exist has its two words NaN,
// so that no compare with it passes.  The tiles are walked in population order with a strict `<` and no cross-lane reduction: a
// row is the same bits whatever else is in the launch.  Everything is fp64 - no fp32, no fast-math function, and no contraction
// of a * b + c.
//
// passing_kernel<EVENTS>   grid (x, y, members), 256 threads, as encounter_kernel with stations in the place of samples.
//     n > 32:  blockIdx.x = a tile of 256 own riders, blockIdx.y = (station, chunk of partners); where tiles x stations leave CUs idle
//              (PassDesc::split) the partners of a station are split over up to 16 workgroups of whole tiles.
//     n <= 32: the cells (station, rider) of a member are packed: workgroup b takes the 256 / n stations from b * (256 / n) on, thread t
//              the rider t % n of station t / n; the one tile holds all of them, and a lane loops over the n slots of ITS station.
//     A pair costs four LDS reads, 23 fp64 operations - eight differences and the five terms g(k), dot(k), g(k+1) of "i passes j" and
//     g'(k), g'(k+1) of "j passes i", the latter in j's frame with the operations j's own lane uses - and their sign tests.  The
//     cross products, the divisions, the sqrt of the partner and the event test sit behind the sign tests, which almost always fail;
//     what passes them is decided by the definition itself, so the filters change no bit.  The leader is the candidate with the
//     smallest g: g against the best so far comes before the division that forms lat, and gap and thw are formed once at the end.
//     EVENTS: a passing under the threshold is stored by the lane of the passer.  Each wave makes one reservation per pass that
//     found any: ballot, popcount, one atomicAdd by its first such lane, the base broadcast; slots past the capacity are counted,
//     not written.  Every chunk leaves its results in device scratch (PassDesc::part_off).
// passing_window_kernel    the second pass, a launch of its own behind the first: thread = road user, a loop over its stations in
//     order.  It takes the chunks of a station in order with a strict `<` - the minimum of (g, j) and of (fabs(lat), j) in dictionary
//     order, which does not depend on where the chunks were cut -, sums their counts, writes the per-station and per-interval arrays,
//     and forms run_* with a strict `<`: the earliest k.
#include "csf_dev.h"

// every product below is rounded before it is added: the whole file, the kernels' bodies included (the lengths are formed there)
#pragma clang fp contract(off)

namespace csf {

constexpr int PASS_BLOCK = 256;
constexpr int PASS_TILE = 256;    // partners per LDS tile: one per thread of the fill
constexpr int PASS_WBLOCK = 64;   // road users per workgroup of the window pass

// (x, y) of road user u in sample k of the call; NaN outside the window
__device__ __forceinline__ double2 pass_pos(const PassDesc &m, int k, int u) {
    if (k >= m.count) return make_double2(NAN, NAN);
    int slot = m.first + k;
    if (slot >= m.cap) slot -= m.cap;
    const double *p = m.s + ((int64_t)slot * m.n + u) * m.ns;
    return make_double2(p[0], p[1]);
}

// station (u, k) and station (u, k + 1) as a partner meets them: NaN where the station does not exist
struct PassStation {
    double2 p0, h0, p1, h1;
    bool exists;             // station (u, k)
};

__device__ __forceinline__ PassStation pass_station(const PassDesc &m, int k, int u) {
#pragma clang fp contract(off)
    const double2 a = pass_pos(m, k, u), b = pass_pos(m, k + 1, u), c = pass_pos(m, k + 2, u);
    const bool fb = isfinite(b.x) && isfinite(b.y);
    const bool e0 = isfinite(a.x) && isfinite(a.y) && fb, e1 = e0 && fb && isfinite(c.x) && isfinite(c.y);
    const double2 none = make_double2(NAN, NAN);
    PassStation s;
    s.exists = e0;
    s.p0 = e0 ? a : none, s.h0 = e0 ? make_double2(b.x - a.x, b.y - a.y) : none;
    s.p1 = e1 ? b : none, s.h1 = e1 ? make_double2(c.x - b.x, c.y - b.y) : none;
    return s;
}

// what a lane has found for its own station among the partners it has seen: the record it leaves (gap and thw are formed at the end)
using PassBest = PassPart;

// where the events of the workgroup's member go
struct PassEv {
    csf_passing_event *ev;
    unsigned long long *count;
    unsigned long long cap;
};

// the values of "the passer passes the other in this interval" in the passer's frame, behind g0 > 0 && g1 <= 0: h, w, g and len of the
// passer's stations k and k + 1 (w = the other's position - the passer's).  true: fabs(lat_at) <= lat_max
__device__ __forceinline__ bool pass_values(const double2 h0, const double2 w0, const double g0, const double len0, const double2 h1,
                                            const double2 w1, const double g1, const double len1, const double lat_max, double &s, double &lat,
                                            double &closing) {
#pragma clang fp contract(off)
    const double cr0 = h0.x * w0.y - h0.y * w0.x, cr1 = h1.x * w1.y - h1.y * w1.x;
    const double a0 = g0 / len0, a1 = g1 / len1, lat0 = cr0 / len0, lat1 = cr1 / len1;
    closing = a0 - a1;
    s = a0 / closing;
    lat = lat0 + s * (lat1 - lat0);
    return fabs(lat) <= lat_max;
}

// len of a direction of travel: sqrt(h.x*h.x + h.y*h.y)
__device__ __forceinline__ double pass_len(const double2 h) {
#pragma clang fp contract(off)
    return sqrt(h.x * h.x + h.y * h.y);
}

__device__ __forceinline__ int pass_kind(double dot) { return dot > 0.0 ? 1 : (dot < 0.0 ? -1 : 0); }

// One ordered pair both ways: own stations (me, k), (me, k + 1) = o with lengths len0, len1; partner uj = slot j of the tile.
template <bool EVENTS>
__device__ __forceinline__ void pass_pair(const PassArgs &a, const PassEv &e, const PassStation &o, const double len0, const double len1,
                                          const double2 q0, const double2 r0, const double2 q1, const double2 r1, const int me, const int uj,
                                          const int k, PassBest &best) {
#pragma clang fp contract(off)
    const double2 w0 = make_double2(q0.x - o.p0.x, q0.y - o.p0.y), w1 = make_double2(q1.x - o.p1.x, q1.y - o.p1.y);     // i's frame
    const double2 v0 = make_double2(o.p0.x - q0.x, o.p0.y - q0.y), v1 = make_double2(o.p1.x - q1.x, o.p1.y - q1.y);     // j's frame
    const double g0 = w0.x * o.h0.x + w0.y * o.h0.y, g1 = w1.x * o.h1.x + w1.y * o.h1.y;
    const double e0 = v0.x * r0.x + v0.y * r0.y, e1 = v1.x * r1.x + v1.y * r1.y;
    const double dot = o.h0.x * r0.x + o.h0.y * r0.y;
    const bool ahead = g0 > 0.0;
    const bool fol = ahead & (dot >= 0.0) & (g0 < best.g);
    const bool made = ahead & (g1 <= 0.0);
    const bool by = (e0 > 0.0) & (e1 <= 0.0);
    if (!(fol | made | by) || uj == me) return;                // (almost always)
    if (fol && len0 > 0.0) {
        const double cr = o.h0.x * w0.y - o.h0.y * w0.x;
        const double lat = cr / len0;
        if (fabs(lat) <= a.band) best.g = g0, best.gj = uj;
    }
    if (by) {                                                  // j passes i, as j's lane forms it
        const double lj0 = pass_len(r0), lj1 = pass_len(r1);
        double s, lat, closing;
        if (lj0 > 0.0 && lj1 > 0.0 && pass_values(r0, v0, e0, lj0, r1, v1, e1, lj1, a.lat_max, s, lat, closing)) {
            const int kind = pass_kind(r0.x * o.h0.x + r0.y * o.h0.y);
            best.bc[0] += kind > 0, best.bc[1] += kind < 0, best.bc[2] += kind == 0;   // (no indexed access: the counts stay in registers)
            if (fabs(lat) < fabs(best.b_lat)) best.b_lat = lat, best.b_t = (double)k + s, best.b_with = uj, best.b_kind = kind;
        }
    }
    if (made) {
        double s = NAN, lat = NAN, closing = NAN;
        const bool hit = len0 > 0.0 && len1 > 0.0 && pass_values(o.h0, w0, g0, len0, o.h1, w1, g1, len1, a.lat_max, s, lat, closing);
        const int kind = pass_kind(dot);
        const double t = (double)k + s;
        if (hit) {
            best.mc[0] += kind > 0, best.mc[1] += kind < 0, best.mc[2] += kind == 0;
            if (fabs(lat) < fabs(best.m_lat)) best.m_lat = lat, best.m_t = t, best.m_with = uj, best.m_kind = kind;
        }
        if (EVENTS) {
            const bool store = hit && fabs(lat) < a.lat_event;
            const unsigned long long mask = __ballot(store);
            if (mask) {
                const int lane = (int)(threadIdx.x & 63);
                const int leader = __ffsll((long long)mask) - 1;
                unsigned long long base = 0;
                if (lane == leader) base = atomicAdd(e.count, (unsigned long long)__popcll(mask));
                base = __shfl(base, leader, 64);
                if (store) {
                    const unsigned long long at = base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
                    if (at < e.cap) {
                        csf_passing_event ev;
                        ev.i = me, ev.j = uj, ev.k = k, ev.kind = kind;
                        ev.t = t, ev.lat = lat, ev.closing = closing;
                        ev.cosine = dot / (len0 * pass_len(r0));
                        e.ev[at] = ev;
                    }
                }
            }
        }
    }
}

// the chunk's results of cell c (PassDesc::part_off)
__device__ __forceinline__ void pass_leave(const PassArgs &a, const PassDesc &m, const int64_t c, const PassStation &o, const double len0, PassBest best) {
    const bool led = best.gj >= 0;
    best.gap = led ? best.g / len0 : INFINITY;
    best.thw = led ? best.gap / len0 : INFINITY;
    if (!o.exists) best.g = best.gap = best.thw = best.m_lat = NAN;
    ((PassPart *)(a.out + m.part_off))[c] = best;
}

template <bool EVENTS>
__global__ __launch_bounds__(PASS_BLOCK) void passing_kernel(const PassArgs a) {
    __shared__ double2 s_p0[PASS_TILE], s_h0[PASS_TILE], s_p1[PASS_TILE], s_h1[PASS_TILE];
    const PassDesc m = a.desc[blockIdx.z];
    const int n = m.n, t = (int)threadIdx.x, stations = m.count - 1;
    if (n <= 0 || stations <= 0) return;
    const int64_t S = (int64_t)stations * n;
    PassBest best{INFINITY, INFINITY, INFINITY, INFINITY, NAN, INFINITY, NAN, -1, -1, 0, -1, 0, {0, 0, 0}, {0, 0, 0}, 0};
    const PassEv ev{(csf_passing_event *)(a.out + m.ev_off), a.count + blockIdx.z, (unsigned long long)m.ev_cap};
    if (n <= ENC_SMALL) {
        const int spw = PASS_BLOCK / n;                        // stations per workgroup
        const int64_t b = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        const int64_t k0 = b * spw;
        if (k0 >= stations) return;                            // (uniform)
        const int ls = t / n, u = t - ls * n;
        const int64_t k = k0 + ls;
        const bool have = ls < spw && k < stations;
        PassStation me;
        me.exists = false;
        me.p0 = me.h0 = me.p1 = me.h1 = make_double2(NAN, NAN);
        if (have) me = pass_station(m, (int)k, u);
        s_p0[t] = me.p0, s_h0[t] = me.h0, s_p1[t] = me.p1, s_h1[t] = me.h1;
        __syncthreads();
        if (!have) return;
        const double len0 = pass_len(me.h0), len1 = pass_len(me.h1);
        if (me.exists) {
            const int s0 = ls * n;
            for (int j = 0; j < n; j++) pass_pair<EVENTS>(a, ev, me, len0, len1, s_p0[s0 + j], s_h0[s0 + j], s_p1[s0 + j], s_h1[s0 + j], u, j, (int)k, best);
        }
        pass_leave(a, m, k * n + u, me, len0, best);
        return;
    }
    // blockIdx.y = (station, chunk of the station's partners)
    const int k = (int)blockIdx.y / m.split, chunk = (int)blockIdx.y - k * m.split;
    const int64_t i = (int64_t)blockIdx.x * PASS_BLOCK + t;
    if (k >= stations || (int64_t)blockIdx.x * PASS_BLOCK >= n) return;   // (uniform: the grid is the largest member's)
    const bool have = i < n;
    const PassStation me = pass_station(m, k, (int)(have ? i : n - 1));   // (clamped: every thread fills tiles and meets the barriers)
    const double len0 = pass_len(me.h0), len1 = pass_len(me.h1);
    const int src0 = chunk * m.chunk_tiles * PASS_TILE;
    const int src1 = n - src0 < m.chunk_tiles * PASS_TILE ? n : src0 + m.chunk_tiles * PASS_TILE;
    for (int base = src0; base < src1; base += PASS_TILE) {
        const int cnt = src1 - base < PASS_TILE ? src1 - base : PASS_TILE;
        __syncthreads();
        if (t < cnt) {
            const PassStation s = pass_station(m, k, base + t);
            s_p0[t] = s.p0, s_h0[t] = s.h0, s_p1[t] = s.p1, s_h1[t] = s.h1;
        }
        __syncthreads();
        if (!me.exists || !have) continue;                    // (a lane past the last rider only fills tiles: it would store events)
        for (int j = 0; j < cnt; j++)                          // (every lane of a wave reads the same partner: LDS broadcasts)
            pass_pair<EVENTS>(a, ev, me, len0, len1, s_p0[j], s_h0[j], s_p1[j], s_h1[j], (int)i, base + j, k, best);
    }
    if (have) pass_leave(a, m, chunk * S + (int64_t)k * n + i, me, len0, best);
}

__global__ __launch_bounds__(PASS_WBLOCK) void passing_window_kernel(const PassArgs a) {
    const PassDesc m = a.desc[blockIdx.z];
    const int n = m.n, stations = m.count - 1;
    const int64_t u = (int64_t)blockIdx.x * PASS_WBLOCK + threadIdx.x;
    if (stations <= 0 || u >= n) return;
    const int64_t S = (int64_t)stations * n, I = S - n;
    // the member's block (PassDesc): the doubles, then the int32 arrays
    double *const od = (double *)(a.out + m.out_off);
    int32_t *const oi = (int32_t *)(od + 2 * S + 4 * I + 6 * (int64_t)n);
    const PassPart *const part = (const PassPart *)(a.out + m.part_off);
    double b_gap = INFINITY, b_thw = INFINITY, b_ml = INFINITY, b_mt = NAN, b_bl = INFINITY, b_bt = NAN;
    int32_t b_gw = -1, b_gk = -1, b_tw = -1, b_tk = -1, b_mw = -1, b_mk = 0, b_bw = -1, b_bk = 0;
    int32_t mc0 = 0, mc1 = 0, mc2 = 0, bc0 = 0, bc1 = 0, bc2 = 0;
    for (int k = 0; k < stations; k++) {                       // (a NaN row - the station does not exist - is never `<`)
        const int64_t c = (int64_t)k * n + u;
        PassPart r = part[c];
        mc0 += r.mc[0], mc1 += r.mc[1], mc2 += r.mc[2], bc0 += r.bc[0], bc1 += r.bc[1], bc2 += r.bc[2];
        for (int q = 1; q < m.split; q++) {                    // the chunks of the partners, in order: the lowest j keeps a tie
            const PassPart x = part[c + q * S];
            mc0 += x.mc[0], mc1 += x.mc[1], mc2 += x.mc[2], bc0 += x.bc[0], bc1 += x.bc[1], bc2 += x.bc[2];
            if (x.g < r.g) r.g = x.g, r.gap = x.gap, r.thw = x.thw, r.gj = x.gj;
            if (fabs(x.m_lat) < fabs(r.m_lat)) r.m_lat = x.m_lat, r.m_t = x.m_t, r.m_with = x.m_with, r.m_kind = x.m_kind;
            if (fabs(x.b_lat) < fabs(r.b_lat)) r.b_lat = x.b_lat, r.b_t = x.b_t, r.b_with = x.b_with, r.b_kind = x.b_kind;
        }
        od[c] = r.gap, od[S + c] = r.thw, oi[c] = r.gj;
        if (r.gap < b_gap) b_gap = r.gap, b_gw = r.gj, b_gk = k;
        if (r.thw < b_thw) b_thw = r.thw, b_tw = r.gj, b_tk = k;
        if (k == stations - 1) continue;                       // (the last station begins no interval)
        double *const di = od + 2 * S;
        int32_t *const ii = oi + S;
        di[c] = r.m_lat, di[I + c] = r.m_t, di[2 * I + c] = r.b_lat, di[3 * I + c] = r.b_t;
        ii[c] = r.m_with, ii[I + c] = r.m_kind, ii[2 * I + c] = r.b_with, ii[3 * I + c] = r.b_kind;
        if (fabs(r.m_lat) < fabs(b_ml)) b_ml = r.m_lat, b_mt = r.m_t, b_mw = r.m_with, b_mk = r.m_kind;
        if (fabs(r.b_lat) < fabs(b_bl)) b_bl = r.b_lat, b_bt = r.b_t, b_bw = r.b_with, b_bk = r.b_kind;
    }
    double *const rd = od + 2 * S + 4 * I + u;
    rd[0] = b_gap, rd[n] = b_thw, rd[2 * n] = b_ml, rd[3 * n] = b_mt, rd[4 * n] = b_bl, rd[5 * n] = b_bt;
    int32_t *const ri = oi + S + 4 * I + u;
    ri[0] = b_gw, ri[n] = b_gk, ri[2 * n] = b_tw, ri[3 * n] = b_tk, ri[4 * n] = b_mw, ri[5 * n] = b_mk, ri[6 * n] = b_bw, ri[7 * n] = b_bk;
    int32_t *const rc = oi + S + 4 * I + 8 * (int64_t)n;
    rc[3 * u] = mc0, rc[3 * u + 1] = mc1, rc[3 * u + 2] = mc2;
    rc[3 * (n + u)] = bc0, rc[3 * (n + u) + 1] = bc1, rc[3 * (n + u) + 2] = bc2;
}

void launch_passing(const PassArgs &a, bool events, dim3 grid, int members, int max_n, hipStream_t st, hipEvent_t t0, hipEvent_t t1) {
    if (members <= 0 || max_n <= 0) return;
    if (events) hipExtLaunchKernelGGL(passing_kernel<true>, grid, dim3(PASS_BLOCK), 0, st, t0, t1, 0, a);
    else hipExtLaunchKernelGGL(passing_kernel<false>, grid, dim3(PASS_BLOCK), 0, st, t0, t1, 0, a);
    hipLaunchKernelGGL(passing_window_kernel, dim3((unsigned)((max_n + PASS_WBLOCK - 1) / PASS_WBLOCK), 1, (unsigned)members), dim3(PASS_WBLOCK), 0, st, a);
}

}  // namespace csf
