// csf_pet.hip — post-encroachment time of a recording (csf_post_encroachment, csf_batch_post_encroachment): who crossed whose path,
// where, and how long after the other had passed.  The definitions are include/csf.h's.
//
// The mapping is encounter_kernel's (csf_encounter.hip) with segments of paths in the place of road users: ONE OWN SEGMENT PER LANE
// - the cells (k, i) of a member flattened, k * n + i, so that a 3-rider scene of 99 segments fills two workgroups and not 99 -, its
// A, r and closed box in registers; the partner segments in LDS tiles of 256 that every lane of a wave reads at the same address at
// the same time (a broadcast).  Partner segments are numbered p = j * (count - 1) + l and walked in that order: a strict `<` then keeps
// the lowest j and the lowest l of a tie, with no cross-lane reduction, so a row is the same bits whatever else is in the launch.
// Everything is fp64 - no fp32, no fast-math function, and no contraction of a * b + c.
//
// pet_kernel<EVENTS>   grid (tiles of 256 own segments, chunks of partners, members), 256 threads.  A tile slot is filled by one thread:
//     the partner's closed box (min / max of its two endpoints; NaN where the segment does not exist, which no compare passes), C, s and
//     (j, l): 72 B per slot, 18 432 B of LDS.  A pair costs two 16-byte LDS reads and the four compares of the box test, which is part
//     of the definition - the three cross products, the decision from num and den, the divisions and the event test sit behind it,
//     and a wave skips them where none of its lanes passed.  The loop is bound by the wait for the two reads, so the boxes of
//     PET_AHEAD partners are read before the first is tested (DESIGN 4.13 has what else was tried).  Where the tiles of own segments alone leave CUs idle (PetDesc::split) the
//     partners of a tile are split over several workgroups; every chunk leaves what ITS partners gave in device scratch.
//     EVENTS: a crossing (i < j) under the threshold is stored by the lane of i.  Each wave makes one reservation per pass that found
//     any: ballot, popcount, one atomicAdd by its first such lane, the base broadcast; slots past the capacity are counted, not written.
// pet_window_kernel    the second pass, a launch of its own behind the first: thread = road user, a loop over its segments in
//     order.  It takes the chunks of a segment in order with a strict `<` - the minimum of (pet, j, l) in dictionary order, which does
//     not depend on where the chunks were cut -, sums their counts, writes seg_*, and forms run_* with a strict `<`: the earliest k.
#include "csf_dev.h"

namespace csf {

constexpr int PET_WBLOCK = 64;    // road users per workgroup of the window pass
constexpr int PET_AHEAD = 2;      // partners whose boxes a lane reads before it tests the first of them (4: 88 VGPRs, 5 waves / SIMD)

// (x, y) of road user u in sample k of the call
__device__ __forceinline__ double2 pet_pos(const PetDesc &m, int k, int u) {
    int slot = m.first + k;
    if (slot >= m.cap) slot -= m.cap;
    const double *p = m.s + ((int64_t)slot * m.n + u) * m.ns;
    return make_double2(p[0], p[1]);
}

// what a lane has found for its own segment among the partners it has seen
struct PetBest {
    double pet, t_own, t_with, x, y;
    int32_t with, count;
};

// the own segment of a lane: A, r, its closed box (NaN where it does not exist: a NaN box overlaps nothing), and who it is
struct PetOwn {
    double ax, ay, rx, ry, lox, loy, hix, hiy, kd;
    int32_t k, i;
    bool have, exists;
};

// Behind the box test: a partner (j, l) with C, s against the own segment o
template <bool EVENTS>
__device__ __forceinline__ void pet_pair(const PetArgs &a, const PetOwn &o, PetBest &best, const int2 jl, const double2 C, const double2 s,
                                         csf_pet_event *const ev, unsigned long long *const ev_count, const unsigned long long ev_cap) {
#pragma clang fp contract(off)
    if (jl.x == o.i) return;
    const double wx = C.x - o.ax, wy = C.y - o.ay;
    const double den = o.rx * s.y - o.ry * s.x;
    const double ns = wx * s.y - wy * s.x;
    const double nt = wx * o.ry - wy * o.rx;
    bool cross = false;
    if (den > 0.0) cross = (0.0 <= ns) & (ns < den) & (0.0 <= nt) & (nt < den);
    else if (den < 0.0) cross = (den < ns) & (ns <= 0.0) & (den < nt) & (nt <= 0.0);
    if (!cross) return;
    const double s_own = ns / den, s_with = nt / den;
    const double t_own = o.kd + s_own, t_with = (double)jl.y + s_with;
    const double pet = fabs(t_with - t_own);
    const double x = o.ax + s_own * o.rx, y = o.ay + s_own * o.ry;
    best.count++;
    if (pet < best.pet) best.pet = pet, best.t_own = t_own, best.t_with = t_with, best.x = x, best.y = y, best.with = jl.x;
    if (EVENTS) {
        const bool hit = (jl.x > o.i) & (pet < a.pet_event);
        const unsigned long long mask = __ballot(hit);
        if (mask) {
            const int lane = (int)(threadIdx.x & 63);
            const int leader = __ffsll((long long)mask) - 1;
            unsigned long long at0 = 0;
            if (lane == leader) at0 = atomicAdd(ev_count, (unsigned long long)__popcll(mask));
            at0 = __shfl(at0, leader, 64);
            if (hit) {
                const unsigned long long at = at0 + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
                if (at < ev_cap) {
                    csf_pet_event e;
                    e.i = o.i, e.j = jl.x, e.k = o.k, e.l = jl.y, e.t_i = t_own, e.t_j = t_with, e.x = x, e.y = y;
                    ev[at] = e;
                }
            }
        }
    }
}

template <bool EVENTS>
__global__ __launch_bounds__(PET_TILE) void pet_kernel(const PetArgs a) {
    __shared__ double2 s_lo[PET_TILE], s_hi[PET_TILE], s_c[PET_TILE], s_s[PET_TILE];
    __shared__ int2 s_jl[PET_TILE];
    const PetDesc m = a.desc[blockIdx.z];
    const int n = m.n, t = (int)threadIdx.x, per = m.count - 1;      // per: segments of one road user
    if (n <= 0 || per <= 0) return;
    const int64_t segs = (int64_t)per * n;
    const int64_t cell0 = (int64_t)blockIdx.x * PET_TILE;
    const int chunk = (int)blockIdx.y;
    if (cell0 >= segs || chunk >= m.split) return;                   // (uniform: the grid is the largest member's)
    const int64_t cell = cell0 + t;
    PetOwn o;
    o.have = cell < segs, o.exists = false, o.k = 0, o.i = -1;
    o.ax = o.ay = o.rx = o.ry = o.lox = o.loy = o.hix = o.hiy = NAN;
    if (o.have) {
        o.k = (int)(cell / n), o.i = (int)(cell - (int64_t)o.k * n);
        const double2 A = pet_pos(m, o.k, o.i), B = pet_pos(m, o.k + 1, o.i);
        o.exists = isfinite(A.x) && isfinite(A.y) && isfinite(B.x) && isfinite(B.y);
        if (o.exists) {
            o.ax = A.x, o.ay = A.y, o.rx = B.x - A.x, o.ry = B.y - A.y;
            o.lox = fmin(A.x, B.x), o.hix = fmax(A.x, B.x), o.loy = fmin(A.y, B.y), o.hiy = fmax(A.y, B.y);
        }
    }
    o.kd = (double)o.k;
    PetBest best{INFINITY, NAN, NAN, NAN, NAN, -1, 0};
    csf_pet_event *const ev = (csf_pet_event *)(a.out + m.ev_off);
    unsigned long long *const ev_count = a.count + blockIdx.z;
    const unsigned long long ev_cap = (unsigned long long)m.ev_cap;
    const int64_t span = (int64_t)m.chunk_tiles * PET_TILE;
    const int64_t p0 = chunk * span, p1 = segs - p0 < span ? segs : p0 + span;
    for (int64_t base = p0; base < p1; base += PET_TILE) {
        const int cnt = p1 - base < PET_TILE ? (int)(p1 - base) : PET_TILE;
        __syncthreads();
        if (t < cnt) {
            const int64_t p = base + t;
            const int j = (int)(p / per), l = (int)(p - (int64_t)j * per);
            const double2 C = pet_pos(m, l, j), D = pet_pos(m, l + 1, j);
            const bool ok = isfinite(C.x) && isfinite(C.y) && isfinite(D.x) && isfinite(D.y);
            s_lo[t] = ok ? make_double2(fmin(C.x, D.x), fmin(C.y, D.y)) : make_double2(NAN, NAN);
            s_hi[t] = ok ? make_double2(fmax(C.x, D.x), fmax(C.y, D.y)) : make_double2(NAN, NAN);
            s_c[t] = C;
            s_s[t] = make_double2(D.x - C.x, D.y - C.y);
            s_jl[t] = make_int2(j, l);
        }
        __syncthreads();
        // (every lane of a wave reads the same slot: LDS broadcasts.)  The boxes of PET_AHEAD partners are read before the first is
        // tested: a wave then waits for the LDS once per PET_AHEAD tests instead of once per test (the loop is bound by that wait)
        int q = 0;
        for (; q + PET_AHEAD <= cnt; q += PET_AHEAD) {
            double2 lo[PET_AHEAD], hi[PET_AHEAD];
#pragma unroll
            for (int u = 0; u < PET_AHEAD; u++) lo[u] = s_lo[q + u], hi[u] = s_hi[q + u];
#pragma unroll
            for (int u = 0; u < PET_AHEAD; u++)
                if ((o.lox <= hi[u].x) & (o.hix >= lo[u].x) & (o.loy <= hi[u].y) & (o.hiy >= lo[u].y))   // the closed boxes overlap (seldom)
                    pet_pair<EVENTS>(a, o, best, s_jl[q + u], s_c[q + u], s_s[q + u], ev, ev_count, ev_cap);
        }
        for (; q < cnt; q++) {
            const double2 lo = s_lo[q], hi = s_hi[q];
            if ((o.lox <= hi.x) & (o.hix >= lo.x) & (o.loy <= hi.y) & (o.hiy >= lo.y))
                pet_pair<EVENTS>(a, o, best, s_jl[q], s_c[q], s_s[q], ev, ev_count, ev_cap);
        }
    }
    const int64_t all = segs * m.split;
    double *const w_pet = (double *)(a.out + m.part_off), *const w_to = w_pet + all, *const w_tw = w_to + all;
    double *const w_x = w_tw + all, *const w_y = w_x + all;
    int32_t *const w_with = (int32_t *)(w_y + all), *const w_count = w_with + all;
    if (o.have) {
        const int64_t at = chunk * segs + cell;
        w_pet[at] = o.exists ? best.pet : NAN;
        w_to[at] = best.t_own, w_tw[at] = best.t_with, w_x[at] = best.x, w_y[at] = best.y;
        w_with[at] = best.with, w_count[at] = best.count;
    }
}

__global__ __launch_bounds__(PET_WBLOCK) void pet_window_kernel(const PetArgs a) {
    const PetDesc m = a.desc[blockIdx.z];
    const int n = m.n, per = m.count - 1;
    const int64_t u = (int64_t)blockIdx.x * PET_WBLOCK + threadIdx.x;
    if (per <= 0 || u >= n) return;
    const int64_t segs = (int64_t)per * n, all = segs * m.split;
    double *const o_pet = (double *)(a.out + m.out_off), *const o_to = o_pet + segs, *const o_tw = o_to + segs;
    double *const r_pet = o_tw + segs, *const r_to = r_pet + n, *const r_tw = r_to + n, *const r_x = r_tw + n, *const r_y = r_x + n;
    int32_t *const o_with = (int32_t *)(r_y + n), *const r_with = o_with + segs, *const r_count = r_with + n;
    const double *const p_pet = (const double *)(a.out + m.part_off), *const p_to = p_pet + all, *const p_tw = p_to + all;
    const double *const p_x = p_tw + all, *const p_y = p_x + all;
    const int32_t *const p_with = (const int32_t *)(p_y + all), *const p_count = p_with + all;
    double b_pet = INFINITY, b_to = NAN, b_tw = NAN, b_x = NAN, b_y = NAN;
    int32_t b_with = -1, total = 0;
    for (int k = 0; k < per; k++) {                                  // (a NaN row - the segment does not exist - is never `<`)
        const int64_t c = (int64_t)k * n + u;
        int64_t from = c;
        double d = p_pet[c];
        total += p_count[c];
        for (int q = 1; q < m.split; q++) {                          // the chunks of the partners, in order: the lowest (j, l) keeps a tie
            const int64_t cq = c + q * segs;
            const double dq = p_pet[cq];
            total += p_count[cq];
            if (dq < d) d = dq, from = cq;
        }
        const double to = p_to[from], tw = p_tw[from];
        const int32_t w = p_with[from];
        o_pet[c] = d, o_to[c] = to, o_tw[c] = tw, o_with[c] = w;
        if (d < b_pet) b_pet = d, b_to = to, b_tw = tw, b_x = p_x[from], b_y = p_y[from], b_with = w;
    }
    r_pet[u] = b_pet, r_to[u] = b_to, r_tw[u] = b_tw, r_x[u] = b_x, r_y[u] = b_y, r_with[u] = b_with, r_count[u] = total;
}

void launch_pet(const PetArgs &a, bool events, dim3 grid, int members, int max_n, hipStream_t st, hipEvent_t t0, hipEvent_t t1) {
    if (members <= 0 || max_n <= 0) return;
    if (events) hipExtLaunchKernelGGL(pet_kernel<true>, grid, dim3(PET_TILE), 0, st, t0, t1, 0, a);
    else hipExtLaunchKernelGGL(pet_kernel<false>, grid, dim3(PET_TILE), 0, st, t0, t1, 0, a);
    hipLaunchKernelGGL(pet_window_kernel, dim3((unsigned)((max_n + PET_WBLOCK - 1) / PET_WBLOCK), 1, (unsigned)members), dim3(PET_WBLOCK), 0, st, a);
}

}  // namespace csf
