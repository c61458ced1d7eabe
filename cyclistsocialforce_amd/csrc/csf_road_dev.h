// csf_road_dev.h - the arithmetic of the road term (intersection.py:226-242), ONCE, for the two kernels that sum every vertex of a
// small road for a wave's RPW receivers: road_kernel (csf_pair.hip: the vertices staged in LDS by the workgroup) and the road items of
// the one-launch tick (csf_mid_body.inc: the vertices straight from memory, asked for one pass ahead).  A receiver's sum depends on the
// order inside a lane - tiles in order, t = lane, lane + 128, ..., the .x / .y halves, then the butterfly - and not on which wave holds
// it: both callers keep that order, so both write the same float.
#pragma once
#include "csf_pair_dev.h"

namespace csf {

// two vertices per lane (packed arithmetic) against the wave's receivers, r relative to the origin of the vertices' tile.
// pf = -F0 (0 for padding and for a missing second vertex), pw = -(sigma + 1) / 2 (read only where NP = 0).
// NP = sigma + 1 when every edge shares one small integer sigma: r^-(sigma+1) is then a power of rsq(r^2); NP = 0: per-vertex exponent.
template <int NP>
__device__ __forceinline__ void road_pair_x2(const v2f px, const v2f py, const v2f pf, const v2f pw, const Recv (&r)[RPW], v2f (&ax)[RPW], v2f (&ay)[RPW]) {
#pragma unroll
    for (int u = 0; u < RPW; u++) {
        const v2f ex = px - r[u].x, ey = py - r[u].y;       // :235-236 (numerators)
        const v2f r2 = ex * ex + ey * ey;                   // :231-234
        v2f m;
        if (NP) {
            v2f inv = rsq2(r2);
            inv = __builtin_elementwise_min(inv, v2f{1e6f, 1e6f});   // r = 0: finite, times ex = ey = 0
            const v2f i2 = inv * inv;
            m = NP == 2 ? i2 : NP == 3 ? i2 * inv : NP == 4 ? i2 * i2 : NP == 5 ? i2 * i2 * inv : i2 * i2 * i2;
        } else {
            v2f lg = pw * v2f{fast_log2(r2.x), fast_log2(r2.y)};
            lg = __builtin_elementwise_min(lg, v2f{120.f, 120.f});   // r = 0: finite, times ex = ey = 0
            m = v2f{fast_exp2(lg.x), fast_exp2(lg.y)};
        }
        m = m * pf;                                         // -F0 r^-(sigma+1)    :238
        ax[u] = m * ex + ax[u];                             // :239-240
        ay[u] = m * ey + ay[u];
    }
}

// a receiver's sum over the wave: the two halves of a lane, then the xor butterfly (every lane ends with the sum)
__device__ __forceinline__ float2 road_wave_sum(const v2f ax, const v2f ay) {
    float sx = ax.x + ax.y, sy = ay.x + ay.y;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sx += __shfl_xor(sx, o, WAVE);
        sy += __shfl_xor(sy, o, WAVE);
    }
    return make_float2(sx, sy);
}

// The road term of RPW receivers against ALL d.nv_pad vertices by ONE wave that meets nobody at a barrier (csf_mid_body.inc): the
// vertices come straight from d.rv - 16 bytes per lane and load, coalesced, at most 32 KB that stay in L2 from tick to tick -, the two
// loads of a pass asked for while the pass before is summed.  (rh, rl)[u]: the receivers' scene coordinates as hi + lo (two_sum), re-based
// on the origin of every tile of 1 024 vertices as road_kernel does it.  A pass is 128 vertices and a tile 1 024, so no pass spans two
// tiles, and nv_pad is a multiple of 64: whether a pass has its second half is uniform.  A missing second half repeats the first with
// pf = 0, which is what road_kernel's LDS reads give it.
template <int NP>
__device__ __forceinline__ void road_sum_from_memory(const Dev &d, const int lane, const float (&rh)[RPW][2], const float (&rl)[RPW][2], float2 (&f)[RPW]) {
    static_assert(TILE == 1024 && TILE % (2 * WAVE) == 0, "the origins of the road vertices are per tile of 1024");
    const int nvp = (int)d.nv_pad;
    Recv r[RPW];
    v2f ax[RPW], ay[RPW];
#pragma unroll
    for (int u = 0; u < RPW; u++) {
        ax[u] = ay[u] = v2f{0.f, 0.f};
        r[u].x = r[u].y = r[u].c = r[u].s = 0.f;
    }
    auto ask = [&](const int p, float4 &v0, float4 &v1) {
        const int t = p + lane;
        v0 = d.rv[t];  // (x, y, -F0, -(sigma+1)/2); padding has F0 = 0
        v1 = d.rv[p + WAVE < nvp ? t + WAVE : t];
    };
    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
    if (nvp > 0) ask(0, v0, v1);
    for (int p = 0; p < nvp; p += 2 * WAVE) {
        if ((p & (TILE - 1)) == 0) {
            const float2 ot = d.rvo[p >> 10];
#pragma unroll
            for (int u = 0; u < RPW; u++) {
                r[u].x = (rh[u][0] - ot.x) + rl[u][0];
                r[u].y = (rh[u][1] - ot.y) + rl[u][1];
                asm volatile("" : "+v"(r[u].x), "+v"(r[u].y));    // stay in VGPRs
            }
        }
        const bool two = p + WAVE < nvp;
        const float4 c0 = v0, c1 = v1;
        if (p + 2 * WAVE < nvp) ask(p + 2 * WAVE, v0, v1);
        const v2f px{c0.x, c1.x}, py{c0.y, c1.y};
        const v2f pf{c0.z, two ? c1.z : 0.0f};
        const v2f pw{NP ? 0.f : c0.w, NP ? 0.f : c1.w};
        road_pair_x2<NP>(px, py, pf, pw, r, ax, ay);
    }
#pragma unroll
    for (int u = 0; u < RPW; u++) f[u] = road_wave_sum(ax[u], ay[u]);
}

}  // namespace csf
