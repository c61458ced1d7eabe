// csf_mid_classes.hip - the one-launch tick (csf_mid.hip) of a mid-size population of SEVERAL PARAMETER SETS AND VEHICLE
// CLASSES, the UncontrolledVehicle's among them (csf_mid_classes).  A translation unit of its own, as csf_small_classes.hip
// is beside csf_agent.hip: the kernels hold agent_body<M, HET = true, FUSED = false, MID> of six classes, and no instance of csf_mid.hip,
// csf_pair.hip or csf_agent.hip is touched.
//
// The workgroup is csf_mid.hip's - wave 0 the per-agent phases of a group of G road users, the other waves the group's pair sums item
// by item from an LDS counter, one barrier between, the records double-buffered and the fp64 snapshot of the tick's start (Dev::rec_w ...,
// Dev::src64) - with what the general path does for such a population put into it:
//   pair items       the plain item of csf_mid_body.inc's Bicycle branch: four receivers against one batch of 64 sources, a source per
//                    lane straight from memory (asked for one item ahead), the precise records in registers.  The lane's source is
//                    evaluated with the PairConsts row of ITS set (vehicle.py:1592-1612, 1095-1101) and masked and handed over with ITS
//                    hfov (intersection.py:733-735) - plain_pair_eval<2, P2R, true>, the field by the source's class.  The rows come from
//                    LDS: staged once per workgroup from Dev::pctab, the tick's rounding bands (set_fov_band: they live in Dev::pc alone)
//                    copied into every row, hfov beside them.  The lane reads Dev::cls[j] with the source record; a padding slot reads
//                    row 0 (plain_pair_sums does the same: padding records are sentinels of any set).  No cull: the far-field bound and
//                    the batch classification are per set.
//   per-agent phases one pass per vehicle CLASS present for each of the two calls: the bits of Dev::model_mask (a kernel argument) asked
//                    one after the other, each a uniform branch around agent_body<M, true, false, MID>, which picks the lane's own row
//                    through agent_params<true> and returns for a lane of another class (as small_classes_kernel's BY_CLASS passes).
//                    Written out and not a loop over the bits with a switch inside: as a loop the six bodies shared one register
//                    allocation across the back edge - 256 VGPRs, 217 of them spilled, 672 bytes of scratch per lane, all of it on
//                    wave 0's path behind the barrier; written out, with a compiler barrier behind each pass, 192 VGPRs and no scratch
//                    (profiles/mid_classes_resource_usage.txt).  The HET path of agent_body holds no barrier, ballot or shuffle (the only
//                    ballot there stands under CHASE, MID == 3).
// Eight waves: the InvPendulum's per-agent code is part of every instance (csf_mid.hip: mid_waves), and 192 VGPRs leave no room for twelve
// (168).  A population that holds a BalancingRiderBicycle keeps the general path (the host asks: tick.inc, mid_takes_classes).
#include "csf_agent_dev.h"
#include "csf_pair_dev.h"
#include "csf_road_dev.h"

namespace csf {

constexpr int MIDC_WAVES = 8;
constexpr int MIDC_ITEMS_MAX = 384;           // (csf_mid.hip: MID_ITEMS_MAX - mid_shape_ok asks for both kernels)

// the per-agent pass of every class present; PHASES / MID: (PH_DEST, 1) in front of the barrier, (PH_COMBINE | PH_INTEGRATE, 2) behind it
#define CSF_MIDC_CLASS_PASS(M, PHASES, MID, RX, RY)                                                                              \
    if ((d.model_mask >> M) & 1) {                                    /* (uniform: the classes of the population, a kernel argument) */ \
        if (mine) agent_body<M, true, false, MID>(d, PHASES, a, nullptr, ka_lines, RX, RY);                                           \
        asm volatile("" ::: "memory");                                /* (nothing of one class's pass is kept for the next) */         \
    }
#define CSF_MIDC_CLASS_PASSES(PHASES, MID, RX, RY)                                                                              \
    CSF_MIDC_CLASS_PASS(CSF_BICYCLE, PHASES, MID, RX, RY)                                                                       \
    CSF_MIDC_CLASS_PASS(CSF_TWOD, PHASES, MID, RX, RY)                                                                          \
    CSF_MIDC_CLASS_PASS(CSF_INVPEND, PHASES, MID, RX, RY)                                                                       \
    CSF_MIDC_CLASS_PASS(CSF_PLANARPOINT, PHASES, MID, RX, RY)                                                                   \
    CSF_MIDC_CLASS_PASS(CSF_PLANARBIKE, PHASES, MID, RX, RY)                                                                    \
    CSF_MIDC_CLASS_PASS(CSF_UNCONTROLLED, PHASES, MID, RX, RY)

// The tick of group `group` of the scene d.  ka_lines: kernarg_touch's result, or 0u where d does not live in the kernarg segment.
template <bool P2R, bool ROAD>
__device__ __forceinline__ void mid_classes_body(const Dev &d, const int group, uint32_t ka_lines) {
    // one partial sum per item - four receivers against one batch of 64 sources -, [2 u + component]: the waves take the items as they
    // come, and the sum over a receiver's items in item order does not depend on who took which
    __shared__ float psum[MIDC_ITEMS_MAX][2 * RPW];
    __shared__ int next_item;
    __shared__ PairConsts ctab[MAX_CLASSES];                      // the sets' rows with this tick's bands (152 B each)
    __shared__ double chfov[MAX_CLASSES];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int G = d.mid_group, sets = G / RPW;
    const int nb = (int)((d.n_src - d.src_beg) >> 6);
    const int items = sets * nb;
    const int64_t g0 = d.lo + (int64_t)group * G;                 // first slot of the group
    const int64_t a = g0 + lane;                                  // (wave 0: lane = road user)
    const int ncl = d.n_classes < MAX_CLASSES ? d.n_classes : MAX_CLASSES;   // (the host admits no more; it indexes LDS)
    kernarg_touched(ka_lines);
    if (threadIdx.x == 0) next_item = 0;
    // the rows, once per workgroup (a thread per set, as stage_classes of csf_small_classes.hip has a lane per road user): the row of
    // Dev::pctab with the bands of this tick's fp32 decisions - the rows of pctab carry none - and the set's hfov beside it
    for (int c = threadIdx.x; c < ncl; c += MIDC_WAVES * WAVE) {
        PairConsts k = d.pctab[c];
        const PairConsts &b = d.pc;
        k.fovA = b.fovA, k.fovB = b.fovB, k.sideA = b.sideA, k.sideB = b.sideB;
        k.fovT0 = b.fovT0, k.fovT1 = b.fovT1, k.clsk = b.clsk;
        k.fovP1 = b.fovP1, k.fovP2 = b.fovP2, k.sideP0 = b.sideP0, k.sideP1 = b.sideP1;
        ctab[c] = k;
        chfov[c] = d.ptab[c].hfov;
    }
    __syncthreads();
    const bool mine = lane < G;
    if (wave == 0) {
        CSF_MIDC_CLASS_PASSES(PH_DEST, 1, 0.0, 0.0)
    } else {   // the pair sums: the other waves take items until there are none left
        auto claim = [&]() {
            int got = 0;
            if (lane == 0) got = atomicAdd(&next_item, 1);
            return __builtin_amdgcn_readfirstlane(got);
        };
        // the sources of an item: one record per lane with the row of its set, straight from memory (asked for one item ahead)
        auto fetch = [&](int item, float4 &q, float2 &o, float2 &qb, int &c) {
            const int64_t j = d.src_beg + ((int64_t)(item % nb) << 6) + lane;
            o = d.rorg[j];
            q = d.rec[j];
            qb = d.has_bike ? d.rec2[j] : make_float2(0.f, 1.f);
            c = j < d.n ? (int)d.cls[j] : 0;                        // (padding records are sentinels of any set)
        };
        int item = claim(), cur_set = -1, c = 0;
        float4 q = make_float4(0.f, 0.f, 1.f, 0.f);
        float2 o = make_float2(0.f, 0.f), qb = make_float2(0.f, 1.f);
        if (item < items) fetch(item, q, o, qb, c);
        Recv r[RPW];
        PreciseRegs pr;
        while (item < items) {
            const int s = item / nb;
            if (s != cur_set) {                                   // (uniform) the receivers of this set: scene coordinates and precise records
                const int64_t j0 = g0 + (int64_t)s * RPW;
#pragma unroll
                for (int u = 0; u < RPW; u++) {
                    const int64_t j = j0 + u < d.hi ? j0 + u : d.hi - 1;   // clamp: results of the duplicates are not used
                    const float4 qr = d.rec[j];
                    const float2 orr = d.rorg[j];
                    pr.rx[u] = qr.x, pr.ry[u] = qr.y, pr.rox[u] = orr.x, pr.roy[u] = orr.y;
                    r[u].x = qr.x + orr.x, r[u].y = qr.y + orr.y, r[u].c = qr.z, r[u].s = qr.w;
                    asm volatile("" : "+v"(r[u].x), "+v"(r[u].y), "+v"(r[u].c), "+v"(r[u].s));  // stay in VGPRs
                }
                cur_set = s;
            }
            const int nxt = claim();
            float4 qn = q;
            float2 on = o, qbn = qb;
            int cn = c;
            if (nxt < items) fetch(nxt, qn, on, qbn, cn);
            float ax[RPW], ay[RPW];
#pragma unroll
            for (int u = 0; u < RPW; u++) ax[u] = ay[u] = 0.0f;
            pr.sx = q.x, pr.sy = q.y, pr.sox = o.x, pr.soy = o.y;
            const float4 qs = make_float4(q.x + o.x, q.y + o.y, q.z, q.w);   // scene coordinates
            const int row = c < ncl ? c : 0;                      // (a row the host has checked, clamped all the same: it indexes LDS)
            plain_pair_eval<2, P2R, true>(d, ctab[row], chfov[row], r, g0 + (int64_t)s * RPW, qs, qb,
                                          (int32_t)(d.src_beg + ((int64_t)(item % nb) << 6) + lane), ax, ay, &pr);
            int idx;
            const float z = reduce8(lane, ax, ay, idx);
            if ((lane & 7) == 0) psum[item][idx] = z;
            item = nxt;
            q = qn;
            o = on;
            qb = qbn;
            c = cn;
        }
        if constexpr (ROAD) {
            // The group's road term as further items of the queue BEHIND the pair items, as in csf_mid_body.inc: item
            // `items + s` is receiver set s against all d.nv_pad vertices, the arithmetic and the order inside a lane road_kernel's
            // (csf_road_dev.h), so d.froad gets the very float that launch would have left.  Lane 0's store has landed before this wave's
            // s_waitcnt vmcnt(0) in front of the barrier; wave 0 asks for d.froad[a] behind it.
            while (item < items + sets) {
                const int s = item - items;
                const int64_t j0 = g0 + (int64_t)s * RPW;
                float rh[RPW][2], rl[RPW][2];
#pragma unroll
                for (int u = 0; u < RPW; u++) {
                    const int64_t j = j0 + u < d.hi ? j0 + u : d.hi - 1;   // clamp: results of the duplicates are not stored
                    const float4 qq = d.rec[j];
                    const float2 oo = d.rorg[j];
                    two_sum(oo.x, qq.x, rh[u][0], rl[u][0]);
                    two_sum(oo.y, qq.y, rh[u][1], rl[u][1]);
                }
                float2 f[RPW];
                switch (d.road_np) {
                case 2: road_sum_from_memory<2>(d, lane, rh, rl, f); break;
                case 3: road_sum_from_memory<3>(d, lane, rh, rl, f); break;
                case 4: road_sum_from_memory<4>(d, lane, rh, rl, f); break;
                case 5: road_sum_from_memory<5>(d, lane, rh, rl, f); break;
                case 6: road_sum_from_memory<6>(d, lane, rh, rl, f); break;
                default: road_sum_from_memory<0>(d, lane, rh, rl, f); break;
                }
#pragma unroll
                for (int u = 0; u < RPW; u++)
                    if (lane == 0 && j0 + u < d.hi) d.froad[j0 + u] = f[u];
                item = claim();
            }
        }
        // (what this wave left in memory for wave 0 - status bits, hand-over entries, with ROAD the road term - has landed before the barrier)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (wave != 0) return;
    double rx = 0.0, ry = 0.0;
    if (mine) {
        const int s = lane / RPW, u = lane % RPW;
        for (int b = 0; b < nb; b++) {
            rx += (double)psum[s * nb + b][2 * u];
            ry += (double)psum[s * nb + b][2 * u + 1];
        }
    }
    CSF_MIDC_CLASS_PASSES(PH_COMBINE | PH_INTEGRATE, 2, rx, ry)
}

template <bool P2R, bool ROAD>
__global__ __launch_bounds__(MIDC_WAVES * WAVE) void mid_classes_kernel(const Dev d) {
    mid_classes_body<P2R, ROAD>(d, (int)blockIdx.x, kernarg_touch<(int)sizeof(Dev) + 4>());
}

// Many independent mid-size scenes of one priority rule in one launch WHATEVER THEIR CLASSES (csf_step_batch): workgroup w ticks group
// groups[w].y of the scene in table slot groups[w].x, its Dev composed from the table's record and the member's MidTick of this tick
// (csf_dev.h: mid_compose) as mid_batch_kernel does it.
template <bool P2R, bool ROAD>
__global__ __launch_bounds__(MIDC_WAVES * WAVE) void mid_classes_batch_kernel(const Dev *__restrict__ table, const MidTick *__restrict__ ticks,
                                                                              const int2 *__restrict__ groups, const int n_groups) {
    if ((int)blockIdx.x >= n_groups) return;                     // (before any load)
    const int2 sg = groups[blockIdx.x];
    Dev dc = table[sg.x];                                        // (the record copied into the kernel: csf_mid.hip, mid_batch_kernel)
    mid_compose(dc, ticks[sg.x]);
    mid_classes_body<P2R, ROAD>(dc, sg.y, 0u);
}

#undef CSF_MIDC_CLASS_PASSES
#undef CSF_MIDC_CLASS_PASS

// a population the kernels are built for (the host asks mid_takes_classes before): the shape of mid_shape_ok, the table within LDS, no
// class but the six
static bool mid_classes_shape_ok(const Dev &d) {
    static_assert(MIDC_ITEMS_MAX == 384, "mid_shape_ok's bound is this kernel's too");
    return mid_shape_ok(d) && d.n_classes >= 1 && d.n_classes <= MAX_CLASSES && (d.model_mask & (1 << CSF_BALANCINGRIDER)) == 0 &&
           d.ptab != nullptr && d.pctab != nullptr && d.pbtab != nullptr && d.cls != nullptr;
}

// false: nothing was launched - the caller must not count the tick as taken
bool launch_mid_classes(const Dev &d, bool road, hipStream_t st) {
    if (!mid_classes_shape_ok(d)) return false;
    const dim3 g((unsigned)((d.hi - d.lo + d.mid_group - 1) / d.mid_group)), b(MIDC_WAVES * WAVE);
    const bool p2r = d.p.priority_rule == CSF_P2R;
    if (p2r && road) hipLaunchKernelGGL((mid_classes_kernel<true, true>), g, b, 0, st, d);
    else if (p2r) hipLaunchKernelGGL((mid_classes_kernel<true, false>), g, b, 0, st, d);
    else if (road) hipLaunchKernelGGL((mid_classes_kernel<false, true>), g, b, 0, st, d);
    else hipLaunchKernelGGL((mid_classes_kernel<false, false>), g, b, 0, st, d);
    return true;
}

void launch_mid_classes_batch(bool p2r, bool road, const Dev *table, const MidTick *ticks, const int2 *groups, int n_groups, hipStream_t st) {
    if (n_groups <= 0) return;
    const dim3 g((unsigned)n_groups), b(MIDC_WAVES * WAVE);
    if (p2r && road) hipLaunchKernelGGL((mid_classes_batch_kernel<true, true>), g, b, 0, st, table, ticks, groups, n_groups);
    else if (p2r) hipLaunchKernelGGL((mid_classes_batch_kernel<true, false>), g, b, 0, st, table, ticks, groups, n_groups);
    else if (road) hipLaunchKernelGGL((mid_classes_batch_kernel<false, true>), g, b, 0, st, table, ticks, groups, n_groups);
    else hipLaunchKernelGGL((mid_classes_batch_kernel<false, false>), g, b, 0, st, table, ticks, groups, n_groups);
}

}  // namespace csf
