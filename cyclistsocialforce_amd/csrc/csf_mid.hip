// csf_mid.hip — the whole tick of a mid-size population (a few dozen to ~1 300 road users) in ONE launch.
//
// Replaces, per tick, the same reference code as csf_pair.hip + csf_agent.hip together: get_untracked_foes
// (intersection.py:690-745), the N calls of calcRepulsiveForce and the column sum (:814-843), the clamp and the road term
// (:841-857), and vehicle.step for every road user (:891-892) - SocialForceIntersection.step (:866-896).
//
// Between 33 and ~1 300 road users - BASELINE config 2 (1 024 TwoDBicycle), and what the reference itself runs under SUMO -
// the tick is latency, not work: the plain pair launch and the per-agent launch take 8 + 7 us at N = 1 024, of which ~9 us are
// the two launches' fixed cost (dispatch, first round trips, teardown).  Here ONE WORKGROUP of twelve waves (eight for the
// InvPendulum's per-agent code) owns a group of G road users (4 ... 32 slots, so that the grid is about one workgroup per CU)
// for the whole tick:
//
//   wave 0        the destination-force phase of the group's road users - queue, navigation state, planner: it needs no sums -
//                 (csf_agent_dev.h: agent_body, lane = road user) ...
//   the others    ... while they form the group's repulsive sums, item by item from an LDS counter, sources in the lanes, straight
//                 from the records in memory, asked for one item ahead.  (ROAD instances, below: behind the pair items the same
//                 queue hands out the group's road term, four receivers against all vertices of a small road per item -
//                 csf_road_dev.h)  The pair items, TwoD field: an item is ONE receiver (wave-uniform, in
//                 scalar registers) against four batches of 64 sources, cull first as in csf_pair.hip - two batches at a time
//                 through the field-of-view test on packed arithmetic, the tracked sources to a queue in LDS, the packed field on
//                 what the queue holds, the rare pairs (near, marginal, on the line ahead of a source) one per lane on the precise
//                 records.  Bicycle field: an item is four receivers against one batch (csf_pair_dev.h: plain_pair_eval - the very
//                 code of pair_kernel).  Column sum by lane exchange, one partial per item (and receiver) to LDS;
//   barrier
//   wave 0        adds a receiver's partials in item order (fp64; whoever took which item: bit-reproducible) and runs the rest
//                 of the per-agent tick: hand-overs, clamp, road term, controller + kinematics, ring, next tick's records.
//
// Nothing leaves the workgroup between the phases: no partial sums in memory, no counters, no fences, no workgroup ever looks at
// another's progress (a first version split a group's sums over several workgroups and let the last one to arrive carry on:
// the arrival protocol - write-through stores, an agent-scope atomic, agent-scope loads - put 3 us of memory round trips on
// every group's critical path, and the per-agent code's 255 registers halved the residency of the pair workgroups: 13 us per
// tick at N = 64 ... 512 against 12.5 with two launches, 22 against 15 at N = 1 024; with __threadfence() 80).  What one
// launch per tick does cost is a DOUBLE BUFFER: a group writes its road users' next records while other groups still read
// this tick's, so the records (rec, recg, rec2) exist twice and the launch writes the half it does not read (Dev::rec_w ...);
// the fp64 positions that undecidable pairs are handed over with come from a snapshot of the tick's start (Dev::src64), which
// the per-agent phase renews for the next tick in the other half as well.
#include "csf_agent_dev.h"
#include "csf_pair_dev.h"
#include "csf_road_dev.h"

namespace csf {

// waves of a workgroup: twelve where the per-agent code of the vehicle class leaves room for three waves per SIMD (168 registers),
// else eight (InvPendulum; the BalancingRider's per-agent chain is longer still and its one-launch tick was measured no faster than
// two launches - 16.4 against 15.6 us at 1 024 riders -: csf_engine.hip keeps that class on two launches) - one workgroup per CU either way, and one more wave per SIMD on the pair sums
__host__ __device__ constexpr int mid_waves(int model) { return model == CSF_INVPEND ? 8 : 12; }
constexpr int MID_GROUP_MAX = 32;             // road users (slots) of a group at most
constexpr int MID_ITEMS_MAX = 384;            // (receiver set, source batch) items of a group at most: 12 KB of partial sums
constexpr int MID_SB = 4;                     // TwoD field: source batches of an item (one receiver against 256 sources)

// ROAD: the pair waves also sum the road term of the group's road users, as items of the same queue behind the pair
// items, where the launch would otherwise follow road_kernel's; everything of it sits under if constexpr (ROAD) in the body, and the
// host picks the instance (tick.inc: mid_road_ok) - Dev is the same.
template <int MODEL, bool P2R, bool ROAD>
__global__ __launch_bounds__(mid_waves(MODEL) * WAVE) void mid_tick_kernel(const Dev d) {
#define MID_GROUP_INDEX blockIdx.x
#define MID_KERNARG_LINES kernarg_touch<(int)sizeof(Dev) + 4>()
#include "csf_mid_body.inc"
#undef MID_GROUP_INDEX
#undef MID_KERNARG_LINES
}

// Many independent mid-size scenes of one vehicle class and priority rule in one launch (csf_step_batch): workgroup w ticks group
// groups[w].y of the scene in table slot groups[w].x.  The workgroups of a tick never look at each other (above), so those of
// different scenes share a grid as they are.  The table holds every member's Dev in a form that does not change from tick to
// tick - the halves of the double buffers by name (rec: the engine's first half, rec_w: its second), tick, stamp and rounding
// bands zero -; what does change is the member's MidTick of this tick, and the kernel composes its Dev from the two.
template <int MODEL, bool P2R, bool ROAD>
__global__ __launch_bounds__(mid_waves(MODEL) * WAVE) void mid_batch_kernel(const Dev *__restrict__ table, const MidTick *__restrict__ ticks,
                                                                            const int2 *__restrict__ groups, const int n_groups) {
    if ((int)blockIdx.x >= n_groups) return;                     // (before any load)
    const int2 sg = groups[blockIdx.x];
    // (the record copied into the kernel, as the single-scene kernel has it in its kernarg segment: csf_agent.hip, small_batch_kernel)
    Dev dc = table[sg.x];
    mid_compose(dc, ticks[sg.x]);
    const Dev &d = dc;
#define MID_GROUP_INDEX sg.y
#define MID_KERNARG_LINES 0u
#include "csf_mid_body.inc"
#undef MID_GROUP_INDEX
#undef MID_KERNARG_LINES
}

// a shape the kernel is built for (csf_engine.hip: mid_fused_ok asks before)
bool mid_shape_ok(const Dev &d) {
    if (d.hi <= d.lo || d.mid_group < RPW || d.mid_group > MID_GROUP_MAX || d.mid_group % RPW != 0) return false;
    return (d.mid_group / RPW) * ((d.n_src - d.src_beg) >> 6) <= MID_ITEMS_MAX;
}

void launch_mid_batch(int model, bool p2r, bool road, const Dev *table, const MidTick *ticks, const int2 *groups, int n_groups, hipStream_t st) {
    if (n_groups <= 0) return;
    const dim3 g((unsigned)n_groups);
#define CSF_MIDB2(MODEL, ROAD)                                                                                                               \
    if (p2r) hipLaunchKernelGGL((mid_batch_kernel<MODEL, true, ROAD>), g, dim3(mid_waves(MODEL) * WAVE), 0, st, table, ticks, groups, n_groups); \
    else hipLaunchKernelGGL((mid_batch_kernel<MODEL, false, ROAD>), g, dim3(mid_waves(MODEL) * WAVE), 0, st, table, ticks, groups, n_groups)
#define CSF_MIDB(MODEL)                 \
    if (road) {                         \
        CSF_MIDB2(MODEL, true);         \
    } else {                            \
        CSF_MIDB2(MODEL, false);        \
    }
    switch (model) {
    case CSF_BICYCLE: CSF_MIDB(CSF_BICYCLE); break;
    case CSF_TWOD: CSF_MIDB(CSF_TWOD); break;
    case CSF_INVPEND: CSF_MIDB(CSF_INVPEND); break;
    case CSF_PLANARBIKE: CSF_MIDB(CSF_PLANARBIKE); break;
    default: CSF_MIDB(CSF_PLANARPOINT); break;
    }
#undef CSF_MIDB
#undef CSF_MIDB2
}

// false: nothing was launched (a shape this kernel is not built for) - the caller must not count the tick as taken
// road: the ROAD instance - the launch sums the road term itself and no launch_road goes in front of it (the caller has asked mid_road_ok)
bool launch_mid_tick(const Dev &d, bool road, hipStream_t st, hipEvent_t t0, hipEvent_t t1) {
    if (!mid_shape_ok(d)) return false;
    const dim3 g((unsigned)((d.hi - d.lo + d.mid_group - 1) / d.mid_group));
    const bool p2r = d.p.priority_rule == CSF_P2R;
#define CSF_MID2(MODEL, ROAD)                                                                                            \
    if (p2r) hipExtLaunchKernelGGL((mid_tick_kernel<MODEL, true, ROAD>), g, dim3(mid_waves(MODEL) * WAVE), 0, st, t0, t1, 0, d);       \
    else hipExtLaunchKernelGGL((mid_tick_kernel<MODEL, false, ROAD>), g, dim3(mid_waves(MODEL) * WAVE), 0, st, t0, t1, 0, d)
#define CSF_MID(MODEL)                 \
    if (road) {                        \
        CSF_MID2(MODEL, true);         \
    } else {                           \
        CSF_MID2(MODEL, false);        \
    }
    switch (d.p.model) {
    case CSF_BICYCLE: CSF_MID(CSF_BICYCLE); break;
    case CSF_TWOD: CSF_MID(CSF_TWOD); break;
    case CSF_INVPEND: CSF_MID(CSF_INVPEND); break;
    case CSF_PLANARBIKE: CSF_MID(CSF_PLANARBIKE); break;
    default: CSF_MID(CSF_PLANARPOINT); break;
    }
#undef CSF_MID
#undef CSF_MID2
    return true;
}

}  // namespace csf
