// csf_scene.hip — calibration of the interaction parameters on the device: many parameter sets x many closed-loop scenes in ONE
// launch, the error against the recorded trajectories summed here.
//
// csf_calib.hip replays recorded forces: no two vehicles are coupled, and the social-force field (f_0, sigma_0..3, e_0, e_1, hfov,
// p_0, p_decay, the priority rule) never acts.  Here the riders of a scene are simulated together by the one-wave tick
// (csf_small_body.inc), workgroup = (candidate set, scene):
//
//   b = set * n_scn + scene            table[b] is the Dev view of the scene's slot block (slot = set * R + rider, pointers shifted
//                                      to the block, n = the scene's riders); p / pc / pb come from the call's table of sets
//   before tick 0                      the block becomes the fresh vehicles of the scene, from the image (csf_scene.h)
//   t = 0 .. len[scene] - 1            one closed-loop tick; then, per rider, d = state - objective[t][rider][f] over the
//                                      objective's features, sum d^2 and sum |d| in fp64, tick order, features in column order
//   at the end                         (sum d^2, sum |d|) -> sums[set * R + rider] in mapped host memory; the host adds the riders
//                                      of a scene in rider order (no reduction across lanes: the order of the sum is fixed)
//
// A rider that follows its recording (csf_scene_calib_replay) is ticked like every other - agent_body is called
// inside small_tick_body - and its lane then overwrites (x, y, psi, v) with the recorded row of that tick: the sources every lane
// reads at the top of the next tick (csf_small_body.inc: sx, sy, spsi, and se of the Bicycle field) are rows 0 - 3 of d.s, so the
// others see the recording.  What the lane does not overwrite - delta, theta, lti, znav, znp, ptr, the status word - is its own and
// read by no other lane; a status bit it raises says nothing about the evaluation.  No loop of agent_body<.., FUSED = true> depends
// on the state for its end: the poll loop and the edge chain are compiled out (CHASE, edge_pending are false), update_destination
// moves the pointer by at most 2, the scaling loop of invpend_step_yaw stops at 40 halvings and at a NaN norm, every other loop has
// a constant trip count - a rider whose state is reset every tick cannot hold its wave.
//
// Scenes with road edges (csf_scene_calib_road): the view of a scene with a road carries rv / rvo / nv / nv_pad /
// road_np and the origin of a stand-alone engine that holds the scene, and small_tick_body stages and sums the road as it does for
// small_batch_kernel, in dynamic LDS sized by the largest road of the data set.  Road parameters per candidate set: see the prologue.
//
// Road users that enter and leave (csf_scene_calib_windows): rider r is in its scene at the ticks win_enter[r] <= t <
// win_exit[r].  Every lane keeps the two bounds of its rider in registers, one ballot per tick makes the presence mask of the scene
// (SceneHook::present), and small_tick_body gates the pair loop, the road term and agent_body with it; the hook below returns before
// the replay / error part for an absent rider.  Before its entry the slot holds what the restore at the head of the launch put there -
// nothing ticks it - so s0 IS the state at the start of tick win_enter[r]; after its exit it keeps its last state.  A data set without
// windows launches scene_eval_kernel<MODEL, false>, where all of this is compiled out.
//
// Rosters that share the lanes of their scene (csf_scene_calib_load_shared): scene_lanes_kernel.  The workgroup runs
// the scene's LANES, and a lane carries the riders of its chain (csf_scene.h) one after the other: at the head of the tick its next
// rider enters at, the lane writes the sums of the rider it carried and makes its slot the newcomer's fresh vehicle from the image -
// SceneLaneHook::takeover, the restore of the launch's head once more.  Sums and samples stay per RIDER; a sample row is written
// only at a tick its rider is present (the host has filled the rest with NaN).
//
// Scenes with more than 32 road users at once (csf_scene_calib_load_wide): scene_wide_kernel.  One workgroup of 256
// threads runs up to WIDE_MAX lanes for all ticks of the scene - wide_tick_body (csf_wide_body.inc), the tick of small_tick_body with
// LDS and workgroup barriers where that one has shuffles and the wave's program order - behind SceneLaneHook, so chains, windows,
// replay, samples and sums are those of scene_lanes_kernel.  An evaluation of such a data set is up to two launches on one stream.
//
// Rider groups with parameter sets of their own (csf_scene_calib_groups): scene_groups_kernel.  The call's table holds
// n_groups records per candidate set, a rider is ticked with its group's record and acts as a source with that record's field and field
// of view (csf_small_body.inc: HOOK::GROUPS).  A data set without groups launches scene_eval_kernel, where none of this exists.
//
// Rider groups on shared lanes and on wide scenes (csf_scene_calib_lane_groups): scene_lanes_groups_kernel and
// scene_wide_groups_kernel.  The group is a property of the RIDER, so a lane's group changes at a takeover: SceneLaneHook<MODEL, true>::seat
// takes it from c.group, restores with the limits of that record and renews the lane's cell of the staged table of source groups.  A
// data set without groups launches scene_lanes_kernel / scene_wide_kernel, where none of this exists.
//
// Several vehicle classes in one scene (csf_scene_calib_classes): scene_mixed_kernel.  It is scene_groups_kernel with the
// vehicle class a property of the group: the record of a group names its class, a source acts with the field of its class, the per-agent
// tick is a uniform switch to agent_body<M> inside the loop over the groups (csf_small_body.inc: SMALL_MIXED), and the replay write-back of
// scene_rider_step branches on the rider's class at run time.  The image the restore reads was rewritten per rider and class by the host
// (abi_scene.inc), and the views' state width is the call's widest class.  A data set without classes launches what it launched before.
//
// Vehicle classes on shared lanes and on wide scenes (csf_scene_calib_lane_classes): scene_lanes_mixed_kernel and
// scene_wide_mixed_kernel in csf_scene_mixed.hip - scene_lanes_groups_kernel / scene_wide_groups_kernel with the class a property of the
// group, so of the rider a lane carries: SceneLaneHook<SMALL_MIXED, true>::seat also makes the lane's class the newcomer's, the tick stages
// the Bicycle cell and picks agent_body<M> by it (csf_small_body.inc, csf_wide_body.inc: SMALL_MIXED), and the replay write-back is that of
// the rider's class.  SceneLaneHook stands in csf_scene_hook.inc for that; no kernel of this file changed.
//
// What exists once ("Folded"): scene_rider_step - the replay write-back or the error terms behind a tick, called by both
// hooks (csf_scene_hook.inc) -, and for_vehicle_class (csf_agent_dev.h), which turns the class of the call into the template argument of whatever is launched.  scene_restore - a
// slot becomes a fresh vehicle from the image - serves scene_groups_kernel and SceneLaneHook::seat; scene_eval_kernel has the same lines
// written out.  The per-set prologue is written out in all four kernels, and scene_groups_kernel / scene_wide_kernel repeat the skeleton
// of scene_eval_kernel / scene_lanes_kernel: with one function for either, sums and states were no longer the parent's bit for bit.
//
// The Dev is copied into the kernel (read through a reference to global memory the compiler contracted a few fp64
// chains differently).  A scene that has ended keeps its last state in every later sample of the optional trajectories.
#include <type_traits>

#include "csf_agent_dev.h"
#include "csf_field.h"
#include "csf_scene.h"

namespace csf {

#include "csf_small_body.inc"
#include "csf_wide_body.inc"

#include "csf_scene_hook.inc"

template <int MODEL, bool WIN>
__global__ __launch_bounds__(64) void scene_eval_kernel(const Dev *__restrict__ table, const SceneSet *__restrict__ sets, const SceneDev c) {
    extern __shared__ float4 srv[];                           // c.road_lds bytes: the largest road of the data set (none: 0 bytes)
    const int b = (int)blockIdx.x;
    if (b >= c.n_sets * c.n_scn) return;
    const int set = b / c.n_scn, scn = b - set * c.n_scn;
    Dev d = table[b];
    {
        const SceneSet ss = sets[set];
        d.p = ss.p;
        d.pc = ss.pc;
#pragma unroll
        for (int k = 0; k < 7; k++) d.pb[k] = ss.pb[k];
        // road parameters of this set: the scene's road with (-F0, -(sigma + 1) / 2) of the set on every vertex - padding keeps
        // F0 = 0 - goes to this workgroup's own block, and the tick stages it from there.  The tick reads rv[v] for v = thread,
        // thread + WAVE, ...: what the same lane has stored here, program order - as the restored block below.
        if (c.road_blk != nullptr && d.nv_pad > 0) {
            float4 *const blk = c.road_blk + (int64_t)set * c.road_stride + (d.rv - c.road_rv);
            const int nv = (int)d.nv, nvp = (int)d.nv_pad;
            for (int v = (int)threadIdx.x; v < nvp; v += WAVE) {
                float4 r = d.rv[v];
                if (v < nv) r.z = ss.road_z, r.w = ss.road_w;
                blk[v] = r;
            }
            d.rv = blk;
            d.road_np = ss.road_np;
        }
    }
    const int lane = (int)threadIdx.x, n = (int)d.n;
    const int64_t first = c.roff[scn];
    const int len = c.len[scn];
    // The restore written out, a second copy of scene_restore: with the call in its place scene_eval_kernel<InvPendulum, false> takes
    // 0.7 - 1.1 % longer on scenes with a road ("Folded").  An array added to the image goes into both.
    if (lane < n) {
        const int64_t a = lane, r = first + lane, cap = d.cap, ic = c.img_cap;
#pragma unroll
        for (int k = 0; k < STATE_ROWS; k++) d.s[k * cap + a] = c.img_s[k * ic + r];
#pragma unroll
        for (int k = 0; k < 5; k++) d.lti[k * cap + a] = c.img_lti[k * ic + r];
#pragma unroll
        for (int k = 0; k < 3; k++) d.znp[k * cap + a] = c.img_znp[k * ic + r];
#pragma unroll
        for (int k = 0; k < 6; k++) d.F[k * cap + a] = 0.0;
        d.ppsi[a] = c.img_ppsi[r];
        d.ti[a] = c.img_ti[r];
        d.status[a] = c.img_status[r];
        d.ptr[a] = c.img_ptr[r];
        d.znav[a] = c.img_znav[r];
        d.hx[a] = c.img_hx0[r];
        d.hy[a] = c.img_hy0[r];
        const double v = c.img_s[3 * ic + r], delta = c.img_s[4 * ic + r];
        d.zrid[a] = v < d.p.v_max_walk ? 0 : 1;
        d.dgood[a] = (-d.p.delta_max_walk < delta && d.p.delta_max_walk > delta) ? 1 : 0;
    }
    // (the restored block is read by every lane of this wave in the first tick: the wave's own stores, program order - as from
    // tick to tick in small_tick_body)
    const int64_t rider = (int64_t)set * c.R + first + lane;
    // (rep_index, win_enter / win_exit and group have R entries: read by the lanes that have a rider only)
    const int rcol = c.rep != nullptr && lane < n ? c.rep_index[first + lane] : -1;
    const int t_in = WIN && lane < n ? c.win_enter[first + lane] : 0, t_out = WIN && lane < n ? c.win_exit[first + lane] : 0;
    SceneHook<MODEL, WIN> hook(c, rider, c.obj + (first + lane) * c.n_feat, rcol >= 0 ? c.rep + (int64_t)rcol * 4 : nullptr,
                               c.states != nullptr && lane < n ? c.states + rider * d.ns : nullptr, t_in, t_out);
    small_tick_body<MODEL>(d, len, nullptr, srv, 0u, 0, hook);
    if (lane >= n) return;
    c.sums[rider] = make_double2(hook.sse, hook.sae);
    // an ended (or empty) scene keeps its last state in every later sample
    if (hook.smp != nullptr)
        while (hook.taken < c.n_samples) hook.sample(d, lane);
}

// Rider groups (csf_scene_calib_groups): scene_eval_kernel with the parameters a property of the RIDER.  `sets` holds
// c.n_groups records per candidate set; Dev::p / pc / pb become record 0's (the priority rule and the road entries are the set's), the
// restore takes the limits of the rider's own record, and the tick reads the rest through the hook (csf_small_body.inc: HOOK::GROUPS).
// The kernel is scene_eval_kernel line for line around the staging of the groups - prologue, hook, epilogue: a change to one is made in
// the other.  The two are not one body, and the prologue is not one function: either gave other bits ("Folded").
template <int MODEL, bool WIN>
__global__ __launch_bounds__(64) void scene_groups_kernel(const Dev *__restrict__ table, const SceneSet *__restrict__ sets, const SceneDev c) {
    extern __shared__ float4 srv[];                           // as scene_eval_kernel
    __shared__ PairConsts g_pc[SCENE_GROUPS_MAX];
    __shared__ double g_hfov[SCENE_GROUPS_MAX], g_vref[SCENE_GROUPS_MAX];
    __shared__ uint8_t g_of[SMALL_MAX];
    const int b = (int)blockIdx.x;
    if (b >= c.n_sets * c.n_scn) return;
    const int set = b / c.n_scn, scn = b - set * c.n_scn;
    const int G = c.n_groups < SCENE_GROUPS_MAX ? c.n_groups : SCENE_GROUPS_MAX;   // (the host refuses more; LDS holds no more)
    const SceneSet *const rec = sets + (int64_t)set * c.n_groups;
    Dev d = table[b];
    {
        const SceneSet ss = rec[0];
        d.p = ss.p;
        d.pc = ss.pc;
#pragma unroll
        for (int k = 0; k < 7; k++) d.pb[k] = ss.pb[k];
        if (c.road_blk != nullptr && d.nv_pad > 0) {          // road parameters of this set: a copy of scene_eval_kernel's lines, one of four
            float4 *const blk = c.road_blk + (int64_t)set * c.road_stride + (d.rv - c.road_rv);
            const int nv = (int)d.nv, nvp = (int)d.nv_pad;
            for (int v = (int)threadIdx.x; v < nvp; v += WAVE) {
                float4 r = d.rv[v];
                if (v < nv) r.z = ss.road_z, r.w = ss.road_w;
                blk[v] = r;
            }
            d.rv = blk;
            d.road_np = ss.road_np;
        }
    }
    const int lane = (int)threadIdx.x, n = (int)d.n;
    const int64_t first = c.roff[scn];
    const int len = c.len[scn];
    // (an entry the host has checked, clamped all the same: it indexes LDS)
    int grp = lane < n ? (int)c.group[first + lane] : 0;
    grp = grp < G ? grp : G - 1;
    // the groups' constants to LDS: lane g < G copies record g word by word; then the wave's own stores, program order (as sx, sy)
    if (lane < G) {
        g_pc[lane] = rec[lane].pc;
        g_hfov[lane] = rec[lane].p.hfov;
        g_vref[lane] = rec[lane].p.v_max_riding[1];
    }
    if (lane < SMALL_MAX) g_of[lane] = (uint8_t)grp;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < n) scene_restore(d, c, lane, first + lane, rec[grp].p.v_max_walk, rec[grp].p.delta_max_walk);
    const int64_t rider = (int64_t)set * c.R + first + lane;
    const int rcol = c.rep != nullptr && lane < n ? c.rep_index[first + lane] : -1;
    const int t_in = WIN && lane < n ? c.win_enter[first + lane] : 0, t_out = WIN && lane < n ? c.win_exit[first + lane] : 0;
    SceneHook<MODEL, WIN, true> hook(c, rider, c.obj + (first + lane) * c.n_feat, rcol >= 0 ? c.rep + (int64_t)rcol * 4 : nullptr,
                                     c.states != nullptr && lane < n ? c.states + rider * d.ns : nullptr, t_in, t_out);
    hook.n_groups = G, hook.grp = grp, hook.rec = rec;
    hook.l_pc = g_pc, hook.l_hfov = g_hfov, hook.l_vref = g_vref, hook.l_grp = g_of;
    small_tick_body<MODEL>(d, len, nullptr, srv, 0u, 0, hook);
    if (lane >= n) return;
    c.sums[rider] = make_double2(hook.sse, hook.sae);
    if (hook.smp != nullptr)
        while (hook.taken < c.n_samples) hook.sample(d, lane);
}

template <int MODEL>
__global__ __launch_bounds__(64) void scene_lanes_kernel(const Dev *__restrict__ table, const SceneSet *__restrict__ sets, const SceneDev c) {
    extern __shared__ float4 srv[];                           // as scene_eval_kernel
    const int b = (int)blockIdx.x;
    if (b >= c.n_sets * c.n_scn) return;
    const int set = b / c.n_scn, scn = b - set * c.n_scn;
    Dev d = table[b];
    {
        const SceneSet ss = sets[set];
        d.p = ss.p;
        d.pc = ss.pc;
#pragma unroll
        for (int k = 0; k < 7; k++) d.pb[k] = ss.pb[k];
        if (c.road_blk != nullptr && d.nv_pad > 0) {          // road parameters of this set: a copy of scene_eval_kernel's lines, one of four
            float4 *const blk = c.road_blk + (int64_t)set * c.road_stride + (d.rv - c.road_rv);
            const int nv = (int)d.nv, nvp = (int)d.nv_pad;
            for (int v = (int)threadIdx.x; v < nvp; v += WAVE) {
                float4 r = d.rv[v];
                if (v < nv) r.z = ss.road_z, r.w = ss.road_w;
                blk[v] = r;
            }
            d.rv = blk;
            d.road_np = ss.road_np;
        }
    }
    const int lane = (int)threadIdx.x, n = (int)d.n;          // n: the scene's lanes
    const int64_t row0 = (int64_t)set * c.R;
    SceneLaneHook<MODEL> hook(c, row0);
    // the first rider of every lane is seated here whenever it enters, as scene_eval_kernel restores everybody at its head: before
    // its entry nothing ticks the slot.  A lane nobody ever rides keeps what it holds and is never present.
    if (lane < n) {
        const int r = c.lane_first[c.lane_off[scn] + lane];
        if (r >= 0) hook.seat(d, lane, r);
    }
    small_tick_body<MODEL>(d, c.len[scn], nullptr, srv, 0u, 0, hook);
    // riders that are never present are in no chain: their sums are (0, 0)
    for (int r = c.roff[scn] + lane; r < c.roff[scn + 1]; r += WAVE)
        if (c.win_enter[r] >= c.win_exit[r]) c.sums[row0 + r] = make_double2(0.0, 0.0);
    // (a chain holds non-empty windows that end within the scene: every rider of it has been seated by the last tick)
    if (lane < n) hook.flush();
}

// wide scenes: one workgroup of 256 threads per (set, wide scene), scn_w[0 .. n_wide) the wide scenes of the data set.  The kernel is
// scene_lanes_kernel line for line but for where the scene comes from, the stride and wide_tick_body; a change to one is made in the other;
// they are not one body for the reason given at scene_groups_kernel.
template <int MODEL>
__global__ __launch_bounds__(256) void scene_wide_kernel(const Dev *__restrict__ table, const SceneSet *__restrict__ sets, const SceneDev c,
                                                         const int32_t *__restrict__ scn_w, const int n_wide) {
    extern __shared__ float4 srv[];                           // as scene_eval_kernel
    const int b = (int)blockIdx.x;
    if (b >= c.n_sets * n_wide) return;                       // (the only early return: before any barrier, the same in every thread)
    const int set = b / n_wide, scn = scn_w[b - set * n_wide];
    Dev d = table[b];
    {
        const SceneSet ss = sets[set];
        d.p = ss.p;
        d.pc = ss.pc;
#pragma unroll
        for (int k = 0; k < 7; k++) d.pb[k] = ss.pb[k];
        if (c.road_blk != nullptr && d.nv_pad > 0) {          // road parameters of this set: a copy of scene_eval_kernel's lines, one of four
            float4 *const blk = c.road_blk + (int64_t)set * c.road_stride + (d.rv - c.road_rv);
            const int nv = (int)d.nv, nvp = (int)d.nv_pad;
            for (int v = (int)threadIdx.x; v < nvp; v += WIDE_MAX) {
                float4 r = d.rv[v];
                if (v < nv) r.z = ss.road_z, r.w = ss.road_w;
                blk[v] = r;
            }
            d.rv = blk;
            d.road_np = ss.road_np;
        }
    }
    const int lane = (int)threadIdx.x, n = (int)d.n;          // n: the scene's lanes (1 .. WIDE_MAX)
    const int64_t row0 = (int64_t)set * c.R;
    SceneLaneHook<MODEL> hook(c, row0);
    if (lane < n) {
        const int r = c.lane_first[c.lane_off[scn] + lane];
        if (r >= 0) hook.seat(d, lane, r);
    }
    wide_tick_body<MODEL>(d, c.len[scn], srv, hook);
    // riders that are never present are in no chain: their sums are (0, 0)
    for (int r = c.roff[scn] + lane; r < c.roff[scn + 1]; r += (int)blockDim.x)
        if (c.win_enter[r] >= c.win_exit[r]) c.sums[row0 + r] = make_double2(0.0, 0.0);
    if (lane < n) hook.flush();
}

// Rider groups on shared lanes (csf_scene_calib_lane_groups): scene_lanes_kernel with the parameters a property of the
// RIDER a lane carries.  `sets` holds c.n_groups records per candidate set, Dev::p / pc / pb become record 0's (the priority rule and the
// road entries are the set's), and the tick reads the rest through the hook (csf_small_body.inc: HOOK::GROUPS).  The kernel is
// scene_lanes_kernel line for line around the staging of the groups, and the staging is scene_groups_kernel's but for the table of the
// lanes' groups, which starts at 0 and is filled by SceneLaneHook::seat: a change to one is made in the others.  Not one body with
// either, for the reason given at scene_groups_kernel.
template <int MODEL>
__global__ __launch_bounds__(64) void scene_lanes_groups_kernel(const Dev *__restrict__ table, const SceneSet *__restrict__ sets, const SceneDev c) {
    extern __shared__ float4 srv[];                           // as scene_eval_kernel
    __shared__ PairConsts g_pc[SCENE_GROUPS_MAX];
    __shared__ double g_hfov[SCENE_GROUPS_MAX], g_vref[SCENE_GROUPS_MAX];
    __shared__ uint8_t g_of[SMALL_MAX];                       // the group of every LANE: that of the rider it carries
    const int b = (int)blockIdx.x;
    if (b >= c.n_sets * c.n_scn) return;
    const int set = b / c.n_scn, scn = b - set * c.n_scn;
    const int G = c.n_groups < SCENE_GROUPS_MAX ? c.n_groups : SCENE_GROUPS_MAX;   // (the host refuses more; LDS holds no more)
    const SceneSet *const rec = sets + (int64_t)set * c.n_groups;
    Dev d = table[b];
    {
        const SceneSet ss = rec[0];
        d.p = ss.p;
        d.pc = ss.pc;
#pragma unroll
        for (int k = 0; k < 7; k++) d.pb[k] = ss.pb[k];
        if (c.road_blk != nullptr && d.nv_pad > 0) {          // road parameters of this set: a copy of scene_eval_kernel's lines
            float4 *const blk = c.road_blk + (int64_t)set * c.road_stride + (d.rv - c.road_rv);
            const int nv = (int)d.nv, nvp = (int)d.nv_pad;
            for (int v = (int)threadIdx.x; v < nvp; v += WAVE) {
                float4 r = d.rv[v];
                if (v < nv) r.z = ss.road_z, r.w = ss.road_w;
                blk[v] = r;
            }
            d.rv = blk;
            d.road_np = ss.road_np;
        }
    }
    const int lane = (int)threadIdx.x, n = (int)d.n;          // n: the scene's lanes
    const int64_t row0 = (int64_t)set * c.R;
    // the groups' constants to LDS: lane g < G copies record g word by word; every lane starts in group 0.  Then the wave's own stores,
    // program order (as sx, sy); seat below stores to the lane's own cell behind this lane's store of the 0.
    if (lane < G) {
        g_pc[lane] = rec[lane].pc;
        g_hfov[lane] = rec[lane].p.hfov;
        g_vref[lane] = rec[lane].p.v_max_riding[1];
    }
    if (lane < SMALL_MAX) g_of[lane] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    SceneLaneHook<MODEL, true> hook(c, row0);
    hook.n_groups = G, hook.rec = rec;
    hook.l_pc = g_pc, hook.l_hfov = g_hfov, hook.l_vref = g_vref, hook.l_grp = g_of, hook.w_grp = g_of;
    if (lane < n) {
        const int r = c.lane_first[c.lane_off[scn] + lane];
        if (r >= 0) hook.seat(d, lane, r);
    }
    small_tick_body<MODEL>(d, c.len[scn], nullptr, srv, 0u, 0, hook);
    // riders that are never present are in no chain: their sums are (0, 0)
    for (int r = c.roff[scn] + lane; r < c.roff[scn + 1]; r += WAVE)
        if (c.win_enter[r] >= c.win_exit[r]) c.sums[row0 + r] = make_double2(0.0, 0.0);
    if (lane < n) hook.flush();
}

// ... and on wide scenes: scene_wide_kernel line for line around the same staging, a change to one is made in the other.  What thread g < G
// stages is read by every thread at the head of the first tick (wide_tick_body: hook.v_ref) - other waves, so a workgroup barrier stands
// behind the staging, reached by all 256 threads: the only return in front of it is the uniform one.
template <int MODEL>
__global__ __launch_bounds__(256) void scene_wide_groups_kernel(const Dev *__restrict__ table, const SceneSet *__restrict__ sets, const SceneDev c,
                                                                const int32_t *__restrict__ scn_w, const int n_wide) {
    extern __shared__ float4 srv[];                           // as scene_eval_kernel
    __shared__ PairConsts g_pc[SCENE_GROUPS_MAX];
    __shared__ double g_hfov[SCENE_GROUPS_MAX], g_vref[SCENE_GROUPS_MAX];
    __shared__ uint8_t g_of[WIDE_MAX];                        // the group of every LANE: that of the rider it carries
    const int b = (int)blockIdx.x;
    if (b >= c.n_sets * n_wide) return;                       // (the only early return: before any barrier, the same in every thread)
    const int set = b / n_wide, scn = scn_w[b - set * n_wide];
    const int G = c.n_groups < SCENE_GROUPS_MAX ? c.n_groups : SCENE_GROUPS_MAX;   // (the host refuses more; LDS holds no more)
    const SceneSet *const rec = sets + (int64_t)set * c.n_groups;
    Dev d = table[b];
    {
        const SceneSet ss = rec[0];
        d.p = ss.p;
        d.pc = ss.pc;
#pragma unroll
        for (int k = 0; k < 7; k++) d.pb[k] = ss.pb[k];
        if (c.road_blk != nullptr && d.nv_pad > 0) {          // road parameters of this set: a copy of scene_eval_kernel's lines
            float4 *const blk = c.road_blk + (int64_t)set * c.road_stride + (d.rv - c.road_rv);
            const int nv = (int)d.nv, nvp = (int)d.nv_pad;
            for (int v = (int)threadIdx.x; v < nvp; v += WIDE_MAX) {
                float4 r = d.rv[v];
                if (v < nv) r.z = ss.road_z, r.w = ss.road_w;
                blk[v] = r;
            }
            d.rv = blk;
            d.road_np = ss.road_np;
        }
    }
    const int lane = (int)threadIdx.x, n = (int)d.n;          // n: the scene's lanes (1 .. WIDE_MAX)
    const int64_t row0 = (int64_t)set * c.R;
    if (lane < G) {
        g_pc[lane] = rec[lane].pc;
        g_hfov[lane] = rec[lane].p.hfov;
        g_vref[lane] = rec[lane].p.v_max_riding[1];
    }
    if (lane < WIDE_MAX) g_of[lane] = 0;                      // (seat below: the same thread's store to the same cell, program order)
    __syncthreads();                                          // the groups' constants are staged
    SceneLaneHook<MODEL, true> hook(c, row0);
    hook.n_groups = G, hook.rec = rec;
    hook.l_pc = g_pc, hook.l_hfov = g_hfov, hook.l_vref = g_vref, hook.l_grp = g_of, hook.w_grp = g_of;
    if (lane < n) {
        const int r = c.lane_first[c.lane_off[scn] + lane];
        if (r >= 0) hook.seat(d, lane, r);
    }
    wide_tick_body<MODEL>(d, c.len[scn], srv, hook);
    // riders that are never present are in no chain: their sums are (0, 0)
    for (int r = c.roff[scn] + lane; r < c.roff[scn + 1]; r += (int)blockDim.x)
        if (c.win_enter[r] >= c.win_exit[r]) c.sums[row0 + r] = make_double2(0.0, 0.0);
    if (lane < n) hook.flush();
}

int launch_scene_eval(int model, const Dev *table, const SceneSet *sets, const SceneDev &c, hipStream_t st, const SceneWideDev *w) {
    int launched = 0;
    for_vehicle_class(model, [&](auto m) {
        constexpr int MODEL = decltype(m)::value;
        if (w != nullptr) {
            // the narrow scenes first, scene_lanes_kernel on their compacted record, then the wide ones: the same stream, so in this order
            SceneDev cn = c;
            cn.n_scn = w->n_narrow, cn.len = w->len_n, cn.roff = w->roff_n, cn.lane_off = w->lane_off_n;
            const int count_n = c.n_sets * w->n_narrow, count_w = c.n_sets * w->n_wide;
            const bool lane_groups = c.group != nullptr;      // (csf_scene_calib_lane_groups: both launches take the grouped kernel)
            if (count_n > 0) {
                if (lane_groups) hipLaunchKernelGGL((scene_lanes_groups_kernel<MODEL>), dim3((unsigned)count_n), dim3(WAVE), c.road_lds, st, table, sets, cn);
                else hipLaunchKernelGGL((scene_lanes_kernel<MODEL>), dim3((unsigned)count_n), dim3(WAVE), c.road_lds, st, table, sets, cn);
                launched++;
            }
            if (count_w > 0) {
                if (lane_groups)
                    hipLaunchKernelGGL((scene_wide_groups_kernel<MODEL>), dim3((unsigned)count_w), dim3(WIDE_MAX), c.road_lds, st, w->table_w, sets, c,
                                       w->scn_w, w->n_wide);
                else
                    hipLaunchKernelGGL((scene_wide_kernel<MODEL>), dim3((unsigned)count_w), dim3(WIDE_MAX), c.road_lds, st, w->table_w, sets, c,
                                       w->scn_w, w->n_wide);
                launched++;
            }
            return;
        }
        const int count = c.n_sets * c.n_scn;
        if (count <= 0) return;
        const bool win = c.win_enter != nullptr && c.win_exit != nullptr;
        const bool lanes = c.lane_off != nullptr;
        const bool groups = c.group != nullptr && !lanes;     // (csf_scene_calib_groups: one slot per rider)
        const bool lane_groups = c.group != nullptr && lanes; // (csf_scene_calib_lane_groups: the group goes with the rider a lane carries)
        const dim3 grid((unsigned)count), block(WAVE);
        if (groups && win) hipLaunchKernelGGL((scene_groups_kernel<MODEL, true>), grid, block, c.road_lds, st, table, sets, c);
        else if (groups) hipLaunchKernelGGL((scene_groups_kernel<MODEL, false>), grid, block, c.road_lds, st, table, sets, c);
        else if (lane_groups) hipLaunchKernelGGL((scene_lanes_groups_kernel<MODEL>), grid, block, c.road_lds, st, table, sets, c);
        else if (lanes) hipLaunchKernelGGL((scene_lanes_kernel<MODEL>), grid, block, c.road_lds, st, table, sets, c);
        else if (win) hipLaunchKernelGGL((scene_eval_kernel<MODEL, true>), grid, block, c.road_lds, st, table, sets, c);
        else hipLaunchKernelGGL((scene_eval_kernel<MODEL, false>), grid, block, c.road_lds, st, table, sets, c);
        launched = 1;
    });
    return launched;
}

}  // namespace csf
