// csf_scene_mixed.hip - closed-loop scene calibration with SEVERAL VEHICLE CLASSES in one scene (csf_scene_calib_classes).
// A translation unit of its own: scene_mixed_kernel holds agent_body of all six classes, and in csf_scene.hip those further callers changed
// what the compiler inlined into every other kernel of that file - here no existing instance is touched.
// The same on shared lanes and on wide scenes (csf_scene_calib_lane_classes): scene_lanes_mixed_kernel, scene_wide_mixed_kernel.
#include <type_traits>

#include "csf_agent_dev.h"
#include "csf_field.h"
#include "csf_scene.h"

namespace csf {

#include "csf_small_body.inc"
#include "csf_wide_body.inc"

#include "csf_scene_hook.inc"

// Several vehicle classes in one scene (csf_scene_calib_classes): scene_groups_kernel with the CLASS a property of the group.
// `sets` holds c.n_groups records per candidate set, and record g names the class of group g (the host has checked it against the loaded
// classes); `ns` is the widest state of the loaded classes - the views carry the engine's own - and the image (c.img_s, img_lti, img_ppsi)
// is the one the host rewrote per rider and class.  The kernel is scene_groups_kernel line for line around the staging of the classes
// and the wider tables (SCENE_CLASS_GROUPS_MAX): a change to one is made in the other.
template <bool WIN>
__global__ __launch_bounds__(64) void scene_mixed_kernel(const Dev *__restrict__ table, const SceneSet *__restrict__ sets, const SceneDev c, const int ns) {
    extern __shared__ float4 srv[];                           // as scene_eval_kernel
    __shared__ PairConsts g_pc[SCENE_CLASS_GROUPS_MAX];
    __shared__ double g_hfov[SCENE_CLASS_GROUPS_MAX], g_vref[SCENE_CLASS_GROUPS_MAX];
    __shared__ uint8_t g_model[SCENE_CLASS_GROUPS_MAX];
    __shared__ uint8_t g_of[SMALL_MAX];
    const int b = (int)blockIdx.x;
    if (b >= c.n_sets * c.n_scn) return;
    const int set = b / c.n_scn, scn = b - set * c.n_scn;
    const int G = c.n_groups < SCENE_CLASS_GROUPS_MAX ? c.n_groups : SCENE_CLASS_GROUPS_MAX;   // (the host refuses more; LDS holds no more)
    const SceneSet *const rec = sets + (int64_t)set * c.n_groups;
    Dev d = table[b];
    d.ns = ns;
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
    const int lane = (int)threadIdx.x, n = (int)d.n;
    const int64_t first = c.roff[scn];
    const int len = c.len[scn];
    // (an entry the host has checked, clamped all the same: it indexes LDS)
    int grp = lane < n ? (int)c.group[first + lane] : 0;
    grp = grp < G ? grp : G - 1;
    // the groups' constants and classes to LDS: lane g < G copies record g; then the wave's own stores, program order (as sx, sy)
    if (lane < G) {
        g_pc[lane] = rec[lane].pc;
        g_hfov[lane] = rec[lane].p.hfov;
        g_vref[lane] = rec[lane].p.v_max_riding[1];
        g_model[lane] = (uint8_t)rec[lane].p.model;
    }
    if (lane < SMALL_MAX) g_of[lane] = (uint8_t)grp;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < n) scene_restore(d, c, lane, first + lane, rec[grp].p.v_max_walk, rec[grp].p.delta_max_walk);
    const int64_t rider = (int64_t)set * c.R + first + lane;
    const int rcol = c.rep != nullptr && lane < n ? c.rep_index[first + lane] : -1;
    const int t_in = WIN && lane < n ? c.win_enter[first + lane] : 0, t_out = WIN && lane < n ? c.win_exit[first + lane] : 0;
    SceneHook<SMALL_MIXED, WIN, true> hook(c, rider, c.obj + (first + lane) * c.n_feat, rcol >= 0 ? c.rep + (int64_t)rcol * 4 : nullptr,
                                           c.states != nullptr && lane < n ? c.states + rider * d.ns : nullptr, t_in, t_out);
    hook.n_groups = G, hook.grp = grp, hook.rec = rec;
    hook.l_pc = g_pc, hook.l_hfov = g_hfov, hook.l_vref = g_vref, hook.l_grp = g_of;
    hook.l_model = g_model, hook.model = rec[grp].p.model;
    small_tick_body<SMALL_MIXED>(d, len, nullptr, srv, 0u, 0, hook);
    if (lane >= n) return;
    c.sums[rider] = make_double2(hook.sse, hook.sae);
    if (hook.smp != nullptr)
        while (hook.taken < c.n_samples) hook.sample(d, lane);
}

// Vehicle classes on shared lanes (csf_scene_calib_lane_classes): scene_lanes_groups_kernel with the CLASS a property of the
// group, so of the RIDER a lane carries - a lane changes its class at a takeover (SceneLaneHook<SMALL_MIXED, true>::seat).  Prologue, staging
// and `ns` are scene_mixed_kernel's, the skeleton is scene_lanes_groups_kernel's (csf_scene.hip): a change to one is made in the others.  A
// lane nobody rides yet has group 0 and that group's class, and is never present.
__global__ __launch_bounds__(64) void scene_lanes_mixed_kernel(const Dev *__restrict__ table, const SceneSet *__restrict__ sets, const SceneDev c,
                                                               const int ns) {
    extern __shared__ float4 srv[];                           // as scene_eval_kernel
    __shared__ PairConsts g_pc[SCENE_CLASS_GROUPS_MAX];
    __shared__ double g_hfov[SCENE_CLASS_GROUPS_MAX], g_vref[SCENE_CLASS_GROUPS_MAX];
    __shared__ uint8_t g_model[SCENE_CLASS_GROUPS_MAX];
    __shared__ uint8_t g_of[SMALL_MAX];                       // the group of every LANE: that of the rider it carries
    const int b = (int)blockIdx.x;
    if (b >= c.n_sets * c.n_scn) return;
    const int set = b / c.n_scn, scn = b - set * c.n_scn;
    const int G = c.n_groups < SCENE_CLASS_GROUPS_MAX ? c.n_groups : SCENE_CLASS_GROUPS_MAX;   // (the host refuses more; LDS holds no more)
    const SceneSet *const rec = sets + (int64_t)set * c.n_groups;
    Dev d = table[b];
    d.ns = ns;
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
    // the groups' constants and classes to LDS: lane g < G copies record g; every lane starts in group 0.  Then the wave's own stores,
    // program order (as sx, sy); seat below reads the class of its group from there and stores to the lane's own cell of g_of
    if (lane < G) {
        g_pc[lane] = rec[lane].pc;
        g_hfov[lane] = rec[lane].p.hfov;
        g_vref[lane] = rec[lane].p.v_max_riding[1];
        g_model[lane] = (uint8_t)rec[lane].p.model;
    }
    if (lane < SMALL_MAX) g_of[lane] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    SceneLaneHook<SMALL_MIXED, true> hook(c, row0);
    hook.n_groups = G, hook.rec = rec;
    hook.l_pc = g_pc, hook.l_hfov = g_hfov, hook.l_vref = g_vref, hook.l_grp = g_of, hook.w_grp = g_of;
    hook.l_model = g_model, hook.model = rec[0].p.model;
    if (lane < n) {
        const int r = c.lane_first[c.lane_off[scn] + lane];
        if (r >= 0) hook.seat(d, lane, r);
    }
    small_tick_body<SMALL_MIXED>(d, c.len[scn], nullptr, srv, 0u, 0, hook);
    // riders that are never present are in no chain: their sums are (0, 0)
    for (int r = c.roff[scn] + lane; r < c.roff[scn + 1]; r += WAVE)
        if (c.win_enter[r] >= c.win_exit[r]) c.sums[row0 + r] = make_double2(0.0, 0.0);
    if (lane < n) hook.flush();
}

// ... and on wide scenes: scene_wide_groups_kernel (csf_scene.hip) with the same additions.  What thread g < G stages is read by every thread
// in seat and at the head of the first tick - other waves, so a workgroup barrier stands behind the staging, reached by all 256 threads: the
// only return in front of it is the uniform one.
__global__ __launch_bounds__(256) void scene_wide_mixed_kernel(const Dev *__restrict__ table, const SceneSet *__restrict__ sets, const SceneDev c,
                                                               const int32_t *__restrict__ scn_w, const int n_wide, const int ns) {
    extern __shared__ float4 srv[];                           // as scene_eval_kernel
    __shared__ PairConsts g_pc[SCENE_CLASS_GROUPS_MAX];
    __shared__ double g_hfov[SCENE_CLASS_GROUPS_MAX], g_vref[SCENE_CLASS_GROUPS_MAX];
    __shared__ uint8_t g_model[SCENE_CLASS_GROUPS_MAX];
    __shared__ uint8_t g_of[WIDE_MAX];                        // the group of every LANE: that of the rider it carries
    const int b = (int)blockIdx.x;
    if (b >= c.n_sets * n_wide) return;                       // (the only early return: before any barrier, the same in every thread)
    const int set = b / n_wide, scn = scn_w[b - set * n_wide];
    const int G = c.n_groups < SCENE_CLASS_GROUPS_MAX ? c.n_groups : SCENE_CLASS_GROUPS_MAX;   // (the host refuses more; LDS holds no more)
    const SceneSet *const rec = sets + (int64_t)set * c.n_groups;
    Dev d = table[b];
    d.ns = ns;
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
        g_model[lane] = (uint8_t)rec[lane].p.model;
    }
    if (lane < WIDE_MAX) g_of[lane] = 0;                      // (seat below: the same thread's store to the same cell, program order)
    __syncthreads();                                          // the groups' constants and classes are staged
    SceneLaneHook<SMALL_MIXED, true> hook(c, row0);
    hook.n_groups = G, hook.rec = rec;
    hook.l_pc = g_pc, hook.l_hfov = g_hfov, hook.l_vref = g_vref, hook.l_grp = g_of, hook.w_grp = g_of;
    hook.l_model = g_model, hook.model = rec[0].p.model;
    if (lane < n) {
        const int r = c.lane_first[c.lane_off[scn] + lane];
        if (r >= 0) hook.seat(d, lane, r);
    }
    wide_tick_body<SMALL_MIXED>(d, c.len[scn], srv, hook);
    // riders that are never present are in no chain: their sums are (0, 0)
    for (int r = c.roff[scn] + lane; r < c.roff[scn + 1]; r += (int)blockDim.x)
        if (c.win_enter[r] >= c.win_exit[r]) c.sums[row0 + r] = make_double2(0.0, 0.0);
    if (lane < n) hook.flush();
}

// `w` (a wide load): the narrow scenes on their compacted record first, then the wide ones - the same stream, so in this order - as
// launch_scene_eval does it (csf_scene.hip)
int launch_scene_mixed(const Dev *table, const SceneSet *sets, const SceneDev &c, int ns, hipStream_t st, const SceneWideDev *w) {
    if (c.group == nullptr) return 0;
    if (w != nullptr) {
        int launched = 0;
        SceneDev cn = c;
        cn.n_scn = w->n_narrow, cn.len = w->len_n, cn.roff = w->roff_n, cn.lane_off = w->lane_off_n;
        const int count_n = c.n_sets * w->n_narrow, count_w = c.n_sets * w->n_wide;
        if (count_n > 0) {
            hipLaunchKernelGGL(scene_lanes_mixed_kernel, dim3((unsigned)count_n), dim3(WAVE), c.road_lds, st, table, sets, cn, ns);
            launched++;
        }
        if (count_w > 0) {
            hipLaunchKernelGGL(scene_wide_mixed_kernel, dim3((unsigned)count_w), dim3(WIDE_MAX), c.road_lds, st, w->table_w, sets, c, w->scn_w,
                               w->n_wide, ns);
            launched++;
        }
        return launched;
    }
    const int count = c.n_sets * c.n_scn;
    if (count <= 0) return 0;
    const dim3 grid((unsigned)count), block(WAVE);
    if (c.lane_off != nullptr) hipLaunchKernelGGL(scene_lanes_mixed_kernel, grid, block, c.road_lds, st, table, sets, c, ns);
    else if (c.win_enter != nullptr && c.win_exit != nullptr) hipLaunchKernelGGL((scene_mixed_kernel<true>), grid, block, c.road_lds, st, table, sets, c, ns);
    else hipLaunchKernelGGL((scene_mixed_kernel<false>), grid, block, c.road_lds, st, table, sets, c, ns);
    return 1;
}

}  // namespace csf
