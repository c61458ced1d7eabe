// csf_scene_mixed.hip - closed-loop scene calibration with SEVERAL VEHICLE CLASSES in one scene (csf_scene_calib_classes).
// A translation unit of its own: scene_mixed_kernel holds agent_body of all six classes, and in csf_scene.hip those further callers changed
// what the compiler inlined into every other kernel of that file - here no existing instance is touched.
#include <type_traits>

#include "csf_agent_dev.h"
#include "csf_field.h"
#include "csf_scene.h"

namespace csf {

#include "csf_small_body.inc"
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

int launch_scene_mixed(const Dev *table, const SceneSet *sets, const SceneDev &c, int ns, hipStream_t st) {
    const int count = c.n_sets * c.n_scn;
    if (count <= 0 || c.group == nullptr || c.lane_off != nullptr) return 0;
    const dim3 grid((unsigned)count), block(WAVE);
    if (c.win_enter != nullptr && c.win_exit != nullptr) hipLaunchKernelGGL((scene_mixed_kernel<true>), grid, block, c.road_lds, st, table, sets, c, ns);
    else hipLaunchKernelGGL((scene_mixed_kernel<false>), grid, block, c.road_lds, st, table, sets, c, ns);
    return 1;
}

}  // namespace csf
