// csf_small_classes.hip - the one-wave and the batched tick of a handful of road users of SEVERAL PARAMETER SETS AND VEHICLE CLASSES, the
// UncontrolledVehicle's among them (csf_small_classes).  A translation unit of its own, as csf_scene_mixed.hip is: the
// kernels hold agent_body<M, HET = true, FUSED = true> of all seven classes, and no instance of csf_agent.hip or csf_scene.hip is touched.
//
// small_tick_body<SMALL_MIXED> (csf_small_body.inc) is fed from the stepping engine's own tables - Dev::ptab / pctab / pbtab / cls,
// model_mask, script / sbeg / slen - where scene_mixed_kernel feeds it from a calibration data set:
//   pair term        the constants are staged per ROAD USER, not per set: lane j < n copies the row of ITS set - pctab[cls[j]], hfov,
//                    v_max_riding[1], model - into LDS cells indexed by lane, so 32 riders may own 32 sets.  The rounding bands of the
//                    tick (set_fov_band) live in the launch's Dev::pc alone - the rows of pctab carry none - and go into every cell.
//   per-agent tick   one pass per vehicle CLASS present (ClassesHook::BY_CLASS; the loop is over the bits of Dev::model_mask), and
//                    agent_body<M, true, true> picks the lane's own row through agent_params<true> as the general path's launches do.
#include "csf_agent_dev.h"
#include "csf_field.h"

namespace csf {

#include "csf_small_body.inc"

// what small_tick_body asks of a GROUPS / SMALL_MIXED hook, answered from cells indexed by the road user (LDS)
struct ClassesHook {
    static constexpr bool MASKED = false;
    static constexpr bool SHARED = false;
    static constexpr bool GROUPS = true;
    static constexpr bool BY_CLASS = true;    // the per-agent tick: a pass per class of Dev::model_mask on the engine's tables
    const PairConsts *l_pc;
    const double *l_hfov, *l_vref;
    const uint8_t *l_model;
    int model;                                // the class of this lane's road user (a lane without one: the TwoD)
    __device__ __forceinline__ const PairConsts *consts(int j) const { return l_pc + j; }
    __device__ __forceinline__ double hfov(int j) const { return l_hfov[j]; }
    __device__ __forceinline__ double v_ref(int lane) const { return l_vref[lane]; }
    __device__ __forceinline__ int own_model() const { return model; }
    __device__ __forceinline__ int src_model(int j) const { return l_model[j]; }
    __device__ __forceinline__ void operator()(const Dev &, int, int, int) {}
};

// The cells of the launch: lane j < n copies the row of its road user's set, then the wave's own stores are made visible to all of
// its lanes (as sx, sy of the body: release fence, wave barrier).  The sets do not change during a launch.
struct ClassCells {
    PairConsts pc[SMALL_MAX];
    double hfov[SMALL_MAX], vref[SMALL_MAX];
    uint8_t model[SMALL_MAX];
};

__device__ __forceinline__ ClassesHook stage_classes(const Dev &d, ClassCells &cells) {
    const int lane = (int)threadIdx.x;
    const int n = (int)d.n < SMALL_MAX ? (int)d.n : SMALL_MAX;     // (the host admits no more; it indexes LDS)
    int model = CSF_TWOD;
    if (lane < n) {
        int c = d.cls[lane];
        c = c < d.n_classes ? c : 0;                               // (a row the host has checked, clamped all the same: it indexes the tables)
        const csf_params *const p = d.ptab + c;
        PairConsts k = d.pctab[c];
        const PairConsts &b = d.pc;                                // the bands of this tick's fp32 decisions
        k.fovA = b.fovA, k.fovB = b.fovB, k.sideA = b.sideA, k.sideB = b.sideB;
        k.fovT0 = b.fovT0, k.fovT1 = b.fovT1, k.clsk = b.clsk;
        k.fovP1 = b.fovP1, k.fovP2 = b.fovP2, k.sideP0 = b.sideP0, k.sideP1 = b.sideP1;
        model = p->model;
        cells.pc[lane] = k;
        cells.hfov[lane] = p->hfov;
        cells.vref[lane] = p->v_max_riding[1];
        cells.model[lane] = (uint8_t)model;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return ClassesHook{cells.pc, cells.hfov, cells.vref, cells.model, model};
}

// One scene, its Dev in the kernarg segment, all ticks of the call in one launch: the twin of small_tick_kernel.
__global__ __launch_bounds__(64) void small_classes_kernel(const Dev d, const int n_ticks) {
    const uint32_t ka_lines = kernarg_touch<(int)sizeof(Dev) + 4>();
    __shared__ float4 srv[SMALL_ROAD_MAX];
    __shared__ ClassCells cells;
    ClassesHook hook = stage_classes(d, cells);
    small_tick_body<SMALL_MIXED>(d, n_ticks, d.snap, srv, ka_lines, d.tick, hook);
}

// Many independent scenes in one launch, whatever their classes (csf_step_batch): workgroup b ticks the scene of table[b].  The twin of
// small_batch_kernel - the record copied into the kernel, the road in dynamic LDS, tick0 from Dev::rec_tick, the read-back packed behind
// the last tick where `pack` says so.
__global__ __launch_bounds__(64) void small_classes_batch_kernel(const Dev *__restrict__ table, const int count, const int n_ticks, const int pack) {
    extern __shared__ float4 srv_dyn[];
    __shared__ ClassCells cells;
    if ((int)blockIdx.x >= count) return;
    const Dev d = table[blockIdx.x];
    const int64_t tick0 = d.rec_tick != nullptr ? *d.rec_tick : 0;
    ClassesHook hook = stage_classes(d, cells);
    small_tick_body<SMALL_MIXED>(d, n_ticks, pack ? d.snap : nullptr, srv_dyn, 0u, tick0, hook);
    if (d.rec_tick != nullptr && threadIdx.x == 0) *d.rec_tick = tick0 + n_ticks;
}

void launch_small_classes(const Dev &d, int n_ticks, hipStream_t st) {
    if (n_ticks <= 0 || d.n <= 0 || d.n > SMALL_MAX) return;
    hipLaunchKernelGGL(small_classes_kernel, dim3(1), dim3(64), 0, st, d, n_ticks);
}

void launch_small_classes_batch(const Dev *table, int count, int max_nv_pad, int n_ticks, bool pack, hipStream_t st) {
    if (n_ticks <= 0 || count <= 0) return;
    const size_t lds = (size_t)max_nv_pad * sizeof(float4);
    hipLaunchKernelGGL(small_classes_batch_kernel, dim3((unsigned)count), dim3(64), lds, st, table, count, n_ticks, pack ? 1 : 0);
}

}  // namespace csf
