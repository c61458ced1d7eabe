// csf_agent.hip — fused per-agent tick (fp64, one lane per agent, SoA state => coalesced).
//
// Replaces, per tick and per agent:
//   PH_DEST       vehicle.calcDestinationForce: destination queue (vehicle.py:545-594), navigation state
//                 machine (:354-457), straight-line force (:1150-1194, 2078-2108) or spline path planner
//                 (:1416-1558; scipy splprep/splev restated as a closed 4..6-point cubic B-spline);
//   PH_COMBINE    column-sum tail of calc_forces: limitMagnitude clamp to |F_dest|, + F_dest, + road
//                 edges, store vehicle.force (intersection.py:841-862; utils.py:56-86);
//   PH_INTEGRATE  vehicle.step: controller + kinematics (vehicle.py:1218-1289, 1386-1414, 1810-1950;
//                 dynamics.py:996-1079), ring-buffer bookkeeping, and the refreshed (x, y, psi) snapshot
//                 (intersection.py:660-677) written as the fp32 source record of the next tick.
// The O(N) work is done in fp64 so that the only fp32 rounding in a tick is the pair sum.
#include <algorithm>

#include "csf_agent_dev.h"
#include "csf_field.h"

namespace csf {

template <int MODEL, bool HET = false>
__global__ __launch_bounds__(256) void agent_kernel(const Dev d, const int phases) {
    const uint32_t ka_lines = kernarg_touch<(int)sizeof(Dev) + 4>();   // (csf_dev.h)
    const int64_t a = d.lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // CSF_TRACE_AGENT (measurement aid, tools/agent_timeline.py): where does a wave's time go?  Every stamp waits for what
    // was issued before it, so the traced kernel is a little slower than the product's.
    uint64_t *const tr = d.atrace ? d.atrace + 8 * ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) : nullptr;
    if (tr != nullptr && (threadIdx.x & 63) == 0) tr[0] = wall_clock64();
    agent_body<MODEL, HET, false>(d, phases, a, tr, ka_lines, 0.0, 0.0);
}

// The per-agent tick BESIDE the pair launch that feeds it (csf_dev.h: part4; engine/tick.inc: enqueue_chase_tick): the same
// code with the sums waited for between the destination-force phase and the rest (agent_body<.., MID = 3>).
template <int MODEL>
// (`phases` is an argument, always all three: with a constant the compiler contracts the fp64 chains of some rider classes differently, and the
// two paths must agree to the last bit)
__global__ __launch_bounds__(256) void agent_chase_kernel(const Dev d, const int phases) {
    const uint32_t ka_lines = kernarg_touch<(int)sizeof(Dev) + 4>();
    const int64_t a = d.lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t *const tr = d.atrace ? d.atrace + 8 * ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) : nullptr;
    if (tr != nullptr && (threadIdx.x & 63) == 0) tr[0] = wall_clock64();
    unsigned long long *const ck = d.chase_clock ? d.chase_clock + 8 * d.chase_slot : nullptr;
    if (ck != nullptr && (threadIdx.x & 63) == 0) atomicMin(ck + 4, (unsigned long long)wall_clock64());
    agent_body<MODEL, false, false, 3>(d, phases, a, tr, ka_lines, 0.0, 0.0);
    if (ck != nullptr) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if ((threadIdx.x & 63) == 0) atomicMax(ck + 6, (unsigned long long)wall_clock64());
    }
}

// One wave that holds the per-agent launch behind it (same stream) back until `want` pair workgroups are through: launched at once the
// 256 per-agent waves would sit on their registers for the whole pair launch and cost it a workgroup per CU.
__global__ __launch_bounds__(64) void chase_gate_kernel(const unsigned *through, unsigned want, unsigned *gave_up, unsigned *gave_up_host, unsigned long long *ck) {
    if (threadIdx.x != 0) return;
    if (ck != nullptr) ck[2] = wall_clock64();
    unsigned spins = 0;
    while ((int)(__hip_atomic_load(through, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - want) < 0) {
        if (++spins > CHASE_SPIN_LIMIT) {
            atomicAdd(gave_up, 1u);
            if (gave_up_host != nullptr) __hip_atomic_store(gave_up_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            break;
        }
        __builtin_amdgcn_s_sleep(32);
    }
    if (ck != nullptr) ck[3] = wall_clock64();
}

__global__ void chase_sync_kernel(const Dev d, float4 *rec_o, float4 *recg_o, float4 *recs_o, float2 *rec2_o, double *cur, int64_t nrecg,
                                  unsigned *through);

// (a hardware queue gets its scratch memory when a kernel that needs some is first dispatched on it - the per-agent kernels spill ~200 bytes
// per lane: this one asks for as much, on the stream that has not run them yet)
__global__ __launch_bounds__(64) void chase_scratch_warm_kernel(unsigned *out, int k) {
    volatile unsigned buf[96];
    for (int i = 0; i < 96; i++) buf[i] = (unsigned)(i * k) + threadIdx.x;
    unsigned acc = 0;
    for (int i = 0; i < 96; i++) acc += buf[(i * 7 + k) % 96];
    if (acc == 0xFFFFFFFFu) out[63] = acc;     // (never, for the k it is called with: nothing is written)
}

void launch_chase_scratch_warm(unsigned *out, hipStream_t st) {
    hipLaunchKernelGGL(chase_scratch_warm_kernel, dim3(256), dim3(64), 0, st, out, 3);
}

// code objects are loaded when a kernel is first asked for: do that where the host waits anyway, not in the first side-by-side tick
void preload_chase_kernels() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, (const void *)chase_gate_kernel);
    (void)hipFuncGetAttributes(&a, (const void *)chase_sync_kernel);
    (void)hipFuncGetAttributes(&a, (const void *)agent_chase_kernel<CSF_TWOD>);
    (void)hipFuncGetAttributes(&a, (const void *)agent_chase_kernel<CSF_INVPEND>);
    (void)hipFuncGetAttributes(&a, (const void *)agent_chase_kernel<CSF_PLANARPOINT>);
    (void)hipGetLastError();
}

bool launch_agent_chase(const Dev &d, hipStream_t st, hipEvent_t t0, hipEvent_t t1) {
    if (d.hi <= d.lo || d.part4 == nullptr || d.n_classes > 1) return false;
    const dim3 g((unsigned)((d.hi - d.lo + 63) / 64)), b(64);
    switch (d.p.model) {
    case CSF_TWOD: break;
    case CSF_INVPEND: break;
    case CSF_PLANARPOINT: break;
    default: return false;
    }
    const int ph = PH_DEST | PH_COMBINE | PH_INTEGRATE;
    hipLaunchKernelGGL(chase_gate_kernel, dim3(1), dim3(64), 0, st, d.chase_misc, d.chase_gate, d.chase_misc + 1, d.chase_err,
                       d.chase_clock ? d.chase_clock + 8 * d.chase_slot : nullptr);
    switch (d.p.model) {
    case CSF_TWOD: hipExtLaunchKernelGGL((agent_chase_kernel<CSF_TWOD>), g, b, 0, st, t0, t1, 0, d, ph); break;
    case CSF_INVPEND: hipExtLaunchKernelGGL((agent_chase_kernel<CSF_INVPEND>), g, b, 0, st, t0, t1, 0, d, ph); break;
    default: hipExtLaunchKernelGGL((agent_chase_kernel<CSF_PLANARPOINT>), g, b, 0, st, t0, t1, 0, d, ph); break;
    }
    return true;
}

#include "csf_small_body.inc"   // the one-wave tick (small_tick_body), shared with csf_scene.hip

template <int MODEL>
__global__ __launch_bounds__(64) void small_tick_kernel(const Dev d, const int n_ticks) {
    const uint32_t ka_lines = kernarg_touch<(int)sizeof(Dev) + 4>();
    __shared__ float4 srv[SMALL_ROAD_MAX];
    NoTickHook none;
    small_tick_body<MODEL>(d, n_ticks, d.snap, srv, ka_lines, d.tick, none);
}

// Many independent scenes of one vehicle class in one launch (csf_step_batch): workgroup b ticks the scene of table[b], all
// n_ticks of the call.  The road is staged in dynamic LDS sized by the launch's largest nv_pad (none without roads), so that
// registers and not an unused road buffer set how many of these waves a CU holds.  `pack`: write every member's read-back into
// its Dev::snap behind the last tick (a per-call choice; the table changes only when a member's Dev does).
template <int MODEL>
__global__ __launch_bounds__(64) void small_batch_kernel(const Dev *__restrict__ table, const int count, const int n_ticks, const int pack) {
    extern __shared__ float4 srv_dyn[];
    if ((int)blockIdx.x >= count) return;
    // (the record copied into the kernel, as the single-scene kernel has it in its kernarg segment: read through a reference to
    // global memory, the compiler contracted a few fp64 chains of the PlanarPoint, PlanarBicycle and InvPendulum riders
    // differently - 1 ulp, and the batch is no longer what csf_step on each member gives)
    const Dev d = table[blockIdx.x];
    // (the table holds Dev::tick = 0: a recording member's count is a word of device memory, moved on here behind the last tick)
    const int64_t tick0 = d.rec_tick != nullptr ? *d.rec_tick : 0;
    NoTickHook none;
    small_tick_body<MODEL>(d, n_ticks, pack ? d.snap : nullptr, srv_dyn, 0u, tick0, none);
    if (d.rec_tick != nullptr && threadIdx.x == 0) *d.rec_tick = tick0 + n_ticks;
}

void launch_small_batch(int model, const Dev *table, int count, int max_nv_pad, int n_ticks, bool pack, hipStream_t st) {
    if (n_ticks <= 0 || count <= 0) return;
    const size_t lds = (size_t)max_nv_pad * sizeof(float4);
    const int pk = pack ? 1 : 0;
    for_vehicle_class(model, [&](auto m) {
        hipLaunchKernelGGL((small_batch_kernel<decltype(m)::value>), dim3((unsigned)count), dim3(64), lds, st, table, count, n_ticks, pk);
    });
}

void launch_small_tick(const Dev &d, int n_ticks, hipStream_t st, hipEvent_t t0, hipEvent_t t1) {
    if (n_ticks <= 0 || d.n <= 0) return;
    for_vehicle_class(d.p.model, [&](auto m) {
        hipExtLaunchKernelGGL((small_tick_kernel<decltype(m)::value>), dim3(1), dim3(64), 0, st, t0, t1, 0, d, n_ticks);
    });
}

// (re)build the fp32 records, the short position ring and the model side-state from the fp64 state:
// Vehicle.__init__ (vehicle.py:154-160, 1728-1736; dynamics.py:828) and update_road_user_positions (:660-677)
__global__ void records_kernel(const Dev d) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= d.n_pad) return;
    if (a >= d.n || !d.alive[a]) {  // sentinel: far away, contributes exactly 0 (exp2 underflow), never NaN
        d.rec[a] = make_float4(1e15f, 1e15f, 1.0f, 0.0f);
        if (a < d.cap) d.recg[a] = d.rec[a];
        if (d.has_bike) d.rec2[a] = make_float2(0.0f, 1.0f);
        if (d.xbuf != nullptr) {
            d.xbuf[2 * a] = d.rec[a];
            d.xbuf[2 * a + 1] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
        }
        return;
    }
    write_record(d, d.ptab[d.cls[a]], a, d.rorg[a], d.s[a], d.s[d.cap + a], d.s[2 * d.cap + a], d.s[3 * d.cap + a]);
}

void launch_agent(const Dev &d, int phases, hipStream_t st, hipEvent_t t0, hipEvent_t t1) {
    if (d.hi <= d.lo) return;
    constexpr int bs = 64;   // one-wave workgroups: 256 waves on 256 CUs measured 0.6 us faster than 64 workgroups of 4
    dim3 g((unsigned)((d.hi - d.lo + bs - 1) / bs)), b(bs);
#define CSF_AGENT(MODEL)                                                                                             \
    if (d.n_classes > 1) hipExtLaunchKernelGGL((agent_kernel<MODEL, true>), g, b, 0, st, t0, t1, 0, d, phases);           \
    else hipExtLaunchKernelGGL((agent_kernel<MODEL, false>), g, b, 0, st, t0, t1, 0, d, phases)
    // every vehicle class of the population in turn (one, unless csf_set_param_classes installed sets of several classes;
    // the launches touch disjoint agents).  The time stamps bracket the first launch.
    for (int m = 0; m < 7; m++) {
        if (!(d.model_mask >> m & 1)) continue;
        switch (m) {
        case CSF_BALANCINGRIDER: CSF_AGENT(CSF_BALANCINGRIDER); break;
        case CSF_UNCONTROLLED: CSF_AGENT(CSF_UNCONTROLLED); break;
        case CSF_BICYCLE: CSF_AGENT(CSF_BICYCLE); break;
        case CSF_TWOD: CSF_AGENT(CSF_TWOD); break;
        case CSF_INVPEND: CSF_AGENT(CSF_INVPEND); break;
        case CSF_PLANARBIKE: CSF_AGENT(CSF_PLANARBIKE); break;
        default: CSF_AGENT(CSF_PLANARPOINT); break;
        }
        t0 = t1 = nullptr;
    }
#undef CSF_AGENT
}

// Vehicle.updateDestination (vehicle.py:545-594) and Vehicle.updateNavState(stop) (vehicle.py:354-457) on their own, for
// the listed agents: the host mirror's methods of the same name run them here (what & 1: queue pointer, what & 2: navigation
// state machine, desired speed and distance to vd_out / ddest_out).  stop[k] >= 0 overrides the stop flag of the current
// destination for this call, as the reference's explicit `stop` argument does.
__global__ void nav_kat_kernel(const Dev d, const int32_t *idx, int64_t m, int what, const int32_t *stop, double *vd_out,
                               double *ddest_out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const int64_t a = idx[k], cap = d.cap;
    Agent g;
    g.a = a;
    g.x = d.s[a];
    g.y = d.s[cap + a];
    g.v = d.s[3 * cap + a];
    g.vdes = d.vdes[a];
    g.qb = d.qbeg[a];
    g.K = d.qlen[a];
    g.ptr = d.ptr[a];
    g.zn = d.znav[a] & 3;
    g.zv0 = d.znp[a];
    g.zd0 = d.znp[cap + a];
    g.zd1 = d.znp[2 * cap + a];
    g.st = d.status[a];
    agent_params<true>(d, a, g);                             // (the class table is there for one parameter set as well)
    load_rows(d, g);
    if (what & 1) {
        update_destination(d, g);
        d.ptr[a] = g.ptr;
    }
    if (what & 2) {
        const bool forced = stop != nullptr && stop[k] >= 0;
        if (forced) g.rs[0] = stop[k] ? 1.0 : 0.0;           // (the row in registers; the slab keeps its flag)
        double ddest;
        const double vd = update_nav(d, g, ddest);
        d.znav[a] = (uint8_t)g.zn;
        d.znp[a] = g.zv0;
        d.znp[cap + a] = g.zd0;
        d.znp[2 * cap + a] = g.zd1;
        d.status[a] = g.st;
        vd_out[k] = vd;
        ddest_out[k] = ddest;
    }
}

void launch_nav_kat(const Dev &d, const int32_t *idx, int64_t m, int what, const int32_t *stop, double *vd_out,
                    double *ddest_out, hipStream_t st) {
    if (m <= 0) return;
    hipLaunchKernelGGL(nav_kat_kernel, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, st, d, idx, m, what, stop, vd_out, ddest_out);
}

// csf_get_tick: everything the host mirror refreshes after a tick, packed for one transfer
__global__ void snapshot_kernel(const Dev d, double *out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // road user i of the population order
    const int64_t n = d.n_live;
    if (i >= n) return;
    const int64_t a = d.order ? d.order[i] : i;
    const int ns = d.ns;
    for (int c = 0; c < ns; c++) out[i * ns + c] = d.s[(int64_t)c * d.cap + a];
    double *F = out + n * ns;
    F[i] = d.F[a];
    F[n + i] = d.F[d.cap + a];
    int32_t *ptr = (int32_t *)(F + 2 * n);
    ptr[i] = d.ptr[a];
    uint8_t *zn = (uint8_t *)(ptr + n);
    const int z = d.znav[a] & 3;
    zn[3 * i + 0] = z == 0;
    zn[3 * i + 1] = z == 1;
    zn[3 * i + 2] = z == 2;
}

void launch_snapshot(const Dev &d, double *out, hipStream_t st) {
    if (d.n_live <= 0) return;
    hipLaunchKernelGGL(snapshot_kernel, dim3((unsigned)((d.n_live + 255) / 256)), dim3(256), 0, st, d, out);
}

// The rings of csf_record / csf_enable_history -> one packed buffer: workgroup row y serves member y, its threads stride over
// the member's samples [count][n][ns] and [count][n][2] in pairs of doubles (16-byte loads and stores; a ring slot is a whole
// number of pairs unless n * ns is odd, then one double at a time).  Sample k of the output is ring slot (first + k) % cap.
__device__ __forceinline__ void gather_ring(const double *__restrict__ ring, double *__restrict__ out, const int64_t row, const int cap,
                                            const int first, const int count, const int64_t i0, const int64_t step) {
    if ((row & 1) == 0) {
        const int64_t rp = row >> 1, total = rp * count;
        for (int64_t j = i0; j < total; j += step) {
            const int64_t k = j / rp, r = j - k * rp;
            const int64_t slot = (first + k) % cap;
            ((double2 *)out)[j] = ((const double2 *)ring)[slot * rp + r];
        }
    } else {
        const int64_t total = row * count;
        for (int64_t j = i0; j < total; j += step) {
            const int64_t k = j / row, r = j - k * row;
            const int64_t slot = (first + k) % cap;
            out[j] = ring[slot * row + r];
        }
    }
}

__global__ __launch_bounds__(256) void record_gather_kernel(const RecDesc *__restrict__ desc, const int members, double *__restrict__ out) {
    if ((int)blockIdx.y >= members) return;
    const RecDesc m = desc[blockIdx.y];
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (m.s != nullptr) gather_ring(m.s, out + m.s_off, (int64_t)m.n * m.ns, m.cap, m.first, m.count, i0, step);
    if (m.F != nullptr) gather_ring(m.F, out + m.F_off, (int64_t)m.n * 2, m.cap, m.first, m.count, i0, step);
}

void launch_record_gather(const RecDesc *desc, int members, int64_t most_doubles, double *out, hipStream_t st) {
    if (members <= 0 || most_doubles <= 0) return;
    // (columns of workgroups: enough for the largest member at 4 pairs per thread, at most 256 - the threads stride over the rest)
    const int64_t want = (most_doubles / 2 + 1023) / 1024;
    const unsigned gx = (unsigned)std::min<int64_t>(std::max<int64_t>(want, 1), 256);
    hipLaunchKernelGGL(record_gather_kernel, dim3(gx, (unsigned)members), dim3(256), 0, st, desc, members, out);
}

void launch_records(const Dev &d, hipStream_t st) {
    if (d.n_pad <= 0) return;
    hipLaunchKernelGGL(records_kernel, dim3((unsigned)((d.n_pad + 255) / 256)), dim3(256), 0, st, d);
}

// The other halves of the double buffers <- this tick's records and fp64 positions, and the gate's counter cleared: what five
// copy / fill calls did when the side-by-side tick was entered (once per re-binning: a launch and its gap each), in one launch.
__global__ void chase_sync_kernel(const Dev d, float4 *rec_o, float4 *recg_o, float4 *recs_o, float2 *rec2_o, double *cur, int64_t nrecg,
                                  unsigned *through) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < d.n_pad) {
        rec_o[i] = d.rec[i];
        if (i < nrecg) recg_o[i] = d.recg[i];
        if (d.recs_valid) recs_o[i] = d.recs[i];
        if (d.has_bike) rec2_o[i] = d.rec2[i];
    }
    if (i < 3 * d.cap) cur[i] = d.s[i];
    if (through != nullptr && i == 0) *through = 0u;
}

// csf_step_batch: the same for every mid-size member of the table whose tick record asks (MID_DUE_SYNC), grid y = table slot.  The
// records of such a member are not binned (no copy in binned order to keep), and nobody waits at a gate.
__global__ void mid_sync_batch_kernel(const Dev *__restrict__ table, const MidTick *__restrict__ ticks) {
    const MidTick t = ticks[blockIdx.y];
    if (!(t.flags & MID_DUE_SYNC)) return;
    Dev d = table[blockIdx.y];
    mid_compose(d, t);                                            // (rec ...: this tick's halves, rec_w ...: the others)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < d.n_pad) {
        d.rec_w[i] = d.rec[i];
        if (i < t.nrecg) d.recg_w[i] = d.recg[i];
        if (d.has_bike) d.rec2_w[i] = d.rec2[i];
    }
    if (i < 3 * d.cap) const_cast<double *>(d.src64)[i] = d.s[i];
}

void launch_mid_batch_sync(const Dev *table, const MidTick *ticks, int slots, int64_t max_elems, hipStream_t st) {
    if (slots <= 0 || max_elems <= 0) return;
    hipLaunchKernelGGL(mid_sync_batch_kernel, dim3((unsigned)((max_elems + 255) / 256), (unsigned)slots), dim3(256), 0, st, table, ticks);
}

void launch_chase_sync(const Dev &d, float4 *rec_o, float4 *recg_o, float4 *recs_o, float2 *rec2_o, double *cur, int64_t nrecg, unsigned *through,
                       hipStream_t st) {
    const int64_t n = std::max<int64_t>(d.n_pad, 3 * d.cap);
    if (n <= 0) return;
    hipLaunchKernelGGL(chase_sync_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d, rec_o, recg_o, recs_o, rec2_o, cur, nrecg, through);
}

// ---- population changes on the device ---------------------------------------------------------------------------------
// One launch applies a batch of changes that the engine collected since the last device call (csf_engine.hip:
// flush_pending).  The items are independent of each other - the host has already dropped a retirement whose slot is
// spawned into again, folded a new queue of a new road user into its spawn record, and kept only the last queue of a
// slot - so they run side by side: thread k takes one retirement, one spawn, one queue, or one queue row.  The records
// are read straight from pinned host memory.
//
// spawn: Vehicle.__init__ (vehicle.py:64-204, 1728-1736; dynamics.py:828) for a new road user placed into a free slot:
//   what csf_add_agents writes into the host mirror on the upload path, plus the fp32 record.  The slot keeps the
//   position of the binned order it had (pos[]) - the host picks slots whose place is in the tail of sentinels behind
//   the sorted batches (csf_engine.hip: rebin), so until the next re-binning the arrivals share a few tail batches.
// retire: remove_road_user (intersection.py:576-634): the slot is no longer integrated and its record becomes the
//   sentinel that contributes exactly nothing as a source.
// requeue: Vehicle.setDestinations (vehicle.py:606-647): the queue of a slot now lives at another place of the slab.
// The batch header travels as a kernel argument (one round trip over PCIe less than reading it from the pinned buffer).
// [b0, b1): the batches of the binned order that receive arrivals in this launch (the host knows the places of the
// sentinel tail it hands out, csf_engine.hip: rebin): the workgroup that finishes last recomputes their bounding circles,
// which saves the bounds_kernel launch in front of the next pair launch.
__global__ __launch_bounds__(256) void patch_kernel(const Dev d, const PatchHeader h, const char *base, unsigned *ticket,
                                                    int b0, int b1) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t cap = d.cap;
    if (k < h.n_retire) {
        const int64_t a = ((const int32_t *)(base + h.off_retire))[k];
        d.alive[a] = 0;
        d.cls[a] = 0;                                              // (its sentinel record is looked up in set 0 from now on)
        const float4 q = make_float4(1e15f, 1e15f, 1.0f, 0.0f);
        d.rec[a] = q;
        d.recg[a] = q;
        if (d.recs_valid) {
            d.recs[d.pos[a]] = q;
            d.recb[d.pos[a]] = q;
        }
        if (d.has_bike) {
            d.rec2[a] = make_float2(0.0f, 1.0f);
            if (d.recs_valid) d.recs2[d.pos[a]] = make_float2(0.0f, 1.0f);
        }
    } else if ((k -= h.n_retire) < h.n_spawn) {
        const SpawnRec r = ((const SpawnRec *)(base + h.off_spawn))[k];
        const int64_t a = r.slot;
        const csf_params &p = d.ptab[r.cls];
        d.cls[a] = (uint8_t)r.cls;
        double s[STATE_ROWS];
        for (int c = 0; c < STATE_ROWS; c++) s[c] = c < d.ns ? r.s[c] : 0.0;
        s[2] = limit_angle(s[2]);                                  // vehicle.py:154-155
        for (int c = 0; c < STATE_ROWS; c++) d.s[c * cap + a] = s[c];
        d.vdes[a] = r.vdes;
        d.qbeg[a] = r.qbeg;
        d.qlen[a] = r.qlen;
        d.ptr[a] = 0;
        d.znav[a] = 0;                                             // vehicle.py:188
        for (int c = 0; c < 3; c++) d.znp[c * cap + a] = 0.0;
        d.ti[a] = 0;                                               // vehicle.py:146
        d.hx[a] = s[0];                                            // traj[:, 0] = s (vehicle.py:159-160)
        d.hy[a] = s[1];
        const double delta = d.ns > 4 ? s[4] : 0.0, theta = d.ns > 5 ? s[5] : 0.0;
        d.lti[0 * cap + a] = delta;                                // vehicle.py:1728
        d.lti[1 * cap + a] = 0.0;
        d.lti[2 * cap + a] = theta;
        d.lti[3 * cap + a] = 0.0;
        d.lti[4 * cap + a] = s[2];
        d.zrid[a] = s[3] < p.v_max_walk ? 0 : 1;                   // vehicle.py:1732-1736
        d.dgood[a] = (-p.delta_max_walk < delta && p.delta_max_walk > delta) ? 1 : 0;
        d.ppsi[a] = s[2];                                          // dynamics.py:828, 987-993
        if (p.model == CSF_BALANCINGRIDER) {                       // dynamics.py:306-307, 350-371: (roll, steer, rates, yaw) mirrored
            d.lti[0 * cap + a] = s[5];
            d.lti[1 * cap + a] = -s[4];
            d.lti[2 * cap + a] = s[7];
            d.lti[3 * cap + a] = -s[6];
            d.lti[4 * cap + a] = -s[2];
            d.ppsi[a] = s[3];                                      // the speed its first gains belong to
        }
        d.slen[a] = 0;                                             // (no prescribed trajectory until csf_set_script gives one)
        for (int c = 0; c < 6; c++) d.F[c * cap + a] = 0.0;
        d.status[a] = 0;
        d.alive[a] = 1;
        // its own origin: where it starts, rounded to 1/4 m; the slot keeps its place of the binned order
        const float2 o = make_float2((float)(0.25 * rint(4.0 * (s[0] - d.ox))), (float)(0.25 * rint(4.0 * (s[1] - d.oy))));
        d.rorg[a] = o;
        write_record(d, p, a, o, s[0], s[1], s[2], s[3]);
    } else if ((k -= h.n_spawn) < h.n_requeue) {
        const QueueRec r = ((const QueueRec *)(base + h.off_requeue))[k];
        d.qbeg[r.slot] = r.qbeg;
        d.qlen[r.slot] = r.qlen;
        const int32_t ptr = r.mode == 1 ? 0 : d.ptr[r.slot];       // vehicle.py:642-645: reset rewinds the pointer
        d.ptr[r.slot] = ptr < r.qlen ? ptr : r.qlen - 1;
    } else if ((k -= h.n_requeue) < 3 * h.n_rows) {
        d.q[3 * h.q_top + k] = ((const double *)(base + h.off_rows))[k];
    }
    if (b1 <= b0) return;                                          // (uniform) no circles to renew
    __shared__ bool last;
    __threadfence();                                               // this thread's records, before the ticket
    __syncthreads();
    if (threadIdx.x == 0) last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    __syncthreads();
    if (!last) return;
    __threadfence();
    for (int bb = b0 + (int)(threadIdx.x >> 6); bb < b1; bb += (int)(blockDim.x >> 6)) batch_circle(d, bb, threadIdx.x & 63, 0.0f, d.bnd);
    if (threadIdx.x == 0) *ticket = 0;                             // for the next launch
}

void launch_patch(const Dev &d, const PatchHeader &h, const void *records, unsigned *ticket, int b0, int b1, int64_t items,
                  hipStream_t st) {
    if (items > 0)
        hipLaunchKernelGGL(patch_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, d, h, (const char *)records, ticket, b0, b1);
}

}  // namespace csf
