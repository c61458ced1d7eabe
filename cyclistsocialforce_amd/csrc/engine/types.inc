// csf_engine.hip — host side of libcsf_hip.so: the C ABI of include/csf.h.
//
// Owns the SoA population in HBM, the HIP streams, the per-tick launch sequence and (for world > 1) the
// RCCL all-gather of the fp32 source records.  There is no CPU compute path in this library: every entry
// point that produces numbers launches the kernels of csf_pair.hip / csf_agent.hip.
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <limits>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <vector>

#include "csf_dev.h"
#include "csf_handout.h"
#include "csf_wg_order.h"
#include "csf_calib.h"
#include "csf_scene.h"

using namespace csf;

namespace {

thread_local std::string g_create_error;

// RCCL is resolved at run time so that single-GPU use does not depend on it.
struct Rccl {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Broadcast)(const void *, void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    std::string err;
    bool load() {
        if (lib) return true;
        for (const char *name : {"librccl.so.1", "librccl.so"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (lib) break;
        }
        if (!lib) {
            err = std::string("cannot load librccl: ") + dlerror();
            return false;
        }
#define SYM(field, name)                                      \
    field = (decltype(field))dlsym(lib, name);                \
    if (!field) {                                             \
        err = std::string("librccl lacks symbol ") + name;    \
        return false;                                         \
    }
        SYM(GetUniqueId, "ncclGetUniqueId")
        SYM(CommInitRank, "ncclCommInitRank")
        SYM(CommDestroy, "ncclCommDestroy")
        SYM(AllGather, "ncclAllGather")
        SYM(AllReduce, "ncclAllReduce")
        SYM(Broadcast, "ncclBroadcast")
        SYM(GroupStart, "ncclGroupStart")
        SYM(GroupEnd, "ncclGroupEnd")
        SYM(GetErrorString, "ncclGetErrorString")
#undef SYM
        return true;
    }
} g_rccl;

// CSF_DEBUG_POISON=1 (read at the first csf_create of the process): a debugging aid for loads whose safety is a property of the
// caller's allocation.  Every device buffer gets a red zone of POISON_GUARD bytes of 0xFF behind it (NaN as float or double, -1 as an
// integer: a load that runs past the end meets poison instead of a neighbour's data or a fault), the slots behind the population and
// the records no slot owns are poisoned instead of zeroed (upload_all, alloc_all) - a kernel whose RESULT depends on any of them
// shows NaN in the suite.  DESIGN.md section 3 lists the loads that are unconditional by design.
bool g_poison = false;
constexpr size_t POISON_GUARD = 1 << 16;

// Device memory that belongs to its holder: freed when the holder goes, moved but never copied.
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) release(), p = o.p, n = o.n, o.p = nullptr, o.n = 0;
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t alloc(size_t count) {
        release();
        n = count;
        if (count == 0) return hipSuccess;
        const size_t guard = g_poison ? POISON_GUARD : 0;
        hipError_t e = hipMalloc((void **)&p, count * sizeof(T) + guard);
        // the clear runs on the NULL stream, which the engine's non-blocking streams do not wait for: finish it here
        if (e == hipSuccess) e = hipMemset(p, 0, count * sizeof(T));
        if (e == hipSuccess && guard) e = hipMemset((char *)p + count * sizeof(T), 0xFF, guard);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        return e;
    }
    // alloc(count) and the host's `count` elements copied in: one result for the chain of a call that stages several buffers
    hipError_t upload(const T *src, size_t count) {
        hipError_t e = alloc(count);
        if (e == hipSuccess && count > 0) e = hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice);
        return e;
    }
    hipError_t upload(const std::vector<T> &src) { return upload(src.data(), src.size()); }
    // device to device, into this buffer as it is allocated: `rows` rows of `count` elements from `src`, whose rows are `pitch` apart
    hipError_t copy_rows(const DevBuf &src, size_t count, size_t pitch, size_t rows = 1) const {
        hipError_t e = hipSuccess;
        for (size_t k = 0; e == hipSuccess && k < rows; k++) e = hipMemcpy(p + k * count, src.p + k * pitch, count * sizeof(T), hipMemcpyDeviceToDevice);
        return e;
    }
    // CSF_DEBUG_POISON: elements [from, n) become 0xFF bytes
    hipError_t poison_from(size_t from) {
        if (!g_poison || !p || from >= n) return hipSuccess;
        hipError_t e = hipMemset(p + from, 0xFF, (n - from) * sizeof(T));
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        return e;
    }
    // grow-only scratch: contents undefined
    hipError_t reserve(size_t count) { return count <= n ? hipSuccess : alloc(count); }
    void release() {   // (the result is ignored: this runs in destructors, and leaves no error behind for the next call to find)
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};
static_assert(!std::is_copy_constructible<DevBuf<char>>::value && !std::is_copy_assignable<DevBuf<char>>::value, "a DevBuf has one owner");

// The same for pinned host memory.  Mapped (the default): `dev` is the address a kernel reaches the buffer by - its stores ARE
// the transfer.  Contents are undefined after alloc and reserve.
template <class T, bool Mapped = true>
struct HostBuf {
    T *p = nullptr, *dev = nullptr;
    size_t n = 0;
    HostBuf() = default;
    HostBuf(const HostBuf &) = delete;
    HostBuf &operator=(const HostBuf &) = delete;
    ~HostBuf() { release(); }
    hipError_t alloc(size_t count) {
        release();
        if (count == 0) return hipSuccess;
        hipError_t e = hipHostMalloc((void **)&p, count * sizeof(T), Mapped ? hipHostMallocMapped : hipHostMallocDefault);
        if (e == hipSuccess && Mapped) e = hipHostGetDevicePointer((void **)&dev, p, 0);
        if (e == hipSuccess) n = count;
        return e;
    }
    // grow-only; a kernel on `st` may still write the old buffer: wait for it before the buffer goes.  floor == 0: exactly `need`
    // elements, else max(2 * need, floor)
    hipError_t reserve(size_t need, hipStream_t st, size_t floor = 0) {
        if (need <= n) return hipSuccess;
        if (p) {
            hipError_t e = hipStreamSynchronize(st);
            if (e != hipSuccess) return e;
        }
        return alloc(floor ? std::max(2 * need, floor) : need);
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = dev = nullptr;
        n = 0;
    }
};
static_assert(!std::is_copy_constructible<HostBuf<char>>::value && !std::is_copy_assignable<HostBuf<char>>::value, "a HostBuf has one owner");

// Measurement and test knobs.  Read from the environment ONCE per engine, in csf_create: nothing on the tick path or in
// a re-binning calls getenv.
struct Knobs {
    double far_eps = 5.9604644775390625e-8;   // CSF_FAR_EPS: bound of the far-field / reach cull (2^-24; 0: off)
    bool reach = true;                        // CSF_REACH=0: no per-pair reach test
    std::string trace_blocks;                 // CSF_TRACE_BLOCKS=<file>: per-wave timeline of the last pair launch
    std::string trace_agent;                  // CSF_TRACE_AGENT=<file>: eight time stamps per wave of the last per-agent launch
    int fake_rank = 0, fake_world = 1;        // CSF_FAKE_SHARD=r/w: only rank r's receiver block of w (timing aid)
    int nsplit = 0;                           // CSF_NSPLIT: source chunks of the pair grid (0: the engine's choice)
    int rpb = 0;                              // CSF_RPB: 32 or 16 receivers per workgroup of the cull kernel (0: the engine's choice)
    int wide = -1;                            // CSF_WIDE: workgroups of 8 waves on tiles of 2048 sources (-1: the engine's choice)
    int pair_variant = -1;                    // CSF_PAIR_VARIANT (-1: by population size)
    int64_t rebin_ticks = 64;                 // CSF_REBIN_TICKS: ticks between two re-binnings (1 .. 120; the tests that step 40 - 48 ticks "across a re-binning" pin 32)
    int fused_mid = 1;                        // CSF_FUSED_MID=0: mid-size populations take a pair launch and a per-agent launch per tick (csf_mid.hip: one launch)
    int batch_mid = 1;                        // CSF_BATCH_MID=0: the mid-size members of a batch are stepped in turn (engine/abi_batch.inc)
    int mid_below = 0;                        // CSF_MID_BELOW: ... for populations smaller than this (0: by vehicle class, mid_below_for)
    int mid_group = 0;                        // CSF_MID_GROUP: road users per workgroup of it, 4 / 8 / 16 / 32 (0: about one workgroup per CU)
    int chase = 1;                            // CSF_CHASE: 0 the per-agent launch behind the pair launch, 2 beside it (enqueue_chase_tick), 1 [default] whichever the engine measures faster on its first stretch of eligible ticks
    std::string chase_clock;                  // CSF_CHASE_CLOCK=<file>
    int debug_throw = 0;                      // CSF_DEBUG_THROW: csf_sync throws (1 std::bad_alloc, 2 std::runtime_error) - the test of the boundary (consts.inc: csf_caught)
    int chase_gate_pct = 85;                  // CSF_CHASE_GATE: per cent of the pair workgroups through before the per-agent kernel is let go
    int fused_small = 1;                      // CSF_FUSED_SMALL=0: a handful of road users take the general path too (csf_agent.hip: small_tick_kernel)
    int small_classes = 0;                    // CSF_SMALL_CLASSES=1: csf_small_classes is on from csf_create (csf_small_classes.hip; DESIGN.md 4.6e)
    int mid_classes = 0;                      // CSF_MID_CLASSES=1: csf_mid_classes is on from csf_create (csf_mid_classes.hip; DESIGN.md 4.7c)
    int mid_road = 0;                         // CSF_MID_ROAD=1: csf_mid_road is on from csf_create (csf_mid.hip: the ROAD instances; DESIGN.md 4.7b)
    int segments = -1;                        // CSF_SEGMENTS
    int handout_index = 0;                    // CSF_HANDOUT=index: the pair kernel's workgroups hand their receivers out in index order (0, default: heaviest first, csf_handout.h)
    int wg_order = 1;                         // CSF_WG_ORDER=1 (default): the receiver groups of a source chunk are handed to the pair kernel's workgroups heaviest first (csf_wg_order.h); 0: in index order; index (CSF_EXPERT=1): costs and orders are kept, the launches take index order
    int wg_order_ticks = 64;                  // CSF_WG_ORDER_TICKS: an order is formed again every this many ticks
    int wg_order_min = 2048;                  // CSF_WG_ORDER_MIN: ... for grids of at least this many workgroups (two rounds of the device's 1 024 slots: in a single round every workgroup starts at once, and a rank's block of an 8-way shard - 64 groups x 16 chunks - lost 2.9 us to the order)
    int seg_grid = 1;                         // CSF_SEG_GRID=0: one launch per parameter set (class-segmented order) instead of one grid
    int far_tight = 1;                        // CSF_FAR_TIGHT=0: the far-field radius prices all n sources at the cut (ln(n / eps) / kappa) also where candidate lists say how many a receiver can meet
    int clist = 1;                            // CSF_CLIST=0: receivers in binned order walk every tile of their chunk (no candidate lists)
    int recv_binned = -1;                     // CSF_RECV_BINNED
    int64_t rebin_churn = 4000;               // CSF_REBIN_CHURN
    int hole_reuse = 1;                       // CSF_HOLE_REUSE: an arrival takes the slot of a road user that left nearby (HoleIndex)
    int hole_export_kernel = 1;               // CSF_HOLE_EXPORT_KERNEL: a kernel writes places and circles into mapped host memory (0: two hipMemcpyAsync)
    int hole_lazy = 1;                        // CSF_HOLE_LAZY: places and circles are read back after a re-binning only where road users came or went in the period before
    double hole_dist = 1.0;                   // CSF_HOLE_DIST: ... within this many median batch radii of the batch's centre
    bool incremental = true;                  // CSF_INCREMENTAL=0: population changes through the host mirror
    int comm_second = -1;                     // CSF_COMM_STREAM=second / main (-1: the communicator times both on its first tick and keeps the faster)
    double fov_band = 1.0;                    // CSF_FOV_BAND: scale of the rounding band of the field-of-view test (0: every pair decided in fp32, as in round 3)
    double rnear = 1.0;                       // CSF_RNEAR: pairs closer than this (m) are evaluated from the precise records (0: none)
    int road_grid = -1;                       // CSF_ROAD_GRID: 1 the lattice of csf_road.hip for any road, 0 never (-1: large networks)
    double road_cell = 0.0;                   // CSF_ROAD_CELL: edge of its cells in m (0: 16)
    void read() {
        auto geti = [](const char *name, int dflt) {
            const char *v = getenv(name);
            return v ? atoi(v) : dflt;
        };
        if (const char *v = getenv("CSF_FAR_EPS")) far_eps = atof(v);
        reach = geti("CSF_REACH", 1) != 0;
        if (const char *v = getenv("CSF_TRACE_BLOCKS")) trace_blocks = v;
        if (const char *v = getenv("CSF_TRACE_AGENT")) trace_agent = v;
        if (const char *v = getenv("CSF_FAKE_SHARD")) {
            int fr = 0, fw = 1;
            if (sscanf(v, "%d/%d", &fr, &fw) == 2 && fw > 1 && fr >= 0 && fr < fw) fake_rank = fr, fake_world = fw;
        }
        // launch-shape knobs whose A/B is settled (DESIGN.md A.3: every setting but the default measured slower): honoured only
        // with CSF_EXPERT=1, so that a stray variable cannot change the product's grid
        const bool expert = geti("CSF_EXPERT", 0) != 0;
        auto gete = [&](const char *name, int dflt) { return expert ? geti(name, dflt) : dflt; };
        nsplit = gete("CSF_NSPLIT", 0);
        rpb = gete("CSF_RPB", 0);
        wide = gete("CSF_WIDE", -1);
        pair_variant = geti("CSF_PAIR_VARIANT", -1);
        chase = geti("CSF_CHASE", 1);
        debug_throw = geti("CSF_DEBUG_THROW", 0);
        if (const char *v = getenv("CSF_CHASE_CLOCK")) chase_clock = v;
        chase_gate_pct = std::max(0, std::min(100, geti("CSF_CHASE_GATE", 85)));
        fused_small = geti("CSF_FUSED_SMALL", 1);
        small_classes = geti("CSF_SMALL_CLASSES", 0) == 1 ? 1 : 0;
        mid_road = geti("CSF_MID_ROAD", 0) == 1 ? 1 : 0;
        mid_classes = geti("CSF_MID_CLASSES", 0) == 1 ? 1 : 0;
        fused_mid = geti("CSF_FUSED_MID", 1);
        mid_below = geti("CSF_MID_BELOW", 0);
        batch_mid = geti("CSF_BATCH_MID", 1);
        mid_group = geti("CSF_MID_GROUP", 0);
        rebin_ticks = std::max(1, std::min(120, geti("CSF_REBIN_TICKS", 64)));
        segments = geti("CSF_SEGMENTS", -1);
        recv_binned = geti("CSF_RECV_BINNED", -1);
        clist = geti("CSF_CLIST", 1);
        far_tight = geti("CSF_FAR_TIGHT", 1);
        seg_grid = gete("CSF_SEG_GRID", 1);
        if (const char *v = getenv("CSF_WG_ORDER")) wg_order = std::string(v) == "index" ? (expert ? 2 : 0) : (atoi(v) == 1 ? 1 : 0);
        wg_order_ticks = std::max(1, geti("CSF_WG_ORDER_TICKS", 64));
        wg_order_min = std::max(0, geti("CSF_WG_ORDER_MIN", 2048));
        if (const char *v = getenv("CSF_HANDOUT")) handout_index = expert && std::string(v) == "index" ? 1 : 0;
        rebin_churn = std::max(1, geti("CSF_REBIN_CHURN", 4000));
        hole_reuse = geti("CSF_HOLE_REUSE", 1);
        hole_lazy = geti("CSF_HOLE_LAZY", 1);
        hole_export_kernel = geti("CSF_HOLE_EXPORT_KERNEL", 1);
        if (const char *v = getenv("CSF_HOLE_DIST")) hole_dist = atof(v);
        incremental = geti("CSF_INCREMENTAL", 1) != 0;
        if (const char *v = getenv("CSF_COMM_STREAM")) comm_second = std::string(v) == "second" ? 1 : 0;
        if (const char *v = getenv("CSF_RNEAR")) rnear = atof(v);
        if (const char *v = getenv("CSF_FOV_BAND")) fov_band = std::max(0.0, atof(v));
        road_grid = geti("CSF_ROAD_GRID", -1);
        if (const char *v = getenv("CSF_ROAD_CELL")) road_cell = atof(v);
    }
};

}  // namespace

// What the ring read-backs keep across calls (csf_get_record, csf_get_history: one per engine; csf_batch_get_record: one per
// batch), grown geometrically like the packed snapshot's buffer: the descriptors the gather kernel reads and the buffer it packs
// the samples into, both mapped host memory - the kernel's stores ARE the transfer, and the host waits once.
struct RecGather {
    HostBuf<RecDesc> desc;
    HostBuf<double> out;
    hipError_t reserve(size_t members, size_t doubles, hipStream_t st) {
        hipError_t r = desc.reserve(members, st, 16);
        return r != hipSuccess ? r : out.reserve(doubles, st, 4096);
    }
};

// What a measure of a recording keeps across calls (one per engine; a batch uses its first member's): the descriptors the kernels read
// (mapped host memory), the packed output on the device - event counters, then every member's block and events, and behind what is
// transferred the chunks' partial results - and the pinned buffer its one copy lands in.
template <class Desc>
struct MeasureScratch {
    HostBuf<Desc> desc;
    DevBuf<unsigned char> dev;
    HostBuf<unsigned char, false> host;
};

// ... csf_flow / csf_batch_flow: and the layout as the kernels read it (mapped host memory)
struct FlowScratch {
    MeasureScratch<FlowDesc> m;
    HostBuf<double> layout;
};

// ... csf_clearance / csf_batch_clearance: and the road as the kernels read it - staged in pinned memory, copied to the device once per call
struct ClrScratch {
    MeasureScratch<ClrDesc> m;
    HostBuf<unsigned char, false> road_host;
    DevBuf<unsigned char> road;
};

// ... csf_body_encounters / csf_batch_body_encounters: and the extents as the kernels read them - staged in pinned memory, copied to the
// device once per call
struct BodyScratch {
    MeasureScratch<BodyDesc> m;
    HostBuf<double, false> ext_host;
    DevBuf<double> ext;
};

struct csf_engine {
    Dev d{};
    Knobs knobs;
    int device = 0;
    // The streams are declared ahead of every buffer: members go in reverse order, so the buffers are freed while the streams exist.
    hipStream_t main = nullptr, comm = nullptr;
    // The members of a loopback group share ONE main stream (ticks and exchanges in order).  It belongs to all of them: the
    // handle lives as long as any member does, whichever is destroyed first (until round 5 it was the first member's, the
    // others were told when that one went - unless another member had gone before and cleared the lists through which they
    // would have been told: a dangling handle, which hipStreamSynchronize happened to tolerate and hipStreamQuery did not)
    struct StreamHold {
        hipStream_t s = nullptr;
        ~StreamHold() {
            if (s) (void)hipStreamDestroy(s);
        }
    };
    std::shared_ptr<StreamHold> main_hold;
    StreamHold comm_hold;                // (the second stream is the engine's own)
    // parameter sets (csf_set_param_classes): classes[0] is d.p; h_cls[slot] the set of a road user
    std::vector<csf_params> classes;
    std::vector<double> class_kappa;     // far_kappa of every set (the grid search is done once per table)
    // Class-segmented order (several parameter sets, binned): every set is a run of places starting at a multiple of 64,
    // and the pair term is one launch of the culling kernel per run with that set's constants (rebin, launch_pair_all).
    struct Segment {
        int32_t cls;
        int64_t beg, end;                 // places
        int32_t chunk_units, n_split, part_base;
        PairConsts pc;
    };
    std::vector<Segment> segs;
    // ... the runs of the TwoD-field sets as ONE grid (csf_pair.hip: SEG): their table on the device, the grid's y extent
    DevBuf<SegDev> segtab;
    std::vector<SegDev> h_segtab;
    int seg_total_by = 0;
    int32_t sent_slot = 0;               // index of a record that is a sentinel for ever
    std::vector<uint8_t> h_cls;
    DevBuf<csf_params> ptab;
    DevBuf<PairConsts> pctab;
    DevBuf<double> pbtab;
    DevBuf<uint8_t> cls;
    bool classes_dirty = true;
    int64_t cap = 0;        // slots: the caller's capacity + head room for arrivals between two re-binnings (csf_create)
    int64_t cap_user = 0;   // road users the caller may have at once
    hipEvent_t ev_integ = nullptr, ev_gather = nullptr;
    std::string err;

    // host mirror (authoritative only while `host_ahead`; the device is authoritative after a tick)
    std::vector<double> h_s, h_vdes, h_znp, h_hx, h_hy, h_lti, h_ppsi, h_F;
    std::vector<int32_t> h_ptr, h_ti, h_dgood;
    std::vector<uint8_t> h_znav, h_zrid;
    std::vector<uint32_t> h_status;
    std::vector<std::vector<double>> h_q;  // per slot: rows of (x, y, stop) - the host is authoritative for the rows
    std::vector<std::vector<double>> h_script;   // per slot: rows (x, y, psi, v) of an UncontrolledVehicle's prescribed trajectory
    DevBuf<double> script;
    DevBuf<int64_t> sbeg;
    DevBuf<int32_t> slen;
    // The population: road user i of the caller's order lives in slot order[i].  Slots are what every device array is
    // indexed by.  csf_remove_agents on a live device copy only kills slots (they keep a sentinel record), csf_add_agents
    // reuses them; a full upload compacts the slots back into population order.
    std::vector<int32_t> order;
    // Dead slots.  `free_tail`: dead at the last re-binning, so their place in the binned order is in the tail of
    // sentinels behind the real batches - a road user spawned into one of them (or into a fresh slot below n_pad) joins a
    // tail batch of other newcomers and stretches no real batch's circle.  `free_recent`: retired since; their places are
    // inside real batches, so they are handed out only when nothing else is left, and move to `free_tail` at the next
    // re-binning.  `slack`: sentinel slots kept behind the population for arrivals (twice what the last period saw).
    std::vector<int32_t> free_tail, free_recent;   // free_tail: descending, so that pop_back hands out ascending slots
    int64_t live_at_rebin = 0, tail_used = 0;       // road users at the last re-binning; sentinel places handed out since
    int64_t tail_flushed = 0;                       // ... of which the device has seen this many (flush_pending)
    bool pend_inplace = false;                      // an arrival of the pending batch took a slot inside a real batch
    // HOLES (road users arriving and leaving every tick, SUMO co-simulation: intersection.py:458-634).  A road user that leaves
    // leaves a hole in a real batch of the binned order; an arrival that starts within that batch's circle can have the hole -
    // the circle does not grow, the sentinel tail does not fill up, and the order lasts its 64 ticks instead of three.  What the
    // host needs for that it reads back once per re-binning, without waiting: the place of every slot and the circles (85 KB at
    // N = 16 384).  The holes are kept in a lattice over the scene by the centre of their batch.
    struct HoleIndex {
        HostBuf<int32_t> pos;                       // slot -> place at the last re-binning
        HostBuf<float4> bnd;                        // circle of every batch then (scene coordinates)
        std::vector<int32_t> hpos;                  // ... copied to ordinary memory when they have landed (the lookups
        std::vector<float4> hbnd;                   //     per arrival and departure are the host's hot loop under traffic)
        hipEvent_t ev = nullptr;
        bool pending = false, ready = false;        // the read-back is under way / the lattice is built
        int64_t places = 0;                         // places that held road users at the re-binning
        double x0 = 0, y0 = 0, cell = 1, inv_cell = 1, reach2 = 0, ox = 0, oy = 0;
        int nx = 0, ny = 0;
        struct Ent { int32_t slot; float x, y; };   // a hole: the slot and the centre of its batch (scene coordinates)
        static constexpr int CELL_CAP = 5;          // holes a lattice cell can list (one more stays in free_recent, unlisted)
        struct alignas(64) Cell { int32_t n; Ent e[CELL_CAP]; };   // one cache line: the host looks a cell up per arrival
        std::vector<Cell> cell_tab;                 // [ny][nx]
        int64_t taken = 0;                          // arrivals that took a leaver's slot (csf_holes_taken: tests, tools)
    } holes;
    std::vector<int32_t> add_slots;                 // csf_add_agents: the slots of the call's arrivals
    int64_t pend_tail_spawns = 0;                   // arrivals of the pending batch that went to the sentinel tail
    DevBuf<unsigned> ticket;                        // patch_kernel: which workgroup finishes last
    // grow-only device scratch of the single-piece entry points (csf_untracked, csf_update_*, csf_count_pairs): no
    // hipMalloc / hipFree per call
    DevBuf<uint8_t> scratch_u8;
    DevBuf<int32_t> scratch_i32;
    DevBuf<double> scratch_f64;
    DevBuf<unsigned long long> scratch_cnt;
    bool tail_tracked = false;                      // the places of the sentinel tail are known (binned single engine)
    std::vector<uint8_t> h_alive;
    bool order_dirty = true;               // the device copy of `order` is stale
    bool incremental = true;               // csf_set_incremental
    int64_t q_top = 0;                     // rows of the queue slab in use
    int64_t churn = 0;                     // road users spawned into free slots since the last re-binning
    std::vector<double> h_road;            // per vertex (x, y, F0, sigma)
    // the lattice over a large road network (csf_road.hip; build_road_grid): what was built, and for which vertex set
    uint64_t road_version = 1, rg_version = 0;
    double rg_cell = 0, rg_gx0 = 0, rg_gy0 = 0, rg_ox = 0, rg_oy = 0;
    int rg_nx = 0, rg_ny = 0;
    DevBuf<float4> rg_v;
    DevBuf<int32_t> rg_start;
    DevBuf<float> rg_c;
    bool dirty = true;                     // host mirror changed since the last upload
    bool device_ahead = false;             // ticks ran since the last download

    DevBuf<double> s, vdes, q, znp, hx, hy, lti, ppsi, F, hist;
    // csf_record: the force ring beside `hist`, the tick counter the batched launch numbers its samples from (csf_dev.h:
    // Dev::rec_tick) and the value that word holds once everything enqueued has run (-1: unknown, written before the next
    // batched launch); rec_fast: this recording keeps the one-wave tick and the batched launch (csf_enable_history's does not)
    DevBuf<double> hist_F;
    DevBuf<int64_t> rec_tick;
    int64_t rec_tick_dev = -1;
    // the ring's first valid sample (include/csf.h, "The lifetime of a recording"): tick / stride when the ring was started
    // (rings_setup) or the roster last changed (roster_changed); every reader refuses what lies before it (record_range)
    int64_t rec_k0 = 0;
    bool rec_fast = false;
    RecGather rgather;
    DevBuf<int64_t> qbeg;
    DevBuf<int32_t> ptr, ti, dgood, qlen, order_dev;
    DevBuf<uint8_t> znav, zrid, alive;
    // Population changes on a current device copy are collected here and applied by ONE kernel launch at the next
    // device call (flush_pending).  The kernel reads its records from pinned, device-visible host memory: a ring of four
    // buffers, each guarded by an event (the kernel that read a buffer has finished long before the ring comes round).
    struct Pending {
        std::vector<int32_t> retire;
        std::vector<SpawnRec> spawn;       // qbeg relative to `rows` until the flush
        std::vector<QueueRec> requeue;     // the same
        std::vector<double> rows;          // (x, y, stop) rows of new and replaced queues
        bool empty() const { return retire.empty() && spawn.empty() && requeue.empty(); }
    } pend;
    // [cap] per slot, ONE 16-byte entry (a leaver or an arrival touches all four of its slot: four arrays were four cache misses each,
    // 819 times per tick at 5 % churn): index of the slot in the pending lists above and in free_recent, -1: not there
    struct SlotIdx {
        int32_t spawn = -1, requeue = -1, retire = -1, recent = -1;
    };
    std::vector<SlotIdx> sidx;
    std::vector<uint8_t> dev_alive;        // [cap] what d.alive holds on the device (as of the last flush or upload)
    struct PinnedSlot {
        HostBuf<char> buf;
        hipEvent_t done = nullptr;
        bool busy = false;
    };
    PinnedSlot pinned[4];
    int pinned_next = 0;
    DevBuf<uint32_t> status;
    DevBuf<float4> rec, recs, recg, recb, rv, kat4, bnd, bnd2;
    // the fused tick of mid-size populations (csf_mid.hip): the other halves of the record double buffers, the two snapshots of
    // (x, y, psi), the arrival counters; mid_synced: the other halves hold this tick's sentinels and the current snapshot holds
    // this tick's state (any other path that writes records or state clears it)
    DevBuf<float4> rec_alt, recg_alt;
    DevBuf<float2> rec2_alt;
    DevBuf<double> src64_a, src64_b;
    bool mid_synced = false, mid_cur_is_a = true;
    int64_t mid_ticks = 0;
    // the per-agent launch beside the pair launch (enqueue_chase_tick): the binned copy's other half, the arrival counters
    // ([groups of 64 slots]) and the gate's / the error word, whether the last tick took this path (the two streams then have to
    // meet before anything else runs), ticks since the counters were cleared, which stream the next pair launch goes to
    DevBuf<float4> recs_alt;
    DevBuf<unsigned> chase_misc;
    HostBuf<unsigned> chase_err;        // a wait gave up: one word of mapped host memory (csf_sync)
    DevBuf<float4> part4;               // the partial sums of a side-by-side tick as tagged 16-byte granules (csf_dev.h: part4)
    DevBuf<unsigned long long> chase_clock;   // CSF_CHASE_CLOCK=<file>: stamps of the last 64 side-by-side ticks, written at csf_destroy
    bool dirty_layout_for_warm() const { return dirty || !segs.empty() || classes.size() != 1; }   // (the warm pair launch of chase_alloc takes the plain single-set launch)
    // CSF_TIME_POP=1 (measurement aid): nanoseconds inside the population calls, by part, printed at csf_destroy
    bool pop_calls_in_period = false;         // an arrival or a departure reached the device since the last re-binning (binning.inc: holes_request)
    bool time_pop = false;
    int64_t tp_ns[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tp_calls = 0;
    std::vector<int32_t> remove_sorted;   // csf_remove_agents: the listed indices sorted, when the caller's are not
    bool chase_prev = false, chase_resume = false;   // resume: the counters and halves are those of the last side-by-side tick (mid_synced says nothing else wrote records since)
    uint32_t chase_round = 0;
    int chase_parity = 0;
    int64_t chase_ticks = 0;
    // CSF_CHASE=1: decided by measurement, once per engine (chase_take): three periods between re-binnings - in turn, side by side, in turn -, bracketed by events on the
    // main stream - whether the two streams got hardware queues of their own is the runtime's business, and without them the
    // side-by-side tick is the slower one
    int chase_state = 0;                // 0 undecided, 1 side by side, -1 in turn
    int cal_phase = 0;                  // 0 idle, 1 .. 3 the periods (in turn, side by side, in turn), 4 waiting for the last event
    hipEvent_t cal_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    double chase_cal_us[2] = {0.0, 0.0};
    int64_t cal_ticks[3] = {0, 0, 0};   // ticks of every period of the measurement
    DevBuf<float2> borg;
    DevBuf<float2> rvo;          // origins of the road-vertex tiles
    DevBuf<int32_t> pos;
    bool bounds_fresh = false;   // d.bnd describes the current records (else: recompute before the pair kernel)
    DevBuf<int32_t> perm, sort_vals, rlist;
    DevBuf<uint32_t> sort_keys, sort_keys_out;
    DevBuf<uint8_t> sort_tmp;
    int64_t ticks_since_rebin = 0;
    // integration steps since the last re-binning that no pair launch went with (csf_apply_forces, csf_replay_forces on forces
    // from elsewhere): the candidate tile lists and the stretch of the circles allow for rebin_ticks + 2 steps of motion, so
    // these count towards the next re-binning like ticks do
    int64_t moved_unbinned = 0;
    bool pair_since_move = false;
    DevBuf<float2> rec2, recs2, part, froad, kat2;
    // candidate tiles of every receiver group (large populations, csf_dev.h: Dev::clist): rebuilt at every re-binning
    DevBuf<float4> tcirc;
    DevBuf<uint16_t> clist;
    DevBuf<int32_t> ccount;
    DevBuf<unsigned> far_stat;   // [2] what launch_candidate_lists found for the far-field bound (tighten_far_bound)
    double far_met = 0.0, far_tail = 0.0, far_T = 0.0;   // ... and what became of it: sources met, tail (x f_0), T in use (0: the plain bound)
    DevBuf<float2> rorg;         // the origin every precise record is relative to, by slot
    DevBuf<float2> reclo;        // what the record's position left over in fp32 (csf_dev.h); travels with the records
    DevBuf<float4> xbuf;         // the exchange records of a sharded run (csf_dev.h: xbuf), allocated with the shard layout
    bool xbuf_fresh = false;     // other ranks' exchange records have arrived and are not yet spread to rec / reclo / rec2
    bool state_all_current = true;   // every live slot's fp64 state on this device is current (false once a rank has ticked)
    // Field-of-view decisions within fp32 rounding of an edge (csf_dev.h: PairConsts::fovA, EdgeRec; set_fov_band): the
    // largest |coordinate| relative to the scene origin at the last upload (road users, prescribed trajectories, arrivals
    // since), and the integration steps since - nobody moves farther than t_s * v_max per step
    double coord_bound0 = 0.0;
    HostBuf<double, false> bound_pin;   // where the positions land when that bound is measured again (set_fov_band)
    int64_t moves = 0;
    int64_t small_ticks = 0;         // ticks run by the one-wave kernel (csf_small_ticks)
    int64_t field_map_launches = 0;  // launches of csf_field_map: one per requested term (csf_field_map_launches)
    int64_t encounter_launches = 0;  // launches of csf_encounters / csf_batch_encounters: two per call (csf_encounter_launches)
    MeasureScratch<EncDesc> enc;
    int64_t pet_launches = 0;        // launches of csf_post_encroachment / csf_batch_post_encroachment: two per call (csf_pet_launches)
    MeasureScratch<PetDesc> pet;
    int64_t passing_launches = 0;    // launches of csf_passing / csf_batch_passing: two per call (csf_passing_launches)
    MeasureScratch<PassDesc> passing;
    int64_t flow_launches = 0;       // launches of csf_flow / csf_batch_flow: two per call (csf_flow_launches)
    FlowScratch flow;
    int64_t clearance_launches = 0;  // launches of csf_clearance / csf_batch_clearance: three per call (csf_clearance_launches)
    ClrScratch clearance;
    int64_t body_launches = 0;       // launches of csf_body_encounters / csf_batch_body_encounters: two per call (csf_body_encounter_launches)
    BodyScratch body;
    bool small_classes = false;      // csf_small_classes: several parameter sets / an UncontrolledVehicle population take the one-wave tick too
    bool mid_road = false;           // csf_mid_road: the one-launch tick sums the road term of a small road itself (tick.inc: mid_road_ok)
    int64_t mid_road_ticks = 0;      // ... and the ticks on which it did (csf_mid_road_ticks; mid_ticks / batch_mid_ticks count them too)
    bool mid_classes = false;        // csf_mid_classes: several parameter sets / an UncontrolledVehicle population take the one-launch tick too (tick.inc: mid_takes_classes)
    int64_t mid_classes_ticks = 0;   // ... and the ticks mid_classes_kernel took (csf_mid_classes_ticks; mid_ticks / batch_mid_ticks / mid_road_ticks count them too)
    int64_t slab_rewrites = 0;       // compact_slab calls (upload_queues sizes the slab by them)
    bool bound_stale = false;        // positions moved without a speed clamp (csf_replay_forces with fix_speed): measure them
    uint32_t edge_stamp = 0;
    DevBuf<EdgeRec> edge;
    DevBuf<unsigned> edge_n;         // [0] ring counter, [1] near / marginal pairs that could not be noted (csf_near_dropped)
    DevBuf<int32_t> edge_head;
    double far_kappa = 0.0;   // lower bound of the field's decay rate (far_kappa())
    double last_gather_ms = 0.0;  // all-gather time accumulated by the last csf_profile_read
    bool ev_gather_recorded = false;
    HostBuf<char> snap;       // csf_get_tick: the packed read-back (snap_need bytes), written by the kernels themselves
    DevBuf<uint64_t> trace;   // CSF_TRACE_BLOCKS (measurement aid)
    // Heaviest group first (csf_wg_order.h, tick.inc: wg_order_apply): two cost tables and two order tables of chunks x groups words.
    // A pair launch uses table k - the parity of its tick; side by side: of its stream, which is the same thing - so whatever
    // touches table k sits in one stream, in order: the launch two ticks back wrote cost[k], the order kernel in front of this
    // launch reads it and writes order[k], this launch reads order[k] and writes cost[k] again; the launch of the tick between,
    // which may still run on the other stream, has the other pair of tables.
    struct WgOrder {
        DevBuf<uint32_t> cost[2];
        DevBuf<int32_t> order[2];
        int64_t groups = 0;                  // the grid the tables are laid out for (a launch of another grid gets none of them)
        int chunks = 0;
        bool cost_ok[2] = {false, false};    // cost[k] was written by a launch of this grid and these tiles
        bool order_ok[2] = {false, false};   // order[k] holds a permutation per chunk of this grid
        int64_t used[2] = {0, 0};            // launches since order[k] was formed
        int last = -1;                       // the tables of the last tick's pair launch (-1: it kept none), and whether it took an order
        bool last_ordered = false;
        void forget() { cost_ok[0] = cost_ok[1] = order_ok[0] = order_ok[1] = false; }   // grid or tiles changed: index order until costs of the new ones are in
    } wgo;
    DevBuf<uint64_t> atrace;  // CSF_TRACE_AGENT (measurement aid)
    size_t trace_words = 0;

    // sharding
    int rank = 0, world = 1;
    ncclComm_t nccl = nullptr;
    bool gather_pending = false;
    // where the all-gather of a tick is issued: in stream order on the main stream, or on the second stream beside the
    // destination-force phase of the next tick (DESIGN §5).  Chosen by the communicator itself on its first tick
    // (calibrate_comm_stream: both orders timed on the REAL communicator, the same answer on every rank) unless
    // CSF_COMM_STREAM says which.
    bool comm_second = false, comm_calibrated = false;
    float comm_cal_us[2] = {0.f, 0.f};       // what the calibration measured per tick: stream order, second stream

    // loopback rehearsal of the sharded path: `world` engines of one process on one device share a stream and exchange
    // their record blocks with device-to-device copies where the ranks of a real run call ncclAllGather
    std::vector<csf_engine *> group;
    bool loopback = false;

    // csf_batch_join: the batch this engine belongs to (shared by its members; engine/abi_batch.inc) and, while it does, the
    // engine's own stream, kept for when it leaves (the members tick on the first member's)
    std::shared_ptr<struct BatchState> batch;
    std::shared_ptr<StreamHold> own_hold;
    // csf_calib_load: the resident calibration data set and the reset image (engine/abi_calib.inc); while it is there the engine
    // takes csf_calib_eval, csf_calib_clear, csf_set_dest_queue (a route for its vehicles) and the read-backs, and refuses everything
    // that steps it, changes its population, parameters or recording, or writes navigation state (calib_refuses)
    std::shared_ptr<struct CalibState> calib;
    // csf_scene_calib_load: the same for closed-loop scenes (engine/abi_scene.inc); such an engine takes csf_scene_calib_eval,
    // csf_scene_calib_clear and the read-backs
    std::shared_ptr<struct SceneCalibState> scene_calib;
    int64_t batch_ticks = 0;         // ticks run inside a batched ONE-WAVE launch (csf_batch_ticks)
    int64_t batch_mid_ticks = 0;     // ticks run inside a batched one-launch tick (csf_batch_mid_ticks; mid_ticks counts them too)
    // csf_step_batch, mid-size members: the launches of a re-binning on the plain order (identity order, records re-expressed) and
    // the copy into the other halves are not enqueued by rebin / mid_prelude but noted here (MID_DUE_*): the batch runs them for
    // all its members that are due in one launch each
    bool mid_defer = false;
    uint32_t mid_deferred = 0;

    // profiling: a fixed pool of event slots, recycled in order (the oldest slot is resolved into the running sums
    // before it is reused, so stepping with profiling left on holds a bounded number of events)
    int profile = 0;             // 0 off, k > 0: time the kernels of every k-th tick
    struct ProfSlot {
        hipEvent_t ev[8] = {};   // pair, road, agent: start / end of the kernel itself; all-gather: recorded around it
        bool pair = false, road = false, agent = false, gather = false;
    };
    std::vector<ProfSlot> prof_pool;
    size_t prof_issued = 0, prof_resolved = 0;
    double prof_ms[4] = {0, 0, 0, 0};   // pair, road, agent, gather
    int64_t prof_cnt[4] = {0, 0, 0, 0}; // launches behind each sum
    int64_t prof_ticks = 0;             // sampled ticks issued (the kernels beside the pair kernel are timed on every 8th)
    std::vector<float> prof_us[4];      // per sampled launch and kernel - pair, road, per-agent, all-gather - (at most PROF_KEEP of each)
};

// (engine/abi_batch.inc; csf_destroy dissolves the batch of the engine it destroys)
static int batch_dissolve(csf_engine *e);

// (defined with the side-by-side tick, used by upload_all)
static bool chase_shape(const csf_engine *e);
static int chase_alloc(csf_engine *e);
