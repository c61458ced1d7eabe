// engine/abi_lifetime.inc - C ABI: version, errors, csf_create / csf_create_v / csf_destroy.
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

// ================================================================================ C ABI ======

extern "C" {

int32_t csf_abi_version(void) { return CSF_ABI_VERSION; }

const char *csf_last_error(const csf_engine *e) { return e ? e->err.c_str() : g_create_error.c_str(); }

csf_engine *csf_create(const csf_params *params, int64_t n_capacity, int32_t device) try {
    if (check_params(nullptr, params)) return nullptr;
    if (n_capacity < 1) {
        fail(nullptr, CSF_E_ARG, "n_capacity must be >= 1");
        return nullptr;
    }
    if (n_capacity > (int64_t)1 << 30) {   // (slots, places and queue rows are 32-bit numbers; the products below stay far from 2^63)
        fail(nullptr, CSF_E_ARG, "n_capacity %lld: an engine holds at most 2^30 road users", (long long)n_capacity);
        return nullptr;
    }
    int ndev = 0;
    hipError_t r = hipGetDeviceCount(&ndev);
    if (r != hipSuccess || ndev <= 0) {
        fail(nullptr, CSF_E_DEVICE, "no HIP device available (%s); this engine has no CPU fallback",
             r != hipSuccess ? hipGetErrorString(r) : "device count 0");
        return nullptr;
    }
    if (device < 0 || device >= ndev) {
        fail(nullptr, CSF_E_DEVICE, "device %d out of range (%d visible)", device, ndev);
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) {
        fail(nullptr, CSF_E_DEVICE, "hipSetDevice(%d) failed", device);
        return nullptr;
    }
    if (const char *pv = getenv("CSF_DEBUG_POISON")) g_poison = atoi(pv) != 0;   // (before the first allocation)
    csf_engine *e = new csf_engine();
    e->device = device;
    e->cap_user = n_capacity;
    // a binned population keeps up to 4096 sentinel slots behind its real batches for arrivals (rebin(), csf_add_agents)
    e->cap = n_capacity + (n_capacity >= BIN_MIN_AGENTS ? std::min<int64_t>(TAIL_SLOTS, n_capacity / 4) : 0);
    // whole batches of 64 slots: n_pad (set_shard) is rounded up to a multiple of 64 and must stay <= cap, the stride of
    // every SoA array - fresh slots are handed out up to n_pad (csf_add_agents)
    e->cap = (e->cap + 63) / 64 * 64;
    e->knobs.read();
    e->small_classes = e->knobs.small_classes != 0;
    e->mid_road = e->knobs.mid_road != 0;
    e->mid_classes = e->knobs.mid_classes != 0;
    e->time_pop = getenv("CSF_TIME_POP") != nullptr;
    e->d.p = *params;
    derive_consts(e);
    auto bail = [&](const char *what) {
        g_create_error = std::string(what) + ": " + e->err;
        csf_destroy(e);
        return (csf_engine *)nullptr;
    };
    if (hipStreamCreateWithFlags(&e->main, hipStreamNonBlocking) != hipSuccess) return bail("stream");
    e->main_hold = std::make_shared<csf_engine::StreamHold>();
    e->main_hold->s = e->main;
    {   // The second stream from ANOTHER priority level: the runtime hands streams of one level out over a small pool of hardware
        // queues (four by default), and two streams that share a queue serialise - the per-agent kernel beside the pair launch
        // (enqueue_chase_tick) then runs behind it after all, with a third launch on top (measured: 120 against 115 us per tick with
        // two engines in one process; 111 with queues of their own).  Priority levels have pools of their own.
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);           // (numerically lower = higher priority)
        if (hi < lo && hipStreamCreateWithPriority(&e->comm, hipStreamNonBlocking, hi) != hipSuccess) e->comm = nullptr;
        (void)hipGetLastError();
        if (!e->comm && hipStreamCreateWithFlags(&e->comm, hipStreamNonBlocking) != hipSuccess) return bail("stream");
        e->comm_hold.s = e->comm;
    }
    if (hipEventCreateWithFlags(&e->ev_integ, hipEventDisableTiming) != hipSuccess) return bail("event");
    if (hipEventCreateWithFlags(&e->ev_gather, hipEventDisableTiming) != hipSuccess) return bail("event");
    if (alloc_all(e) != CSF_OK) return bail("allocation");
    set_shard(e);
    return e;
} catch (...) { csf_caught(nullptr); return nullptr; }

size_t csf_params_size(void) { return sizeof(csf_params); }

csf_engine *csf_create_v(const csf_params *params, size_t params_size, int32_t abi_version, int64_t n_capacity, int32_t device) try {
    // before anything is read from `params`: a hand-declared struct of another ABI is shorter (or longer) than ours
    if (params_size != sizeof(csf_params) || abi_version != CSF_ABI_VERSION) {
        fail(nullptr, CSF_E_ABI, "csf_create_v: the caller's csf_params has %zu bytes and ABI %d, this library's has %zu bytes and ABI %d "
             "(include/csf.h: field order and size are ABI)", params_size, (int)abi_version, sizeof(csf_params), (int)CSF_ABI_VERSION);
        return nullptr;
    }
    return csf_create(params, n_capacity, device);
} catch (...) { csf_caught(nullptr); return nullptr; }

int csf_destroy(csf_engine *e) try {
    if (!e) return CSF_OK;
    (void)hipSetDevice(e->device);
    if (e->batch) (void)batch_dissolve(e);   // (the other members go on as single engines, each on its own stream again)
    if (e->main) (void)hipStreamSynchronize(e->main);
    if (e->comm) (void)hipStreamSynchronize(e->comm);
    if (e->time_pop && e->tp_calls > 0)
        fprintf(stderr, "CSF_TIME_POP per call (us): remove: loop %.1f (of it holes_add %.1f) compaction %.1f | add: slots %.1f (of it holes_take %.1f) fill %.1f | queues %.1f  [%lld calls]\n",
                e->tp_ns[0] / 1e3 / e->tp_calls, e->tp_ns[1] / 1e3 / e->tp_calls, e->tp_ns[2] / 1e3 / e->tp_calls, e->tp_ns[3] / 1e3 / e->tp_calls,
                e->tp_ns[4] / 1e3 / e->tp_calls, e->tp_ns[5] / 1e3 / e->tp_calls, e->tp_ns[6] / 1e3 / e->tp_calls, (long long)e->tp_calls);
    if (e->chase_clock.p) {
        std::vector<unsigned long long> h(128 * 8);
        if (hipMemcpy(h.data(), e->chase_clock.p, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost) == hipSuccess) {
            static std::atomic<int> g_clock_files{0};     // (one file per engine of the process, in the order they are destroyed)
            const int fk = g_clock_files.fetch_add(1);
            const std::string path = fk == 0 ? e->knobs.chase_clock : e->knobs.chase_clock + "." + std::to_string(fk);
            if (FILE *f = fopen(path.c_str(), "wb")) {
                fwrite(h.data(), sizeof(h[0]), h.size(), f);
                fwrite(&e->chase_ticks, sizeof e->chase_ticks, 1, f);
                fclose(f);
            }
        }
    }
    if (e->atrace.p) {  // CSF_TRACE_AGENT=<file>: the stamps of the last per-agent launch
        std::vector<uint64_t> h(e->atrace.n);
        if (hipMemcpy(h.data(), e->atrace.p, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost) == hipSuccess) {
            if (FILE *f = fopen(e->knobs.trace_agent.c_str(), "wb")) {
                fwrite(h.data(), sizeof(uint64_t), h.size(), f);
                fclose(f);
            }
        }
    }
    if (e->trace.p) {  // CSF_TRACE_BLOCKS=<file>: workgroup timeline of the last pair-kernel launch
        std::vector<uint64_t> h(e->trace_words);
        if (hipMemcpy(h.data(), e->trace.p, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost) == hipSuccess) {
            if (FILE *f = fopen(e->knobs.trace_blocks.c_str(), "wb")) {
                fwrite(h.data(), sizeof(uint64_t), h.size(), f);
                fclose(f);
            }
        }
    }
    if (e->nccl && g_rccl.CommDestroy) g_rccl.CommDestroy(e->nccl);
    for (auto &sl : e->prof_pool)
        for (hipEvent_t ev : sl.ev)
            if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : e->cal_ev)
        if (ev) (void)hipEventDestroy(ev);
    if (e->ev_integ) (void)hipEventDestroy(e->ev_integ);
    if (e->ev_gather) (void)hipEventDestroy(e->ev_gather);
    if (e->holes.ev) (void)hipEventDestroy(e->holes.ev);
    for (auto &sl : e->pinned)
        if (sl.done) (void)hipEventDestroy(sl.done);
    for (csf_engine *m : e->group)          // the others of a loopback group lose this member: no group any more (csf_step_group says so)
        if (m != e) m->group.clear();
    // every buffer of the engine goes with it, ahead of its streams (the order of csf_engine's members); the main stream itself
    // goes with its last holder
    delete e;
    return CSF_OK;
} catch (...) { return csf_caught(nullptr); }   // (the engine may be gone by now: the sentence goes where csf_last_error(NULL) finds it)

int64_t csf_num_agents(const csf_engine *e) { return e ? (int64_t)e->order.size() : 0; }
int32_t csf_num_states(const csf_engine *e) { return e ? e->d.ns : 0; }
