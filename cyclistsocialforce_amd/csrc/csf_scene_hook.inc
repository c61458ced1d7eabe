// csf_scene_hook.inc - what the closed-loop calibration kernels share behind a tick of the one-wave tick: the restore of a slot from the
// image, the rider step, SceneHook and SceneLaneHook.  Included by csf_scene.hip and by csf_scene_mixed.hip inside namespace csf, behind csf_small_body.inc:
// an include and not a translation unit of its own, for the reason given at csf_small_body.inc.

// slot `slot` of the block becomes the fresh vehicle of rider `rider` (row of the image): Vehicle.__init__ (vehicle.py:64-204,
// 1728-1736), see patch_kernel's spawn.  The walk limits are those of the rider's own parameter set.  An array added to the image
// goes in here and into the copy at the head of scene_eval_kernel.
__device__ __forceinline__ void scene_restore(const Dev &d, const SceneDev &c, int64_t slot, int64_t rider, double v_max_walk,
                                              double delta_max_walk) {
    const int64_t a = slot, r = rider, cap = d.cap, ic = c.img_cap;
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
    d.zrid[a] = v < v_max_walk ? 0 : 1;
    d.dgood[a] = (-delta_max_walk < delta && delta_max_walk > delta) ? 1 : 0;
}

// behind tick t, for a lane whose rider is present: a replayed rider (rep: its recorded (x, y, psi, v) after tick 0) takes the
// recorded row, a simulated one adds its error terms against obj (its objective at tick 0) to sse / sae.  `balancing`: the rider is a
// BalancingRiderBicycle - the class of the instance, or under scene_mixed_kernel that of the rider's group (a run-time value there only)
template <int MODEL>
__device__ __forceinline__ void scene_rider_step(const Dev &d, const SceneDev &c, int t, int lane, const double *rep, const double *obj,
                                                 double &sse, double &sae, const bool balancing = MODEL == CSF_BALANCINGRIDER) {
    if (rep != nullptr) {
        // vehicle.s written from the recording (calibration.py:455-460) and what csf_push_state keeps consistent with it
        // (abi_population.inc): this lane's own stores behind its tick's, program order.  Nothing is added to sse / sae.
        const double *r = rep + (int64_t)t * c.n_rep * 4;
        const double x = r[0], y = r[1], psi = r[2], v = r[3];
        const int64_t cap = d.cap;
        d.s[lane] = x;
        d.s[cap + lane] = y;
        d.s[2 * cap + lane] = psi;
        d.s[3 * cap + lane] = v;
        if (balancing) {                                  // (ppsi is the speed of the gains there; the yaw is -x[4], unwrapped)
            const double twopi = 6.283185307179586476925286766559, own = d.lti[4 * cap + lane];
            d.lti[4 * cap + lane] = -psi + twopi * nearbyint((own + psi) / twopi);
        } else {
            d.ppsi[lane] = psi;
        }
        const int64_t slot = d.ti[lane] & (d.hist_len - 1);
        d.hx[slot * cap + lane] = x;
        d.hy[slot * cap + lane] = y;
    } else {
        const double *o = obj + (int64_t)t * c.R * c.n_feat;
        for (int k = 0; k < c.n_feat; k++) {
            const int f = c.feat[k];
            // (a row the class does not have stays zero in the reference's traj: vehicle.py:158-160)
            const double sv = f < d.ns ? d.s[(int64_t)f * d.cap + lane] : 0.0;
            const double e = sv - o[k];                   // a plain difference, no angle wrap: calibration.py:49, 76
            sse += e * e;
            sae += fabs(e);
        }
    }
}

// what SceneHook holds of the rider groups (csf_small_body.inc: HOOK::GROUPS): nothing without them
template <bool GRP>
struct SceneGroupPart {};
template <>
struct SceneGroupPart<true> {
    int n_groups = 1;             // groups of the call (2 .. SCENE_GROUPS_MAX)
    int grp = 0;                  // the group of this lane's rider (a lane without a rider: 0)
    const SceneSet *rec = nullptr;        // the n_groups records of this workgroup's candidate set (global memory, uniform)
    // staged by the kernel in LDS: the pair constants, field of view and v_max_riding[1] of every group, and the group of every rider
    const PairConsts *l_pc = nullptr;
    const double *l_hfov = nullptr, *l_vref = nullptr;
    const uint8_t *l_grp = nullptr;
    __device__ __forceinline__ const PairConsts *consts(int j) const { return l_pc + l_grp[j]; }
    __device__ __forceinline__ double hfov(int j) const { return l_hfov[l_grp[j]]; }
    __device__ __forceinline__ double v_ref(int) const { return l_vref[grp]; }
    // (g is uniform: scalar loads from the record)
    __device__ __forceinline__ void select(Dev &dg, int g) const {
        dg.p = rec[g].p;
#pragma unroll
        for (int k = 0; k < 7; k++) dg.pb[k] = rec[g].pb[k];
    }
};

// ... and of their vehicle classes (csf_small_body.inc: SMALL_MIXED): the class of every group, staged beside its constants
struct SceneMixedPart : SceneGroupPart<true> {
    int model = CSF_TWOD;         // the class of this lane's rider (a lane without a rider: its group 0's)
    const uint8_t *l_model = nullptr;     // [n_groups] (LDS)
    __device__ __forceinline__ int own_model() const { return model; }
    __device__ __forceinline__ int src_model(int j) const { return l_model[l_grp[j]]; }
    __device__ __forceinline__ int group_model(int g) const { return rec[g].p.model; }
};

// behind every tick: lane = rider of the scene, its error terms (a replayed rider: its recorded state instead) and, on a sampled
// tick, its state
template <int MODEL, bool WIN, bool GRP = false>
struct SceneHook : std::conditional_t<MODEL == SMALL_MIXED, SceneMixedPart, SceneGroupPart<GRP>> {
    static constexpr bool MASKED = WIN;
    static constexpr bool SHARED = false;
    static constexpr bool GROUPS = GRP;
    const SceneDev &c;
    const int64_t rider;          // set * R + first rider of the scene + lane: row of sums and of a sample
    const double *obj;            // objective of this lane's rider at tick 0
    const double *rep;            // recorded (x, y, psi, v) of this lane's rider after tick 0; NULL: the rider is simulated
    double *smp;                  // where this lane's next sample goes (NULL: none)
    int wait;                     // ticks until the next sampled one
    int taken = 0;                // samples written
    double sse = 0.0, sae = 0.0;
    const int t_in, t_out;        // WIN: this lane's rider is present at the ticks t_in <= t < t_out (a lane without a rider: never)
    __device__ __forceinline__ SceneHook(const SceneDev &c_, int64_t rider_, const double *obj_, const double *rep_, double *smp_, int t_in_,
                                         int t_out_)
        : c(c_), rider(rider_), obj(obj_), rep(rep_), smp(smp_), wait(c_.stride - 1), t_in(t_in_), t_out(t_out_) {}
    // the riders of the scene that are present at tick t, bit = lane: called by all 64 lanes, the same value in each
    __device__ __forceinline__ uint64_t present(int t) const { return __ballot(t_in <= t && t < t_out); }
    __device__ __forceinline__ void sample(const Dev &d, int lane) {
        for (int r = 0; r < d.ns; r++) smp[r] = d.s[(int64_t)r * d.cap + lane];
        smp += (int64_t)c.n_sets * c.R * d.ns;
        taken++;
    }
    __device__ __forceinline__ void operator()(const Dev &d, int t, int lane, int n) {
        if (lane >= n) return;
        // (not in the scene: nothing of a recording is written, nothing is summed; a sample shows what the slot holds)
        if constexpr (MODEL == SMALL_MIXED) {
            if (!WIN || (t_in <= t && t < t_out)) scene_rider_step<MODEL>(d, c, t, lane, rep, obj, sse, sae, this->model == CSF_BALANCINGRIDER);
        } else {
            if (!WIN || (t_in <= t && t < t_out)) scene_rider_step<MODEL>(d, c, t, lane, rep, obj, sse, sae);
        }
        if (smp != nullptr) {
            if (wait == 0) {
                sample(d, lane);
                wait = c.stride;
            }
            wait--;
        }
    }
};

// what SceneLaneHook holds of the rider groups beside SceneGroupPart: the staged table of the lanes' groups once more, to write to - a
// lane's group changes with its rider (DESIGN.md 4.10h)
template <bool GRP>
struct SceneLaneGroupPart : SceneGroupPart<GRP> {};
template <>
struct SceneLaneGroupPart<true> : SceneGroupPart<true> {
    uint8_t *w_grp = nullptr;     // l_grp, writable: a lane stores to its own cell only
};
// ... and beside SceneMixedPart (csf_scene_calib_lane_classes; DESIGN.md 4.10j): the same cell, the class goes with the group
struct SceneLaneMixedPart : SceneMixedPart {
    uint8_t *w_grp = nullptr;
};

// behind every tick, and at its head: lane = LANE of the scene and the rider it carries at the moment.  GRP (csf_scene_calib_lane_groups;
// DESIGN.md 4.10h): the riders are in groups, and the lane's group is its rider's - `grp` and the lane's cell of the staged table are
// renewed by seat.  A lane nobody rides yet has group 0 and is never present.  MODEL == SMALL_MIXED (csf_scene_calib_lane_classes; DESIGN.md
// 4.10j; always with GRP): the groups are of several vehicle classes, and `model` - what small_tick_body / wide_tick_body stage the Bicycle
// cell by and what the replay write-back branches on - becomes the class of the newcomer's group in seat as well.
template <int MODEL, bool GRP = false>
struct SceneLaneHook : std::conditional_t<MODEL == SMALL_MIXED, SceneLaneMixedPart, SceneLaneGroupPart<GRP>> {
    static constexpr bool MASKED = true;
    static constexpr bool SHARED = true;
    static constexpr bool GROUPS = GRP;
    const SceneDev &c;
    const int64_t row0;           // set * R: first row of the set in sums and in a sample
    int cur = -1;                 // the rider this lane carries (0 .. R - 1), -1: nobody yet
    int nxt = -1;                 // who takes over next, -1: nobody
    int nxt_in = 0x7fffffff;      // ... and the tick it enters at
    int t_in = 0, t_out = 0;      // the window of cur (nobody: never present)
    const double *obj = nullptr;  // objective of cur at tick 0
    const double *rep = nullptr;  // recorded (x, y, psi, v) of cur after tick 0; NULL: it is simulated
    int wait;                     // ticks until the next sampled one
    int taken = 0;                // sampled ticks so far
    double sse = 0.0, sae = 0.0;
    __device__ __forceinline__ SceneLaneHook(const SceneDev &c_, int64_t row0_) : c(c_), row0(row0_), wait(c_.stride - 1) {}
    __device__ __forceinline__ void follower(int r) {
        nxt = r;
        nxt_in = r >= 0 ? c.win_enter[r] : 0x7fffffff;
    }
    // the lane's slot becomes rider r's fresh vehicle - what scene_eval_kernel restores at its head, and what was constant per slot
    // there - and the lane's registers become r's
    __device__ __forceinline__ void seat(const Dev &d, int lane, int r) {
        const int64_t a = lane;
        if constexpr (GRP) {
            // the lane's group becomes r's (an entry the host has checked, clamped all the same: it indexes LDS), the restore takes the
            // limits of r's own record.  The store goes to the lane's OWN cell of the staged table and to no other; the other lanes
            // read it in the pair loop of this tick, and what orders the two is what orders the takeover's stores to the slot:
            //   one-wave tick   the takeover stands at the head of the tick, in front of the staging stores and their fence + wave
            //                   barrier; the pair loop of the tick before ended in front of the wave barrier at that tick's foot
            //   wide tick       the takeover stands behind barrier 2 of the tick before - its pair loop has ended - and in front of
            //                   barrier 1 of its own tick, behind which the pair loop reads the table
            int g = (int)c.group[r];
            g = g < this->n_groups ? g : this->n_groups - 1;
            this->grp = g;
            this->w_grp[lane] = (uint8_t)g;
            if constexpr (MODEL == SMALL_MIXED) this->model = this->l_model[g];   // (staged before the first seat, never written again)
            scene_restore(d, c, a, r, this->rec[g].p.v_max_walk, this->rec[g].p.delta_max_walk);
        } else {
            scene_restore(d, c, a, r, d.p.v_max_walk, d.p.delta_max_walk);
        }
        // (what scene_eval_kernel's riders keep from the load of the data set: a slot is theirs alone there)
        d.vdes[a] = c.img_vdes[r];
        d.qbeg[a] = c.img_qbeg[r];
        d.qlen[a] = c.img_qlen[r];
        cur = r;
        t_in = c.win_enter[r], t_out = c.win_exit[r];
        obj = c.obj + (int64_t)r * c.n_feat;
        const int rcol = c.rep != nullptr ? c.rep_index[r] : -1;
        rep = rcol >= 0 ? c.rep + (int64_t)rcol * 4 : nullptr;
        follower(c.rider_next[r]);
    }
    // the sums of the rider the lane has carried go to its row
    __device__ __forceinline__ void flush() {
        if (cur >= 0) c.sums[row0 + cur] = make_double2(sse, sae);
        sse = sae = 0.0;
    }
    // head of tick t (csf_small_body.inc: HOOK::SHARED): no shuffle, no ballot, no barrier; stores to this lane's own slot and rows
    __device__ __forceinline__ void takeover(const Dev &d, int t, int lane) {
        while (nxt_in <= t) {
            flush();
            seat(d, lane, nxt);
        }
    }
    // (wide_tick_body: the flag of this lane alone - 256 lanes have no ballot)
    __device__ __forceinline__ bool here(int t) const { return t_in <= t && t < t_out; }
    __device__ __forceinline__ uint64_t present(int t) const { return __ballot(t_in <= t && t < t_out); }
    __device__ __forceinline__ void operator()(const Dev &d, int t, int lane, int n) {
        if (lane >= n) return;
        const bool here = t_in <= t && t < t_out;
        if constexpr (MODEL == SMALL_MIXED) {                                    // (the write-back of a replayed rider is that of ITS class)
            if (here) scene_rider_step<MODEL>(d, c, t, lane, rep, obj, sse, sae, this->model == CSF_BALANCINGRIDER);
        } else {
            if (here) scene_rider_step<MODEL>(d, c, t, lane, rep, obj, sse, sae);   // (else: the lane is empty at this tick)
        }
        if (c.states != nullptr) {
            if (wait == 0) {
                if (here) {
                    double *smp = c.states + ((int64_t)taken * c.n_sets * c.R + row0 + cur) * d.ns;
                    for (int r = 0; r < d.ns; r++) smp[r] = d.s[(int64_t)r * d.cap + lane];
                }
                taken++;
                wait = c.stride;
            }
            wait--;
        }
    }
};
