// csf_small_body.inc - the one-wave tick of a handful of road users (DESIGN.md 4.6): included by csf_agent.hip (small_tick_kernel,
// small_batch_kernel), by csf_scene.hip (scene_eval_kernel), by csf_scene_mixed.hip (scene_mixed_kernel, scene_lanes_mixed_kernel) and by csf_small_classes.hip inside namespace csf, behind csf_agent_dev.h and csf_field.h.  An
// include and not a __device__ function of a translation unit of its own, as csf_mid_body.inc is (DESIGN.md 4.6d): the kernels of
// csf_agent.hip keep the instruction stream they had when the body stood in that file.
//
// wide_tick_body (csf_wide_body.inc) is this body for a workgroup.  What the two share as functions stands in csf_tick_terms.h, included
// below: the Bicycle field's entry of a lane.  The pair loop, the road loop and the switch to agent_body<M> are still written out in both -
// marked TWIN COPY or with a note: a change in one is made in the other.
//
// HOOK: what a caller does behind every tick - hook(d, t, lane, n) is called by all 64 lanes once the tick's stores are issued
// (lanes 0 .. n - 1 have just written their road user's state: their own stores, program order).  NoTickHook is empty and
// compiles to nothing; csf_scene.hip sums an error there.
//
// HOOK::MASKED (DESIGN.md 4.10d): the hook knows which road users are in the scene at a tick.  hook.present(t) is then called by all
// 64 lanes at the head of tick t and returns the same 64-bit mask in every lane - bit j: road user j is present (a ballot: scalar
// registers).  An absent road user is no source, no receiver, is not ticked and gets no road term; its lane still stages its
// (unchanged) state, takes part in every shuffle and barrier and calls the hook - the mask gates work, never the control flow
// around a barrier or a shuffle.  With MASKED == false every use of the mask is compiled out (if constexpr) and the body is the one
// it was before there was a mask.
//
// HOOK::SHARED (DESIGN.md 4.10e): a lane's slot takes several road users in turn.  hook.takeover(d, t, lane) is then called by all
// 64 lanes at the head of tick t, before hook.present(t): a lane whose next occupant enters at t makes its slot that road user's
// fresh vehicle.  The step holds no shuffle, ballot or barrier and stores to the lane's own slot only; what the other lanes read of
// it they read afterwards, in program order - as they read the stores of the tick before.  With SHARED == false it is compiled out.
//
// HOOK::GROUPS (DESIGN.md 4.10g): the road users carry one of hook.n_groups parameter sets of the one vehicle class, Dev::p / pc / pb
// being group 0's.  The parameters become a property of the road user:
//   pair term        hook.consts(j) / hook.hfov(j) are the field constants and the field of view of SOURCE j's set (LDS, indexed by the
//                    source's group: the loop over the sources keeps its order, so the sum of a receiver is formed in today's order
//                    whatever the labels); hook.v_ref(lane) the v_max_riding[1] of the lane's own set for its Bicycle (e, ...) entry.
//                    The priority rule stays Dev::p's - it belongs to the intersection (csf_pair.hip: launch_pair takes d.pc.p2r).
//   per-agent tick   a loop over the groups, uniform: hook.select(dg, g) puts record g's p / pb into a copy of the Dev and the lanes
//                    whose road user is of group g run agent_body on it; a group nobody present belongs to is skipped (a ballot).
//                    n_groups is a kernel argument: no loop added here depends on the state for its end.
// With GROUPS == false all of it is compiled out and the body is the one it was.
//
// MODEL == SMALL_MIXED (DESIGN.md 4.10i; csf_scene.hip: scene_mixed_kernel): the vehicle CLASS is a property of the group too.  The hook
// is a GROUPS hook that also knows the classes - hook.own_model() the class of the lane's own road user, hook.src_model(j) that of
// source j (LDS), hook.group_model(g) that of group g (uniform):
//   pair term        source j acts with the field of ITS class (intersection.py:797-823; csf_pair.hip for has_bike && (model_mask & ~1)):
//                    field_bicycle with the (e, 1 / sqrt(1 - e^2)) its own lane has staged, or field_twod.  `se` has a cell per lane
//                    and is written by the lanes whose road user is a Bicycle; nobody reads another cell.  The loop order is unchanged.
//   per-agent tick   inside the uniform loop over the groups a uniform switch on the group's class to agent_body<M>; no barrier,
//                    shuffle or ballot stands under a divergent condition.
// Every line of it stands under `if constexpr (MIXED)`: an instance of a real class is the one it was.
//
// HOOK::BY_CLASS (DESIGN.md 4.6e; csf_small_classes.hip: the stepping engine's own mixed populations): a SMALL_MIXED hook whose cells are
// indexed by the road user, not by a group, and whose per-agent tick runs on the engine's tables - one pass per vehicle CLASS present, the
// loop uniform over the bits of Dev::model_mask (a kernel argument), agent_body<M, HET = true> picking the lane's own row of Dev::ptab / pbtab
// and returning for a lane of another class; the UncontrolledVehicle's class is among them.  A hook without the member has it false
// (HookByClass), and every line of it stands under that condition.
constexpr int SMALL_MIXED = -1;   // (no enum csf_model)

#include "csf_tick_terms.h"   // bicycle_se: shared with csf_wide_body.inc

template <class H, class = void>
struct HookByClass { static constexpr bool value = false; };
template <class H>
struct HookByClass<H, decltype((void)H::BY_CLASS)> { static constexpr bool value = H::BY_CLASS; };

struct NoTickHook {
    static constexpr bool MASKED = false;
    static constexpr bool SHARED = false;
    static constexpr bool GROUPS = false;
    __device__ __forceinline__ void operator()(const Dev &, int, int, int) {}
};

// ---- a handful of road users: the whole tick in one wave, any number of ticks in one launch ---------------------------------
// The reference's own scenarios (three cyclists at a crossing, scenarios/*.py; BASELINE config 1) are latency, not work: a pair
// launch and a per-agent launch of 5 - 6 us each, nearly all of it launch, teardown and first round trips (DESIGN 4.3).  Up to
// SMALL_MAX road users of one class (not the UncontrolledVehicle's) are ticked by ONE wave instead - lane = road user - with nothing between the
// phases but the wave's own program order, and csf_step(n) is one launch for all n ticks:
//   snapshot (x, y, psi) of every road user, staged in LDS                intersection.py:660-677
//   every source j of the lane's group in turn: receiver - source formed in fp64; the field of view and
//   np.sign(phi) decided in fp32 on that difference with the band of ITS rounding (csf_field.h: tracked_precise,
//   side_undecided - the predicates of the pair kernels' exact path) and, inside the band, as the reference decides them -
//   fp64 atan2 -> limitAngle -> angleDifference (csf_dev.h: untracked_exact_xy), acos -> limitAngle -> sign
//   (sign_phi_exact); the field in fp32, summed in fp64 (per group in source order, the groups pairwise)
//                                                                         intersection.py:690-745, 814-843; vehicle.py:1560-1648
//   the per-agent tick with that sum (agent_body<FUSED>)                  see the head of this file
// No records are binned, nothing is noted or handed over: every yes / no is settled on the spot.
// The body is shared by small_tick_kernel (one scene, its Dev in the kernarg segment) and small_batch_kernel (one scene per
// workgroup, the Dev records in a table in global memory): `srv` is the LDS that stages the road, `snap` the packed read-back
// behind the last tick (NULL: none), `tick0` the ticks the engine has done before this launch (what the samples of csf_record and
// csf_enable_history are numbered from: sample k = state after tick (k + 1) * stride).
template <int MODEL, class HOOK>
__device__ __forceinline__ void small_tick_body(const Dev &d, const int n_ticks, double *const snap, float4 *const srv, const uint32_t ka_lines,
                                                const int64_t tick0, HOOK &hook) {
    // Lane = (receiver, source group): with P the power of two that holds the road users, lane % P is the receiver and lane / P
    // one of 64 / P groups that share the sources between them (source j belongs to group j % G) - all 64 lanes work on the
    // pair term whatever the population, and the groups' sums meet in lanes 0 .. n - 1, which then tick their road user.
    __shared__ double sx[SMALL_MAX], sy[SMALL_MAX], spsi[SMALL_MAX], scs[SMALL_MAX], ssn[SMALL_MAX];
    constexpr bool MIXED = MODEL == SMALL_MIXED;
    __shared__ float2 se[MODEL == CSF_BICYCLE || MIXED ? SMALL_MAX : 1];   // Bicycle field: (e, 1 / sqrt(1 - e^2)) of every source (vehicle.py:1062-1064)
    const int lane = (int)threadIdx.x;
    const int n = (int)d.n;
    int P = 1;
    while (P < n) P <<= 1;
    const int G = WAVE / P, i = lane & (P - 1), grp = lane / P;
    const int64_t cap = d.cap;
    const bool live = i < n;
    const int64_t a = live ? i : 0;
    const PairConsts k = d.pc;
    const bool p2r = d.p.priority_rule == CSF_P2R;
    // road elements (intersection.py:226-242; the curve scenario's ~1 500 vertices): staged once per launch - they are static
    const int nvp = (int)d.nv_pad;
    for (int v = lane; v < nvp; v += WAVE) srv[v] = d.rv[v];
    // the recording (Dev::hist, hist_F): ticks until the next sampled one and its ring slot, divided out once per launch and
    // counted on from there (uniform: scalar registers, nothing of it in the tick loop but a compare and an add)
    int rec_wait = -1, rec_next = 0;
    if (d.hist != nullptr) {
        const int64_t rem = (tick0 + 1) % d.hist_stride;
        rec_wait = rem == 0 ? 0 : (int)(d.hist_stride - rem);
        rec_next = (int)(((tick0 + 1 + rec_wait) / d.hist_stride - 1) % d.hist_cap);
    }
    for (int t = 0; t < n_ticks; t++) {
        int rec_slot = -1;
        if (rec_wait == 0) {
            rec_slot = rec_next;
            rec_next = rec_next + 1 == d.hist_cap ? 0 : rec_next + 1;
            rec_wait = d.hist_stride;
        }
        if (rec_wait > 0) rec_wait--;
        // who is in the scene at this tick (uniform); `act`: this lane's receiver is live and present, `mine`: this lane has a road
        // user to tick (lane < n: i == lane, the receiver is the lane's own road user)
        uint64_t here = ~0ull;
        bool act = live, mine = lane < n;
        if constexpr (HOOK::SHARED) hook.takeover(d, t, lane);
        if constexpr (HOOK::MASKED) {
            here = hook.present(t);
            act = live && ((here >> i) & 1ull) != 0;
            mine = mine && act;
        }
        // (own stores of the previous tick: the lanes of the first group wrote them, in this wave: program order)
        const double x = d.s[a], y = d.s[cap + a], psi = d.s[2 * cap + a];
        double sp, cp;
        sincos(psi, &sp, &cp);
        if (lane < n) sx[lane] = x, sy[lane] = y, spsi[lane] = psi, scs[lane] = cp, ssn[lane] = sp;
        bool bike = MODEL == CSF_BICYCLE;
        if constexpr (MIXED) bike = hook.own_model() == CSF_BICYCLE;
        if (bike && lane < n) {                                    // (what write_record keeps in rec2 for the pair kernels)
            double vref = d.p.v_max_riding[1];
            if constexpr (HOOK::GROUPS) vref = hook.v_ref(lane);   // (the lane's own set: what write_record takes for rec2)
            se[lane] = bicycle_se(d.s[3 * cap + a], vref);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const Recv r{0.f, 0.f, (float)cp, (float)sp};
        double rx = 0.0, ry = 0.0;
        // (TRIED: the body of this loop from `ex = x - xs` to `ry += wy` as exact_pair_term(...) of csf_tick_terms.h, for both bodies.  In the
        // shape that kept the parent's bits - the sum in and out by value - it kept every resource figure and opcode count too, but over five
        // rounds 6 of 92 figures were slower than the parent by more than its spread, scene_eval_kernel<TwoD> at 256 sets by 0.7 %:
        // profiles/tick_terms_ab.txt, 1. and 3.  So the loop stays written out twice.)
        // (TWIN COPY: the pair loop of wide_tick_body, csf_wide_body.inc, is this loop for a workgroup; a change here is made there too)
        for (int j = grp; j < n; j += G) {                         // (lanes of one group: the same j)
            const double xs = sx[j], ys = sy[j], ps = spsi[j];
            const PairConsts *kp = &k;                             // the SOURCE's field and field of view (intersection.py:733-735, 815)
            double hfov = d.p.hfov;
            if constexpr (HOOK::GROUPS) kp = hook.consts(j), hfov = hook.hfov(j);
            const PairConsts &ks = *kp;
            const double ex = x - xs, ey = y - ys;                 // vehicle.py:1615-1616
            // the receiver itself and a road user on the very same spot (D2) add nothing
            if constexpr (HOOK::MASKED) {
                if (((here >> j) & 1ull) == 0) continue;           // (a road user that is not there is nobody's source)
            }
            if (!act || j == i || (ex == 0.0 && ey == 0.0)) continue;
            const float dx = (float)ex, dy = (float)ey, r2 = fmaxf(dx * dx + dy * dy, 1e-30f);
            const float4 q = make_float4(0.f, 0.f, (float)scs[j], (float)ssn[j]);
            bool edge;
            bool seen = p2r ? tracked_precise<true>(ks, ks.chs, r, dx, dy, r2, edge) : tracked_precise<false>(ks, ks.chs, r, dx, dy, r2, edge);
            if (edge) seen = !untracked_exact_xy(xs, ys, x, y, psi, hfov, p2r);   // (one pair in a million)
            if (!seen) continue;
            int sg = 1;
            float F, gx, gy;
            bool bike_src = MODEL == CSF_BICYCLE;
            if constexpr (MIXED) bike_src = hook.src_model(j) == CSF_BICYCLE;
            if (bike_src) {                                         // vehicle.py:1054-1147: no jump at phi = 0
                field_bicycle(ks, q, se[j], dx, dy, r2, F, gx, gy);
            } else {
                float sgf = 0.0f;                                   // 0: the sign of the fp32 sine
                if (side_undecided(ks, q, dx, dy, r2)) {
                    sg = sign_phi_exact(xs, ys, ps, x, y);
                    sgf = sg < 0 ? -1.0f : 1.0f;
                }
                field_twod(ks, r, q, dx, dy, r2, F, gx, gy, sgf);
            }
            double wx = (double)(F * gx), wy = (double)(F * gy);
            if (sg == 0) {                                          // phi = 0 exactly: no tangential part, |F| = P along the line
                const double Pm = sqrt(wx * wx + wy * wy), il = 1.0 / sqrt(ex * ex + ey * ey);
                wx = Pm * ex * il;
                wy = Pm * ey * il;
            }
            rx += wx;
            ry += wy;
        }
        // the groups' sums of a receiver, added pairwise in a fixed order: every lane of it ends with the total
        for (int o = P; o < WAVE; o <<= 1) {
            rx += __shfl_xor(rx, o, WAVE);
            ry += __shfl_xor(ry, o, WAVE);
        }
        if (nvp > 0) {
            // (TRIED: this loop as road_term_share(d, srv, nvp, x, y, grp, G) of csf_tick_terms.h, for both bodies - the same bits and the same
            // resource figures, but figures of the scene kernels slower than the parent's by more than its spread: profiles/tick_terms_ab.txt, 4.
            // The loop of wide_tick_body, csf_wide_body.inc, is the other copy: a change here is made there too.)
            // vertices as offsets from the origin of their tile of 1 024 (csf_dev.h: rv, rvo): the receiver's offset from it is formed
            // in fp64; the sum as road_kernel forms it (fp32, r^-(sigma+1) as a power of rsq(r^2) where every edge shares an integer sigma)
            float qx = 0.f, qy = 0.f;
            const double bx = x - d.ox, by = y - d.oy;
            for (int base = 0; base < nvp; base += 1024) {
                const float2 ot = d.rvo[base >> 10];
                const float rxo = (float)(bx - (double)ot.x), ryo = (float)(by - (double)ot.y);
                const int cnt = nvp - base < 1024 ? nvp - base : 1024;
                for (int u = grp; u < cnt; u += G) {
                    const float4 v = srv[base + u];                // (x, y, -F0, -(sigma + 1) / 2); padding has F0 = 0
                    const float ex = v.x - rxo, ey = v.y - ryo, r2 = ex * ex + ey * ey;
                    float m;
                    if (d.road_np) {
                        const float inv = fminf(fast_rsq(r2), 1e6f), i2 = inv * inv;   // r = 0: finite, times ex = ey = 0
                        m = d.road_np == 2 ? i2 : d.road_np == 3 ? i2 * inv : d.road_np == 4 ? i2 * i2 : d.road_np == 5 ? i2 * i2 * inv : i2 * i2 * i2;
                    } else {
                        m = fast_exp2(fminf(v.w * fast_log2(r2), 120.f));
                    }
                    m *= v.z;
                    qx = m * ex + qx;
                    qy = m * ey + qy;
                }
            }
            for (int o = P; o < WAVE; o <<= 1) {
                qx += __shfl_xor(qx, o, WAVE);
                qy += __shfl_xor(qy, o, WAVE);
            }
            if (mine) d.froad[lane] = make_float2(qx, qy);        // (agent_body reads it back: the same lane, program order)
        }
        __builtin_amdgcn_wave_barrier();                          // (the staged snapshot is read by every lane before it is renewed)
        if constexpr (HookByClass<HOOK>::value) {
            // (TRIED: one agent_body_of_class<HET, WITH_UNCONTROLLED> for this switch and its two twins - SGPR spills and AGPRs of all six kernels that hold it moved: profiles/tick_terms_resource_usage.txt, 3.)
            constexpr int PH = PH_DEST | PH_COMBINE | PH_INTEGRATE;
#pragma nounroll
            for (int m = 0; m < 7; m++) {                          // (uniform: the classes of the population, a kernel argument)
                if (((d.model_mask >> m) & 1) == 0) continue;
                switch (m) {                                        // (agent_body<M, true>: a lane of another class returns at once)
                case CSF_BICYCLE: if (mine) agent_body<CSF_BICYCLE, true, true>(d, PH, lane, nullptr, ka_lines, rx, ry, rec_slot); break;
                case CSF_TWOD: if (mine) agent_body<CSF_TWOD, true, true>(d, PH, lane, nullptr, ka_lines, rx, ry, rec_slot); break;
                case CSF_INVPEND: if (mine) agent_body<CSF_INVPEND, true, true>(d, PH, lane, nullptr, ka_lines, rx, ry, rec_slot); break;
                case CSF_PLANARPOINT: if (mine) agent_body<CSF_PLANARPOINT, true, true>(d, PH, lane, nullptr, ka_lines, rx, ry, rec_slot); break;
                case CSF_PLANARBIKE: if (mine) agent_body<CSF_PLANARBIKE, true, true>(d, PH, lane, nullptr, ka_lines, rx, ry, rec_slot); break;
                case CSF_BALANCINGRIDER: if (mine) agent_body<CSF_BALANCINGRIDER, true, true>(d, PH, lane, nullptr, ka_lines, rx, ry, rec_slot); break;
                case CSF_UNCONTROLLED: if (mine) agent_body<CSF_UNCONTROLLED, true, true>(d, PH, lane, nullptr, ka_lines, rx, ry, rec_slot); break;
                default: break;
                }
            }
        } else if constexpr (HOOK::GROUPS) {
            Dev dg = d;
#pragma nounroll
            for (int g = 0; g < hook.n_groups; g++) {               // (uniform; the body of agent_body is emitted once, here)
                const bool turn = mine && hook.grp == g;
                if (__ballot(turn) == 0ull) continue;
                hook.select(dg, g);
                if constexpr (MIXED) {
                    constexpr int PH = PH_DEST | PH_COMBINE | PH_INTEGRATE;
                    // (the switch of BY_CLASS above without the UncontrolledVehicle, and the one of csf_wide_body.inc: see the note there)
                    switch (hook.group_model(g)) {                  // (uniform: the class of the group, from its record)
                    case CSF_BICYCLE: if (turn) agent_body<CSF_BICYCLE, false, true>(dg, PH, lane, nullptr, ka_lines, rx, ry, rec_slot); break;
                    case CSF_TWOD: if (turn) agent_body<CSF_TWOD, false, true>(dg, PH, lane, nullptr, ka_lines, rx, ry, rec_slot); break;
                    case CSF_INVPEND: if (turn) agent_body<CSF_INVPEND, false, true>(dg, PH, lane, nullptr, ka_lines, rx, ry, rec_slot); break;
                    case CSF_PLANARPOINT: if (turn) agent_body<CSF_PLANARPOINT, false, true>(dg, PH, lane, nullptr, ka_lines, rx, ry, rec_slot); break;
                    case CSF_PLANARBIKE: if (turn) agent_body<CSF_PLANARBIKE, false, true>(dg, PH, lane, nullptr, ka_lines, rx, ry, rec_slot); break;
                    case CSF_BALANCINGRIDER: if (turn) agent_body<CSF_BALANCINGRIDER, false, true>(dg, PH, lane, nullptr, ka_lines, rx, ry, rec_slot); break;
                    default: break;                                 // (the host admits the six classes only)
                    }
                } else {
                    if (turn) agent_body<MODEL, false, true>(dg, PH_DEST | PH_COMBINE | PH_INTEGRATE, lane, nullptr, ka_lines, rx, ry, rec_slot);
                }
            }
        } else {
            if (mine) agent_body<MODEL, false, true>(d, PH_DEST | PH_COMBINE | PH_INTEGRATE, lane, nullptr, ka_lines, rx, ry, rec_slot);
        }
        hook(d, t, lane, n);
    }
    // csf_step_get_tick: what snapshot_kernel would pack in a launch of its own (slots are the population order here)
    if (snap != nullptr && lane < n) {
        const int ns = d.ns;
        for (int c = 0; c < ns; c++) snap[(int64_t)lane * ns + c] = d.s[(int64_t)c * cap + lane];
        double *F = snap + (int64_t)n * ns;
        F[lane] = d.F[lane];
        F[n + lane] = d.F[cap + lane];
        int32_t *ptr = (int32_t *)(F + 2 * n);
        ptr[lane] = d.ptr[lane];
        uint8_t *zn = (uint8_t *)(ptr + n);
        const int z = d.znav[lane] & 3;
        zn[3 * lane + 0] = z == 0;
        zn[3 * lane + 1] = z == 1;
        zn[3 * lane + 2] = z == 2;
    }
}
