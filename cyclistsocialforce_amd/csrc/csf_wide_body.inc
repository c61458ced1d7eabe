// csf_wide_body.inc - the tick of csf_small_body.inc for ONE WORKGROUP of 256 threads: 33 .. WIDE_MAX road users present at once
// (DESIGN.md 4.10f).  Included by csf_scene.hip (scene_wide_kernel) and by csf_scene_mixed.hip (scene_wide_mixed_kernel) inside namespace
// csf, behind csf_small_body.inc - and so behind csf_tick_terms.h (bicycle_se).  The pair loop, the road loop and the switch to
// agent_body<M> are second copies of small_tick_body's, marked below.
//
// Thread = (receiver, source group) as in the one-wave tick, over four waves: with P the power of two that holds the lanes - 64, 128
// or 256, never less than a wave - and G = 256 / P, thread tid has receiver i = tid & (P - 1) and source group grp = tid / P; source j
// belongs to group j % G.  Threads tid < n OWN lane tid: they stage it, add the groups' sums of it and tick it with
// agent_body<MODEL, false, true>, which holds no shuffle, ballot or LDS and so does not care which wave it runs in.
//
// What crosses waves goes through LDS between two workgroup barriers; inside the tick loop no wave reads from global memory what
// another wave has written:
//   head of tick t    hook.takeover (the owner's own slot), then every owner stages (x, y, psi, cos, sin) of its lane - its own stores of
//                     the tick before, program order -, the Bicycle field's se, and the lane's presence flag           | barrier 1
//   pair + road       every thread takes ITS RECEIVER'S (x, y, psi, cos, sin) and presence from the staging - never from d.s - and
//                     writes its group's partial sums to part[grp][i] (fp64) and rpart[grp][i] (fp32)                  | barrier 2
//   owner             adds the G partial sums of its lane in the fixed order below, ticks its lane, calls the hook (own slot only)
// The staging is renewed behind barrier 2 of the tick before and read before barrier 2 of its own tick; the partial sums are written
// behind barrier 1 and read before barrier 1 of the next tick: two barriers per tick order every LDS cell.
//
// Order of the sums (fixed, whatever the hardware does): within a group the sources in ascending j, as the one-wave tick; the groups
// pairwise, G = 4: (g0 + g1) + (g2 + g3), G = 2: g0 + g1, G = 1: g0 - for the pair term in fp64 and for the road term in fp32.  The
// one-wave tick adds its 64 / P groups pairwise by xor-shuffles; at equal G the two orders agree, but the wide P is at least 64 where
// the one-wave P is at most 32, so the two kernels differ in the order of the fp64 sums and in nothing else.
//
// BARRIERS: every __syncthreads() below is reached by all 256 threads.  n_ticks is the scene's and uniform; presence, `live`, `mine`
// and `continue` gate work, never a barrier (the rule csf_small_body.inc states for the wave barrier).  The caller returns early
// only before it calls this body.
//
// HOOK is SceneLaneHook's interface: takeover(d, t, lane) and here(t) at the head of a tick (no shuffle, ballot or barrier, stores to
// the thread's own slot only), hook(d, t, lane, n) behind it.
//
// HOOK::GROUPS (DESIGN.md 4.10h): the parts of small_tick_body of that name, all behind `if constexpr` - the source's PairConsts and field
// of view in the pair loop (LDS, indexed by the source's group: the order of a receiver's sum does not depend on the labels), hook.v_ref
// for the Bicycle se entry, and the loop over the groups around agent_body.  A lane's cell of the staged group table is written by
// hook.takeover - behind barrier 2 of the tick before, in front of barrier 1 of its own - and read in the pair loop between the two
// barriers of the tick.  The skip ballot of the group loop is per wave; groups gate work, never a barrier.
//
// MODEL == SMALL_MIXED (DESIGN.md 4.10j; csf_scene_mixed.hip: scene_wide_mixed_kernel): the parts of small_tick_body of that name, all behind
// `if constexpr (MIXED)` - `se` has a cell per lane, staged by the owners whose rider is a Bicycle (hook.own_model(), renewed by the takeover
// at the head of the tick: the model cell, se and shere are all staged between the takeover and barrier 1); a source acts with the field of
// ITS class (hook.src_model(j), LDS); and inside the per-wave loop over the groups a uniform switch on the group's class leads to
// agent_body<M>.  Classes gate work, never a barrier, and the order of a receiver's sum does not depend on them.  An instance of a real class
// is the one it was.
template <int MODEL, class HOOK>
__device__ __forceinline__ void wide_tick_body(const Dev &d, const int n_ticks, float4 *const srv, HOOK &hook) {
    __shared__ double sx[WIDE_MAX], sy[WIDE_MAX], spsi[WIDE_MAX], scs[WIDE_MAX], ssn[WIDE_MAX];
    constexpr bool MIXED = MODEL == SMALL_MIXED;
    __shared__ float2 se[MODEL == CSF_BICYCLE || MIXED ? WIDE_MAX : 1];   // Bicycle field: (e, 1 / sqrt(1 - e^2)) of every source
    __shared__ int shere[WIDE_MAX];                              // lane j holds a road user at this tick (a 64-bit ballot cannot hold 256 lanes)
    __shared__ double2 part[WIDE_MAX];                           // [G][P] the groups' partial sums of the pair term
    __shared__ float2 rpart[WIDE_MAX];                           // [G][P] ... and of the road term
    const int tid = (int)threadIdx.x;
    const int n = (int)d.n;
    int P = WAVE;
    while (P < n) P <<= 1;
    const int G = WIDE_MAX / P, i = tid & (P - 1), grp = tid / P;
    const int64_t cap = d.cap;
    const bool live = i < n;
    const PairConsts k = d.pc;
    const bool p2r = d.p.priority_rule == CSF_P2R;
    // road elements: staged once per launch.  Thread tid reads rv[tid], rv[tid + 256], ...: with road parameters per set what the same
    // thread has stored in the kernel's prologue (stride 256 there as well), program order; barrier 1 of the first tick publishes srv
    const int nvp = (int)d.nv_pad;
    for (int v = tid; v < nvp; v += WIDE_MAX) srv[v] = d.rv[v];
    for (int t = 0; t < n_ticks; t++) {
        hook.takeover(d, t, tid);
        const bool own_here = tid < n && hook.here(t);
        if (tid < n) {
            // (own stores of the previous tick or of the takeover: this thread wrote them, program order)
            const double x = d.s[tid], y = d.s[cap + tid], psi = d.s[2 * cap + tid];
            double sp, cp;
            sincos(psi, &sp, &cp);
            sx[tid] = x, sy[tid] = y, spsi[tid] = psi, scs[tid] = cp, ssn[tid] = sp;
            shere[tid] = own_here ? 1 : 0;
            bool bike = MODEL == CSF_BICYCLE;
            if constexpr (MIXED) bike = hook.own_model() == CSF_BICYCLE;   // (the class of the rider the takeover above has seated)
            if (bike) {
                double vref = d.p.v_max_riding[1];
                if constexpr (HOOK::GROUPS) vref = hook.v_ref(tid);   // (the lane's own set, as in small_tick_body)
                se[tid] = bicycle_se(d.s[3 * cap + tid], vref);
            }
        }
        __syncthreads();                                          // barrier 1: the staging of this tick is complete
        const int a = live ? i : 0;
        const bool act = live && shere[a] != 0, mine = own_here;
        const double x = sx[a], y = sy[a], psi = spsi[a];
        const double cp = scs[a], sp = ssn[a];
        const Recv r{0.f, 0.f, (float)cp, (float)sp};
        double rx = 0.0, ry = 0.0;
        // ---- TWIN COPY of the pair loop of small_tick_body (csf_small_body.inc, "for (int j = grp; ..."): the same fp64 differences,
        // the same predicates and fields, fp32 field, fp64 sum.  A change there is made here too. ----
        for (int j = grp; j < n; j += G) {                         // (threads of one group: the same j)
            const double xs = sx[j], ys = sy[j], ps = spsi[j];
            const PairConsts *kp = &k;                             // the SOURCE's field and field of view (intersection.py:733-735, 815)
            double hfov = d.p.hfov;
            if constexpr (HOOK::GROUPS) kp = hook.consts(j), hfov = hook.hfov(j);
            const PairConsts &ks = *kp;
            const double ex = x - xs, ey = y - ys;                 // vehicle.py:1615-1616
            if (shere[j] == 0) continue;                           // (a road user that is not there is nobody's source)
            // the receiver itself and a road user on the very same spot (D2) add nothing
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
        // ---- end of the TWIN COPY ----
        part[grp * P + i] = make_double2(rx, ry);
        if (nvp > 0) {
            // the road term as small_tick_body forms it (vertices as offsets from the origin of their tile of 1 024, fp32 sum), the
            // vertices of a tile shared between the groups
            // (the second copy of that loop: see the note there; a change there is made here too)
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
            rpart[grp * P + i] = make_float2(qx, qy);
        }
        __syncthreads();                                          // barrier 2: the partial sums of this tick are complete
        if (tid < n) {                                            // (tid < n: i == tid, the receiver is the thread's own lane)
            if (G == 4) {
                const double2 p0 = part[tid], p1 = part[P + tid], p2 = part[2 * P + tid], p3 = part[3 * P + tid];
                rx = (p0.x + p1.x) + (p2.x + p3.x);
                ry = (p0.y + p1.y) + (p2.y + p3.y);
            } else if (G == 2) {
                const double2 p0 = part[tid], p1 = part[P + tid];
                rx = p0.x + p1.x;
                ry = p0.y + p1.y;
            }                                                     // (G == 1: the thread's own sum)
            if (nvp > 0 && mine) {
                float2 q = rpart[tid];
                if (G == 4) {
                    const float2 q1 = rpart[P + tid], q2 = rpart[2 * P + tid], q3 = rpart[3 * P + tid];
                    q = make_float2((q.x + q1.x) + (q2.x + q3.x), (q.y + q1.y) + (q2.y + q3.y));
                } else if (G == 2) {
                    const float2 q1 = rpart[P + tid];
                    q = make_float2(q.x + q1.x, q.y + q1.y);
                }
                d.froad[tid] = q;                                 // (agent_body reads it back: the same thread, program order)
            }
            if constexpr (!HOOK::GROUPS) {
                if (mine) agent_body<MODEL, false, true>(d, PH_DEST | PH_COMBINE | PH_INTEGRATE, tid, nullptr, 0u, rx, ry, -1);
            }
        }
        if constexpr (HOOK::GROUPS) {
            // the loop over the groups of small_tick_body, per WAVE: g and the ballot are uniform in a wave, agent_body holds no barrier,
            // and a wave none of whose present owners is of group g skips the pass.  It stands outside `tid < n` - all 64 lanes of a
            // wave take the same trips - and in front of no barrier that a skipped pass could miss: the next one is barrier 1.
            Dev dg = d;
#pragma nounroll
            for (int g = 0; g < hook.n_groups; g++) {               // (the body of agent_body is emitted once, here)
                const bool turn = mine && hook.grp == g;
                if (__ballot(turn) == 0ull) continue;
                hook.select(dg, g);
                if constexpr (MIXED) {
                    constexpr int PH = PH_DEST | PH_COMBINE | PH_INTEGRATE;
                    // (the switch of small_tick_body, csf_small_body.inc - written out a third time: see the note there)
                    switch (hook.group_model(g)) {                  // (uniform: the class of the group, from its record)
                    case CSF_BICYCLE: if (turn) agent_body<CSF_BICYCLE, false, true>(dg, PH, tid, nullptr, 0u, rx, ry, -1); break;
                    case CSF_TWOD: if (turn) agent_body<CSF_TWOD, false, true>(dg, PH, tid, nullptr, 0u, rx, ry, -1); break;
                    case CSF_INVPEND: if (turn) agent_body<CSF_INVPEND, false, true>(dg, PH, tid, nullptr, 0u, rx, ry, -1); break;
                    case CSF_PLANARPOINT: if (turn) agent_body<CSF_PLANARPOINT, false, true>(dg, PH, tid, nullptr, 0u, rx, ry, -1); break;
                    case CSF_PLANARBIKE: if (turn) agent_body<CSF_PLANARBIKE, false, true>(dg, PH, tid, nullptr, 0u, rx, ry, -1); break;
                    case CSF_BALANCINGRIDER: if (turn) agent_body<CSF_BALANCINGRIDER, false, true>(dg, PH, tid, nullptr, 0u, rx, ry, -1); break;
                    default: break;                                 // (the host admits the six classes only)
                    }
                } else {
                    if (turn) agent_body<MODEL, false, true>(dg, PH_DEST | PH_COMBINE | PH_INTEGRATE, tid, nullptr, 0u, rx, ry, -1);
                }
            }
        }
        hook(d, t, tid, n);
    }
}
