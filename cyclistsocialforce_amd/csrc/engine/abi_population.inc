// engine/abi_population.inc - C ABI: road users arriving and leaving, queues, roads, parameter sets, pushed states.
// (a section of csf_engine.hip: included there, in this order; not a translation unit of its own)

// What a road user's constructor makes of vehicle.s beside it, with the limits of ITS parameter set: the state of the rider
// model's integrator and the riding / walking state (vehicle.py:1728-1736; dynamics.py:195-197, 828, 987-993).  For a
// BalancingRiderBicycle (dynamics.py:306-307, 350-371): roll, steer, their rates and the yaw in the bike model's frame
// (steer, yaw mirrored), and the speed its first gains belong to.
static void side_state(csf_engine *e, size_t a, const csf_params &p) {
    const size_t cap = (size_t)e->cap;
    const double *s = e->h_s.data() + a;
    const double delta = s[4 * cap];
    e->h_zrid[a] = s[3 * cap] < p.v_max_walk ? 0 : 1;            // vehicle.py:1732-1736
    e->h_dgood[a] = (-p.delta_max_walk < delta && p.delta_max_walk > delta) ? 1 : 0;
    if (p.model == CSF_BALANCINGRIDER) {
        e->h_lti[0 * cap + a] = s[5 * cap];
        e->h_lti[1 * cap + a] = -s[4 * cap];
        e->h_lti[2 * cap + a] = s[7 * cap];
        e->h_lti[3 * cap + a] = -s[6 * cap];
        e->h_lti[4 * cap + a] = -s[2 * cap];
        e->h_ppsi[a] = s[3 * cap];
        return;
    }
    e->h_lti[0 * cap + a] = delta;                               // vehicle.py:1728
    e->h_lti[1 * cap + a] = 0.0;
    e->h_lti[2 * cap + a] = s[5 * cap];
    e->h_lti[3 * cap + a] = 0.0;
    e->h_lti[4 * cap + a] = s[2 * cap];
    e->h_ppsi[a] = s[2 * cap];                                   // dynamics.py:828, 987-993
}

// The roster has changed (arrivals, departures - a replacement is both): a state ring begins a new stretch here, its samples of
// before are gone (include/csf.h, "the lifetime of a recording").  The ring is laid out [sample][road user] with the population
// of the tick that wrote the sample, and row i of it is road user i of THAT roster: neither survives the change.  With a ring
// the change goes through the host mirror (can_patch_device), which leaves slots == population order again (compact_host).
static void roster_changed(csf_engine *e) {
    if (e->d.hist != nullptr) e->rec_k0 = e->d.tick / e->d.hist_stride;
}

// q_off / q_rows: NULL (every new road user gets the one-row queue of vehicle.py:183-185) or the destination queues the arrivals
// START with, CSR - what csf_add_agents followed by csf_set_dest_queue(reset = 1) on the new road users leaves, in one pass
// over them (csf_replace_agents)
static int add_agents_impl(csf_engine *e, int64_t n, const double *s0, const double *v_desired, const int64_t *q_off, const double *q_rows) {
    if (!e) return CSF_E_ARG;
    if (int crc = calib_refuses(e, "csf_add_agents")) return crc;
    if (n < 0 || (n > 0 && (!s0 || !v_desired))) return fail(e, CSF_E_ARG, "csf_add_agents: bad arguments");
    int64_t q_total = 0;
    if (q_off != nullptr) {
        if (!q_rows) return fail(e, CSF_E_ARG, "csf_replace_agents: queue offsets without rows");
        for (int64_t k = 0; k < n; k++) {
            if (q_off[k + 1] <= q_off[k]) return fail(e, CSF_E_ARG, "csf_replace_agents: an arrival's destination queue must have a row");
            if (q_off[k + 1] - q_off[k] > MAX_QUEUE_ROWS) return fail(e, CSF_E_ARG, "csf_replace_agents: a destination queue of %lld rows (at most %lld)", (long long)(q_off[k + 1] - q_off[k]), (long long)MAX_QUEUE_ROWS);
        }
        q_total = n > 0 ? q_off[n] - q_off[0] : 0;
    }
    if ((int64_t)e->order.size() + n > e->cap_user) return fail(e, CSF_E_CAPACITY, "capacity %lld exceeded", (long long)e->cap_user);
    if (n == 0) return CSF_OK;
    HIPCHK(e, hipSetDevice(e->device));
    Dev &d = e->d;
    const int64_t reuse = std::min<int64_t>(n, (int64_t)(e->free_tail.size() + e->free_recent.size()));
    // collected for the device when its copy is current, the new slots have a place in the binned order (slot < n_pad)
    // and the start rows fit behind the queues already in the slab
    bool patch = can_patch_device(e) && d.n + (n - reuse) <= d.n_pad;
    if (patch && e->q_top + (int64_t)(e->pend.rows.size() / 3) + std::max(n, q_total) > d.qcap) {
        int rc = compact_slab(e, std::max(n, q_total));
        if (rc) return rc;
    }
    if (!patch) {
        int rc = prepare_mutation(e);
        if (rc) return rc;
    }
    const int ns = d.ns;
    const int64_t cap = e->cap;
    const csf_params &p = d.p;
    // first the slots (an arrival in a leaver's slot lands anywhere in the per-slot arrays of the host: asked for ahead of the
    // loop that fills them - the loop's time was cache misses, 55 us per tick with 819 arrivals), then the road users
    std::vector<int32_t> &slot_of = e->add_slots;
    slot_of.resize((size_t)n);
    const auto ta0 = std::chrono::steady_clock::now();
    int64_t ta_holes = 0;
    for (int64_t k = 0; k < n; k++) {
        int64_t a;
        bool tail = true;
        int32_t hole = -1;
        if (patch && e->tail_tracked && e->knobs.hole_reuse && !e->free_recent.empty() && holes_ready(e)) {
            if (e->time_pop) {
                const auto h0 = std::chrono::steady_clock::now();
                hole = holes_take(e, s0[k * ns], s0[k * ns + 1]);
                ta_holes += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - h0).count();
            } else {
                hole = holes_take(e, s0[k * ns], s0[k * ns + 1]);      // the slot of a road user that left from around here
            }
        }
        if (hole >= 0) {
            a = hole;
            tail = false;
            e->pend_inplace = true;                              // (the circles are renewed before the next pair launch)
            d.clist = nullptr;
        } else if (!e->free_tail.empty()) {                      // the next place of the sentinel tail
            a = e->free_tail.back();
            e->free_tail.pop_back();
        } else if (patch ? d.n < d.n_pad : e->free_recent.empty()) {   // a fresh slot: the tail continues there
            a = d.n++;
        } else if (!e->free_recent.empty()) {                    // (inside a real batch: only when nothing else is left)
            a = e->free_recent.back();
            e->free_recent.pop_back();
            e->sidx[(size_t)a].recent = -1;
            tail = false;
            e->pend_inplace = true;
            d.clist = nullptr;                                   // (a real batch's circle stretches: no candidate lists until the re-binning)
        } else {
            a = d.n++;
        }
        if (tail) e->tail_used++, e->pend_tail_spawns += patch ? 1 : 0;
        slot_of[(size_t)k] = (int32_t)a;
        __builtin_prefetch(&e->h_vdes[(size_t)a], 1);
        __builtin_prefetch(&e->h_q[(size_t)a], 1);
        __builtin_prefetch(&e->h_alive[(size_t)a], 1);
        __builtin_prefetch(&e->h_cls[(size_t)a], 1);
        __builtin_prefetch(&e->sidx[(size_t)a], 1);
    }
    const auto ta1 = std::chrono::steady_clock::now();
    for (int64_t k = 0; k < n; k++) {
        const int64_t a = slot_of[(size_t)k];
        const double *s = s0 + k * ns;
        e->h_vdes[a] = v_desired[k];
        const double *qr = q_off ? q_rows + 3 * q_off[k] : nullptr;         // its queue: given, or the start row (vehicle.py:183-185)
        const int32_t qn = q_off ? (int32_t)(q_off[k + 1] - q_off[k]) : 1;
        if (qr) e->h_q[a].assign(qr, qr + 3 * (size_t)qn);
        else e->h_q[a].assign({s[0], s[1], 0.0});
        e->h_alive[a] = 1;
        e->h_cls[a] = 0;
        e->order.push_back((int32_t)a);
        if (patch) {                                             // a record for the patch kernel, which writes the rest
            if (e->sidx[(size_t)a].retire >= 0) {             // the slot was freed in this batch: the spawn resets all of it
                const int32_t at = e->sidx[(size_t)a].retire, last = e->pend.retire.back();
                e->pend.retire[(size_t)at] = last;
                e->sidx[(size_t)last].retire = at;
                e->pend.retire.pop_back();
                e->sidx[(size_t)a].retire = -1;
            }
            drop_pending_requeue(e, (size_t)a);                  // (defensive: a retirement has dropped it already)
            SpawnRec r;
            r.slot = (int32_t)a;
            r.qlen = qn;
            r.qbeg = (int64_t)(e->pend.rows.size() / 3);
            for (int c = 0; c < STATE_ROWS; c++) r.s[c] = c < ns ? s[c] : 0.0;
            e->coord_bound0 = std::max({e->coord_bound0, std::fabs(s[0] - d.ox), std::fabs(s[1] - d.oy)});   // (set_fov_band)
            r.vdes = v_desired[k];
            r.cls = 0;
            r.pad = 0;
            if (qr) e->pend.rows.insert(e->pend.rows.end(), qr, qr + 3 * (size_t)qn);
            else e->pend.rows.insert(e->pend.rows.end(), {s[0], s[1], 0.0});
            e->sidx[(size_t)a].spawn = (int32_t)e->pend.spawn.size();
            e->pend.spawn.push_back(r);
            continue;
        }
        for (int c = 0; c < STATE_ROWS; c++) e->h_s[c * cap + a] = c < ns ? s[c] : 0.0;
        e->h_s[2 * cap + a] = limit_angle_h(s[2]);               // vehicle.py:154-155
        e->h_ptr[a] = 0;
        e->h_znav[a] = 0;                                        // vehicle.py:188
        for (int c = 0; c < 3; c++) e->h_znp[c * cap + a] = 0.0;
        e->h_ti[a] = 0;                                          // vehicle.py:146
        e->h_hx[a] = s[0];                                       // traj[:, 0] = s  (vehicle.py:159-160)
        e->h_hy[a] = s[1];
        side_state(e, (size_t)a, p);
        for (int c = 0; c < 6; c++) e->h_F[c * cap + a] = 0.0;
        e->h_status[a] = 0;
    }
    if (e->time_pop) {
        e->tp_ns[3] += std::chrono::duration_cast<std::chrono::nanoseconds>(ta1 - ta0).count();
        e->tp_ns[4] += ta_holes;
        e->tp_ns[5] += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - ta1).count();
    }
    d.n_live = (int64_t)e->order.size();
    e->order_dirty = true;
    // The candidate tile lists were built for the receiver groups and the tiles of the last re-binning: an arrival sits in the
    // sentinel tail (or a fresh slot behind it) - its group had an empty circle then and lists nothing, and groups behind
    // the old last one have no list at all.  Until the next re-binning every group walks every tile again.
    d.clist = nullptr;
    d.ccount = nullptr;
    if (!patch) {
        set_shard(e);
    } else {
        // (without the binned order a slot is its own place: the sources end with the last slot in use)
        const int64_t n_src = e->tail_tracked ? std::min(d.n_pad, (e->live_at_rebin + e->tail_used + 63) / 64 * 64)
                              : (d.classify ? d.n_pad : std::min(d.n_pad, (d.n + 63) / 64 * 64));
        if (e->segs.empty() && (n_src > d.n_src || !e->tail_tracked)) {     // (segments: the chunks are the runs', until the re-binning)
            d.n_src = std::max(n_src, d.n_src);
            set_chunks(e);
        }
    }
    roster_changed(e);
    return CSF_OK;
}

int csf_add_agents(csf_engine *e, int64_t n, const double *s0, const double *v_desired) try { return add_agents_impl(e, n, s0, v_desired, nullptr, nullptr); } catch (...) { return csf_caught(e); }

int csf_remove_agents(csf_engine *e, int64_t n, const int32_t *idx);

int csf_replace_agents(csf_engine *e, int64_t n_leave, const int32_t *idx_leave, int64_t n_arrive, const double *s0, const double *v_desired,
                       const int64_t *q_offsets, const double *q_rows) try {
    if (!e) return CSF_E_ARG;
    if (int crc = calib_refuses(e, "csf_replace_agents")) return crc;
    if (n_leave < 0 || n_arrive < 0 || (n_arrive > 0 && (!q_offsets || !q_rows))) return fail(e, CSF_E_ARG, "csf_replace_agents: bad arguments");
    if ((int64_t)e->order.size() - n_leave + n_arrive > e->cap_user) return fail(e, CSF_E_CAPACITY, "capacity %lld exceeded", (long long)e->cap_user);
    int rc = n_leave > 0 ? csf_remove_agents(e, n_leave, idx_leave) : CSF_OK;
    if (rc) return rc;
    return n_arrive > 0 ? add_agents_impl(e, n_arrive, s0, v_desired, q_offsets, q_rows) : CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_remove_agents(csf_engine *e, int64_t n, const int32_t *idx) try {
    if (!e) return CSF_E_ARG;
    if (int crc = calib_refuses(e, "csf_remove_agents")) return crc;
    if (n < 0 || (n > 0 && !idx)) return fail(e, CSF_E_ARG, "csf_remove_agents: bad arguments");
    HIPCHK(e, hipSetDevice(e->device));
    const int64_t pop = (int64_t)e->order.size();
    // The listed indices in ascending order without repeats (what a caller that walks its population produces: the mirror's
    // remove_road_users_by_id, tools/churn_rate.py): no mark array over the population, and the survivors are moved down block by
    // block - with 5 % of 16 384 road users leaving per tick the mark-and-copy loop over all of them was 40 us of every tick.
    bool ascending = true;
    for (int64_t k = 0; k < n; k++) {
        if (idx[k] < 0 || idx[k] >= pop) return fail(e, CSF_E_ARG, "agent index %d out of range", idx[k]);
        if (k > 0 && idx[k] <= idx[k - 1]) ascending = false;
    }
    if (n == 0) return CSF_OK;
    const int32_t *lst = idx;
    std::vector<int32_t> &sorted = e->remove_sorted;
    if (!ascending) {                                            // any order, repeats allowed: sorted and made unique here
        sorted.assign(idx, idx + n);
        std::sort(sorted.begin(), sorted.end());
        sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
        lst = sorted.data();
        n = (int64_t)sorted.size();
    }
    const bool patch = can_patch_device(e);
    if (patch) e->pop_calls_in_period = true;
    if (!patch) {
        int rc = prepare_mutation(e);
        if (rc) return rc;
    }
    const auto tp0 = std::chrono::steady_clock::now();
    int64_t tp_holes = 0;
    for (int64_t k = 0; k < n; k++) {
        const int32_t a = e->order[(size_t)lst[k]];
        e->h_alive[(size_t)a] = 0;
        e->h_cls[(size_t)a] = 0;                                // (a dead slot's sentinel record is looked up in set 0: the table may shrink)
        e->h_q[(size_t)a].clear();
        e->h_script[(size_t)a].clear();
        e->sidx[(size_t)a].recent = (int32_t)e->free_recent.size();
        e->free_recent.push_back(a);
        if (!patch) continue;
        if (e->tail_tracked && e->knobs.hole_reuse) {
            if (e->time_pop) {
                const auto h0 = std::chrono::steady_clock::now();
                holes_add(e, a);
                tp_holes += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - h0).count();
            } else {
                holes_add(e, a);
            }
        }
        drop_pending_requeue(e, (size_t)a);                      // a queue collected for the road user that leaves
        if (e->sidx[(size_t)a].spawn >= 0) {                  // added and removed within one batch: never reaches the device
            const int32_t at = e->sidx[(size_t)a].spawn;
            const SpawnRec last = e->pend.spawn.back();
            e->pend.spawn[(size_t)at] = last;
            e->sidx[(size_t)last.slot].spawn = at;
            e->pend.spawn.pop_back();
            e->sidx[(size_t)a].spawn = -1;
            if (!e->dev_alive[(size_t)a]) continue;              // dead on the device, or never used: nothing to undo
        }                                                        // (else: its previous occupant is still alive there)
        e->sidx[(size_t)a].retire = (int32_t)e->pend.retire.size();
        e->pend.retire.push_back(a);
    }
    const auto tp1 = std::chrono::steady_clock::now();
    {   // the remaining road users keep their relative order: the blocks between two leavers move down
        int32_t *o = e->order.data();
        int64_t w = lst[0];
        for (int64_t k = 0; k < n; k++) {
            const int64_t from = (int64_t)lst[k] + 1, to = k + 1 < n ? (int64_t)lst[k + 1] : pop;
            if (to > from) std::memmove(o + w, o + from, (size_t)(to - from) * sizeof(int32_t));
            w += to - from;
        }
        e->order.resize((size_t)w);
    }
    if (e->time_pop) {
        e->tp_ns[0] += std::chrono::duration_cast<std::chrono::nanoseconds>(tp1 - tp0).count();
        e->tp_ns[1] += tp_holes;
        e->tp_ns[2] += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - tp1).count();
        e->tp_calls++;
    }
    e->d.n_live = (int64_t)e->order.size();
    e->order_dirty = true;
    if (!patch) {                                                // the host mirror is authoritative now: close the holes
        compact_host(e);
        set_shard(e);
    }
    roster_changed(e);
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_set_dest_queue(csf_engine *e, int64_t n, const int32_t *agent, const int64_t *offsets,
                       const double *xyz_stop, int32_t reset) try {
    if (!e) return CSF_E_ARG;
    if (e->scene_calib) return calib_refuses(e, "csf_set_dest_queue");   // (the queues are part of that data set, the pointers of its image)
    if (n < 0 || (n > 0 && (!agent || !offsets || !xyz_stop))) return fail(e, CSF_E_ARG, "csf_set_dest_queue: bad arguments");
    const int64_t pop = (int64_t)e->order.size();
    // rows the slab must take: every listed queue is written out whole, as it will be after ITS entry of the call (a
    // road user listed twice in an appending call has the rows of its first entry copied again by the second)
    int64_t total = 0;
    std::unordered_map<int32_t, int64_t> grown;                  // appending call: rows of a road user after its last entry
    for (int64_t k = 0; k < n; k++) {
        if (agent[k] < 0 || agent[k] >= pop) return fail(e, CSF_E_ARG, "agent index %d out of range", agent[k]);
        if (offsets[k + 1] < offsets[k]) return fail(e, CSF_E_ARG, "offsets must be non-decreasing");
        if (reset && offsets[k + 1] == offsets[k]) return fail(e, CSF_E_ARG, "reset with an empty queue");
        int64_t rows = offsets[k + 1] - offsets[k];
        if (rows > MAX_QUEUE_ROWS) return fail(e, CSF_E_ARG, "a destination queue of %lld rows (at most %lld)", (long long)rows, (long long)MAX_QUEUE_ROWS);
        if (!reset) {
            auto it = n > 1 ? grown.find(agent[k]) : grown.end();
            rows += it != grown.end() ? it->second : (int64_t)e->h_q[(size_t)e->order[(size_t)agent[k]]].size() / 3;
            if (n > 1) grown[agent[k]] = rows;
        }
        total += rows;
    }
    if (n == 0) return CSF_OK;
    HIPCHK(e, hipSetDevice(e->device));
    // on a current device copy the new queues are appended to the slab and the slots pointed at them
    const bool patch = can_patch_device(e);
    if (patch) e->pop_calls_in_period = true;
    if (patch && e->q_top + (int64_t)(e->pend.rows.size() / 3) + total > e->d.qcap) {
        // (the queues being replaced are still counted among the live ones: room for both)
        int rc = compact_slab(e, total);
        if (rc) return rc;
    }
    if (!patch) {
        int rc = prepare_mutation(e, true);                // (a loaded calibration engine takes a route for its vehicles: abi_calib.inc)
        if (rc) return rc;
    }
    for (int64_t k = 0; k < n; k++) {
        const size_t a = (size_t)e->order[(size_t)agent[k]];
        std::vector<double> &qa = e->h_q[a];
        if (reset) {                                             // vehicle.py:642-645
            qa.clear();
            if (reset == 1) e->h_ptr[a] = 0;                     // reset == 2: rows edited in place, pointer kept
        }
        qa.insert(qa.end(), xyz_stop + 3 * offsets[k], xyz_stop + 3 * offsets[k + 1]);  // :646-647
        const int32_t nrows = (int32_t)(qa.size() / 3);
        if (e->h_ptr[a] >= nrows) e->h_ptr[a] = nrows - 1;
        if (!patch) continue;
        const int64_t at_rows = (int64_t)(e->pend.rows.size() / 3);
        e->pend.rows.insert(e->pend.rows.end(), qa.begin(), qa.end());
        if (e->sidx[a].spawn >= 0) {                          // a road user of this batch: its spawn record takes the queue
            SpawnRec &r = e->pend.spawn[(size_t)e->sidx[a].spawn];   // (a new road user's pointer is 0 either way)
            r.qbeg = at_rows;
            r.qlen = nrows;
            continue;
        }
        QueueRec r;
        r.slot = (int32_t)a;
        r.qlen = nrows;
        r.qbeg = at_rows;
        r.mode = reset;
        r.pad = 0;
        if (e->sidx[a].requeue >= 0) {                        // replaced twice in one batch: the last one counts, and a
            QueueRec &old = e->pend.requeue[(size_t)e->sidx[a].requeue];   // rewind requested by either is kept
            if (old.mode == 1) r.mode = 1;
            old = r;
        } else {
            e->sidx[a].requeue = (int32_t)e->pend.requeue.size();
            e->pend.requeue.push_back(r);
        }
    }
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_set_road_vertices(csf_engine *e, int32_t n_edges, const int64_t *offsets, const double *xy,
                          const double *F0, const double *sigma) try {
    if (!e) return CSF_E_ARG;
    if (n_edges < 0 || (n_edges > 0 && (!offsets || !xy || !F0 || !sigma)))
        return fail(e, CSF_E_ARG, "csf_set_road_vertices: bad arguments");
    for (int32_t k = 0; k < n_edges; k++)
        if (offsets[k] < 0 || offsets[k + 1] < offsets[k]) return fail(e, CSF_E_ARG, "csf_set_road_vertices: offsets[%d .. %d] run backwards", k, k + 1);
    HIPCHK(e, hipSetDevice(e->device));
    int rc = prepare_mutation(e);
    if (rc) return rc;
    e->h_road.clear();
    e->road_version++;
    for (int32_t k = 0; k < n_edges; k++)
        for (int64_t v = offsets[k]; v < offsets[k + 1]; v++) {
            e->h_road.push_back(xy[2 * v]);
            e->h_road.push_back(xy[2 * v + 1]);
            e->h_road.push_back(F0[k]);
            e->h_road.push_back(sigma[k]);
        }
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_set_incremental(csf_engine *e, int32_t on) try {
    if (!e) return CSF_E_ARG;
    if (int crc = calib_refuses(e, "csf_set_incremental")) return crc;
    e->incremental = on != 0;
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_set_params(csf_engine *e, const csf_params *params) try {
    if (!e) return CSF_E_ARG;
    if (int crc = calib_refuses(e, "csf_set_params")) return crc;
    int rc = check_params(e, params);
    if (rc) return rc;
    if (params->model != e->d.p.model) return fail(e, CSF_E_ARG, "the model of an engine cannot change");
    if (params->t_s != e->d.p.t_s || params->traj_len != e->d.p.traj_len)
        return fail(e, CSF_E_ARG, "t_s is immutable (parameters.py:516-528)");
    e->d.p = *params;
    derive_consts(e);
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_set_param_classes(csf_engine *e, int32_t n_classes, const csf_params *classes) try {
    if (!e) return CSF_E_ARG;
    if (int crc = calib_refuses(e, "csf_set_param_classes")) return crc;
    if (n_classes < 1 || n_classes > 256 || !classes) return fail(e, CSF_E_ARG, "csf_set_param_classes: 1 to 256 parameter sets");
    for (int32_t c = 0; c < n_classes; c++) {
        int rc = check_params(e, classes + c);
        if (rc) return rc;
        if (classes[c].t_s != e->d.p.t_s || classes[c].traj_len != e->d.p.traj_len)
            return fail(e, CSF_E_ARG, "parameter set %d: the vehicles of one intersection share t_s (parameters.py:516-528)", c);
    }
    for (int32_t a : e->order)
        if (e->h_cls[(size_t)a] >= n_classes)
            return fail(e, CSF_E_ARG, "a road user still uses parameter set %d", (int)e->h_cls[(size_t)a]);
    if (e->d.hist != nullptr) {                                // the history ring was sized for the present state layout
        int ns = 0;
        for (int32_t c = 0; c < n_classes; c++) ns = std::max(ns, NS_OF[classes[c].model]);
        if (ns != e->d.ns)
            return fail(e, CSF_E_STATE, "parameter sets of a wider vehicle class after csf_enable_history: install the sets first");
    }
    HIPCHK(e, hipSetDevice(e->device));
    int rc = flush_pending(e);                                 // (changes collected for the device assume one parameter set)
    if (rc) return rc;
    const int32_t rule = e->d.p.priority_rule;
    e->classes.assign(classes, classes + n_classes);
    for (csf_params &c : e->classes) c.priority_rule = rule;
    e->d.p = e->classes[0];
    derive_consts(e);
    e->ticks_since_rebin = 1 << 20;                            // binned or not may have changed: decide again (rebin)
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_set_agent_class(csf_engine *e, int64_t n, const int32_t *idx, const int32_t *cls) try {
    if (!e) return CSF_E_ARG;
    if (int crc = calib_refuses(e, "csf_set_agent_class")) return crc;
    if (n < 0 || (n > 0 && (!idx || !cls))) return fail(e, CSF_E_ARG, "csf_set_agent_class: bad arguments");
    const int64_t pop = (int64_t)e->order.size();
    for (int64_t k = 0; k < n; k++) {
        if (idx[k] < 0 || idx[k] >= pop) return fail(e, CSF_E_ARG, "agent index %d out of range", idx[k]);
        if (cls[k] < 0 || cls[k] >= (int32_t)e->classes.size())
            return fail(e, CSF_E_ARG, "parameter set %d of %d (csf_set_param_classes first)", cls[k], (int)e->classes.size());
    }
    bool device_rows_stale = false;
    for (int64_t k = 0; k < n; k++) {
        const size_t a = (size_t)e->order[(size_t)idx[k]];
        if (e->sidx[a].spawn >= 0) {                          // an arrival still on its way to the device: its spawn record
            e->pend.spawn[(size_t)e->sidx[a].spawn].cls = cls[k];   // carries the set, the patch kernel writes the row and
            e->h_cls[a] = (uint8_t)cls[k];                       // derives the start state with the set's limits
            continue;
        }
        if (e->h_cls[a] != (uint8_t)cls[k]) device_rows_stale = true;
        e->h_cls[a] = (uint8_t)cls[k];
        // A road user that has not moved yet is what its constructor made of it, with the limits of ITS set
        // (vehicle.py:1728-1736).  Only where the host mirror is the state of record: nothing collected for the device
        // (the mirror does not hold what a pending batch will write) and no tick since the last upload.
        if (!e->device_ahead && e->pend.empty() && e->h_ti[a] == 0) {
            side_state(e, a, e->classes[(size_t)cls[k]]);
            e->dirty = true;
        }
    }
    if (device_rows_stale) e->classes_dirty = true;            // (the slots' rows are uploaded with the table)
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_set_priority_rule(csf_engine *e, int32_t rule) try {
    if (!e) return CSF_E_ARG;
    if (rule < 0 || rule > 1) return fail(e, CSF_E_ARG, "unknown priority rule %d", rule);
    if (int crc = calib_refuses(e, "csf_set_priority_rule")) return crc;
    e->d.p.priority_rule = rule;
    derive_consts(e);
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_set_v_desired(csf_engine *e, int64_t n, const int32_t *idx, const double *v_desired) try {
    if (!e) return CSF_E_ARG;
    if (n < 0 || (n > 0 && (!idx || !v_desired))) return fail(e, CSF_E_ARG, "csf_set_v_desired: bad arguments");
    if (int crc = calib_refuses(e, "csf_set_v_desired")) return crc;
    for (int64_t k = 0; k < n; k++)
        if (idx[k] < 0 || idx[k] >= (int64_t)e->order.size()) return fail(e, CSF_E_ARG, "agent index %d out of range", idx[k]);
    HIPCHK(e, hipSetDevice(e->device));
    for (int64_t k = 0; k < n; k++) {
        const size_t a = (size_t)e->order[(size_t)idx[k]];
        e->h_vdes[a] = v_desired[k];
        // an arrival still on its way to the device: its spawn record carries the desired speed (the patch kernel writes
        // d.vdes[a] from it AFTER the copy below)
        if (e->sidx[a].spawn >= 0) e->pend.spawn[(size_t)e->sidx[a].spawn].vdes = v_desired[k];
    }
    if (!e->dirty) {  // device copy is current: patch it in place
        HIPCHK(e, hipStreamSynchronize(e->main));
        HIPCHK(e, hipMemcpy(e->vdes.p, e->h_vdes.data(), (size_t)e->d.n * sizeof(double), hipMemcpyHostToDevice));
    }
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_push_state(csf_engine *e, int64_t n, const int32_t *idx, const double *s) try {
    if (!e) return CSF_E_ARG;
    if (n < 0 || (n > 0 && (!idx || !s))) return fail(e, CSF_E_ARG, "csf_push_state: bad arguments");
    for (int64_t k = 0; k < n; k++)
        if (idx[k] < 0 || idx[k] >= (int64_t)e->order.size()) return fail(e, CSF_E_ARG, "agent index %d out of range", idx[k]);
    HIPCHK(e, hipSetDevice(e->device));
    int rc = prepare_mutation(e);
    if (rc) return rc;
    const int ns = e->d.ns;
    const int64_t cap = e->cap;
    for (int64_t k = 0; k < n; k++) {
        const int64_t a = e->order[(size_t)idx[k]];
        for (int c = 0; c < ns; c++) e->h_s[c * cap + a] = s[k * ns + c];
        // keep the model side-state consistent with the pushed vehicle.s
        const int model = e->classes[e->h_cls[(size_t)a]].model;
        if (model == CSF_BALANCINGRIDER) {
            // The integrator restarts from the written vehicle.s (dynamics.py:350-371; roll, steer and yaw keep the winding
            // number they have, the rates are states of vehicle.s); the speed its gains belong to stays (dynamics.py:671-673).
            // (The reference object would ignore the write: BalancingRiderDynamics.step overwrites bicycle.s from its own
            // x and v, dynamics.py:697-704.  Here a written state moves the rider, as for every other class.)
            const double twopi = 6.283185307179586476925286766559;
            auto rewind = [&](double own, double wrapped) { return wrapped + twopi * std::nearbyint((own - wrapped) / twopi); };
            double *x = e->h_lti.data() + a;
            x[0 * cap] = rewind(x[0 * cap], e->h_s[5 * cap + a]);
            x[1 * cap] = rewind(x[1 * cap], -e->h_s[4 * cap + a]);
            x[2 * cap] = e->h_s[7 * cap + a];
            x[3 * cap] = -e->h_s[6 * cap + a];
            x[4 * cap] = rewind(x[4 * cap], -e->h_s[2 * cap + a]);
        } else {
            e->h_ppsi[a] = e->h_s[2 * cap + a];
        }
        if (model == CSF_PLANARBIKE) e->h_lti[a] = e->h_s[4 * cap + a];   // dynamics.x[0] = delta
        const int slot = e->h_ti[a] & (e->d.hist_len - 1);
        e->h_hx[(size_t)slot * cap + a] = e->h_s[a];
        e->h_hy[(size_t)slot * cap + a] = e->h_s[cap + a];
    }
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_get_integrator_state(csf_engine *e, double *x, double *psi_unwrapped, uint8_t *zrid) try {
    if (!e) return CSF_E_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    int rc = upload_all(e);
    if (rc) return rc;
    rc = csf_sync(e);
    if (rc) return rc;
    const int64_t n = (int64_t)e->order.size();
    if (n == 0) return CSF_OK;
    if (x && (rc = read_rows(e, e->lti.p, 5, x, true))) return rc;
    if (psi_unwrapped && (rc = read_rows(e, e->ppsi.p, 1, psi_unwrapped, false))) return rc;
    if (zrid) {
        std::vector<uint8_t> z((size_t)n);
        if ((rc = read_rows(e, e->zrid.p, 1, z.data(), false))) return rc;
        for (int64_t a = 0; a < n; a++) {
            zrid[2 * a] = z[(size_t)a] != 0;                     // vehicle.py:1949-1950
            zrid[2 * a + 1] = z[(size_t)a] == 0;
        }
    }
    return CSF_OK;
} catch (...) { return csf_caught(e); }

int csf_set_integrator_state(csf_engine *e, int64_t n, const int32_t *idx, const double *x, const double *psi_unwrapped,
                             const uint8_t *zrid) try {
    if (!e) return CSF_E_ARG;
    if (n < 0 || (n > 0 && !idx)) return fail(e, CSF_E_ARG, "csf_set_integrator_state: bad arguments");
    for (int64_t k = 0; k < n; k++)
        if (idx[k] < 0 || idx[k] >= (int64_t)e->order.size()) return fail(e, CSF_E_ARG, "agent index %d out of range", idx[k]);
    HIPCHK(e, hipSetDevice(e->device));
    int rc = prepare_mutation(e);
    if (rc) return rc;
    const int64_t cap = e->cap;
    for (int64_t k = 0; k < n; k++) {
        const int64_t a = e->order[(size_t)idx[k]];
        if (x)
            for (int c = 0; c < 5; c++) e->h_lti[c * cap + a] = x[k * 5 + c];
        if (psi_unwrapped) e->h_ppsi[a] = psi_unwrapped[k];
        if (zrid) e->h_zrid[a] = zrid[2 * k] ? 1 : 0;
    }
    return CSF_OK;
} catch (...) { return csf_caught(e); }
