/*
 * csf.h — C ABI of the MI355X cyclist social-force stepping engine (libcsf_hip.so).
 *
 * The reference (chris-konrad/cyclistsocialforce) is pure Python and has no FFI of its own; the
 * drop-in seam is `SocialForceIntersection.step()` (intersection.py:866-896), i.e. one population
 * tick.  Each entry point below names the reference code it replaces.  The Python host
 * (cyclistsocialforce_amd/) binds these with ctypes; INTEGRATION.md shows the stub a maintainer of
 * the reference would add.
 *
 * Conventions
 *   - plain pointers and sizes only; host arrays are borrowed for the duration of a call;
 *     outputs are written into caller-allocated buffers;
 *   - every function returns 0 on success or a negative csf_status_code; the message is available
 *     from csf_last_error(engine) (or csf_last_error(NULL) when creation itself failed);
 *   - an engine is bound to one HIP device and one host thread at a time (not re-entrant);
 *   - there is NO CPU fallback: without a usable gfx950 device csf_create fails with CSF_E_DEVICE.
 */
#ifndef CSF_H
#define CSF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSF_ABI_VERSION 9

/* rider models — vehicle.py:990 (Bicycle), :1292 (TwoDBicycle), :1651 (InvPendulumBicycle),
 * :1991 (PlanarPointBicycle), :2031 (PlanarBicycle); :920 (UncontrolledVehicle: follows a prescribed trajectory
 * - csf_set_script -, exerts the TwoDBicycle field with its own parameters, feels no force) */
enum csf_model { CSF_BICYCLE = 0, CSF_TWOD = 1, CSF_INVPEND = 2, CSF_PLANARPOINT = 3, CSF_PLANARBIKE = 4, CSF_UNCONTROLLED = 5,
                 CSF_BALANCINGRIDER = 6 /* vehicle.py:1953 (BalancingRiderBicycle: 8 states - x, y, psi, v, delta, phi, deltadot, phidot) */ };

/* priority rule — intersection.py:263, 739-741 */
enum csf_priority_rule { CSF_UNREGULATED = 0, CSF_P2R = 1 };

enum csf_status_code {
    CSF_OK = 0,
    CSF_E_ARG = -1,      /* bad argument (null pointer, size, index out of range) */
    CSF_E_DEVICE = -2,   /* no usable HIP device / HIP runtime error */
    CSF_E_CAPACITY = -3, /* more agents than the engine was created for */
    CSF_E_STATE = -4,    /* call not valid in the current engine state */
    CSF_E_COMM = -5,     /* RCCL error */
    CSF_E_ABI = -6,      /* the caller's csf_params (size) or ABI version is not this library's: csf_create_v */
    CSF_E_HOST = -7      /* the host ran out of memory (or another C++ exception was caught at the boundary: none crosses it);
                          * the engine is good for csf_last_error and csf_destroy only */
};

/* per-agent status bits reported by csf_status() (reference: exceptions / prints) */
#define CSF_ST_SPLINE 1u   /* vehicle.py:1495-1507: splprep would raise on duplicate points */
#define CSF_ST_NAN 2u      /* a force became non-finite (vehicle.py:1180-1185 "Isnan!") */
#define CSF_ST_NAVSTATE 4u /* vehicle.py:416-425: navigation state not one-hot */
#define CSF_ST_UNCONTROLLABLE 8u /* dynamics.py:1212-1214: PlanarBicycle at v <= 0 ("System not controllable!") */

/* POD mirror of the reference's parameter objects (parameters.py).  One set per engine = per vehicle
 * class; v_desired_default is per agent (csf_add_agents), whole parameter sets per agent: csf_set_param_classes.
 * Field order is ABI. */
typedef struct csf_params {
    /* VehicleParameters — parameters.py:430-508 */
    double t_s, d_arrived_inter, d_arrived_stop, v_max_stop, v_max_harddecel, hfov;
    double f_0, e_0, e_1, sigma_0, sigma_1, sigma_2, sigma_3;
    /* BicycleParameters — parameters.py:780-800 */
    double v_max_riding[2], p_decay, p_0, l, l_2, delta_max, a_max[2], a_desired_default[2];
    double k_p_v, k_p_delta, g;
    /* InvPendulumBicycleParameters — parameters.py:1429-1472 */
    double h, m, i_bike_longlong, i_steer_vertvert, c_steer, v_max_walk, delta_max_walk;
    /* PlanarPointBicycleParameters — parameters.py:1180-1201 (gain = -Re(pole), dynamics.py:933-940) */
    double k_psi;
    /* PlanarBicycleParameters — parameters.py:1203-1211: the two desired poles of the steer / yaw loop (re, im, re, im) */
    double pb_poles[4];
    /* BalancingRiderBicycleParameters — parameters.py:1214-1411; dynamics.py:261-705 (ABI 8).  The linearised Whipple-Carvallo
     * bicycle (Meijaard, Papadopoulos, Ruina & Schwab 2007: M q'' + v C1 q' + (g K0 + v^2 K2) q = f, q = (roll, steer)) as the
     * 2 x 2 blocks of its state matrix (row-major: M^-1 g K0, M^-1 K2, M^-1 C1), the steer-torque column of M^-1, the yaw row
     * (cos(lam) / w, cos(lam) c / w: dynamics.py:301-303), and the control model: the desired closed-loop poles as straight
     * lines over speed - (intercept, slope) of p0_real, p1_real, p1_imag, p2_real, p2_imag (parameters.py:1400-1409; fixed
     * poles: slopes 0) -, or fixed gains (br_mode 2: dynamics.py:604-605) */
    double br_minv_k0g[4], br_minv_k2[4], br_minv_c1[4], br_minv_steer[2], br_yaw[2], br_pole_fun[10], br_gains[5];
    int32_t model;         /* enum csf_model */
    int32_t priority_rule; /* enum csf_priority_rule */
    int32_t traj_len;      /* columns of the reference's traj ring buffer, int(30 / t_s) — vehicle.py:159 */
    int32_t br_mode;       /* BalancingRider: 0 poles from br_pole_fun at the current speed, 2 the gains br_gains */
} csf_params;

typedef struct csf_engine csf_engine;

/* ---- lifetime -------------------------------------------------------------------------------- */

/* SocialForceIntersection.__init__ (intersection.py:259-330): an empty population of one vehicle
 * class on HIP device `device`.  `n_capacity` bounds the number of agents.  Returns NULL on failure. */
csf_engine *csf_create(const csf_params *params, int64_t n_capacity, int32_t device);
/* The same for a caller that is NOT compiled against this header (ABI 9) - a ctypes / cffi binding declares csf_params by hand,
 * and a struct that has fallen behind the header (members were inserted in ABI 8) would make csf_create read `model` from
 * whatever lies behind the caller's memory.  csf_create_v refuses - NULL, csf_last_error(NULL) names both figures, nothing is
 * read from `params` - unless params_size == csf_params_size() and abi_version == csf_abi_version().  Bindings call this one;
 * csf_params_size() is what sizeof(csf_params) was when the library was built. */
csf_engine *csf_create_v(const csf_params *params, size_t params_size, int32_t abi_version, int64_t n_capacity, int32_t device);
size_t csf_params_size(void);
int csf_destroy(csf_engine *e);
const char *csf_last_error(const csf_engine *e);
int32_t csf_abi_version(void);

/* ---- population ------------------------------------------------------------------------------ */

/* Vehicle.__init__ (vehicle.py:64-204) for n agents at once: s0 is [n, n_states] row-major
 * (n_states = 5, 5, 6, 4, 5 by model), v_desired is [n].  Every new agent gets the single-row
 * destination queue (x0, y0, 0) of vehicle.py:183-185.  add_road_user: intersection.py:458-539. */
int csf_add_agents(csf_engine *e, int64_t n, const double *s0, const double *v_desired);

/* remove_road_user / remove_road_users_by_id (intersection.py:576-634): indices into the current
 * population, any order; the remaining agents keep their relative order. */
int csf_remove_agents(csf_engine *e, int64_t n, const int32_t *idx);

/* One traffic step in one call (ABI 9): the listed road users leave (as csf_remove_agents), n_arrive new ones join behind the remaining
 * ones (as csf_add_agents) and START with the given destination queues (CSR, at least one row each: what csf_set_dest_queue with
 * reset = 1 on the new road users would leave) - what SUMO co-simulation does every step (scenario.py:376-466: find_entered_exited,
 * remove_road_users_by_id, add_road_user + its route).  The same population and order as the three calls; one pass over the arrivals
 * instead of two, no start-row queue that is replaced at once. */
int csf_replace_agents(csf_engine *e, int64_t n_leave, const int32_t *idx_leave, int64_t n_arrive, const double *s0, const double *v_desired,
                       const int64_t *q_offsets, const double *q_rows);

/* How csf_add_agents / csf_remove_agents / csf_set_dest_queue reach the device once ticks have run (the per-tick arrivals
 * and departures of SUMO co-simulation, intersection.py:429-453, 458-634; scenario.py:376-466).  on != 0 (default): the
 * calls only record what to do, and the next device call applies the batch with one small launch - a removed road user
 * leaves a dead slot with a sentinel record, a new one takes a free slot whose place in the binned order lies in the tail
 * of sentinels behind the sorted batches, a replaced queue is appended to the queue slab (rewritten from the host's copy of
 * the queues when full); no download, no upload; the binned order is renewed when ticks x arrivals since the last renewal
 * reaches a few thousand.  The capacity holds up to 4096 extra slots for this.  on == 0: every change goes through the host
 * mirror (download, edit, upload, re-sort), which is also what sharded engines and engines with the history ring do.
 * The population order seen by every other entry point is the same either way.
 * On a sharded run (csf_comm_init) the population calls, csf_push_state and csf_set_integrator_state are COLLECTIVE: every rank
 * makes the same calls in the same order; before the first change after a tick the ranks exchange the fp64 state of their blocks
 * (a rank integrates only its own: one all-gather per state array on packed blocks), and the next tick starts from the upload with
 * new shard bounds.  The contract is the collective's: a call that only SOME ranks make blocks those ranks inside the exchange until
 * the others make it too - guard rank-dependent edits (e.g. a conditional push of vehicle.s) with the same condition on every rank. */
int csf_set_incremental(csf_engine *e, int32_t on);

/* Vehicle.setDestinations (vehicle.py:606-647) for n agents: CSR (offsets[n+1], xyz_stop[sum,3]);
 * reset = 0 appends to the agent's queue, reset = 1 replaces it and rewinds the pointer, reset = 2 replaces
 * it and keeps the pointer (rows edited in place: Vehicle.stop / Vehicle.go set the stop flag of the current
 * destination, vehicle.py:459-535). */
int csf_set_dest_queue(csf_engine *e, int64_t n, const int32_t *agent, const int64_t *offsets,
                       const double *xyz_stop, int32_t reset);

/* RoadEdge objects (intersection.py:214-242) flattened: CSR over vertices, one (F0, sigma) per edge. */
int csf_set_road_vertices(csf_engine *e, int32_t n_edges, const int64_t *offsets, const double *xy,
                          const double *F0, const double *sigma);

int csf_set_params(csf_engine *e, const csf_params *params);           /* parameter mutation between ticks */

/* Every reference vehicle owns its params object (vehicle.py:64-204): the field vehicle i exerts is evaluated with ITS
 * f_0 / sigma_* / e_* (vehicle.py:1592-1612; p_0 / p_decay for the Bicycle field, :1095-1101) and masked with ITS hfov
 * (intersection.py:733-735), and it steers, accelerates, brakes and arrives with its own gains and limits.
 * csf_set_param_classes installs 1 to 256 parameter sets (same t_s and traj_len as the engine; set 0 replaces the
 * engine's own, the priority rule stays the intersection's); csf_set_agent_class assigns sets to road users (new road
 * users start in set 0; a road user that has not taken a tick yet is re-initialised as the constructor of its set's
 * class would, vehicle.py:1728-1736).  The sets may be of different vehicle CLASSES (intersection.py:797-823 calls each
 * vehicle's own methods, so any mix may share an intersection): every row of s0 / csf_get_state then has the widest
 * layout among them (csf_num_states; states a class does not have stay 0), so install the sets before csf_add_agents.
 * With more than one set the engine evaluates the pair term either with a plain O(N^2) kernel that looks every source's
 * set up, or - from about 2048 road users per set, up to 16 sets, unsharded - with one launch of its culling kernel per
 * set over that set's run of the binned order.
 * An arrival whose set is assigned before the next device call (csf_add_agents, then csf_set_agent_class) takes it along in
 * its spawn record. */
int csf_set_param_classes(csf_engine *e, int32_t n_classes, const csf_params *classes);
int csf_set_agent_class(csf_engine *e, int64_t n, const int32_t *idx, const int32_t *cls);
int csf_set_v_desired(csf_engine *e, int64_t n, const int32_t *idx, const double *v_desired);
int csf_set_priority_rule(csf_engine *e, int32_t rule);                /* intersection.py:324 */

/* host-side mutation of vehicle.s between ticks (calibration.py:455-460): s is [n, n_states] */
int csf_push_state(csf_engine *e, int64_t n, const int32_t *idx, const double *s);

/* The hidden state of the rider models' integrators, which vehicle.s does not carry (ABI 7): x [n, 5] = vehicle.x of an
 * InvPendulumBicycle (vehicle.py:1728-1733, 1843: delta, ddelta, theta, dtheta, psi - the yaw UNWRAPPED, which is what the
 * commanded yaw arctan2(Fy, Fx) of vehicle.py:1832 is compared with), for PlanarBicycle x[., 0] = dynamics.x[0] (delta,
 * dynamics.py:195-197); psi_unwrapped [n] = the yaw state of the PlanarPoint / PlanarBicycle integrators (dynamics.py:828,
 * 943-966, 987-993); zrid [n, 2] = vehicle.zrid, one-hot riding / walking (vehicle.py:1735-1736, 1932-1950).  Any pointer
 * may be NULL.  csf_push_state replaces vehicle.s only (calibration.py:455-460 does the same to the reference object); a
 * caller that moves a population from one engine - or from the reference - to another needs these as well. */
int csf_get_integrator_state(csf_engine *e, double *x, double *psi_unwrapped, uint8_t *zrid);
int csf_set_integrator_state(csf_engine *e, int64_t n, const int32_t *idx, const double *x, const double *psi_unwrapped,
                             const uint8_t *zrid);

int64_t csf_num_agents(const csf_engine *e);
int32_t csf_num_states(const csf_engine *e);

/* ---- the hot call ---------------------------------------------------------------------------- */

/* n_ticks x SocialForceIntersection.step() (intersection.py:866-896): FOV mask + all-pairs repulsive
 * field + column sum + clamp (:690-845), destination force (vehicle.py:1416-1558), road edges
 * (:853-857), controller + kinematics (vehicle.py:1218-1272, 1810-1950; dynamics.py:996-1079) and the
 * position snapshot (:660-677).  Asynchronous: returns once the work is enqueued; csf_sync waits. */
int csf_step(csf_engine *e, int64_t n_ticks);
int csf_sync(csf_engine *e);

/* calc_forces() alone (intersection.py:747-864): forces of the next tick from the current snapshot.
 * Like the reference it advances the destination queue / navigation state of every agent. */
int csf_calc_forces(csf_engine *e);
/* vehicle.step(Fx, Fy) for every agent with caller-supplied forces (calibration.py:438-460 replay,
 * intersection.py:891-894).  Fx, Fy are [n]. */
int csf_apply_forces(csf_engine *e, const double *Fx, const double *Fy);
/* Calibration replay (calibration.py:438-460): n_ticks x vehicle.step(Fx[t][a], Fy[t][a]) for every agent with
 * recorded forces, in one call.  Fx, Fy are [n_ticks, n] row-major.  lengths is [n] or NULL: agent a is stepped
 * for its first lengths[a] ticks only (sequences of different length).  fix_speed != 0 sets v = |F| before every
 * step (calibration.py:454-458).  states_out is NULL or [n_ticks / stride, n, n_states]: the state after ticks
 * stride, 2*stride, ...  (vehicle.traj).  Single-device entry point. */
int csf_replay_forces(csf_engine *e, int64_t n_ticks, const double *Fx, const double *Fy, const int32_t *lengths,
                      int32_t fix_speed, int32_t stride, double *states_out);
/* calcDestinationForce() of every agent (vehicle.py:1189-1194, 1416-1558); mutates queue pointer and
 * navigation state exactly like the reference does. */
int csf_dest_force(csf_engine *e, double *Fx, double *Fy);

/* ---- read-back (all synchronise first) -------------------------------------------------------- */

/* s_out [n, n_states]; dest_ptr [n] (destpointer), znav [n,3] one-hot, tick = ticks since creation.
 * Any output pointer may be NULL. */
int csf_get_state(csf_engine *e, double *s_out, int32_t *dest_ptr, uint8_t *znav, int64_t *tick);
/* Everything the host mirror of SocialForceIntersection.step() refreshes after a tick (intersection.py:860-862,
 * 660-677; vehicle.py:1279-1282), in ONE device-to-host transfer: csf_get_state + csf_get_forces cost nine separate
 * copies of ~12 us each, which dominated the per-tick call at the reference's own population sizes (3 - 30
 * cyclists).  A kernel packs the row-major state, destination pointers, navigation state and total forces into a
 * pinned staging buffer; any output pointer may be NULL. */
int csf_get_tick(csf_engine *e, double *s_out, int32_t *dest_ptr, uint8_t *znav, double *Fx, double *Fy,
                 int64_t *tick);
/* total force of the last evaluated tick (vehicle.force, intersection.py:860-861) */
int csf_get_forces(csf_engine *e, double *Fx, double *Fy);
/* parts of it: destination force and clamped repulsive sum (before road edges) */
int csf_get_force_parts(csf_engine *e, double *Fdest_x, double *Fdest_y, double *Frep_x, double *Frep_y);
int csf_status(csf_engine *e, uint32_t *per_agent_flags);

/* opt-in history (vehicle.traj, vehicle.py:159, 1407-1410): record every `stride`-th tick into a
 * device ring of `capacity` samples; csf_get_history copies samples [first, first+n) (sample k = state
 * after tick (k+1)*stride) of all agents into out [n_samples, n_agents, n_states]. */
int csf_enable_history(csf_engine *e, int32_t stride, int32_t capacity);
int csf_get_history(csf_engine *e, int64_t first_sample, int64_t n_samples, double *out);
/* An engine with csf_enable_history is ticked by the general path (two launches per tick, or one for a mid-size population), and
 * inside a batch by csf_step in turn.  csf_record is the recording that keeps the fast paths: the same state ring (same layout,
 * same sample numbering, csf_get_history reads it) and, with CSF_REC_FORCE, a second ring [capacity][n_agents][2] of the total
 * force (Fx, Fy as csf_get_forces returns them after the sampled tick) - written by whatever kernel ticks the engine, the
 * one-wave kernel and the batched launch of csf_step_batch included (see csf_small_ticks).  The state ring is always kept.
 * Calling either again starts a new ring; the later call decides which path the engine takes.
 *
 * The lifetime of a recording.  A state ring has a FIRST VALID SAMPLE k0, and every reader of the ring refuses what lies before it:
 *  - csf_record / csf_enable_history called at tick T with stride s set k0 = T / s (integer division): sample k is the state after
 *    tick (k + 1) * s, so k >= T / s are exactly the samples written into this ring.  A ring begun at tick 0 has k0 = 0.
 *  - Every call that changes the roster sets k0 = tick / stride at that moment: csf_add_agents with n > 0, csf_remove_agents with
 *    n > 0, csf_replace_agents with anybody leaving or arriving (also one for one: row i of a sample is road user i of the roster
 *    of ITS tick).  A change of the roster starts a new stretch of the recording; the samples of the stretch before are gone - the
 *    ring is not re-allocated, and sample numbers go on counting from tick 0.  A refused population call changes nothing, k0 included.
 *  - csf_push_state, parameter, parameter-set, queue, script and desired-speed calls leave k0 alone.
 *  - Readers are csf_get_history, csf_get_record, csf_batch_get_record, csf_encounters (with a window), csf_post_encroachment,
 *    csf_passing, csf_flow and their csf_batch_* forms.  first_sample < k0 - for the batch forms n_last > tick / stride - k0 of a
 *    member - is CSF_E_ARG, "samples [a, b) are not in the ring (have h, capacity c, first readable sample r)", like a sample the
 *    ring has overwritten or not yet taken (r = max(k0, h - c)), and before anything is written, launched or counted.
 *
 * csf_get_record: samples [first_sample, first_sample + n_samples) as s_out [n_samples, n_agents, n_states] and F_out
 * [n_samples, n_agents, 2]; one of the two may be NULL.  One gather launch and one wait, whatever n_samples is. */
#define CSF_REC_STATE 1u
#define CSF_REC_FORCE 2u
int csf_record(csf_engine *e, int32_t stride, int32_t capacity, uint32_t what);
int csf_get_record(csf_engine *e, int64_t first_sample, int64_t n_samples, double *s_out, double *F_out);

/* ---- force-field maps ----------------------------------------------------------------------------- */

/* The force field at m arbitrary probe points (x, y, psi [m]; scenarios/curve-scenario.py:90-125): what a road user would
 * feel there.  `what` names the terms; with both, Fx, Fy = crowd + road, added in fp64.  Every pair is evaluated - no
 * far-field cull.  psi may be NULL only without CSF_FIELD_CROWD (it enters the TwoD field itself, vehicle.py:1595).  skip: -1,
 * or a road user (population order) that is left out as a source - what THAT road user would feel elsewhere.  One launch per
 * requested term whatever m is (csf_field_map_launches counts them); pending uploads are brought in, the engine's work is
 * waited for, and the engine is left exactly as it was.  An empty population / no road gives zeros; a probe with a
 * non-finite coordinate gets NaN, the others are not affected.  Refused (CSF_E_ARG / CSF_E_STATE, nothing changed): NULL
 * arrays, m < 0, what == 0 or unknown bits, FOV without CROWD, skip out of range, a rank of a sharded run or a member of a
 * loopback group, an engine that holds a calibration data set.  While csf_profile_enable is on, the crowd launch is timed as
 * kernel 0 and the road launch as kernel 1 of csf_profile_kernels / csf_profile_samples_of. */
#define CSF_FIELD_CROWD 1u   /* sum of the live road users' fields (each its class's field, its own parameter set), unclamped */
#define CSF_FIELD_ROAD  2u   /* road-edge term of csf_set_road_vertices */
#define CSF_FIELD_FOV   4u   /* with CROWD: the probe is a receiver of heading psi - field-of-view mask and priority rule applied */
int csf_field_map(csf_engine *e, int64_t m, const double *x, const double *y, const double *psi,
                  uint32_t what, int32_t skip, double *Fx, double *Fy);
int csf_field_map_launches(const csf_engine *e, int64_t *n_launches);

/* ---- encounters: proximity and time to collision of a recording ---------------------------------- */

/* How close the road users came, to whom and when, and how many seconds from a collision they were - formed on the device from
 * the state ring that csf_record / csf_enable_history keep, or from the current state.
 *
 * For one sample and road user i, take its position p_i = (x, y), heading psi and speed v from rows 0-3 of its state, as
 * csf_get_state returns them. Its velocity is u_i = v_i (cos psi_i, sin psi_i). Every road user is a disc of the call's `radius`,
 * and R = 2 radius.
 *
 * For j != i, let w = p_j - p_i and c = u_j - u_i. Let a = c.c, b = w.c and q = w.w - R^2.
 *
 * - d_ij = sqrt(w.w).
 * - ttc_ij is the time to collision at constant velocity. It takes four cases:
 *   - If q <= 0 the discs overlap now, and ttc_ij is 0.
 *   - Otherwise, if b >= 0 or a == 0 or b^2 - a q < 0, the discs never meet, and ttc_ij is +inf.
 *   - Otherwise ttc_ij is q / (-b + sqrt(b^2 - a q)). This is the root written without cancellation. Use this form, not
 *     (-b - sqrt)/a.
 * - Per (sample, i), report four values:
 *   - d_min = min_j d_ij.
 *   - d_with = the j that gives it.
 *   - ttc_min = min_j ttc_ij.
 *   - ttc_with = the j that gives it, or -1 when ttc_min is +inf.
 * - Ties go to the lowest j. A strict < in population order gives this.
 * - All of this is computed in fp64 from the fp64 ring. It is a diagnostic with exact yes/no cases, and CDNA4 runs vector fp64
 *   at half the fp32 rate. The implementation uses no fp32 and no fast-math functions.
 * - d_ij and ttc_ij are bitwise symmetric in (i, j), because negating w and c is exact. Rely on that for the events below.
 * - A road user with a non-finite x, y, psi or v in a sample is neither receiver nor partner in that sample.
 *   - Its own row is NaN / -1.
 *   - Nobody else's row is affected.
 * - A population of one gives +inf / -1.
 *
 * Over the window of a call, per road user, report the minimum d_min and the minimum ttc_min. With each go its partner and the
 * absolute sample index at which it occurred. On ties the earliest sample wins.  (A minimum of +inf - nobody else in any sample,
 * or no course that meets - has partner -1 and sample -1; the current state counts as sample -1.)
 *
 * Events are optional. An event is a (sample, i < j) with d_ij < d_event or ttc_ij < ttc_event. It is stored as
 * {int64 sample; int32 i, j; double d, ttc;}. Either threshold may be <= 0 to switch it off.
 *
 * The caller gives a capacity. The call always returns the total number found. It stores at most `capacity` events. When
 * total <= capacity it returns them sorted by (sample, i, j), so the result is deterministic although slots are handed out by
 * atomics. When total > capacity the stored subset is unspecified. */
typedef struct csf_encounter_event {
    int64_t sample;
    int32_t i, j;
    double d, ttc;
} csf_encounter_event;
/* Where the results of one engine go; any pointer may be NULL (that array is not returned).  n = the road users, n_samples the
 * samples the call covers.  event_capacity = 0 with events NULL counts the events without storing any. */
typedef struct csf_encounter_out {
    double *d_min;            /* [n_samples, n] */
    int32_t *d_with;          /* [n_samples, n] */
    double *ttc_min;          /* [n_samples, n] */
    int32_t *ttc_with;        /* [n_samples, n] */
    double *run_d_min;        /* [n] the window's minima ... */
    int32_t *run_d_with;      /* [n] ... the partner ... */
    int64_t *run_d_sample;    /* [n] ... and the sample of each */
    double *run_ttc_min;      /* [n] */
    int32_t *run_ttc_with;    /* [n] */
    int64_t *run_ttc_sample;  /* [n] */
    csf_encounter_event *events;  /* [event_capacity] */
    int64_t event_capacity;
    int64_t n_events;         /* written: the events found, stored or not */
    int64_t first_sample;     /* written: the index of the first sample covered (-1: the current state) */
} csf_encounter_out;
/* Samples [first_sample, first_sample + n_samples) of the engine's state ring, numbered and range-checked as csf_get_record has
 * them (not before the ring's first valid sample: "the lifetime of a recording" at csf_record); with first_sample == -1 and n_samples == 1 the current state (no ring needed, population order).  Pending uploads are
 * brought in, both streams are waited for as the read-backs do, and the engine is left exactly as it was.  Two launches whatever
 * the sizes are - every pair of every sample, then the window's minima over the per-sample arrays - with one transfer and one wait
 * (the launch counter below grows by 2 per call that covers anything).  An empty population or n_samples == 0
 * succeeds with n_events = 0.  Refused without side effects (CSF_E_ARG / CSF_E_STATE, with a message): a NULL out; a negative or
 * non-finite radius; n_samples < 0 or above 65535; samples that are not in the ring; no ring when a window is asked for; a
 * negative event capacity, or a capacity with a NULL buffer; a rank of a sharded run or a member of a loopback group; an engine
 * that holds a calibration data set.  While csf_profile_enable is on, the first launch is timed as kernel 0. */
int csf_encounters(csf_engine *e, int64_t first_sample, int64_t n_samples, double radius, double d_event, double ttc_event,
                   csf_encounter_out *out);
/* The last n_last samples of every member of a batch (in join order) that records, all members in the same two launches, with one
 * transfer and one wait; outs [count].  A member without a ring is skipped: its n_events becomes 0 and its first_sample -2.  A
 * recording member with fewer than n_last samples in its ring makes the call a refusal before anything is written. */
int csf_batch_encounters(csf_engine *const *engines, int32_t count, int64_t n_last, double radius, double d_event, double ttc_event,
                         csf_encounter_out *outs);
/* launches of the two calls above so far (a batch counts on its first member) */
int csf_encounter_launches(const csf_engine *e, int64_t *n_launches);

/* ---- post-encroachment time: path crossings of a recording --------------------------------------- */

/* Who crossed whose path, where, and how long after the other had passed - formed on the device from the state ring that
 * csf_record / csf_enable_history keep.
 *
 * A call covers samples [first_sample, first_sample + c) of the state ring. Number them k = 0 ... c-1 inside the call, and let
 * m = c - 1.
 *
 * Segments.
 * - P_i(k) = (x, y) is rows 0 and 1 of road user i's state in sample k, the fp64 bits of the ring.
 * - Segment (i, k), for k = 0 ... m-1, runs from A = P_i(k) to B = P_i(k+1), with r = B - A.
 * - A segment exists if all four coordinates are finite.
 * - psi and v are not read.
 *
 * Terms of one pair. Take own segment (i, k) with A, r and partner segment (j, l), j != i, with C = P_j(l), s = P_j(l+1) - C.
 * Both must exist. Let w = C - A.
 * - den = r.x*s.y - r.y*s.x
 * - ns = w.x*s.y - w.y*s.x
 * - nt = w.x*r.y - w.y*r.x
 * - Each term is two products and one subtraction in fp64. None is contracted to an FMA (#pragma clang fp contract(off), as in
 *   csf_encounter.hip). No fp32 and no fast-math functions are used.
 *
 * Box test. The closed bounding boxes of the two segments overlap. Each box is the min and max of its two endpoints, compared
 * with >= / <= in x and in y.
 *
 * inside(num).
 * - If den > 0, it is 0 <= num && num < den.
 * - If den < 0, it is den < num && num <= 0.
 * - If den == 0 (parallel, collinear, or a stationary road user), it is false.
 *
 * Crossing. The paths cross on this pair iff the boxes overlap and inside(ns) and inside(nt).
 * - The decision is made from num and den, never from a quotient.
 * - The intervals are half open, so a crossing through a shared vertex counts on exactly one segment of each path.
 * - The box test is part of the definition. Any coarser cull by boxes over these boxes is therefore exact.
 *
 * Values of a crossing.
 * - s_own = ns / den and s_with = nt / den. Either may round to 1.0.
 * - t_own = (double)k + s_own and t_with = (double)l + s_with, in samples from the first sample of the call.
 * - pet = fabs(t_with - t_own).
 * - x = A.x + s_own * r.x and y = A.y + s_own * r.y, each a product and then a sum.
 *
 * Symmetry. Seen from (j, l), den, ns and nt are the exact negatives with the roles swapped. So the decision, both times and
 * pet are bitwise symmetric in (i, j). The point is taken on the own segment of whoever reports it, and may differ in the last
 * bit.
 *
 * Per own segment (k, i).
 * - seg_pet is the minimum pet over all (j, l).
 * - With it go seg_with (the j), seg_t_own and seg_t_with.
 * - Ties go to the lowest j, then the lowest l. A strict < in that loop order gives this.
 * - No crossing gives +inf / -1 / NaN / NaN.
 * - An own segment that does not exist gives NaN / -1 / NaN / NaN and is nobody's partner. Nobody else's row changes.
 *
 * Per road user over the call.
 * - run_pet is the minimum seg_pet over k, the earliest k on ties.
 * - With it go run_with, run_t_own, run_t_with, run_x, run_y.
 * - run_count (int32) is the number of crossings (k, j, l) on the road user's path.
 * - No crossing gives +inf / -1 / NaN ... / 0.
 *
 * Events.
 * - Events are optional (pet_event > 0; +inf is allowed and means every crossing).
 * - An event is a crossing with i < j and pet < pet_event.
 * - It is stored as {int32 i, j, k, l; double t_i, t_j, x, y;}: 48 bytes, point and times as i reports them, k and l counted
 *   from the call's first sample.
 * - Capacity, total count, "sorted by (i, j, k, l) when total <= capacity, unspecified subset otherwise" are exactly as for
 *   csf_encounter_event.
 *
 * Small calls. n_samples < 2, or a population of one, succeeds with nothing found. */
typedef struct csf_pet_event {
    int32_t i, j, k, l;
    double t_i, t_j, x, y;
} csf_pet_event;
/* Where the results of one engine go; any pointer may be NULL (that array is not returned).  n = the road users, n_samples the
 * samples the call covers.  event_capacity = 0 with events NULL counts the events without storing any.  With n_samples < 2 the
 * seg_* arrays have no rows and run_* are written as "no crossing". */
typedef struct csf_pet_out {
    double *seg_pet;          /* [n_samples-1, n] */
    int32_t *seg_with;        /* [n_samples-1, n] */
    double *seg_t_own;        /* [n_samples-1, n] */
    double *seg_t_with;       /* [n_samples-1, n] */
    double *run_pet;          /* [n] the smallest seg_pet ... */
    int32_t *run_with;        /* [n] ... whose path was crossed ... */
    double *run_t_own;        /* [n] ... when the road user was there ... */
    double *run_t_with;       /* [n] ... when the other was ... */
    double *run_x;            /* [n] ... and where */
    double *run_y;            /* [n] */
    int32_t *run_count;       /* [n] crossings on the road user's path */
    csf_pet_event *events;    /* [event_capacity] */
    int64_t event_capacity;
    int64_t n_events;         /* written: the events found, stored or not */
    int64_t first_sample;     /* written: the index of the first sample covered */
} csf_pet_out;
/* Samples [first_sample, first_sample + n_samples) of the engine's state ring, numbered and range-checked as csf_get_record has
 * them (not before the ring's first valid sample: "the lifetime of a recording" at csf_record), on rings of csf_record and csf_enable_history alike.  Pending uploads are brought in, both streams are waited for as the
 * read-backs do, and the engine is left exactly as it was.  TWO launches whatever the sizes are - every pair of segments, then
 * the per-segment and per-road-user minima - with one hipMemsetAsync of the event counters, one transfer and one wait (the launch
 * counter below grows by 2 per call that covers a segment).  Refused without side effects (CSF_E_ARG / CSF_E_STATE, with a
 * message, launch counter unchanged): a NULL out; first_sample == -1 (the current state has no path) or no ring; n_samples < 0 or
 * above 65535; samples that are not in the ring; a NaN or -inf pet_event; a negative event capacity, or a capacity with a NULL
 * buffer; a rank of a sharded run or a member of a loopback group; an engine that holds a calibration data set.  While
 * csf_profile_enable is on, the first launch is timed as kernel 0. */
int csf_post_encroachment(csf_engine *e, int64_t first_sample, int64_t n_samples, double pet_event, csf_pet_out *out);
/* The last n_last samples of every member of a batch (in join order) that records, all members in the same two launches, with one
 * transfer and one wait; outs [count].  A member without a ring is skipped: its n_events becomes 0 and its first_sample -2.  A
 * recording member with fewer than n_last samples in its ring makes the call a refusal before anything is written. */
int csf_batch_post_encroachment(csf_engine *const *engines, int32_t count, int64_t n_last, double pet_event, csf_pet_out *outs);
/* launches of the two calls above so far (a batch counts on its first member) */
int csf_pet_launches(const csf_engine *e, int64_t *n_launches);

/* ---- following and passing: gaps, overtakings and meetings of a recording ------------------------ */

/* Who rode behind whom, at what gap and time headway, and who overtook or met whom, when, and with how much lateral clearance -
 * formed on the device from the state ring that csf_record / csf_enable_history keep.
 *
 * A call covers samples [first_sample, first_sample + c) of the state ring, numbered k = 0 ... c-1 inside the call. P_i(k) = (x, y)
 * are the fp64 bits of the ring.
 *
 * Stations.
 * - Station (i, k), for k = 0 ... c-2, has the direction of travel h_i(k) = P_i(k+1) - P_i(k).
 * - It also has hh = h.x*h.x + h.y*h.y and len = sqrt(hh).
 * - A station exists if all four coordinates are finite.
 * - A station moves if it exists and hh > 0.
 *
 * Terms of an ordered pair (i, j), j != i, at station k.
 * - Both stations must exist and (i, k) must move.
 * - Always subtract, never negate: w = P_j(k) - P_i(k).
 * - With h = h_i(k):
 *   - g = w.x*h.x + w.y*h.y is how far j is ahead of i, in m * m/sample.
 *   - cr = h.x*w.y - h.y*w.x is positive when j is on i's left.
 *   - dot = h.x*h_j(k).x + h.y*h_j(k).y.
 * - Each term is two products and one sum or difference in fp64. None is contracted to an FMA (#pragma clang fp contract(off)).
 *   No fp32 and no fast-math functions are used.
 * - a = g / len and lat = cr / len, in metres.
 *
 * Following, per station (k, i).
 * - j is a candidate leader iff the terms exist, g > 0, fabs(lat) <= band and dot >= 0.
 * - dot >= 0 means a stationary j ahead counts and an oncoming j does not.
 * - The leader is the candidate with the smallest g. Ties go to the lowest j (a strict < in population order).
 * - Report three values:
 *   - gap = g / len, in metres.
 *   - gap_with = j.
 *   - thw = gap / len, in samples.
 * - If there is no candidate, or (i, k) exists but does not move, the row is +inf / -1 / +inf.
 * - If (i, k) does not exist, the row is NaN / -1 / NaN, and (i, k) is nobody's partner.
 *
 * Passing, per interval k = 0 ... c-3.
 * - "i passes j in interval k" holds iff all of the following hold:
 *   - Stations (i, k) and (i, k+1) move.
 *   - Stations (j, k) and (j, k+1) exist.
 *   - g(k) > 0 && g(k+1) <= 0, each with its own station's h.
 *   - fabs(lat_at) <= lat_max, with lat_at as below.
 * - The interval is half open. A partner exactly abeam at a sample counts in the interval that ends there and nowhere else.
 * - The values are:
 *   - s = a0 / (a0 - a1).
 *   - t = (double)k + s.
 *   - lat_at = lat0 + s * (lat1 - lat0).
 *   - closing = a0 - a1, in m/sample.
 *   - kind is +1 (overtaking) if dot(k) > 0, -1 (meeting) if < 0, and 0 otherwise. Kind 0 covers a stationary partner or an
 *     exactly perpendicular one.
 *   - cosine = dot(k) / (len_i(k) * len_j(k)). It is NaN for a stationary partner.
 * - Comparisons are made as written, so a NaN fails them.
 *
 * Made and received.
 * - Per interval (k, i), made_* is the passing by i with the smallest fabs(lat_at), lowest j on ties: made_lat (signed),
 *   made_with, made_t, made_kind.
 * - by_* is the passing OF i by some j with the smallest fabs(lat_at), lowest j on ties. Here lat_at, t and kind are as the passer
 *   j reports them.
 * - The lane of i evaluates "j passes i" itself, in j's frame, with the same operations in the same order as j's lane:
 *   w' = P_i - P_j, and so on. IEEE gives a - b == -(b - a), so both lanes form the same bits. The results therefore need no
 *   atomics, and a row does not depend on what else is in the launch.
 * - Rows with no passing are +inf / -1 / NaN / 0.
 * - Row made_*[k, i] is NaN / -1 / NaN / 0 if station (i, k) does not exist.
 *
 * Per road user over the call.
 * - run_gap and run_thw are each the minimum over the stations. Each comes with its partner and its k, the earliest k on ties.
 * - run_made_* and run_by_* are each the minimum fabs(lat) over the intervals, earliest k on ties. Each comes with lat, with, t
 *   and kind.
 * - run_made[n][3] and run_by[n][3] (int32) count passings as (overtaking, meeting, other).
 *
 * Events.
 * - Events are optional. They are on when lat_event > 0; +inf means every passing.
 * - An event is an ORDERED passing (i passes j) with fabs(lat_at) < lat_event.
 * - It is stored by the passer's lane as {int32 i, j, k, kind; double t, lat, closing, cosine;}, 48 bytes.
 * - Capacity, total count, "sorted by (i, j, k) when total <= capacity" and "unspecified subset otherwise" are exactly as for
 *   csf_pet_event.
 *
 * Small calls.
 * - c < 2 gives no stations.
 * - c < 3 gives no intervals.
 * - A population of one finds nothing.
 * - All of these succeed. */
typedef struct csf_passing_event {
    int32_t i, j, k, kind;
    double t, lat, closing, cosine;
} csf_passing_event;
/* Where the results of one engine go; any pointer may be NULL (that array is not returned).  n = the road users, c = n_samples.
 * event_capacity = 0 with events NULL counts the events without storing any.  With c < 2 the per-station arrays have no rows,
 * with c < 3 the per-interval arrays have none, and run_* are written as "nothing found" (+inf / -1 / NaN / 0, k = -1).  t and
 * the k of run_gap_k / run_thw_k count from the call's first sample. */
typedef struct csf_passing_out {
    double *gap;              /* [c-1, n] metres to the leader */
    int32_t *gap_with;        /* [c-1, n] the leader */
    double *thw;              /* [c-1, n] time headway, in samples */
    double *made_lat;         /* [c-2, n] signed clearance of the passing i made with the smallest fabs ... */
    int32_t *made_with;       /* [c-2, n] ... whom it passed ... */
    double *made_t;           /* [c-2, n] ... when ... */
    int32_t *made_kind;       /* [c-2, n] ... and +1 overtaking, -1 meeting, 0 other */
    double *by_lat;           /* [c-2, n] the passing OF i with the smallest fabs(lat_at), as the passer reports it */
    int32_t *by_with;         /* [c-2, n] the passer */
    double *by_t;             /* [c-2, n] */
    int32_t *by_kind;         /* [c-2, n] */
    double *run_gap;          /* [n] the smallest gap ... */
    int32_t *run_gap_with;    /* [n] ... to whom ... */
    int32_t *run_gap_k;       /* [n] ... at which station */
    double *run_thw;          /* [n] the smallest headway, likewise */
    int32_t *run_thw_with;    /* [n] */
    int32_t *run_thw_k;       /* [n] */
    double *run_made_lat;     /* [n] the passing made with the smallest fabs(lat) */
    int32_t *run_made_with;   /* [n] */
    double *run_made_t;       /* [n] */
    int32_t *run_made_kind;   /* [n] */
    double *run_by_lat;       /* [n] the passing received with the smallest fabs(lat) */
    int32_t *run_by_with;     /* [n] */
    double *run_by_t;         /* [n] */
    int32_t *run_by_kind;     /* [n] */
    int32_t *run_made;        /* [n, 3] passings made: overtakings, meetings, others */
    int32_t *run_by;          /* [n, 3] passings received */
    csf_passing_event *events;   /* [event_capacity] */
    int64_t event_capacity;
    int64_t n_events;         /* written: the events found, stored or not */
    int64_t first_sample;     /* written: the index of the first sample covered */
} csf_passing_out;
/* Samples [first_sample, first_sample + n_samples) of the engine's state ring, numbered and range-checked as csf_get_record has
 * them (not before the ring's first valid sample: "the lifetime of a recording" at csf_record), on rings of csf_record and csf_enable_history alike.  Pending uploads are brought in, both streams are waited for as the
 * read-backs do, and the engine is left exactly as it was.  TWO launches whatever the sizes are - every ordered pair at every
 * station, then the window pass - with one hipMemsetAsync of the event counters, one transfer and one wait (the launch counter
 * below grows by 2 per call that covers a station).  Refused without side effects (CSF_E_ARG / CSF_E_STATE, with a message,
 * launch counter unchanged): a NULL out; first_sample == -1 (the current state has no direction of travel) or no ring;
 * n_samples < 0 or above 65535; samples that are not in the ring; band NaN or negative (+inf is allowed); lat_max NaN or <= 0
 * (+inf is allowed); lat_event NaN or -inf; a negative event capacity, or a capacity with a NULL buffer; a rank of a sharded run
 * or a member of a loopback group; an engine that holds a calibration data set.  While csf_profile_enable is on, the first
 * launch is timed as kernel 0. */
int csf_passing(csf_engine *e, int64_t first_sample, int64_t n_samples, double band, double lat_max, double lat_event, csf_passing_out *out);
/* The last n_last samples of every member of a batch (in join order) that records, all members in the same two launches, with one
 * transfer and one wait; outs [count].  A member without a ring is skipped: its n_events becomes 0 and its first_sample -2.  A
 * recording member with fewer than n_last samples in its ring makes the call a refusal before anything is written. */
int csf_batch_passing(csf_engine *const *engines, int32_t count, int64_t n_last, double band, double lat_max, double lat_event,
                      csf_passing_out *outs);
/* launches of the two calls above so far (a batch counts on its first member) */
int csf_passing_launches(const csf_engine *e, int64_t *n_launches);

/* ---- flow: crossings of counting lines, occupancy of areas and of a grid, of a recording --------- */

/* How many road users crossed a cross-section, in which direction and at what speed, how many were inside a stretch of path at each
 * sample and how far they rode there, and where on the plane they spent their time - formed on the device from the state ring that
 * csf_record / csf_enable_history keep.
 *
 * A call covers samples [first_sample, first_sample + c) of the state ring, numbered k = 0 ... c-1 inside the call. P_i(k) = (x, y)
 * are the fp64 bits of the ring.
 *
 * General rules.
 * - Every term below is at most two products and one sum or difference in fp64, formed as written.
 * - Nothing is contracted to an FMA (#pragma clang fp contract(off)). No fp32 and no fast-math functions are used.
 * - sqrt and / are the correctly rounded ones.
 * - Comparisons are made as written, so a NaN fails them.
 * - Always subtract, never negate.
 *
 * Samples and stations.
 * - Sample (i, k) exists iff both coordinates are finite.
 * - Station (i, k), for k <= c-2, exists iff samples k and k+1 exist.
 * - At a station h = P(k+1) - P(k), hh = h.x*h.x + h.y*h.y and len = sqrt(hh). len is in metres per sample.
 *
 * Layout. csf_flow_layout is shared by all members of a batch. It holds:
 * - lines [L, 4] = ax, ay, bx, by, with L <= 64;
 * - areas [R, 5] = ax, ay, bx, by, half_width, with R <= 64;
 * - a grid x0, y0, h, nx, ny, where nx == 0 means no grid and nx*ny <= 2^20.
 * For a line or an area, d = B - A, dd = d.x*d.x + d.y*d.y and ld = sqrt(dd).
 *
 * Lines, per station (i, k) and line l.
 * - Side values: s(P) = d.x*(P.y - A.y) - d.y*(P.x - A.x), which is positive on the left of A -> B. s0 = s(P(k)) and
 *   s1 = s(P(k+1)).
 * - A sign change is (s0 > 0) != (s1 > 0). A point exactly on the line counts as on the right. A path that touches the line and
 *   turns back therefore crosses twice, once in each direction.
 * - t = s0 / (s0 - s1).
 * - The crossing point is X = (P(k).x + t*h.x, P(k).y + t*h.y).
 * - u = ((X.x - A.x)*d.x + (X.y - A.y)*d.y) / dd.
 * - A crossing is a sign change with u >= 0 && u <= 1.
 * - dir is +1 if s0 > 0 (left to right) and -1 otherwise.
 * - time = (double)k + t.
 * - speed = len.
 *
 * Areas are oriented rectangles around a centre line, as for a stretch of cycle path. Per sample (i, k) that exists and area r:
 * - w = P - A.
 * - g = w.x*d.x + w.y*d.y.
 * - cr = d.x*w.y - d.y*w.x.
 * - The sample is inside iff g >= 0 && g <= dd && fabs(cr) <= half_width*ld.
 *
 * Grid, per sample that exists.
 * - cx = floor((P.x - x0)/h) and cy likewise.
 * - The sample is inside iff cx >= 0 && cx < nx && cy >= 0 && cy < ny. The test is made on the doubles before any conversion.
 *
 * Results.
 * - Each (road user, interval, line) has at most one crossing, so the results carry no reduction order except the stated
 *   sequential sum over k of in_dist. All other aggregates are integers.
 * - in_dist starts from +0.0 and is the sum over k = 0 ... c-2, in this order, of len_i(k) for the existing stations whose sample k
 *   is inside.
 *
 * Events.
 * - An event is a crossing, stored by the lane that found it as {int32 i, l, k, dir; double t, u, speed;}, 40 bytes.
 * - n_events counts every crossing found, stored or not, and is always written.
 * - When n_events <= event_capacity the events are sorted by (i, l, k). Otherwise an unspecified subset is stored, exactly as for
 *   csf_passing_event.
 *
 * Small calls.
 * - c < 2 gives no intervals.
 * - n = 0, L = R = nx = 0 and a population of one are all fine.
 * - All of these succeed. */
typedef struct csf_flow_layout {
    const double *lines;      /* [n_lines, 4] ax, ay, bx, by */
    const double *areas;      /* [n_areas, 5] ax, ay, bx, by, half_width */
    int32_t n_lines;          /* L: 0 ... 64 */
    int32_t n_areas;          /* R: 0 ... 64 */
    double x0;                /* the grid's origin ... */
    double y0;
    double h;                 /* ... the side of a cell, in metres ... */
    int32_t nx;               /* ... and the cells along x and y; nx == 0 && ny == 0: no grid */
    int32_t ny;
} csf_flow_layout;
typedef struct csf_flow_event {
    int32_t i, l, k, dir;
    double t, u, speed;
} csf_flow_event;
/* Where the results of one engine go; any pointer may be NULL (that array is not returned), and the arrays of an absent part of
 * the layout have no rows.  n = the road users, c = n_samples, L, R, nx, ny the layout's.  event_capacity = 0 with events NULL
 * counts the events without storing any.  t counts from the call's first sample. */
typedef struct csf_flow_out {
    int32_t *line_count;      /* [c-1, L, 2] crossings in interval k by direction (index 0: +1, 1: -1) */
    int32_t *cross_n;         /* [n, L, 2] crossings of each road user over the call */
    double *first_t;          /* [n, L] a road user's first crossing of a line (the lowest k): when; +inf if none ... */
    double *first_u;          /* [n, L] ... where along the line; NaN if none ... */
    double *first_speed;      /* [n, L] ... at what speed; NaN if none ... */
    int32_t *first_dir;       /* [n, L] ... and in which direction; 0 if none */
    int32_t *occupancy;       /* [c, R] road users inside at sample k */
    int32_t *in_samples;      /* [n, R] samples inside */
    int32_t *in_first;        /* [n, R] first sample inside, -1 if never */
    int32_t *in_last;         /* [n, R] last sample inside, -1 if never */
    double *in_dist;          /* [n, R] metres ridden inside */
    int32_t *grid_count;      /* [ny, nx] samples in each cell over the call */
    csf_flow_event *events;   /* [event_capacity] */
    int64_t event_capacity;
    int64_t n_events;         /* written: the crossings found, stored or not */
    int64_t n_outside;        /* written: the existing samples outside the grid (0 without a grid) */
    int64_t first_sample;     /* written: the index of the first sample covered */
} csf_flow_out;
/* Samples [first_sample, first_sample + n_samples) of the engine's state ring, numbered and range-checked as csf_get_record has
 * them (not before the ring's first valid sample: "the lifetime of a recording" at csf_record), on rings of csf_record and csf_enable_history alike.  Pending uploads are brought in, both streams are waited for as the
 * read-backs do, and the engine is left exactly as it was.  TWO launches whatever the sizes are - every (sample, road user) cell
 * against the layout, then the walk along k of every (road user, line or area) - with one hipMemsetAsync of the counters, one
 * transfer and one wait (the launch counter below grows by 2 per call that covers a sample of a road user).  Refused without side
 * effects (CSF_E_ARG / CSF_E_STATE, with a message, launch counter unchanged): a NULL out or layout; n_lines or n_areas outside
 * 0 ... 64, or a count above 0 with a NULL array; a line or area with a non-finite coordinate or dd == 0; half_width NaN, negative
 * or +inf; with a grid, h not finite or <= 0, x0 or y0 not finite; nx or ny negative, exactly one of them 0, or nx*ny > 2^20;
 * first_sample < 0 (the current state has no interval) or no ring; n_samples < 0 or above 65535; samples that are not in the
 * ring; more than 2^31 (sample, road user) cells; a negative event capacity, or a capacity with a NULL buffer; a rank of a sharded
 * run or a member of a loopback group; an engine that holds a calibration data set.  While csf_profile_enable is on, the first
 * launch is timed as kernel 0. */
int csf_flow(csf_engine *e, int64_t first_sample, int64_t n_samples, const csf_flow_layout *layout, csf_flow_out *out);
/* The last n_last samples of every member of a batch (in join order) that records, all members in the same two launches, with one
 * transfer and one wait; outs [count].  A member without a ring is skipped: its n_events becomes 0 and its first_sample -2.  A
 * recording member with fewer than n_last samples in its ring makes the call a refusal before anything is written, and so do
 * members x grid cells above 2^24. */
int csf_batch_flow(csf_engine *const *engines, int32_t count, int64_t n_last, const csf_flow_layout *layout, csf_flow_out *outs);
/* launches of the two calls above so far (a batch counts on its first member) */
int csf_flow_launches(const csf_engine *e, int64_t *n_launches);

/* ---- road clearance: edge distances and edge crossings of a recording ---------------------------- */

/* How close to the road's edges every road user came, where across the width of the path it rode, and whether it left the road -
 * formed on the device from the state ring that csf_record / csf_enable_history keep.
 *
 * A call covers samples [first_sample, first_sample + c) of the state ring, numbered k = 0 ... c-1 inside the call. P_i(k) = (x, y)
 * are the fp64 bits of rows 0 and 1 of the ring. The general rules are those of the flow section above: every term is at most two
 * products and one sum or difference in fp64, formed as written and never contracted; sqrt and / are the correctly rounded ones;
 * comparisons are made as written, so a NaN fails them.
 *
 * The road is given to the call (csf_clearance_road); it is NOT the engine's packed fp32 vertices. It is n_edges polylines as
 * csf_set_road_vertices takes them: offsets [n_edges + 1] into xy [V][2], every polyline with at least 2 vertices. Its
 * S = V - n_edges segments A -> B (consecutive vertices of a polyline) are numbered g = 0 ... S-1 in the order of the polylines; a
 * result names a segment as (edge, seg), seg counted within the polyline. For a segment dx = bx - ax, dy = by - ay,
 * dd = dx*dx + dy*dy.
 *
 * Samples and stations.
 * - Cell (k, i) exists iff both coordinates of P_i(k) are finite.
 * - Station (k, i), for k <= c-2, exists iff cells k and k+1 exist. At a station w = P(k+1) - P(k): the direction of travel.
 *
 * Distance, per cell P = (px, py) and segment.
 * - rx = px - ax, ry = py - ay.
 * - gg = rx*dx + ry*dy.
 * - t = gg / dd, then t = t > 0 ? t : 0.0, then t = t > 1 ? 1.0 : t.
 * - qx = ax + t*dx, qy = ay + t*dy.
 * - ex = qx - px, ey = qy - py.
 * - d2 = ex*ex + ey*ey.
 * The nearest segment is the lowest g with the smallest d2 (a strict < from +inf). d = sqrt(d2); t is that segment's.
 *
 * Left and right, per station and segment, with the ex, ey of sample k.
 * - z = wx*ey - wy*ex.
 * - A segment with z > 0 is on the left of the direction of travel, one with z < 0 on its right; z == 0 (straight ahead, behind,
 *   or not moving) is neither.
 * - left / right are the square roots of the smallest d2 among each, the lowest g on ties; +inf where there is none.
 *
 * Crossing, per station and segment: the flow section's test with the segment as the line.
 * - s(P) = dx*(P.y - ay) - dy*(P.x - ax); s0 = s(P(k)), s1 = s(P(k+1)).
 * - A sign change is (s0 > 0) != (s1 > 0).
 * - tt = s0 / (s0 - s1).
 * - The crossing point is C = (P(k).x + tt*wx, P(k).y + tt*wy).
 * - u = ((C.x - ax)*dx + (C.y - ay)*dy) / dd.
 * - A crossing is a sign change with u >= 0 && u <= 1. dir is +1 if s0 > 0 and -1 otherwise.
 * - A path through a vertex shared by two consecutive segments may count on both (u == 1 of one, u == 0 of the next).
 *
 * Per road user.
 * - d_min is the smallest d over k (strict <, so the lowest k on ties) with its k, edge and seg; +inf and -1 if never present.
 * - left_min and right_min likewise over the stations; +inf and -1 where no station has a segment on that side.
 * - near_samples counts the samples with d < d_event, near_first and near_last are the first and last of them (-1: none).
 *   d_event == 0 finds none.
 * - cross_n is the number of crossings.
 *
 * Events.
 * - An event is a crossing, stored by the lane that found it as {int32 i, k, edge, seg, dir; double t, u;} with t = k + tt: 40 bytes.
 * - n_events counts every crossing found, stored or not, and is always written.
 * - When n_events <= event_capacity the events are sorted by (i, k, edge, seg). Otherwise an unspecified subset is stored.
 *
 * Small calls. c == 0 or no road users succeeds without a launch and writes "nothing found"; c == 1 has samples and no station. */
typedef struct csf_clearance_road {
    const int64_t *offsets;   /* [n_edges + 1] first vertex of every polyline, and V */
    const double *xy;         /* [V, 2] */
    int32_t n_edges;
} csf_clearance_road;
typedef struct csf_clearance_event {
    int32_t i, k, edge, seg, dir;
    double t, u;
} csf_clearance_event;
/* Where the results of one engine go; any pointer may be NULL (that array is not returned).  n = the road users, c = n_samples.
 * event_capacity = 0 with events NULL counts the events without storing any. */
typedef struct csf_clearance_out {
    double *d;                /* [c, n] distance to the nearest segment; NaN without a cell */
    int32_t *edge;            /* [c, n] ... its polyline; -1 */
    int32_t *seg;             /* [c, n] ... its place in the polyline; -1 */
    double *t;                /* [c, n] ... the clamped place along it; NaN */
    double *left;             /* [c-1, n] nearest on the left; +inf: none; NaN: no station */
    double *right;            /* [c-1, n] nearest on the right */
    int32_t *left_edge;       /* [c-1, n] -1 */
    int32_t *right_edge;      /* [c-1, n] -1 */
    int32_t *cross;           /* [c-1, n] segments crossed at the station */
    double *d_min;            /* [n] */
    int32_t *d_min_k;         /* [n] */
    int32_t *d_min_edge;      /* [n] */
    int32_t *d_min_seg;       /* [n] */
    double *left_min;         /* [n] */
    int32_t *left_min_k;      /* [n] */
    double *right_min;        /* [n] */
    int32_t *right_min_k;     /* [n] */
    int32_t *near_samples;    /* [n] */
    int32_t *near_first;      /* [n] */
    int32_t *near_last;       /* [n] */
    int32_t *cross_n;         /* [n] */
    int32_t *near_count;      /* [c] road users with d < d_event at sample k */
    int32_t *cross_count;     /* [c-1] crossings at the stations k */
    csf_clearance_event *events;   /* [event_capacity] */
    int64_t event_capacity;
    int64_t n_events;         /* written: the crossings found, stored or not */
    int64_t first_sample;     /* written: the index of the first sample covered */
} csf_clearance_out;
/* Samples [first_sample, first_sample + n_samples) of the engine's state ring, numbered and range-checked as for the flow call
 * above, on rings of csf_record and csf_enable_history alike.  Pending uploads are brought in, both streams are waited for, and the
 * engine is left exactly as it was.  THREE launches whatever the sizes are - every cell against every chunk of 512 segments (the
 * grid's third extent), the chunks put together in the order of their index with the same strict < (the result does not depend on
 * the chunk size), then the walk along k of every road user - with one upload of the road, one hipMemsetAsync of the counters, one
 * transfer and one wait (the launch counter below grows by 3 per call that covers a sample of a road user).  Refused without side
 * effects (CSF_E_ARG / CSF_E_STATE, with a message, launch counter unchanged): a NULL out or road; n_edges < 1, NULL offsets or xy;
 * offsets that do not start at 0 or a polyline with fewer than 2 vertices (which covers offsets that are not monotone); more than
 * 2^20 segments; a non-finite coordinate; a segment with dd == 0 or non-finite dd (the message names edge and segment); d_event
 * negative or not finite; everything the flow call refuses for its window and engine; (sample, road user) cells x segments above
 * 2^40; a negative event capacity, or a capacity with a NULL buffer.  While csf_profile_enable is on, the first launch is timed as
 * kernel 0. */
int csf_clearance(csf_engine *e, int64_t first_sample, int64_t n_samples, const csf_clearance_road *road, double d_event, csf_clearance_out *out);
/* The last n_last samples of every member of a batch (in join order) that records, at ONE road shared by all members, in the same
 * three launches, with one transfer and one wait; outs [count].  A member without a ring is skipped: its n_events becomes 0 and
 * its first_sample -2.  A recording member with fewer than n_last samples in its ring makes the call a refusal before anything is
 * written, and so do members x chunks of segments above 65535 and the cells of all members x segments above 2^40. */
int csf_batch_clearance(csf_engine *const *engines, int32_t count, int64_t n_last, const csf_clearance_road *road, double d_event, csf_clearance_out *outs);
/* launches of the two calls above so far (a batch counts on its first member) */
int csf_clearance_launches(const csf_engine *e, int64_t *n_launches);

/* ---- body encounters: gaps and time to contact between vehicle outlines of a recording ----------- */

/* csf_encounters makes every road user a disc of one radius.  Here every road user is an oriented rectangle of its own size, and
 * the call reports the free gap between the outlines and the constant-velocity time to contact of the outlines (DESIGN.md
 * section 4.17).
 *
 * Outline.
 * - Road user i has ext[i] = (front, rear, half_width). These are the metres from the point (x, y) of its state to the front end
 *   and to the rear end along the heading, and the half width. A call carries one triple per road user.
 * - Take x, y, psi, v from rows 0 - 3 of the state, as csf_encounters does.
 * - cs = cos psi, sn = sin psi.
 * - L = 0.5 (front + rear), W = half_width, o = 0.5 (front - rear).
 * - The centre is m = (x + o cs, y + o sn). The velocity is u = (v cs, v sn).
 *
 * Pair (i, j), j != i.
 * - w = m_j - m_i, c = u_j - u_i.
 * - cr = cs_i cs_j + sn_i sn_j, sr = cs_i sn_j - sn_i cs_j.
 * - Four axes in the order h_i, n_i, h_j, n_j, with h = (cs, sn) and n = (-sn, cs). For each axis:
 *   - the place s_k = w . e_k;
 *   - the rate g_k = c . e_k;
 *   - the reach r_k.
 * - The products are written wx*cs + wy*sn and wy*cs - wx*sn.
 * - The reaches are:
 *   - r_0 = L_i + (L_j |cr| + W_j |sr|)
 *   - r_1 = W_i + (L_j |sr| + W_j |cr|)
 *   - r_2 = L_j + (L_i |cr| + W_i |sr|)
 *   - r_3 = W_j + (L_i |sr| + W_i |cr|)
 * - sep = max_k (|s_k| - r_k). The bodies overlap iff sep <= 0. Touching counts as overlap.
 *
 * Gap.
 * - The gap is 0 if the bodies overlap.
 * - Otherwise it is sqrt(min d2) over eight corner-to-box distances.
 * - For the four corners (a, b) in {+1, -1}^2 of j in the frame of i:
 *   - X = s_0 + (a L_j cr - b W_j sr)
 *   - Y = s_1 + (a L_j sr + b W_j cr)
 *   - dx = max(|X| - L_i, 0), dy = max(|Y| - W_i, 0)
 *   - d2 = dx dx + dy dy
 * - Do the same for the corners of i in the frame of j, with -s_2, -s_3, cr, -sr and the roles of i and j exchanged.
 * - Take the minimum with a strict < from +inf.
 *
 * Time to contact. Headings and velocities are held constant.
 * - ttc = 0 if the bodies overlap.
 * - Otherwise go per axis:
 *   - If g_k == 0 and |s_k| > r_k, the pair never meets.
 *   - If g_k == 0 otherwise, the axis constrains nothing.
 *   - If g_k != 0, ta = (-r_k - s_k) / g_k, tb = (r_k - s_k) / g_k, enter_k = min(ta, tb), leave_k = max(ta, tb).
 * - T_in = max_k enter_k, T_out = min_k leave_k.
 * - ttc = +inf if the pair never meets, or T_in > T_out, or T_in < 0. Otherwise ttc = T_in.
 *
 * Arithmetic.
 * - No term is contracted to an FMA.
 * - / and sqrt are the correctly rounded ones.
 * - There is no fp32 and no fast math.
 * - gap_ij and ttc_ij are bitwise symmetric in (i, j).
 *
 * Per (sample, i).
 * - gap_min, gap_with, ttc_min, ttc_with.
 * - The lowest j wins on ties.
 * - The partner is -1 where the minimum is +inf.
 * - A road user with a non-finite x, y, psi, v is neither receiver nor partner. Its own row is NaN / -1.
 * - A population of one gives +inf / -1.
 *
 * Per road user over the window.
 * - run_gap_min, run_ttc_min, each with its partner and its absolute sample. The earliest sample wins on ties.
 * - overlap_n: the number of samples in which its gap_min is 0.
 * - The current state counts as sample -1.
 *
 * Events {int64 sample; int32 i, j; double gap, ttc;} for i < j:
 * - An event needs gap_ij <= gap_event or ttc_ij < ttc_event.
 * - gap_event < 0 switches the gap test off.
 * - gap_event == 0 lists exactly the collisions.
 * - ttc_event <= 0 switches the ttc test off.
 * - Capacity, counting and sorting by (sample, i, j) are as for csf_encounter_event. */
typedef struct csf_body_event {
    int64_t sample;
    int32_t i, j;
    double gap, ttc;
} csf_body_event;
/* Where the results of one engine go; any pointer may be NULL (that array is not returned).  n = the road users, n_samples the
 * samples the call covers.  event_capacity = 0 with events NULL counts the events without storing any. */
typedef struct csf_body_out {
    double *gap_min;          /* [n_samples, n] */
    int32_t *gap_with;        /* [n_samples, n] */
    double *ttc_min;          /* [n_samples, n] */
    int32_t *ttc_with;        /* [n_samples, n] */
    double *run_gap_min;      /* [n] the window's minima ... */
    int32_t *run_gap_with;    /* [n] ... the partner ... */
    int64_t *run_gap_sample;  /* [n] ... and the sample of each */
    double *run_ttc_min;      /* [n] */
    int32_t *run_ttc_with;    /* [n] */
    int64_t *run_ttc_sample;  /* [n] */
    int64_t *overlap_n;       /* [n] samples in which gap_min is 0 */
    csf_body_event *events;   /* [event_capacity] */
    int64_t event_capacity;
    int64_t n_events;         /* written: the events found, stored or not */
    int64_t first_sample;     /* written: the index of the first sample covered (-1: the current state) */
} csf_body_out;
/* Samples [first_sample, first_sample + n_samples) of the engine's state ring, numbered and range-checked as csf_encounters has
 * them; first_sample == -1 with n_samples == 1 is the current state.  ext [n][3] are the extents (front, rear, half_width) of the
 * road users in population order.  The engine is left exactly as it was.  Two launches whatever the sizes are, one upload of the
 * extents, one memset, one transfer and one wait (the launch counter below grows by 2 per call that covers anything).  Refused
 * without side effects (CSF_E_ARG / CSF_E_STATE, with a message): everything csf_encounters refuses; a NULL ext; a non-finite
 * extent; front < 0, rear < 0, front + rear <= 0 or half_width <= 0 (the message names the road user); a non-finite threshold.
 * While csf_profile_enable is on, the first launch is timed as kernel 0. */
int csf_body_encounters(csf_engine *e, int64_t first_sample, int64_t n_samples, const double *ext, double gap_event, double ttc_event,
                        csf_body_out *out);
/* The last n_last samples of every member of a batch (in join order) that records, all members in the same two launches; exts
 * [count] pointers to every member's extents, outs [count].  A member without a ring is skipped: its n_events becomes 0 and its
 * first_sample -2 (its exts entry is not read).  Refusals as for csf_batch_encounters and the call above. */
int csf_batch_body_encounters(csf_engine *const *engines, int32_t count, int64_t n_last, const double *const *exts, double gap_event,
                              double ttc_event, csf_body_out *outs);
/* launches of the two calls above so far (a batch counts on its first member) */
int csf_body_encounter_launches(const csf_engine *e, int64_t *n_launches);

/* ---- single-function entry points for known-answer tests -------------------------------------- */

/* calcRepulsiveForce of one source at m receivers through the device code of the pair kernel
 * (vehicle.py:1560-1648 for TWOD/INVPEND/PLANARPOINT engines, :1054-1147 for BICYCLE engines).
 * src = (x, y, psi, v); receivers x, y, psi [m]; apply_fov != 0 also applies the mask of
 * intersection.py:690-745 (masked pairs return 0). */
int csf_pair_force(csf_engine *e, const double *src, int64_t m, const double *x, const double *y,
                   const double *psi, int32_t apply_fov, double *Fx, double *Fy);

/* get_untracked_foes() (intersection.py:690-745) as the matrix the reference returns: out [n, n] bytes, row = source i,
 * column = receiver j, 1 = "j ignores i" (the diagonal is 1), from the test the pair kernels apply.  n <= 46340. */
int csf_untracked(csf_engine *e, uint8_t *out);
/* Vehicle.updateDestination() (vehicle.py:545-594) for the listed agents, on its own: the queue pointer moves exactly as
 * it does at the start of calcDestinationForce(). */
int csf_update_destination(csf_engine *e, int64_t n, const int32_t *idx);
/* Vehicle.updateNavState(stop) (vehicle.py:354-457) for the listed agents: advances the three-state machine and returns
 * what the reference returns, (vd, ddest).  stop is NULL or [n]: >= 0 stands in for the stop flag of the current
 * destination (the reference passes it explicitly), < 0 reads the flag of the queue row. */
int csf_update_nav_state(csf_engine *e, int64_t n, const int32_t *idx, const int32_t *stop, double *vd, double *ddest);
/* vehicle.destpointer assigned from the host (Vehicle.stop types 1 and 2 step it back: vehicle.py:486-502) */
int csf_set_dest_pointer(csf_engine *e, int64_t n, const int32_t *idx, const int32_t *ptr);

/* UncontrolledVehicle.__init__(s0, trajectory) (vehicle.py:925-960): the prescribed trajectory of the listed road users
 * (of a CSF_UNCONTROLLED parameter set), rows (x, y, psi, v) = the columns of the reference's `traj`; at tick i the
 * state becomes row i while there is one (vehicle.py:964-979).  An empty range restores the default: the reference's
 * ring of zeros behind the start state (vehicle.py:158-160), i.e. the vehicle sits at (0, 0) from its first tick on. */
int csf_set_script(csf_engine *e, int64_t n, const int32_t *agent, const int64_t *offsets, const double *rows);

/* ---- sharding over the GPUs of one node ------------------------------------- */

/* The population is replicated on the host side of every rank; rank r integrates the contiguous
 * receiver block [r*N/world, (r+1)*N/world) and all-gathers the fp32 source records (x, y, cos psi,
 * sin psi [, e, k]) of the other blocks with one RCCL all-gather per tick on a second HIP stream.
 * Call csf_comm_unique_id on rank 0, distribute the 128 bytes out of band (torch.distributed), then
 * csf_comm_init on every rank before the first csf_step.  world == 1 needs none of this. */
#define CSF_UNIQUE_ID_BYTES 128
int csf_comm_unique_id(uint8_t id_out[CSF_UNIQUE_ID_BYTES]);
int csf_comm_init(csf_engine *e, const uint8_t id[CSF_UNIQUE_ID_BYTES], int32_t rank, int32_t world);
/* the receiver block of this rank: [lo, hi) */
int csf_shard_range(const csf_engine *e, int64_t *lo, int64_t *hi);

/* Rehearsal of the sharded path on ONE device (tests; no reference counterpart): `world` engines holding the same
 * population become ranks 0 .. world-1 of a loopback group.  They share one HIP stream, and where the ranks of a real
 * run call ncclAllGather the group copies every member's record block into the record arrays of the others.  Everything
 * else - shard bounds and padding, sentinel records, the receiver lists, the re-binning from gathered records, the
 * stale fp64 state of foreign agents - is the code path of csf_comm_init.  Members are stepped together with
 * csf_step_group (engines in rank order); csf_step on a member fails. */
int csf_comm_init_loopback(csf_engine *const *engines, int32_t world);
int csf_step_group(csf_engine *const *engines, int32_t world, int64_t n_ticks);

/* ---- batches of independent scenes -------------------------------------------------------------- */

/* Many small, independent scenes stepped together (the junctions of a SUMO network, parameter sweeps): `count` engines on
 * one device, each with its own population, road and parameters, become one batch.  They must be distinct, on one device,
 * not sharded, not in a loopback group and not in another batch; otherwise the call is refused and nothing changes.  The
 * members then share one HIP stream (each member's own stream is waited for first).  csf_step_batch steps every member by
 * n_ticks: the members the one-wave tick takes (see csf_small_ticks) run in ONE launch per vehicle class present - one wave
 * per scene, all ticks of the call - and, with csf_small_classes on, those of several parameter sets or classes in ONE further launch
 * whatever their classes (a small member of several sets or of the UncontrolledVehicle's class is stepped in turn otherwise);
 * the members the one-launch tick takes (see csf_mid_ticks: 33 ... 2 175 road users of one
 * parameter set), where the batch has at least two of them, run tick by tick in ONE launch per vehicle class and priority rule
 * and with / without road edges present - a member's road is summed inside that launch where csf_mid_road is on, the road is on no
 * lattice and has at most 2 048 padded vertices; every other member is stepped by csf_step in turn - among them a mid-size member
 * with road edges while csf_mid_road is off (the default), above that cap or on a lattice (its road term is a launch of its own per
 * tick), one with several parameter sets, a BalancingRider or UncontrolledVehicle population above 32 road users, and a single
 * mid-size member.  CSF_BATCH_MID=0 steps the mid-size members in turn as well.  Bit for bit what csf_step on
 * each member would give.  `engines` must be the batch in join order.  csf_batch_leave dissolves the batch, and so does
 * csf_destroy of a member: the others go on as single engines, and csf_step_batch on them fails with CSF_E_STATE. */
int csf_batch_join(csf_engine *const *engines, int32_t count);
int csf_batch_leave(csf_engine *const *engines, int32_t count);
int csf_step_batch(csf_engine *const *engines, int32_t count, int64_t n_ticks);
/* the outputs of csf_get_tick for one member; any pointer may be NULL */
typedef struct csf_tick_out {
    double *s_out;
    int32_t *dest_ptr;
    uint8_t *znav;
    double *Fx;
    double *Fy;
    int64_t *tick;
} csf_tick_out;
/* csf_step_batch, then the csf_get_tick outputs of every member (out[count]): the batched launch packs the read-back of its
 * members behind their last tick, and the host waits once for all of them. */
int csf_step_batch_get_tick(csf_engine *const *engines, int32_t count, int64_t n_ticks, const csf_tick_out *out);
/* The last n_last samples of every member of a batch (in join order) whose out[i] names an output: s [n_last, n_agents, n_states],
 * F [n_last, n_agents, 2] (either may be NULL; both NULL: the member is left out), first_sample (may be NULL) receives the index
 * of the first sample returned.  A named member without a recording (csf_record; csf_enable_history for states), or with
 * fewer than n_last samples in its ring, makes the call a refusal before anything is written.  One gather launch, one transfer
 * and one wait for the whole batch. */
typedef struct csf_record_out {
    double *s;
    double *F;
    int64_t *first_sample;
} csf_record_out;
int csf_batch_get_record(csf_engine *const *engines, int32_t count, int64_t n_last, const csf_record_out *out);
/* ticks this engine has run inside a batched ONE-WAVE launch (csf_small_ticks counts them too) */
int csf_batch_ticks(const csf_engine *e, int64_t *n_ticks);
/* ticks this engine has run inside a batched one-launch tick of mid-size members (csf_mid_ticks counts them too) */
int csf_batch_mid_ticks(const csf_engine *e, int64_t *n_ticks);
/* kernel launches and copy commands that csf_step_batch / csf_step_batch_get_tick have enqueued for the batched members - one-wave
 * and mid-size - of this engine's batch since csf_batch_join; what csf_step enqueues for the members stepped in turn is not
 * counted.  CSF_E_STATE: the engine is in no batch. */
int csf_batch_launches(const csf_engine *e, int64_t *n_launches);

/* ---- measurement ------------------------------------------------------------------------------ */

/* HIP-event time of the pair kernel, measured on the stream it is launched on: enable with on = k > 0 to
 * bracket the kernel on every k-th tick (an event record costs a few microseconds of launch gap, so the timed
 * region of bench.py samples every 8th tick), run csf_step, then read the accumulated milliseconds and the
 * number of sampled launches (reset on read). */
int csf_profile_enable(csf_engine *e, int32_t on);
int csf_profile_read(csf_engine *e, double *pair_ms, double *agent_ms, int64_t *launches);
/* The same with every kernel of the tick: ms[4] = accumulated milliseconds of the pair kernel, the road-edge kernel, the
 * per-agent kernel (each from the start / end time stamps of the kernel's own dispatch) and the all-gather, launches[4]
 * = the number of launches behind each sum; resets the sums.  The pair kernel is timed on every sampled tick, the
 * others on every 8th of them (a time stamp costs a few microseconds of launch gap).  The events come from a fixed pool
 * that is recycled in order, so profiling may stay enabled for any number of ticks.  csf_profile_samples copies the
 * pair-kernel time of every sampled launch since the last reset (microseconds, at most `capacity`, at most 65 536 are
 * kept) WITHOUT resetting. */
int csf_profile_kernels(csf_engine *e, double ms[4], int64_t launches[4]);
int csf_profile_samples(csf_engine *e, double *pair_us, int64_t capacity, int64_t *n_samples);
/* ... of any of the four (ABI 9): kernel = 0 pair, 1 road, 2 per-agent, 3 all-gather - what a median needs (a mean of ~40 sampled
 * launches is moved by one launch that met a re-binning or a clock step; bench.py and tools/ report median, min and max). */
int csf_profile_samples_of(csf_engine *e, int32_t kernel, double *us, int64_t capacity, int64_t *n_samples);
/* What ONE launch of the pair kernel on the current snapshot does (the roofline of bench.py is computed from it):
 *   counts[0]  pair evaluations - calls of the force field vehicle.py:1560-1648 for a (source, receiver) pair, after the
 *              mask of intersection.py:690-745, the far-field cull and the per-pair reach test;
 *   counts[1]  sources put through the per-lane tests (field of view and reach);
 *   counts[2], counts[3]  full (128 pairs) and partial evaluation passes.
 * Runs one extra launch with device counters; the state of the simulation is not advanced.  All -1 when the engine's
 * pair kernel does not count (kernel_name, if not NULL, names the kernel either way). */
int csf_count_pairs(csf_engine *e, int64_t counts[4], const char **kernel_name);
/* Pairs the pair kernels could NOT hand to their exact path since the engine was created (0 in every run seen so far).
 * The kernels decide the field of view (intersection.py:690-745) in fp32 and note every pair inside the rounding band of
 * an edge, and every pair closer than 1 m, in a per-wave list of 32 entries (emptied between receivers when half full);
 * noted pairs are re-decided and re-evaluated from the precise records, and what is undecidable even there goes to the
 * per-agent kernel, which decides as the reference does (fp64 atan2 -> limitAngle -> angleDifference).  An entry that
 * found its list full, or a hand-over ring that overflowed within one tick, is counted here; such a pair keeps the fp32
 * result. */
int csf_near_dropped(csf_engine *e, int64_t *n_dropped);
/* The order in which a workgroup of the pair kernel hands its receivers to its waves, computed on the host exactly as the kernel
 * computes it (csrc/csf_handout.h; needs no engine and no device): cand[r] / inside[r] are the candidate batches of receiver r in
 * the tile and those of them wholly inside its field of view, n <= 64.  rank[r]: the claim that takes receiver r - heavier
 * visits first, within a weight class by index - or -1 where cand[r] is empty; weight[r] (may be NULL): the visit's weight.
 * Returns the number of receivers ranked, -1 on bad arguments. */
int csf_handout_ranks(const uint32_t *cand, const uint32_t *inside, int32_t n, int32_t *rank, int32_t *weight);
/* The order in which the receiver groups of one source chunk are handed to the pair kernel's workgroups, computed on the host
 * exactly as the order kernel computes it (csrc/csf_wg_order.h; needs no engine and no device): order[rank] = group, heavier
 * groups first, equal costs in index order - a permutation of 0 .. n - 1 whatever the costs are.  Returns n, -1 on bad arguments. */
int csf_wg_order_ranks(const uint32_t *cost, int32_t n, int32_t *order);
/* Which kernel a pair launch takes, decided on the host by the function every launch asks (csrc/csf_pair.hip: pair_shape; tests).
 * csf_pair_shape_of needs no engine and no device.  in[CSF_PAIR_SHAPE_IN]: priority to the right, parameter sets, has_bike, model_mask,
 * vehicle class (enum csf_model), classify, recs_valid, pair_variant, recv_binned, rpb, wide, reach, order tables given, the segmented
 * one-grid launch, receivers of the launch, 0.  out[CSF_PAIR_SHAPE_OUT]: family (0 none, 1 pair_kernel with the source's own set per
 * pair, 2 pair_kernel, 3 pair_bike_kernel, 4 pair_cull_kernel, 5 pair_cull_kernel on the segmented grid), field, receivers per wave
 * (Bicycle), priority to the right, classify, binr, ord, reach, rpb, waves (cull family), receivers per workgroup, threads per
 * workgroup, sources per tile, gridDim.x, groups of the order tables (0: none); *name (may be NULL): the kernel's name in profiles.  Returns CSF_PAIR_SHAPE_OUT, -1 on bad
 * arguments.  csf_pair_shape_words fills `in` with the words of this engine's next pair launch (uploads what is pending). */
#define CSF_PAIR_SHAPE_IN 16
#define CSF_PAIR_SHAPE_OUT 15
int csf_pair_shape_of(const int32_t *in, int32_t *out, const char **name);
int csf_pair_shape_words(csf_engine *e, int32_t *in);
/* Read-back of the tables the last tick's pair launch used (measurement and tests; waits for the device): *groups x *chunks words
 * each; *ordered: 1 where that launch took its groups by an order table - then order[c * groups + k] is the group workgroup k of chunk
 * c served -, 0 where it took them in index order (order is left alone); cost[c * groups + g]: what the launch left for group g of
 * chunk c, 28 x tests + 58 x evaluations.  *groups = 0: that launch kept no tables (another kernel, CSF_WG_ORDER=0, no tick yet).
 * cost / order may be NULL; both hold `capacity` words, and a grid of more words is CSF_E_ARG. */
int csf_wg_order_tables(csf_engine *e, int64_t *groups, int32_t *chunks, int32_t *ordered, uint32_t *cost, int32_t *order, int64_t capacity);
/* Where a sharded engine issues the all-gather of a tick: 0 in stream order on its main stream, 1 on a second stream beside
 * the destination-force phase of the next tick.  Unless CSF_COMM_STREAM=main|second says which, the communicator times both
 * orders itself on its first tick - 32 launches each of the pair kernel + the collective on the records as they are, the
 * slowest rank's times shared through the communicator so that every rank decides alike - and keeps the faster;
 * us_per_tick (may be NULL) receives the two measurements (0 when nothing was measured). */
int csf_comm_stream_order(const csf_engine *e, int32_t *second_stream, double us_per_tick[2]);
/* milliseconds between the end of the agent kernel and the end of the RCCL all-gather, accumulated over the launches
 * of the last csf_profile_read (0 for an unsharded engine) */
int csf_profile_gather(const csf_engine *e, double *gather_ms);
/* Ticks this engine has run in its one-wave kernel (ABI 6).  Up to 32 road users of one parameter set (any rider class; not
 * UncontrolledVehicle) - the reference's own scenarios, e.g. the three cyclists of scenarios/ - on one device, with no road or a small one (at most 2048 vertices), without profiling and without the history ring of csf_enable_history (a recording by csf_record keeps this path): csf_step(e, n) is then ONE
 * launch of one wave for all n ticks (lane = road user; field-of-view decisions and np.sign(phi) on the fp64 difference of
 * the two positions, inside the band of fp32 rounding by the reference's own fp64 chain, intersection.py:690-745,
 * vehicle.py:1617-1625), instead of a pair launch and a per-agent launch per tick.  CSF_FUSED_SMALL=0 or a pinned CSF_PAIR_VARIANT keep the general path. */
int csf_small_ticks(const csf_engine *e, int64_t *n_ticks);
/* The one-wave tick and the batched launch for populations of SEVERAL PARAMETER SETS AND VEHICLE CLASSES (no change
 * of CSF_ABI_VERSION or csf_params: bind it where the library exports it).  on = 1: a population that meets every other condition of
 * csf_small_ticks and has more than one parameter set (csf_set_param_classes: any sets of any classes, up to one per road user) or is of
 * class CSF_UNCONTROLLED is ticked by small_classes_kernel - one wave, all ticks of csf_step in one launch, the constants of the field
 * staged per road user and one pass of the per-agent tick per vehicle class present - instead of a pair launch and one per-agent launch
 * per class and tick; inside a batch, csf_step_batch steps all such members in ONE further launch whatever their classes.  csf_small_ticks
 * and csf_batch_ticks count these ticks; csf_record and csf_step_get_tick work as on the one-wave path.  A single set of a rider class
 * keeps its kernel bit for bit, switch or no switch.  on = 0 (the default; CSF_SMALL_CLASSES=1 in the environment of csf_create turns it
 * on from the start): every call takes the kernels it took before there was a switch.  The results agree with the general path's within
 * the rounding of the pair sum (2e-5 m over 40 ticks), not bit for bit.  CSF_E_ARG for e == NULL or on outside 0 / 1; refused like
 * csf_step while a calibration data set is held; a refused call changes nothing. */
int csf_small_classes(csf_engine *e, int32_t on);
/* Ticks this engine has run as ONE launch each (ABI 7; csf_mid.hip).  Between 33 and ~3 000 road users of one parameter set on
 * one device - BASELINE config 2, and what the reference runs under SUMO - a tick is launch latency, not work: the pair sums
 * of a receiver group (intersection.py:690-745, 814-843) and the per-agent tick of its road users (:841-862, 891-892) share
 * one grid, ONE workgroup per receiver group: its first wave runs the destination-force phase while the others form the pair
 * sums, and behind the workgroup's barrier the same wave carries on with the group's road users; the
 * next tick's records go to the other half of a double buffer.  CSF_FUSED_MID=0, a pinned CSF_PAIR_VARIANT or per-kernel profiling keep the two launches. */
int csf_mid_ticks(const csf_engine *e, int64_t *n_ticks);
/* The ROAD TERM INSIDE the one-launch tick (no change of CSF_ABI_VERSION or csf_params: bind it where the library
 * exports it).  A population that csf_mid_ticks' tick takes and that has road edges (csf_set_road_vertices) runs road_kernel in front of
 * every tick: two launches again, and inside a batch such a member is stepped in turn.  on = 1: where the road is on no lattice
 * (CSF_ROAD_GRID) and has at most 2 048 padded vertices, the pair waves of the one launch sum the road term too (intersection.py:226-242)
 * - as further items of their queue, the vertices straight from memory, the arithmetic and its order those of road_kernel - and
 * csf_step_batch takes such members into its batched launch, one launch per vehicle class, priority rule and with / without road.  Bit
 * for bit what the two launches give.  Any other road keeps the launch of its own.  on = 0 (the default; CSF_MID_ROAD=1 in the environment
 * of csf_create turns it on from the start): every call takes the kernels it took before there was a switch.  CSF_E_ARG for e == NULL or
 * on outside 0 / 1; refused like csf_step while a calibration data set is held; a refused call changes nothing.
 * csf_mid_road_ticks: the ticks whose road term was summed inside the one-launch tick (csf_mid_ticks and, in a batch, csf_batch_mid_ticks
 * count them too). */
int csf_mid_road(csf_engine *e, int32_t on);
int csf_mid_road_ticks(const csf_engine *e, int64_t *n_ticks);
/* The one-launch tick for mid-size populations of SEVERAL PARAMETER SETS AND VEHICLE CLASSES (no change of
 * CSF_ABI_VERSION or csf_params: bind it where the library exports it).  A population that meets every other condition of csf_mid_ticks
 * but has more than one parameter set (csf_set_param_classes) or is of class CSF_UNCONTROLLED takes the general path: a pair launch and
 * one per-agent launch PER VEHICLE CLASS every tick, and inside a batch it is stepped in turn.  on = 1: such a population of at most
 * 1 024 road users without a CSF_BALANCINGRIDER set (257 ... 1 023 road users of ONE vehicle class whose road term is not summed inside the
 * launch keep the general path: measured slower) is ticked by mid_classes_kernel (csf_mid_classes.hip) - ONE launch per tick, the
 * workgroup of csf_mid_ticks, every source evaluated with the constants and the field of view of ITS set (staged in LDS), one pass of the
 * per-agent phases per vehicle class present, an UncontrolledVehicle following its script - and csf_step_batch steps all such members of
 * one priority rule and with / without road in ONE launch per tick whatever their classes.  With csf_mid_road on as well the launch sums
 * the road term of a small road itself (bit for bit what road_kernel leaves).  csf_mid_ticks, csf_batch_mid_ticks and csf_mid_road_ticks
 * count these ticks as they count the other one-launch ticks; csf_mid_classes_ticks counts them alone.  A single set of a rider class keeps
 * mid_tick_kernel bit for bit, switch or no switch; a population with a BalancingRider set keeps the general path.  on = 0 (the default;
 * CSF_MID_CLASSES=1 in the environment of csf_create turns it on from the start): every call takes the kernels it took before there was a
 * switch.  The results agree with the general path's within the rounding of the pair sum (its partial sums are formed per batch of 64
 * sources and added in fp64), not bit for bit.  CSF_E_ARG for e == NULL or on outside 0 / 1; refused like csf_step while a calibration
 * data set is held; a refused call changes nothing. */
int csf_mid_classes(csf_engine *e, int32_t on);
int csf_mid_classes_ticks(const csf_engine *e, int64_t *n_ticks);
/* Ticks whose per-agent launch ran BESIDE the pair launch that feeds it (ABI 9).  From a few thousand road users
 * of one TwoD-field class on one device, a tick of csf_step(e, n >= 4) is a pair launch on one of the engine's two streams and the
 * per-agent kernel on the other: every wave runs its destination-force phase (vehicle.py:1416-1558) at once and takes up the column
 * sums of its 64 road users (intersection.py:841-862) as soon as the pair workgroups that form them have arrived, while the rest of the
 * pair launch drains; the next tick's records go to the other half of a double buffer.  Bit-identical to the two launches in turn.
 * Per-tick calls, re-binning ticks, roads, history, shards and several parameter sets take the launches in turn.
 * Whether it pays depends on the runtime giving the engine's two streams hardware queues of their own (two streams on one queue
 * serialise, and the tick is then a launch LONGER): unless CSF_CHASE=0 (never) or 2 (always) says otherwise, an engine times three whole periods
 * between re-binnings (64 ticks each: in turn, side by side, in turn) in its first call of 200 ticks or more after tick 256 (clocks that
 * have come up; the mean of the two in-turn periods cancels what is left of the ramp) and keeps the faster - engines of the same kind created later in the process take the finding over - csf_chase_calibration: side_by_side 1 / -1 / 0 (not measured yet),
 * us_per_tick = {in turn, side by side} (0 when nothing was measured).  Both ways give the same states. */
int csf_chase_ticks(const csf_engine *e, int64_t *n_ticks);
int csf_chase_calibration(const csf_engine *e, int32_t *side_by_side, double us_per_tick[2]);

/* Arrivals that took the slot of a road user who had left from nearby (ABI 8).  Under traffic - road users arriving and leaving
 * every tick, intersection.py:458-634 - a slot freed inside a batch of the binned order is handed to the next arrival that starts
 * within that batch's bounding circle (up to CSF_HOLE_DIST median radii from its centre, [1.0]; CSF_HOLE_REUSE=0 switches it off):
 * the circle does not grow and the sentinel tail of the order, which every receiver tests source by source, fills more slowly. */
int csf_holes_taken(const csf_engine *e, int64_t *n);
/* csf_step(e, n_ticks) followed by csf_get_tick(...) in one call (ABI 6): what a caller that looks at every tick does -
 * SocialForceIntersection.step() refreshes vehicle.s, znav and force after each tick (intersection.py:866-896).  On the
 * one-wave path the kernel packs the read-back itself behind its last tick: one launch and one wait per call.  Arguments as
 * csf_get_tick's (any output may be NULL). */
int csf_step_get_tick(csf_engine *e, int64_t n_ticks, double *s_out, int32_t *dest_ptr, uint8_t *znav, double *Fx, double *Fy,
                      int64_t *tick);

/* Calibration on the device (calibration.py:243-526).  The optimiser of the reference calls its objective
 * hundreds of times; each call replays every recorded sequence with one candidate parameter set (:438-460) and sums an error over
 * the trajectories (:27-77).  csf_calib_load makes an EMPTY engine (capacity >= max_sets * n_seq, max_sets <= 256; one parameter
 * set, no road, no recording; not a member of a batch or of a communicator; not an UncontrolledVehicle's) hold a data set: n_seq
 * sequences of up to n_ticks ticks - their start states s0 [n_seq][n_states], the recorded forces Fx, Fy [n_ticks][n_seq], the
 * ticks of each (lengths [n_seq], 0 .. n_ticks; NULL: all of them), the objective [n_ticks][n_seq][n_feat] and the rows of
 * vehicle.traj its columns are compared with (feat [n_feat], 0 .. 5 = x, y, psi, v, delta, theta; a row the vehicle class does not have
 * compares 0, as the reference's traj holds 0 there).  It creates max_sets * n_seq road users - slot set * n_seq + seq - and keeps an
 * image of what csf_add_agents made of them.
 * csf_calib_eval evaluates n_sets <= max_sets candidate sets (checked as csf_create_v checks: params_size, abi_version; all of the
 * engine's vehicle class, t_s and traj_len) in ONE launch: every (set, sequence) starts from the image - an evaluation does not
 * depend on the one before -, replays its sequence through the per-agent tick of csf_replay_forces (fix_speed: calibration.py:455-458)
 * and sums, in fp64 and tick order, d = state after tick t - objective[t] over the features (no angle wrap): sums_out
 * [n_sets][n_seq][2] = (sum d^2, sum |d|).  calc_sse_timesteps is the sum of the first over the sequences, calc_maesse_samples the sum of
 * (second / (length * n_feat))^2.  states_out (may be NULL): [n_ticks / stride][n_sets * n_seq][n_states], the state after every
 * stride-th tick; a sequence that has ended keeps its last state.  Launches and copies per call do not depend on n_ticks, n_sets or
 * n_seq (csf_calib_launches counts the launches).  While the data set is held the engine refuses csf_step and every call that changes
 * the population or its parameters (CSF_E_STATE); the read-backs show the end of the last evaluation.  csf_set_dest_queue alone stays open
 * (on the device path and through the host mirror alike): a
 * fresh reference vehicle's only destination is its start (vehicle.py:183-185), and the Bicycle / TwoD / walking InvPendulum controllers
 * scale the desired speed within 3 m of the last destination (vehicle.py:1226-1232) - a data set recorded on a route is replayed with
 * that route's queue (no tick of a replay moves the queue pointer; the queue is not part of the image).  csf_calib_clear drops the
 * data set and empties the engine.  A refused call changes nothing. */
int csf_calib_load(csf_engine *e, int32_t n_seq, int64_t n_ticks, const double *s0, const double *Fx, const double *Fy, const int32_t *lengths,
                   const double *objective, int32_t n_feat, const int32_t *feat, int32_t max_sets);
int csf_calib_eval(csf_engine *e, int32_t n_sets, const csf_params *params, size_t params_size, int32_t abi_version, int32_t fix_speed,
                   double *sums_out, int32_t stride, double *states_out);
int csf_calib_launches(const csf_engine *e, int64_t *n_launches);
int csf_calib_clear(csf_engine *e);

/* Calibration of the interaction parameters on closed-loop scenes.  A replay of recorded forces (above) couples
 * no two vehicles, so the parameters of the social-force field - f_0, sigma_0..3, e_0, e_1, hfov, p_0, p_decay, the priority rule - act
 * only when the riders of a scene are simulated together.  csf_scene_calib_load makes an EMPTY engine (one parameter set, no road of its own, no
 * recording; not a member of a batch or of a communicator; not an UncontrolledVehicle's) hold a data set of n_scn scenes: scene q has
 * n_riders[q] road users (1 .. 32) of the engine's class, R = sum n_riders; per rider the start state s0 [R][n_states], v_desired [R] and a
 * destination queue in CSR form as csf_set_dest_queue takes it with reset = 1 (dest_offsets [R + 1], dest_xyz_stop rows of (x, y, stop); at
 * least one row each); per scene its ticks (lengths [n_scn], 0 .. n_ticks; NULL: all of them); the objective [n_ticks][R][n_feat] and the rows
 * of vehicle.traj its columns are compared with (feat [n_feat], 0 .. 5 = x, y, psi, v, delta, theta; a row the vehicle class does not have
 * compares 0).  The engine's capacity must be >= max_sets * R, max_sets <= 256.  It creates the max_sets * R road users - slot set * R +
 * rider, the scenes of a set one after the other - and keeps an image of every per-slot array that a closed-loop tick writes and a later
 * tick reads: the state, the integrator's side-state, ring column and status as csf_calib_load does, and with them the destination pointer,
 * the navigation state and its latched parameters, and the row of the short position ring that the spline planner reads first.
 * csf_scene_calib_eval evaluates n_sets <= max_sets candidate sets (checked as csf_create_v checks: params_size, abi_version; all of the
 * engine's vehicle class, t_s and traj_len; the priority rule is the set's own) in ONE launch, one workgroup of one wave per (set, scene):
 * it restores its scene from the image, runs the one-wave tick of csf_step (csf_small_ticks) for lengths[scene] ticks and adds after every
 * tick, per rider, in fp64 and tick order, d = state after tick t - objective[t][rider][f] over the features (no angle wrap): sums_out
 * [n_sets][R][2] = (sum d^2, sum |d|) PER RIDER - the caller adds the riders of a scene in rider order, so the order of every sum is fixed.
 * calc_sse_timesteps is the sum of the first over all riders; calc_maesse_samples the sum over the scenes of (sum of the second over the
 * scene's riders / (length * n_riders * n_feat))^2.  states_out (may be NULL): [n_ticks / stride][n_sets * R][n_states], the state after every
 * stride-th tick (stride >= 1); a scene that has ended keeps its last state.  An evaluation does not depend on the one before, on the place
 * of a set in the call or on the other sets in it; launches and copies per call do not depend on n_ticks, n_sets or the scenes
 * (csf_scene_calib_launches counts the launches).  While the data set is held the engine refuses csf_step and every call that changes the
 * population, its queues, its parameters or its recording, and csf_calib_load (CSF_E_STATE; csf_scene_calib_load refuses an engine that holds
 * the data set of csf_calib_load likewise); the read-backs show the end of the last evaluation.  csf_scene_calib_clear drops the data set and
 * empties the engine - through the host mirror, so that no dead slot stays behind and a small population added next takes the one-wave
 * tick of csf_step again.  A refused call changes nothing.
 *
 * csf_scene_calib_replay marks riders of the held data set that FOLLOW THEIR RECORDING instead of being fitted:
 * replayed [R] (non-zero: replayed; n_rep of them, numbered in rider order) and rows [n_ticks][n_rep][4] = (x, y, psi, v) of every replayed
 * rider AFTER tick t - the row alignment of the objective.  Such a rider starts from its s0 like every other (the recording's time 0), is
 * put on rows[t] behind every tick t < lengths[its scene] - what csf_push_state does to vehicle.s, with the unwrapped yaw and the position
 * ring kept consistent - and so acts on the others as a source of the candidate set's field only: its entries of sums_out are (0, 0), its
 * rows 0 .. 3 of states_out are the recording, its other rows and its status bits say nothing about the evaluation.  This is the ego
 * (leave-one-out) form of an evaluation, and how a road user that the candidate set cannot simulate enters a scene.  The rows read must be
 * finite (CSF_E_ARG); the rounding bands of an evaluation cover the largest recorded coordinate.  It may be called any number of times
 * between evaluations; replayed == NULL (or no non-zero entry) drops the replay, and evaluations are again what they are without one, bit
 * for bit.  rows may be NULL when nothing is replayed.  CSF_E_STATE without a closed-loop data set; everything that can fail runs before
 * anything is replaced.  csf_scene_calib_clear frees the replay with the rest.
 *
 * csf_scene_calib_road gives scenes of the held data set ROAD EDGES, shared by all candidate sets: the edges as
 * csf_set_road_vertices takes them (offsets [n_edges + 1], xy, F0 [n_edges], sigma [n_edges]) and edge_scene [n_edges], the scene of every
 * edge, non-decreasing; a scene without an entry has no road.  Every tick adds the road-edge force to every rider of such a scene
 * (intersection.py:226-242, 853-857) as the one-wave tick of csf_step does for an engine that holds the scene and its road: the road is
 * packed relative to the origin that engine would have.  A scene's road has at most 2 048 vertices and, padded to a multiple of 64, at most
 * 16 384 / P of them, P the power of two that holds the scene's riders.  It may be called any number of times between evaluations;
 * n_edges == 0 drops every road and evaluations are again what they are without one, bit for bit.  Refused with nothing changed:
 * CSF_E_STATE without a closed-loop data set (the data set of csf_calib_load included); CSF_E_ARG for a NULL array, a scene index out of
 * range or decreasing, offsets that run backwards, a value that is not finite, a road beyond those limits.  csf_scene_calib_load still
 * refuses an engine with a road of its own (csf_set_road_vertices).  csf_scene_calib_clear frees the roads with the rest.
 *
 * csf_scene_calib_eval_road is csf_scene_calib_eval with road parameters per candidate set: road_F0 [n_sets] and road_sigma [n_sets] replace
 * F0 and sigma of EVERY road vertex for that set (the reference's edges share one RoadElementParameters).  Both NULL: the loaded roads'
 * own values - csf_scene_calib_eval is this call with both NULL.  CSF_E_ARG for one array without the other, F0 < 0 or a value that is not
 * finite (csf_set_road_vertices places no other limit on sigma, and neither does this call); CSF_E_STATE when no scene has a road.
 *
 * csf_scene_calib_windows gives every rider of the held data set a PRESENCE WINDOW: enter [R] and exit [R], rider
 * r is in its scene at the ticks enter[r] <= t < exit[r], with 0 <= enter[r] <= exit[r] <= the length of its scene.  At every other tick
 * the rider is not there (intersection.py: add_vehicle / remove_vehicle between two steps): no other rider reads it as a source, it is not
 * ticked, not put on its recording (csf_scene_calib_replay), feels no road, and nothing is added to its sums.  Before its entry its slot
 * holds the fresh vehicle every evaluation starts from, so its row of s0 is its state at the start of tick enter[r]; after its exit the
 * slot keeps its last state, and the samples of states_out show what the slot holds.  enter[r] == exit[r]: never present, sums (0, 0).
 * Rows of the objective and of the replayed rows outside a rider's window are never used.  Both arrays NULL drops the windows, and
 * evaluations are again what they are without them, bit for bit; with windows every evaluation is still ONE launch.  The call is
 * independent of csf_scene_calib_replay and csf_scene_calib_road and of their order.  Refused with the held windows unchanged: CSF_E_STATE
 * without a closed-loop data set (the data set of csf_calib_load included); CSF_E_ARG for one array without the other or a bound outside
 * that range.  csf_scene_calib_clear frees the windows with the rest.
 *
 * csf_scene_calib_load_shared is csf_scene_calib_load for scenes whose ROSTER may exceed 32 road users as long as
 * at most 32 are present at a tick: n_riders[q] >= 1 without an upper bound of its own (R <= 2^24 in all), 1 <= n_lanes[q] <= 32 lanes of the one-wave tick, and per
 * rider its lane [R] (0 .. n_lanes - 1 of its scene) and its presence window enter [R], exit [R] as csf_scene_calib_windows takes them.
 * Riders of one lane take turns on it: the non-empty windows of two of them do not overlap (exit == enter of the next is a handover
 * without an idle tick: at that tick the first is gone and the second is the fresh vehicle).  A rider with enter == exit is never
 * present whatever its lane.  Every evaluation is still ONE launch; sums_out stays [n_sets][R][2] and states_out [samples][n_sets x R]
 * [n_states], both per RIDER: a row of states_out is written only at a sampled tick its rider is present at, every other row of it is
 * NaN, and a rider that is never present has the sums (0, 0).  The engine holds every rider once, the fresh vehicles the reset image
 * is taken from, and runs max_sets x sum(n_lanes) slots: its capacity must be >= max(R, max_sets x sum(n_lanes)).  The field-of-view
 * bands are sized from the starts of all R riders.  csf_scene_calib_replay (replayed [R]), csf_scene_calib_road (the vertex limit
 * is that of the scene's LANES), both evaluation calls, csf_scene_calib_launches and csf_scene_calib_clear work as on any data set;
 * csf_scene_calib_windows is refused with CSF_E_STATE, because the windows belong to the load.  Refused with the engine empty and
 * usable: everything csf_scene_calib_load refuses, and CSF_E_ARG for a lane count or a lane out of range, a window outside 0 <= enter
 * <= exit <= the length of the scene, or two riders of one lane whose non-empty windows overlap.
 *
 * csf_scene_calib_load_wide is csf_scene_calib_load_shared for scenes with MORE THAN 32 ROAD USERS AT ONCE:
 * 1 <= n_lanes[q] <= 256, and wide_from (1 .. 257) decides per scene which kernel runs it.  A scene with n_lanes[q] >= wide_from is WIDE:
 * one workgroup of 256 threads per (set, scene) simulates it closed loop for all its ticks - the tick of the one-wave path with the all-to-all
 * dependence carried through LDS and workgroup barriers, P = 64, 128 or 256 the power of two that holds its lanes.  Every other scene
 * runs on the one-wave tick exactly as after csf_scene_calib_load_shared, bit for bit.  33 is the natural wide_from - the smallest scene the
 * one-wave tick cannot take; it is NOT a measured crossover -, 1 sends every scene to the wide kernel, a tuning knob, and above 33 a
 * scene of more than 32 lanes that stays below wide_from is refused (CSF_E_ARG: the one-wave tick cannot take it).  An evaluation launches, on one stream, the kernel of the narrow
 * scenes if there are any and then the kernel of the wide ones if there are any - still one copy in and one wait -, and
 * csf_scene_calib_launches counts each kernel launched.  A wide scene differs from the same scene on the one-wave tick in the order of
 * the fp64 sums of the pair term (and of the fp32 sums of the road term) alone.  csf_scene_calib_road reads its rule with the P above: a wide scene
 * takes 256, 128 or 64 vertices (padded).  csf_scene_calib_replay, both evaluation calls, csf_scene_calib_launches, csf_scene_calib_clear and the
 * refusals while a data set is held are those of any data set; csf_scene_calib_windows is refused as after csf_scene_calib_load_shared.
 * Refused with the engine empty and usable: everything csf_scene_calib_load_shared refuses with 256 in the place of 32, and CSF_E_ARG
 * for wide_from outside 1 .. 257.  csf_scene_calib_load and csf_scene_calib_load_shared keep their limit of 32.
 *
 * csf_scene_calib_groups gives the riders of the held data set GROUPS that carry parameter sets of their own -
 * e-bikes and city bikes, commuters and children: group [R] holds 0 .. n_groups - 1 per rider, n_groups <= 4.  It may be called any
 * number of times between evaluations on an engine that holds a csf_scene_calib_load data set; NULL or n_groups <= 1 drops the groups, and
 * evaluations are then what they were, bit for bit.  Refused with a message and nothing changed: CSF_E_STATE without a closed-loop data
 * set (the data set of csf_calib_load included) and after csf_scene_calib_load_shared / _load_wide; CSF_E_ARG for n_groups > 4 and for an
 * entry >= n_groups.  Device buffers are allocated and filled before anything is replaced; csf_scene_calib_clear frees them.
 *
 * csf_scene_calib_eval_groups evaluates n_sets candidates of n_groups parameter sets each: params [n_sets][n_groups], record (k, g) what
 * the riders of group g carry in candidate k; everything else - road_F0 / road_sigma (NULL or [n_sets], per candidate), sums_out,
 * stride, states_out and their layout - is csf_scene_calib_eval_road's.  A rider is ticked with its own record and restored with its
 * limits; as a source of the field it acts with its own record's field and field of view (intersection.py:733-735, 815), replayed riders
 * included; the priority rule of a candidate is record (k, 0)'s (it belongs to the intersection, as under csf_set_param_classes) and
 * the rounding bands take the largest speed clamp among the candidate's records.  n_groups must equal the loaded one (CSF_E_ARG), every
 * record is checked as csf_scene_calib_eval checks a set and must be of the engine's vehicle class (CSF_E_ARG).  Without loaded groups
 * n_groups must be 1 and the call IS csf_scene_calib_eval_road.  While groups are loaded csf_scene_calib_eval and
 * csf_scene_calib_eval_road are refused with CSF_E_STATE: one set cannot say what group 1 carries.
 *
 * csf_scene_calib_lane_groups is csf_scene_calib_groups for a data set of csf_scene_calib_load_shared /
 * csf_scene_calib_load_wide: group [R] per RIDER as there, and a lane's parameters change with the rider it carries - at a takeover the
 * lane's slot is restored with the newcomer's limits, it is ticked with the newcomer's record and acts as a source with that record's
 * field and field of view.  The evaluation is csf_scene_calib_eval_groups, on the kernels of the shared and the wide scenes (one launch,
 * or up to two after csf_scene_calib_load_wide); presence windows, replay, roads, samples and sums are what they are without groups.
 * NULL or n_groups <= 1 drops the groups, and evaluations are then what they were, bit for bit.  The checks, the allocate-before-replace
 * order and the refusals are csf_scene_calib_groups's, but for the data set: CSF_E_STATE on a plain csf_scene_calib_load data set (that one
 * takes csf_scene_calib_groups), without a closed-loop data set and with csf_calib_load's; CSF_E_ARG for n_groups > 4 and for an entry
 * >= n_groups.  csf_scene_calib_clear frees the groups with the rest.  csf_scene_calib_groups keeps its refusal on such a data set.
 *
 * csf_scene_calib_classes gives the riders of a csf_scene_calib_load data set groups of DIFFERENT VEHICLE CLASSES -
 * a Bicycle among TwoDBicycles, a BalancingRiderBicycle among InvPendulumBicycles, all simulated: group [R] holds 0 .. n_groups - 1 per
 * rider, 2 <= n_groups <= 12 (six classes x two kinds of rider), models [n_groups] the enum csf_model of every group (not
 * CSF_UNCONTROLLED; the engine's own class need not be among them) and s0 [R][8] the start states in the WIDEST layout (x, y, psi, v,
 * delta, theta, steer rate, roll rate) - the load kept the columns of the engine's class only.  The call rewrites the reset image per
 * rider: the state rows its class has (the others 0), the integrator's side state of that class and the first row of the position ring,
 * as csf_add_agents makes them for a fresh vehicle of that class.  While classes are held csf_num_states - and the layout of states_out
 * and of the read-backs - is the widest of the LOADED classes, and rows a class lacks stay 0.  The evaluation is
 * csf_scene_calib_eval_groups with params [n_sets][n_groups] and params[k * n_groups + g].model == models[g] (CSF_E_ARG names set, group
 * and both classes): ONE launch, a rider is ticked by the per-agent tick of its class with its own record, restored with its limits, and
 * acts as a source with the field of ITS class - the Bicycle's or the TwoD one - and its record's field of view (intersection.py:797-823);
 * the priority rule of a candidate is record (k, 0)'s.  csf_scene_calib_eval / _eval_road are refused (CSF_E_STATE) as under groups.
 * Replay (a replayed BalancingRider keeps its unwrapped yaw consistent as csf_push_state does), windows, roads and road parameters per
 * candidate, loaded before or after, work as without classes.  The call replaces groups loaded by csf_scene_calib_groups, and that call
 * replaces these; (NULL, 0, NULL, NULL) drops the classes - the data set is what it was after the load, evaluations bit for bit what
 * they were.  Everything is validated and allocated before anything is replaced: a refused call leaves the held groups or classes in
 * force.  CSF_E_STATE without a closed-loop data set and on a data set of csf_scene_calib_load_shared / _load_wide (mixed classes need
 * csf_scene_calib_load); CSF_E_ARG for n_groups outside 2 .. 12, an entry of group >= n_groups, an entry of models outside the six classes,
 * a NULL array.  csf_scene_calib_clear frees the classes with the rest.
 *
 * csf_scene_calib_lane_classes is csf_scene_calib_classes for a data set of csf_scene_calib_load_shared /
 * csf_scene_calib_load_wide: the same arguments and limits, the same rewritten image, and the class is a property of the RIDER a lane
 * carries - at a takeover the lane's slot becomes the newcomer's fresh vehicle of ITS class (rows that class lacks are 0), from that tick
 * on the lane is ticked by that class's per-agent tick, acts as a source with that class's field and, replayed, takes that class's
 * write-back.  A lane nobody rides yet has group 0 and is never present.  The evaluation is csf_scene_calib_eval_groups on
 * scene_lanes_mixed_kernel / scene_wide_mixed_kernel: one launch, or up to two after csf_scene_calib_load_wide.  The call replaces the
 * groups of csf_scene_calib_lane_groups, and that call replaces these; (NULL, 0, NULL, NULL) drops the classes.  CSF_E_STATE on a plain
 * csf_scene_calib_load data set (that one takes csf_scene_calib_classes), without a closed-loop data set and with csf_calib_load's;
 * CSF_E_ARG as csf_scene_calib_classes.  A refused call changes nothing.  csf_scene_calib_classes keeps its refusal on such a data set. */
int csf_scene_calib_classes(csf_engine *e, const uint8_t *group, int32_t n_groups, const int32_t *models, const double *s0);
int csf_scene_calib_lane_classes(csf_engine *e, const uint8_t *group, int32_t n_groups, const int32_t *models, const double *s0);
int csf_scene_calib_groups(csf_engine *e, const uint8_t *group, int32_t n_groups);
int csf_scene_calib_lane_groups(csf_engine *e, const uint8_t *group, int32_t n_groups);
int csf_scene_calib_eval_groups(csf_engine *e, int32_t n_sets, int32_t n_groups, const csf_params *params,
                                size_t params_size, int32_t abi_version,
                                const double *road_F0, const double *road_sigma,
                                double *sums_out, int32_t stride, double *states_out);
int csf_scene_calib_load_wide(csf_engine *e, int32_t n_scn, const int32_t *n_riders, const int32_t *n_lanes,
                              const int32_t *lane, const int32_t *enter, const int32_t *exit, int64_t n_ticks,
                              const double *s0, const double *v_desired,
                              const int64_t *dest_offsets, const double *dest_xyz_stop,
                              const int32_t *lengths, const double *objective,
                              int32_t n_feat, const int32_t *feat, int32_t max_sets, int32_t wide_from);
int csf_scene_calib_load_shared(csf_engine *e, int32_t n_scn, const int32_t *n_riders, const int32_t *n_lanes,
                                const int32_t *lane, const int32_t *enter, const int32_t *exit, int64_t n_ticks,
                                const double *s0, const double *v_desired,
                                const int64_t *dest_offsets, const double *dest_xyz_stop,
                                const int32_t *lengths, const double *objective,
                                int32_t n_feat, const int32_t *feat, int32_t max_sets);
int csf_scene_calib_load(csf_engine *e, int32_t n_scn, const int32_t *n_riders, int64_t n_ticks,
                         const double *s0, const double *v_desired,
                         const int64_t *dest_offsets, const double *dest_xyz_stop,
                         const int32_t *lengths, const double *objective,
                         int32_t n_feat, const int32_t *feat, int32_t max_sets);
int csf_scene_calib_eval(csf_engine *e, int32_t n_sets, const csf_params *params,
                         size_t params_size, int32_t abi_version,
                         double *sums_out, int32_t stride, double *states_out);
int csf_scene_calib_eval_road(csf_engine *e, int32_t n_sets, const csf_params *params,
                              size_t params_size, int32_t abi_version,
                              const double *road_F0, const double *road_sigma,
                              double *sums_out, int32_t stride, double *states_out);
int csf_scene_calib_replay(csf_engine *e, const uint8_t *replayed, const double *rows);
int csf_scene_calib_road(csf_engine *e, int32_t n_edges, const int32_t *edge_scene, const int64_t *offsets,
                         const double *xy, const double *F0, const double *sigma);
int csf_scene_calib_windows(csf_engine *e, const int32_t *enter, const int32_t *exit);
int csf_scene_calib_launches(const csf_engine *e, int64_t *n_launches);
int csf_scene_calib_clear(csf_engine *e);

/* Far-field radius of the pair kernel (metres; +inf when the cull is off).  The repulsive field of
 * vehicle.py:1560-1648 decays at least like f_0 exp(-kappa rho); sources beyond
 * R = ln(n / eps) / kappa together add less than eps * f_0 (eps = 2^-24 unless the environment variable
 * CSF_FAR_EPS says otherwise; CSF_FAR_EPS=0 evaluates every pair) to a receiver's force, which is below
 * the resolution of the fp32 column sum; batches of binned source records entirely beyond R are skipped.
 * The reference has no such cut-off: this is the engine's only approximation besides fp32. */
int csf_far_radius(const csf_engine *e, double *radius_m);

#ifdef __cplusplus
}
#endif
#endif /* CSF_H */
