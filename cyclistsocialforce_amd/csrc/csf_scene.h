// csf_scene.h — what the closed-loop calibration kernel (csf_scene.hip: scene_eval_kernel) is handed beside the table of Dev views,
// shared with the host side (engine/abi_scene.inc).
#pragma once
#include "csf_calib.h"

namespace csf {

// One candidate parameter set of a call, as the one-wave tick reads it from Dev: the set, what derive_pair_consts / the rounding
// bands make of it, and the PlanarBicycle step matrices (derive_planarbike).  The host composes n_sets of them per call.
struct SceneSet {
    csf_params p;
    PairConsts pc;
    double pb[7];
    // csf_scene_calib_eval_road: what this set puts in place of (-F0, -(sigma + 1) / 2) of every road vertex, and the Dev::road_np of
    // its sigma.  Read only when SceneDev::road_blk is set.
    float road_z, road_w;
    int32_t road_np, pad[3];
};

// Rider groups (csf_scene_calib_groups): the riders of a scene carry one of up to SCENE_GROUPS_MAX parameter sets of the
// engine's vehicle class.  The call's table of sets is then [n_sets][n_groups] SceneSet records, record (set, g) what group g carries in
// candidate set `set`; the road entries and the rounding bands of a set are the same in all of its records, and so is the priority rule
// (record 0's: the rule belongs to the intersection, as under csf_set_param_classes).
constexpr int SCENE_GROUPS_MAX = 4;

// Several vehicle classes in one scene (csf_scene_calib_classes): the groups are then also of different vehicle classes -
// record (set, g) names the class of group g -, and the call takes up to SCENE_CLASS_GROUPS_MAX of them: six classes x two kinds of rider.
// Every other call keeps SCENE_GROUPS_MAX.
constexpr int SCENE_CLASS_GROUPS_MAX = 12;

// The data set of csf_scene_calib_load, resident on the device, and the reset image.  The image is indexed by RIDER (0 .. R - 1,
// the scenes one after the other): every set starts every scene from the same state, so one copy of what csf_add_agents made of
// the first set's slots serves all of them.  It holds every per-slot array that a closed-loop tick (agent_body<.., FUSED = true>
// under small_tick_body) writes and a later tick reads:
//   s [STATE_ROWS], lti [5], ppsi, ti, status      as csf_calib.h
//   ptr, znav, znp [3]                             the destination pointer, the navigation state and its latched parameters
//   hx0, hy0                                       row 0 of the short position ring - the only row a tick reads before a tick of
//                                                  the same evaluation has written it (ti starts at 0: load_ring, twod_dest)
// zrid and dgood follow from the image's state and the limits of the evaluation's own set (vehicle.py:1732-1736).  The force
// rows are written before they are read in every tick; they are cleared so that the read-backs of a scene of length 0 show
// nothing of the evaluation before.  The fp32 records are written and never read by the one-wave tick.
struct SceneDev {
    const double *obj;           // [n_ticks][R][n_feat]
    const int32_t *len;          // [n_scn] ticks of every scene (0 .. n_ticks)
    const int32_t *roff;         // [n_scn + 1] first rider of every scene
    int32_t n_scn, n_ticks, n_feat, R;
    int32_t feat[CALIB_MAX_FEAT];
    int64_t img_cap;             // stride of the image's rows
    const double *img_s, *img_lti, *img_ppsi, *img_znp, *img_hx0, *img_hy0;
    const int32_t *img_ti, *img_ptr;
    const uint32_t *img_status;
    const uint8_t *img_znav;
    double2 *sums;               // [n_sets][R] (sum d^2, sum |d|) per rider: mapped host memory
    double *states;              // [n_ticks / stride][n_sets * R][ns], NULL: none
    int32_t stride, n_samples, n_sets, n_rep;
    // Riders that follow their recording (csf_scene_calib_replay): they are put on their recorded (x, y, psi, v) behind every tick
    // and act as sources of the field only; no error is summed for them.  rep == NULL: no rider is replayed.
    const int32_t *rep_index;    // [R] -1: simulated, else the rider's column of rep
    const double *rep;           // [n_ticks][n_rep][4] (x, y, psi, v) AFTER tick t: the row alignment of obj
    // Scene roads (csf_scene_calib_road).  The view of a scene with a road points rv / rvo at the scene's part of
    // road_rv / its tile origins.  With road parameters per candidate set (road_blk != NULL) workgroup (set, scene) first writes the
    // scene's road with the set's (road_z, road_w) to ITS block road_blk + set * road_stride + (rv - road_rv) and stages from there.
    const float4 *road_rv;       // the packed roads of all scenes, one after the other (NULL: no scene has a road)
    float4 *road_blk;            // [n_sets][road_stride], NULL: the roads keep their own parameters
    int64_t road_stride;         // vertices (padded) of all scenes together
    uint32_t road_lds;           // bytes of dynamic LDS: the largest nv_pad of the data set x 16
    // Presence windows (csf_scene_calib_windows): rider r is in its scene at the ticks win_enter[r] <= t < win_exit[r]
    // and at every other tick neither source nor receiver, not ticked, not replayed and not summed.  NULL: no windows - everybody is
    // there from tick 0 to the scene's last, and the launch is the instance without a mask.
    const int32_t *win_enter, *win_exit;   // [R]
    // Shared lanes (csf_scene_calib_load_shared), read by scene_lanes_kernel only.  The view of a scene has n = its
    // LANES, slot = set * Lsum + lane_off[scene] + lane (Lsum: the lanes of all scenes; the table's views hold it), and a lane carries the riders of its chain one after the other: lane_first,
    // then rider_next of the rider it carries, -1 ends the chain.  A chain holds riders of the lane's scene with a non-empty window,
    // in entry order, the windows of two neighbours not overlapping; a rider that is never present is in no chain.  The image then
    // also holds what was constant per slot while a slot had one rider and agent_body<.., FUSED = true> reads:
    //   vdes, qbeg, qlen                               the desired speed and the rider's destination queue in Dev::q
    const int32_t *lane_off;     // [n_scn + 1] first lane of every scene (NULL: the data set does not share lanes)
    const int32_t *lane_first;   // [Lsum] rider (0 .. R - 1) a lane carries first, -1: nobody
    const int32_t *rider_next;   // [R] who takes the lane over from this rider, -1: nobody
    const double *img_vdes;
    const int64_t *img_qbeg;
    const int32_t *img_qlen;
    // Rider groups (csf_scene_calib_groups), read by scene_groups_kernel - and, on shared lanes (csf_scene_calib_lane_groups;
    // DESIGN.md 4.10h), by scene_lanes_groups_kernel / scene_wide_groups_kernel - only: the group of every rider, and the sets are
    // [n_sets][n_groups] records.  NULL: no groups - every rider carries record `set` of [n_sets], and the launch is today's.
    const uint8_t *group;        // [R] 0 .. n_groups - 1
    int32_t n_groups;            // 2 .. SCENE_GROUPS_MAX with `group` (the kernels of csf_scene_mixed.hip: 2 .. SCENE_CLASS_GROUPS_MAX), else 0
};

// Wide scenes (csf_scene_calib_load_wide): a data set on shared lanes whose scenes with n_lanes >= wide_from run on
// scene_wide_kernel - one workgroup of 256 threads per (set, scene), up to WIDE_MAX lanes - and the others on scene_lanes_kernel as
// after csf_scene_calib_load_shared.  SceneDev stays the record of the whole data set (scene_wide_kernel reads it by scene index);
// scene_lanes_kernel is handed the NARROW scenes alone, compacted: its own table, lengths, lane offsets and first riders.  roff_n[k + 1]
// is the first rider of the NEXT narrow scene (of the data set's end behind the last), so the kernel's loop over the riders that are
// never present may also write the (0, 0) of such riders of a wide scene in between - the value scene_wide_kernel writes there too,
// later on the same stream.
struct SceneWideDev {
    const Dev *table_w;          // [n_sets][n_wide] the views of the wide scenes
    const int32_t *scn_w;        // [n_wide] their scene index
    int32_t n_wide, n_narrow;
    const int32_t *len_n, *roff_n, *lane_off_n;   // [n_narrow], [n_narrow + 1], [n_narrow]: what scene_lanes_kernel reads per scene
};

// One evaluation: workgroup b = set * n_scn + scene runs the scene of table[b] with the constants of sets[set].  With `w` (a wide load)
// `table` holds the narrow scenes and up to two kernels are launched on `st`, the narrow scenes first.  Returns the kernels launched.
int launch_scene_eval(int model, const Dev *table, const SceneSet *sets, const SceneDev &c, hipStream_t st, const SceneWideDev *w = nullptr);

// One evaluation with vehicle classes loaded: scene_mixed_kernel on a csf_scene_calib_load data set (csf_scene_calib_classes), `ns` the
// widest state of the loaded classes; scene_lanes_mixed_kernel on shared lanes (csf_scene_calib_lane_classes: c.lane_off is set) and, with
// `w` (a wide load), the narrow scenes on it and then the wide ones on scene_wide_mixed_kernel.  Returns the kernels launched (0 .. 2).
int launch_scene_mixed(const Dev *table, const SceneSet *sets, const SceneDev &c, int ns, hipStream_t st, const SceneWideDev *w = nullptr);

}  // namespace csf
