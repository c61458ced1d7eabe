"""ctypes binding of libcsf_hip.so (include/csf.h).

The library is the only compute path of this package: if it is missing or cannot be loaded the import of
the engine fails loudly — there is no NumPy/CPU fallback.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# CSF_LIB selects another build of the same library (kernel A/B measurements, tools/ab.sh)
LIB_PATH = os.environ.get("CSF_LIB") or os.path.join(HERE, "libcsf_hip.so")

BICYCLE, TWOD, INVPEND, PLANARPOINT, PLANARBIKE, UNCONTROLLED, BALANCINGRIDER = 0, 1, 2, 3, 4, 5, 6
UNREGULATED, P2R = 0, 1
N_STATES = {BICYCLE: 5, TWOD: 5, INVPEND: 6, PLANARPOINT: 4, PLANARBIKE: 5, UNCONTROLLED: 4, BALANCINGRIDER: 8}
UNIQUE_ID_BYTES = 128
ST_SPLINE, ST_NAN, ST_NAVSTATE, ST_UNCONTROLLABLE = 1, 2, 4, 8

# every symbol include/csf.h declares (tests check that the library exports all of them)
SYMBOLS = (
    "csf_create", "csf_destroy", "csf_last_error", "csf_abi_version", "csf_add_agents", "csf_remove_agents",
    "csf_set_dest_queue", "csf_set_road_vertices", "csf_set_params", "csf_set_param_classes", "csf_set_agent_class", "csf_set_v_desired",
    "csf_set_priority_rule", "csf_push_state", "csf_num_agents", "csf_num_states", "csf_step", "csf_sync",
    "csf_calc_forces", "csf_apply_forces", "csf_replay_forces", "csf_dest_force", "csf_get_state", "csf_get_forces",
    "csf_get_force_parts", "csf_status", "csf_enable_history", "csf_get_history", "csf_pair_force",
    "csf_comm_unique_id", "csf_comm_init", "csf_shard_range", "csf_profile_enable", "csf_profile_read",
    "csf_far_radius", "csf_get_tick", "csf_profile_gather", "csf_profile_kernels", "csf_profile_samples",
    "csf_count_pairs", "csf_comm_init_loopback", "csf_step_group", "csf_untracked", "csf_update_destination",
    "csf_update_nav_state", "csf_set_dest_pointer", "csf_set_incremental", "csf_set_script", "csf_near_dropped", "csf_comm_stream_order", "csf_small_ticks", "csf_step_get_tick",
    "csf_get_integrator_state", "csf_set_integrator_state", "csf_mid_ticks", "csf_holes_taken",
    "csf_create_v", "csf_params_size", "csf_profile_samples_of", "csf_chase_ticks", "csf_chase_calibration", "csf_replace_agents",
    "csf_batch_join", "csf_batch_leave", "csf_step_batch", "csf_step_batch_get_tick", "csf_batch_ticks",
    "csf_batch_mid_ticks", "csf_batch_launches",
    "csf_record", "csf_get_record", "csf_batch_get_record",
    "csf_calib_load", "csf_calib_eval", "csf_calib_launches", "csf_calib_clear",
    "csf_scene_calib_load", "csf_scene_calib_eval", "csf_scene_calib_launches", "csf_scene_calib_clear",
    "csf_scene_calib_replay",
    "csf_scene_calib_road", "csf_scene_calib_eval_road",
    "csf_scene_calib_windows",
    "csf_scene_calib_load_shared",
    "csf_scene_calib_load_wide",
    "csf_scene_calib_groups", "csf_scene_calib_eval_groups",
    "csf_scene_calib_lane_groups",
    "csf_scene_calib_classes",
    "csf_scene_calib_lane_classes",
    "csf_small_classes",
    "csf_mid_road", "csf_mid_road_ticks",
    "csf_mid_classes", "csf_mid_classes_ticks",
    "csf_handout_ranks",
    "csf_wg_order_ranks", "csf_wg_order_tables",
    "csf_pair_shape_of", "csf_pair_shape_words",
    "csf_field_map", "csf_field_map_launches",
    "csf_encounters", "csf_batch_encounters", "csf_encounter_launches",
    "csf_post_encroachment", "csf_batch_post_encroachment", "csf_pet_launches",
    "csf_passing", "csf_batch_passing", "csf_passing_launches",
    "csf_flow", "csf_batch_flow", "csf_flow_launches",
    "csf_clearance", "csf_batch_clearance", "csf_clearance_launches",
    "csf_body_encounters", "csf_batch_body_encounters", "csf_body_encounter_launches",
)
ABI_VERSION = 9
REC_STATE, REC_FORCE = 1, 2
FIELD_CROWD, FIELD_ROAD, FIELD_FOV = 1, 2, 4


class Params(C.Structure):
    """csf_params of include/csf.h (field order is ABI)."""

    _fields_ = [
        ("t_s", C.c_double), ("d_arrived_inter", C.c_double), ("d_arrived_stop", C.c_double),
        ("v_max_stop", C.c_double), ("v_max_harddecel", C.c_double), ("hfov", C.c_double),
        ("f_0", C.c_double), ("e_0", C.c_double), ("e_1", C.c_double),
        ("sigma_0", C.c_double), ("sigma_1", C.c_double), ("sigma_2", C.c_double), ("sigma_3", C.c_double),
        ("v_max_riding", C.c_double * 2), ("p_decay", C.c_double), ("p_0", C.c_double),
        ("l", C.c_double), ("l_2", C.c_double), ("delta_max", C.c_double),
        ("a_max", C.c_double * 2), ("a_desired_default", C.c_double * 2),
        ("k_p_v", C.c_double), ("k_p_delta", C.c_double), ("g", C.c_double),
        ("h", C.c_double), ("m", C.c_double), ("i_bike_longlong", C.c_double),
        ("i_steer_vertvert", C.c_double), ("c_steer", C.c_double),
        ("v_max_walk", C.c_double), ("delta_max_walk", C.c_double),
        ("k_psi", C.c_double), ("pb_poles", C.c_double * 4),
        ("br_minv_k0g", C.c_double * 4), ("br_minv_k2", C.c_double * 4), ("br_minv_c1", C.c_double * 4),
        ("br_minv_steer", C.c_double * 2), ("br_yaw", C.c_double * 2), ("br_pole_fun", C.c_double * 10), ("br_gains", C.c_double * 5),
        ("model", C.c_int32), ("priority_rule", C.c_int32), ("traj_len", C.c_int32), ("br_mode", C.c_int32),
    ]


class TickOut(C.Structure):
    """csf_tick_out of include/csf.h: the outputs of csf_get_tick for one member of a batch (any may be NULL)."""

    _fields_ = [("s_out", C.c_void_p), ("dest_ptr", C.c_void_p), ("znav", C.c_void_p), ("Fx", C.c_void_p), ("Fy", C.c_void_p),
                ("tick", C.POINTER(C.c_int64))]


class RecordOut(C.Structure):
    """csf_record_out of include/csf.h: where the last samples of one member of a batch go (s and F NULL: the member is left out)."""

    _fields_ = [("s", C.c_void_p), ("F", C.c_void_p), ("first_sample", C.POINTER(C.c_int64))]


class EncounterEvent(C.Structure):
    """csf_encounter_event of include/csf.h: a (sample, i < j) under a threshold"""

    _fields_ = [("sample", C.c_int64), ("i", C.c_int32), ("j", C.c_int32), ("d", C.c_double), ("ttc", C.c_double)]


class EncounterOut(C.Structure):
    """csf_encounter_out of include/csf.h: where the encounter measures of one engine go (any pointer may be NULL)"""

    _fields_ = [("d_min", C.c_void_p), ("d_with", C.c_void_p), ("ttc_min", C.c_void_p), ("ttc_with", C.c_void_p),
                ("run_d_min", C.c_void_p), ("run_d_with", C.c_void_p), ("run_d_sample", C.c_void_p),
                ("run_ttc_min", C.c_void_p), ("run_ttc_with", C.c_void_p), ("run_ttc_sample", C.c_void_p),
                ("events", C.c_void_p), ("event_capacity", C.c_int64), ("n_events", C.c_int64), ("first_sample", C.c_int64)]


class PetEvent(C.Structure):
    """csf_pet_event of include/csf.h: a crossing of the paths of i < j under the threshold, as i reports it"""

    _fields_ = [("i", C.c_int32), ("j", C.c_int32), ("k", C.c_int32), ("l", C.c_int32),
                ("t_i", C.c_double), ("t_j", C.c_double), ("x", C.c_double), ("y", C.c_double)]


class PetOut(C.Structure):
    """csf_pet_out of include/csf.h: where the path crossings of one engine go (any pointer may be NULL)"""

    _fields_ = [("seg_pet", C.c_void_p), ("seg_with", C.c_void_p), ("seg_t_own", C.c_void_p), ("seg_t_with", C.c_void_p),
                ("run_pet", C.c_void_p), ("run_with", C.c_void_p), ("run_t_own", C.c_void_p), ("run_t_with", C.c_void_p),
                ("run_x", C.c_void_p), ("run_y", C.c_void_p), ("run_count", C.c_void_p),
                ("events", C.c_void_p), ("event_capacity", C.c_int64), ("n_events", C.c_int64), ("first_sample", C.c_int64)]


class PassingEvent(C.Structure):
    """csf_passing_event of include/csf.h: i passes j in interval k under the threshold, as i reports it"""

    _fields_ = [("i", C.c_int32), ("j", C.c_int32), ("k", C.c_int32), ("kind", C.c_int32),
                ("t", C.c_double), ("lat", C.c_double), ("closing", C.c_double), ("cosine", C.c_double)]


class PassingOut(C.Structure):
    """csf_passing_out of include/csf.h: where the gaps and passings of one engine go (any pointer may be NULL)"""

    _fields_ = [("gap", C.c_void_p), ("gap_with", C.c_void_p), ("thw", C.c_void_p),
                ("made_lat", C.c_void_p), ("made_with", C.c_void_p), ("made_t", C.c_void_p), ("made_kind", C.c_void_p),
                ("by_lat", C.c_void_p), ("by_with", C.c_void_p), ("by_t", C.c_void_p), ("by_kind", C.c_void_p),
                ("run_gap", C.c_void_p), ("run_gap_with", C.c_void_p), ("run_gap_k", C.c_void_p),
                ("run_thw", C.c_void_p), ("run_thw_with", C.c_void_p), ("run_thw_k", C.c_void_p),
                ("run_made_lat", C.c_void_p), ("run_made_with", C.c_void_p), ("run_made_t", C.c_void_p), ("run_made_kind", C.c_void_p),
                ("run_by_lat", C.c_void_p), ("run_by_with", C.c_void_p), ("run_by_t", C.c_void_p), ("run_by_kind", C.c_void_p),
                ("run_made", C.c_void_p), ("run_by", C.c_void_p),
                ("events", C.c_void_p), ("event_capacity", C.c_int64), ("n_events", C.c_int64), ("first_sample", C.c_int64)]


class FlowLayout(C.Structure):
    """csf_flow_layout of include/csf.h: the counting lines, areas and grid every member of a call is measured at"""

    _fields_ = [("lines", C.c_void_p), ("areas", C.c_void_p), ("n_lines", C.c_int32), ("n_areas", C.c_int32),
                ("x0", C.c_double), ("y0", C.c_double), ("h", C.c_double), ("nx", C.c_int32), ("ny", C.c_int32)]


class FlowEvent(C.Structure):
    """csf_flow_event of include/csf.h: road user i crosses line l in interval k"""

    _fields_ = [("i", C.c_int32), ("l", C.c_int32), ("k", C.c_int32), ("dir", C.c_int32),
                ("t", C.c_double), ("u", C.c_double), ("speed", C.c_double)]


class FlowOut(C.Structure):
    """csf_flow_out of include/csf.h: where the crossings and occupancies of one engine go (any pointer may be NULL)"""

    _fields_ = [("line_count", C.c_void_p), ("cross_n", C.c_void_p),
                ("first_t", C.c_void_p), ("first_u", C.c_void_p), ("first_speed", C.c_void_p), ("first_dir", C.c_void_p),
                ("occupancy", C.c_void_p), ("in_samples", C.c_void_p), ("in_first", C.c_void_p), ("in_last", C.c_void_p), ("in_dist", C.c_void_p),
                ("grid_count", C.c_void_p),
                ("events", C.c_void_p), ("event_capacity", C.c_int64), ("n_events", C.c_int64), ("n_outside", C.c_int64), ("first_sample", C.c_int64)]


class ClearanceRoad(C.Structure):
    """csf_clearance_road of include/csf.h: the polylines every member of a call is measured against"""

    _fields_ = [("offsets", C.c_void_p), ("xy", C.c_void_p), ("n_edges", C.c_int32)]


class ClearanceEvent(C.Structure):
    """csf_clearance_event of include/csf.h: road user i crosses segment (edge, seg) at station k"""

    _fields_ = [("i", C.c_int32), ("k", C.c_int32), ("edge", C.c_int32), ("seg", C.c_int32), ("dir", C.c_int32),
                ("t", C.c_double), ("u", C.c_double)]


class ClearanceOut(C.Structure):
    """csf_clearance_out of include/csf.h: where the edge distances and crossings of one engine go (any pointer may be NULL)"""

    _fields_ = [("d", C.c_void_p), ("edge", C.c_void_p), ("seg", C.c_void_p), ("t", C.c_void_p),
                ("left", C.c_void_p), ("right", C.c_void_p), ("left_edge", C.c_void_p), ("right_edge", C.c_void_p), ("cross", C.c_void_p),
                ("d_min", C.c_void_p), ("d_min_k", C.c_void_p), ("d_min_edge", C.c_void_p), ("d_min_seg", C.c_void_p),
                ("left_min", C.c_void_p), ("left_min_k", C.c_void_p), ("right_min", C.c_void_p), ("right_min_k", C.c_void_p),
                ("near_samples", C.c_void_p), ("near_first", C.c_void_p), ("near_last", C.c_void_p), ("cross_n", C.c_void_p),
                ("near_count", C.c_void_p), ("cross_count", C.c_void_p),
                ("events", C.c_void_p), ("event_capacity", C.c_int64), ("n_events", C.c_int64), ("first_sample", C.c_int64)]


class BodyEvent(C.Structure):
    """csf_body_event of include/csf.h: a (sample, i < j) whose outlines are under a threshold"""

    _fields_ = [("sample", C.c_int64), ("i", C.c_int32), ("j", C.c_int32), ("gap", C.c_double), ("ttc", C.c_double)]


class BodyOut(C.Structure):
    """csf_body_out of include/csf.h: where the body encounters of one engine go (any pointer may be NULL)"""

    _fields_ = [("gap_min", C.c_void_p), ("gap_with", C.c_void_p), ("ttc_min", C.c_void_p), ("ttc_with", C.c_void_p),
                ("run_gap_min", C.c_void_p), ("run_gap_with", C.c_void_p), ("run_gap_sample", C.c_void_p),
                ("run_ttc_min", C.c_void_p), ("run_ttc_with", C.c_void_p), ("run_ttc_sample", C.c_void_p), ("overlap_n", C.c_void_p),
                ("events", C.c_void_p), ("event_capacity", C.c_int64), ("n_events", C.c_int64), ("first_sample", C.c_int64)]


class EngineError(RuntimeError):
    pass


_lib = None

# csf_pair_shape_of (include/csf.h): the input words and the words of the answer, in order
PAIR_SHAPE_IN, PAIR_SHAPE_OUT = 16, 15
PAIR_SHAPE_INPUTS = ("p2r", "n_classes", "has_bike", "model_mask", "model", "classify", "recs_valid", "pair_variant", "recv_binned", "rpb", "wide",
                     "reach", "tables", "segments", "nloc")
PAIR_SHAPE_FIELDS = ("family", "field", "rw", "p2r", "classify", "binr", "ord", "reach", "rpb", "cw", "per_group", "threads", "tile", "grid_x", "order_groups")


def pair_shape_of(lib, words):
    """the answer of csf_pair_shape_of for PAIR_SHAPE_IN int32 input words (a ctypes array), as a dict with the kernel's name"""
    out = (C.c_int32 * PAIR_SHAPE_OUT)()
    name = C.c_char_p()
    if lib.csf_pair_shape_of(words, out, C.byref(name)) != PAIR_SHAPE_OUT:
        raise EngineError("csf_pair_shape_of refused its arguments")
    return dict(zip(PAIR_SHAPE_FIELDS, out), name=name.value.decode())


def load():
    """Load libcsf_hip.so; raises EngineError if the HIP extension is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C cyclistsocialforce_amd/csrc`). This package has no CPU fallback."
        )
    try:
        L = C.CDLL(LIB_PATH)
    except OSError as exc:  # pragma: no cover - depends on the machine
        raise EngineError(f"cannot load {LIB_PATH}: {exc}") from exc
    vp, i32, i64, dp = C.c_void_p, C.c_int32, C.c_int64, C.c_void_p
    L.csf_create.restype = vp
    L.csf_create.argtypes = [C.POINTER(Params), i64, i32]
    L.csf_create_v.restype = vp
    L.csf_create_v.argtypes = [C.POINTER(Params), C.c_size_t, i32, i64, i32]
    L.csf_params_size.restype = C.c_size_t
    L.csf_params_size.argtypes = []
    L.csf_destroy.argtypes = [vp]
    L.csf_last_error.restype = C.c_char_p
    L.csf_last_error.argtypes = [vp]
    L.csf_abi_version.restype = i32
    L.csf_add_agents.argtypes = [vp, i64, dp, dp]
    L.csf_remove_agents.argtypes = [vp, i64, vp]
    L.csf_replace_agents.argtypes = [vp, i64, vp, i64, dp, dp, vp, dp]
    L.csf_set_dest_queue.argtypes = [vp, i64, vp, vp, dp, i32]
    L.csf_set_road_vertices.argtypes = [vp, i32, vp, dp, dp, dp]
    L.csf_set_params.argtypes = [vp, C.POINTER(Params)]
    L.csf_set_param_classes.argtypes = [vp, i32, C.POINTER(Params)]
    L.csf_set_agent_class.argtypes = [vp, i64, vp, vp]
    L.csf_set_v_desired.argtypes = [vp, i64, vp, dp]
    L.csf_set_priority_rule.argtypes = [vp, i32]
    L.csf_push_state.argtypes = [vp, i64, vp, dp]
    L.csf_num_agents.restype = i64
    L.csf_num_agents.argtypes = [vp]
    L.csf_num_states.restype = i32
    L.csf_num_states.argtypes = [vp]
    L.csf_step.argtypes = [vp, i64]
    L.csf_sync.argtypes = [vp]
    L.csf_calc_forces.argtypes = [vp]
    L.csf_apply_forces.argtypes = [vp, dp, dp]
    L.csf_replay_forces.argtypes = [vp, i64, dp, dp, vp, i32, i32, dp]
    L.csf_dest_force.argtypes = [vp, dp, dp]
    L.csf_get_state.argtypes = [vp, dp, vp, vp, C.POINTER(i64)]
    L.csf_get_forces.argtypes = [vp, dp, dp]
    L.csf_get_force_parts.argtypes = [vp, dp, dp, dp, dp]
    L.csf_status.argtypes = [vp, vp]
    L.csf_enable_history.argtypes = [vp, i32, i32]
    L.csf_get_history.argtypes = [vp, i64, i64, dp]
    L.csf_pair_force.argtypes = [vp, dp, i64, dp, dp, dp, i32, dp, dp]
    L.csf_comm_unique_id.argtypes = [vp]
    L.csf_comm_init.argtypes = [vp, vp, i32, i32]
    L.csf_shard_range.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.csf_profile_enable.argtypes = [vp, i32]
    L.csf_profile_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i64)]
    L.csf_far_radius.argtypes = [vp, C.POINTER(C.c_double)]
    L.csf_profile_gather.argtypes = [vp, C.POINTER(C.c_double)]
    L.csf_get_tick.argtypes = [vp, dp, vp, vp, dp, dp, C.POINTER(i64)]
    pd = C.POINTER(C.c_double)
    L.csf_profile_kernels.argtypes = [vp, pd, C.POINTER(i64)]
    L.csf_profile_samples.argtypes = [vp, dp, i64, C.POINTER(i64)]
    L.csf_profile_samples_of.argtypes = [vp, i32, dp, i64, C.POINTER(i64)]
    L.csf_count_pairs.argtypes = [vp, C.POINTER(i64), C.POINTER(C.c_char_p)]   # int64 counts[4]
    L.csf_comm_init_loopback.argtypes = [C.POINTER(vp), i32]
    L.csf_step_group.argtypes = [C.POINTER(vp), i32, i64]
    L.csf_untracked.argtypes = [vp, vp]
    L.csf_update_destination.argtypes = [vp, i64, vp]
    L.csf_update_nav_state.argtypes = [vp, i64, vp, vp, dp, dp]
    L.csf_set_dest_pointer.argtypes = [vp, i64, vp, vp]
    L.csf_set_incremental.argtypes = [vp, i32]
    L.csf_set_script.argtypes = [vp, i64, vp, vp, dp]
    L.csf_near_dropped.argtypes = [vp, C.POINTER(i64)]
    if hasattr(L, "csf_handout_ranks"):
        L.csf_handout_ranks.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    if hasattr(L, "csf_wg_order_ranks"):
        L.csf_wg_order_ranks.argtypes = [C.POINTER(C.c_uint32), C.c_int32, C.POINTER(C.c_int32)]
        L.csf_wg_order_tables.argtypes = [vp, C.POINTER(i64), C.POINTER(i32), C.POINTER(i32), vp, vp, i64]
    if hasattr(L, "csf_pair_shape_of"):
        L.csf_pair_shape_of.argtypes = [C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_char_p)]
        L.csf_pair_shape_words.argtypes = [vp, C.POINTER(i32)]
    L.csf_comm_stream_order.argtypes = [vp, C.POINTER(i32), dp]
    L.csf_small_ticks.argtypes = [vp, C.POINTER(i64)]
    L.csf_field_map.argtypes = [vp, i64, dp, dp, dp, C.c_uint32, i32, dp, dp]
    L.csf_field_map_launches.argtypes = [vp, C.POINTER(i64)]
    if hasattr(L, "csf_encounters"):             # (CSF_LIB may name an older build for an A/B measurement: it lacks these three)
        f64 = C.c_double
        L.csf_encounters.argtypes = [vp, i64, i64, f64, f64, f64, C.POINTER(EncounterOut)]
        L.csf_batch_encounters.argtypes = [C.POINTER(vp), i32, i64, f64, f64, f64, C.POINTER(EncounterOut)]
        L.csf_encounter_launches.argtypes = [vp, C.POINTER(i64)]
    if hasattr(L, "csf_post_encroachment"):      # (likewise)
        L.csf_post_encroachment.argtypes = [vp, i64, i64, C.c_double, C.POINTER(PetOut)]
        L.csf_batch_post_encroachment.argtypes = [C.POINTER(vp), i32, i64, C.c_double, C.POINTER(PetOut)]
        L.csf_pet_launches.argtypes = [vp, C.POINTER(i64)]
    if hasattr(L, "csf_passing"):                # (likewise)
        L.csf_passing.argtypes = [vp, i64, i64, C.c_double, C.c_double, C.c_double, C.POINTER(PassingOut)]
        L.csf_batch_passing.argtypes = [C.POINTER(vp), i32, i64, C.c_double, C.c_double, C.c_double, C.POINTER(PassingOut)]
        L.csf_passing_launches.argtypes = [vp, C.POINTER(i64)]
    if hasattr(L, "csf_flow"):                   # (likewise)
        L.csf_flow.argtypes = [vp, i64, i64, C.POINTER(FlowLayout), C.POINTER(FlowOut)]
        L.csf_batch_flow.argtypes = [C.POINTER(vp), i32, i64, C.POINTER(FlowLayout), C.POINTER(FlowOut)]
        L.csf_flow_launches.argtypes = [vp, C.POINTER(i64)]
    if hasattr(L, "csf_clearance"):              # (likewise)
        L.csf_clearance.argtypes = [vp, i64, i64, C.POINTER(ClearanceRoad), C.c_double, C.POINTER(ClearanceOut)]
        L.csf_batch_clearance.argtypes = [C.POINTER(vp), i32, i64, C.POINTER(ClearanceRoad), C.c_double, C.POINTER(ClearanceOut)]
        L.csf_clearance_launches.argtypes = [vp, C.POINTER(i64)]
    if hasattr(L, "csf_body_encounters"):        # (likewise)
        f64 = C.c_double
        L.csf_body_encounters.argtypes = [vp, i64, i64, vp, f64, f64, C.POINTER(BodyOut)]
        L.csf_batch_body_encounters.argtypes = [C.POINTER(vp), i32, i64, C.POINTER(vp), f64, f64, C.POINTER(BodyOut)]
        L.csf_body_encounter_launches.argtypes = [vp, C.POINTER(i64)]
    L.csf_step_get_tick.argtypes = [vp, i64, vp, vp, vp, vp, vp, C.POINTER(i64)]
    L.csf_mid_ticks.argtypes = [vp, C.POINTER(i64)]
    L.csf_holes_taken.argtypes = [vp, C.POINTER(i64)]
    L.csf_chase_ticks.argtypes = [vp, C.POINTER(i64)]
    L.csf_chase_calibration.argtypes = [vp, C.POINTER(i32), dp]
    L.csf_get_integrator_state.argtypes = [vp, dp, dp, vp]
    L.csf_set_integrator_state.argtypes = [vp, i64, vp, dp, dp, vp]
    L.csf_batch_join.argtypes = [C.POINTER(vp), i32]
    L.csf_batch_leave.argtypes = [C.POINTER(vp), i32]
    L.csf_step_batch.argtypes = [C.POINTER(vp), i32, i64]
    L.csf_step_batch_get_tick.argtypes = [C.POINTER(vp), i32, i64, C.POINTER(TickOut)]
    L.csf_batch_ticks.argtypes = [vp, C.POINTER(i64)]
    if hasattr(L, "csf_batch_mid_ticks"):        # (the same: an older build lacks these two)
        L.csf_batch_mid_ticks.argtypes = [vp, C.POINTER(i64)]
        L.csf_batch_launches.argtypes = [vp, C.POINTER(i64)]
    if hasattr(L, "csf_record"):                 # (CSF_LIB may name an older build for an A/B measurement: it lacks these three)
        L.csf_record.argtypes = [vp, i32, i32, C.c_uint32]
        L.csf_get_record.argtypes = [vp, i64, i64, dp, dp]
        L.csf_batch_get_record.argtypes = [C.POINTER(vp), i32, i64, C.POINTER(RecordOut)]
    if hasattr(L, "csf_calib_load"):             # (the same)
        L.csf_calib_load.argtypes = [vp, i32, i64, dp, dp, dp, vp, dp, i32, vp, i32]
        L.csf_calib_eval.argtypes = [vp, i32, C.POINTER(Params), C.c_size_t, i32, i32, dp, i32, dp]
        L.csf_calib_launches.argtypes = [vp, C.POINTER(i64)]
        L.csf_calib_clear.argtypes = [vp]
    if hasattr(L, "csf_scene_calib_load"):       # (the same)
        L.csf_scene_calib_load.argtypes = [vp, i32, vp, i64, dp, dp, vp, dp, vp, dp, i32, vp, i32]
        L.csf_scene_calib_eval.argtypes = [vp, i32, C.POINTER(Params), C.c_size_t, i32, dp, i32, dp]
        L.csf_scene_calib_launches.argtypes = [vp, C.POINTER(i64)]
        L.csf_scene_calib_clear.argtypes = [vp]
    if hasattr(L, "csf_scene_calib_replay"):     # (the same)
        L.csf_scene_calib_replay.argtypes = [vp, vp, dp]
    if hasattr(L, "csf_scene_calib_road"):       # (the same)
        L.csf_scene_calib_road.argtypes = [vp, i32, vp, vp, dp, dp, dp]
        L.csf_scene_calib_eval_road.argtypes = [vp, i32, C.POINTER(Params), C.c_size_t, i32, dp, dp, dp, i32, dp]
    if hasattr(L, "csf_scene_calib_windows"):    # (the same)
        L.csf_scene_calib_windows.argtypes = [vp, vp, vp]
    if hasattr(L, "csf_scene_calib_load_shared"):   # (the same)
        L.csf_scene_calib_load_shared.argtypes = [vp, i32, vp, vp, vp, vp, vp, i64, dp, dp, vp, dp, vp, dp, i32, vp, i32]
    if hasattr(L, "csf_scene_calib_load_wide"):     # (the same)
        L.csf_scene_calib_load_wide.argtypes = [vp, i32, vp, vp, vp, vp, vp, i64, dp, dp, vp, dp, vp, dp, i32, vp, i32, i32]
    if hasattr(L, "csf_scene_calib_groups"):        # (the same)
        L.csf_scene_calib_groups.argtypes = [vp, vp, i32]
        L.csf_scene_calib_eval_groups.argtypes = [vp, i32, i32, C.POINTER(Params), C.c_size_t, i32, dp, dp, dp, i32, dp]
    if hasattr(L, "csf_scene_calib_lane_groups"):   # (the same)
        L.csf_scene_calib_lane_groups.argtypes = [vp, vp, i32]
    if hasattr(L, "csf_scene_calib_classes"):       # (the same)
        L.csf_scene_calib_classes.argtypes = [vp, vp, i32, vp, dp]
    if hasattr(L, "csf_scene_calib_lane_classes"):  # (the same)
        L.csf_scene_calib_lane_classes.argtypes = [vp, vp, i32, vp, dp]
    if hasattr(L, "csf_small_classes"):             # (the same)
        L.csf_small_classes.argtypes = [vp, i32]
    if hasattr(L, "csf_mid_road"):                  # (the same)
        L.csf_mid_road.argtypes = [vp, i32]
        L.csf_mid_road_ticks.argtypes = [vp, C.POINTER(i64)]
    if hasattr(L, "csf_mid_classes"):               # (the same)
        L.csf_mid_classes.argtypes = [vp, i32]
        L.csf_mid_classes_ticks.argtypes = [vp, C.POINTER(i64)]
    if L.csf_abi_version() != ABI_VERSION:
        raise EngineError(f"libcsf_hip.so has ABI {L.csf_abi_version()}, expected {ABI_VERSION}")
    if L.csf_params_size() != C.sizeof(Params):
        raise EngineError(f"csf_params: the library's has {L.csf_params_size()} bytes, this binding's {C.sizeof(Params)} "
                          "(include/csf.h and _ffi.Params are out of step)")
    _lib = L
    return L
