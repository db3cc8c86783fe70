"""ctypes binding of libcsm_hip.so (the C ABI declared in include/csm_hip.h).

The library is built in-tree (my-lidar-graph-slam-v2_amd/csrc/libcsm_hip.so) by
__graft_entry__.build(). There is no fallback: if the shared object is missing
the import fails, and without a GPU every compute entry point returns
CSM_ENODEV.
"""
import ctypes as C
import importlib.util
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
# CSM_HIP_LIB: a tuning build of the same library (tools/build_variant.sh), for A/B runs on one box
LIB_PATH = os.environ.get("CSM_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "csrc", "libcsm_hip.so")

CSM_OK = 0
CSM_ENOENT = -2
CSM_EIO = -5
CSM_ENOMEM = -12
CSM_ENODEV = -19
CSM_EINVAL = -22

FLAG_EDGE_BAND = 1
FLAG_KEY_TIE = 2
FLAG_F64_TIE = 4
FLAG_LITERAL = 8
FLAG_PROJ_DELTA = 16


class Config(C.Structure):
    _fields_ = [("device_id", C.c_int32), ("tuning_off", C.c_uint32), ("map_uncertain_cap", C.c_int32),
                ("reserved", C.c_int32 * 5)]


# csm_config.tuning_off bits (include/csm_hip.h)
TUNE_NO_LANE_MAP, TUNE_NO_XCD_MAP, TUNE_NO_PAIR_TAIL, TUNE_NO_TWO_SLICES = 1, 2, 4, 8
TUNE_NO_THETA_MAJOR, TUNE_NO_TILE_SPLIT, TUNE_MAP_HOST_PROJECTION, TUNE_NO_JOINT = 16, 32, 64, 128
TUNE_NO_BOUND_PASS = 256
TUNE_NO_TWO_PHASE, TUNE_FORCE_TWO_PHASE, TUNE_NO_GRAPHS = 512, 1024, 2048
TUNE_GREEDY_LITERAL_SUMS = 4096
GREEDY_KERNEL_SIZE_MAX = 8
GROUP_FORCE_RCCL = 1


class SearchInfo(C.Structure):
    _fields_ = [("nominal_candidates", C.c_int64), ("coarse_nodes_scored", C.c_int64),
                ("fine_candidates_scored", C.c_int64), ("two_phase", C.c_int32), ("graph_replayed", C.c_int32),
                ("blocks_scored", C.c_int64), ("blocks_skipped", C.c_int64)]


class Geometry(C.Structure):
    _fields_ = [("resolution", C.c_double), ("offset_x", C.c_double),
                ("offset_y", C.c_double)]


class Scan(C.Structure):
    _fields_ = [("angles", C.POINTER(C.c_double)),
                ("ranges", C.POINTER(C.c_double)),
                ("n_points", C.c_int32), ("reserved", C.c_int32),
                ("relative_sensor_pose", C.c_double * 3)]


class CorrelativeParams(C.Structure):
    _fields_ = [("range_x", C.c_double), ("range_y", C.c_double),
                ("range_theta", C.c_double), ("low_resolution", C.c_int32),
                ("reserved", C.c_int32), ("score_threshold", C.c_double),
                ("known_rate_threshold", C.c_double)]


class BnbParams(C.Structure):
    _fields_ = [("range_x", C.c_double), ("range_y", C.c_double),
                ("range_theta", C.c_double), ("node_height_max", C.c_int32),
                ("reserved", C.c_int32), ("score_threshold", C.c_double),
                ("known_rate_threshold", C.c_double)]


class ScanNode(C.Structure):
    _fields_ = [("global_pose", C.c_double * 3), ("scan", Scan), ("min_range", C.c_double),
                ("max_range", C.c_double)]


class MapBuilderParams(C.Structure):
    _fields_ = [("usable_range_min", C.c_double), ("usable_range_max", C.c_double),
                ("prob_hit", C.c_double), ("prob_miss", C.c_double), ("subpixel_scale", C.c_int32)]


class MapShape(C.Structure):
    _fields_ = [("resolution", C.c_double), ("offset_x", C.c_double), ("offset_y", C.c_double),
                ("rows", C.c_int32), ("cols", C.c_int32), ("log2_block_size", C.c_int32)]


class MapBuildInfo(C.Structure):
    _fields_ = [("rays", C.c_int64), ("cell_updates", C.c_int64), ("saturated_reads", C.c_int64),
                ("first_known_row", C.c_int32), ("first_known_col", C.c_int32),
                ("device_projection", C.c_int32), ("reserved", C.c_int32),
                ("host_us", C.c_double), ("device_us", C.c_double)]


class MapBuildJob(C.Structure):
    _fields_ = [("map_id", C.c_uint64), ("shape", MapShape), ("global_map_pose", C.c_double * 3),
                ("nodes", C.POINTER(ScanNode)), ("n_nodes", C.c_int32), ("status", C.c_int32),
                ("info", MapBuildInfo)]


class MapBatchParams(C.Structure):
    _fields_ = [("scratch_limit_bytes", C.c_int64)]


class MapBatchInfo(C.Structure):
    _fields_ = [("chunks", C.c_int32), ("host_projection_jobs", C.c_int32), ("scan_bytes_uploaded", C.c_int64),
                ("host_us", C.c_double), ("device_us", C.c_double)]


class GlobalMapParams(C.Structure):
    _fields_ = [("scratch_limit_bytes", C.c_int64), ("rank_direct_max", C.c_int32), ("rank_tile", C.c_int32)]


class GlobalMapInfo(C.Structure):
    _fields_ = [("parts", C.c_int32), ("max_hits_per_cell", C.c_int32), ("direct_cells", C.c_int64),
                ("sorted_cells", C.c_int64), ("tiled_cells", C.c_int64), ("beams", C.c_int64),
                ("host_us", C.c_double), ("device_us", C.c_double)]


class GridSearchParams(C.Structure):
    _fields_ = [("range_x", C.c_double), ("range_y", C.c_double), ("range_theta", C.c_double),
                ("step_x", C.c_double), ("step_y", C.c_double), ("step_theta", C.c_double),
                ("score_threshold", C.c_double), ("known_rate_threshold", C.c_double)]


class Result(C.Structure):
    _fields_ = [("found", C.c_int32), ("best_x", C.c_int32),
                ("best_y", C.c_int32), ("best_theta", C.c_int32),
                ("key", C.c_uint64), ("sum_values", C.c_uint32),
                ("known", C.c_uint32), ("tie_count", C.c_uint32),
                ("flags", C.c_uint32), ("score", C.c_double)]


class Summary(C.Structure):
    _fields_ = [("pose_found", C.c_int32), ("win_x", C.c_int32),
                ("win_y", C.c_int32), ("win_theta", C.c_int32),
                ("step_x", C.c_double), ("step_y", C.c_double),
                ("step_theta", C.c_double), ("sensor_pose", C.c_double * 3),
                ("best_sensor_pose", C.c_double * 3),
                ("estimated_pose", C.c_double * 3),
                ("input_setup_us", C.c_double), ("optimization_us", C.c_double),
                ("candidates", C.c_int64), ("raw", Result)]


class RefineParams(C.Structure):
    _fields_ = [("covariance_scale", C.c_double), ("iterations_max", C.c_int32), ("reserved", C.c_int32),
                ("convergence_threshold", C.c_double), ("lambda_", C.c_double)]


class RefineResult(C.Structure):
    _fields_ = [("normalized_initial_cost", C.c_double), ("normalized_cost", C.c_double),
                ("sensor_pose", C.c_double * 3), ("best_sensor_pose", C.c_double * 3),
                ("estimated_pose", C.c_double * 3), ("covariance", C.c_double * 9),
                ("hessian", C.c_double * 9), ("lambda_", C.c_double), ("iterations", C.c_int32),
                ("reserved", C.c_int32)]


class GreedyParams(C.Structure):
    _fields_ = [("map_resolution", C.c_double), ("hit_and_missed_dist", C.c_double),
                ("occupancy_threshold", C.c_double), ("kernel_size", C.c_int32), ("reserved", C.c_int32),
                ("standard_deviation", C.c_double), ("scaling_factor", C.c_double)]


class HillClimbingParams(C.Structure):
    _fields_ = [("linear_step", C.c_double), ("angular_step", C.c_double),
                ("max_iterations", C.c_int32), ("max_refinements", C.c_int32), ("cost", GreedyParams)]


class HillClimbingResult(C.Structure):
    _fields_ = [("normalized_initial_cost", C.c_double), ("normalized_cost", C.c_double),
                ("sensor_pose", C.c_double * 3), ("best_sensor_pose", C.c_double * 3),
                ("estimated_pose", C.c_double * 3), ("covariance", C.c_double * 9),
                ("diff_translation", C.c_double), ("diff_rotation", C.c_double),
                ("iterations", C.c_int32), ("refinements", C.c_int32), ("replays", C.c_int32),
                ("host_path", C.c_int32), ("cost_evaluations", C.c_int64)]


# pose-graph optimization (include/csm_hip.h)
PG_SOLVER_SPARSE_CHOLESKY, PG_SOLVER_CONJUGATE_GRADIENT, PG_SOLVER_SCHUR_CHOLESKY = 0, 1, 2
PG_SCHUR_MAX_LOCAL = 4096
PG_LOSS_SQUARED, PG_LOSS_HUBER, PG_LOSS_CAUCHY, PG_LOSS_FAIR, PG_LOSS_GEMAN_MCCLURE, PG_LOSS_WELSCH = range(6)


class PoseGraphEdge(C.Structure):
    _fields_ = [("local_map_index", C.c_int32), ("scan_index", C.c_int32), ("is_loop", C.c_int32),
                ("reserved", C.c_int32), ("relative_pose", C.c_double * 3), ("information", C.c_double * 9)]


class PoseGraphLMParams(C.Structure):
    _fields_ = [("iterations_max", C.c_int32), ("solver_type", C.c_int32), ("loss_type", C.c_int32),
                ("reserved", C.c_int32), ("error_tolerance", C.c_double), ("loss_scale", C.c_double)]


class PoseGraphLMInfo(C.Structure):
    _fields_ = [("steps", C.c_int32), ("reserved", C.c_int32), ("cg_iterations", C.c_int64),
                ("initial_error", C.c_double), ("final_error", C.c_double), ("final_lambda", C.c_double)]


class PoseGraphLMStep(C.Structure):
    _fields_ = [("total_error", C.c_double), ("lambda_", C.c_double), ("rhs_norm2", C.c_double),
                ("residual_norm2", C.c_double),
                ("cg_iterations", C.c_int32), ("reserved", C.c_int32)]


class PoseGraphPair(C.Structure):
    _fields_ = [("local_map_index", C.c_int32), ("scan_index", C.c_int32)]


class PoseGraphMarginal(C.Structure):
    _fields_ = [("local_cov", C.c_double * 9), ("scan_cov", C.c_double * 9), ("cross_cov", C.c_double * 9),
                ("relative_cov", C.c_double * 9), ("finite", C.c_int32), ("reserved", C.c_int32)]


class PoseGraphMarginalsInfo(C.Structure):
    _fields_ = [("n_columns", C.c_int32), ("reserved", C.c_int32)]


class LoopQuery(C.Structure):
    _fields_ = [("map_id", C.c_uint64), ("geometry", Geometry), ("scan", Scan),
                ("initial_pose", C.c_double * 3)]


class Window(C.Structure):
    _fields_ = [("n_theta", C.c_int32), ("n_points", C.c_int32),
                ("win_x", C.c_int32), ("win_y", C.c_int32),
                ("low_resolution", C.c_int32), ("coarse_level", C.c_int32),
                ("min_known", C.c_int32), ("merge_mode", C.c_int32),
                ("score_threshold", C.c_double)]


PEAKS_MAX = 16


class PeaksParams(C.Structure):
    _fields_ = [("k_max", C.c_int32), ("excl_x", C.c_int32), ("excl_y", C.c_int32), ("excl_theta", C.c_int32),
                ("scratch_limit_bytes", C.c_int64)]


VOLUME_BINS = 1024


class VolumeParams(C.Structure):
    _fields_ = [("temperature", C.c_double), ("scratch_limit_bytes", C.c_int64)]


class VolumeMoments(C.Structure):
    _fields_ = [("best", Result), ("m0", C.c_int64), ("m1", C.c_int64 * 3), ("m2", C.c_int64 * 6),
                ("support", C.c_int64), ("border_support", C.c_int64), ("bin_shift", C.c_int32),
                ("reserved", C.c_int32)]


class VolumeSummary(C.Structure):
    _fields_ = [("summary", Summary), ("moments", VolumeMoments), ("mean_offset", C.c_double * 3),
                ("sensor_covariance", C.c_double * 9), ("covariance", C.c_double * 9)]


class MotionPrior(C.Structure):
    _fields_ = [("information", C.c_double * 9), ("steps", C.c_double * 3), ("scratch_limit_bytes", C.c_int64)]


class PriorResult(C.Structure):
    _fields_ = [("best", Result), ("unweighted", Result), ("penalty", C.c_int64), ("penalised_key", C.c_int64),
                ("Q", C.c_int64 * 6)]


class PriorSummary(C.Structure):
    _fields_ = [("summary", Summary), ("prior", PriorResult)]


LIKELIHOOD_MAX_RADIUS = 16


class LikelihoodParams(C.Structure):
    _fields_ = [("radius", C.c_int32), ("occupied_min", C.c_uint32), ("keep_unknown", C.c_int32),
                ("reserved", C.c_int32), ("kernel", C.c_void_p)]


DISTANCE_MAX_RADIUS, DISTANCE_NONE = 255, 0xFFFFFFFF


class DistanceParams(C.Structure):
    _fields_ = [("radius", C.c_int32), ("occupied_min", C.c_uint32), ("keep_unknown", C.c_int32),
                ("reserved", C.c_int32), ("table", C.c_void_p)]


RAY_CHECK_MAX_SCALE = 512


class RayCheckParams(C.Structure):
    _fields_ = [("usable_range_min", C.c_double), ("usable_range_max", C.c_double),
                ("subpixel_scale", C.c_int32), ("end_tolerance", C.c_int32),
                ("occupied_min", C.c_uint32), ("free_max", C.c_uint32), ("scratch_limit_bytes", C.c_int64)]


class RayCheckResult(C.Structure):
    _fields_ = [("beams", C.c_int32), ("usable", C.c_int32), ("walked", C.c_int32), ("blocked", C.c_int32),
                ("end_inside", C.c_int32), ("end_occupied", C.c_int32), ("end_free", C.c_int32),
                ("end_unknown", C.c_int32),
                ("cells", C.c_int64), ("cells_free", C.c_int64), ("cells_unknown", C.c_int64),
                ("cells_near", C.c_int64), ("cells_blocking", C.c_int64),
                ("max_depth", C.c_int32), ("host_beams", C.c_int32)]


LOOP_SEARCH_MAX_K, LOOP_SEARCH_MAX_NODES, LOOP_SEARCH_MAX_MAPS = 16, 1 << 20, 1 << 16


class LoopSearchParams(C.Structure):
    _fields_ = [("travel_dist_threshold", C.c_double), ("node_dist_threshold", C.c_double),
                ("n_per_query", C.c_int32), ("one_per_map", C.c_int32)]


class LoopCandidate(C.Structure):
    _fields_ = [("query_scan_index", C.c_int32), ("ref_scan_index", C.c_int32), ("ref_map_index", C.c_int32),
                ("reserved", C.c_int32), ("dist_sq", C.c_double)]


class LoopSearchInfo(C.Structure):
    _fields_ = [("pairs_evaluated", C.c_int64), ("pairs_eligible", C.c_int64)]


LOOP_CONSISTENCY_MAX_EDGES, LOOP_CONSISTENCY_MAX_CHI2_EDGES = 8192, 2048


class LoopConsistencyInfo(C.Structure):
    _fields_ = [("consistent_pairs", C.c_int64), ("bad_pivots", C.c_int64), ("clique_size", C.c_int32),
                ("winning_seed", C.c_int32), ("seeds_run", C.c_int32), ("reserved", C.c_int32)]


DESCRIPTOR_MAX_RINGS, DESCRIPTOR_MAX_SECTORS, DESCRIPTOR_MAX_BEAMS = 32, 128, 65536
APPEARANCE_REF_CHUNK, APPEARANCE_TABLE_BYTES = 128, 64 << 20


class DescriptorParams(C.Structure):
    _fields_ = [("n_rings", C.c_int32), ("n_sectors", C.c_int32), ("range_min", C.c_double),
                ("range_max", C.c_double)]


class AppearanceParams(C.Structure):
    _fields_ = [("descriptor", DescriptorParams), ("travel_dist_threshold", C.c_double),
                ("max_distance", C.c_uint32), ("min_cell_sum", C.c_uint32), ("n_per_query", C.c_int32),
                ("one_per_map", C.c_int32)]


class AppearanceCandidate(C.Structure):
    _fields_ = [("query_scan_index", C.c_int32), ("ref_scan_index", C.c_int32), ("ref_map_index", C.c_int32),
                ("shift", C.c_int32), ("distance", C.c_uint32), ("ring_distance", C.c_uint32)]


POSE_UNCERTAIN, POSE_HOST_PROJECTED = 1, 2
POSE_SET_MAX_POSES = 1 << 18


class PoseSet(C.Structure):
    _fields_ = [("map_id", C.c_uint64), ("geometry", Geometry), ("scan", Scan), ("poses", C.POINTER(C.c_double)),
                ("n_poses", C.c_int32), ("reserved", C.c_int32)]


class PoseRecord(C.Structure):
    _fields_ = [("sum_values", C.c_uint32), ("known", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class PoseSetsInfo(C.Structure):
    _fields_ = [("poses", C.c_int64), ("uncertain_poses", C.c_int32), ("changed_poses", C.c_int32),
                ("host_us", C.c_double), ("device_us", C.c_double)]


class PoseUpdateParams(C.Structure):
    _fields_ = [("temperature", C.c_double), ("known_rate_threshold", C.c_double), ("n_out", C.c_int32),
                ("reserved", C.c_int32), ("offset", C.c_uint64)]


class PoseUpdateInfo(C.Structure):
    _fields_ = [("m0", C.c_uint64), ("key_max", C.c_uint64), ("best_index", C.c_int32), ("support", C.c_int32),
                ("bin_shift", C.c_int32), ("found", C.c_int32)]


CAST_NONE, CAST_OCCUPIED, CAST_UNKNOWN = 0, 1, 2


class RayCastParams(C.Structure):
    _fields_ = [("range_max", C.c_double), ("range_min", C.c_double), ("subpixel_scale", C.c_int32),
                ("occupied_min", C.c_uint32), ("unknown_stops", C.c_int32), ("reserved", C.c_int32),
                ("scratch_limit_bytes", C.c_int64)]


class RayCastRecord(C.Structure):
    _fields_ = [("cell_x", C.c_int32), ("cell_y", C.c_int32), ("value", C.c_uint32), ("kind", C.c_int32),
                ("dist2", C.c_int64)]


class RayCastInfo(C.Structure):
    _fields_ = [("rays", C.c_int64), ("host_rays", C.c_int64), ("cells_read", C.c_int64),
                ("cells_to_stop", C.c_int64), ("host_us", C.c_double), ("device_us", C.c_double)]


# name -> (restype, argtypes); mirrors include/csm_hip.h one to one
_P = C.POINTER
_ctx = C.c_void_p
SIGNATURES = {
    "csm_create": (C.c_int, [_P(Config), _P(_ctx)]),
    "csm_destroy": (C.c_int, [_ctx]),
    "csm_last_error": (C.c_char_p, [_ctx]),
    "csm_set_stream": (C.c_int, [_ctx, C.c_void_p]),
    "csm_synchronize": (C.c_int, [_ctx]),
    "csm_upload_grid": (C.c_int, [_ctx, C.c_uint64, C.c_void_p, C.c_int32, C.c_int32]),
    "csm_upload_grid_blocks": (C.c_int, [_ctx, C.c_uint64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "csm_has_grid": (C.c_int, [_ctx, C.c_uint64]),
    "csm_release_grid": (C.c_int, [_ctx, C.c_uint64]),
    "csm_build_pyramid": (C.c_int, [_ctx, C.c_uint64, _P(C.c_int32), C.c_int32]),
    "csm_download_level": (C.c_int, [_ctx, C.c_uint64, C.c_int32, C.c_void_p]),
    "csm_build_pyramids": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    "csm_copy_last_batch_records": (C.c_int, [_ctx, C.c_void_p]),
    "csm_host_search_step": (C.c_int, [C.c_double, C.c_void_p, C.c_int32,
                                       _P(C.c_double), _P(C.c_double), _P(C.c_double)]),
    "csm_host_window": (C.c_int, [C.c_double, C.c_double]),
    "csm_host_min_known": (C.c_int, [C.c_int32, C.c_double]),
    "csm_host_compound": (None, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "csm_host_inverse_compound": (None, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "csm_host_move_backward": (None, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "csm_host_project": (C.c_int, [_P(Geometry), C.c_void_p, C.c_double, C.c_int32,
                                   C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "csm_host_probability_lut": (None, [C.c_void_p]),
    "csm_project_scan": (C.c_int, [_ctx, _P(Geometry), C.c_void_p, C.c_double, C.c_int32, C.c_void_p,
                                   C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                   _P(C.c_int32)]),
    "csm_score_window": (C.c_int, [_ctx, C.c_uint64, _P(Window), C.c_void_p,
                                   C.c_void_p, _P(Result)]),
    "csm_score_window_dev": (C.c_int, [_ctx, C.c_uint64, _P(Window), C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "csm_score_windows_dev": (C.c_int, [_ctx, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "csm_score_windows_dump_dev": (C.c_int, [_ctx, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "csm_bound_pass_stats": (C.c_int, [_ctx, _P(C.c_uint64), _P(C.c_uint64)]),
    "csm_last_search_info": (C.c_int, [_ctx, C.c_void_p]),
    "csm_resolve_window_dev": (C.c_int, [_ctx, C.c_uint64, _P(Window), C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "csm_score_window_dump": (C.c_int, [_ctx, C.c_uint64, _P(Window), C.c_void_p,
                                        C.c_void_p, _P(Result), C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "csm_correlative_match": (C.c_int, [_ctx, C.c_uint64, _P(Geometry), _P(Scan),
                                        C.c_void_p, _P(CorrelativeParams), _P(Summary)]),
    "csm_score_window_peaks": (C.c_int, [_ctx, C.c_uint64, _P(Window), C.c_void_p, C.c_void_p, _P(PeaksParams),
                                         _P(Result), _P(C.c_int32)]),
    "csm_correlative_peaks": (C.c_int, [_ctx, C.c_uint64, _P(Geometry), _P(Scan), C.c_void_p,
                                        _P(CorrelativeParams), _P(PeaksParams), _P(Summary), _P(C.c_int32)]),
    "csm_correlative_peaks_batch": (C.c_int, [_ctx, _P(LoopQuery), C.c_int32, _P(CorrelativeParams),
                                              _P(PeaksParams), _P(Summary), _P(C.c_int32)]),
    "csm_score_window_moments": (C.c_int, [_ctx, C.c_uint64, _P(Window), C.c_void_p, C.c_void_p, _P(VolumeParams),
                                           _P(VolumeMoments)]),
    "csm_correlative_covariance": (C.c_int, [_ctx, C.c_uint64, _P(Geometry), _P(Scan), C.c_void_p,
                                             _P(CorrelativeParams), _P(VolumeParams), _P(VolumeSummary)]),
    "csm_correlative_covariance_batch": (C.c_int, [_ctx, _P(LoopQuery), C.c_int32, _P(CorrelativeParams),
                                                   _P(VolumeParams), _P(VolumeSummary)]),
    "csm_host_volume_weights": (C.c_int, [C.c_int32, C.c_double, C.c_void_p, _P(C.c_int32)]),
    "csm_host_volume_covariance": (C.c_int, [_P(VolumeMoments), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p]),
    "csm_host_motion_prior": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "csm_host_prior_from_robot_information": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "csm_score_window_prior": (C.c_int, [_ctx, C.c_uint64, _P(Window), C.c_void_p, C.c_void_p, _P(MotionPrior),
                                         _P(PriorResult)]),
    "csm_correlative_match_prior": (C.c_int, [_ctx, C.c_uint64, _P(Geometry), _P(Scan), C.c_void_p,
                                              _P(CorrelativeParams), _P(MotionPrior), _P(PriorSummary)]),
    "csm_correlative_match_prior_batch": (C.c_int, [_ctx, _P(LoopQuery), C.c_int32, _P(CorrelativeParams),
                                                    _P(MotionPrior), _P(PriorSummary)]),
    "csm_host_likelihood_radius": (C.c_int, [C.c_double, C.c_double]),
    "csm_host_likelihood_kernel": (C.c_int, [C.c_double, C.c_double, C.c_int32, C.c_void_p]),
    "csm_host_likelihood_map": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _P(LikelihoodParams), C.c_void_p]),
    "csm_build_likelihood_map": (C.c_int, [_ctx, C.c_uint64, C.c_uint64, _P(LikelihoodParams)]),
    "csm_build_likelihood_maps": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, _P(LikelihoodParams)]),
    "csm_host_distance_kernel": (C.c_int, [C.c_double, C.c_double, C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "csm_host_distance_transform": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "csm_host_distance_map": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _P(DistanceParams), C.c_void_p]),
    "csm_distance_transform": (C.c_int, [_ctx, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]),
    "csm_build_distance_map": (C.c_int, [_ctx, C.c_uint64, C.c_uint64, _P(DistanceParams)]),
    "csm_build_distance_maps": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, _P(DistanceParams)]),
    "csm_host_ray_check_values": (C.c_int, [C.c_double, C.c_double, _P(C.c_uint32), _P(C.c_uint32)]),
    "csm_host_ray_check": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _P(Geometry), _P(Scan), C.c_void_p,
                                     _P(RayCheckParams), _P(RayCheckResult), C.c_void_p]),
    "csm_ray_check_batch": (C.c_int, [_ctx, _P(LoopQuery), C.c_int32, _P(RayCheckParams), _P(RayCheckResult),
                                      C.c_void_p]),
    "csm_host_ray_cast_min_dist2": (C.c_int, [C.c_double, C.c_double, C.c_int32, _P(C.c_int64)]),
    "csm_host_ray_cast_ranges": (C.c_int, [C.c_void_p, C.c_int64, C.c_double, C.c_int32, C.c_double, C.c_void_p]),
    "csm_host_ray_cast": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _P(Geometry), _P(Scan), C.c_void_p, C.c_int32,
                                    _P(RayCastParams), C.c_void_p]),
    "csm_ray_cast": (C.c_int, [_ctx, _P(PoseSet), C.c_int32, _P(RayCastParams), C.c_void_p, _P(RayCastInfo)]),
    "csm_score_pose_sets": (C.c_int, [_ctx, _P(PoseSet), C.c_int32, C.c_void_p, _P(PoseSetsInfo)]),
    "csm_host_score_poses": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _P(Geometry), _P(Scan), C.c_void_p,
                                       C.c_int32, C.c_void_p]),
    "csm_host_score_from_sums": (C.c_int, [C.c_uint32, C.c_uint32, C.c_int32, _P(C.c_double), _P(C.c_double)]),
    "csm_pose_set_update": (C.c_int, [_ctx, _P(PoseSet), _P(PoseUpdateParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                      _P(PoseUpdateInfo), _P(PoseSetsInfo)]),
    "csm_host_pose_set_update": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _P(PoseUpdateParams), C.c_void_p,
                                           C.c_void_p, _P(PoseUpdateInfo)]),
    "csm_bnb_match_batch": (C.c_int, [_ctx, _P(LoopQuery), C.c_int32,
                                      _P(BnbParams), _P(Summary)]),
    "csm_correlative_match_batch": (C.c_int, [_ctx, _P(LoopQuery), C.c_int32,
                                              _P(CorrelativeParams), _P(Summary)]),
    "csm_grid_search_match": (C.c_int, [_ctx, C.c_uint64, _P(Geometry), _P(Scan), C.c_void_p,
                                        _P(GridSearchParams), _P(Summary)]),
    "csm_construct_map_from_scans": (C.c_int, [_ctx, C.c_uint64, _P(MapShape), C.c_void_p, _P(ScanNode),
                                               C.c_int32, _P(MapBuilderParams), _P(MapBuildInfo)]),
    "csm_host_map_resize": (C.c_int, [_P(MapShape), C.c_void_p, C.c_int32, C.c_void_p]),
    "csm_update_map_with_scan": (C.c_int, [_ctx, C.c_uint64, _P(MapShape), C.c_void_p, _P(ScanNode),
                                           _P(MapBuilderParams), _P(MapBuildInfo)]),
    "csm_construct_maps_from_scans": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "csm_host_map_batch_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                          _P(C.c_int32)]),
    "csm_construct_global_map": (C.c_int, [_ctx, C.c_uint64, _P(MapShape), C.c_void_p, _P(ScanNode), C.c_int32,
                                           _P(MapBuilderParams), _P(GlobalMapParams), _P(MapBuildInfo),
                                           _P(GlobalMapInfo)]),
    "csm_host_global_map_parts": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                            _P(C.c_int32)]),
    "csm_host_global_scan_poses": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "csm_set_block_allocation": (C.c_int, [_ctx, C.c_uint64, C.c_int32, C.c_void_p]),
    "csm_cost_covariance_batch": (C.c_int, [_ctx, _P(LoopQuery), C.c_int32, C.c_void_p, C.c_double,
                                            _P(RefineResult)]),
    "csm_linear_solver_batch": (C.c_int, [_ctx, _P(LoopQuery), C.c_int32, _P(RefineParams), _P(RefineResult)]),
    "csm_greedy_cost_covariance_batch": (C.c_int, [_ctx, _P(LoopQuery), C.c_int32, C.c_void_p, _P(GreedyParams),
                                                   _P(HillClimbingResult)]),
    "csm_hill_climbing_batch": (C.c_int, [_ctx, _P(LoopQuery), C.c_int32, _P(HillClimbingParams),
                                          _P(HillClimbingResult)]),
    "csm_host_greedy_cost": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _P(Geometry), _P(Scan), C.c_void_p,
                                       _P(GreedyParams), _P(C.c_double), C.c_void_p]),
    "csm_host_hill_climbing": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _P(Geometry), _P(Scan), C.c_void_p,
                                         _P(HillClimbingParams), _P(HillClimbingResult)]),
    "csm_pose_graph_lm": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, _P(PoseGraphEdge), C.c_int32,
                                    _P(PoseGraphLMParams), _P(C.c_double), _P(PoseGraphLMInfo),
                                    _P(PoseGraphLMStep)]),
    "csm_host_pose_graph_lm": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, _P(PoseGraphEdge), C.c_int32,
                                         _P(PoseGraphLMParams), _P(C.c_double), _P(PoseGraphLMInfo),
                                         _P(PoseGraphLMStep)]),
    "csm_host_pose_graph_loss": (C.c_int, [C.c_int32, C.c_double, C.c_double, _P(C.c_double), _P(C.c_double)]),
    "csm_pose_graph_marginals": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, _P(PoseGraphEdge),
                                           C.c_int32, C.c_int32, C.c_double, _P(PoseGraphPair), C.c_int32,
                                           _P(PoseGraphMarginal), _P(PoseGraphMarginalsInfo)]),
    "csm_host_pose_graph_marginals": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, _P(PoseGraphEdge),
                                                C.c_int32, C.c_int32, C.c_double, _P(PoseGraphPair), C.c_int32,
                                                _P(PoseGraphMarginal), _P(PoseGraphMarginalsInfo)]),
    "csm_host_loop_search_ranges": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "csm_host_loop_gate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _P(C.c_double)]),
    "csm_host_information_from_covariance": (C.c_int, [C.c_void_p, C.c_void_p]),
    "csm_host_travel_distances": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "csm_host_loop_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_int32, _P(LoopSearchParams), C.c_void_p, C.c_void_p,
                                       _P(LoopSearchInfo)]),
    "csm_loop_search": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                  C.c_void_p, C.c_int32, _P(LoopSearchParams), C.c_void_p, C.c_void_p,
                                  _P(LoopSearchInfo)]),
    "csm_host_scan_descriptors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, _P(DescriptorParams),
                                            C.c_void_p, C.c_void_p]),
    "csm_scan_descriptors": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, _P(DescriptorParams),
                                       C.c_void_p, C.c_void_p]),
    "csm_host_descriptor_shift_angle": (C.c_int, [C.c_int32, C.c_int32, _P(C.c_double)]),
    "csm_host_appearance_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_void_p, C.c_void_p, C.c_int32, _P(AppearanceParams), C.c_void_p,
                                             C.c_void_p, _P(LoopSearchInfo)]),
    "csm_appearance_search": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_void_p, C.c_void_p, C.c_int32, _P(AppearanceParams), C.c_void_p,
                                        C.c_void_p, _P(LoopSearchInfo)]),
    "csm_host_loop_candidates_nearest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                                   _P(C.c_int32)]),
    "csm_host_loop_consistency": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, _P(PoseGraphEdge), C.c_int32,
                                            C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                            C.c_void_p, _P(LoopConsistencyInfo), C.c_void_p, C.c_void_p]),
    "csm_loop_consistency": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, _P(PoseGraphEdge), C.c_int32,
                                       C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                       C.c_void_p, _P(LoopConsistencyInfo), C.c_void_p, C.c_void_p]),
    "csm_shard_bounds": (None, [C.c_int32, C.c_int32, C.c_int32, _P(C.c_int32), _P(C.c_int32)]),
    "csm_group_create": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_void_p)]),
    "csm_group_create_ex": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint32, _P(C.c_void_p)]),
    "csm_group_destroy": (C.c_int, [C.c_void_p]),
    "csm_group_size": (C.c_int32, [C.c_void_p]),
    "csm_group_member": (C.c_void_p, [C.c_void_p, C.c_int32]),
    "csm_group_last_error": (C.c_char_p, [C.c_void_p]),
    "csm_group_bnb_match_batch": (C.c_int, [C.c_void_p, _P(LoopQuery), C.c_int32, _P(BnbParams), _P(Summary)]),
    "csm_group_correlative_match_batch": (C.c_int, [C.c_void_p, _P(LoopQuery), C.c_int32,
                                                    _P(CorrelativeParams), _P(Summary)]),
    "csm_allgather_results": (C.c_int, [C.c_void_p, C.c_void_p]),
    "csm_group_gathered_records_dev": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_void_p), _P(C.c_int32)]),
    "csm_group_exchange_info": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_double)]),
    "csm_enable_kernel_timing": (C.c_int, [_ctx, C.c_int32]),
    "csm_kernel_time": (C.c_int, [_ctx, C.c_char_p, _P(C.c_double), _P(C.c_int64)]),
    "csm_reset_kernel_timing": (C.c_int, [_ctx]),
    "csm_version": (C.c_char_p, []),
    "csm_debug_live_bytes": (C.c_int, [_P(C.c_int64), _P(C.c_int64)]),
    "csm_debug_grid_known": (C.c_int, [_ctx, C.c_uint64, _P(C.c_int32)]),
}

_lib = None


def load():
    """Load libcsm_hip.so and declare every entry point. Raises if missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libcsm_hip.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(expected at %s)" % LIB_PATH)
    # A process that also uses PyTorch must end up with ONE HIP runtime: torch ships its
    # own libamdhip64, and whichever of the two runtimes initialises second finds no GPU.
    # Importing torch first makes libcsm_hip.so bind to the copy torch has already loaded
    # (the configuration every GPU test and bench.py run in). Without torch installed the
    # library uses /opt/rocm's runtime, as a C++ caller does.
    if "torch" not in sys.modules and importlib.util.find_spec("torch") is not None:
        import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
