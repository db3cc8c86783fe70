"""Thin Python host layer over the C ABI (include/csm_hip.h).

Mirrors the reference's matcher interface for the hot path:
  ScanMatcherCorrelativeHIP.optimize_pose(...)   <- ScanMatcherCorrelative::OptimizePose
  (src/my_lidar_graph_slam/mapping/scan_matcher_correlative.cpp:92-244)
  LoopDetectorBranchBoundHIP.detect(...)         <- LoopDetectorBranchBound::Detect
  (src/my_lidar_graph_slam/mapping/loop_detector_branch_bound.cpp:59-156)
All arithmetic happens in libcsm_hip.so; this file only marshals numpy arrays.
"""
import contextlib
import ctypes as C
import math

import numpy as np

from . import _lib as L


class CsmError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("csm_hip error %d: %s" % (code, text))
        self.code = code


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _scan_nodes(nodes, as_f64, keep):
    """An array of csm_scan_node for node dicts(pose, angles, ranges, rel_pose, min_range, max_range),
    never of length zero. as_f64 converts an angle or range array; what the array points at is
    appended to keep."""
    arr = (L.ScanNode * max(len(nodes), 1))()
    for i, nd in enumerate(nodes):
        a_, r_ = as_f64(nd["angles"]), as_f64(nd["ranges"])
        keep += [a_, r_]
        arr[i].global_pose[:] = list(nd["pose"])
        arr[i].scan.angles = a_.ctypes.data_as(C.POINTER(C.c_double))
        arr[i].scan.ranges = r_.ctypes.data_as(C.POINTER(C.c_double))
        arr[i].scan.n_points = a_.size
        arr[i].scan.relative_sensor_pose[:] = list(nd.get("rel_pose", (0.0, 0.0, 0.0)))
        arr[i].min_range = nd.get("min_range", 0.0)
        arr[i].max_range = nd.get("max_range", 1e9)
    keep.append(arr)
    return arr


def result_to_dict(r):
    return dict(found=int(r.found), best_x=int(r.best_x), best_y=int(r.best_y),
                best_theta=int(r.best_theta), key=int(r.key),
                sum_values=int(r.sum_values), known=int(r.known),
                tie_count=int(r.tie_count), flags=int(r.flags), score=float(r.score))


def summary_to_dict(s):
    return dict(pose_found=int(s.pose_found), win_x=s.win_x, win_y=s.win_y,
                win_theta=s.win_theta, step_x=s.step_x, step_y=s.step_y,
                step_theta=s.step_theta, sensor_pose=list(s.sensor_pose),
                best_sensor_pose=list(s.best_sensor_pose),
                estimated_pose=list(s.estimated_pose),
                input_setup_us=s.input_setup_us, optimization_us=s.optimization_us,
                candidates=int(s.candidates), raw=result_to_dict(s.raw))


class PreparedQueries:
    """Context.prepare_queries()'s result: the csm_loop_query array plus the
    numpy arrays its pointers refer to."""

    def __init__(self, arr, keep):
        self.arr, self.keep, self.n = arr, keep, len(arr)


class SummaryArray:
    """The csm_summary array of a batch call, converted on demand."""

    def __init__(self, out):
        self.out = out

    def __len__(self):
        return len(self.out)

    def __getitem__(self, i):
        return summary_to_dict(self.out[i])

    def __iter__(self):
        return (summary_to_dict(o) for o in self.out)

    def record_bytes(self):
        """The 48-byte csm_result of every query, back to back (what the ranks all-gather)."""
        n, size, off = len(self.out), C.sizeof(L.Summary), L.Summary.raw.offset
        flat = np.frombuffer(self.out, dtype=np.uint8).reshape(n, size)
        return np.ascontiguousarray(flat[:, off:off + C.sizeof(L.Result)]).reshape(-1)

    def total(self, field):
        return sum(int(getattr(o, field)) for o in self.out)


# ---- host-only helpers (no GPU needed) ----

def host_search_step(resolution, ranges):
    lib = L.load()
    r = _f64(ranges)
    sx, sy, st = C.c_double(), C.c_double(), C.c_double()
    rc = lib.csm_host_search_step(resolution, _ptr(r), r.size, C.byref(sx), C.byref(sy), C.byref(st))
    if rc:
        raise CsmError(rc, "csm_host_search_step")
    return sx.value, sy.value, st.value


def host_map_resize(shape, box, expand=False):
    """GridMap::Resize / Expand on an index box (min col, min row, max col, max
    row; inclusive). Returns (new shape dict, (first row, first col) in the old frame)."""
    sh = L.MapShape(shape["res"], shape["off_x"], shape["off_y"], shape["rows"], shape["cols"],
                    shape["log2_block"])
    b = np.ascontiguousarray(box, dtype=np.int32)
    shift = np.zeros(2, np.int32)
    rc = L.load().csm_host_map_resize(C.byref(sh), _ptr(b), 1 if expand else 0, _ptr(shift))
    if rc:
        raise CsmError(rc, "csm_host_map_resize")
    return (dict(res=sh.resolution, off_x=sh.offset_x, off_y=sh.offset_y, rows=sh.rows, cols=sh.cols,
                 log2_block=sh.log2_block_size), (int(shift[0]), int(shift[1])))


def host_map_batch_plan(n_beams, n_cells_upper, scratch_limit_bytes=0):
    """csm_host_map_batch_plan: how csm_construct_maps_from_scans cuts its jobs into chunks. Returns
    (chunk of each job, scratch bytes of each chunk); 0 = the default limit of 1 GiB."""
    nb = np.ascontiguousarray(n_beams, dtype=np.int64)
    nc = np.ascontiguousarray(n_cells_upper, dtype=np.int64)
    if nb.ndim != 1 or nb.shape != nc.shape:
        raise ValueError("n_beams and n_cells_upper must be 1-D and equally long")
    chunk_of = np.zeros(max(nb.size, 1), np.int32)
    chunk_bytes = np.zeros(max(nb.size, 1), np.int64)
    n_chunks = C.c_int32(0)
    rc = L.load().csm_host_map_batch_plan(_ptr(nb), _ptr(nc), nb.size, int(scratch_limit_bytes), _ptr(chunk_of),
                                          _ptr(chunk_bytes), C.byref(n_chunks))
    if rc:
        raise CsmError(rc, "csm_host_map_batch_plan")
    return [int(c) for c in chunk_of[:nb.size]], [int(b) for b in chunk_bytes[:n_chunks.value]]


def host_global_map_parts(n_beams, n_cells, scratch_limit_bytes=0):
    """csm_host_global_map_parts: how csm_construct_global_map cuts its nodes into parts, given each
    node's beams and the cells of the resized map. Returns (part of each node, scratch bytes of each
    part); 0 = the default limit of 1 GiB."""
    nb = np.ascontiguousarray(n_beams, dtype=np.int64)
    if nb.ndim != 1:
        raise ValueError("n_beams must be 1-D")
    part_of = np.zeros(max(nb.size, 1), np.int32)
    part_bytes = np.zeros(max(nb.size, 1), np.int64)
    n_parts = C.c_int32(0)
    rc = L.load().csm_host_global_map_parts(_ptr(nb), nb.size, int(n_cells), int(scratch_limit_bytes),
                                            _ptr(part_of), _ptr(part_bytes), C.byref(n_parts))
    if rc:
        raise CsmError(rc, "csm_host_global_map_parts")
    return [int(c) for c in part_of[:nb.size]], [int(b) for b in part_bytes[:n_parts.value]]


def host_global_scan_poses(local_map_pose, local_poses):
    """csm_host_global_scan_poses: Compound(local map pose, each scan node's local pose), as
    GridMapBuilder::ConstructMapFromAllScans composes them. Returns an (n, 3) array."""
    lp = np.ascontiguousarray(local_poses, dtype=np.float64).reshape(-1, 3)
    out = np.zeros_like(lp)
    rc = L.load().csm_host_global_scan_poses(_ptr(_f64(local_map_pose)), _ptr(lp), lp.shape[0], _ptr(out))
    if rc:
        raise CsmError(rc, "csm_host_global_scan_poses")
    return out


def debug_live_bytes():
    """csm_debug_live_bytes: (device, pinned) bytes the library holds, over the whole process."""
    dev, pin = C.c_int64(0), C.c_int64(0)
    L.load().csm_debug_live_bytes(C.byref(dev), C.byref(pin))
    return dev.value, pin.value


def host_window(rng, step):
    return L.load().csm_host_window(rng, step)


def host_min_known(n, thr):
    return L.load().csm_host_min_known(n, thr)


def host_compound(a, b):
    out = np.zeros(3)
    L.load().csm_host_compound(_ptr(_f64(a)), _ptr(_f64(b)), _ptr(out))
    return out


def host_inverse_compound(a, b):
    out = np.zeros(3)
    L.load().csm_host_inverse_compound(_ptr(_f64(a)), _ptr(_f64(b)), _ptr(out))
    return out


def host_move_backward(a, b):
    out = np.zeros(3)
    L.load().csm_host_move_backward(_ptr(_f64(a)), _ptr(_f64(b)), _ptr(out))
    return out


def host_project(geom, sensor_pose, step_theta, win_theta, angles, ranges, want_products=False):
    lib = L.load()
    a, r = _f64(angles), _f64(ranges)
    n, nt = a.size, 2 * win_theta + 1
    col = np.zeros((nt, n), np.int32)
    row = np.zeros((nt, n), np.int32)
    rc_ = np.zeros((nt, n)) if want_products else None
    rs_ = np.zeros((nt, n)) if want_products else None
    g = L.Geometry(*geom)
    sp = _f64(sensor_pose)
    rc = lib.csm_host_project(C.byref(g), _ptr(sp), step_theta, win_theta, _ptr(a), _ptr(r), n,
                              _ptr(col), _ptr(row),
                              _ptr(rc_) if want_products else None,
                              _ptr(rs_) if want_products else None)
    if rc:
        raise CsmError(rc, "csm_host_project")
    return (col, row, rc_, rs_) if want_products else (col, row)


def greedy_params(map_resolution=0.05, hit_and_missed_dist=0.075, occupancy_threshold=0.1, kernel_size=1,
                  standard_deviation=0.05, scaling_factor=1.0):
    """csm_greedy_params; defaults as launcher_settings_default.json "CostGreedyEndpoint"."""
    return L.GreedyParams(map_resolution, hit_and_missed_dist, occupancy_threshold, kernel_size, 0,
                          standard_deviation, scaling_factor)


def hill_climbing_params(linear_step=0.1, angular_step=0.1, max_iterations=100, max_refinements=5, greedy=None):
    g = greedy if isinstance(greedy, L.GreedyParams) else greedy_params(**(greedy or {}))
    return L.HillClimbingParams(linear_step, angular_step, max_iterations, max_refinements, g)


def _scan_struct(angles, ranges, rel_pose):
    a, r = _f64(angles), _f64(ranges)
    sc = L.Scan()
    sc.angles = a.ctypes.data_as(C.POINTER(C.c_double))
    sc.ranges = r.ctypes.data_as(C.POINTER(C.c_double))
    sc.n_points = a.size
    sc.relative_sensor_pose[:] = list(rel_pose)
    return sc, (a, r)


def _correlative_params(range_x, range_y, range_theta, low_resolution, score_threshold, known_rate_threshold):
    p = L.CorrelativeParams()
    p.range_x, p.range_y, p.range_theta = range_x, range_y, range_theta
    p.low_resolution = low_resolution
    p.score_threshold, p.known_rate_threshold = score_threshold, known_rate_threshold
    return p


def _hits(hit_col, hit_row):
    """The hit indices of a pre-projected window as the C ABI takes them."""
    return np.ascontiguousarray(hit_col, dtype=np.int32), np.ascontiguousarray(hit_row, dtype=np.int32)


def host_greedy_cost(grid, geom, angles, ranges, sensor_pose, greedy=None, covariance=False):
    """csm_host_greedy_cost: Cost() (ScalingFactor applied, not normalized), and
    ComputeCovariance() if asked."""
    g = np.ascontiguousarray(grid, dtype=np.uint16)
    sc, keep = _scan_struct(angles, ranges, (0.0, 0.0, 0.0))
    p = greedy if isinstance(greedy, L.GreedyParams) else greedy_params(**(greedy or {}))
    cost = C.c_double()
    cov = np.zeros(9)
    rc = L.load().csm_host_greedy_cost(_ptr(g), g.shape[0], g.shape[1], C.byref(L.Geometry(*geom)),
                                       C.byref(sc), _ptr(_f64(sensor_pose)), C.byref(p), C.byref(cost),
                                       _ptr(cov) if covariance else None)
    if rc:
        raise CsmError(rc, "csm_host_greedy_cost")
    return (cost.value, cov.reshape(3, 3)) if covariance else cost.value


def host_hill_climbing(grid, geom, angles, ranges, rel_pose, init_pose, linear_step=0.1, angular_step=0.1,
                       max_iterations=100, max_refinements=5, greedy=None):
    """csm_host_hill_climbing: the library's host restatement of OptimizePose."""
    g = np.ascontiguousarray(grid, dtype=np.uint16)
    sc, keep = _scan_struct(angles, ranges, rel_pose)
    p = hill_climbing_params(linear_step, angular_step, max_iterations, max_refinements, greedy)
    out = L.HillClimbingResult()
    rc = L.load().csm_host_hill_climbing(_ptr(g), g.shape[0], g.shape[1], C.byref(L.Geometry(*geom)),
                                         C.byref(sc), _ptr(_f64(init_pose)), C.byref(p), C.byref(out))
    if rc:
        raise CsmError(rc, "csm_host_hill_climbing")
    return Context._hill_to_dict(out)


def host_volume_weights(n_points, temperature):
    """(table uint32[VOLUME_BINS], bin_shift): the fixed-point weights of the volume covariance
    (csm_host_volume_weights)."""
    table = np.zeros(L.VOLUME_BINS, np.uint32)
    shift = C.c_int32(0)
    rc = L.load().csm_host_volume_weights(n_points, temperature, _ptr(table), C.byref(shift))
    if rc != 0:
        raise CsmError(rc, "csm_host_volume_weights")
    return table, shift.value


def moments_struct(m):
    """csm_volume_moments from a dict with m0, m1[3], m2[6] (the other fields default to 0)."""
    out = L.VolumeMoments()
    out.m0 = m["m0"]
    out.m1[:] = list(m["m1"])
    out.m2[:] = list(m["m2"])
    out.support, out.border_support = m.get("support", 0), m.get("border_support", 0)
    out.bin_shift = m.get("bin_shift", 0)
    return out


def host_volume_covariance(moments, steps, estimated_pose, rel_pose):
    """(mean_offset[3], sensor_covariance[9], covariance[9]) as lists of floats, from a moments dict
    (csm_host_volume_covariance)."""
    m = moments_struct(moments)
    st, est, rel = _f64(steps), _f64(estimated_pose), _f64(rel_pose)
    mean, scov, cov = np.zeros(3), np.zeros(9), np.zeros(9)
    rc = L.load().csm_host_volume_covariance(C.byref(m), _ptr(st), _ptr(est), _ptr(rel), _ptr(mean), _ptr(scov),
                                             _ptr(cov))
    if rc != 0:
        raise CsmError(rc, "csm_host_volume_covariance")
    return mean.tolist(), scov.tolist(), cov.tolist()


def moments_to_dict(m):
    return dict(best=result_to_dict(m.best), m0=m.m0, m1=list(m.m1), m2=list(m.m2), support=m.support,
                border_support=m.border_support, bin_shift=m.bin_shift)


def volume_summary_to_dict(v):
    return dict(summary=summary_to_dict(v.summary), moments=moments_to_dict(v.moments),
                mean_offset=list(v.mean_offset), sensor_covariance=list(v.sensor_covariance),
                covariance=list(v.covariance))


def host_motion_prior(information, steps, n_points, d_max):
    """Q[6] (Python ints, order xx xy xt yy yt tt): the quantised prior terms of a 3 x 3 information matrix
    (csm_host_motion_prior). d_max = max(n_theta, nx, ny) - 1 of the window."""
    lam, st = _f64(information).reshape(-1), _f64(steps)
    if lam.size != 9 or st.size != 3:
        raise CsmError(L.CSM_EINVAL, "host_motion_prior: information must be 3 x 3, steps 3")
    q = np.zeros(6, np.int64)
    rc = L.load().csm_host_motion_prior(_ptr(lam), _ptr(st), n_points, d_max, _ptr(q))
    if rc != 0:
        raise CsmError(rc, "csm_host_motion_prior")
    return [int(v) for v in q]


def host_prior_from_robot_information(robot_information, initial_pose, rel_pose):
    """The 9 doubles of J^T Lambda_robot J: the information of the sensor pose from that of the robot pose
    (csm_host_prior_from_robot_information)."""
    lam, init, rel = _f64(robot_information).reshape(-1), _f64(initial_pose), _f64(rel_pose)
    if lam.size != 9:
        raise CsmError(L.CSM_EINVAL, "host_prior_from_robot_information: information must be 3 x 3")
    out = np.zeros(9)
    rc = L.load().csm_host_prior_from_robot_information(_ptr(lam), _ptr(init), _ptr(rel), _ptr(out))
    if rc != 0:
        raise CsmError(rc, "csm_host_prior_from_robot_information")
    return out.tolist()


def motion_prior(information, steps=(0.0, 0.0, 0.0), scratch_limit_bytes=0):
    """csm_motion_prior from a 3 x 3 (or flat, row-major) information matrix."""
    lam = _f64(information).reshape(-1)
    if lam.size != 9:
        raise CsmError(L.CSM_EINVAL, "motion_prior: information must be 3 x 3")
    p = L.MotionPrior()
    p.information[:] = lam.tolist()
    p.steps[:] = list(steps)
    p.scratch_limit_bytes = scratch_limit_bytes
    return p


def prior_result_to_dict(r):
    return dict(best=result_to_dict(r.best), unweighted=result_to_dict(r.unweighted), penalty=int(r.penalty),
                penalised_key=int(r.penalised_key), Q=[int(v) for v in r.Q])


def prior_summary_to_dict(v):
    return dict(summary=summary_to_dict(v.summary), prior=prior_result_to_dict(v.prior))


def host_likelihood_radius(sigma, resolution):
    """ceil(3 sigma / resolution) clamped to 1..LIKELIHOOD_MAX_RADIUS (csm_host_likelihood_radius)."""
    r = L.load().csm_host_likelihood_radius(sigma, resolution)
    if r < 0:
        raise CsmError(r, "csm_host_likelihood_radius")
    return r


def host_likelihood_kernel(sigma, resolution, radius):
    """T[0 .. radius^2] as uint32: the integer Gaussian of a likelihood field, indexed by the squared cell
    distance (csm_host_likelihood_kernel)."""
    if not 1 <= radius <= L.LIKELIHOOD_MAX_RADIUS:
        raise CsmError(L.CSM_EINVAL, "host_likelihood_kernel: radius out of range")
    table = np.zeros(radius * radius + 1, np.uint32)
    rc = L.load().csm_host_likelihood_kernel(sigma, resolution, radius, _ptr(table))
    if rc != 0:
        raise CsmError(rc, "csm_host_likelihood_kernel")
    return table


def likelihood_params(sigma=None, resolution=None, radius=None, occupied_min=32768, keep_unknown=False,
                      kernel=None):
    """(csm_likelihood_params, the table it points at): the table is `kernel` if given (radius required), else
    that of (sigma, resolution) at `radius` (default: host_likelihood_radius). Keep the table alive with the
    struct."""
    if kernel is None:
        if radius is None:
            radius = host_likelihood_radius(sigma, resolution)
        kernel = host_likelihood_kernel(sigma, resolution, radius)
    elif radius is None:
        raise CsmError(L.CSM_EINVAL, "likelihood_params: a kernel table needs its radius")
    table = np.ascontiguousarray(kernel, dtype=np.uint32)
    if 1 <= radius <= L.LIKELIHOOD_MAX_RADIUS and table.size < radius * radius + 1:
        raise CsmError(L.CSM_EINVAL, "likelihood_params: the table needs radius^2 + 1 entries")
    p = L.LikelihoodParams(radius, occupied_min, 1 if keep_unknown else 0, 0, table.ctypes.data)
    return p, table


def host_likelihood_map(grid, sigma=None, resolution=None, radius=None, occupied_min=32768, keep_unknown=False,
                        kernel=None):
    """The likelihood field of a dense uint16 grid on the host (csm_host_likelihood_map): the definition
    the device build is compared with."""
    g = np.ascontiguousarray(grid, dtype=np.uint16)
    p, table = likelihood_params(sigma, resolution, radius, occupied_min, keep_unknown, kernel)
    out = np.zeros_like(g)
    rc = L.load().csm_host_likelihood_map(_ptr(g), g.shape[0], g.shape[1], C.byref(p), _ptr(out))
    if rc != 0:
        raise CsmError(rc, "csm_host_likelihood_map")
    return out


def host_distance_kernel(sigma, resolution, radius, peak=65534, floor_value=1):
    """T[0 .. radius^2] as uint16: floor_value + the integer Gaussian of height peak - floor_value, indexed by
    the squared cell distance (csm_host_distance_kernel)."""
    if not 1 <= radius <= L.DISTANCE_MAX_RADIUS:
        raise CsmError(L.CSM_EINVAL, "host_distance_kernel: radius out of range")
    table = np.zeros(radius * radius + 1, np.uint16)
    rc = L.load().csm_host_distance_kernel(sigma, resolution, radius, peak, floor_value, _ptr(table))
    if rc != 0:
        raise CsmError(rc, "csm_host_distance_kernel")
    return table


def distance_params(sigma=None, resolution=None, radius=None, occupied_min=32768, keep_unknown=False, table=None,
                    peak=65534, floor_value=1):
    """(csm_distance_params, the table it points at): the table is `table` if given (radius required), else
    that of (sigma, resolution, peak, floor_value) at `radius` (default: ceil(3 sigma / resolution) clamped to
    1..DISTANCE_MAX_RADIUS). Keep the table alive with the struct."""
    if table is None:
        if radius is None:
            if not (sigma is not None and resolution is not None and sigma > 0 and resolution > 0):
                raise CsmError(L.CSM_EINVAL, "distance_params: sigma and resolution > 0, or a table")
            radius = int(min(float(L.DISTANCE_MAX_RADIUS), max(1.0, math.ceil(3.0 * (sigma / resolution)))))
        table = host_distance_kernel(sigma, resolution, radius, peak, floor_value)
    elif radius is None:
        raise CsmError(L.CSM_EINVAL, "distance_params: a table needs its radius")
    t = np.asarray(table)
    if t.size and (t.min() < 0 or t.max() > 65535):
        raise CsmError(L.CSM_EINVAL, "distance_params: table entries are uint16")
    t = np.ascontiguousarray(t, dtype=np.uint16)
    if 1 <= radius <= L.DISTANCE_MAX_RADIUS and t.size < radius * radius + 1:
        raise CsmError(L.CSM_EINVAL, "distance_params: the table needs radius^2 + 1 entries")
    p = L.DistanceParams(radius, occupied_min, 1 if keep_unknown else 0, 0, t.ctypes.data)
    return p, t


def host_distance_transform(grid, occupied_min=32768):
    """(d2, nearest) of a dense uint16 grid on the host, uint32 each (csm_host_distance_transform):
    DISTANCE_NONE everywhere when the grid has no obstacle."""
    g = np.ascontiguousarray(grid, dtype=np.uint16)
    d2, nearest = np.zeros(g.shape, np.uint32), np.zeros(g.shape, np.uint32)
    rc = L.load().csm_host_distance_transform(_ptr(g), g.shape[0], g.shape[1], occupied_min, _ptr(d2), _ptr(nearest))
    if rc != 0:
        raise CsmError(rc, "csm_host_distance_transform")
    return d2, nearest


def host_distance_map(grid, sigma=None, resolution=None, radius=None, occupied_min=32768, keep_unknown=False,
                      table=None, peak=65534, floor_value=1):
    """The distance field of a dense uint16 grid on the host (csm_host_distance_map): what the device build
    is compared with."""
    g = np.ascontiguousarray(grid, dtype=np.uint16)
    p, t = distance_params(sigma, resolution, radius, occupied_min, keep_unknown, table, peak, floor_value)
    out = np.zeros_like(g)
    rc = L.load().csm_host_distance_map(_ptr(g), g.shape[0], g.shape[1], C.byref(p), _ptr(out))
    if rc != 0:
        raise CsmError(rc, "csm_host_distance_map")
    return out


def host_ray_check_values(prob_occupied=0.65, prob_free=0.35):
    """csm_host_ray_check_values: (occupied_min, free_max), the raw cell values at two probabilities."""
    occ, fre = C.c_uint32(), C.c_uint32()
    rc = L.load().csm_host_ray_check_values(prob_occupied, prob_free, C.byref(occ), C.byref(fre))
    if rc:
        raise CsmError(rc, "csm_host_ray_check_values")
    return occ.value, fre.value


def ray_check_params(usable_range_min=0.01, usable_range_max=20.0, subpixel_scale=100, occupied_min=None,
                     free_max=None, end_tolerance=1, scratch_limit_bytes=0):
    """A csm_ray_check_params. occupied_min / free_max default to the values of P = 0.65 / 0.35."""
    if occupied_min is None or free_max is None:
        occ, fre = host_ray_check_values()
        occupied_min = occ if occupied_min is None else occupied_min
        free_max = fre if free_max is None else free_max
    return L.RayCheckParams(usable_range_min, usable_range_max, subpixel_scale, end_tolerance, occupied_min,
                            free_max, scratch_limit_bytes)


RAY_CHECK_FIELDS = tuple(name for name, _ in L.RayCheckResult._fields_)


def ray_check_to_dict(r):
    return {name: int(getattr(r, name)) for name in RAY_CHECK_FIELDS}


def host_ray_check(grid, geom, angles, ranges, rel_pose, pose, per_beam=False, params=None, **kw):
    """csm_host_ray_check: the free-space check of one scan at the robot pose `pose` on a dense grid, as a
    dict of the record's fields; with per_beam also the int32 word of every beam."""
    g = np.ascontiguousarray(grid, dtype=np.uint16)
    sc, keep = _scan_struct(angles, ranges, rel_pose)
    p = params if params is not None else ray_check_params(**kw)
    out = L.RayCheckResult()
    words = np.zeros(max(sc.n_points, 1), np.int32)
    rc = L.load().csm_host_ray_check(_ptr(g), g.shape[0], g.shape[1], C.byref(L.Geometry(*geom)), C.byref(sc),
                                     _ptr(_f64(pose)), C.byref(p), C.byref(out), _ptr(words) if per_beam else None)
    if rc:
        raise CsmError(rc, "csm_host_ray_check")
    return (ray_check_to_dict(out), words[:sc.n_points]) if per_beam else ray_check_to_dict(out)


CAST_RECORD = np.dtype([("cell_x", "<i4"), ("cell_y", "<i4"), ("value", "<u4"), ("kind", "<i4"), ("dist2", "<i8")])
CAST_NONE, CAST_OCCUPIED, CAST_UNKNOWN = L.CAST_NONE, L.CAST_OCCUPIED, L.CAST_UNKNOWN


def ray_cast_params(range_max=20.0, range_min=0.0, subpixel_scale=100, occupied_min=None, unknown_stops=0,
                    scratch_limit_bytes=0):
    """A csm_ray_cast_params. occupied_min defaults to the value of P = 0.65 (host_ray_check_values)."""
    if occupied_min is None:
        occupied_min = host_ray_check_values()[0]
    return L.RayCastParams(range_max, range_min, subpixel_scale, occupied_min, int(unknown_stops), 0,
                           scratch_limit_bytes)


def ray_cast_info_to_dict(i):
    return dict(rays=int(i.rays), host_rays=int(i.host_rays), cells_read=int(i.cells_read),
                cells_to_stop=int(i.cells_to_stop), host_us=float(i.host_us), device_us=float(i.device_us))


def _cast_scan(angles, ranges):
    """A csm_scan as the cast reads it: beam angles, and limits or None (a null pointer)."""
    a = _f64(angles).reshape(-1)
    r = None if ranges is None else _f64(ranges).reshape(-1)
    if r is not None and r.size != a.size:
        raise CsmError(L.CSM_EINVAL, "ray cast: one limit per angle")
    sc = L.Scan()
    sc.n_points = a.size
    if a.size:                           # never a pointer to nothing
        sc.angles = a.ctypes.data_as(C.POINTER(C.c_double))
        if r is not None:
            sc.ranges = r.ctypes.data_as(C.POINTER(C.c_double))
    return sc, (a, r)


def host_ray_cast_min_dist2(range_min, resolution, subpixel_scale):
    """csm_host_ray_cast_min_dist2: the least dist2 a stopping cell may have."""
    out = C.c_int64()
    rc = L.load().csm_host_ray_cast_min_dist2(range_min, resolution, subpixel_scale, C.byref(out))
    if rc:
        raise CsmError(rc, "csm_host_ray_cast_min_dist2")
    return out.value


def host_ray_cast_ranges(records, resolution, subpixel_scale, none_value=0.0):
    """csm_host_ray_cast_ranges: the f64 range of every record (any shape), none_value where it did not stop."""
    rec = np.ascontiguousarray(records, dtype=CAST_RECORD)
    out = np.zeros(rec.shape, np.float64)
    rc = L.load().csm_host_ray_cast_ranges(_ptr(rec) if rec.size else None, rec.size, resolution, subpixel_scale,
                                           none_value, _ptr(out) if rec.size else None)
    if rc:
        raise CsmError(rc, "csm_host_ray_cast_ranges")
    return out


def host_ray_cast(grid, geom, angles, poses, ranges=None, params=None, **kw):
    """csm_host_ray_cast: beams at `angles` cast from every map-local sensor pose of `poses` (n, 3) through a
    dense grid, step by step: a CAST_RECORD array (n, len(angles)). ranges: a limit per beam, or None."""
    g = np.ascontiguousarray(grid, dtype=np.uint16)
    sc, keep = _cast_scan(angles, ranges)
    p = _poses(poses)
    prm = params if params is not None else ray_cast_params(**kw)
    out = np.zeros((p.shape[0], sc.n_points), CAST_RECORD)
    rc = L.load().csm_host_ray_cast(_ptr(g), g.shape[0], g.shape[1], C.byref(L.Geometry(*geom)), C.byref(sc),
                                    _ptr(p) if p.size else None, p.shape[0], C.byref(prm),
                                    _ptr(out) if out.size else None)
    if rc:
        raise CsmError(rc, "csm_host_ray_cast")
    return out


POSE_RECORD = np.dtype([("sum_values", "<u4"), ("known", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])


def _poses(poses):
    p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    return p


def host_score_poses(grid, geom, angles, ranges, poses):
    """csm_host_score_poses: the (S, K) record of the scan at every map-local sensor pose of `poses` (n, 3) on
    a dense grid, as a POSE_RECORD array."""
    g = np.ascontiguousarray(grid, dtype=np.uint16)
    sc, keep = _scan_struct(angles, ranges, (0.0, 0.0, 0.0))
    p = _poses(poses)
    out = np.zeros(p.shape[0], POSE_RECORD)
    rc = L.load().csm_host_score_poses(_ptr(g), g.shape[0], g.shape[1], C.byref(L.Geometry(*geom)), C.byref(sc),
                                       _ptr(p), p.shape[0], _ptr(out))
    if rc:
        raise CsmError(rc, "csm_host_score_poses")
    return out


def host_score_from_sums(sum_values, known, n_points):
    """csm_host_score_from_sums: (normalised score, known rate) of a record."""
    score, rate = C.c_double(), C.c_double()
    rc = L.load().csm_host_score_from_sums(int(sum_values), int(known), n_points, C.byref(score), C.byref(rate))
    if rc:
        raise CsmError(rc, "csm_host_score_from_sums")
    return score.value, rate.value


def pose_update_to_dict(u):
    return dict(m0=int(u.m0), key_max=int(u.key_max), best_index=int(u.best_index), support=int(u.support),
                bin_shift=int(u.bin_shift), found=int(u.found))


def pose_sets_info_to_dict(i):
    return dict(poses=int(i.poses), uncertain_poses=int(i.uncertain_poses), changed_poses=int(i.changed_poses),
                host_us=float(i.host_us), device_us=float(i.device_us))


def host_pose_set_update(records, n_points, temperature, known_rate_threshold=0.0, n_out=None, offset=0):
    """csm_host_pose_set_update on a POSE_RECORD array: (weights uint32, ancestors int32, update dict)."""
    rec = np.ascontiguousarray(records, dtype=POSE_RECORD)
    n_out = rec.size if n_out is None else n_out
    prm = L.PoseUpdateParams(temperature, known_rate_threshold, n_out, 0, offset & 0xFFFFFFFFFFFFFFFF)
    weights = np.zeros(max(rec.size, 1), np.uint32)
    ancestors = np.zeros(max(n_out, 1), np.int32)
    upd = L.PoseUpdateInfo()
    rc = L.load().csm_host_pose_set_update(_ptr(rec), rec.size, n_points, C.byref(prm), _ptr(weights),
                                           _ptr(ancestors), C.byref(upd))
    if rc:
        raise CsmError(rc, "csm_host_pose_set_update")
    return weights[:rec.size], ancestors[:max(n_out, 0)], pose_update_to_dict(upd)


def effective_sample_size(weights):
    """(sum w)^2 / sum w^2 in f64, 0.0 when every weight is 0 (not part of the C ABI)."""
    w = np.asarray(weights, dtype=np.float64)
    s2 = float(np.sum(w * w))
    return float(np.sum(w)) ** 2 / s2 if s2 > 0.0 else 0.0


def host_probability_lut():
    lut = np.zeros(65536)
    L.load().csm_host_probability_lut(_ptr(lut))
    return lut


PG_SOLVERS = {"SparseCholesky": L.PG_SOLVER_SPARSE_CHOLESKY, "ConjugateGradient": L.PG_SOLVER_CONJUGATE_GRADIENT,
              "SchurCholesky": L.PG_SOLVER_SCHUR_CHOLESKY}
PG_LOSSES = {"Squared": L.PG_LOSS_SQUARED, "Huber": L.PG_LOSS_HUBER, "Cauchy": L.PG_LOSS_CAUCHY,
             "Fair": L.PG_LOSS_FAIR, "GemanMcClure": L.PG_LOSS_GEMAN_MCCLURE, "Welsch": L.PG_LOSS_WELSCH}


def pose_graph_params(iterations_max=10, error_tolerance=1e-4, solver="ConjugateGradient", loss="Huber",
                      loss_scale=0.01):
    """csm_pose_graph_lm_params; defaults as launcher_settings_default.json "PoseGraphOptimizerLM".
    solver / loss: a name (SolverType, LossFunctionType) or the CSM_PG_* number."""
    st = PG_SOLVERS[solver] if isinstance(solver, str) else int(solver)
    lt = PG_LOSSES[loss] if isinstance(loss, str) else int(loss)
    return L.PoseGraphLMParams(int(iterations_max), st, lt, 0, float(error_tolerance), float(loss_scale))


def pose_graph_edges(edges):
    """A csm_pose_graph_edge array from dicts {local, scan, rel (3), info (3x3 or 9), loop}
    (EdgePose: mLocalMapNodeIdx, mScanNodeIdx, mRelativePose, mInformationMat, mIsLoopConstraint)."""
    if isinstance(edges, C.Array):
        return edges
    arr = (L.PoseGraphEdge * max(len(edges), 1))()
    for e, d in zip(arr, edges):
        e.local_map_index = int(d["local"])
        e.scan_index = int(d["scan"])
        e.is_loop = 1 if d.get("loop") else 0
        e.relative_pose[:] = [float(v) for v in d["rel"]]
        e.information[:] = [float(v) for v in np.asarray(d["info"], dtype=np.float64).reshape(9)]
    return arr


def _pose_graph_run(fn, head, local_poses, scan_poses, edges, lambda_, params):
    lp = np.array(local_poses, dtype=np.float64).reshape(-1, 3)
    sp = np.array(scan_poses, dtype=np.float64).reshape(-1, 3)
    ea = pose_graph_edges(edges)
    n_edges = len(edges)
    lam = C.c_double(lambda_)
    info = L.PoseGraphLMInfo()
    trace = (L.PoseGraphLMStep * max(params.iterations_max, 1))()
    rc = fn(*head, _ptr(lp), lp.shape[0], _ptr(sp), sp.shape[0], ea, n_edges, C.byref(params), C.byref(lam),
            C.byref(info), trace)
    out = dict(steps=info.steps, cg_iterations=int(info.cg_iterations), initial_error=info.initial_error,
               final_error=info.final_error, lambda_=lam.value,
               trace=[dict(total_error=t.total_error, lambda_=t.lambda_, rhs_norm2=t.rhs_norm2,
                           residual_norm2=t.residual_norm2,
                           cg_iterations=t.cg_iterations) for t in trace[:info.steps]] if rc == 0 else [])
    return rc, lp, sp, out


def host_pose_graph_lm(local_poses, scan_poses, edges, lambda_=1e-4, params=None, **kw):
    """csm_host_pose_graph_lm: the library's sequential restatement of PoseGraphOptimizerLM::Optimize.
    Returns (local poses [n, 3], scan poses [m, 3], info dict with the per-step trace and the final
    lambda_). params: pose_graph_params(...), or its keyword arguments."""
    p = params if params is not None else pose_graph_params(**kw)
    rc, lp, sp, out = _pose_graph_run(L.load().csm_host_pose_graph_lm, (), local_poses, scan_poses, edges,
                                      lambda_, p)
    if rc:
        raise CsmError(rc, "csm_host_pose_graph_lm")
    return lp, sp, out


def host_pose_graph_loss(loss, scale, squared_error):
    """(Loss(t), Weight(t)) of a robust loss function (csm_host_pose_graph_loss)."""
    lo, w = C.c_double(), C.c_double()
    lt = PG_LOSSES[loss] if isinstance(loss, str) else int(loss)
    rc = L.load().csm_host_pose_graph_loss(lt, scale, squared_error, C.byref(lo), C.byref(w))
    if rc:
        raise CsmError(rc, "csm_host_pose_graph_loss")
    return lo.value, w.value


def _pose_graph_marginals_run(fn, head, local_poses, scan_poses, edges, pairs, loss, loss_scale):
    lp = np.array(local_poses, dtype=np.float64).reshape(-1, 3)
    sp = np.array(scan_poses, dtype=np.float64).reshape(-1, 3)
    ea = pose_graph_edges(edges)
    lt = PG_LOSSES[loss] if isinstance(loss, str) else int(loss)
    pa = (L.PoseGraphPair * max(len(pairs), 1))()
    for d, (s, t) in zip(pa, pairs):
        d.local_map_index = int(s)
        d.scan_index = -1 if t is None else int(t)
    out = (L.PoseGraphMarginal * max(len(pairs), 1))()
    info = L.PoseGraphMarginalsInfo()
    rc = fn(*head, _ptr(lp), lp.shape[0], _ptr(sp), sp.shape[0], ea, len(edges), lt, float(loss_scale), pa,
            len(pairs), out, C.byref(info))
    recs = [dict(local_cov=np.array(m.local_cov).reshape(3, 3), scan_cov=np.array(m.scan_cov).reshape(3, 3),
                 cross_cov=np.array(m.cross_cov).reshape(3, 3), relative_cov=np.array(m.relative_cov).reshape(3, 3),
                 finite=int(m.finite)) for m in out[:len(pairs)]] if rc == 0 else []
    return rc, recs, dict(n_columns=info.n_columns)


def host_pose_graph_marginals(local_poses, scan_poses, edges, pairs, loss="Huber", loss_scale=0.01):
    """csm_host_pose_graph_marginals: the sequential restatement of Context.pose_graph_marginals.
    pairs: (local map index, scan index or None / -1 for the local map node alone). Returns (one dict
    per pair: local_cov, scan_cov, cross_cov, relative_cov as [3, 3] arrays and finite; info dict)."""
    rc, recs, info = _pose_graph_marginals_run(L.load().csm_host_pose_graph_marginals, (), local_poses, scan_poses,
                                               edges, pairs, loss, loss_scale)
    if rc:
        raise CsmError(rc, "csm_host_pose_graph_marginals")
    return recs, info


def host_loop_search_ranges(relative_cov, n_sigma, min_range, max_range):
    """(range_x, range_y, range_theta) of a loop search from a pair's relative_cov
    (csm_host_loop_search_ranges): 2 n_sigma standard deviations, clamped."""
    cov, lo, hi, out = _f64(relative_cov).reshape(-1), _f64(min_range), _f64(max_range), np.zeros(3)
    if cov.size != 9 or lo.size != 3 or hi.size != 3:
        raise CsmError(L.CSM_EINVAL, "host_loop_search_ranges: relative_cov must be 3 x 3, the bounds 3")
    rc = L.load().csm_host_loop_search_ranges(_ptr(cov), float(n_sigma), _ptr(lo), _ptr(hi), _ptr(out))
    if rc:
        raise CsmError(rc, "csm_host_loop_search_ranges")
    return out


def host_loop_gate(relative_cov, match_cov, predicted, measured):
    """chi2 = d^T (relative_cov + match_cov)^-1 d of a found loop against the graph's prediction
    (csm_host_loop_gate)."""
    a, b, p, m = _f64(relative_cov).reshape(-1), _f64(match_cov).reshape(-1), _f64(predicted), _f64(measured)
    if a.size != 9 or b.size != 9 or p.size != 3 or m.size != 3:
        raise CsmError(L.CSM_EINVAL, "host_loop_gate: covariances must be 3 x 3, poses 3")
    chi2 = C.c_double()
    rc = L.load().csm_host_loop_gate(_ptr(a), _ptr(b), _ptr(p), _ptr(m), C.byref(chi2))
    if rc:
        raise CsmError(rc, "csm_host_loop_gate")
    return chi2.value


def host_information_from_covariance(cov):
    """The exactly symmetric inverse of a 3 x 3 covariance (csm_host_information_from_covariance): what
    host_prior_from_robot_information takes."""
    a, out = _f64(cov).reshape(-1), np.zeros((3, 3))
    if a.size != 9:
        raise CsmError(L.CSM_EINVAL, "host_information_from_covariance: cov must be 3 x 3")
    rc = L.load().csm_host_information_from_covariance(_ptr(a), _ptr(out))
    if rc:
        raise CsmError(rc, "csm_host_information_from_covariance")
    return out


def _loop_consistency_run(fn, head, local_poses, scan_poses, edges, gate, drift_var_per_metre, local_travel,
                          scan_travel, n_seeds, want_adjacency, want_chi2):
    lp = np.ascontiguousarray(local_poses, dtype=np.float64).reshape(-1, 3)
    sp = np.ascontiguousarray(scan_poses, dtype=np.float64).reshape(-1, 3)
    ea = pose_graph_edges(edges)
    m = len(edges)
    words = (max(m, 1) + 63) // 64
    dv = None if drift_var_per_metre is None else _f64(drift_var_per_metre).reshape(-1)
    lt = None if local_travel is None else _f64(local_travel).reshape(-1)
    st = None if scan_travel is None else _f64(scan_travel).reshape(-1)
    if (dv is not None and dv.size != 3) or (lt is not None and lt.size != lp.shape[0]) or \
            (st is not None and st.size != sp.shape[0]):
        raise CsmError(L.CSM_EINVAL, "loop_consistency: three drift variances, one travel value per node")
    selected = np.zeros(max(m, 1), np.int32)
    degree = np.zeros(max(m, 1), np.int32)
    info = L.LoopConsistencyInfo()
    adj = np.zeros((max(m, 1), words), np.uint64) if want_adjacency else None
    chi = np.zeros((max(m, 1), max(m, 1))) if want_chi2 else None
    opt = lambda a: None if a is None else _ptr(a)
    rc = fn(*head, _ptr(lp), lp.shape[0], _ptr(sp), sp.shape[0], ea, m, float(gate), opt(dv), opt(lt), opt(st),
            int(n_seeds), _ptr(selected), _ptr(degree), C.byref(info), opt(adj), opt(chi))
    out = dict(selected=selected[:m], degree=degree[:m],
               info=dict(consistent_pairs=int(info.consistent_pairs), bad_pivots=int(info.bad_pivots),
                         clique_size=int(info.clique_size), winning_seed=int(info.winning_seed),
                         seeds_run=int(info.seeds_run)))
    if want_adjacency:
        out["adjacency"] = adj[:m]
    if want_chi2:
        out["chi2"] = chi[:m, :m]
    return rc, out


def host_loop_consistency(local_poses, scan_poses, edges, gate, drift_var_per_metre=None, local_travel=None,
                          scan_travel=None, n_seeds=0, want_adjacency=False, want_chi2=False):
    """csm_host_loop_consistency: the sequential restatement of Context.loop_consistency, same arguments and
    result."""
    rc, out = _loop_consistency_run(L.load().csm_host_loop_consistency, (), local_poses, scan_poses, edges, gate,
                                    drift_var_per_metre, local_travel, scan_travel, n_seeds, want_adjacency,
                                    want_chi2)
    if rc:
        raise CsmError(rc, "csm_host_loop_consistency")
    return out


def loop_edges_from_matches(matches):
    """Edge dicts (pose_graph_edges) from detector output. matches: dicts with local (local map node index),
    scan (scan node index), pose (the estimated map-local scan pose = the measured InverseCompound(x_s, x_t))
    and covariance (3 x 3, the match's pose covariance). The information matrix is the covariance's exactly
    symmetric inverse (host_information_from_covariance); every edge is a loop edge."""
    return [dict(local=int(m["local"]), scan=int(m["scan"]), rel=[float(v) for v in m["pose"]],
                 info=host_information_from_covariance(m["covariance"]), loop=True) for m in matches]


# csm_loop_candidate as a numpy record: 24 bytes, the struct's layout
LOOP_CANDIDATE_DTYPE = np.dtype([("query_scan_index", np.int32), ("ref_scan_index", np.int32),
                                 ("ref_map_index", np.int32), ("reserved", np.int32), ("dist_sq", np.float64)])
assert LOOP_CANDIDATE_DTYPE.itemsize == C.sizeof(L.LoopCandidate)


def host_travel_distances(scan_poses):
    """csm_host_travel_distances: the accumulated travel distance at each scan node, summed in order with
    glibc's hypot as LoopSearcherNearest::Search accumulates it."""
    sp = np.ascontiguousarray(scan_poses, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(sp.shape[0])
    rc = L.load().csm_host_travel_distances(_ptr(sp), sp.shape[0], _ptr(out))
    if rc:
        raise CsmError(rc, "csm_host_travel_distances")
    return out


def _loop_search_run(fn, head, scan_poses, scan_map_index, travel, query_index, query_travel, n_ref, n_maps,
                     travel_dist_threshold, node_dist_threshold, n_per_query, one_per_map):
    sp = np.ascontiguousarray(scan_poses, dtype=np.float64).reshape(-1, 3)
    mi = np.ascontiguousarray(scan_map_index, dtype=np.int32).reshape(-1)
    tr = np.ascontiguousarray(travel, dtype=np.float64).reshape(-1)
    qi = np.ascontiguousarray(query_index, dtype=np.int32).reshape(-1)
    if mi.size != sp.shape[0] or tr.size != sp.shape[0]:
        raise CsmError(L.CSM_EINVAL, "loop_search: one map index and one travel value per scan node")
    if query_travel is None:
        if qi.size and (qi.min() < 0 or qi.max() >= tr.size):
            raise CsmError(L.CSM_EINVAL, "loop_search: a query index out of range")
        qt = np.ascontiguousarray(tr[qi])
    else:
        qt = np.ascontiguousarray(np.broadcast_to(np.asarray(query_travel, dtype=np.float64), qi.shape))
    n_ref = sp.shape[0] if n_ref is None else int(n_ref)
    n_maps = (int(mi.max()) + 1 if mi.size else 0) if n_maps is None else int(n_maps)
    k = int(n_per_query)
    p = L.LoopSearchParams(float(travel_dist_threshold), float(node_dist_threshold), k, int(one_per_map))
    slots = max(min(k, L.LOOP_SEARCH_MAX_K), 1)
    out = np.zeros((max(qi.size, 1), slots), LOOP_CANDIDATE_DTYPE)
    counts = np.zeros(max(qi.size, 1), np.int32)
    info = L.LoopSearchInfo()
    rc = fn(*head, _ptr(sp), _ptr(mi), _ptr(tr), sp.shape[0], n_maps, n_ref, _ptr(qi), _ptr(qt), qi.size, C.byref(p),
            _ptr(out), _ptr(counts), C.byref(info))
    return rc, out[:qi.size], counts[:qi.size], dict(pairs_evaluated=int(info.pairs_evaluated),
                                                     pairs_eligible=int(info.pairs_eligible))


def host_loop_search(scan_poses, scan_map_index, travel, query_index, query_travel=None, n_ref=None,
                     travel_dist_threshold=10.0, node_dist_threshold=2.0, n_per_query=2, one_per_map=False,
                     n_maps=None):
    """csm_host_loop_search: the sequential restatement of Context.loop_search, same arguments and result."""
    rc, out, counts, info = _loop_search_run(L.load().csm_host_loop_search, (), scan_poses, scan_map_index, travel,
                                             query_index, query_travel, n_ref, n_maps, travel_dist_threshold,
                                             node_dist_threshold, n_per_query, one_per_map)
    if rc:
        raise CsmError(rc, "csm_host_loop_search")
    return out, counts, info


def host_loop_candidates_nearest(records, counts, n_total):
    """csm_host_loop_candidates_nearest: the first n_total of all used records of a loop search, ordered by
    (dist_sq, ref_scan_index, query_scan_index). records: [n_q, n_per_query] of LOOP_CANDIDATE_DTYPE."""
    rec = np.ascontiguousarray(records, dtype=LOOP_CANDIDATE_DTYPE)
    cnt = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
    if rec.ndim != 2 or rec.shape[0] != cnt.size:
        raise CsmError(L.CSM_EINVAL, "host_loop_candidates_nearest: records must be [n_q, n_per_query], one count per row")
    out = np.zeros(max(int(n_total), 1), LOOP_CANDIDATE_DTYPE)
    n_out = C.c_int32(0)
    rc = L.load().csm_host_loop_candidates_nearest(_ptr(rec), _ptr(cnt), rec.shape[0], rec.shape[1], int(n_total),
                                                   _ptr(out), C.byref(n_out))
    if rc:
        raise CsmError(rc, "csm_host_loop_candidates_nearest")
    return out[:n_out.value]


# csm_appearance_candidate as a numpy record: 24 bytes, the struct's layout
APPEARANCE_CANDIDATE_DTYPE = np.dtype([("query_scan_index", np.int32), ("ref_scan_index", np.int32),
                                       ("ref_map_index", np.int32), ("shift", np.int32), ("distance", np.uint32),
                                       ("ring_distance", np.uint32)])
assert APPEARANCE_CANDIDATE_DTYPE.itemsize == C.sizeof(L.AppearanceCandidate)


def _scan_descriptors_run(fn, head, angles, ranges, offsets, n_rings, n_sectors, range_min, range_max):
    an = np.ascontiguousarray(angles, dtype=np.float64).reshape(-1)
    rg = np.ascontiguousarray(ranges, dtype=np.float64).reshape(-1)
    off = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1)
    if an.size != rg.size or off.size < 1 or (off.size > 1 and int(off.max()) > an.size):
        raise CsmError(L.CSM_EINVAL, "scan_descriptors: one range per angle, offsets within them")
    if an.size == 0:                    # never a pointer to nothing
        an, rg = np.zeros(1), np.zeros(1)
    p = L.DescriptorParams(int(n_rings), int(n_sectors), float(range_min), float(range_max))
    n = off.size - 1
    cells = max(min(int(n_rings), L.DESCRIPTOR_MAX_RINGS), 1) * max(min(int(n_sectors), L.DESCRIPTOR_MAX_SECTORS), 1)
    out = np.zeros((max(n, 1), cells), np.uint8)
    used = np.zeros(max(n, 1), np.int32)
    rc = fn(*head, _ptr(an), _ptr(rg), _ptr(off), n, C.byref(p), _ptr(out), _ptr(used))
    if rc:
        return rc, None, None
    return rc, out[:n].reshape(n, int(n_rings), int(n_sectors)), used[:n]


def ragged_scans(scans):
    """(angles, ranges) pairs -> the three arrays a descriptor build takes: angles, ranges, offsets."""
    sizes = [len(a) for a, _ in scans]
    cat = lambda i: (np.concatenate([np.asarray(s[i], np.float64).reshape(-1) for s in scans])
                     if scans else np.zeros(0))
    return cat(0), cat(1), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def host_scan_descriptors(angles, ranges, offsets, n_rings=20, n_sectors=64, range_min=0.5, range_max=20.0):
    """csm_host_scan_descriptors: the polar descriptors of ragged scans (scan i is beams offsets[i] ..
    offsets[i + 1]). Returns (descriptors [n_scans, n_rings, n_sectors] uint8, beams_used [n_scans])."""
    rc, out, used = _scan_descriptors_run(L.load().csm_host_scan_descriptors, (), angles, ranges, offsets, n_rings,
                                          n_sectors, range_min, range_max)
    if rc:
        raise CsmError(rc, "csm_host_scan_descriptors")
    return out, used


def host_descriptor_shift_angle(shift, n_sectors):
    """csm_host_descriptor_shift_angle: theta_query - theta_ref that a candidate's shift implies."""
    out = C.c_double()
    rc = L.load().csm_host_descriptor_shift_angle(int(shift), int(n_sectors), C.byref(out))
    if rc:
        raise CsmError(rc, "csm_host_descriptor_shift_angle")
    return out.value


def _appearance_run(fn, head, descriptors, scan_map_index, travel, query_index, query_travel, n_ref, n_maps,
                    travel_dist_threshold, max_distance, min_cell_sum, n_per_query, one_per_map, n_rings, n_sectors,
                    range_min, range_max):
    d = np.ascontiguousarray(descriptors, dtype=np.uint8)
    if d.ndim != 3:
        raise CsmError(L.CSM_EINVAL, "appearance_search: descriptors must be [n_scan, n_rings, n_sectors]")
    n_rings = d.shape[1] if n_rings is None else int(n_rings)
    n_sectors = d.shape[2] if n_sectors is None else int(n_sectors)
    mi = np.ascontiguousarray(scan_map_index, dtype=np.int32).reshape(-1)
    tr = np.ascontiguousarray(travel, dtype=np.float64).reshape(-1)
    qi = np.ascontiguousarray(query_index, dtype=np.int32).reshape(-1)
    if mi.size != d.shape[0] or tr.size != d.shape[0]:
        raise CsmError(L.CSM_EINVAL, "appearance_search: one map index and one travel value per scan node")
    if query_travel is None:
        if qi.size and (qi.min() < 0 or qi.max() >= tr.size):
            raise CsmError(L.CSM_EINVAL, "appearance_search: a query index out of range")
        qt = np.ascontiguousarray(tr[qi])
    else:
        qt = np.ascontiguousarray(np.broadcast_to(np.asarray(query_travel, dtype=np.float64), qi.shape))
    n_ref = d.shape[0] if n_ref is None else int(n_ref)
    n_maps = (int(mi.max()) + 1 if mi.size else 0) if n_maps is None else int(n_maps)
    k = int(n_per_query)
    p = L.AppearanceParams(L.DescriptorParams(n_rings, n_sectors, float(range_min), float(range_max)),
                           float(travel_dist_threshold), int(max_distance), int(min_cell_sum), k, int(one_per_map))
    slots = max(min(k, L.LOOP_SEARCH_MAX_K), 1)
    out = np.zeros((max(qi.size, 1), slots), APPEARANCE_CANDIDATE_DTYPE)
    counts = np.zeros(max(qi.size, 1), np.int32)
    info = L.LoopSearchInfo()
    rc = fn(*head, _ptr(d), _ptr(mi), _ptr(tr), d.shape[0], n_maps, n_ref, _ptr(qi), _ptr(qt), qi.size, C.byref(p),
            _ptr(out), _ptr(counts), C.byref(info))
    return rc, out[:qi.size], counts[:qi.size], dict(pairs_evaluated=int(info.pairs_evaluated),
                                                     pairs_eligible=int(info.pairs_eligible))


def host_appearance_search(descriptors, scan_map_index, travel, query_index, query_travel=None, n_ref=None,
                           travel_dist_threshold=10.0, max_distance=0xffffffff, min_cell_sum=0, n_per_query=2,
                           one_per_map=False, n_maps=None, n_rings=None, n_sectors=None, range_min=0.5,
                           range_max=20.0):
    """csm_host_appearance_search: the sequential restatement of Context.appearance_search, same arguments and
    result."""
    rc, out, counts, info = _appearance_run(L.load().csm_host_appearance_search, (), descriptors, scan_map_index,
                                            travel, query_index, query_travel, n_ref, n_maps, travel_dist_threshold,
                                            max_distance, min_cell_sum, n_per_query, one_per_map, n_rings, n_sectors,
                                            range_min, range_max)
    if rc:
        raise CsmError(rc, "csm_host_appearance_search")
    return out, counts, info


class Context:
    """One csm_ctx: owns the device grids, workspaces and a stream."""

    def __init__(self, device_id=0, tuning_off=0, map_uncertain_cap=0):
        """tuning_off: L.TUNE_* bits (switch launch optimisations off: A/B runs, tests)."""
        self.lib = L.load()
        self._ctx = C.c_void_p()
        cfg = L.Config()
        cfg.device_id = device_id
        cfg.tuning_off = tuning_off
        cfg.map_uncertain_cap = map_uncertain_cap
        rc = self.lib.csm_create(C.byref(cfg), C.byref(self._ctx))
        if rc:
            self._ctx = C.c_void_p()
            raise CsmError(rc, "csm_create failed (no GPU?)")
        self.shapes = {}

    def close(self):
        if self._ctx:
            self.lib.csm_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise CsmError(rc, self.lib.csm_last_error(self._ctx).decode())

    def set_stream(self, stream_ptr):
        self._check(self.lib.csm_set_stream(self._ctx, C.c_void_p(stream_ptr)))

    def synchronize(self):
        self._check(self.lib.csm_synchronize(self._ctx))

    def upload_grid(self, map_id, grid):
        g = np.ascontiguousarray(grid, dtype=np.uint16)
        self._check(self.lib.csm_upload_grid(self._ctx, map_id, _ptr(g), g.shape[0], g.shape[1]))
        self.shapes[map_id] = g.shape

    def upload_grid_blocks(self, map_id, blocks, block_rows, block_cols, log2_block):
        """Block-sparse upload (the reference's own storage): blocks[br * block_cols + bc] is a
        (2^k, 2^k) uint16 array or None for an unallocated block."""
        keep = [None if b is None else np.ascontiguousarray(b, dtype=np.uint16) for b in blocks]
        side = 1 << log2_block
        if any(b is not None and b.shape != (side, side) for b in keep):
            raise ValueError("upload_grid_blocks: every block must be (%d, %d)" % (side, side))
        ptrs = (C.c_void_p * len(keep))(*[None if b is None else b.ctypes.data for b in keep])
        self._check(self.lib.csm_upload_grid_blocks(self._ctx, map_id, ptrs, block_rows, block_cols, log2_block))
        self.shapes[map_id] = (block_rows << log2_block, block_cols << log2_block)

    def has_grid(self, map_id):
        return bool(self.lib.csm_has_grid(self._ctx, map_id))

    def debug_grid_known(self, map_id):
        """csm_debug_grid_known (test hook): (first row, first column) of the resident map holding a non-zero
        cell, (rows, cols) if it has none."""
        out = (C.c_int32 * 2)()
        rc = self.lib.csm_debug_grid_known(self._ctx, map_id, out)
        if rc != 0:
            raise CsmError(rc, "csm_debug_grid_known: map %d not resident" % map_id)
        return out[0], out[1]

    def release_grid(self, map_id):
        self._check(self.lib.csm_release_grid(self._ctx, map_id))
        self.shapes.pop(map_id, None)

    def build_pyramid(self, map_id, win_sizes):
        w = np.ascontiguousarray(win_sizes, dtype=np.int32)
        self._check(self.lib.csm_build_pyramid(
            self._ctx, map_id, w.ctypes.data_as(C.POINTER(C.c_int32)), w.size))

    def project_scan(self, geom, sensor_pose, step_theta, win_theta, angles, ranges, cap=1 << 20):
        """csm_project_scan: the device projection with its certificate. Returns
        (col [nt, n], row [nt, n], flat indices of the uncertified entries, their full count)."""
        a, r = _f64(angles), _f64(ranges)
        n, nt = a.size, 2 * win_theta + 1
        col = np.zeros((nt, n), np.int32)
        row = np.zeros((nt, n), np.int32)
        unc = np.zeros(cap, np.uint32)
        count = C.c_int32(0)
        g = L.Geometry(*geom)
        sp = _f64(sensor_pose)
        self._check(self.lib.csm_project_scan(self._ctx, C.byref(g), _ptr(sp), step_theta, win_theta,
                                              _ptr(a), _ptr(r), n, _ptr(col), _ptr(row), _ptr(unc), cap,
                                              C.byref(count)))
        return col, row, unc[:min(count.value, cap)].copy(), count.value

    def build_pyramids(self, map_ids, win_sizes):
        """csm_build_pyramids: box-max(win) of every listed map for every win, built where missing."""
        ids = np.ascontiguousarray(map_ids, dtype=np.uint64)
        w = np.ascontiguousarray(win_sizes, dtype=np.int32)
        self._check(self.lib.csm_build_pyramids(self._ctx, _ptr(ids), ids.size, _ptr(w), w.size))

    def build_likelihood_map(self, src, dst, sigma=None, resolution=None, radius=None, occupied_min=32768,
                             keep_unknown=False, kernel=None):
        """csm_build_likelihood_map: the likelihood field of the resident map `src` built on the device under
        `dst` (an ordinary map id from then on). Table as in likelihood_params()."""
        p, table = likelihood_params(sigma, resolution, radius, occupied_min, keep_unknown, kernel)
        self._check(self.lib.csm_build_likelihood_map(self._ctx, src, dst, C.byref(p)))
        self.shapes[dst] = self.shapes[src]

    def build_likelihood_maps(self, srcs, dsts, sigma=None, resolution=None, radius=None, occupied_min=32768,
                              keep_unknown=False, kernel=None):
        """csm_build_likelihood_maps: srcs[i] -> dsts[i], all in one launch."""
        s = np.ascontiguousarray(srcs, dtype=np.uint64)
        d = np.ascontiguousarray(dsts, dtype=np.uint64)
        if s.size != d.size:
            raise CsmError(L.CSM_EINVAL, "build_likelihood_maps: as many destinations as sources")
        p, table = likelihood_params(sigma, resolution, radius, occupied_min, keep_unknown, kernel)
        self._check(self.lib.csm_build_likelihood_maps(self._ctx, _ptr(s), _ptr(d), s.size, C.byref(p)))
        for a, b in zip(srcs, dsts):
            self.shapes[b] = self.shapes[a]

    def distance_transform(self, map_id, occupied_min=32768, want_d2=True, want_nearest=True):
        """csm_distance_transform: (d2, nearest) of the resident map, uint32 [rows, cols] each, computed on
        the device; an output that is not wanted is None."""
        if map_id in self.shapes or self.has_grid(map_id):
            rows, cols = self.shapes[map_id]        # resident but of unknown shape: KeyError, as download_level
        else:
            rows, cols = 1, 1                       # not resident: nothing is written, the call says CSM_ENOENT
        d2 = np.zeros((rows, cols), np.uint32) if want_d2 else None
        nearest = np.zeros((rows, cols), np.uint32) if want_nearest else None
        self._check(self.lib.csm_distance_transform(self._ctx, map_id, occupied_min,
                                                    _ptr(d2) if want_d2 else None,
                                                    _ptr(nearest) if want_nearest else None))
        return d2, nearest

    def build_distance_map(self, src, dst, sigma=None, resolution=None, radius=None, occupied_min=32768,
                           keep_unknown=False, table=None, peak=65534, floor_value=1):
        """csm_build_distance_map: the distance field of the resident map `src` built on the device under
        `dst` (an ordinary map id from then on). Table as in distance_params()."""
        p, t = distance_params(sigma, resolution, radius, occupied_min, keep_unknown, table, peak, floor_value)
        self._check(self.lib.csm_build_distance_map(self._ctx, src, dst, C.byref(p)))
        self.shapes[dst] = self.shapes[src]

    def build_distance_maps(self, srcs, dsts, sigma=None, resolution=None, radius=None, occupied_min=32768,
                            keep_unknown=False, table=None, peak=65534, floor_value=1):
        """csm_build_distance_maps: srcs[i] -> dsts[i], all on one launch chain."""
        s = np.ascontiguousarray(srcs, dtype=np.uint64)
        d = np.ascontiguousarray(dsts, dtype=np.uint64)
        if s.size != d.size:
            raise CsmError(L.CSM_EINVAL, "build_distance_maps: as many destinations as sources")
        p, t = distance_params(sigma, resolution, radius, occupied_min, keep_unknown, table, peak, floor_value)
        self._check(self.lib.csm_build_distance_maps(self._ctx, _ptr(s), _ptr(d), s.size, C.byref(p)))
        for a, b in zip(srcs, dsts):
            self.shapes[b] = self.shapes[a]

    def copy_last_batch_records(self, dst_ptr):
        """Device-to-device copy of the last batch's records (query order) into dst_ptr."""
        self._check(self.lib.csm_copy_last_batch_records(self._ctx, C.c_void_p(dst_ptr)))

    def download_level(self, map_id, level):
        out = np.zeros(self.shapes[map_id], np.uint16)
        self._check(self.lib.csm_download_level(self._ctx, map_id, level, _ptr(out)))
        return out

    @staticmethod
    def make_window(n_theta, n_points, win_x, win_y, low_resolution, coarse_level,
                    min_known, score_threshold, merge_mode=0):
        w = L.Window()
        w.merge_mode = merge_mode
        w.n_theta, w.n_points = n_theta, n_points
        w.win_x, w.win_y = win_x, win_y
        w.low_resolution, w.coarse_level = low_resolution, coarse_level
        w.min_known, w.score_threshold = min_known, score_threshold
        return w

    def score_window(self, map_id, window, hit_col, hit_row, dump=False):
        col, row = _hits(hit_col, hit_row)
        res = L.Result()
        if not dump:
            self._check(self.lib.csm_score_window(self._ctx, map_id, C.byref(window),
                                                  _ptr(col), _ptr(row), C.byref(res)))
            return result_to_dict(res)
        Lr = window.low_resolution
        nxc = -(-(2 * window.win_x + 1) // Lr)
        nyc = -(-(2 * window.win_y + 1) // Lr)
        s = np.zeros((window.n_theta, nxc * Lr, nyc * Lr), np.uint32)
        k = np.zeros((window.n_theta, nxc * Lr, nyc * Lr), np.uint16)
        ck = np.zeros((window.n_theta, nxc, nyc), np.uint16)
        self._check(self.lib.csm_score_window_dump(self._ctx, map_id, C.byref(window),
                                                   _ptr(col), _ptr(row), C.byref(res),
                                                   _ptr(s), _ptr(k), _ptr(ck)))
        return result_to_dict(res), s, k, ck

    def score_window_dev(self, map_id, window, col_ptr, row_ptr, out_ptr):
        self._check(self.lib.csm_score_window_dev(self._ctx, map_id, C.byref(window),
                                                  C.c_void_p(col_ptr), C.c_void_p(row_ptr),
                                                  C.c_void_p(out_ptr)))

    def prepare_windows(self, map_ids, windows, col_ptrs, row_ptrs):
        """The argument arrays of score_windows_dev(), built once for a batch
        that is scored repeatedly."""
        n = len(windows)
        ids = (C.c_uint64 * n)(*map_ids)
        wins = (L.Window * n)(*windows)
        cols = (C.c_void_p * n)(*col_ptrs)
        rows = (C.c_void_p * n)(*row_ptrs)
        return n, ids, wins, cols, rows

    def score_windows_dev(self, prepared, out_ptr):
        """csm_score_window_dev for many windows in one launch chain; `prepared`
        from prepare_windows(); out_ptr: device pointer to n 48-byte records."""
        n, ids, wins, cols, rows = prepared
        self._check(self.lib.csm_score_windows_dev(self._ctx, n, ids, wins, cols, rows,
                                                   C.c_void_p(out_ptr)))

    def score_windows_dump_dev(self, prepared, out_ptr, dump_s_ptrs=None, dump_k_ptrs=None, dump_f_ptrs=None):
        """score_windows_dev() that also writes, for the windows whose device pointers
        (0 = none) are given, every candidate's integer sums (S uint32, K uint16) and / or
        its fp32 key from the bound pass, [n_theta][nx][ny] each."""
        n, ids, wins, cols, rows = prepared

        def arr(ptrs):
            return (C.c_void_p * n)(*[p or None for p in ptrs]) if ptrs is not None else None
        self._check(self.lib.csm_score_windows_dump_dev(self._ctx, n, ids, wins, cols, rows, C.c_void_p(out_ptr),
                                                        arr(dump_s_ptrs), arr(dump_k_ptrs), arr(dump_f_ptrs)))

    def last_search_info(self):
        """What the last correlative_match() evaluated (nominal / coarse nodes / fine candidates,
        two_phase, graph_replayed: 1 when its launch chain was a replayed HIP graph)."""
        info = L.SearchInfo()
        self._check(self.lib.csm_last_search_info(self._ctx, C.byref(info)))
        return {k: getattr(info, k) for k, _ in info._fields_}

    def bound_pass_stats(self):
        """(candidate blocks the exact kernel scored, blocks it skipped after the fp32 bound
        pass) since the last call."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.csm_bound_pass_stats(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def correlative_match(self, map_id, geom, angles, ranges, rel_pose, init_pose,
                          range_x, range_y, range_theta, low_resolution,
                          score_threshold=0.0, known_rate_threshold=0.0):
        scan, keep = _scan_struct(angles, ranges, rel_pose)
        g = L.Geometry(*geom)
        p = _correlative_params(range_x, range_y, range_theta, low_resolution, score_threshold, known_rate_threshold)
        init = _f64(init_pose)
        out = L.Summary()
        self._check(self.lib.csm_correlative_match(self._ctx, map_id, C.byref(g), C.byref(scan),
                                                   _ptr(init), C.byref(p), C.byref(out)))
        return summary_to_dict(out)

    @staticmethod
    def peaks_params(k_max, excl=(0, 0, 0), scratch_limit_bytes=0):
        """csm_peaks_params: excl = exclusion radii (x, y, theta) in search steps."""
        return L.PeaksParams(k_max, excl[0], excl[1], excl[2], scratch_limit_bytes)

    def score_window_peaks(self, map_id, window, hit_col, hit_row, k_max, excl=(0, 0, 0), scratch_limit_bytes=0):
        """The K best distinct poses of one pre-projected window (csm_score_window_peaks): the list of
        the peaks' records, best first."""
        col, row = _hits(hit_col, hit_row)
        pk = self.peaks_params(k_max, excl, scratch_limit_bytes)
        out = (L.Result * max(1, min(k_max, L.PEAKS_MAX)))()
        n = C.c_int32(0)
        self._check(self.lib.csm_score_window_peaks(self._ctx, map_id, C.byref(window), _ptr(col), _ptr(row),
                                                    C.byref(pk), out, C.byref(n)))
        return [result_to_dict(out[j]) for j in range(n.value)]

    def correlative_peaks(self, map_id, geom, angles, ranges, rel_pose, init_pose, range_x, range_y, range_theta,
                          low_resolution, k_max, excl=(0, 0, 0), score_threshold=0.0, known_rate_threshold=0.0,
                          scratch_limit_bytes=0):
        """correlative_match() returning the K best distinct poses (csm_correlative_peaks): a list of
        summaries, best first."""
        scan, keep = _scan_struct(angles, ranges, rel_pose)
        g = L.Geometry(*geom)
        p = _correlative_params(range_x, range_y, range_theta, low_resolution, score_threshold, known_rate_threshold)
        init = _f64(init_pose)
        pk = self.peaks_params(k_max, excl, scratch_limit_bytes)
        out = (L.Summary * max(1, min(k_max, L.PEAKS_MAX)))()
        n = C.c_int32(0)
        self._check(self.lib.csm_correlative_peaks(self._ctx, map_id, C.byref(g), C.byref(scan), _ptr(init),
                                                   C.byref(p), C.byref(pk), out, C.byref(n)))
        return [summary_to_dict(out[j]) for j in range(n.value)]

    def correlative_peaks_batch(self, queries, range_x, range_y, range_theta, low_resolution, k_max,
                                excl=(0, 0, 0), score_threshold=0.0, known_rate_threshold=0.0,
                                scratch_limit_bytes=0, as_records=False):
        """correlative_match_batch() returning the K best distinct poses of every query
        (csm_correlative_peaks_batch): one list of summaries per query, best first. as_records: the C
        arrays (summaries [n * k_max], peak counts [n]) instead."""
        prep = self.prepare_queries(queries)
        p = _correlative_params(range_x, range_y, range_theta, low_resolution, score_threshold, known_rate_threshold)
        pk = self.peaks_params(k_max, excl, scratch_limit_bytes)
        kk = max(1, min(k_max, L.PEAKS_MAX))
        out = (L.Summary * (prep.n * kk))()
        n = (C.c_int32 * prep.n)()
        self._check(self.lib.csm_correlative_peaks_batch(self._ctx, prep.arr, prep.n, C.byref(p), C.byref(pk), out, n))
        if as_records:
            return out, n
        return [[summary_to_dict(out[i * kk + j]) for j in range(n[i])] for i in range(prep.n)]

    def score_window_moments(self, map_id, window, hit_col, hit_row, temperature, scratch_limit_bytes=0):
        """The winner and the integer moments of one pre-projected window's score volume
        (csm_score_window_moments), as a dict."""
        col, row = _hits(hit_col, hit_row)
        vp = L.VolumeParams(temperature, scratch_limit_bytes)
        out = L.VolumeMoments()
        self._check(self.lib.csm_score_window_moments(self._ctx, map_id, C.byref(window), _ptr(col), _ptr(row),
                                                      C.byref(vp), C.byref(out)))
        return moments_to_dict(out)

    def correlative_covariance(self, map_id, geom, angles, ranges, rel_pose, init_pose, range_x, range_y,
                               range_theta, low_resolution, temperature, score_threshold=0.0,
                               known_rate_threshold=0.0, scratch_limit_bytes=0):
        """correlative_match() with the pose covariance read off the score volume
        (csm_correlative_covariance): a dict of summary, moments, mean_offset, sensor_covariance,
        covariance."""
        scan, keep = _scan_struct(angles, ranges, rel_pose)
        g = L.Geometry(*geom)
        p = _correlative_params(range_x, range_y, range_theta, low_resolution, score_threshold, known_rate_threshold)
        init = _f64(init_pose)
        vp = L.VolumeParams(temperature, scratch_limit_bytes)
        out = L.VolumeSummary()
        self._check(self.lib.csm_correlative_covariance(self._ctx, map_id, C.byref(g), C.byref(scan), _ptr(init),
                                                        C.byref(p), C.byref(vp), C.byref(out)))
        return volume_summary_to_dict(out)

    def correlative_covariance_batch(self, queries, range_x, range_y, range_theta, low_resolution, temperature,
                                     score_threshold=0.0, known_rate_threshold=0.0, scratch_limit_bytes=0,
                                     as_records=False):
        """correlative_match_batch() with the volume covariance of every query
        (csm_correlative_covariance_batch): one dict per query. as_records: the C array instead."""
        prep = self.prepare_queries(queries)
        p = _correlative_params(range_x, range_y, range_theta, low_resolution, score_threshold, known_rate_threshold)
        vp = L.VolumeParams(temperature, scratch_limit_bytes)
        out = (L.VolumeSummary * prep.n)()
        self._check(self.lib.csm_correlative_covariance_batch(self._ctx, prep.arr, prep.n, C.byref(p), C.byref(vp),
                                                              out))
        if as_records:
            return out
        return [volume_summary_to_dict(out[i]) for i in range(prep.n)]

    def score_window_prior(self, map_id, window, hit_col, hit_row, information, steps, scratch_limit_bytes=0):
        """The winner of one pre-projected window under a motion prior, next to the unweighted one
        (csm_score_window_prior), as a dict."""
        col, row = _hits(hit_col, hit_row)
        pr = motion_prior(information, steps, scratch_limit_bytes)
        out = L.PriorResult()
        self._check(self.lib.csm_score_window_prior(self._ctx, map_id, C.byref(window), _ptr(col), _ptr(row),
                                                    C.byref(pr), C.byref(out)))
        return prior_result_to_dict(out)

    def correlative_match_prior(self, map_id, geom, angles, ranges, rel_pose, init_pose, range_x, range_y,
                                range_theta, low_resolution, information, score_threshold=0.0,
                                known_rate_threshold=0.0, scratch_limit_bytes=0):
        """correlative_match() under a motion prior on the offset from the initial pose
        (csm_correlative_match_prior): a dict of summary (from the winner under the prior) and prior."""
        scan, keep = _scan_struct(angles, ranges, rel_pose)
        g = L.Geometry(*geom)
        p = _correlative_params(range_x, range_y, range_theta, low_resolution, score_threshold, known_rate_threshold)
        init = _f64(init_pose)
        pr = motion_prior(information, scratch_limit_bytes=scratch_limit_bytes)
        out = L.PriorSummary()
        self._check(self.lib.csm_correlative_match_prior(self._ctx, map_id, C.byref(g), C.byref(scan), _ptr(init),
                                                         C.byref(p), C.byref(pr), C.byref(out)))
        return prior_summary_to_dict(out)

    def correlative_match_prior_batch(self, queries, range_x, range_y, range_theta, low_resolution, informations,
                                      score_threshold=0.0, known_rate_threshold=0.0, scratch_limit_bytes=0,
                                      as_records=False):
        """correlative_match_batch() under one motion prior per query (csm_correlative_match_prior_batch):
        one dict per query. informations: one 3 x 3 matrix per query. as_records: the C array instead."""
        prep = self.prepare_queries(queries)
        if len(informations) != prep.n:
            raise CsmError(L.CSM_EINVAL, "correlative_match_prior_batch: one information matrix per query")
        p = _correlative_params(range_x, range_y, range_theta, low_resolution, score_threshold, known_rate_threshold)
        priors = (L.MotionPrior * prep.n)(*[motion_prior(lam, scratch_limit_bytes=scratch_limit_bytes)
                                            for lam in informations])
        out = (L.PriorSummary * prep.n)()
        self._check(self.lib.csm_correlative_match_prior_batch(self._ctx, prep.arr, prep.n, C.byref(p), priors, out))
        if as_records:
            return out
        return [prior_summary_to_dict(out[i]) for i in range(prep.n)]

    def construct_map_from_scans(self, map_id, shape, map_pose, nodes, usable_range_min=0.01,
                                 usable_range_max=20.0, prob_hit=0.62, prob_miss=0.46,
                                 subpixel_scale=100):
        """GridMapBuilder::ConstructMapFromScans
        (src/my_lidar_graph_slam/mapping/grid_map_builder.cpp:561-695) on the
        device; the result becomes the resident grid `map_id`. shape = dict(res,
        off_x, off_y, rows, cols, log2_block) of the map before the call; nodes =
        dicts(pose, angles, ranges, rel_pose, min_range, max_range). Returns
        (new shape dict, info dict); defaults as launcher_settings_default.json:183-186."""
        return self._map_build(map_id, shape, map_pose, nodes, False, usable_range_min, usable_range_max,
                               prob_hit, prob_miss, subpixel_scale)

    def update_map_with_scan(self, map_id, shape, map_pose, node, usable_range_min=0.01,
                             usable_range_max=20.0, prob_hit=0.62, prob_miss=0.46, subpixel_scale=100):
        """The grid half of GridMapBuilder::UpdateGridMap
        (src/my_lidar_graph_slam/mapping/grid_map_builder.cpp:389-494): one scan
        node on top of the resident map `map_id`, which grows if it has to."""
        return self._map_build(map_id, shape, map_pose, [node], True, usable_range_min, usable_range_max,
                               prob_hit, prob_miss, subpixel_scale)

    def construct_maps_from_scans(self, jobs, usable_range_min=0.01, usable_range_max=20.0, prob_hit=0.62,
                                  prob_miss=0.46, subpixel_scale=100, scratch_limit_bytes=0):
        """csm_construct_maps_from_scans: construct_map_from_scans for many maps in one call (what
        GridMapBuilder::AfterLoopClosure announces and leaves undone). jobs = dicts(map_id, shape,
        map_pose, nodes) with the single call's meanings; the builder settings hold for all of them.
        Returns ([(new shape dict, info dict, status), ...], batch info dict). A job the single call
        would refuse gets its status (and its shape back unchanged) while the others complete; only a
        refusal of the whole call raises."""
        arr = (L.MapBuildJob * max(len(jobs), 1))()
        keep, shared = [], {}

        def as_f64(a):
            # the same array object is handed over at the same address: the library uploads it once
            if id(a) not in shared:
                shared[id(a)] = (a, _f64(a))
            return shared[id(a)][1]

        for j, job in enumerate(jobs):
            shape = job["shape"]
            arr[j].map_id = job["map_id"]
            arr[j].shape = L.MapShape(shape["res"], shape["off_x"], shape["off_y"], shape["rows"], shape["cols"],
                                      shape["log2_block"])
            arr[j].global_map_pose[:] = list(job["map_pose"])
            nodes = job["nodes"]
            nd_arr = _scan_nodes(nodes, as_f64, keep)
            arr[j].nodes = nd_arr if nodes else None
            arr[j].n_nodes = len(nodes)
        prm = L.MapBuilderParams(usable_range_min, usable_range_max, prob_hit, prob_miss, subpixel_scale)
        bp = L.MapBatchParams(int(scratch_limit_bytes))
        binfo = L.MapBatchInfo()
        rc = self.lib.csm_construct_maps_from_scans(self._ctx, arr, len(jobs), C.byref(prm), C.byref(bp),
                                                    C.byref(binfo))
        if rc and (rc != L.CSM_EINVAL or not jobs or all(arr[j].status == 0 for j in range(len(jobs)))):
            self._check(rc)                    # the whole call was refused, or failed on the device
        out = []
        for j, job in enumerate(jobs):
            sh, status = arr[j].shape, int(arr[j].status)
            if status == 0:
                self.shapes[job["map_id"]] = (sh.rows, sh.cols)
            elif not self.has_grid(job["map_id"]):
                self.shapes.pop(job["map_id"], None)
            out.append((dict(res=sh.resolution, off_x=sh.offset_x, off_y=sh.offset_y, rows=sh.rows, cols=sh.cols,
                             log2_block=sh.log2_block_size),
                        {name: getattr(arr[j].info, name) for name, _ in L.MapBuildInfo._fields_}, status))
        return out, {name: getattr(binfo, name) for name, _ in L.MapBatchInfo._fields_}

    def construct_global_map(self, map_id, shape, map_pose, nodes, usable_range_min=0.01, usable_range_max=20.0,
                             prob_hit=0.62, prob_miss=0.46, subpixel_scale=100, scratch_limit_bytes=0,
                             rank_direct_max=0, rank_tile=0):
        """csm_construct_global_map (GridMapBuilder::ConstructGlobalMap, grid_map_builder.cpp:162-184):
        construct_map_from_scans for one map of many scans, cast in parts of at most
        scratch_limit_bytes of scratch, long hit lists sorted (rank_direct_max, rank_tile; 0 = the
        defaults). Returns (new shape dict, info dict, global info dict)."""
        sh = L.MapShape(shape["res"], shape["off_x"], shape["off_y"], shape["rows"], shape["cols"],
                        shape["log2_block"])
        keep = []
        arr = _scan_nodes(nodes, _f64, keep)
        prm = L.MapBuilderParams(usable_range_min, usable_range_max, prob_hit, prob_miss, subpixel_scale)
        gp = L.GlobalMapParams(int(scratch_limit_bytes), int(rank_direct_max), int(rank_tile))
        info, ginfo = L.MapBuildInfo(), L.GlobalMapInfo()
        mp = _f64(map_pose)
        rc = self.lib.csm_construct_global_map(self._ctx, map_id, C.byref(sh), _ptr(mp), arr if nodes else None,
                                               len(nodes), C.byref(prm), C.byref(gp), C.byref(info),
                                               C.byref(ginfo))
        if rc and not self.has_grid(map_id):
            self.shapes.pop(map_id, None)       # a ray left the resized map: the map was dropped
        self._check(rc)
        self.shapes[map_id] = (sh.rows, sh.cols)
        new_shape = dict(res=sh.resolution, off_x=sh.offset_x, off_y=sh.offset_y, rows=sh.rows,
                         cols=sh.cols, log2_block=sh.log2_block_size)
        return (new_shape, {name: getattr(info, name) for name, _ in L.MapBuildInfo._fields_},
                {name: getattr(ginfo, name) for name, _ in L.GlobalMapInfo._fields_})

    def _map_build(self, map_id, shape, map_pose, nodes, keep_cells, usable_range_min, usable_range_max,
                   prob_hit, prob_miss, subpixel_scale):
        sh = L.MapShape(shape["res"], shape["off_x"], shape["off_y"], shape["rows"], shape["cols"],
                        shape["log2_block"])
        keep = []
        arr = _scan_nodes(nodes, _f64, keep)
        prm = L.MapBuilderParams(usable_range_min, usable_range_max, prob_hit, prob_miss, subpixel_scale)
        info = L.MapBuildInfo()
        mp = _f64(map_pose)
        if keep_cells:
            self._check(self.lib.csm_update_map_with_scan(self._ctx, map_id, C.byref(sh), _ptr(mp), arr,
                                                          C.byref(prm), C.byref(info)))
        else:
            self._check(self.lib.csm_construct_map_from_scans(self._ctx, map_id, C.byref(sh), _ptr(mp), arr,
                                                              len(nodes), C.byref(prm), C.byref(info)))
        self.shapes[map_id] = (sh.rows, sh.cols)
        new_shape = dict(res=sh.resolution, off_x=sh.offset_x, off_y=sh.offset_y, rows=sh.rows,
                         cols=sh.cols, log2_block=sh.log2_block_size)
        return new_shape, {name: getattr(info, name) for name, _ in L.MapBuildInfo._fields_}

    def grid_search_match(self, map_id, geom, angles, ranges, rel_pose, init_pose,
                          range_x, range_y, range_theta, step_x, step_y, step_theta,
                          score_threshold=0.0, known_rate_threshold=0.0):
        """ScanMatcherGridSearch::OptimizePose
        (src/my_lidar_graph_slam/mapping/scan_matcher_grid_search.cpp:69-190)."""
        scan, keep = _scan_struct(angles, ranges, rel_pose)
        g = L.Geometry(*geom)
        p = L.GridSearchParams(range_x, range_y, range_theta, step_x, step_y, step_theta,
                               score_threshold, known_rate_threshold)
        init = _f64(init_pose)
        out = L.Summary()
        self._check(self.lib.csm_grid_search_match(self._ctx, map_id, C.byref(g), C.byref(scan),
                                                   _ptr(init), C.byref(p), C.byref(out)))
        return summary_to_dict(out)

    def prepare_queries(self, queries):
        """Flatten a list of dict(map_id, geom, angles, ranges, rel_pose,
        init_pose) into the C array the batch entry points take. A caller that
        repeats a batch (or a C++ caller, which holds such an array anyway)
        passes the result instead of the list and skips the per-call marshalling."""
        if isinstance(queries, PreparedQueries):
            return queries
        n = len(queries)
        arr = (L.LoopQuery * n)()
        keep = []
        for i, q in enumerate(queries):
            a, r = _f64(q["angles"]), _f64(q["ranges"])
            keep.append((a, r))
            arr[i].map_id = q["map_id"]
            arr[i].geometry = L.Geometry(*q["geom"])
            arr[i].scan.angles = a.ctypes.data_as(C.POINTER(C.c_double))
            arr[i].scan.ranges = r.ctypes.data_as(C.POINTER(C.c_double))
            arr[i].scan.n_points = a.size
            arr[i].scan.relative_sensor_pose[:] = list(q["rel_pose"])
            arr[i].initial_pose[:] = list(q["init_pose"])
        return PreparedQueries(arr, keep)

    def correlative_match_batch(self, queries, range_x, range_y, range_theta, low_resolution,
                                score_threshold, known_rate_threshold, as_records=False):
        """queries: list of dict(map_id, geom, angles, ranges, rel_pose, init_pose)
        or prepare_queries()'s result. as_records: return the C summaries
        (SummaryArray) instead of dicts."""
        prep = self.prepare_queries(queries)
        p = _correlative_params(range_x, range_y, range_theta, low_resolution, score_threshold, known_rate_threshold)
        out = (L.Summary * prep.n)()
        self._check(self.lib.csm_correlative_match_batch(self._ctx, prep.arr, prep.n, C.byref(p), out))
        return SummaryArray(out) if as_records else [summary_to_dict(o) for o in out]

    def _pose_sets(self, sets):
        """A csm_pose_set array for dicts(map_id, geom, angles, ranges, poses); sets that pass the same angle
        and range arrays share their pointers, so the library stages the scan once."""
        arr = (L.PoseSet * max(len(sets), 1))()
        keep, counts = [], []
        for i, s in enumerate(sets):
            a, r, p = _f64(s["angles"]), _f64(s["ranges"]), _poses(s["poses"])
            keep += [a, r, p]
            arr[i].map_id = s["map_id"]
            arr[i].geometry = L.Geometry(*s["geom"])
            arr[i].scan.angles = a.ctypes.data_as(C.POINTER(C.c_double))
            arr[i].scan.ranges = r.ctypes.data_as(C.POINTER(C.c_double))
            arr[i].scan.n_points = a.size
            arr[i].poses = p.ctypes.data_as(C.POINTER(C.c_double))
            arr[i].n_poses = p.shape[0]
            counts.append(p.shape[0])
        return arr, keep, counts

    def score_pose_sets(self, sets):
        """csm_score_pose_sets: every set's scan at every map-local SENSOR pose of the set, all sets in one
        launch chain. sets: dicts(map_id, geom, angles, ranges, poses (n, 3)). Returns (a POSE_RECORD array
        per set, the call's info dict)."""
        arr, keep, counts = self._pose_sets(sets)
        out = np.zeros(max(sum(counts), 1), POSE_RECORD)
        info = L.PoseSetsInfo()
        self._check(self.lib.csm_score_pose_sets(self._ctx, arr, len(sets), _ptr(out), C.byref(info)))
        ends = np.cumsum([0] + counts)
        return [out[ends[i]:ends[i + 1]].copy() for i in range(len(sets))], pose_sets_info_to_dict(info)

    def pose_set_update(self, map_id, geom, angles, ranges, poses, temperature, known_rate_threshold=0.0,
                        n_out=None, offset=0):
        """csm_pose_set_update: scores the set and turns the scores into integer weights and a systematically
        resampled set of n_out ancestors (default: as many as poses). Returns a dict(records, weights,
        ancestors, update, info)."""
        arr, keep, counts = self._pose_sets([dict(map_id=map_id, geom=geom, angles=angles, ranges=ranges,
                                                  poses=poses)])
        n = counts[0]
        n_out = n if n_out is None else n_out
        prm = L.PoseUpdateParams(temperature, known_rate_threshold, n_out, 0, offset & 0xFFFFFFFFFFFFFFFF)
        rec = np.zeros(max(n, 1), POSE_RECORD)
        weights = np.zeros(max(n, 1), np.uint32)
        ancestors = np.zeros(max(n_out, 1), np.int32)
        upd, info = L.PoseUpdateInfo(), L.PoseSetsInfo()
        self._check(self.lib.csm_pose_set_update(self._ctx, arr, C.byref(prm), _ptr(rec), _ptr(weights),
                                                 _ptr(ancestors), C.byref(upd), C.byref(info)))
        return dict(records=rec[:n], weights=weights[:n], ancestors=ancestors[:max(n_out, 0)],
                    update=pose_update_to_dict(upd), info=pose_sets_info_to_dict(info))

    def score_pixel_accurate_many(self, map_id, geom, angles, ranges, poses, rel_pose=None):
        """ScorePixelAccurate::Score at many poses: a list of dict(normalized_score, score, known_rate,
        sum_values, known, flags). poses are map-local sensor poses, or robot poses when rel_pose (the scan's
        relative sensor pose) is given: csm_host_compound is then applied on the host."""
        p = _poses(poses)
        if rel_pose is not None:
            p = np.array([host_compound(q, rel_pose) for q in p]).reshape(-1, 3)
        recs, _ = self.score_pose_sets([dict(map_id=map_id, geom=geom, angles=angles, ranges=ranges, poses=p)])
        n = _f64(angles).size
        out = []
        for r in recs[0]:
            norm, rate = host_score_from_sums(r["sum_values"], r["known"], n)
            out.append(dict(normalized_score=norm, score=norm * n, known_rate=rate, sum_values=int(r["sum_values"]),
                            known=int(r["known"]), flags=int(r["flags"])))
        return out

    def score_pixel_accurate(self, map_id, geom, angles, ranges, pose, rel_pose=None):
        """ScorePixelAccurate::Score(gridMap, scan, mapLocalSensorPose) at one pose."""
        return self.score_pixel_accurate_many(map_id, geom, angles, ranges, [pose], rel_pose)[0]

    def measurement_update(self, map_id, geom, angles, ranges, poses, temperature, known_rate_threshold=0.0,
                           n_out=None, offset=0, rel_pose=None):
        """ParticleSetHIP::MeasurementUpdate: pose_set_update plus the effective sample size of the weights
        (f64, on the host). Robot poses when rel_pose is given."""
        p = _poses(poses)
        if rel_pose is not None:
            p = np.array([host_compound(q, rel_pose) for q in p]).reshape(-1, 3)
        out = self.pose_set_update(map_id, geom, angles, ranges, p, temperature, known_rate_threshold, n_out, offset)
        out["effective_sample_size"] = effective_sample_size(out["weights"])
        return out

    def ray_cast(self, sets, params=None, **kw):
        """csm_ray_cast: every set's beams cast from every map-local SENSOR pose of the set through its resident
        map. sets: dicts(map_id, geom, angles, poses (n, 3)[, ranges: a limit per beam]); sets that pass the
        same arrays share their pointers, so the library stages them once. Returns (a CAST_RECORD array
        (n_poses, n_points) per set, the call's info dict)."""
        arr = (L.PoseSet * max(len(sets), 1))()
        keep, shapes = [], []
        for i, s in enumerate(sets):
            sc, held = _cast_scan(s["angles"], s.get("ranges"))
            p = _poses(s["poses"])
            keep += [held, p]
            arr[i].map_id = s["map_id"]
            arr[i].geometry = L.Geometry(*s["geom"])
            arr[i].scan = sc
            if p.size:
                arr[i].poses = p.ctypes.data_as(C.POINTER(C.c_double))
            arr[i].n_poses = p.shape[0]
            shapes.append((p.shape[0], int(sc.n_points)))
        prm = params if params is not None else ray_cast_params(**kw)
        ends = np.cumsum([0] + [a * b for a, b in shapes])
        out = np.zeros(max(int(ends[-1]), 1), CAST_RECORD)
        info = L.RayCastInfo()
        self._check(self.lib.csm_ray_cast(self._ctx, arr, len(sets), C.byref(prm), _ptr(out), C.byref(info)))
        return ([out[ends[i]:ends[i + 1]].reshape(shapes[i]).copy() for i in range(len(sets))],
                ray_cast_info_to_dict(info))

    def virtual_scan(self, map_id, geom, pose, angles, ranges=None, params=None, **kw):
        """A scan of the resident map from the map-local sensor pose `pose`: (angles, ranges) of the beams that
        stopped, in beam order, ready for scan_descriptors, correlative_match (with a zero relative sensor
        pose) and ray_check_batch. The ranges are csm_host_ray_cast_ranges' (centre of the sensor's sub-pixel
        to the centre of the stopping cell)."""
        prm = params if params is not None else ray_cast_params(**kw)
        a = _f64(angles).reshape(-1)
        recs, _ = self.ray_cast([dict(map_id=map_id, geom=geom, angles=a, ranges=ranges, poses=[pose])], params=prm)
        rec = recs[0][0]
        hit = rec["kind"] != CAST_NONE
        rng = host_ray_cast_ranges(rec, geom[0], prm.subpixel_scale)
        return a[hit].copy(), rng[hit].copy()

    def ray_check_batch(self, queries, poses=None, per_beam=False, params=None, **kw):
        """csm_ray_check_batch: the free-space check of every query's scan against its resident map at the
        query's init_pose (a map-local robot pose, e.g. a summary's estimated_pose). poses: one pose per
        query that replaces its init_pose, so the output of correlative_peaks_batch can be fed in peak by
        peak. Returns a list of dicts; with per_beam also a list of int32 arrays, one per query."""
        prep = self.prepare_queries(queries)
        arr = prep.arr
        if poses is not None:
            if len(poses) != prep.n:
                raise ValueError("one pose per query")
            arr = (L.LoopQuery * prep.n)()
            C.memmove(arr, prep.arr, C.sizeof(arr))
            for i, pose in enumerate(poses):
                arr[i].initial_pose[:] = list(pose)
        p = params if params is not None else ray_check_params(**kw)
        out = (L.RayCheckResult * prep.n)()
        counts = [int(arr[i].scan.n_points) for i in range(prep.n)]
        words = np.zeros(max(sum(counts), 1), np.int32)
        self._check(self.lib.csm_ray_check_batch(self._ctx, arr, prep.n, C.byref(p), out,
                                                 _ptr(words) if per_beam else None))
        records = [ray_check_to_dict(o) for o in out]
        if not per_beam:
            return records
        ends = np.cumsum([0] + counts)
        return records, [words[ends[i]:ends[i + 1]].copy() for i in range(prep.n)]

    def bnb_match_batch(self, queries, range_x, range_y, range_theta, node_height_max,
                        score_threshold, known_rate_threshold, as_records=False):
        """As correlative_match_batch, for the branch-and-bound detector."""
        prep = self.prepare_queries(queries)
        p = L.BnbParams()
        p.range_x, p.range_y, p.range_theta = range_x, range_y, range_theta
        p.node_height_max = node_height_max
        p.score_threshold, p.known_rate_threshold = score_threshold, known_rate_threshold
        out = (L.Summary * prep.n)()
        self._check(self.lib.csm_bnb_match_batch(self._ctx, prep.arr, prep.n, C.byref(p), out))
        return SummaryArray(out) if as_records else [summary_to_dict(o) for o in out]

    def set_block_allocation(self, map_id, log2_block_size, allocated):
        """csm_set_block_allocation: uint8 [block rows, block cols] (None: derive from the cells)."""
        a = None if allocated is None else np.ascontiguousarray(allocated, dtype=np.uint8)
        self._check(self.lib.csm_set_block_allocation(self._ctx, map_id, log2_block_size,
                                                      None if a is None else _ptr(a)))

    @staticmethod
    def _refine_to_dict(r):
        return dict(normalized_initial_cost=r.normalized_initial_cost, normalized_cost=r.normalized_cost,
                    sensor_pose=list(r.sensor_pose), best_sensor_pose=list(r.best_sensor_pose),
                    estimated_pose=list(r.estimated_pose),
                    covariance=np.array(r.covariance).reshape(3, 3),
                    hessian=np.array(r.hessian).reshape(3, 3), lambda_=r.lambda_, iterations=r.iterations)

    def cost_covariance_batch(self, queries, sensor_poses, covariance_scale=1e4):
        """CostSquareError::Cost / n and ComputeCovariance at the given sensor poses."""
        prep = self.prepare_queries(queries)
        sp = _f64(sensor_poses).reshape(prep.n, 3)
        out = (L.RefineResult * prep.n)()
        self._check(self.lib.csm_cost_covariance_batch(self._ctx, prep.arr, prep.n, _ptr(sp),
                                                       covariance_scale, out))
        return [self._refine_to_dict(o) for o in out]

    def linear_solver_batch(self, queries, iterations_max=10, convergence_threshold=1e-4, lambda_=1e-4,
                            covariance_scale=1e4):
        """ScanMatcherLinearSolver::OptimizePose per query (init_pose = robot pose to refine);
        defaults as launcher_settings_default.json:28-35, 11-13."""
        prep = self.prepare_queries(queries)
        p = L.RefineParams(covariance_scale, iterations_max, 0, convergence_threshold, lambda_)
        out = (L.RefineResult * prep.n)()
        self._check(self.lib.csm_linear_solver_batch(self._ctx, prep.arr, prep.n, C.byref(p), out))
        return [self._refine_to_dict(o) for o in out]

    @staticmethod
    def _hill_to_dict(r):
        return dict(normalized_initial_cost=r.normalized_initial_cost, normalized_cost=r.normalized_cost,
                    sensor_pose=list(r.sensor_pose), best_sensor_pose=list(r.best_sensor_pose),
                    estimated_pose=list(r.estimated_pose), covariance=np.array(r.covariance).reshape(3, 3),
                    diff_translation=r.diff_translation, diff_rotation=r.diff_rotation,
                    iterations=r.iterations, refinements=r.refinements, replays=r.replays,
                    host_path=r.host_path, cost_evaluations=int(r.cost_evaluations))

    def greedy_cost_covariance_batch(self, queries, sensor_poses, greedy=None, as_records=False):
        """CostGreedyEndpoint::Cost / n and ComputeCovariance at the given sensor poses.
        greedy: greedy_params(...) or a dict of its keyword arguments (default settings if None)."""
        prep = self.prepare_queries(queries)
        sp = _f64(sensor_poses).reshape(prep.n, 3)
        p = greedy_params(**(greedy or {})) if not isinstance(greedy, L.GreedyParams) else greedy
        out = (L.HillClimbingResult * prep.n)()
        self._check(self.lib.csm_greedy_cost_covariance_batch(self._ctx, prep.arr, prep.n, _ptr(sp),
                                                              C.byref(p), out))
        return out if as_records else [self._hill_to_dict(o) for o in out]

    def hill_climbing_batch(self, queries, linear_step=0.1, angular_step=0.1, max_iterations=100,
                            max_refinements=5, greedy=None, as_records=False):
        """ScanMatcherHillClimbing::OptimizePose per query (init_pose = map-local robot pose);
        defaults as launcher_settings_default.json "ScanMatcherHillClimbing" / "CostGreedyEndpoint"."""
        prep = self.prepare_queries(queries)
        p = hill_climbing_params(linear_step, angular_step, max_iterations, max_refinements, greedy)
        out = (L.HillClimbingResult * prep.n)()
        self._check(self.lib.csm_hill_climbing_batch(self._ctx, prep.arr, prep.n, C.byref(p), out))
        return out if as_records else [self._hill_to_dict(o) for o in out]

    def pose_graph_lm(self, local_poses, scan_poses, edges, lambda_, params=None, **kw):
        """PoseGraphOptimizerLM::Optimize on the device (csm_pose_graph_lm). Returns new arrays
        (local poses [n, 3], scan poses [m, 3]) and a dict: steps, cg_iterations, initial_error,
        final_error, lambda_ (the final damping factor) and trace (one dict per LM step)."""
        p = params if params is not None else pose_graph_params(**kw)
        rc, lp, sp, out = _pose_graph_run(self.lib.csm_pose_graph_lm, (self._ctx,), local_poses, scan_poses,
                                          edges, lambda_, p)
        self._check(rc)
        return lp, sp, out

    def pose_graph_marginals(self, local_poses, scan_poses, edges, pairs, loss="Huber", loss_scale=0.01):
        """Marginal covariances of (local map node, scan node) pairs on the device
        (csm_pose_graph_marginals); arguments and result as host_pose_graph_marginals."""
        rc, recs, info = _pose_graph_marginals_run(self.lib.csm_pose_graph_marginals, (self._ctx,), local_poses,
                                                   scan_poses, edges, pairs, loss, loss_scale)
        self._check(rc)
        return recs, info

    def loop_search(self, scan_poses, scan_map_index, travel, query_index, query_travel=None, n_ref=None,
                    travel_dist_threshold=10.0, node_dist_threshold=2.0, n_per_query=2, one_per_map=False,
                    n_maps=None):
        """csm_loop_search: the loop candidates of the query nodes on the device. scan_poses [n, 3];
        scan_map_index [n] non-decreasing; travel [n] non-decreasing (host_travel_distances); query_index:
        distinct scan node indices; query_travel: one value or one per query (None: each query's own travel);
        n_ref (None: n): nodes [0, n_ref) may be reference nodes; n_maps (None: the greatest map index + 1).
        Returns (records [n_q, n_per_query] of LOOP_CANDIDATE_DTYPE, unused slots with ref_scan_index -1;
        counts [n_q]; info dict: pairs_evaluated, pairs_eligible)."""
        rc, out, counts, info = _loop_search_run(self.lib.csm_loop_search, (self._ctx,), scan_poses, scan_map_index,
                                                 travel, query_index, query_travel, n_ref, n_maps,
                                                 travel_dist_threshold, node_dist_threshold, n_per_query, one_per_map)
        self._check(rc)
        return out, counts, info

    def loop_consistency(self, local_poses, scan_poses, edges, gate, drift_var_per_metre=None, local_travel=None,
                         scan_travel=None, n_seeds=0, want_adjacency=False, want_chi2=False):
        """csm_loop_consistency: which loop edges agree with each other, on the device. local_poses [n, 3],
        scan_poses [m, 3]: the current estimates; edges: as pose_graph_lm takes them (is_loop is not read); gate:
        the chi-square bound of a pair's cycle; the drift model (all three or none): drift_var_per_metre (3),
        local_travel [n], scan_travel [m]; n_seeds: greedy searches from the vertices of highest degree (0: all).
        Returns a dict: selected int32 [M] (the largest consistent set found), degree int32 [M], info
        (consistent_pairs, bad_pivots, clique_size, winning_seed, seeds_run), and on request adjacency uint64
        [M, ceil(M / 64)] and chi2 float64 [M, M] (M <= LOOP_CONSISTENCY_MAX_CHI2_EDGES). Every byte equals
        host_loop_consistency's."""
        rc, out = _loop_consistency_run(self.lib.csm_loop_consistency, (self._ctx,), local_poses, scan_poses, edges,
                                        gate, drift_var_per_metre, local_travel, scan_travel, n_seeds,
                                        want_adjacency, want_chi2)
        self._check(rc)
        return out

    def scan_descriptors(self, angles, ranges, offsets, n_rings=20, n_sectors=64, range_min=0.5, range_max=20.0):
        """csm_scan_descriptors: the polar descriptors of ragged scans on the device; arguments and result as
        host_scan_descriptors, byte for byte."""
        rc, out, used = _scan_descriptors_run(self.lib.csm_scan_descriptors, (self._ctx,), angles, ranges, offsets,
                                              n_rings, n_sectors, range_min, range_max)
        self._check(rc)
        return out, used

    def appearance_search(self, descriptors, scan_map_index, travel, query_index, query_travel=None, n_ref=None,
                          travel_dist_threshold=10.0, max_distance=0xffffffff, min_cell_sum=0, n_per_query=2,
                          one_per_map=False, n_maps=None, n_rings=None, n_sectors=None, range_min=0.5,
                          range_max=20.0):
        """csm_appearance_search: loop candidates by what the scans look like. descriptors [n, n_rings,
        n_sectors] uint8 (scan_descriptors); scan_map_index, travel, query_index, query_travel, n_ref and n_maps
        as loop_search takes them. A pair is a candidate when the least L1 distance over all sector shifts is at
        most max_distance and both descriptors sum to min_cell_sum or more. Returns (records [n_q, n_per_query]
        of APPEARANCE_CANDIDATE_DTYPE ordered by (distance, reference node), unused slots with ref_scan_index
        -1; counts [n_q]; info dict: pairs_evaluated, pairs_eligible)."""
        rc, out, counts, info = _appearance_run(self.lib.csm_appearance_search, (self._ctx,), descriptors,
                                                scan_map_index, travel, query_index, query_travel, n_ref, n_maps,
                                                travel_dist_threshold, max_distance, min_cell_sum, n_per_query,
                                                one_per_map, n_rings, n_sectors, range_min, range_max)
        self._check(rc)
        return out, counts, info

    def enable_kernel_timing(self, on=True):
        self._check(self.lib.csm_enable_kernel_timing(self._ctx, 1 if on else 0))

    def reset_kernel_timing(self):
        self._check(self.lib.csm_reset_kernel_timing(self._ctx))

    def kernel_time(self, name):
        ms, n = C.c_double(), C.c_int64()
        self._check(self.lib.csm_kernel_time(self._ctx, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value


def host_shard_bounds(n_queries, member, n_members):
    lo, hi = C.c_int32(), C.c_int32()
    L.load().csm_shard_bounds(n_queries, member, n_members, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


class Group:
    """csm_group: one context per listed device inside this process; batches are cut
    into contiguous blocks, one host thread per member, one all-gather of the
    records (RCCL when the devices differ)."""

    def __init__(self, device_ids, force_rccl=False, tuning_off=0):
        self.lib = L.load()
        self._g = C.c_void_p()
        ids = np.ascontiguousarray(device_ids, dtype=np.int32)
        cfg = L.Config()
        cfg.tuning_off = tuning_off
        rc = self.lib.csm_group_create_ex(_ptr(ids), ids.size, C.byref(cfg),
                                          L.GROUP_FORCE_RCCL if force_rccl else 0, C.byref(self._g))
        if rc:
            self._g = C.c_void_p()
            raise CsmError(rc, "csm_group_create failed")
        self.members = []
        for k in range(self.lib.csm_group_size(self._g)):
            ctx = Context.__new__(Context)          # a view of the member: the group owns it
            ctx.lib, ctx.shapes = self.lib, {}
            ctx._ctx = C.c_void_p(self.lib.csm_group_member(self._g, k))
            ctx.close = lambda: None
            self.members.append(ctx)

    def close(self):
        if self._g:
            for m in self.members:
                m._ctx = C.c_void_p()
            self.lib.csm_group_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise CsmError(rc, self.lib.csm_group_last_error(self._g).decode())

    def upload_grids(self, queries, grids):
        """Every query's map to the member whose block holds the query."""
        n, m = len(queries), len(self.members)
        for k, ctx in enumerate(self.members):
            lo, hi = host_shard_bounds(n, k, m)
            for q in queries[lo:hi]:
                if not ctx.has_grid(q["map_id"]):
                    ctx.upload_grid(q["map_id"], grids[q["map_id"]])

    def bnb_match_batch(self, queries, range_x, range_y, range_theta, node_height_max,
                        score_threshold, known_rate_threshold, as_records=False):
        prep = self.members[0].prepare_queries(queries)
        p = L.BnbParams()
        p.range_x, p.range_y, p.range_theta = range_x, range_y, range_theta
        p.node_height_max = node_height_max
        p.score_threshold, p.known_rate_threshold = score_threshold, known_rate_threshold
        out = (L.Summary * prep.n)()
        self._check(self.lib.csm_group_bnb_match_batch(self._g, prep.arr, prep.n, C.byref(p), out))
        return SummaryArray(out) if as_records else [summary_to_dict(o) for o in out]

    def gathered_records(self, member):
        """Member `member`'s device buffer after the exchange, read back: uint8 [n_members, block, 48]."""
        dev, block = C.c_void_p(), C.c_int32()
        self._check(self.lib.csm_group_gathered_records_dev(self._g, member, C.byref(dev), C.byref(block)))
        m = len(self.members)
        n_bytes = m * block.value * C.sizeof(L.Result)
        out = np.zeros(n_bytes, np.uint8)
        self.members[member].synchronize()
        # a plain device-to-host copy of a raw pointer
        import ctypes
        hip = ctypes.CDLL("libamdhip64.so")
        rc = hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), dev, ctypes.c_size_t(n_bytes), 2)
        if rc:
            raise CsmError(rc, "hipMemcpy failed")
        return out.reshape(m, block.value, C.sizeof(L.Result))

    def exchange_info(self):
        used, us = C.c_int32(), C.c_double()
        self._check(self.lib.csm_group_exchange_info(self._g, C.byref(used), C.byref(us)))
        return bool(used.value), us.value


@contextlib.contextmanager
def _query_map(ctx, nonce, map_id, grid, likelihood_sigma=None, resolution=None, distance_sigma=None,
               distance_radius=None):
    """The residency rule of the three matchers below, for one optimize_pose call: the map lies under
    map_id, or under the matcher's nonce id when it is a throw-away map (map_id None, like
    LocalMapId::Invalid in scan_matcher_correlative_fpga.cpp:177-184); grid is uploaded when the map is
    throw-away or not resident (grid None: it is resident already, the per-LocalMapId cache of the loop
    detectors). With a likelihood_sigma the map's field lies under its id | LIKELIHOOD_ID_BIT: the field
    follows the map, built when the map was uploaded just now or has no field yet. With a distance_sigma
    it is the distance field instead (Context.build_distance_map), under ScanMatcherCorrelativeHIP.field_id.
    Yields (map id, id to search on); a throw-away map and its field are released when the call ends."""
    mid = nonce if map_id is None else map_id
    uploaded = grid is not None and (map_id is None or not ctx.has_grid(mid))
    if uploaded:
        ctx.upload_grid(mid, grid)
    search_id = mid
    if likelihood_sigma is not None:
        search_id = mid | ScanMatcherCorrelativeHIP.LIKELIHOOD_ID_BIT
        if uploaded or not ctx.has_grid(search_id):
            ctx.build_likelihood_map(mid, search_id, likelihood_sigma, resolution)
    elif distance_sigma is not None:
        search_id = ScanMatcherCorrelativeHIP.field_id(mid, ScanMatcherCorrelativeHIP.DISTANCE_ID_BIT)
        if uploaded or not ctx.has_grid(search_id):
            ctx.build_distance_map(mid, search_id, distance_sigma, resolution, distance_radius)
    yield mid, search_id
    if map_id is None:
        ctx.release_grid(mid)
        if search_id != mid:
            ctx.release_grid(search_id)


class ScanMatcherCorrelativeHIP:
    """Drop-in for ScanMatcherCorrelative (constructor arguments as in
    src/my_lidar_graph_slam/scan_matcher_factory.cpp:173-177)."""

    # the likelihood field of map id m lives under m | LIKELIHOOD_ID_BIT (callers' ids are below 2^62, the
    # adapters' own throw-away ids start there: bit 63 is free in both)
    LIKELIHOOD_ID_BIT = 1 << 63
    # ... and its distance field under m | DISTANCE_ID_BIT, for a caller's id m (below 2^62)
    DISTANCE_ID_BIT = 1 << 62

    @classmethod
    def field_id(cls, map_id, bit):
        """Where the field of map_id lies. A caller's id: map_id | bit. The adapters' own throw-away ids
        carry bit 62 already, so a throw-away map's field, of either kind, lies under bit 63: a matcher
        has one kind of field, and the field goes with the map when the call ends."""
        return map_id | (cls.LIKELIHOOD_ID_BIT if map_id & bit else bit)

    def __init__(self, name, low_resolution, range_x, range_y, range_theta, ctx=None, prior_information=None,
                 likelihood_sigma=None, covariance_scale=1e4, distance_sigma=None, distance_radius=None):
        """prior_information: a 3 x 3 information matrix of the sensor pose's offset from the initial pose
        (beyond the reference); optimize_pose then goes through csm_correlative_match_prior.
        likelihood_sigma: the sensor noise in metres (beyond the reference); optimize_pose then searches on
        the map's likelihood field (Context.build_likelihood_map at the default radius, occupied_min and
        keep_unknown, under map id | LIKELIHOOD_ID_BIT) and adds, from the ORIGINAL occupancy map -- cost,
        covariance and refinement are bilinear in occupancy and must not see the spread values --
        out["cost"] (cost_covariance_batch at the best sensor pose) and out["refined"] (linear_solver_batch
        from the estimated pose), both with covariance_scale.
        distance_sigma (metres), distance_radius (cells; default ceil(3 sigma / resolution), at most
        DISTANCE_MAX_RADIUS): the same on the map's distance field (Context.build_distance_map at the default
        peak, floor, occupied_min and keep_unknown, under field_id(map id, DISTANCE_ID_BIT)), whose radius is
        not limited to 16 cells. Giving both sigmas is CSM_EINVAL."""
        if likelihood_sigma is not None and distance_sigma is not None:
            raise CsmError(L.CSM_EINVAL, "ScanMatcherCorrelativeHIP: likelihood_sigma or distance_sigma, not both")
        self.distance_sigma, self.distance_radius = distance_sigma, distance_radius
        self.name = name
        self.low_resolution = low_resolution
        self.range_x, self.range_y, self.range_theta = range_x, range_y, range_theta
        self.ctx = ctx or Context()
        self.prior_information = prior_information
        self.likelihood_sigma = likelihood_sigma
        self.covariance_scale = covariance_scale
        self._nonce = 1 << 62

    def optimize_pose(self, grid, geom, angles, ranges, rel_pose, init_pose,
                      map_id=None, score_threshold=0.0, known_rate_threshold=0.0):
        """grid may be None when map_id is already resident (the per-LocalMapId
        cache of the loop detectors); a throw-away latest map gets a nonce id,
        like LocalMapId::Invalid in scan_matcher_correlative_fpga.cpp:177-184."""
        with _query_map(self.ctx, self._nonce, map_id, grid, self.likelihood_sigma, geom[0], self.distance_sigma,
                        self.distance_radius) as (mid, search_id):
            if self.prior_information is not None:
                # the summary of the winner under the prior, with the unweighted winner and the penalty beside it
                both = self.ctx.correlative_match_prior(search_id, geom, angles, ranges, rel_pose, init_pose,
                                                        self.range_x, self.range_y, self.range_theta,
                                                        self.low_resolution, self.prior_information,
                                                        score_threshold, known_rate_threshold)
                out = dict(both["summary"], unweighted=both["prior"]["unweighted"], prior=both["prior"])
            else:
                out = self.ctx.correlative_match(search_id, geom, angles, ranges, rel_pose, init_pose,
                                                 self.range_x, self.range_y, self.range_theta,
                                                 self.low_resolution, score_threshold,
                                                 known_rate_threshold)
            if search_id != mid:
                q = dict(map_id=mid, geom=geom, angles=angles, ranges=ranges, rel_pose=rel_pose,
                         init_pose=out["estimated_pose"])
                out["cost"] = self.ctx.cost_covariance_batch([q], [out["best_sensor_pose"]], self.covariance_scale)[0]
                out["refined"] = self.ctx.linear_solver_batch([q], covariance_scale=self.covariance_scale)[0]
        return out


class ScanMatcherGridSearchHIP:
    """Drop-in for ScanMatcherGridSearch (constructor arguments as in
    src/my_lidar_graph_slam/scan_matcher_factory.cpp, "GridSearch" branch:
    ranges then steps)."""

    def __init__(self, name, range_x, range_y, range_theta, step_x, step_y, step_theta, ctx=None):
        if not (step_x > 0 and step_y > 0 and step_theta > 0):
            raise ValueError("steps must be positive")
        self.name = name
        self.ranges = (range_x, range_y, range_theta)
        self.steps = (step_x, step_y, step_theta)
        self.ctx = ctx or Context()
        self._nonce = (1 << 62) + 1

    def optimize_pose(self, grid, geom, angles, ranges, rel_pose, init_pose,
                      map_id=None, score_threshold=0.0, known_rate_threshold=0.0):
        with _query_map(self.ctx, self._nonce, map_id, grid) as (mid, _):
            return self.ctx.grid_search_match(mid, geom, angles, ranges, rel_pose, init_pose,
                                              *self.ranges, *self.steps, score_threshold,
                                              known_rate_threshold)


class ScanMatcherHillClimbingHIP:
    """Drop-in for ScanMatcherHillClimbing with the GreedyEndpoint cost (constructor
    arguments as in src/my_lidar_graph_slam/scan_matcher_factory.cpp:103-130; `greedy`
    holds the CostConfigGroup's keys as greedy_params() keyword arguments)."""

    def __init__(self, name, linear_step, angular_step, max_iterations, max_refinements, greedy=None, ctx=None):
        self.name = name
        self.params = hill_climbing_params(linear_step, angular_step, max_iterations, max_refinements, greedy)
        self.ctx = ctx or Context()
        self._nonce = (1 << 62) + 2

    def optimize_pose(self, grid, geom, angles, ranges, rel_pose, init_pose, map_id=None):
        """ScanMatchingSummary fields plus the matcher's metrics; grid may be None when
        map_id is resident; a throw-away latest map gets a nonce id."""
        p = self.params
        with _query_map(self.ctx, self._nonce, map_id, grid) as (mid, _):
            q = dict(map_id=mid, geom=geom, angles=angles, ranges=ranges, rel_pose=rel_pose, init_pose=init_pose)
            out = self.ctx.hill_climbing_batch([q], p.linear_step, p.angular_step, p.max_iterations,
                                               p.max_refinements, p.cost)[0]
        out["pose_found"] = 1          # OptimizePose always finds a pose
        return out


class PoseGraphOptimizerLMHIP:
    """Drop-in for PoseGraphOptimizerLM with the ConjugateGradient solver, or with the direct
    "SchurCholesky" solver in place of SparseCholesky, which is not provided (constructor arguments as
    the optimizer's settings group, launcher_settings_default.json "PoseGraphOptimizerLM"). The damping
    factor is kept between optimize() calls, as the reference's mLambda member is."""

    def __init__(self, solver="ConjugateGradient", iterations_max=10, error_tolerance=1e-4, initial_lambda=1e-4,
                 loss="Huber", loss_scale=0.01, ctx=None):
        self.params = pose_graph_params(iterations_max, error_tolerance, solver, loss, loss_scale)
        if self.params.solver_type not in (L.PG_SOLVER_CONJUGATE_GRADIENT, L.PG_SOLVER_SCHUR_CHOLESKY):
            raise CsmError(L.CSM_EINVAL, "PoseGraphOptimizerLMHIP: only the ConjugateGradient and SchurCholesky "
                                         "solvers are provided")
        self.lambda_ = float(initial_lambda)
        self.ctx = ctx or Context()
        self.last_info = None

    def optimize(self, local_map_nodes, scan_nodes, edges):
        """Optimize(localMapNodes, scanNodes, poseGraphEdges): returns the updated (local, scan)
        pose arrays; the metrics of the call are in last_info."""
        lp, sp, info = self.ctx.pose_graph_lm(local_map_nodes, scan_nodes, edges, self.lambda_, self.params)
        self.lambda_ = info["lambda_"]
        self.last_info = info
        return lp, sp

    def marginals(self, local_map_nodes, scan_nodes, edges, pairs):
        """Marginal covariances of the pairs at the given poses, with the optimizer's loss function
        (Context.pose_graph_marginals): one dict per pair."""
        return self.ctx.pose_graph_marginals(local_map_nodes, scan_nodes, edges, pairs, self.params.loss_type,
                                             self.params.loss_scale)[0]


def loop_search_graph(scan_poses, local_maps, last_finished_map):
    """What LoopSearchHint holds, as the arrays a loop search takes. local_maps: (scan_node_min,
    scan_node_max) of each local map, inclusive, contiguous runs from node 0. Returns (poses of the nodes up
    to the last finished map's last, map index of each, their travel distances, n_ref = the first node of
    the last finished map, query_index = its nodes)."""
    runs = [(int(a), int(b)) for a, b in local_maps][:int(last_finished_map) + 1]
    if not runs or int(last_finished_map) < 0 or int(last_finished_map) >= len(local_maps):
        raise CsmError(L.CSM_EINVAL, "loop search: last_finished_map names no local map")
    if runs[0][0] != 0 or any(b < a for a, b in runs) or any(runs[i + 1][0] != runs[i][1] + 1
                                                              for i in range(len(runs) - 1)):
        raise CsmError(L.CSM_EINVAL, "loop search: local maps must be contiguous runs of scan nodes from node 0")
    sp = np.ascontiguousarray(scan_poses, dtype=np.float64).reshape(-1, 3)
    n = runs[-1][1] + 1
    if n > sp.shape[0]:
        raise CsmError(L.CSM_EINVAL, "loop search: a local map names a scan node that is not given")
    sp = sp[:n]
    map_index = np.repeat(np.arange(len(runs), dtype=np.int32), [b - a + 1 for a, b in runs])
    return sp, map_index, host_travel_distances(sp), runs[-1][0], np.arange(runs[-1][0], n, dtype=np.int32)


class LoopSearcherNearestHIP:
    """Drop-in for LoopSearcherNearest (constructor arguments as its settings group: TravelDistThreshold,
    NodeDistThreshold, NumOfCandidateNodes). search() returns the reference's candidate set, with the
    choice among equal distances at the cut specified (host_loop_candidates_nearest). The metric inputs of
    the last call are in last_metrics (AccumTravelDist, NodeDist per candidate, NumOfCandidateNodes)."""

    def __init__(self, travel_dist_threshold, node_dist_threshold, num_of_candidate_nodes, ctx=None):
        self.travel_dist_threshold = float(travel_dist_threshold)
        self.node_dist_threshold = float(node_dist_threshold)
        self.num_of_candidate_nodes = int(num_of_candidate_nodes)
        self.ctx = ctx or Context()
        self.last_metrics = None
        self.last_info = None

    def search(self, scan_poses, local_maps, accum_travel_dist, last_finished_map):
        """Search(searchHint): queries are the nodes of the last finished local map, references the nodes
        of the maps before it, every gate measured from accum_travel_dist. Returns (query scan node,
        reference scan node, reference local map) triples, nearest first."""
        sp, map_index, travel, n_ref, queries = loop_search_graph(scan_poses, local_maps, last_finished_map)
        rec, counts, self.last_info = self.ctx.loop_search(
            sp, map_index, travel, queries, float(accum_travel_dist), n_ref, self.travel_dist_threshold,
            self.node_dist_threshold, self.num_of_candidate_nodes, False)
        kept = host_loop_candidates_nearest(rec, counts, self.num_of_candidate_nodes)
        self.last_metrics = dict(AccumTravelDist=float(accum_travel_dist), NodeDist=[float(d) for d in kept["dist_sq"]],
                                 NumOfCandidateNodes=len(kept))
        return [(int(c["query_scan_index"]), int(c["ref_scan_index"]), int(c["ref_map_index"])) for c in kept]

    def search_per_map(self, scan_poses, local_maps, last_finished_map, query_nodes, n_per_query):
        """The one_per_map form: per query node the nearest reference node of each local map, the
        n_per_query nearest maps. Any node up to the last finished map's last may be a reference (the
        query's own local map never is) and each query's gate is measured from its own travel distance:
        the offline search of a finished graph. Returns the used (query, ref scan, ref map) triples, query
        by query in the order given."""
        sp, map_index, travel, _, _ = loop_search_graph(scan_poses, local_maps, last_finished_map)
        rec, counts, self.last_info = self.ctx.loop_search(
            sp, map_index, travel, query_nodes, None, None, self.travel_dist_threshold, self.node_dist_threshold,
            n_per_query, True, len(local_maps[:int(last_finished_map) + 1]))
        return [(int(c["query_scan_index"]), int(c["ref_scan_index"]), int(c["ref_map_index"]))
                for row, n in zip(rec, counts) for c in row[:n]]


class LoopSearcherAppearanceHIP:
    """The loop searcher by appearance, beside LoopSearcherNearestHIP and on the same loop_search_graph inputs
    plus the scans: scans[i] = (angles, ranges) of scan node i. A node's descriptor is built once, when a
    search first sees the node, and kept; a later search builds only those of new nodes (reset() forgets them).
    search() and search_per_map() return (query scan node, reference scan node, reference local map) triples
    as LoopSearcherNearestHIP does; last_records holds the records behind them (shift, distance,
    ring_distance) and last_headings the heading difference theta_query - theta_ref each shift implies: the
    centre of the theta window of the matcher that follows."""

    def __init__(self, travel_dist_threshold, max_distance, num_of_candidate_nodes, n_rings=20, n_sectors=64,
                 range_min=0.5, range_max=20.0, min_cell_sum=0, ctx=None):
        self.travel_dist_threshold = float(travel_dist_threshold)
        self.max_distance = int(max_distance)
        self.num_of_candidate_nodes = int(num_of_candidate_nodes)
        self.shape = (int(n_rings), int(n_sectors))
        self.range_min, self.range_max = float(range_min), float(range_max)
        self.min_cell_sum = int(min_cell_sum)
        self.ctx = ctx or Context()
        self.last_info = self.last_records = self.last_headings = None
        self.reset()

    def reset(self):
        self.descriptors = np.zeros((0,) + self.shape, np.uint8)
        self.beams_used = np.zeros(0, np.int32)

    def _descriptors(self, scans, n):
        """The descriptors of nodes [0, n): those kept, and the new nodes' in one device call."""
        have = self.descriptors.shape[0]
        if n > len(scans):
            raise CsmError(L.CSM_EINVAL, "loop search: a local map names a scan node whose scan is not given")
        if n > have:
            d, used = self.ctx.scan_descriptors(*ragged_scans(scans[have:n]), self.shape[0], self.shape[1],
                                                self.range_min, self.range_max)
            self.descriptors = np.concatenate([self.descriptors, d])
            self.beams_used = np.concatenate([self.beams_used, used])
        return self.descriptors[:n]

    def _run(self, desc, map_index, travel, queries, query_travel, n_ref, k, one_per_map, n_maps=None):
        rec, counts, self.last_info = self.ctx.appearance_search(
            desc, map_index, travel, queries, query_travel, n_ref, self.travel_dist_threshold, self.max_distance,
            self.min_cell_sum, k, one_per_map, n_maps, range_min=self.range_min, range_max=self.range_max)
        return np.concatenate([row[:n] for row, n in zip(rec, counts)]) if len(rec) else rec.reshape(-1)

    def _finish(self, used):
        self.last_records = used
        self.last_headings = [host_descriptor_shift_angle(c["shift"], self.shape[1]) for c in used]
        return [(int(c["query_scan_index"]), int(c["ref_scan_index"]), int(c["ref_map_index"])) for c in used]

    def search(self, scan_poses, local_maps, accum_travel_dist, last_finished_map, scans):
        """Queries are the nodes of the last finished local map, references the nodes of the maps before it,
        every gate measured from accum_travel_dist: the num_of_candidate_nodes pairs of least (distance,
        reference node, query node), nearest first."""
        sp, map_index, travel, n_ref, queries = loop_search_graph(scan_poses, local_maps, last_finished_map)
        used = self._run(self._descriptors(scans, len(sp)), map_index, travel, queries, float(accum_travel_dist),
                         n_ref, self.num_of_candidate_nodes, False)
        order = np.lexsort((used["query_scan_index"], used["ref_scan_index"], used["distance"]))
        return self._finish(used[order][:self.num_of_candidate_nodes])

    def search_per_map(self, scan_poses, local_maps, last_finished_map, query_nodes, n_per_query, scans):
        """Per query node the most similar reference node of each local map, the n_per_query most similar
        maps; any node up to the last finished map's last may be a reference and each query's gate is measured
        from its own travel distance. Returns the used triples, query by query in the order given."""
        sp, map_index, travel, _, _ = loop_search_graph(scan_poses, local_maps, last_finished_map)
        return self._finish(self._run(self._descriptors(scans, len(sp)), map_index, travel, query_nodes, None, None,
                                      n_per_query, True, len(local_maps[:int(last_finished_map) + 1])))
