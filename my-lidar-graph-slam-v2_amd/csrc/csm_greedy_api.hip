/* csm_greedy_api.hip -- host side of the greedy-endpoint cost / covariance batch and the
 * hill-climbing matcher, with their kernels (csm_greedy_kernels.hip) and the host restatements
 * (csm_host_greedy_cost, csm_host_hill_climbing) that are both the fallback of uncertified queries
 * and the CPU-testable reference. A translation unit of libcsm_hip.so of its own. */
#include "csm_internal.hpp"

#include "csm_greedy_kernels.hip"


namespace {

/* CostGreedyEndpoint::SetupLookupTable (cost_function_greedy_endpoint.cpp:160-196) and the
 * two integer thresholds of the occupancy tests (:72-80) */
struct GreedyTables {
    std::vector<double> lut;     /* (2k+1)^2, ky-major */
    double def = 0.0;
    std::vector<double> vals;    /* ascending distinct values of lut + def */
    std::vector<uint8_t> off_rank;
    int default_rank = 0;
    int vh_lo = 65536, vm_hi = 0;
};

bool greedy_params_ok(const csm_greedy_params* p)
{
    return p && p->kernel_size >= 0 && p->kernel_size <= CSM_GREEDY_KERNEL_SIZE_MAX &&
           p->standard_deviation > 0.0 && std::isfinite(p->standard_deviation) &&
           std::isfinite(p->map_resolution) && std::isfinite(p->hit_and_missed_dist) &&
           std::isfinite(p->occupancy_threshold) && std::isfinite(p->scaling_factor);
}

bool hill_params_ok(const csm_hill_climbing_params* p)
{
    return p && greedy_params_ok(&p->cost) && p->linear_step > 0.0 && std::isfinite(p->linear_step) &&
           p->angular_step > 0.0 && std::isfinite(p->angular_step) && p->max_iterations >= 1;
}

bool scan_ok(const csm_scan* s)
{
    return s && s->angles && s->ranges && s->n_points >= 1 && scan_is_finite(s);
}

const double* probability_lut()
{
    static std::vector<double> lut = [] {
        std::vector<double> v(65536);
        csm_host_probability_lut(v.data());
        return v;
    }();
    return lut.data();
}

bool build_tables(const csm_greedy_params& p, GreedyTables& T)
{
    const int k = p.kernel_size, K = 2 * k + 1;
    const double variance = p.standard_deviation * p.standard_deviation;
    T.lut.assign((size_t)K * K, 0.0);
    for (int ky = -k; ky <= k; ++ky) {
        for (int kx = -k; kx <= k; ++kx) {
            const double dx = p.map_resolution * kx, dy = p.map_resolution * ky;
            const double sq = dx * dx + dy * dy;
            T.lut[(size_t)(k + ky) * K + (k + kx)] = -std::exp(-0.5 * sq / variance);
        }
    }
    const double mdx = p.map_resolution * (k + 1), mdy = p.map_resolution * (k + 1);
    const double msq = mdx * mdx + mdy * mdy;
    T.def = -std::exp(-0.5 * msq / variance);
    /* ranks from the computed doubles: equal values share a rank, whatever produced them */
    T.vals = T.lut;
    T.vals.push_back(T.def);
    std::sort(T.vals.begin(), T.vals.end());
    T.vals.erase(std::unique(T.vals.begin(), T.vals.end()), T.vals.end());
    if ((int)T.vals.size() > kGreedyMaxVals)
        return false;
    auto rank_of = [&](double v) {
        return (int)(std::lower_bound(T.vals.begin(), T.vals.end(), v) - T.vals.begin());
    };
    T.off_rank.assign((size_t)K * K, 0);
    for (size_t t = 0; t < T.lut.size(); ++t)
        T.off_rank[t] = (uint8_t)rank_of(T.lut[t]);
    T.default_rank = rank_of(T.def);
    /* LUT[v] is non-decreasing on 1..65535: "hit < thr" fails from the first v with LUT[v] >= thr
     * on, "missed > thr" fails up to the last v with LUT[v] <= thr */
    const double* plut = probability_lut();
    for (int v = 2; v < 65536; ++v)
        if (plut[v] < plut[v - 1])
            return false;
    T.vh_lo = 65536;
    T.vm_hi = 0;
    for (int v = 1; v < 65536; ++v) {
        if (T.vh_lo == 65536 && !(plut[v] < p.occupancy_threshold))
            T.vh_lo = v;
        if (!(plut[v] > p.occupancy_threshold))
            T.vm_hi = v;
    }
    return true;
}

/* CostGreedyEndpoint::Cost, statement by statement (cost_function_greedy_endpoint.cpp:34-98) */
double host_cost(const uint16_t* grid, int rows, int cols, const csm_geometry& geom, const csm_scan& scan,
                 const double pose[3], const csm_greedy_params& p, const GreedyTables& T)
{
    const double* plut = probability_lut();
    auto prob_or = [&](int row, int col) {
        /* GridMap::ProbabilityOr(row, col, UnknownProbability = 0.0) */
        if (row < 0 || row >= rows || col < 0 || col >= cols)
            return 0.0;
        return plut[grid[(size_t)row * cols + col]];
    };
    const int k = p.kernel_size, K = 2 * k + 1;
    double sum = 0.0;
    for (int i = 0; i < scan.n_points; ++i) {
        const double r = scan.ranges[i], a = scan.angles[i];
        /* ScanData::HitAndMissedPoint: two hit points of one direction, at r and at r - HitAndMissedDist */
        double hx, hy, mx, my;
        host_hit_point(pose[0], pose[1], pose[2], r, a, &hx, &hy);
        host_hit_point(pose[0], pose[1], pose[2], r - p.hit_and_missed_dist, a, &mx, &my);
        const int hc = cell_index(hx, geom.offset_x, geom.resolution);
        const int hr = cell_index(hy, geom.offset_y, geom.resolution);
        const int mc = cell_index(mx, geom.offset_x, geom.resolution);
        const int mr = cell_index(my, geom.offset_y, geom.resolution);
        double mn = T.def;
        for (int ky = -k; ky <= k; ++ky) {
            for (int kx = -k; kx <= k; ++kx) {
                const double hp = prob_or(hr + ky, hc + kx);
                const double mp = prob_or(mr + ky, mc + kx);
                if (hp == 0.0 || mp == 0.0)
                    continue;
                if (hp < p.occupancy_threshold || mp > p.occupancy_threshold)
                    continue;
                mn = std::min(mn, T.lut[(size_t)(k + ky) * K + (k + kx)]);
            }
        }
        sum += mn;
    }
    sum *= p.scaling_factor;
    return sum;
}

/* ComputeGradient + ComputeCovariance (cost_function_greedy_endpoint.cpp:101-157) */
void host_covariance(const uint16_t* grid, int rows, int cols, const csm_geometry& geom, const csm_scan& scan,
                     const double pose[3], const csm_greedy_params& p, const GreedyTables& T, double cov[9])
{
    const double dl = geom.resolution, da = 1e-2;
    const double d[3][3] = { { dl, 0.0, 0.0 }, { 0.0, dl, 0.0 }, { 0.0, 0.0, da } };
    double g[3];
    for (int j = 0; j < 3; ++j) {
        const double plus[3] = { pose[0] + d[j][0], pose[1] + d[j][1], pose[2] + d[j][2] };
        const double minus[3] = { pose[0] - d[j][0], pose[1] - d[j][1], pose[2] - d[j][2] };
        const double diff = host_cost(grid, rows, cols, geom, scan, plus, p, T) -
                            host_cost(grid, rows, cols, geom, scan, minus, p, T);
        g[j] = 0.5 * diff / (j < 2 ? dl : da);
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            cov[3 * i + j] = g[i] * g[j];
    cov[0] += 0.1;
    cov[4] += 0.1;
    cov[8] += 0.1;
}

void fill_metrics(const double initial_pose[3], csm_hill_climbing_result& r)
{
    r.diff_translation = std::hypot(initial_pose[0] - r.estimated_pose[0], initial_pose[1] - r.estimated_pose[1]);
    r.diff_rotation = std::abs(initial_pose[2] - r.estimated_pose[2]);
}

/* ScanMatcherHillClimbing::OptimizePose, statement by statement (scan_matcher_hill_climbing.cpp:72-180) */
void host_hill_climbing(const uint16_t* grid, int rows, int cols, const csm_geometry& geom, const csm_scan& scan,
                        const double initial_pose[3], const csm_hill_climbing_params& hp, const GreedyTables& T,
                        csm_hill_climbing_result& out)
{
    static const double move_x[] = { 1.0, -1.0, 0.0, 0.0, 0.0, 0.0 };
    static const double move_y[] = { 0.0, 0.0, 1.0, -1.0, 0.0, 0.0 };
    static const double move_t[] = { 0.0, 0.0, 0.0, 0.0, 1.0, -1.0 };
    std::memset(&out, 0, sizeof(out));
    double sensor[3];
    csm_host_compound(initial_pose, scan.relative_sensor_pose, sensor);
    const double initial_cost = host_cost(grid, rows, cols, geom, scan, sensor, hp.cost, T);
    const double n = static_cast<double>(scan.n_points);
    double min_cost = initial_cost;
    double best[3] = { sensor[0], sensor[1], sensor[2] };
    int iterations = 0, refinements = 0;
    double lin = hp.linear_step, ang = hp.angular_step;
    bool updated = false;
    int64_t evals = 1;
    do {
        double min_local = min_cost;
        double best_local[3] = { best[0], best[1], best[2] };
        updated = false;
        for (int i = 0; i < 6; ++i) {
            double pose[3] = { best[0], best[1], best[2] };
            pose[0] += move_x[i] * lin;
            pose[1] += move_y[i] * lin;
            pose[2] += move_t[i] * ang;
            const double c = host_cost(grid, rows, cols, geom, scan, pose, hp.cost, T);
            ++evals;
            if (c < min_local) {
                min_local = c;
                for (int j = 0; j < 3; ++j)
                    best_local[j] = pose[j];
                updated = true;
            }
        }
        if (updated) {
            min_cost = min_local;
            for (int j = 0; j < 3; ++j)
                best[j] = best_local[j];
        } else {
            ++refinements;
            lin *= 0.5;
            ang *= 0.5;
        }
    } while ((updated || refinements < hp.max_refinements) && (++iterations < hp.max_iterations));
    out.normalized_initial_cost = initial_cost / n;
    out.normalized_cost = min_cost / n;
    for (int j = 0; j < 3; ++j) {
        out.sensor_pose[j] = sensor[j];
        out.best_sensor_pose[j] = best[j];
    }
    csm_host_move_backward(best, scan.relative_sensor_pose, out.estimated_pose);
    host_covariance(grid, rows, cols, geom, scan, best, hp.cost, T, out.covariance);
    out.iterations = iterations;
    out.refinements = refinements;
    out.cost_evaluations = evals + 6;
    fill_metrics(initial_pose, out);
}

/* sensor_poses != null: cost + covariance at those poses (mode 1); else OptimizePose (mode 0) */
int run_greedy_batch(csm_ctx* ctx, const csm_loop_query* queries, int32_t n, const double* sensor_poses,
                     const csm_hill_climbing_params& hp, csm_hill_climbing_result* out)
{
    const bool hill = sensor_poses == nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    GreedyTables T;
    if (!build_tables(hp.cost, T))
        return fail(ctx, CSM_EINVAL, "greedy cost: value table does not fit");
    size_t scan_total = 0, scratch_total = 0;
    std::vector<size_t> scan_off((size_t)n), scratch_off((size_t)n);
    for (int i = 0; i < n; ++i) {
        const csm_loop_query& q = queries[i];
        if (!scan_ok(&q.scan) || !(q.geometry.resolution > 0.0))
            return fail(ctx, CSM_EINVAL, "query %d: empty scan, non-finite beam or bad geometry", i);
        if (q.scan.n_points > 10240)
            return fail(ctx, CSM_EINVAL, "query %d: more than 10240 beams", i);
        if (!find_grid(ctx, q.map_id))
            return fail(ctx, CSM_ENOENT, "query %d: map %llu not resident", i, (unsigned long long)q.map_id);
        scan_off[i] = scan_total;
        scan_total += 2 * (size_t)q.scan.n_points;
        scratch_off[i] = scratch_total;
        if (q.scan.n_points > kGreedyLdsBeams)
            scratch_total += (size_t)kGreedySlots * ((q.scan.n_points + 15) & ~15);
    }
    int rc;
    if ((rc = ensure(ctx, ctx->g_scans, scan_total * 8 + 64))) return rc;
    if ((rc = ensure(ctx, ctx->g_jobs, (size_t)n * (sizeof(GreedyJob) + sizeof(GreedyOut)) + 256))) return rc;
    if ((rc = ensure(ctx, ctx->g_tab, sizeof(GreedyTab) + 64))) return rc;
    if (scratch_total && (rc = ensure(ctx, ctx->g_scratch, scratch_total + 64))) return rc;

    GreedyTab tab;
    std::memset(&tab, 0, sizeof(tab));
    for (size_t v = 0; v < T.vals.size(); ++v)
        tab.vals[v] = T.vals[v];
    for (size_t t = 0; t < T.off_rank.size(); ++t)
        tab.off_rank[t] = T.off_rank[t];
    tab.hit_missed_dist = hp.cost.hit_and_missed_dist;
    tab.scaling = hp.cost.scaling_factor;
    tab.linear_step = hp.linear_step;
    tab.angular_step = hp.angular_step;
    tab.k = hp.cost.kernel_size;
    tab.n_vals = (int)T.vals.size();
    tab.default_rank = T.default_rank;
    tab.vh_lo = T.vh_lo;
    tab.vm_hi = T.vm_hi;
    tab.max_iterations = hp.max_iterations;
    tab.max_refinements = hp.max_refinements;
    tab.literal = ctx->tune.greedy_literal ? 1 : 0;

    std::vector<double> stage(scan_total);
    std::vector<GreedyJob> jobs((size_t)n);
    std::vector<std::array<double, 3>> start((size_t)n);
    double* d_scans = reinterpret_cast<double*>(ctx->g_scans.p);
    GreedyJob* d_jobs = reinterpret_cast<GreedyJob*>(ctx->g_jobs.p);
    GreedyOut* d_out = reinterpret_cast<GreedyOut*>(d_jobs + n);
    for (int i = 0; i < n; ++i) {
        const csm_loop_query& q = queries[i];
        const int np = q.scan.n_points;
        std::memcpy(stage.data() + scan_off[i], q.scan.angles, (size_t)np * 8);
        std::memcpy(stage.data() + scan_off[i] + np, q.scan.ranges, (size_t)np * 8);
        const DeviceGrid& g = *find_grid(ctx, q.map_id);
        GreedyJob& J = jobs[i];
        std::memset(&J, 0, sizeof(J));
        J.cells = g.levels[0].cells;
        J.angles = d_scans + scan_off[i];
        J.ranges = d_scans + scan_off[i] + np;
        J.scratch = np > kGreedyLdsBeams ? reinterpret_cast<uint8_t*>(ctx->g_scratch.p) + scratch_off[i] : nullptr;
        J.rows = g.rows;
        J.cols = g.cols;
        J.pitch = g.pitch;
        J.n = np;
        J.mode = hill ? 0 : 1;
        J.stride = (np + 15) & ~15;
        J.res = q.geometry.resolution;
        J.off_x = q.geometry.offset_x;
        J.off_y = q.geometry.offset_y;
        if (hill)
            csm_host_compound(q.initial_pose, q.scan.relative_sensor_pose, start[i].data());   /* :89-93 */
        else
            for (int j = 0; j < 3; ++j)
                start[i][j] = sensor_poses[3 * i + j];
        for (int j = 0; j < 3; ++j)
            J.start[j] = start[i][j];
    }
    HIP_TRY(ctx, hipMemcpyAsync(ctx->g_tab.p, &tab, sizeof(tab), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_scans, stage.data(), scan_total * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_jobs, jobs.data(), (size_t)n * sizeof(GreedyJob), hipMemcpyHostToDevice,
                                ctx->stream));
    {
        ScopedTimer tm(ctx, "greedy");
        const int e = launch(k_greedy, dim3(n), dim3(kGreedyBlock), ctx->stream,
                             reinterpret_cast<const GreedyTab*>(ctx->g_tab.p), d_jobs, d_out);
        if ((rc = launched_ok(ctx, e, "greedy")))
            return rc;
    }
    std::vector<GreedyOut> res((size_t)n);
    HIP_TRY(ctx, hipMemcpyAsync(res.data(), d_out, (size_t)n * sizeof(GreedyOut), hipMemcpyDeviceToHost,
                                ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

    std::map<uint64_t, std::vector<uint16_t>> host_grids;   /* maps of the queries the host finishes */
    for (int i = 0; i < n; ++i) {
        const csm_loop_query& q = queries[i];
        const GreedyOut& o = res[i];
        csm_hill_climbing_result& r = out[i];
        std::memset(&r, 0, sizeof(r));
        if (o.uncertain) {
            const DeviceGrid& g = *find_grid(ctx, q.map_id);
            auto it = host_grids.find(q.map_id);
            if (it == host_grids.end()) {
                std::vector<uint16_t> cells((size_t)g.rows * g.cols);
                if ((rc = csm_download_level(ctx, q.map_id, 0, cells.data())))
                    return rc;
                it = host_grids.emplace(q.map_id, std::move(cells)).first;
            }
            if (hill) {
                host_hill_climbing(it->second.data(), g.rows, g.cols, q.geometry, q.scan, q.initial_pose, hp, T, r);
            } else {
                const double c = host_cost(it->second.data(), g.rows, g.cols, q.geometry, q.scan, start[i].data(),
                                           hp.cost, T);
                r.normalized_initial_cost = r.normalized_cost = c / static_cast<double>(q.scan.n_points);
                for (int j = 0; j < 3; ++j)
                    r.sensor_pose[j] = r.best_sensor_pose[j] = start[i][j];
                csm_host_move_backward(r.best_sensor_pose, q.scan.relative_sensor_pose, r.estimated_pose);
                host_covariance(it->second.data(), g.rows, g.cols, q.geometry, q.scan, start[i].data(), hp.cost, T,
                                r.covariance);
                r.cost_evaluations = 7;
                fill_metrics(q.initial_pose, r);
            }
            r.host_path = 1;
            continue;
        }
        const double np = static_cast<double>(q.scan.n_points);
        r.normalized_initial_cost = o.initial_cost / np;
        r.normalized_cost = o.cost / np;
        for (int j = 0; j < 3; ++j) {
            r.sensor_pose[j] = start[i][j];
            r.best_sensor_pose[j] = o.best[j];
        }
        csm_host_move_backward(r.best_sensor_pose, q.scan.relative_sensor_pose, r.estimated_pose);
        for (int j = 0; j < 9; ++j)
            r.covariance[j] = o.cov[j];
        r.iterations = o.iterations;
        r.refinements = o.refinements;
        r.replays = o.replays;
        r.cost_evaluations = o.evals;
        fill_metrics(q.initial_pose, r);
    }
    return CSM_OK;
}

} /* namespace */

extern "C" {

int csm_greedy_cost_covariance_batch(csm_ctx* ctx, const csm_loop_query* queries, int32_t n_queries,
                                     const double* sensor_poses, const csm_greedy_params* params,
                                     csm_hill_climbing_result* out)
{
    if (!ctx || !queries || n_queries < 1 || !sensor_poses || !out || !greedy_params_ok(params))
        return fail(ctx, CSM_EINVAL, "csm_greedy_cost_covariance_batch: bad arguments");
    for (int i = 0; i < 3 * n_queries; ++i)
        if (!std::isfinite(sensor_poses[i]))
            return fail(ctx, CSM_EINVAL, "csm_greedy_cost_covariance_batch: non-finite sensor pose");
    csm_hill_climbing_params hp {};
    hp.linear_step = hp.angular_step = 1.0;
    hp.max_iterations = 1;
    hp.cost = *params;
    return run_greedy_batch(ctx, queries, n_queries, sensor_poses, hp, out);
}

int csm_hill_climbing_batch(csm_ctx* ctx, const csm_loop_query* queries, int32_t n_queries,
                            const csm_hill_climbing_params* params, csm_hill_climbing_result* out)
{
    if (!ctx || !queries || n_queries < 1 || !out || !hill_params_ok(params))
        return fail(ctx, CSM_EINVAL, "csm_hill_climbing_batch: bad arguments");
    for (int i = 0; i < n_queries; ++i)
        for (int j = 0; j < 3; ++j)
            if (!std::isfinite(queries[i].initial_pose[j]))
                return fail(ctx, CSM_EINVAL, "csm_hill_climbing_batch: non-finite initial pose");
    return run_greedy_batch(ctx, queries, n_queries, nullptr, *params, out);
}

int csm_host_greedy_cost(const uint16_t* grid, int32_t rows, int32_t cols, const csm_geometry* geom,
                         const csm_scan* scan, const double sensor_pose[3], const csm_greedy_params* params,
                         double* cost, double* covariance)
{
    GreedyTables T;
    if (!grid || rows < 1 || cols < 1 || !geom || !(geom->resolution > 0.0) || !scan_ok(scan) || !sensor_pose ||
        !cost || !greedy_params_ok(params) || !build_tables(*params, T))
        return CSM_EINVAL;
    *cost = host_cost(grid, rows, cols, *geom, *scan, sensor_pose, *params, T);
    if (covariance)
        host_covariance(grid, rows, cols, *geom, *scan, sensor_pose, *params, T, covariance);
    return CSM_OK;
}

int csm_host_hill_climbing(const uint16_t* grid, int32_t rows, int32_t cols, const csm_geometry* geom,
                           const csm_scan* scan, const double initial_pose[3],
                           const csm_hill_climbing_params* params, csm_hill_climbing_result* out)
{
    GreedyTables T;
    if (!grid || rows < 1 || cols < 1 || !geom || !(geom->resolution > 0.0) || !scan_ok(scan) || !initial_pose ||
        !out || !hill_params_ok(params) || !build_tables(params->cost, T))
        return CSM_EINVAL;
    host_hill_climbing(grid, rows, cols, *geom, *scan, initial_pose, *params, T, *out);
    return CSM_OK;
}

} /* extern "C" */
