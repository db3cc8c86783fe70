/* csm_cost_api.hip -- host side of the batched cost / covariance / linear-solver
 * entry points, with their kernels (csm_cost_kernels.hip). A translation unit of
 * libcsm_hip.so of its own. */
#include "csm_internal.hpp"

#include "csm_cost_kernels.hip"


namespace csm_host {

namespace {

int launch_block_allocation(csm_ctx* ctx, DeviceGrid& g, int log2b, const uint8_t* carried, int carried_brows,
                            int carried_bcols, int carried_br0, int carried_bc0)
{
    const int brows = (g.rows + (1 << log2b) - 1) >> log2b, bcols = (g.cols + (1 << log2b) - 1) >> log2b;
    const size_t bytes = (size_t)brows * bcols;
    if (bytes > 0x7fffffff)
        return fail(ctx, CSM_EINVAL, "block allocation: %zu blocks", bytes);
    if (int rc = grow(ctx, g.alloc, bytes, bytes + 64, false))
        return rc;
    const int e = launch(k_block_allocation, dim3((unsigned)bytes), dim3(256), ctx->stream, g.levels[0].cells, g.rows,
                         g.cols, g.pitch, log2b, bcols, carried, carried_brows, carried_bcols, carried_br0, carried_bc0,
                         g.alloc.as<uint8_t>());
    if (int rc = launched_ok(ctx, e, "block allocation"))
        return rc;
    g.alloc_log2 = log2b;
    g.alloc_bcols = bcols;
    g.alloc_stale = false;
    return CSM_OK;
}

} /* namespace */

int ensure_allocation(csm_ctx* ctx, DeviceGrid& g)
{
    if (!g.alloc_stale)
        return CSM_OK;          /* current, or a bitmap as given / carried (never stale) */
    return launch_block_allocation(ctx, g, g.alloc_log2, nullptr, 0, 0, 0, 0);
}

int build_allocation(csm_ctx* ctx, DeviceGrid& g, int log2b, const uint8_t* carried, int carried_brows,
                     int carried_bcols, int carried_br0, int carried_bc0)
{
    g.alloc_derived = false;
    return launch_block_allocation(ctx, g, log2b, carried, carried_brows, carried_bcols, carried_br0, carried_bc0);
}

} /* namespace csm_host */

namespace {

/* poses: n x 3 sensor poses (sensor_given) or null = Compound(query initial pose, relative sensor pose) */
int run_cost_batch(csm_ctx* ctx, const csm_loop_query* queries, int32_t n, const double* sensor_poses,
                   const csm_refine_params* prm, bool refine, csm_refine_result* out)
{
    if (!ctx || !queries || n < 1 || !prm || !out || !(prm->covariance_scale > 0.0) ||
        (refine && (prm->iterations_max < 1 || !(prm->convergence_threshold >= 0.0))))
        return fail(ctx, CSM_EINVAL, "bad arguments");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc;
    size_t scan_total = 0;
    std::vector<size_t> scan_off((size_t)n);
    for (int i = 0; i < n; ++i) {
        const csm_loop_query& q = queries[i];
        if (!q.scan.angles || !q.scan.ranges || q.scan.n_points < 1 || !scan_is_finite(&q.scan))
            return fail(ctx, CSM_EINVAL, "query %d: empty scan or non-finite beam", i);
        DeviceGrid* g = find_grid(ctx, q.map_id);
        if (!g)
            return fail(ctx, CSM_ENOENT, "query %d: map %llu not resident", i, (unsigned long long)q.map_id);
        if ((rc = ensure_allocation(ctx, *g)))
            return rc;
        scan_off[i] = scan_total;
        scan_total += 2 * (size_t)q.scan.n_points;
    }
    if ((rc = ensure(ctx, ctx->c_scans, scan_total * 8 + 64))) return rc;
    if ((rc = ensure(ctx, ctx->c_jobs, (size_t)n * (sizeof(CostJob) + sizeof(CostOut)) + 256))) return rc;
    /* host staging owned by the context: the sources of the asynchronous uploads stay alive */
    ctx->c_stage.resize(scan_total);
    ctx->c_job_stage.resize((size_t)n);
    double* d_scans = reinterpret_cast<double*>(ctx->c_scans.p);
    CostJob* d_jobs = reinterpret_cast<CostJob*>(ctx->c_jobs.p);
    CostOut* d_out = reinterpret_cast<CostOut*>(d_jobs + n);
    for (int i = 0; i < n; ++i) {
        const csm_loop_query& q = queries[i];
        const int np = q.scan.n_points;
        std::memcpy(ctx->c_stage.data() + scan_off[i], q.scan.angles, (size_t)np * 8);
        std::memcpy(ctx->c_stage.data() + scan_off[i] + np, q.scan.ranges, (size_t)np * 8);
        const DeviceGrid& g = *find_grid(ctx, q.map_id);
        CostJob& J = ctx->c_job_stage[i];
        std::memset(&J, 0, sizeof(J));
        J.cells = g.levels[0].cells;
        J.rows = g.rows;
        J.cols = g.cols;
        J.pitch = g.pitch;
        J.alloc = g.alloc.as<uint8_t>();
        J.log2_block = g.alloc_log2;
        J.block_cols = g.alloc_bcols;
        J.res = q.geometry.resolution;
        J.off_x = q.geometry.offset_x;
        J.off_y = q.geometry.offset_y;
        J.angles = d_scans + scan_off[i];
        J.ranges = d_scans + scan_off[i] + np;
        J.n = np;
        J.iterations_max = refine ? prm->iterations_max : 0;
        if (sensor_poses) {
            for (int k = 0; k < 3; ++k)
                J.sensor_pose[k] = sensor_poses[3 * i + k];
        } else {
            /* scan_matcher_linear_solver.cpp:78-81 */
            csm_host_compound(q.initial_pose, q.scan.relative_sensor_pose, J.sensor_pose);
        }
        J.convergence_threshold = prm->convergence_threshold;
        J.lambda = prm->lambda;
        J.covariance_scale = prm->covariance_scale;
        J.lut = ctx->lut_dev.as<double>();
        J.out = d_out + i;
    }
    HIP_TRY(ctx, hipMemcpyAsync(d_scans, ctx->c_stage.data(), scan_total * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_jobs, ctx->c_job_stage.data(), (size_t)n * sizeof(CostJob),
                                hipMemcpyHostToDevice, ctx->stream));
    {
        ScopedTimer tm(ctx, "cost_refine");
        const int e = launch(k_cost_refine, dim3(n), dim3(kCostBlock), ctx->stream, d_jobs);
        if ((rc = launched_ok(ctx, e, "cost refine")))
            return rc;
    }
    std::vector<CostOut> res((size_t)n);
    HIP_TRY(ctx, hipMemcpyAsync(res.data(), d_out, (size_t)n * sizeof(CostOut), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < n; ++i) {
        const csm_loop_query& q = queries[i];
        const CostOut& o = res[i];
        csm_refine_result& r = out[i];
        std::memset(&r, 0, sizeof(r));
        const double np = static_cast<double>(q.scan.n_points);
        r.normalized_initial_cost = o.initial_cost / np;
        r.normalized_cost = o.cost / np;
        for (int k = 0; k < 3; ++k) {
            r.sensor_pose[k] = ctx->c_job_stage[i].sensor_pose[k];
            r.best_sensor_pose[k] = o.best_sensor_pose[k];
        }
        /* scan_matcher_linear_solver.cpp:118-119 / scan_matcher_correlative.cpp:214-216 */
        csm_host_move_backward(r.best_sensor_pose, q.scan.relative_sensor_pose, r.estimated_pose);
        for (int k = 0; k < 9; ++k) {
            r.covariance[k] = o.covariance[k];
            r.hessian[k] = o.hessian[k];
        }
        r.lambda = o.lambda;
        r.iterations = o.iterations;
    }
    return CSM_OK;
}

} /* namespace */

extern "C" {

int csm_set_block_allocation(csm_ctx* ctx, uint64_t map_id, int32_t log2_block_size, const uint8_t* allocated)
{
    if (!ctx || log2_block_size < 0 || log2_block_size > 12)
        return fail(ctx, CSM_EINVAL, "csm_set_block_allocation: bad arguments");
    DeviceGrid* g = find_grid(ctx, map_id);
    if (!g)
        return fail(ctx, CSM_ENOENT, "map %llu not resident", (unsigned long long)map_id);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    g->alloc_log2 = log2_block_size;
    g->alloc_derived = true;
    g->alloc_stale = true;
    if (!allocated)
        return CSM_OK;              /* back to the rule "a block with a known cell is allocated" */
    const int bs = 1 << log2_block_size;
    const int brows = (g->rows + bs - 1) >> log2_block_size, bcols = (g->cols + bs - 1) >> log2_block_size;
    const size_t bytes = (size_t)brows * bcols;
    if (int rc = grow(ctx, g->alloc, bytes, bytes + 64, false))
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(g->alloc.p, allocated, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    g->alloc_bcols = bcols;
    g->alloc_derived = false;
    g->alloc_stale = false;
    return CSM_OK;
}

int csm_cost_covariance_batch(csm_ctx* ctx, const csm_loop_query* queries, int32_t n_queries,
                              const double* sensor_poses, double covariance_scale, csm_refine_result* out)
{
    if (!sensor_poses)
        return fail(ctx, CSM_EINVAL, "csm_cost_covariance_batch: bad arguments");
    csm_refine_params prm {};
    prm.covariance_scale = covariance_scale;
    return run_cost_batch(ctx, queries, n_queries, sensor_poses, &prm, false, out);
}

int csm_linear_solver_batch(csm_ctx* ctx, const csm_loop_query* queries, int32_t n_queries,
                            const csm_refine_params* params, csm_refine_result* out)
{
    return run_cost_batch(ctx, queries, n_queries, nullptr, params, true, out);
}

} /* extern "C" */
