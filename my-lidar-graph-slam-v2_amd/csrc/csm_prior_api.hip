/* csm_prior_api.hip -- the winner of a window under a motion prior (csm_score_window_prior,
 * csm_correlative_match_prior, csm_correlative_match_prior_batch, and the host restatements
 * csm_host_motion_prior / csm_host_prior_from_robot_information), with its kernels
 * (csm_prior_kernels.hip). A translation unit of libcsm_hip.so of its own.
 *
 * A unit on the volume's host driver (csm_peaks.hpp: volume_window, volume_batch), which runs the peaks'
 * stages: per chunk the scans are projected, every candidate is scored exactly and dumped, the coarse known
 * counts are counted (peaks_score_chunk; with 0 rounds no selection round of the peaks runs). What is this
 * unit's own: the quantisation of the prior (the named window's check of its sized window; the batch's
 * pre-pass ahead of the driver) and the chunk body (run_chunk) -- two launches on the same stream without a
 * host wait: one pass over every window's volume that keeps the winner under the prior and the unweighted
 * one side by side (one record per workgroup), and the pick that writes both records of every window. One
 * copy brings the csm_prior_results back. Scratch beyond the peaks' owners: pr_tab (job table, workgroup
 * records, results) and pr_pin. */
#include "csm_peaks.hpp"

#include "csm_prior_kernels.hip"

namespace {

int check_prior(csm_ctx* ctx, const csm_motion_prior* pr, const char* who)
{
    if (!pr || pr->scratch_limit_bytes < 0)
        return fail(ctx, CSM_EINVAL, "%s: no prior, or a negative scratch limit", who);
    return CSM_OK;
}

int d_max_of(const PeakWindow& pw) { return std::max(pw.w.n_theta, std::max(pw.f.nx, pw.f.ny)) - 1; }

int quantise(csm_ctx* ctx, const csm_motion_prior* pr, const double steps[3], int n_points, int d_max, int64_t Q[6],
             int index)
{
    if (csm_host_motion_prior(pr->information, steps, n_points, d_max, Q) != CSM_OK)
        return fail(ctx, CSM_EINVAL,
                    "window %d: the prior's information must be finite and symmetric, and its penalty over offsets "
                    "up to %d steps must stay below 2^62 key units", index, d_max);
    return CSM_OK;
}

/* The chunk body: windows [lo, hi) with their volume scored (ch): both winners. res[i - lo] receives them
 * (Q[i - lo] goes in and is returned in the record). */
int run_chunk(csm_ctx* ctx, const std::vector<PeakWindow>& wins, int lo, int hi, const PeakChunk& ch,
              const int64_t (*Q)[6], csm_prior_result* res)
{
    const int m = hi - lo;
    int rc;
    /* pr_tab: [jobs][workgroup records][results]; pr_pin: [jobs][results] */
    const size_t jobs_bytes = align256((size_t)m * sizeof(PriorJob));
    const size_t part_bytes = align256((size_t)m * kPeakBlocksMax * sizeof(PriorBest));
    const size_t out_bytes = (size_t)m * sizeof(csm_prior_result);
    if ((rc = reserve(ctx, ctx->pr_tab, jobs_bytes + part_bytes + out_bytes))) return rc;
    const size_t pin_bytes = jobs_bytes + out_bytes;
    if ((rc = grow(ctx, ctx->pr_pin, pin_bytes, pin_bytes + pin_bytes / 4, false))) return rc;
    char* const dev = ctx->pr_tab.as<char>();
    PriorJob* const jobs_dev = reinterpret_cast<PriorJob*>(dev);
    PriorBest* const part_dev = reinterpret_cast<PriorBest*>(dev + jobs_bytes);
    csm_prior_result* const out_dev = reinterpret_cast<csm_prior_result*>(dev + jobs_bytes + part_bytes);
    char* const pin = ctx->pr_pin.as<char>();
    PriorJob* const jobs_pin = reinterpret_cast<PriorJob*>(pin);
    char* const out_pin = pin + jobs_bytes;
    int blocks_max = 1;
    for (int k = 0; k < m; ++k) {
        const int64_t total = wins[lo + k].total;
        PriorJob& J = jobs_pin[k];
        for (int i = 0; i < 6; ++i)
            J.Q[i] = Q[k][i];
        J.out = out_dev + k;
        J.partial = part_dev + (size_t)k * kPeakBlocksMax;
        J.blocks = (int)std::min<int64_t>(kPeakBlocksMax, std::max<int64_t>(1, (total + 8191) / 8192));
        const int64_t chunk = (total + J.blocks - 1) / J.blocks;
        J.chunk = (int)((chunk + kPriorRun - 1) / kPriorRun * kPriorRun);
        blocks_max = std::max(blocks_max, J.blocks);
    }
    HIP_TRY(ctx, hipMemcpyAsync(jobs_dev, jobs_pin, (size_t)m * sizeof(PriorJob), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(out_dev, 0, out_bytes, ctx->stream));
    {
        ScopedTimer tm(ctx, "prior_select");
        if ((rc = launched_ok(ctx, csm_launch::launch(k_prior_argmax, dim3(blocks_max, m), dim3(kPriorBlock), ctx->stream,
                                                      ch.jobs_dev, (const PriorJob*)jobs_dev), "prior arg-max")))
            return rc;
        if ((rc = launched_ok(ctx, csm_launch::launch_lds(ctx->device, k_prior_pick, dim3(m), dim3(kPriorBlock),
                                                          (size_t)ch.n_points_max * 8, ctx->stream, ch.jobs_dev,
                                                          (const PriorJob*)jobs_dev), "prior pick")))
            return rc;
    }
    HIP_TRY(ctx, hipMemcpyAsync(out_pin, out_dev, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(res, out_pin, out_bytes);
    for (int k = 0; k < m; ++k)
        for (int i = 0; i < 6; ++i)
            res[k].Q[i] = Q[k][i];
    return CSM_OK;
}

/* The prior as a unit on the volume: no selection round of the peaks; the body leaves window i's result in
 * res[i], from Q[i]. The named-window entry adds its check, which fills Q[0]. */
VolumeUnit prior_unit(csm_ctx* ctx, int64_t scratch_limit, const int64_t (*Q)[6], csm_prior_result* res)
{
    VolumeUnit u;
    u.scratch_limit = scratch_limit;
    u.body = [=](std::vector<PeakWindow>& wins, int lo, int hi, const PeakChunk& ch) {
        return run_chunk(ctx, wins, lo, hi, ch, Q + lo, res + lo);
    };
    return u;
}

int prior_batch(csm_ctx* ctx, const csm_loop_query* queries, int n, const csm_correlative_params* prm,
                const csm_motion_prior* priors, csm_prior_summary* out)
{
    int rc;
    const double t0 = clock_us();
    std::vector<int64_t> Q((size_t)n * 6);
    int64_t (*const Qs)[6] = reinterpret_cast<int64_t (*)[6]>(Q.data());
    /* every refusal of the prior before anything is allocated (the set-up below may build a coarse level):
     * a window's shape needs nothing but the steps and the resident map. A query the set-up refuses anyway
     * (bad scan, map not resident) is left to it. */
    const int L = prm->low_resolution;
    for (int i = 0; i < n; ++i) {
        const csm_loop_query& q = queries[i];
        if (!q.scan.angles || !q.scan.ranges || q.scan.n_points < 1 || !scan_is_finite(&q.scan))
            continue;
        const DeviceGrid* g = find_grid(ctx, q.map_id);
        if (!g)
            continue;
        double st[3];
        csm_host_search_step(q.geometry.resolution, q.scan.ranges, q.scan.n_points, &st[0], &st[1], &st[2]);
        const int wx = csm_host_window(prm->range_x, st[0]), wy = csm_host_window(prm->range_y, st[1]);
        const int wt = csm_host_window(prm->range_theta, st[2]);
        if (wx < 0 || wy < 0 || wt < 0)
            continue;
        const WindowFrame f = window_frame(*g, wx, wy, L);
        const int d_max = std::max(2 * wt + 1, std::max(f.nx, f.ny)) - 1;
        if ((rc = quantise(ctx, &priors[i], st, q.scan.n_points, d_max, Qs[i], i))) return rc;
    }
    std::vector<csm_summary> head;
    std::vector<csm_prior_result> res(n);
    double setup, opt;
    const VolumeUnit unit = prior_unit(ctx, priors[0].scratch_limit_bytes, Qs, res.data());
    if ((rc = volume_batch(ctx, unit, queries, n, prm, t0, head, &setup, &opt))) return rc;
    std::memset(out, 0, sizeof(csm_prior_summary) * (size_t)n);
    for (int i = 0; i < n; ++i) {
        out[i].prior = res[i];
        fill_summary(out[i].summary, head[i], res[i].best, res[i].best.found, queries[i].scan.relative_sensor_pose,
                     setup, opt);
    }
    return CSM_OK;
}

} /* namespace */

extern "C" {

int csm_host_motion_prior(const double information[9], const double steps[3], int32_t n_points, int32_t d_max,
                          int64_t Q[6])
{
    if (!information || !steps || !Q || n_points < 1 || d_max < 0)
        return CSM_EINVAL;
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(information[i]))
            return CSM_EINVAL;
    for (int a = 0; a < 3; ++a)
        for (int b = a + 1; b < 3; ++b)
            if (information[3 * a + b] != information[3 * b + a])
                return CSM_EINVAL;
    const double N = (double)n_points;
    unsigned __int128 q_max = 0;
    int64_t tmp[6];
    for (int k = 0; k < 6; ++k) {
        const int a = kA[k], b = kB[k];
        const double m = a == b ? 0.5 : 1.0;
        const double q = ((((N / kKeyToScore) * m) * information[3 * a + b]) * steps[a]) * steps[b];
        const double v = q * 256.0;
        if (!(std::fabs(v) < 9223372036854775808.0))       /* also a NaN from non-finite steps */
            return CSM_EINVAL;
        tmp[k] = (int64_t)std::floor(v + 0.5);
        const unsigned __int128 mag = tmp[k] < 0 ? (unsigned __int128)(-(__int128)tmp[k]) : (unsigned __int128)tmp[k];
        q_max = std::max(q_max, mag);
    }
    const unsigned __int128 side = (unsigned __int128)d_max;
    if (6 * q_max * side * side >= ((unsigned __int128)1 << 62))
        return CSM_EINVAL;
    for (int k = 0; k < 6; ++k)
        Q[k] = tmp[k];
    return CSM_OK;
}

int csm_host_prior_from_robot_information(const double robot_information[9], const double initial_pose[3],
                                          const double rel_pose[3], double out[9])
{
    if (!robot_information || !initial_pose || !rel_pose || !out)
        return CSM_EINVAL;
    const double* const R = robot_information;
    double J[3][3], T[3][3];         /* J at the initial pose; J^T R, then (J^T R) J; each sum ((k0 + k1) + k2) */
    move_backward_jacobian(initial_pose[2], rel_pose, J);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            T[i][j] = (J[0][i] * R[j] + J[1][i] * R[3 + j]) + J[2][i] * R[6 + j];
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
            const double v = (T[i][0] * J[0][j] + T[i][1] * J[1][j]) + T[i][2] * J[2][j];
            out[3 * i + j] = v;
            out[3 * j + i] = v;
        }
    return CSM_OK;
}

int csm_score_window_prior(csm_ctx* ctx, uint64_t map_id, const csm_window* w, const int32_t* hit_col,
                           const int32_t* hit_row, const csm_motion_prior* prior, csm_prior_result* out)
{
    if (!ctx || !w || !hit_col || !hit_row || !out)
        return fail(ctx, CSM_EINVAL, "csm_score_window_prior: bad arguments");
    if (int rc = check_prior(ctx, prior, "csm_score_window_prior"))
        return rc;
    int64_t Q[1][6];
    VolumeUnit unit = prior_unit(ctx, prior->scratch_limit_bytes, Q, out);
    unit.check = [&](const PeakWindow& pw, int index) {
        return quantise(ctx, prior, prior->steps, w->n_points, d_max_of(pw), Q[0], index);
    };
    return volume_window(ctx, unit, map_id, w, hit_col, hit_row);
}

int csm_correlative_match_prior_batch(csm_ctx* ctx, const csm_loop_query* queries, int32_t n_queries,
                                      const csm_correlative_params* prm, const csm_motion_prior* priors,
                                      csm_prior_summary* out)
{
    if (!ctx || !queries || n_queries < 1 || !prm || !priors || !out || prm->low_resolution < 1)
        return fail(ctx, CSM_EINVAL, "csm_correlative_match_prior_batch: bad arguments");
    for (int i = 0; i < n_queries; ++i)
        if (int rc = check_prior(ctx, &priors[i], "csm_correlative_match_prior_batch"))
            return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return prior_batch(ctx, queries, n_queries, prm, priors, out);
}

int csm_correlative_match_prior(csm_ctx* ctx, uint64_t map_id, const csm_geometry* geom, const csm_scan* scan,
                                const double initial_pose[3], const csm_correlative_params* prm,
                                const csm_motion_prior* prior, csm_prior_summary* out)
{
    if (!ctx || !geom || !scan || !initial_pose || !prm || !out || prm->low_resolution < 1)
        return fail(ctx, CSM_EINVAL, "csm_correlative_match_prior: bad arguments");
    if (int rc = check_prior(ctx, prior, "csm_correlative_match_prior"))
        return rc;
    const csm_loop_query q = single_query(map_id, geom, scan, initial_pose);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return prior_batch(ctx, &q, 1, prm, prior, out);
}

} /* extern "C" */
