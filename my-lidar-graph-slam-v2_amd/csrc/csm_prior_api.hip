/* csm_prior_api.hip -- the winner of a window under a motion prior (csm_score_window_prior,
 * csm_correlative_match_prior, csm_correlative_match_prior_batch, and the host restatements
 * csm_host_motion_prior / csm_host_prior_from_robot_information), with its kernels
 * (csm_prior_kernels.hip). A translation unit of libcsm_hip.so of its own.
 *
 * The volume comes from the peaks' stages (csm_peaks.hpp): per chunk the scans are projected, every
 * candidate is scored exactly and dumped, the coarse known counts are counted (peaks_score_chunk: no
 * selection round of the peaks runs). Two launches follow on the same stream without a host wait: one pass
 * over every window's volume that keeps the winner under the prior and the unweighted one side by side
 * (one record per workgroup), and the pick that writes both records of every window. One copy brings the
 * csm_prior_results back. Scratch beyond the peaks' owners: pr_tab (job table, workgroup records,
 * results) and pr_pin. */
#include "csm_peaks.hpp"

#include "csm_prior_kernels.hip"

namespace {

/* score = key * kKeyToScore / n_points */
constexpr double kKeyToScore = 0.998 / (65534.0 * 499.0);

static const int kA[6] = { 0, 0, 0, 1, 1, 2 }, kB[6] = { 0, 1, 2, 1, 2, 2 };    /* xx xy xt yy yt tt */

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

/* Windows [lo, hi) with their hit indices in pk_hits: volume, both winners. res[i - lo] receives them
 * (Q[i - lo] goes in and is returned in the record). */
int run_chunk(csm_ctx* ctx, std::vector<PeakWindow>& wins, int lo, int hi, const int64_t (*Q)[6], int64_t scratch_limit,
              csm_prior_result* res)
{
    const int m = hi - lo;
    int rc;
    const csm_peaks_params one = { 1, 0, 0, 0, scratch_limit };
    PeakChunk ch;
    if ((rc = peaks_score_chunk(ctx, wins, lo, hi, &one, &ch))) return rc;

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

int prior_batch(csm_ctx* ctx, const csm_loop_query* queries, int n, const csm_correlative_params* prm,
                const csm_motion_prior* priors, csm_prior_summary* out)
{
    int rc;
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t limit = priors[0].scratch_limit_bytes;
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
    std::vector<PeakWindow> wins;
    std::vector<csm_summary> head;
    if ((rc = peaks_prepare_queries(ctx, queries, n, prm, limit, wins, head))) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    std::vector<csm_prior_result> res(n);
    for (int lo = 0, hi; lo < n; lo = hi) {
        hi = peaks_next_chunk(wins, lo, limit);
        if ((rc = peaks_project_chunk(ctx, queries, wins, head, lo, hi))) return rc;
        if ((rc = run_chunk(ctx, wins, lo, hi, Qs + lo, limit, res.data() + lo))) return rc;
    }
    const auto t2 = std::chrono::steady_clock::now();
    const double setup = std::chrono::duration<double, std::micro>(t1 - t0).count() / n;
    const double opt = std::chrono::duration<double, std::micro>(t2 - t1).count() / n;
    std::memset(out, 0, sizeof(csm_prior_summary) * (size_t)n);
    for (int i = 0; i < n; ++i) {
        csm_prior_summary& v = out[i];
        v.prior = res[i];
        csm_summary& o = v.summary;
        o = head[i];
        o.input_setup_us = setup;
        o.optimization_us = opt;
        if (!res[i].best.found)
            continue;
        o.raw = res[i].best;
        peaks_fill_poses(o, queries[i].scan.relative_sensor_pose);
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
    /* J: MoveBackward(sensor pose, rel_pose) by the sensor pose, at the initial pose */
    const double sn = std::sin(initial_pose[2]), cs = std::cos(initial_pose[2]);
    const double J[3][3] = { { 1.0, 0.0, sn * rel_pose[0] + cs * rel_pose[1] },
                             { 0.0, 1.0, -cs * rel_pose[0] + sn * rel_pose[1] },
                             { 0.0, 0.0, 1.0 } };
    double T[3][3];         /* J^T R, then (J^T R) J; each sum ((k0 + k1) + k2) */
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
    int rc;
    if ((rc = check_prior(ctx, prior, "csm_score_window_prior"))) return rc;
    std::vector<PeakWindow> wins(1);
    PeakWindow& pw = wins[0];
    pw.map_id = map_id;
    pw.w = *w;
    if ((rc = peaks_size_window(ctx, pw, prior->scratch_limit_bytes, 0))) return rc;
    int64_t Q[1][6];
    if ((rc = quantise(ctx, prior, prior->steps, w->n_points, d_max_of(pw), Q[0], 0))) return rc;
    if (w->low_resolution > 1 &&
        (w->coarse_level < 0 || w->coarse_level >= (int)pw.grid->levels.size() || pw.grid->levels[w->coarse_level].stale ||
         pw.grid->levels[w->coarse_level].win != w->low_resolution))
        return fail(ctx, CSM_ENOENT, "level %d does not hold box-max(%d)", w->coarse_level, w->low_resolution);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t hn = (size_t)w->n_theta * w->n_points;
    if ((rc = reserve(ctx, ctx->pk_hits, hn * 8))) return rc;
    pw.hit_off = 0;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->pk_hits.p, hit_col, hn * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->pk_hits.as<int32_t>() + hn, hit_row, hn * 4, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = run_chunk(ctx, wins, 0, 1, Q, prior->scratch_limit_bytes, out))) {
        (void)hipStreamSynchronize(ctx->stream);    /* no copy from the caller's arrays stays pending */
        return rc;
    }
    return CSM_OK;
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
    csm_loop_query q;
    std::memset(&q, 0, sizeof(q));
    q.map_id = map_id;
    q.geometry = *geom;
    q.scan = *scan;
    for (int k = 0; k < 3; ++k)
        q.initial_pose[k] = initial_pose[k];
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return prior_batch(ctx, &q, 1, prm, prior, out);
}

} /* extern "C" */
