/* csm_volume_api.hip -- pose covariance read off a window's whole score volume (csm_score_window_moments,
 * csm_correlative_covariance, csm_correlative_covariance_batch, and the host restatements
 * csm_host_volume_weights / csm_host_volume_covariance), with its kernels (csm_volume_kernels.hip). A
 * translation unit of libcsm_hip.so of its own.
 *
 * A unit on the volume's host driver (csm_peaks.hpp: volume_window, volume_batch), which runs the peaks'
 * stages: per chunk the scans are projected, every candidate is scored exactly and dumped, the coarse known
 * counts are counted and ONE selection round picks the winner. What is this unit's own: the temperature
 * checks ahead of the driver, the range check of a sized window, and the chunk body (run_chunk) -- two more
 * launches on the same stream without a host wait: the moments of every window of the chunk (one record
 * per workgroup) and their sums per window. One copy brings the csm_volume_moments back; the covariance is
 * a fixed f64 expression of them on the host. Scratch beyond the peaks' owners: vc_tab (job table, weight
 * tables, workgroup records, results) and vc_pin. */
#include "csm_peaks.hpp"

#include "csm_volume_kernels.hip"

namespace {

constexpr double kWeightOne = 16777216.0;     /* 2^24 */

bool temperature_ok(double tau, int n_points)
{
    return std::isfinite(tau) && tau > 0.0 && ((17.0 * tau) * (double)n_points) / kKeyToScore < 4611686018427387904.0;
}

int check_params(csm_ctx* ctx, const csm_volume_params* vp, const char* who)
{
    if (!vp || !std::isfinite(vp->temperature) || !(vp->temperature > 0.0) || vp->scratch_limit_bytes < 0)
        return fail(ctx, CSM_EINVAL, "%s: temperature must be finite and > 0, scratch limit >= 0", who);
    return CSM_OK;
}

/* The refusals that are the moments' own: sums that could leave int64, a band that leaves the key range. */
int check_range(csm_ctx* ctx, const PeakWindow& pw, const csm_volume_params* vp, int index)
{
    const unsigned __int128 side = (unsigned __int128)(std::max(pw.w.n_theta, std::max(pw.f.nx, pw.f.ny)) - 1);
    if ((unsigned __int128)pw.total * side * side * ((unsigned __int128)1 << 24) >= ((unsigned __int128)1 << 63))
        return fail(ctx, CSM_EINVAL, "window %d: the second moments of %lld candidates could leave int64", index,
                    (long long)pw.total);
    if (!temperature_ok(vp->temperature, pw.w.n_points))
        return fail(ctx, CSM_EINVAL, "window %d: temperature %g puts the weight band beyond 2^62 keys", index,
                    vp->temperature);
    return CSM_OK;
}

struct WeightTable {
    uint32_t w[CSM_VOLUME_BINS];
    int32_t shift;
};

/* The chunk body: windows [lo, hi) with their volume scored and their winner picked (ch): moments.
 * mom[i - lo] receives them. */
int run_chunk(csm_ctx* ctx, const std::vector<PeakWindow>& wins, int lo, int hi, const PeakChunk& ch,
              const csm_volume_params* vp, csm_volume_moments* mom)
{
    const int m = hi - lo;
    int rc;
    /* one weight table per beam count of the chunk */
    std::map<int, int> table_of;
    std::vector<WeightTable> tables;
    for (int i = lo; i < hi; ++i) {
        const int np = wins[i].w.n_points;
        if (table_of.count(np))
            continue;
        table_of[np] = (int)tables.size();
        tables.emplace_back();
        csm_host_volume_weights(np, vp->temperature, tables.back().w, &tables.back().shift);
    }
    /* vc_tab: [jobs | tables][workgroup records][results]; vc_pin: [jobs | tables][results] */
    const size_t jobs_bytes = align256((size_t)m * sizeof(VolJob));
    const size_t tab_bytes = tables.size() * sizeof(uint32_t) * CSM_VOLUME_BINS;
    const size_t part_bytes = align256((size_t)m * kPeakBlocksMax * sizeof(VolSums));
    const size_t out_bytes = (size_t)m * sizeof(csm_volume_moments);
    if ((rc = reserve(ctx, ctx->vc_tab, jobs_bytes + tab_bytes + part_bytes + out_bytes))) return rc;
    const size_t pin_bytes = jobs_bytes + tab_bytes + out_bytes;
    if ((rc = grow(ctx, ctx->vc_pin, pin_bytes, pin_bytes + pin_bytes / 4, false))) return rc;
    char* const dev = ctx->vc_tab.as<char>();
    VolJob* const jobs_dev = reinterpret_cast<VolJob*>(dev);
    uint32_t* const tab_dev = reinterpret_cast<uint32_t*>(dev + jobs_bytes);
    VolSums* const part_dev = reinterpret_cast<VolSums*>(dev + jobs_bytes + tab_bytes);
    csm_volume_moments* const out_dev = reinterpret_cast<csm_volume_moments*>(dev + jobs_bytes + tab_bytes + part_bytes);
    char* const pin = ctx->vc_pin.as<char>();
    VolJob* const jobs_pin = reinterpret_cast<VolJob*>(pin);
    char* const out_pin = pin + jobs_bytes + tab_bytes;
    int blocks_max = 1;
    for (int k = 0; k < m; ++k) {
        const int ti = table_of[wins[lo + k].w.n_points];
        VolJob& J = jobs_pin[k];
        J.table = tab_dev + (size_t)ti * CSM_VOLUME_BINS;
        J.partial = part_dev + (size_t)k * kPeakBlocksMax;
        J.out = out_dev + k;
        J.bin_shift = tables[ti].shift;
        J.pad = 0;
        blocks_max = std::max(blocks_max, ch.jobs_pin[k].blocks);
    }
    for (size_t ti = 0; ti < tables.size(); ++ti)
        std::memcpy(pin + jobs_bytes + ti * sizeof(tables[ti].w), tables[ti].w, sizeof(tables[ti].w));
    HIP_TRY(ctx, hipMemcpyAsync(dev, pin, jobs_bytes + tab_bytes, hipMemcpyHostToDevice, ctx->stream));
    {
        ScopedTimer tm(ctx, "volume_moments");
        if ((rc = launched_ok(ctx, csm_launch::launch(k_volume_moments, dim3(blocks_max, m), dim3(kVolBlock), ctx->stream,
                                                      ch.jobs_dev, (const VolJob*)jobs_dev), "volume moments")))
            return rc;
    }
    {
        ScopedTimer tm(ctx, "volume_reduce");
        if ((rc = launched_ok(ctx, csm_launch::launch(k_volume_reduce, dim3(m), dim3(kVolBlock), ctx->stream,
                                                      ch.jobs_dev, (const VolJob*)jobs_dev), "volume reduction")))
            return rc;
    }
    HIP_TRY(ctx, hipMemcpyAsync(out_pin, out_dev, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(mom, out_pin, out_bytes);
    return CSM_OK;
}

/* The covariance as a unit on the volume: one selection round picks the winner, the range check runs on the
 * sized window, the body leaves window i's moments in mom[i]. */
VolumeUnit covariance_unit(csm_ctx* ctx, const csm_volume_params* vp, csm_volume_moments* mom)
{
    VolumeUnit u;
    u.sel.rounds = 1;
    u.scratch_limit = vp->scratch_limit_bytes;
    u.check = [=](const PeakWindow& pw, int index) { return check_range(ctx, pw, vp, index); };
    u.body = [=](std::vector<PeakWindow>& wins, int lo, int hi, const PeakChunk& ch) {
        return run_chunk(ctx, wins, lo, hi, ch, vp, mom + lo);
    };
    return u;
}

int covariance_batch(csm_ctx* ctx, const csm_loop_query* queries, int n, const csm_correlative_params* prm,
                     const csm_volume_params* vp, csm_volume_summary* out)
{
    const double t0 = clock_us();
    /* every refusal before anything is allocated: the windows' shapes need nothing but the steps */
    for (int i = 0; i < n; ++i)
        if (queries[i].scan.n_points >= 1 && !temperature_ok(vp->temperature, queries[i].scan.n_points))
            return fail(ctx, CSM_EINVAL, "query %d: temperature %g puts the weight band beyond 2^62 keys", i,
                        vp->temperature);
    std::vector<csm_summary> head;
    std::vector<csm_volume_moments> mom(n);
    double setup, opt;
    if (int rc = volume_batch(ctx, covariance_unit(ctx, vp, mom.data()), queries, n, prm, t0, head, &setup, &opt))
        return rc;
    std::memset(out, 0, sizeof(csm_volume_summary) * (size_t)n);
    for (int i = 0; i < n; ++i) {
        csm_volume_summary& v = out[i];
        v.moments = mom[i];
        csm_summary& o = v.summary;
        fill_summary(o, head[i], mom[i].best, mom[i].best.found, queries[i].scan.relative_sensor_pose, setup, opt);
        if (!mom[i].best.found)
            continue;
        const double steps[3] = { o.step_x, o.step_y, o.step_theta };
        csm_host_volume_covariance(&v.moments, steps, o.estimated_pose, queries[i].scan.relative_sensor_pose,
                                   v.mean_offset, v.sensor_covariance, v.covariance);
    }
    return CSM_OK;
}

} /* namespace */

extern "C" {

int csm_host_volume_weights(int32_t n_points, double temperature, uint32_t table[CSM_VOLUME_BINS], int32_t* bin_shift)
{
    if (n_points < 1 || !table || !bin_shift || !temperature_ok(temperature, n_points))
        return CSM_EINVAL;
    const double N = (double)n_points;
    const int64_t band_keys = (int64_t)std::ceil(((17.0 * temperature) * N) / kKeyToScore);
    int32_t s = 0;
    while ((band_keys >> s) >= CSM_VOLUME_BINS)
        ++s;
    for (int64_t b = 0; b < CSM_VOLUME_BINS; ++b)
        table[b] = (uint32_t)std::floor(kWeightOne * std::exp(-((double)(b << s) * kKeyToScore) / (N * temperature)) + 0.5);
    *bin_shift = s;
    return CSM_OK;
}

int csm_host_volume_covariance(const csm_volume_moments* m, const double steps[3], const double estimated_pose[3],
                               const double rel_pose[3], double mean_offset[3], double sensor_cov[9], double cov[9])
{
    if (!m || !steps || !estimated_pose || !rel_pose || !mean_offset || !sensor_cov || !cov)
        return CSM_EINVAL;
    for (int i = 0; i < 3; ++i)
        mean_offset[i] = 0.0;
    for (int i = 0; i < 9; ++i)
        sensor_cov[i] = cov[i] = 0.0;
    if (m->m0 <= 0)
        return CSM_OK;
    const double m0 = (double)m->m0;
    for (int k = 0; k < 6; ++k) {
        const int a = kA[k], b = kB[k];
        const __int128 num = (__int128)m->m0 * m->m2[k] - (__int128)m->m1[a] * m->m1[b];
        const double idx = (double)num / (m0 * m0);
        const double v = (idx * steps[a]) * steps[b];
        sensor_cov[3 * a + b] = v;
        sensor_cov[3 * b + a] = v;
    }
    for (int a = 0; a < 3; ++a)
        mean_offset[a] = ((double)m->m1[a] / m0) * steps[a];
    double J[3][3], T[3][3];         /* J at the estimated pose; J S, then (J S) J^T; each sum ((k0 + k1) + k2) */
    move_backward_jacobian(estimated_pose[2], rel_pose, J);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            T[i][j] = (J[i][0] * sensor_cov[j] + J[i][1] * sensor_cov[3 + j]) + J[i][2] * sensor_cov[6 + j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            cov[3 * i + j] = (T[i][0] * J[j][0] + T[i][1] * J[j][1]) + T[i][2] * J[j][2];
    return CSM_OK;
}

int csm_score_window_moments(csm_ctx* ctx, uint64_t map_id, const csm_window* w, const int32_t* hit_col,
                             const int32_t* hit_row, const csm_volume_params* vp, csm_volume_moments* out)
{
    if (!ctx || !w || !hit_col || !hit_row || !out)
        return fail(ctx, CSM_EINVAL, "csm_score_window_moments: bad arguments");
    if (int rc = check_params(ctx, vp, "csm_score_window_moments"))
        return rc;
    if (w->n_points >= 1 && !temperature_ok(vp->temperature, w->n_points))
        return fail(ctx, CSM_EINVAL, "csm_score_window_moments: temperature %g puts the weight band beyond 2^62 keys",
                    vp->temperature);
    return volume_window(ctx, covariance_unit(ctx, vp, out), map_id, w, hit_col, hit_row);
}

int csm_correlative_covariance_batch(csm_ctx* ctx, const csm_loop_query* queries, int32_t n_queries,
                                     const csm_correlative_params* prm, const csm_volume_params* vp,
                                     csm_volume_summary* out)
{
    if (!ctx || !queries || n_queries < 1 || !prm || !out || prm->low_resolution < 1)
        return fail(ctx, CSM_EINVAL, "csm_correlative_covariance_batch: bad arguments");
    if (int rc = check_params(ctx, vp, "csm_correlative_covariance_batch"))
        return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return covariance_batch(ctx, queries, n_queries, prm, vp, out);
}

int csm_correlative_covariance(csm_ctx* ctx, uint64_t map_id, const csm_geometry* geom, const csm_scan* scan,
                               const double initial_pose[3], const csm_correlative_params* prm,
                               const csm_volume_params* vp, csm_volume_summary* out)
{
    if (!ctx || !geom || !scan || !initial_pose || !prm || !out || prm->low_resolution < 1)
        return fail(ctx, CSM_EINVAL, "csm_correlative_covariance: bad arguments");
    if (int rc = check_params(ctx, vp, "csm_correlative_covariance"))
        return rc;
    const csm_loop_query q = single_query(map_id, geom, scan, initial_pose);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return covariance_batch(ctx, &q, 1, prm, vp, out);
}

} /* extern "C" */
