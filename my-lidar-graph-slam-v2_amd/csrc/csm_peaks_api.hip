/* csm_peaks_api.hip -- the K best distinct poses per window (csm_score_window_peaks, csm_correlative_peaks,
 * csm_correlative_peaks_batch), with their kernels (csm_peaks_kernels.hip). A translation unit of
 * libcsm_hip.so of its own.
 *
 * A batch is cut into chunks whose score volumes fit the scratch limit. Per chunk: the scans are projected
 * on the device (a window with an entry the projection cannot certify is projected again on the host),
 * the batched exhaustive chain scores every candidate exactly and dumps S and K
 * (csm_score_windows_dump_dev), the coarse nodes' known counts are counted, and k_max selection rounds
 * of two launches each pick the peaks of all the chunk's windows, with no host wait between the rounds.
 * The records and the peak counts come back in one copy. The host waits for the projection's flags and
 * for that copy (and wherever the scoring chain itself waits). The scratch lives in the context's owners
 * (pk_vol, pk_hits, pk_tab, pk_pin).
 *
 * The three entry shapes -- a named window with the caller's hit indices, a batch of queries, one query --
 * are the host driver's (volume_window, volume_batch, single_query; declared in csm_peaks.hpp, defined
 * here), which the covariance and the prior use too. To the driver the peaks are a unit like those two:
 * k_max selection rounds, no check of a sized window, and a chunk body that launches nothing and copies
 * the records back (peaks_unit). */
#include "csm_peaks.hpp"

#include "csm_peaks_kernels.hip"

namespace {

int check_params(csm_ctx* ctx, const csm_peaks_params* pk, const char* who)
{
    if (!pk || pk->k_max < 1 || pk->k_max > CSM_PEAKS_MAX || pk->excl_x < 0 || pk->excl_y < 0 ||
        pk->excl_theta < 0 || pk->scratch_limit_bytes < 0)
        return fail(ctx, CSM_EINVAL, "%s: k_max must be 1..%d, exclusion radii and scratch limit >= 0", who,
                    CSM_PEAKS_MAX);
    return CSM_OK;
}

} /* namespace */

namespace csm_host {

int peaks_size_window(csm_ctx* ctx, PeakWindow& pw, int64_t scratch_limit, int index)
{
    const csm_window& w = pw.w;
    if (w.n_theta < 1 || (w.n_theta & 1) == 0 || w.n_points < 1 || w.win_x < 0 || w.win_y < 0 || w.low_resolution < 1)
        return fail(ctx, CSM_EINVAL, "window %d: bad window", index);
    pw.grid = find_grid(ctx, pw.map_id);
    if (!pw.grid)
        return fail(ctx, CSM_ENOENT, "window %d: map %llu not resident", index, (unsigned long long)pw.map_id);
    const int L = w.low_resolution;
    pw.f = window_frame(*pw.grid, w.win_x, w.win_y, L);
    pw.total = (int64_t)w.n_theta * pw.f.nx * pw.f.ny;
    if (pw.total > kPeaksMaxCandidates)
        return fail(ctx, CSM_EINVAL, "window %d: %lld candidates, more than the %lld the peak selection takes", index,
                    (long long)pw.total, (long long)kPeaksMaxCandidates);
    pw.vol_bytes = align256((size_t)pw.total * 4) + align256((size_t)pw.total * 2) +
                   (L > 1 ? align256((size_t)(pw.total / (L * L)) * 2) : 0);
    const int64_t limit = scratch_limit ? scratch_limit : kPeaksDefaultScratch;
    if ((int64_t)pw.vol_bytes > limit)
        return fail(ctx, CSM_EINVAL, "window %d: its score volume (%zu bytes) exceeds the scratch limit (%lld)", index,
                    pw.vol_bytes, (long long)limit);
    return CSM_OK;
}

/* The stages up to the selection: job table, exact scores, coarse known counts. */
static int peaks_score_chunk(csm_ctx* ctx, std::vector<PeakWindow>& wins, int lo, int hi, const PeakRounds& sel,
                             PeakChunk* out)
{
    const int m = hi - lo, k_max = std::max(1, sel.rounds);
    int rc;
    size_t vol_total = 0;
    for (int i = lo; i < hi; ++i)
        vol_total += wins[i].vol_bytes;
    if ((rc = reserve(ctx, ctx->pk_vol, vol_total))) return rc;

    /* pk_tab: [jobs][chain records][peak records | states][workgroup records] */
    const size_t jobs_bytes = align256((size_t)m * sizeof(PeakJob));
    const size_t chain_bytes = align256((size_t)m * sizeof(csm_result));
    const size_t back_bytes = (size_t)m * k_max * sizeof(csm_result) + (size_t)m * 8;
    const size_t part_bytes = (size_t)m * kPeakBlocksMax * sizeof(BlockBest);
    if ((rc = reserve(ctx, ctx->pk_tab, jobs_bytes + chain_bytes + align256(back_bytes) + part_bytes))) return rc;
    const size_t pin_bytes = jobs_bytes + align256(back_bytes);
    if ((rc = grow(ctx, ctx->pk_pin, pin_bytes, pin_bytes + pin_bytes / 4, false))) return rc;
    char* const tab = ctx->pk_tab.as<char>();
    PeakJob* const jobs_dev = reinterpret_cast<PeakJob*>(tab);
    csm_result* const chain_dev = reinterpret_cast<csm_result*>(tab + jobs_bytes);
    csm_result* const rec_dev = reinterpret_cast<csm_result*>(tab + jobs_bytes + chain_bytes);
    int32_t* const state_dev = reinterpret_cast<int32_t*>(rec_dev + (size_t)m * k_max);
    BlockBest* const part_dev = reinterpret_cast<BlockBest*>(tab + jobs_bytes + chain_bytes + align256(back_bytes));
    PeakJob* const jobs_pin = ctx->pk_pin.as<PeakJob>();
    char* const back_pin = ctx->pk_pin.as<char>() + jobs_bytes;

    std::vector<uint64_t> ids(m);
    std::vector<csm_window> cw(m);
    std::vector<const int32_t*> cols(m), rows(m);
    std::vector<uint32_t*> ds(m);
    std::vector<uint16_t*> dk(m);
    char* vol = ctx->pk_vol.as<char>();
    int n_points_max = 0;
    long nodes_max = 0;
    for (int k = 0; k < m; ++k) {
        const PeakWindow& pw = wins[lo + k];
        const DeviceGrid& g = *pw.grid;
        const int L = pw.w.low_resolution;
        ids[k] = pw.map_id;
        cw[k] = pw.w;
        cols[k] = reinterpret_cast<const int32_t*>(ctx->pk_hits.as<char>() + pw.hit_off);
        rows[k] = cols[k] + (size_t)pw.w.n_theta * pw.w.n_points;
        ds[k] = reinterpret_cast<uint32_t*>(vol);
        vol += align256((size_t)pw.total * 4);
        dk[k] = reinterpret_cast<uint16_t*>(vol);
        vol += align256((size_t)pw.total * 2);
        PeakJob& J = jobs_pin[k];
        std::memset(&J, 0, sizeof(J));
        J.s = ds[k];
        J.k = dk[k];
        if (L > 1) {
            J.ck = reinterpret_cast<uint16_t*>(vol);
            vol += align256((size_t)(pw.total / (L * L)) * 2);
            J.coarse = g.levels[pw.w.coarse_level].cells;
            nodes_max = std::max<long>(nodes_max, (long)(pw.total / (L * L)));
        }
        J.cells = g.levels[0].cells;
        J.rows = g.rows;
        J.cols = g.cols;
        J.pitch = g.pitch;
        J.hit_col = cols[k];
        J.hit_row = rows[k];
        J.lut = ctx->lut_dev.as<double>();
        J.chain = chain_dev + k;
        J.out = rec_dev + (size_t)k * k_max;
        J.state = state_dev + 2 * k;
        J.partial = part_dev + (size_t)k * kPeakBlocksMax;
        J.n_theta = pw.w.n_theta;
        J.n_points = pw.w.n_points;
        J.win_theta = (pw.w.n_theta - 1) / 2;
        J.nx = pw.f.nx;
        J.ny = pw.f.ny;
        J.L = L;
        J.x_lo = pw.f.x_lo;
        J.y_lo = pw.f.y_lo;
        J.min_known = pw.w.min_known;
        J.blocks = (int)std::min<int64_t>(kPeakBlocksMax, std::max<int64_t>(1, (pw.total + 8191) / 8192));
        J.chunk = (int)((pw.total + J.blocks - 1) / J.blocks);
        J.k_max = k_max;
        J.excl_x = sel.excl_x;
        J.excl_y = sel.excl_y;
        J.excl_theta = sel.excl_theta;
        J.score_thr = pw.w.score_threshold;
        n_points_max = std::max(n_points_max, pw.w.n_points);
    }

    /* every candidate's exact sums: the batched exhaustive chain with its dumps */
    if ((rc = csm_score_windows_dump_dev(ctx, m, ids.data(), cw.data(), cols.data(), rows.data(), chain_dev, ds.data(),
                                         dk.data(), nullptr)))
        return rc;

    HIP_TRY(ctx, hipMemcpyAsync(jobs_dev, jobs_pin, (size_t)m * sizeof(PeakJob), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(rec_dev, 0, back_bytes, ctx->stream));
    if (nodes_max > 0) {
        ScopedTimer tm(ctx, "peaks_coarse");
        const unsigned bx = (unsigned)std::min<long>(256, (nodes_max + kPeakBlock - 1) / kPeakBlock);
        if ((rc = launched_ok(ctx, csm_launch::launch(k_peaks_coarse_known, dim3(bx, m), dim3(kPeakBlock), ctx->stream,
                                                      (const PeakJob*)jobs_dev), "coarse known count")))
            return rc;
    }
    out->jobs_dev = jobs_dev;
    out->jobs_pin = jobs_pin;
    out->rec_dev = rec_dev;
    out->back_bytes = back_bytes;
    out->back_pin = back_pin;
    out->n_points_max = n_points_max;
    return CSM_OK;
}

int peaks_select_chunk(csm_ctx* ctx, std::vector<PeakWindow>& wins, int lo, int hi, const PeakRounds& sel,
                       PeakChunk* out)
{
    const int m = hi - lo;
    int rc;
    if ((rc = peaks_score_chunk(ctx, wins, lo, hi, sel, out))) return rc;
    const PeakJob* const jobs_dev = out->jobs_dev;
    const int n_points_max = out->n_points_max;
    int blocks_max = 1;
    for (int k = 0; k < m; ++k)
        blocks_max = std::max(blocks_max, out->jobs_pin[k].blocks);
    if (sel.rounds > 0) {
        ScopedTimer tm(ctx, "peaks_select");
        for (int round = 0; round < sel.rounds; ++round) {
            if ((rc = launched_ok(ctx, csm_launch::launch(k_peaks_argmax, dim3(blocks_max, m), dim3(kPeakBlock), ctx->stream,
                                                          jobs_dev, round), "peak arg-max")))
                return rc;
            if ((rc = launched_ok(ctx, csm_launch::launch_lds(ctx->device, k_peaks_pick, dim3(m), dim3(kPeakBlock),
                                                              (size_t)n_points_max * 8, ctx->stream,
                                                              jobs_dev, round), "peak pick")))
                return rc;
        }
    }
    return CSM_OK;
}

} /* namespace csm_host */

namespace {

/* The peaks' chunk body: nothing to launch. rec[k * k_max + j] and n_peaks[k] of the chunk's window k receive
 * the result. */
int copy_back(csm_ctx* ctx, const PeakChunk& ch, int m, int k_max, csm_result* rec, int32_t* n_peaks)
{
    char* const back_pin = ch.back_pin;
    HIP_TRY(ctx, hipMemcpyAsync(back_pin, ch.rec_dev, ch.back_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(rec, back_pin, (size_t)m * k_max * sizeof(csm_result));
    const int32_t* state = reinterpret_cast<const int32_t*>(back_pin + (size_t)m * k_max * sizeof(csm_result));
    for (int k = 0; k < m; ++k)
        n_peaks[k] = state[2 * k];
    return CSM_OK;
}

/* The peaks as a unit on the volume: k_max rounds, no check of their own; window i's records go to
 * rec[i * k_max ...] and its count to n_peaks[i]. */
VolumeUnit peaks_unit(csm_ctx* ctx, const csm_peaks_params* pk, csm_result* rec, int32_t* n_peaks)
{
    VolumeUnit u;
    const int k_max = pk->k_max;
    u.sel = { k_max, pk->excl_x, pk->excl_y, pk->excl_theta };
    u.scratch_limit = pk->scratch_limit_bytes;
    u.body = [=](std::vector<PeakWindow>&, int lo, int hi, const PeakChunk& ch) {
        return copy_back(ctx, ch, hi - lo, k_max, rec + (size_t)lo * k_max, n_peaks + lo);
    };
    return u;
}

} /* namespace */

namespace csm_host {

int peaks_next_chunk(const std::vector<PeakWindow>& wins, int lo, int64_t scratch_limit)
{
    const int64_t limit = scratch_limit ? scratch_limit : kPeaksDefaultScratch;
    int64_t sum = 0;
    int hi = lo;
    while (hi < (int)wins.size() && (hi == lo || sum + (int64_t)wins[hi].vol_bytes <= limit))
        sum += (int64_t)wins[hi++].vol_bytes;
    return hi;
}

int peaks_prepare_queries(csm_ctx* ctx, const csm_loop_query* queries, int n, const csm_correlative_params* prm,
                          int64_t scratch_limit, std::vector<PeakWindow>& wins, std::vector<csm_summary>& head)
{
    int rc;
    const int L = prm->low_resolution;
    wins.assign(n, PeakWindow());
    head.resize(n);
    for (int i = 0; i < n; ++i) {
        const csm_loop_query& q = queries[i];
        if (!q.scan.angles || !q.scan.ranges || q.scan.n_points < 1 || !scan_is_finite(&q.scan))
            return fail(ctx, CSM_EINVAL, "query %d: empty scan or non-finite beam", i);
        csm_summary& o = head[i];
        std::memset(&o, 0, sizeof(o));
        csm_host_compound(q.initial_pose, q.scan.relative_sensor_pose, o.sensor_pose);
        csm_host_search_step(q.geometry.resolution, q.scan.ranges, q.scan.n_points, &o.step_x, &o.step_y, &o.step_theta);
        o.win_x = csm_host_window(prm->range_x, o.step_x);
        o.win_y = csm_host_window(prm->range_y, o.step_y);
        o.win_theta = csm_host_window(prm->range_theta, o.step_theta);
        PeakWindow& pw = wins[i];
        pw.map_id = q.map_id;
        pw.w.n_theta = 2 * o.win_theta + 1;
        pw.w.n_points = q.scan.n_points;
        pw.w.win_x = o.win_x;
        pw.w.win_y = o.win_y;
        pw.w.low_resolution = L;
        pw.w.min_known = csm_host_min_known(q.scan.n_points, prm->known_rate_threshold);
        pw.w.score_threshold = prm->score_threshold;
        pw.w.merge_mode = merging_pays(q.scan.angles, q.scan.ranges, q.scan.n_points, q.geometry.resolution) ? 0 : 1;
        if ((rc = peaks_size_window(ctx, pw, scratch_limit, i))) return rc;
        o.candidates = pw.total;
    }
    {
        PendingBoxes pending;       /* an error return before the launch leaves what it holds stale */
        for (int i = 0; i < n; ++i)
            if ((rc = level_for_window(ctx, *wins[i].grid, L, &wins[i].w.coarse_level, &pending))) return rc;
        if ((rc = launch_box_jobs(ctx, pending))) return rc;
    }
    return CSM_OK;
}

int peaks_project_chunk(csm_ctx* ctx, const csm_loop_query* queries, std::vector<PeakWindow>& wins,
                        const std::vector<csm_summary>& head, int lo, int hi)
{
    int rc;
    const int m = hi - lo;
    /* pk_hits: [scans][hit indices]; pk_pin (staging): [projection jobs | flag words][scans] */
    size_t scan_bytes = 0, hit_bytes = 0;
    for (int i = lo; i < hi; ++i)
        scan_bytes += (size_t)wins[i].w.n_points * 16;
    scan_bytes = align256(scan_bytes);
    for (int i = lo; i < hi; ++i) {
        wins[i].hit_off = scan_bytes + hit_bytes;
        hit_bytes += align256((size_t)wins[i].w.n_theta * wins[i].w.n_points * 8);
    }
    const size_t proj_bytes = align256((size_t)m * sizeof(ProjJob)), flag_bytes = align256((size_t)m * 4);
    if ((rc = reserve(ctx, ctx->pk_hits, scan_bytes + hit_bytes + proj_bytes + flag_bytes))) return rc;
    const size_t pin_bytes = proj_bytes + flag_bytes + scan_bytes;
    if ((rc = grow(ctx, ctx->pk_pin, pin_bytes, pin_bytes + pin_bytes / 4, false))) return rc;
    char* const dev = ctx->pk_hits.as<char>();
    ProjJob* const proj_dev = reinterpret_cast<ProjJob*>(dev + scan_bytes + hit_bytes);
    uint32_t* const flags_dev = reinterpret_cast<uint32_t*>(dev + scan_bytes + hit_bytes + proj_bytes);
    ProjJob* const proj_pin = ctx->pk_pin.as<ProjJob>();
    uint32_t* const flags_pin = reinterpret_cast<uint32_t*>(ctx->pk_pin.as<char>() + proj_bytes);
    double* const scans_pin = reinterpret_cast<double*>(ctx->pk_pin.as<char>() + proj_bytes + flag_bytes);
    size_t off = 0;
    int n_points_max = 0, n_theta_max = 0;
    for (int i = lo; i < hi; ++i) {
        const csm_loop_query& q = queries[i];
        const int np = q.scan.n_points;
        std::memcpy(scans_pin + off, q.scan.angles, (size_t)np * 8);
        std::memcpy(scans_pin + off + np, q.scan.ranges, (size_t)np * 8);
        int32_t* col = reinterpret_cast<int32_t*>(dev + wins[i].hit_off);
        ProjJob& I = proj_pin[i - lo];
        I = proj_job(q.geometry, head[i].sensor_pose, head[i].step_theta, head[i].win_theta, np,
                     reinterpret_cast<double*>(dev) + off, reinterpret_cast<double*>(dev) + off + np, col,
                     col + (size_t)wins[i].w.n_theta * np);
        I.flags = flags_dev + (i - lo);
        I.flag_uncertain = 1;
        off += 2 * (size_t)np;
        n_points_max = std::max(n_points_max, np);
        n_theta_max = std::max(n_theta_max, wins[i].w.n_theta);
    }
    std::memset(flags_pin, 0, flag_bytes);
    HIP_TRY(ctx, hipMemcpyAsync(dev, scans_pin, off * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(proj_dev, proj_pin, proj_bytes + flag_bytes, hipMemcpyHostToDevice, ctx->stream));
    {
        ScopedTimer tm(ctx, "project");
        const int pb = ceil_div(n_points_max, kBlock);
        if ((rc = launched_ok(ctx, csm_launch::project_batch(ctx->stream, dim3(pb, proj_theta_groups(n_theta_max, (long)pb * m), m),
                                                             proj_dev), "projection")))
            return rc;
    }
    HIP_TRY(ctx, hipMemcpyAsync(flags_pin, flags_dev, (size_t)m * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = lo; i < hi; ++i) {
        if (!(flags_pin[i - lo] & CSM_FLAG_PROJ_DELTA))
            continue;
        /* an entry too close to a cell edge for the device's sin / cos: this window with glibc */
        const csm_loop_query& q = queries[i];
        const size_t hn = (size_t)wins[i].w.n_theta * q.scan.n_points;
        std::vector<int32_t> cr(2 * hn);
        csm_host_project(&q.geometry, head[i].sensor_pose, head[i].step_theta, head[i].win_theta, q.scan.angles,
                         q.scan.ranges, q.scan.n_points, cr.data(), cr.data() + hn, nullptr, nullptr);
        HIP_TRY(ctx, hipMemcpy(dev + wins[i].hit_off, cr.data(), hn * 8, hipMemcpyHostToDevice));
    }
    return CSM_OK;
}

/* ---- the host driver of the units on the volume ---- */

int volume_window(csm_ctx* ctx, const VolumeUnit& u, uint64_t map_id, const csm_window* w, const int32_t* hit_col,
                  const int32_t* hit_row)
{
    int rc;
    std::vector<PeakWindow> wins(1);
    PeakWindow& pw = wins[0];
    pw.map_id = map_id;
    pw.w = *w;
    if ((rc = peaks_size_window(ctx, pw, u.scratch_limit, 0))) return rc;
    if (u.check && (rc = u.check(pw, 0))) return rc;
    if (w->low_resolution > 1 && !level_holds(*pw.grid, w->coarse_level, w->low_resolution))
        return fail(ctx, CSM_ENOENT, "level %d does not hold box-max(%d)", w->coarse_level, w->low_resolution);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t hn = (size_t)w->n_theta * w->n_points;
    if ((rc = reserve(ctx, ctx->pk_hits, hn * 8))) return rc;
    pw.hit_off = 0;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->pk_hits.p, hit_col, hn * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->pk_hits.as<int32_t>() + hn, hit_row, hn * 4, hipMemcpyHostToDevice, ctx->stream));
    PeakChunk ch;
    if ((rc = peaks_select_chunk(ctx, wins, 0, 1, u.sel, &ch)) || (rc = u.body(wins, 0, 1, ch)))
        (void)hipStreamSynchronize(ctx->stream);    /* no copy from the caller's arrays stays pending */
    return rc;
}

int volume_batch(csm_ctx* ctx, const VolumeUnit& u, const csm_loop_query* queries, int n,
                 const csm_correlative_params* prm, double t0_us, std::vector<csm_summary>& head, double* setup_us,
                 double* opt_us)
{
    int rc;
    std::vector<PeakWindow> wins;
    if ((rc = peaks_prepare_queries(ctx, queries, n, prm, u.scratch_limit, wins, head))) return rc;
    for (int i = 0; u.check && i < n; ++i)
        if ((rc = u.check(wins[i], i))) return rc;
    const double t1_us = clock_us();
    for (int lo = 0, hi; lo < n; lo = hi) {
        hi = peaks_next_chunk(wins, lo, u.scratch_limit);
        PeakChunk ch;
        if ((rc = peaks_project_chunk(ctx, queries, wins, head, lo, hi))) return rc;
        if ((rc = peaks_select_chunk(ctx, wins, lo, hi, u.sel, &ch))) return rc;
        if ((rc = u.body(wins, lo, hi, ch))) return rc;
    }
    *setup_us = (t1_us - t0_us) / n;
    *opt_us = (clock_us() - t1_us) / n;
    return CSM_OK;
}

void fill_summary(csm_summary& o, const csm_summary& head, const csm_result& raw, bool found,
                  const double rel_pose[3], double setup_us, double opt_us)
{
    o = head;
    o.input_setup_us = setup_us;
    o.optimization_us = opt_us;
    if (!found)
        return;
    o.raw = raw;
    o.pose_found = o.raw.found;
    o.best_sensor_pose[0] = o.sensor_pose[0] + o.raw.best_x * o.step_x;
    o.best_sensor_pose[1] = o.sensor_pose[1] + o.raw.best_y * o.step_y;
    o.best_sensor_pose[2] = o.sensor_pose[2] + o.raw.best_theta * o.step_theta;
    csm_host_move_backward(o.best_sensor_pose, rel_pose, o.estimated_pose);
}

csm_loop_query single_query(uint64_t map_id, const csm_geometry* geom, const csm_scan* scan,
                            const double initial_pose[3])
{
    csm_loop_query q;
    std::memset(&q, 0, sizeof(q));
    q.map_id = map_id;
    q.geometry = *geom;
    q.scan = *scan;
    for (int k = 0; k < 3; ++k)
        q.initial_pose[k] = initial_pose[k];
    return q;
}

} /* namespace csm_host */

namespace {

int peaks_batch(csm_ctx* ctx, const csm_loop_query* queries, int n, const csm_correlative_params* prm,
                const csm_peaks_params* pk, csm_summary* out, int32_t* n_peaks)
{
    const double t0 = clock_us();
    const int k_max = pk->k_max;
    std::vector<csm_summary> head;
    std::vector<csm_result> rec((size_t)n * k_max);
    double setup, opt;
    if (int rc = volume_batch(ctx, peaks_unit(ctx, pk, rec.data(), n_peaks), queries, n, prm, t0, head, &setup, &opt))
        return rc;
    std::memset(out, 0, sizeof(csm_summary) * (size_t)n * k_max);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n_peaks[i]; ++j)
            fill_summary(out[(size_t)i * k_max + j], head[i], rec[(size_t)i * k_max + j], true,
                         queries[i].scan.relative_sensor_pose, setup, opt);
    return CSM_OK;
}

} /* namespace */

extern "C" {

int csm_score_window_peaks(csm_ctx* ctx, uint64_t map_id, const csm_window* w, const int32_t* hit_col,
                           const int32_t* hit_row, const csm_peaks_params* pk, csm_result* out, int32_t* n_peaks)
{
    if (!ctx || !w || !hit_col || !hit_row || !out || !n_peaks)
        return fail(ctx, CSM_EINVAL, "csm_score_window_peaks: bad arguments");
    if (int rc = check_params(ctx, pk, "csm_score_window_peaks"))
        return rc;
    return volume_window(ctx, peaks_unit(ctx, pk, out, n_peaks), map_id, w, hit_col, hit_row);
}

int csm_correlative_peaks_batch(csm_ctx* ctx, const csm_loop_query* queries, int32_t n_queries,
                                const csm_correlative_params* prm, const csm_peaks_params* pk, csm_summary* out,
                                int32_t* n_peaks)
{
    if (!ctx || !queries || n_queries < 1 || !prm || !out || !n_peaks || prm->low_resolution < 1)
        return fail(ctx, CSM_EINVAL, "csm_correlative_peaks_batch: bad arguments");
    if (int rc = check_params(ctx, pk, "csm_correlative_peaks_batch"))
        return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return peaks_batch(ctx, queries, n_queries, prm, pk, out, n_peaks);
}

int csm_correlative_peaks(csm_ctx* ctx, uint64_t map_id, const csm_geometry* geom, const csm_scan* scan,
                          const double initial_pose[3], const csm_correlative_params* prm,
                          const csm_peaks_params* pk, csm_summary* out, int32_t* n_peaks)
{
    if (!ctx || !geom || !scan || !initial_pose || !prm || !out || !n_peaks || prm->low_resolution < 1)
        return fail(ctx, CSM_EINVAL, "csm_correlative_peaks: bad arguments");
    if (int rc = check_params(ctx, pk, "csm_correlative_peaks"))
        return rc;
    const csm_loop_query q = single_query(map_id, geom, scan, initial_pose);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return peaks_batch(ctx, &q, 1, prm, pk, out, n_peaks);
}

} /* extern "C" */
