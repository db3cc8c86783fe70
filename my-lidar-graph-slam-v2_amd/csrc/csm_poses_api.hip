/* csm_poses_api.hip -- a scan scored at the poses of a set (csm_score_pose_sets), the measurement update of
 * a particle set (csm_pose_set_update) and the host restatements csm_host_score_poses /
 * csm_host_score_from_sums / csm_host_pose_set_update (include/csm_hip.h), with their kernels
 * (csm_poses_kernels.hip). A translation unit of libcsm_hip.so of its own.
 *
 * A call is checked first (every set, every map: a refused call has run nothing). Then: one upload ([jobs]
 * [prefixes][angles][ranges][poses], and the weight table of an update, from ps_pin into ps_tab),
 * k_pose_prep over the beams of the distinct scans, k_pose_score over all sets, one read-back of the
 * count of marked poses. If there are any: their list is fetched, the host projects exactly those poses
 * with glibc (csm_host_project) and k_pose_rescore scores them from the host's indices, in batches of at
 * most kFixBatchBytes of indices. An update queues k_pose_weights and k_pose_resample behind that. One
 * read-back of [counters][records][weights][ancestors][update record] ends the call. Nothing the context
 * keeps between calls is touched but these workspaces. */
#include "csm_matchers.hpp"     /* kKeyToScore */

#include "csm_poses_kernels.hip"

namespace {

constexpr double kPoseMaxCell = 1073741824.0;                 /* 2^30 */
constexpr int    kPoseMaxPoints = 65536;                      /* S = sum of n_points values <= 65535 fits uint32 */
constexpr long long kPoseMaxCallPoses = 1ll << 30;
constexpr size_t kFixBatchBytes = 64u << 20;
constexpr int    kPoseGroupsWanted = 2048;                    /* workgroups of k_pose_score a call aims at */

/* What both the device entry and the host restatement refuse about a set. ang_max: max |a_i|. */
bool pose_set_ok(const csm_geometry* geom, const csm_scan* scan, const double* poses, int n_poses, double* ang_max)
{
    if (!geom || !scan || n_poses < 0 || (n_poses > 0 && !poses) || scan->n_points < 1 ||
        scan->n_points > kPoseMaxPoints || !scan->angles || !scan->ranges)
        return false;
    if (!geometry_is_finite(geom))
        return false;
    const double res = geom->resolution;
    double r_max = 0.0, a_max = 0.0;
    for (int i = 0; i < scan->n_points; ++i) {
        if (!std::isfinite(scan->angles[i]) || !std::isfinite(scan->ranges[i]))
            return false;
        r_max = std::max(r_max, std::fabs(scan->ranges[i]));
        a_max = std::max(a_max, std::fabs(scan->angles[i]));
    }
    for (int p = 0; p < n_poses; ++p) {
        const double* q = poses + 3 * (size_t)p;
        if (!std::isfinite(q[0]) || !std::isfinite(q[1]) || !std::isfinite(q[2]))
            return false;
        if (!((std::fabs(q[0] - geom->offset_x) + r_max) / res < kPoseMaxCell) ||
            !((std::fabs(q[1] - geom->offset_y) + r_max) / res < kPoseMaxCell))
            return false;
    }
    if (ang_max)
        *ang_max = a_max;
    return true;
}

bool update_params_ok(const csm_pose_update_params* p, int n_poses, int n_points, uint32_t* table, int32_t* shift)
{
    if (!p || n_poses < 0 || n_poses > CSM_POSE_SET_MAX_POSES || p->n_out < 0 || p->n_out > CSM_POSE_SET_MAX_POSES ||
        std::isnan(p->known_rate_threshold) || n_points < 1)
        return false;
    return csm_host_volume_weights(n_points, p->temperature, table, shift) == CSM_OK;
}

/* Scores the sets; with `prm`, sets[0] is the one set of an update. */
int run_sets(csm_ctx* ctx, const csm_pose_set* sets, int n_sets, csm_pose_record* out, csm_pose_sets_info* info,
             const csm_pose_update_params* prm, uint32_t* weights, int32_t* ancestors, csm_pose_update_info* update)
{
    std::vector<double> ang_max((size_t)std::max(n_sets, 1), 0.0);
    long long total_ll = 0;
    for (int k = 0; k < n_sets; ++k) {
        const csm_pose_set& s = sets[k];
        if (!pose_set_ok(&s.geometry, &s.scan, s.poses, s.n_poses, &ang_max[k]))
            return fail(ctx, CSM_EINVAL, "pose set %d: needs n_poses >= 0, 1 <= n_points <= %d, finite poses, angles, "
                        "ranges and geometry, a resolution > 0, and cell coordinates below 2^30", k, kPoseMaxPoints);
        const DeviceGrid* g = find_grid(ctx, s.map_id);
        if (!g || g->levels.empty())
            return fail(ctx, CSM_ENOENT, "pose set %d: map %llu is not resident", k, (unsigned long long)s.map_id);
        total_ll += s.n_poses;
    }
    if (total_ll >= kPoseMaxCallPoses)
        return fail(ctx, CSM_EINVAL, "pose sets: %lld poses in one call (the limit is 2^30)", total_ll);
    uint32_t table[CSM_VOLUME_BINS];
    int32_t bin_shift = 0;
    if (prm && !update_params_ok(prm, sets[0].n_poses, sets[0].scan.n_points, table, &bin_shift))
        return fail(ctx, CSM_EINVAL, "pose set update: n_poses and n_out in 0..%d, a threshold that is a number and "
                    "a temperature csm_host_volume_weights accepts", CSM_POSE_SET_MAX_POSES);
    const int total = (int)total_ll;
    const int n_out = prm ? prm->n_out : 0;
    if (info) {
        std::memset(info, 0, sizeof(*info));
        info->poses = total;
    }
    if (update) {
        std::memset(update, 0, sizeof(*update));
        update->best_index = -1;
        update->bin_shift = bin_shift;
    }
    if (total == 0) {                        /* nothing to launch; an update of no pose finds nothing */
        for (int j = 0; j < n_out; ++j)
            ancestors[j] = -1;
        return CSM_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    /* the distinct scans of the call, in first-use order */
    ScanTable scans;
    std::vector<long long> trip_at((size_t)n_sets);
    for (int k = 0; k < n_sets; ++k)
        trip_at[k] = scans.slot(sets[k].scan, k);
    const int nb = (int)scans.beams;     /* <= n_sets * 65536; n_sets is an int32 of sets that each hold a pose list */
    if (scans.beams >= (1ll << 30))
        return fail(ctx, CSM_EINVAL, "pose sets: %lld beams of distinct scans in one call (the limit is 2^30)",
                    scans.beams);

    /* poses per workgroup: as many as keep about kPoseGroupsWanted workgroups in flight, a multiple of the
     * wavefronts of a workgroup, 4 .. kPoseGroupMax (more poses per staged scan gained nothing: DESIGN 4k) */
    int group_poses = std::min(kPoseGroupMax, std::max(4, total / kPoseGroupsWanted));
    group_poses = group_poses / 4 * 4;

    /* upload block: [jobs][pre_group][angles][ranges][poses][table] */
    Carve up;
    up.take((size_t)n_sets * sizeof(PoseJob));
    const size_t pre_at = up.take(((size_t)n_sets + 1) * 4);
    const size_t angles_at = up.take((size_t)nb * 8), ranges_at = up.take((size_t)nb * 8);
    const size_t poses_at = up.take((size_t)total * 24), table_at = up.off;
    const size_t table_bytes = prm ? sizeof(table) : 0, up_bytes = table_at + table_bytes;
    /* work block: [counters + list] | [records][weights][ancestors][update record] | [triples][prefix sums];
     * a piece a plain scoring call does not have is a take(0), which advances nothing */
    const size_t rec_bytes = (size_t)total * sizeof(csm_pose_record);
    const size_t w_bytes = prm ? (size_t)total * 4 : 0, upd_bytes = prm ? sizeof(csm_pose_update_info) : 0;
    Carve wk;
    wk.take(((size_t)total + 2) * 4);
    const size_t records_at = wk.take(rec_bytes);
    const size_t w_at = wk.take(w_bytes), anc_at = wk.take(prm ? (size_t)n_out * 4 : 0);
    const size_t upd_at = wk.take(upd_bytes), back_bytes = upd_at + upd_bytes;
    const size_t trips_at = wk.take((size_t)nb * sizeof(PoseTriple)), prefix_at = wk.off;
    const size_t work_bytes = prefix_at + (prm ? (size_t)total * 8 : 0);
    int rc, e;
    if ((rc = reserve(ctx, ctx->ps_tab, up_bytes))) return rc;
    if ((rc = reserve(ctx, ctx->ps_work, work_bytes))) return rc;
    if ((rc = reserve(ctx, ctx->ps_pin, up_bytes))) return rc;
    if ((rc = reserve(ctx, ctx->ps_back, back_bytes))) return rc;
    char* const pin = ctx->ps_pin.as<char>();
    char* const tab = ctx->ps_tab.as<char>();
    char* const work = ctx->ps_work.as<char>();
    char* const back = ctx->ps_back.as<char>();

    std::vector<PoseJob> jobs((size_t)n_sets);
    std::vector<uint32_t> pre_group((size_t)n_sets + 1, 0u), pre_pose((size_t)n_sets + 1, 0u);
    for (int k = 0; k < n_sets; ++k) {
        const csm_pose_set& s = sets[k];
        const DeviceGrid& g = *find_grid(ctx, s.map_id);
        PoseJob& J = jobs[k];
        J.cells = g.levels[0].cells;
        J.rows = g.rows;
        J.cols = g.cols;
        J.pitch = g.pitch;
        J.n_points = s.scan.n_points;
        J.trip_at = trip_at[k];
        J.pose_at = pre_pose[k];
        J.n_poses = s.n_poses;
        J.pad = 0;
        J.off_x = s.geometry.offset_x;
        J.off_y = s.geometry.offset_y;
        J.inv_res = 1.0 / s.geometry.resolution;
        J.ang_max = ang_max[k];
        pre_pose[k + 1] = pre_pose[k] + (uint32_t)s.n_poses;
        pre_group[k + 1] = pre_group[k] + (uint32_t)ceil_div(s.n_poses, group_poses);
    }
    std::memcpy(pin, jobs.data(), (size_t)n_sets * sizeof(PoseJob));
    std::memcpy(pin + pre_at, pre_group.data(), ((size_t)n_sets + 1) * 4);
    double* const angles_pin = reinterpret_cast<double*>(pin + angles_at);
    double* const ranges_pin = reinterpret_cast<double*>(pin + ranges_at);
    double* const poses_pin = reinterpret_cast<double*>(pin + poses_at);
    for (int k : scans.first_use) {
        const csm_scan& sc = sets[k].scan;
        std::memcpy(angles_pin + trip_at[k], sc.angles, (size_t)sc.n_points * 8);
        std::memcpy(ranges_pin + trip_at[k], sc.ranges, (size_t)sc.n_points * 8);
    }
    for (int k = 0; k < n_sets; ++k)
        if (sets[k].n_poses)
            std::memcpy(poses_pin + 3 * (size_t)pre_pose[k], sets[k].poses, (size_t)sets[k].n_poses * 24);
    if (prm)
        std::memcpy(pin + table_at, table, table_bytes);

    PoseChunk ch;
    ch.jobs = reinterpret_cast<const PoseJob*>(tab);
    ch.pre_group = reinterpret_cast<const uint32_t*>(tab + pre_at);
    ch.angles = reinterpret_cast<const double*>(tab + angles_at);
    ch.ranges = reinterpret_cast<const double*>(tab + ranges_at);
    ch.poses = reinterpret_cast<const double*>(tab + poses_at);
    ch.trips = reinterpret_cast<PoseTriple*>(work + trips_at);
    ch.records = reinterpret_cast<csm_pose_record*>(work + records_at);
    ch.unc = reinterpret_cast<uint32_t*>(work);
    ch.n_sets = n_sets;
    ch.n_beams = nb;
    ch.group_poses = group_poses;
    ch.pad = 0;

    CallSpan span(ctx);
    if (!span.a || !span.b)
        return fail(ctx, CSM_EIO, "pose sets: hipEventCreate failed");
    HIP_TRY(ctx, hipMemcpyAsync(tab, pin, up_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(work, 0, 8, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(span.a, ctx->stream));
    {
        ScopedTimer tm(ctx, "pose_prep");
        e = launch(k_pose_prep, dim3((unsigned)ceil_div(nb, kPoseBlock)), dim3(kPoseBlock), ctx->stream, ch);
    }
    if ((rc = launched_ok(ctx, e, "pose prep"))) return rc;
    {
        ScopedTimer tm(ctx, "pose_score");
        e = launch(k_pose_score, dim3(pre_group[n_sets]), dim3(kPoseBlock), ctx->stream, ch);
    }
    if ((rc = launched_ok(ctx, e, "pose score"))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(back, work, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t n_unc = reinterpret_cast<const uint32_t*>(back)[0];
    if (n_unc > (uint32_t)total)
        return fail(ctx, CSM_EIO, "internal: %u poses marked of %d", n_unc, total);

    double host_us = 0.0;
    if (n_unc > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(back + 8, work + 8, (size_t)n_unc * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const std::vector<uint32_t> list(reinterpret_cast<const uint32_t*>(back) + 2,
                                         reinterpret_cast<const uint32_t*>(back) + 2 + n_unc);
        /* ps_pin's upload block has been consumed (the stream has drained): it stages the batches now */
        for (uint32_t u0 = 0; u0 < n_unc;) {
            std::vector<PoseFix> fixes;
            size_t ints = 0;
            uint32_t u1 = u0;
            while (u1 < n_unc) {
                const uint32_t pose = list[u1];
                const int k = (int)(std::upper_bound(pre_pose.begin(), pre_pose.end(), pose) - pre_pose.begin()) - 1;
                const size_t need = 2 * (size_t)sets[k].scan.n_points;
                if (u1 > u0 && (ints + need) * 4 > kFixBatchBytes)
                    break;
                fixes.push_back({ pose, k, (long long)ints });
                ints += need;
                ++u1;
            }
            /* fix batch: [fixes][hit indices] */
            const size_t fix_bytes = align256(fixes.size() * sizeof(PoseFix));
            const size_t batch_bytes = fix_bytes + ints * 4;
            if ((rc = reserve(ctx, ctx->ps_pin, batch_bytes))) return rc;
            if ((rc = reserve(ctx, ctx->ps_fix, batch_bytes))) return rc;
            char* const fpin = ctx->ps_pin.as<char>();
            char* const fdev = ctx->ps_fix.as<char>();
            std::memcpy(fpin, fixes.data(), fixes.size() * sizeof(PoseFix));
            int32_t* const hits = reinterpret_cast<int32_t*>(fpin + fix_bytes);
            const double t0 = clock_us();
            for (const PoseFix& f : fixes) {
                const csm_pose_set& s = sets[f.set];
                const double* const pose = s.poses + 3 * (size_t)(f.pose - pre_pose[f.set]);
                csm_host_project(&s.geometry, pose, 0.0, 0, s.scan.angles, s.scan.ranges, s.scan.n_points,
                                 hits + f.hit_at, hits + f.hit_at + s.scan.n_points, nullptr, nullptr);
            }
            host_us += clock_us() - t0;
            HIP_TRY(ctx, hipMemcpyAsync(fdev, fpin, batch_bytes, hipMemcpyHostToDevice, ctx->stream));
            {
                ScopedTimer tm(ctx, "pose_rescore");
                const dim3 fix_groups((unsigned)ceil_div((int)fixes.size(), kPoseBlock / 64));
                e = launch(k_pose_rescore, fix_groups, dim3(kPoseBlock), ctx->stream, ch,
                           reinterpret_cast<const PoseFix*>(fdev), reinterpret_cast<const int32_t*>(fdev + fix_bytes),
                           (int)fixes.size());
            }
            if ((rc = launched_ok(ctx, e, "pose rescore"))) return rc;
            u0 = u1;
            if (u0 < n_unc)
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     /* the next batch is staged in the same block */
        }
    }
    if (prm) {
        PoseUpdate pu;
        pu.records = ch.records;
        pu.table = reinterpret_cast<const uint32_t*>(tab + table_at);
        pu.weights = reinterpret_cast<uint32_t*>(work + w_at);
        pu.prefix = reinterpret_cast<unsigned long long*>(work + prefix_at);
        pu.ancestors = reinterpret_cast<int32_t*>(work + anc_at);
        pu.info = reinterpret_cast<csm_pose_update_info*>(work + upd_at);
        pu.n_poses = total;
        pu.n_out = n_out;
        pu.min_known = csm_host_min_known(sets[0].scan.n_points, prm->known_rate_threshold);
        pu.bin_shift = bin_shift;
        pu.offset = prm->offset;
        {
            ScopedTimer tm(ctx, "pose_weights");
            e = launch(k_pose_weights, dim3(1), dim3(kPoseUpdateBlock), ctx->stream, pu);
        }
        if ((rc = launched_ok(ctx, e, "pose weights"))) return rc;
        if (n_out > 0) {
            ScopedTimer tm(ctx, "pose_resample");
            e = launch(k_pose_resample, dim3((unsigned)ceil_div(n_out, kPoseBlock)), dim3(kPoseBlock), ctx->stream, pu);
            if ((rc = launched_ok(ctx, e, "pose resample"))) return rc;
        }
    }
    HIP_TRY(ctx, hipEventRecord(span.b, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(back, work, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(back + records_at, work + records_at, back_bytes - records_at, hipMemcpyDeviceToHost,
                                ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(out, back + records_at, rec_bytes);
    if (prm) {
        std::memcpy(weights, back + w_at, w_bytes);
        if (n_out)
            std::memcpy(ancestors, back + anc_at, (size_t)n_out * 4);
        if (update)
            std::memcpy(update, back + upd_at, upd_bytes);
    }
    if (info) {
        float ms = 0.0f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, span.a, span.b));
        info->uncertain_poses = (int32_t)n_unc;
        info->changed_poses = (int32_t)reinterpret_cast<const uint32_t*>(back)[1];
        info->host_us = host_us;
        info->device_us = 1e3 * (double)ms;
    }
    return CSM_OK;
}

} /* namespace */

extern "C" {

int csm_host_score_poses(const uint16_t* grid, int32_t rows, int32_t cols, const csm_geometry* geom,
                         const csm_scan* scan, const double* poses, int32_t n_poses, csm_pose_record* out)
{
    if (!grid || rows < 1 || cols < 1 || (n_poses > 0 && !out) || !pose_set_ok(geom, scan, poses, n_poses, nullptr))
        return CSM_EINVAL;
    const int n = scan->n_points;
    std::vector<int32_t> col((size_t)n), row((size_t)n);
    for (int p = 0; p < n_poses; ++p) {
        csm_host_project(geom, poses + 3 * (size_t)p, 0.0, 0, scan->angles, scan->ranges, n, col.data(), row.data(),
                         nullptr, nullptr);
        uint32_t s = 0, k = 0;
        for (int i = 0; i < n; ++i) {
            if (col[i] < 0 || col[i] >= cols || row[i] < 0 || row[i] >= rows)
                continue;
            const uint32_t v = grid[(size_t)row[i] * cols + col[i]];
            s += v;
            k += v != 0u;
        }
        out[p] = { s, k, 0u, 0u };
    }
    return CSM_OK;
}

int csm_host_score_from_sums(uint32_t sum_values, uint32_t known, int32_t n_points, double* score, double* known_rate)
{
    if (n_points < 1 || !score || !known_rate)
        return CSM_EINVAL;
    const uint64_t key = 32268ull * known + 499ull * sum_values;
    *score = ((double)key * kKeyToScore) / (double)n_points;
    *known_rate = (double)known / (double)n_points;
    return CSM_OK;
}

int csm_host_pose_set_update(const csm_pose_record* records, int32_t n_poses, int32_t n_points,
                             const csm_pose_update_params* prm, uint32_t* weights, int32_t* ancestors,
                             csm_pose_update_info* update)
{
    uint32_t table[CSM_VOLUME_BINS];
    int32_t shift = 0;
    if (!update || !update_params_ok(prm, n_poses, n_points, table, &shift) || (n_poses > 0 && (!records || !weights)) ||
        (prm->n_out > 0 && !ancestors))
        return CSM_EINVAL;
    const int min_known = csm_host_min_known(n_points, prm->known_rate_threshold);
    auto key_of = [](const csm_pose_record& r) { return 32268ull * r.known + 499ull * r.sum_values; };
    std::memset(update, 0, sizeof(*update));
    update->best_index = -1;
    update->bin_shift = shift;
    for (int i = 0; i < n_poses; ++i) {
        if ((int64_t)records[i].known < min_known)
            continue;
        const uint64_t key = key_of(records[i]);
        if (!update->found || key > update->key_max) {
            update->found = 1;
            update->key_max = key;
            update->best_index = i;
        }
    }
    std::vector<uint64_t> prefix((size_t)n_poses);
    uint64_t m0 = 0;
    for (int i = 0; i < n_poses; ++i) {
        uint32_t w = 0;
        if (update->found && (int64_t)records[i].known >= min_known) {
            const uint64_t bin = (update->key_max - key_of(records[i])) >> shift;
            w = bin < (uint64_t)CSM_VOLUME_BINS ? table[bin] : 0u;
        }
        weights[i] = w;
        update->support += w != 0u;
        m0 += w;
        prefix[i] = m0;
    }
    update->m0 = m0;
    for (int j = 0; j < prm->n_out; ++j) {
        if (!update->found || m0 == 0) {
            ancestors[j] = -1;
            continue;
        }
        const uint64_t T = ((uint64_t)j * m0 + prm->offset % m0) / (uint64_t)prm->n_out;
        ancestors[j] = (int32_t)(std::upper_bound(prefix.begin(), prefix.end(), T) - prefix.begin());
    }
    return CSM_OK;
}

int csm_score_pose_sets(csm_ctx* ctx, const csm_pose_set* sets, int32_t n_sets, csm_pose_record* out,
                        csm_pose_sets_info* info)
{
    if (!ctx || n_sets < 0 || (n_sets > 0 && !sets))
        return fail(ctx, CSM_EINVAL, "csm_score_pose_sets: bad arguments");
    long long total = 0;
    for (int k = 0; k < n_sets; ++k)
        total += std::max(sets[k].n_poses, 0);
    if (total > 0 && !out)
        return fail(ctx, CSM_EINVAL, "csm_score_pose_sets: no room for the records");
    return run_sets(ctx, sets, n_sets, out, info, nullptr, nullptr, nullptr, nullptr);
}

int csm_pose_set_update(csm_ctx* ctx, const csm_pose_set* set, const csm_pose_update_params* prm,
                        csm_pose_record* records, uint32_t* weights, int32_t* ancestors,
                        csm_pose_update_info* update, csm_pose_sets_info* info)
{
    if (!ctx || !set || !prm || !update || (set->n_poses > 0 && (!records || !weights)) ||
        (prm->n_out > 0 && !ancestors))
        return fail(ctx, CSM_EINVAL, "csm_pose_set_update: bad arguments");
    return run_sets(ctx, set, 1, records, info, prm, weights, ancestors, update);
}

} /* extern "C" */
