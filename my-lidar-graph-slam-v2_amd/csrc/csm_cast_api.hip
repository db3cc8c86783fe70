/* csm_cast_api.hip -- virtual scans: csm_ray_cast and the host restatements csm_host_ray_cast,
 * csm_host_ray_cast_min_dist2, csm_host_ray_cast_ranges (include/csm_hip.h), with their kernels
 * (csm_cast_kernels.hip). A translation unit of libcsm_hip.so of its own; what it shares with the ray check
 * (csm_ray_api.hip) is csm_ray.hpp.
 *
 * A call is checked first (every set, every pose, every map: a refused call has run nothing) and then cut into
 * chunks of consecutive poses; a chunk holds segments, each the poses of one set that fall into it. Per chunk:
 * one upload ([segments][prefixes][poses][the distinct scans], from the pinned block into the table),
 * k_cast_project over all rays, one small read-back (the uncertified rays), their records from glibc scattered
 * in by k_cast_patch, k_cast_walk, one read-back of [records][workgroup counters]. Nothing the context keeps
 * between calls is touched but the ray check's workspaces, which the two entries share (both run to their end
 * on the context's stream before they return). */
#include "csm_internal.hpp"

#include "csm_cast_kernels.hip"

static_assert(sizeof(csm_ray_cast_record) == kCastRecordBytes && sizeof(CastRecord) == kCastRecordBytes &&
              offsetof(csm_ray_cast_record, value) == offsetof(CastRecord, value) &&
              offsetof(csm_ray_cast_record, kind) == offsetof(CastRecord, kind) &&
              offsetof(csm_ray_cast_record, dist2) == offsetof(CastRecord, dist2),
              "k_cast_walk writes csm_ray_cast_record");

namespace {

constexpr int64_t kCastMaxM = 1ll << 31;             /* m of min_dist2 = m^2: above every |D| */

bool cast_params_ok(const csm_ray_cast_params* p)
{
    return p && p->subpixel_scale >= 1 && p->subpixel_scale <= CSM_RAY_CHECK_MAX_SCALE && p->occupied_min >= 1u &&
           p->occupied_min <= 65535u && (p->unknown_stops == 0 || p->unknown_stops == 1) &&
           p->scratch_limit_bytes >= 0 && std::isfinite(p->range_max) && p->range_max > 0.0 && p->range_min >= 0.0;
}

int64_t cast_min_dist2(double range_min, double resolution, int scale)
{
    const double m = std::ceil(2.0 * range_min / (resolution / scale));
    const int64_t mi = m < (double)kCastMaxM ? (int64_t)m : kCastMaxM;
    return mi * mi;
}

/* geometry, scan and poses of a set as the cast reads them; s [n_poses][2] receives the sensors' sub-pixel
 * indices. false: refused */
bool cast_set_ok(const csm_geometry* geom, const csm_scan* scan, const double* poses, int32_t n_poses,
                 const csm_ray_cast_params* p, int32_t* s)
{
    if (!geom || !scan || scan->n_points < 0 || n_poses < 0 || (scan->n_points > 0 && !scan->angles) ||
        (n_poses > 0 && !poses) || !geometry_is_finite(geom))
        return false;
    for (int i = 0; i < scan->n_points; ++i)
        if (!std::isfinite(scan->angles[i]))
            return false;
    for (int k = 0; k < n_poses; ++k) {
        const double* S = poses + 3 * (size_t)k;
        if (!std::isfinite(S[0]) || !std::isfinite(S[1]) || !std::isfinite(S[2]) ||
            !ray_frame(geom, S, p->range_max, p->subpixel_scale, s + 2 * (size_t)k))
            return false;
    }
    return true;
}

/* beam i of a scan: false if it is not cast, else its limit */
bool cast_limit(const csm_scan* scan, int i, double range_max, double* limit)
{
    if (!scan->ranges) {
        *limit = range_max;
        return true;
    }
    const double r = scan->ranges[i];
    if (!(r > 0.0))
        return false;
    *limit = r < range_max ? r : range_max;
    return true;
}

/* the end point of a cast beam as glibc gives it (kRayUnusable: not cast); the cast does not use H */
RayRec cast_host_rec(const double S[3], const csm_geometry* geom, double scaled_res, const csm_scan* scan, int i,
                     double range_max)
{
    RayRec rec = { kRayUnusable, 0, 0, 0 };
    double limit;
    if (cast_limit(scan, i, range_max, &limit)) {
        rec = ray_host_rec(S, geom, scaled_res, limit, scan->angles[i]);
        rec.hx = rec.hy = 0;
    }
    return rec;
}

/* Chunks of consecutive poses: a pose of n beams counts 48 n + 64 bytes. */
int64_t cast_pose_bytes(int n) { return 48ll * n + 64; }

struct CastPart {              /* a segment on the host */
    int set, pose0, n_poses;
};

} /* namespace */

extern "C" {

int csm_host_ray_cast_min_dist2(double range_min, double resolution, int32_t subpixel_scale, int64_t* min_dist2)
{
    if (!min_dist2 || !(range_min >= 0.0) || !std::isfinite(resolution) || !(resolution > 0.0) ||
        subpixel_scale < 1 || subpixel_scale > CSM_RAY_CHECK_MAX_SCALE)
        return CSM_EINVAL;
    *min_dist2 = cast_min_dist2(range_min, resolution, subpixel_scale);
    return CSM_OK;
}

int csm_host_ray_cast_ranges(const csm_ray_cast_record* records, int64_t n, double resolution,
                             int32_t subpixel_scale, double none_value, double* ranges)
{
    if (n < 0 || (n > 0 && (!records || !ranges)) || !std::isfinite(resolution) || !(resolution > 0.0) ||
        subpixel_scale < 1 || subpixel_scale > CSM_RAY_CHECK_MAX_SCALE)
        return CSM_EINVAL;
    const double half = 0.5 * (resolution / subpixel_scale);
    for (int64_t k = 0; k < n; ++k)
        ranges[k] = records[k].kind != CSM_CAST_NONE ? half * std::sqrt((double)records[k].dist2) : none_value;
    return CSM_OK;
}

int csm_host_ray_cast(const uint16_t* grid, int32_t rows, int32_t cols, const csm_geometry* geom,
                      const csm_scan* scan, const double* poses, int32_t n_poses,
                      const csm_ray_cast_params* prm, csm_ray_cast_record* records)
{
    if (!grid || rows < 1 || cols < 1 || !cast_params_ok(prm))
        return CSM_EINVAL;
    std::vector<int32_t> s(2 * (size_t)std::max(n_poses, 0));
    if (!cast_set_ok(geom, scan, poses, n_poses, prm, s.data()) ||
        (!records && n_poses > 0 && scan->n_points > 0))
        return CSM_EINVAL;
    const int scale = prm->subpixel_scale;
    const double scaled_res = geom->resolution / scale;
    const int64_t min_dist2 = cast_min_dist2(prm->range_min, geom->resolution, scale);
    std::vector<Cell> walk;
    for (int k = 0; k < n_poses; ++k) {
        const double* S = poses + 3 * (size_t)k;
        const int sx = s[2 * (size_t)k], sy = s[2 * (size_t)k + 1];
        const Cell sensor(host_floor_div(sx, scale), host_floor_div(sy, scale));
        for (int i = 0; i < scan->n_points; ++i) {
            csm_ray_cast_record out;
            std::memset(&out, 0, sizeof(out));
            const RayRec rec = cast_host_rec(S, geom, scaled_res, scan, i, prm->range_max);
            if (rec.ex != kRayUnusable) {
                const int bx = host_floor_div(std::min(sx, rec.ex), scale), by = host_floor_div(std::min(sy, rec.ey), scale);
                ray_step_cells(sx - bx * scale, sy - by * scale, rec.ex - bx * scale, rec.ey - by * scale, scale, walk);
                /* from the sensor's end */
                if (Cell(walk.front().first + bx, walk.front().second + by) != sensor)
                    std::reverse(walk.begin(), walk.end());
                for (const Cell& c : walk) {
                    const int x = c.first + bx, y = c.second + by;
                    if (x < 0 || x >= cols || y < 0 || y >= rows)
                        continue;
                    const int64_t dx = 2ll * x * scale + scale - 2ll * sx - 1, dy = 2ll * y * scale + scale - 2ll * sy - 1;
                    const int64_t d2 = dx * dx + dy * dy;
                    if (d2 < min_dist2)
                        continue;
                    const uint32_t v = grid[(size_t)y * cols + x];
                    const int kind = v >= prm->occupied_min ? CSM_CAST_OCCUPIED
                                     : (prm->unknown_stops && v == 0) ? CSM_CAST_UNKNOWN : CSM_CAST_NONE;
                    if (kind != CSM_CAST_NONE) {
                        out.cell_x = x;
                        out.cell_y = y;
                        out.value = v;
                        out.kind = kind;
                        out.dist2 = d2;
                        break;
                    }
                }
            }
            records[(size_t)k * scan->n_points + i] = out;
        }
    }
    return CSM_OK;
}

int csm_ray_cast(csm_ctx* ctx, const csm_pose_set* sets, int32_t n_sets, const csm_ray_cast_params* prm,
                 csm_ray_cast_record* records, csm_ray_cast_info* info)
{
    if (!ctx || n_sets < 0 || (n_sets > 0 && !sets))
        return fail(ctx, CSM_EINVAL, "csm_ray_cast: bad arguments");
    if (!cast_params_ok(prm))
        return fail(ctx, CSM_EINVAL, "ray cast: need occupied_min in 1..65535, subpixel_scale in 1..%d, unknown_stops "
                    "0 | 1, scratch_limit_bytes >= 0, a finite range_max > 0 and range_min >= 0",
                    CSM_RAY_CHECK_MAX_SCALE);
    std::vector<std::vector<int32_t>> sub((size_t)n_sets);     /* the sensors' sub-pixel indices */
    int64_t total = 0;
    for (int i = 0; i < n_sets; ++i) {
        const csm_pose_set& st = sets[i];
        if (st.n_poses >= (1 << 30))
            return fail(ctx, CSM_EINVAL, "ray cast: set %d has 2^30 or more poses", i);
        sub[i].resize(2 * (size_t)std::max(st.n_poses, 0));
        if (!cast_set_ok(&st.geometry, &st.scan, st.poses, st.n_poses, prm, sub[i].data()))
            return fail(ctx, CSM_EINVAL, "ray cast: set %d has bad angles, geometry or poses, a sensor more than 2^20 "
                        "cells from the map's origin, or range_max / resolution > 2^20", i);
        const DeviceGrid* g = find_grid(ctx, st.map_id);
        if (!g || g->levels.empty())
            return fail(ctx, CSM_ENOENT, "map %llu not resident", (unsigned long long)st.map_id);
        total += (int64_t)st.n_poses * st.scan.n_points;
    }
    if (total > 0 && !records)
        return fail(ctx, CSM_EINVAL, "csm_ray_cast: records is null");
    if (info)
        std::memset(info, 0, sizeof(*info));
    if (total == 0)
        return CSM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    const int64_t limit = prm->scratch_limit_bytes ? prm->scratch_limit_bytes : kRayDefaultScratch;
    const uint32_t unc_cap = ray_unc_cap(ctx);
    const size_t unc_bytes = align256(((size_t)unc_cap + 1) * 4);
    const int scale = prm->subpixel_scale;
    bool host_projection = ctx->tune.map_host_projection;
    int64_t rays_done = 0, host_rays = 0, cells_read = 0, cells_to_stop = 0;
    double host_us = 0.0, device_us = 0.0;
    CallSpan span(ctx, info != nullptr);
    if (info && (!span.a || !span.b))
        return fail(ctx, CSM_EIO, "ray cast: hipEventCreate failed");

    int set = 0, pose = 0;                 /* the next pose to take */
    while (set < n_sets) {
        /* the chunk: parts of consecutive sets */
        std::vector<CastPart> parts;
        int64_t bytes = 0, rays_ll = 0, poses_ll = 0;
        while (set < n_sets) {
            const csm_pose_set& st = sets[set];
            const int left = st.n_poses - pose;
            if (left <= 0 || st.scan.n_points == 0) {       /* nothing to cast: no part */
                ++set;
                pose = 0;
                continue;
            }
            const int64_t each = cast_pose_bytes(st.scan.n_points);
            int64_t fit = std::min<int64_t>((limit - bytes) / each, ((1ll << 30) - 1 - rays_ll) / st.scan.n_points);
            if (fit < 1 && parts.empty())
                fit = 1;
            if (fit < 1)
                break;
            const int take = (int)std::min<int64_t>(fit, left);
            parts.push_back({ set, pose, take });
            bytes += each * take;
            rays_ll += (int64_t)take * st.scan.n_points;
            poses_ll += take;
            pose += take;
            if (pose < st.n_poses)
                break;                                      /* the chunk is full */
            ++set;
            pose = 0;
        }
        if (parts.empty())
            break;
        const int ns = (int)parts.size(), nr = (int)rays_ll, np = (int)poses_ll;

        /* the distinct scans of the chunk, in first-use order */
        ScanTable table;
        std::vector<long long> scan_at((size_t)ns);     /* of [angles | ranges], in doubles */
        for (int k = 0; k < ns; ++k)
            scan_at[k] = 2 * table.slot(sets[parts[k].set].scan, k);

        /* upload block: [segments][pre_ray][pre_group][poses][scans]; the tables are one piece */
        Carve up;
        up.take((size_t)ns * sizeof(CastSeg) + 2 * ((size_t)ns + 1) * 4);
        const size_t poses_at = up.take((size_t)np * sizeof(CastPose)), scans_at = up.off;
        const size_t up_bytes = scans_at + 2 * (size_t)table.beams * 8;
        int rc, e;
        if ((rc = reserve(ctx, ctx->rc_tab, up_bytes))) return rc;
        /* staged first: the work block is sized by the prefixes */
        const size_t patch_bytes = std::max((size_t)unc_cap * sizeof(RayPatch), (size_t)nr * sizeof(RayRec));
        if ((rc = reserve(ctx, ctx->rc_pin, up_bytes + patch_bytes))) return rc;
        char* const pin = ctx->rc_pin.as<char>();
        char* const tab = ctx->rc_tab.as<char>();
        CastSeg* const seg_stage = reinterpret_cast<CastSeg*>(pin);
        uint32_t* const pre_ray = reinterpret_cast<uint32_t*>(pin + (size_t)ns * sizeof(CastSeg));
        uint32_t* const pre_group = pre_ray + ns + 1;
        CastPose* const P = reinterpret_cast<CastPose*>(pin + poses_at);
        double* const scans = reinterpret_cast<double*>(pin + scans_at);
        pre_ray[0] = pre_group[0] = 0;
        long long pose_at = 0;
        for (int k = 0; k < ns; ++k) {
            const csm_pose_set& st = sets[parts[k].set];
            const DeviceGrid& g = *find_grid(ctx, st.map_id);
            CastSeg& J = seg_stage[k];
            J.cells = g.levels[0].cells;
            J.rows = g.rows;
            J.cols = g.cols;
            J.pitch = g.pitch;
            J.n_beams = st.scan.n_points;
            J.angles_at = scan_at[k];
            J.ranges_at = st.scan.ranges ? scan_at[k] + st.scan.n_points : -1;
            J.pose_at = pose_at;
            J.n_poses = parts[k].n_poses;
            J.groups = ceil_div(st.scan.n_points, kCastGroup);
            J.off_x = st.geometry.offset_x;
            J.off_y = st.geometry.offset_y;
            J.res = st.geometry.resolution;
            J.scaled_res = st.geometry.resolution / scale;
            J.min_dist2 = cast_min_dist2(prm->range_min, st.geometry.resolution, scale);
            for (int p = 0; p < parts[k].n_poses; ++p) {
                const size_t at = (size_t)parts[k].pose0 + p;
                CastPose& Q = P[pose_at + p];
                Q.x = st.poses[3 * at];
                Q.y = st.poses[3 * at + 1];
                Q.theta = st.poses[3 * at + 2];
                Q.sx = sub[parts[k].set][2 * at];
                Q.sy = sub[parts[k].set][2 * at + 1];
            }
            pose_at += parts[k].n_poses;
            pre_ray[k + 1] = pre_ray[k] + (uint32_t)((int64_t)parts[k].n_poses * st.scan.n_points);
            pre_group[k + 1] = pre_group[k] + (uint32_t)((int64_t)parts[k].n_poses * J.groups);
        }
        for (int k : table.first_use) {
            const csm_scan& sc = sets[parts[k].set].scan;
            std::memcpy(scans + scan_at[k], sc.angles, (size_t)sc.n_points * 8);
            if (sc.ranges)
                std::memcpy(scans + scan_at[k] + sc.n_points, sc.ranges, (size_t)sc.n_points * 8);
            else
                std::memset(scans + scan_at[k] + sc.n_points, 0, (size_t)sc.n_points * 8);
        }
        const uint32_t n_groups = pre_group[ns];

        /* work block: [uncertified count + list][records][workgroup counters] | [ray records][patches]; what
         * goes back, list, records and counters, is one piece */
        const size_t rec_bytes = (size_t)nr * kCastRecordBytes, cnt_bytes = (size_t)n_groups * 8;
        const size_t back_bytes = unc_bytes + rec_bytes + cnt_bytes;
        Carve wk;
        wk.take(back_bytes);
        const size_t recs_at = wk.take((size_t)nr * sizeof(RayRec)), patch_at = wk.off;
        const size_t work_bytes = patch_at + (size_t)unc_cap * sizeof(RayPatch);
        if ((rc = reserve(ctx, ctx->rc_work, work_bytes))) return rc;
        if ((rc = reserve(ctx, ctx->rc_back, back_bytes))) return rc;
        char* const work = ctx->rc_work.as<char>();
        char* const back = ctx->rc_back.as<char>();

        HIP_TRY(ctx, hipMemcpyAsync(tab, pin, up_bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(work, 0, unc_bytes, ctx->stream));
        if (info)
            HIP_TRY(ctx, hipEventRecord(span.a, ctx->stream));

        CastChunk ch;
        ch.segs = reinterpret_cast<const CastSeg*>(tab);
        ch.pre_ray = reinterpret_cast<const uint32_t*>(tab + (size_t)ns * sizeof(CastSeg));
        ch.pre_group = ch.pre_ray + ns + 1;
        ch.poses = reinterpret_cast<const CastPose*>(tab + poses_at);
        ch.scans = reinterpret_cast<const double*>(tab + scans_at);
        ch.unc = reinterpret_cast<uint32_t*>(work);
        ch.records = reinterpret_cast<CastRecord*>(work + unc_bytes);
        ch.group_cells = reinterpret_cast<uint32_t*>(work + unc_bytes + rec_bytes);
        ch.recs = reinterpret_cast<RayRec*>(work + recs_at);
        ch.unc_cap = unc_cap;
        ch.n_segs = ns;
        ch.n_rays = nr;
        ch.range_max = prm->range_max;
        ch.scale = scale;
        ch.unknown_stops = prm->unknown_stops;
        ch.occupied_min = prm->occupied_min;
        ch.pad = 0;

        uint32_t n_unc = 0;
        if (!host_projection) {
            {
                ScopedTimer tm(ctx, "cast_project");
                e = launch(k_cast_project, dim3((unsigned)ceil_div(nr, 256)), dim3(256), ctx->stream, ch);
            }
            if ((rc = launched_ok(ctx, e, "cast project"))) return rc;
            HIP_TRY(ctx, hipMemcpyAsync(back, work, unc_bytes, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            n_unc = reinterpret_cast<const uint32_t*>(back)[0];
            if (n_unc > unc_cap) {
                host_projection = true;     /* too many rays on cell edges: this chunk and the rest on the host */
                n_unc = 0;
            }
        }
        char* const patch_pin = pin + up_bytes;
        auto pose_of = [&](int k, int p) { return sets[parts[k].set].poses + 3 * ((size_t)parts[k].pose0 + p); };
        if (host_projection) {
            RayRec* const all = reinterpret_cast<RayRec*>(patch_pin);
            const double t0 = clock_us();
            for (int k = 0; k < ns; ++k) {
                const csm_pose_set& st = sets[parts[k].set];
                const int n = st.scan.n_points;
                for (int p = 0; p < parts[k].n_poses; ++p)
                    for (int i = 0; i < n; ++i) {
                        const RayRec rec = cast_host_rec(pose_of(k, p), &st.geometry, seg_stage[k].scaled_res, &st.scan,
                                                         i, prm->range_max);
                        host_rays += rec.ex != kRayUnusable;
                        all[(size_t)pre_ray[k] + (size_t)p * n + i] = rec;
                    }
            }
            host_us += clock_us() - t0;
            HIP_TRY(ctx, hipMemcpyAsync(ch.recs, all, (size_t)nr * sizeof(RayRec), hipMemcpyHostToDevice, ctx->stream));
        } else if (n_unc > 0) {
            /* the rays the device could not certify: exactly as glibc has them, and patched in */
            const uint32_t* const list = reinterpret_cast<const uint32_t*>(back) + 1;
            RayPatch* const patches = reinterpret_cast<RayPatch*>(patch_pin);
            const double t0 = clock_us();
            for (uint32_t u = 0; u < n_unc; ++u) {
                const uint32_t b = list[u];
                const int k = (int)(std::upper_bound(pre_ray, pre_ray + ns + 1, b) - pre_ray) - 1;
                const csm_pose_set& st = sets[parts[k].set];
                const int local = (int)(b - pre_ray[k]);
                const int p = local / st.scan.n_points, i = local - p * st.scan.n_points;
                patches[u].beam = b;
                patches[u].rec = cast_host_rec(pose_of(k, p), &st.geometry, seg_stage[k].scaled_res, &st.scan, i,
                                               prm->range_max);
            }
            host_us += clock_us() - t0;
            host_rays += n_unc;
            RayPatch* const patches_dev = reinterpret_cast<RayPatch*>(work + patch_at);
            HIP_TRY(ctx, hipMemcpyAsync(patches_dev, patches, (size_t)n_unc * sizeof(RayPatch), hipMemcpyHostToDevice,
                                        ctx->stream));
            e = launch(k_cast_patch, dim3((unsigned)ceil_div((int)n_unc, 256)), dim3(256), ctx->stream, patches_dev,
                       (int)n_unc, ch.recs);
            if ((rc = launched_ok(ctx, e, "cast patch"))) return rc;
        }
        {
            ScopedTimer tm(ctx, "cast_walk");
            e = launch(k_cast_walk, dim3(n_groups), dim3(256), ctx->stream, ch);
        }
        if ((rc = launched_ok(ctx, e, "cast walk"))) return rc;
        if (info)
            HIP_TRY(ctx, hipEventRecord(span.b, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(back + unc_bytes, work + unc_bytes, rec_bytes + cnt_bytes, hipMemcpyDeviceToHost,
                                    ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        std::memcpy(records + rays_done, back + unc_bytes, rec_bytes);
        const uint32_t* const cnt = reinterpret_cast<const uint32_t*>(back + unc_bytes + rec_bytes);
        for (uint32_t gi = 0; gi < n_groups; ++gi) {
            cells_read += cnt[2 * (size_t)gi];
            cells_to_stop += cnt[2 * (size_t)gi + 1];
        }
        if (info) {
            float ms = 0.0f;
            HIP_TRY(ctx, hipEventElapsedTime(&ms, span.a, span.b));
            device_us += 1e3 * (double)ms;
        }
        rays_done += nr;
    }
    if (info) {
        info->rays = rays_done;
        info->host_rays = host_rays;
        info->cells_read = cells_read;
        info->cells_to_stop = cells_to_stop;
        info->host_us = host_us;
        info->device_us = device_us;
    }
    return CSM_OK;
}

} /* extern "C" */
