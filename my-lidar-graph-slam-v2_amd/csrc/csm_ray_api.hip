/* csm_ray_api.hip -- the free-space check of loop candidates: csm_ray_check_batch and the host
 * restatements csm_host_ray_check / csm_host_ray_check_values (include/csm_hip.h), with their kernels
 * (csm_ray_kernels.hip). A translation unit of libcsm_hip.so of its own; what it shares with the ray cast
 * (csm_cast_api.hip) is csm_ray.hpp.
 *
 * A batch is checked first (every query, every map: a refused call has run nothing) and then cut into chunks
 * of consecutive queries. Per chunk: one upload ([queries][prefixes][the distinct scans], from rc_pin into
 * rc_tab), k_ray_project over all beams, one small read-back (the uncertified beams), their records from
 * glibc scattered in by k_ray_patch, k_ray_walk, one read-back of [records][per-beam words]. Nothing the
 * context keeps between calls is touched but these workspaces. */
#include "csm_internal.hpp"

#include "csm_ray_kernels.hip"

static_assert(sizeof(csm_ray_check_result) == kRayRecordBytes &&
              offsetof(csm_ray_check_result, usable) == 4 * kRayUsable &&
              offsetof(csm_ray_check_result, end_unknown) == 4 * kRayEndUnknown &&
              offsetof(csm_ray_check_result, cells) == 32 &&
              offsetof(csm_ray_check_result, cells_blocking) == 32 + 8 * (kRayCellsBlocking - kRayCells) &&
              offsetof(csm_ray_check_result, max_depth) == kRayMaxDepthAt,
              "k_ray_walk adds to the record by these offsets");

namespace {

bool ray_params_ok(const csm_ray_check_params* p)
{
    return p && p->subpixel_scale >= 1 && p->subpixel_scale <= CSM_RAY_CHECK_MAX_SCALE && p->end_tolerance >= 0 &&
           p->free_max > 0 && p->free_max < p->occupied_min && p->occupied_min <= 65535u &&
           p->scratch_limit_bytes >= 0 && !std::isnan(p->usable_range_min) && !std::isnan(p->usable_range_max);
}

/* the sensor pose S and its sub-pixel index (ray_frame, csm_ray.hpp); false: the query is refused */
bool ray_query_frame(const csm_geometry* geom, const csm_scan* scan, const double pose[3],
                     const csm_ray_check_params* p, double S[3], int32_t s[2])
{
    if (!geom || !scan || !pose || scan->n_points < 0 || (scan->n_points > 0 && (!scan->angles || !scan->ranges)))
        return false;
    if (!geometry_is_finite(geom))
        return false;
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(pose[k]) || !std::isfinite(scan->relative_sensor_pose[k]))
            return false;
    for (int i = 0; i < scan->n_points; ++i)
        if (!std::isfinite(scan->angles[i]))
            return false;
    csm_host_compound(pose, scan->relative_sensor_pose, S);
    return ray_frame(geom, S, p->usable_range_max, p->subpixel_scale, s);
}

/* Chunks of consecutive queries: a query of n beams counts 36 n + 256 bytes (record, word, scan, table
 * entry); a chunk is closed before the query that would take it past the limit. */
int64_t ray_query_bytes(int n) { return 36ll * n + 256; }

} /* namespace */

extern "C" {

int csm_host_ray_check_values(double prob_occupied, double prob_free, uint32_t* occupied_min, uint32_t* free_max)
{
    if (!occupied_min || !free_max || !std::isfinite(prob_occupied) || !std::isfinite(prob_free))
        return CSM_EINVAL;
    std::vector<double> lut(65536);
    csm_host_probability_lut(lut.data());
    uint32_t occ = 0, fre = 0;
    for (uint32_t v = 1; v < 65536u && !occ; ++v)
        if (lut[v] >= prob_occupied)
            occ = v;
    for (uint32_t v = 65535u; v >= 1u && !fre; --v)
        if (lut[v] <= prob_free)
            fre = v;
    if (!occ || !fre || fre >= occ)
        return CSM_EINVAL;
    *occupied_min = occ;
    *free_max = fre;
    return CSM_OK;
}

int csm_host_ray_check(const uint16_t* grid, int32_t rows, int32_t cols, const csm_geometry* geom,
                       const csm_scan* scan, const double pose[3], const csm_ray_check_params* prm,
                       csm_ray_check_result* result, int32_t* per_beam)
{
    double S[3];
    int32_t s[2];
    if (!grid || rows < 1 || cols < 1 || !result || !ray_params_ok(prm) ||
        !ray_query_frame(geom, scan, pose, prm, S, s))
        return CSM_EINVAL;
    const int scale = prm->subpixel_scale;
    const double scaled_res = geom->resolution / scale;
    csm_ray_check_result out;
    std::memset(&out, 0, sizeof(out));
    out.beams = scan->n_points;
    std::vector<Cell> walk;
    auto inside = [rows, cols](int x, int y) { return x >= 0 && x < cols && y >= 0 && y < rows; };
    for (int i = 0; i < scan->n_points; ++i) {
        const double r = scan->ranges[i];
        int word = -2;
        if (r > prm->usable_range_min && r < prm->usable_range_max) {
            ++out.usable;
            const RayRec rec = ray_host_rec(S, geom, scaled_res, r, scan->angles[i]);
            const int bx = host_floor_div(std::min(s[0], rec.ex), scale), by = host_floor_div(std::min(s[1], rec.ey), scale);
            ray_step_cells(s[0] - bx * scale, s[1] - by * scale, rec.ex - bx * scale, rec.ey - by * scale, scale, walk);
            const Cell end(host_floor_div(rec.ex, scale) - bx, host_floor_div(rec.ey, scale) - by);
            const auto it = std::find(walk.begin(), walk.end(), end);      /* grid_map_builder.cpp:904-910 */
            if (it != walk.end())
                walk.erase(it);
            bool any = false;
            int depth = 0;
            for (const Cell& c : walk) {
                const int x = c.first + bx, y = c.second + by;
                if (!inside(x, y))
                    continue;
                any = true;
                const uint32_t v = grid[(size_t)y * cols + x];
                ++out.cells;
                if (v == 0) {
                    ++out.cells_unknown;
                } else if (v <= prm->free_max) {
                    ++out.cells_free;
                } else if (v >= prm->occupied_min) {
                    const int d = std::max(std::abs(x - rec.hx), std::abs(y - rec.hy));
                    if (d > prm->end_tolerance) {
                        ++out.cells_blocking;
                        depth = std::max(depth, d);
                    } else {
                        ++out.cells_near;
                    }
                }
            }
            const bool end_in = inside(rec.hx, rec.hy);
            if (end_in) {
                const uint32_t v = grid[(size_t)rec.hy * cols + rec.hx];
                ++out.end_inside;
                out.end_unknown += v == 0;
                out.end_free += v != 0 && v <= prm->free_max;
                out.end_occupied += v >= prm->occupied_min;
            }
            word = -1;
            if (any || end_in) {
                ++out.walked;
                word = depth;
                out.blocked += depth > 0;
                out.max_depth = std::max(out.max_depth, depth);
            }
        }
        if (per_beam)
            per_beam[i] = word;
    }
    *result = out;
    return CSM_OK;
}

int csm_ray_check_batch(csm_ctx* ctx, const csm_loop_query* queries, int32_t n_queries,
                        const csm_ray_check_params* prm, csm_ray_check_result* results, int32_t* per_beam)
{
    if (!ctx || !queries || n_queries < 1 || !results)
        return fail(ctx, CSM_EINVAL, "csm_ray_check_batch: bad arguments");
    if (!ray_params_ok(prm))
        return fail(ctx, CSM_EINVAL, "ray check: need 0 < free_max < occupied_min <= 65535, subpixel_scale in 1..%d, "
                    "end_tolerance >= 0, scratch_limit_bytes >= 0 and usable ranges that are numbers",
                    CSM_RAY_CHECK_MAX_SCALE);
    struct Frame {
        double S[3];
        int32_t s[2];
    };
    std::vector<Frame> frames((size_t)n_queries);
    for (int i = 0; i < n_queries; ++i) {
        const csm_loop_query& q = queries[i];
        if (!ray_query_frame(&q.geometry, &q.scan, q.initial_pose, prm, frames[i].S, frames[i].s))
            return fail(ctx, CSM_EINVAL, "ray check: query %d has a bad scan, geometry or pose, a sensor more than "
                        "2^20 cells from the map's origin, or usable_range_max / resolution > 2^20", i);
        const DeviceGrid* g = find_grid(ctx, q.map_id);
        if (!g || g->levels.empty())
            return fail(ctx, CSM_ENOENT, "map %llu not resident", (unsigned long long)q.map_id);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    const int64_t limit = prm->scratch_limit_bytes ? prm->scratch_limit_bytes : kRayDefaultScratch;
    const uint32_t unc_cap = ray_unc_cap(ctx);
    const size_t unc_bytes = align256(((size_t)unc_cap + 1) * 4);
    const int scale = prm->subpixel_scale;
    bool host_projection = ctx->tune.map_host_projection;
    size_t words_done = 0;

    for (int q0 = 0; q0 < n_queries;) {
        /* the chunk [q0, q1) */
        int q1 = q0;
        int64_t bytes = 0, beams_ll = 0;
        while (q1 < n_queries && (q1 == q0 || (bytes + ray_query_bytes(queries[q1].scan.n_points) <= limit &&
                                                beams_ll + queries[q1].scan.n_points < (1ll << 30)))) {
            bytes += ray_query_bytes(queries[q1].scan.n_points);
            beams_ll += queries[q1].scan.n_points;
            ++q1;
        }
        const int nq = q1 - q0, nb = (int)beams_ll;

        /* the distinct scans of the chunk, in first-use order */
        ScanTable table;
        std::vector<long long> scan_at((size_t)nq);     /* of [angles | ranges], in doubles */
        for (int k = 0; k < nq; ++k)
            scan_at[k] = 2 * table.slot(queries[q0 + k].scan, k);

        /* upload block: [queries][pre_beam][pre_group][scans]; the three tables are one piece */
        const size_t tab_bytes = align256((size_t)nq * sizeof(RayQuery) + 2 * ((size_t)nq + 1) * 4);
        const size_t up_bytes = tab_bytes + 2 * (size_t)table.beams * 8;
        /* work block: [uncertified count + list][records][words] | [ray records][patches]; what goes back,
         * list, records and words, is one piece */
        const size_t rec_bytes = (size_t)nq * kRayRecordBytes, word_bytes = (size_t)nb * 4;
        const size_t back_bytes = unc_bytes + rec_bytes + word_bytes;
        Carve wk;
        wk.take(back_bytes);
        const size_t recs_at = wk.take((size_t)nb * sizeof(RayRec)), patch_at = wk.off;
        const size_t patch_bytes = std::max((size_t)unc_cap * sizeof(RayPatch), (size_t)nb * sizeof(RayRec));
        const size_t work_bytes = patch_at + (size_t)unc_cap * sizeof(RayPatch);
        int rc, e;
        if ((rc = reserve(ctx, ctx->rc_tab, up_bytes))) return rc;
        if ((rc = reserve(ctx, ctx->rc_work, work_bytes))) return rc;
        if ((rc = reserve(ctx, ctx->rc_pin, up_bytes + patch_bytes))) return rc;
        if ((rc = reserve(ctx, ctx->rc_back, back_bytes))) return rc;
        char* const pin = ctx->rc_pin.as<char>();
        char* const tab = ctx->rc_tab.as<char>();
        char* const work = ctx->rc_work.as<char>();
        char* const back = ctx->rc_back.as<char>();

        RayQuery* const Q = reinterpret_cast<RayQuery*>(pin);
        uint32_t* const pre_beam = reinterpret_cast<uint32_t*>(pin + (size_t)nq * sizeof(RayQuery));
        uint32_t* const pre_group = pre_beam + nq + 1;
        double* const scans = reinterpret_cast<double*>(pin + tab_bytes);
        pre_beam[0] = pre_group[0] = 0;
        for (int k = 0; k < nq; ++k) {
            const csm_loop_query& q = queries[q0 + k];
            const DeviceGrid& g = *find_grid(ctx, q.map_id);
            RayQuery& J = Q[k];
            J.cells = g.levels[0].cells;
            J.rows = g.rows;
            J.cols = g.cols;
            J.pitch = g.pitch;
            J.n_beams = q.scan.n_points;
            J.angles_at = scan_at[k];
            J.ranges_at = scan_at[k] + q.scan.n_points;
            J.x = frames[q0 + k].S[0];
            J.y = frames[q0 + k].S[1];
            J.theta = frames[q0 + k].S[2];
            J.off_x = q.geometry.offset_x;
            J.off_y = q.geometry.offset_y;
            J.res = q.geometry.resolution;
            J.scaled_res = q.geometry.resolution / scale;
            J.sx = frames[q0 + k].s[0];
            J.sy = frames[q0 + k].s[1];
            J.pad[0] = J.pad[1] = 0;
            pre_beam[k + 1] = pre_beam[k] + (uint32_t)q.scan.n_points;
            pre_group[k + 1] = pre_group[k] + (uint32_t)ceil_div(q.scan.n_points, kRayGroup);
        }
        for (int k : table.first_use) {
            const csm_scan& sc = queries[q0 + k].scan;
            if (sc.n_points) {
                std::memcpy(scans + scan_at[k], sc.angles, (size_t)sc.n_points * 8);
                std::memcpy(scans + scan_at[k] + sc.n_points, sc.ranges, (size_t)sc.n_points * 8);
            }
        }
        HIP_TRY(ctx, hipMemcpyAsync(tab, pin, up_bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(work, 0, unc_bytes + rec_bytes, ctx->stream));

        RayChunk ch;
        ch.queries = reinterpret_cast<const RayQuery*>(tab);
        ch.pre_beam = reinterpret_cast<const uint32_t*>(tab + (size_t)nq * sizeof(RayQuery));
        ch.pre_group = ch.pre_beam + nq + 1;
        ch.scans = reinterpret_cast<const double*>(tab + tab_bytes);
        ch.unc = reinterpret_cast<uint32_t*>(work);
        ch.records = reinterpret_cast<unsigned char*>(work + unc_bytes);
        ch.words = reinterpret_cast<int32_t*>(work + unc_bytes + rec_bytes);
        ch.recs = reinterpret_cast<RayRec*>(work + recs_at);
        ch.unc_cap = unc_cap;
        ch.n_queries = nq;
        ch.n_beams = nb;
        ch.min_range = prm->usable_range_min;
        ch.max_range = prm->usable_range_max;
        ch.scale = scale;
        ch.tolerance = prm->end_tolerance;
        ch.occupied_min = prm->occupied_min;
        ch.free_max = prm->free_max;

        std::vector<int32_t> host_beams((size_t)nq, 0);
        uint32_t n_unc = 0;
        if (nb > 0 && !host_projection) {
            {
                ScopedTimer tm(ctx, "ray_project");
                e = launch(k_ray_project, dim3((unsigned)ceil_div(nb, 256)), dim3(256), ctx->stream, ch);
            }
            if ((rc = launched_ok(ctx, e, "ray project"))) return rc;
            HIP_TRY(ctx, hipMemcpyAsync(back, work, unc_bytes, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            n_unc = reinterpret_cast<const uint32_t*>(back)[0];
            if (n_unc > unc_cap) {
                host_projection = true;     /* too many beams on cell edges: this chunk and the rest on the host */
                n_unc = 0;
            }
        }
        char* const patch_pin = pin + up_bytes;
        if (nb > 0 && host_projection) {
            RayRec* const all = reinterpret_cast<RayRec*>(patch_pin);
            for (int k = 0; k < nq; ++k) {
                const csm_loop_query& q = queries[q0 + k];
                for (int i = 0; i < q.scan.n_points; ++i) {
                    const double r = q.scan.ranges[i];
                    RayRec rec = { kRayUnusable, 0, 0, 0 };
                    if (r > prm->usable_range_min && r < prm->usable_range_max) {
                        rec = ray_host_rec(frames[q0 + k].S, &q.geometry, Q[k].scaled_res, r, q.scan.angles[i]);
                        ++host_beams[k];
                    }
                    all[pre_beam[k] + i] = rec;
                }
            }
            HIP_TRY(ctx, hipMemcpyAsync(ch.recs, all, (size_t)nb * sizeof(RayRec), hipMemcpyHostToDevice, ctx->stream));
        } else if (n_unc > 0) {
            /* the beams the device could not certify: exactly as glibc has them, and patched in */
            const uint32_t* const list = reinterpret_cast<const uint32_t*>(back) + 1;
            RayPatch* const patches = reinterpret_cast<RayPatch*>(patch_pin);
            for (uint32_t u = 0; u < n_unc; ++u) {
                const uint32_t b = list[u];
                const int k = (int)(std::upper_bound(pre_beam, pre_beam + nq + 1, b) - pre_beam) - 1;
                const csm_loop_query& q = queries[q0 + k];
                const int i = (int)(b - pre_beam[k]);
                patches[u].beam = b;
                patches[u].rec = ray_host_rec(frames[q0 + k].S, &q.geometry, Q[k].scaled_res, q.scan.ranges[i],
                                              q.scan.angles[i]);
                ++host_beams[k];
            }
            RayPatch* const patches_dev = reinterpret_cast<RayPatch*>(work + patch_at);
            HIP_TRY(ctx, hipMemcpyAsync(patches_dev, patches, (size_t)n_unc * sizeof(RayPatch), hipMemcpyHostToDevice,
                                        ctx->stream));
            e = launch(k_ray_patch, dim3((unsigned)ceil_div((int)n_unc, 256)), dim3(256), ctx->stream, patches_dev,
                       (int)n_unc, ch.recs);
            if ((rc = launched_ok(ctx, e, "ray patch"))) return rc;
        }
        if (pre_group[nq] > 0) {
            ScopedTimer tm(ctx, "ray_walk");
            e = launch(k_ray_walk, dim3(pre_group[nq]), dim3(256), ctx->stream, ch);
            if ((rc = launched_ok(ctx, e, "ray walk"))) return rc;
        }
        const size_t fetch = rec_bytes + (per_beam ? word_bytes : 0);
        HIP_TRY(ctx, hipMemcpyAsync(back + unc_bytes, work + unc_bytes, fetch, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        std::memcpy(results + q0, back + unc_bytes, rec_bytes);
        for (int k = 0; k < nq; ++k) {
            results[q0 + k].beams = queries[q0 + k].scan.n_points;
            results[q0 + k].host_beams = host_beams[k];
        }
        if (per_beam && word_bytes) {
            std::memcpy(per_beam + words_done, back + unc_bytes + rec_bytes, word_bytes);
            words_done += (size_t)nb;
        }
        q0 = q1;
    }
    return CSM_OK;
}

} /* extern "C" */
