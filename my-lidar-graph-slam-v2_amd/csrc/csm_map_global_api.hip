/* csm_map_global_api.hip -- host side of csm_construct_global_map
 * (GridMapBuilder::ConstructGlobalMap, src/mapping/grid_map_builder.cpp:162-184), its planner
 * csm_host_global_map_parts and csm_host_global_scan_poses (include/csm_hip.h), with their
 * kernels (csm_map_global_kernels.hip). A translation unit of libcsm_hip.so of its own.
 *
 * One map of many scans. The host steps are those of csm_map_build.hpp; what this file keeps is
 * the cut of the nodes into parts, the order of the phases and the launches:
 *   bounds   every piece of the nodes is projected (certified on the device, the uncertain beams
 *            patched by glibc, or on the host under map_patch_rays's rules) for its bounding box
 *            only; the boxes are merged
 *   resize   map_resize and map_claim_grid ONCE, on the merged box
 *   cast     per part, in node order, the update chain on the fixed frame: the first part on
 *            cleared cells, every later one on top of the cells the earlier ones left
 *            (MapJob.keep_cells, no Expand). A cell's value depends only on its own sequence of
 *            hits and misses in ray order, and the parts' sequences concatenate.
 * The counter block stays on the device through all parts (update and saturation totals add, the
 * first-known minima only fall, the error flag is sticky) and is read back once. */
#include "csm_map_build.hpp"

#include "csm_map_global_kernels.hip"

namespace {

constexpr int64_t kGmapDefaultLimit = 1ll << 30;
constexpr int64_t kGmapBeamsMax = 1ll << 24;     /* per part: ray numbers and MapNode.beam_base */
constexpr int64_t kGmapCellsMax = 1ll << 28;
constexpr int32_t kGmapDirectDefault = 32;
constexpr int32_t kGmapTileDefault = 4096;       /* 16 KB of LDS */
constexpr int32_t kGmapTileMax = 16384;          /* 64 KB: what one workgroup may take without an attribute */

/* the scratch of one part: what csm_host_map_batch_plan counts for a job of that size */
int64_t part_scratch(int64_t n_beams, int64_t n_cells)
{
    int32_t chunk_of = 0, n_chunks = 0;
    int64_t bytes = 0;
    (void)csm_host_map_batch_plan(&n_beams, &n_cells, 1, 0, &chunk_of, &bytes, &n_chunks);
    return bytes;
}

/* one part of the nodes on its way through a phase */
struct Part : MapBuild {
    int first = 0;                         /* its first node in the caller's array */
};

/* the device buffers of a build, sized for its largest part */
struct Scratch {
    MapRay* rays = nullptr;
    MapNode* nodes = nullptr;
    unsigned long long* counters = nullptr;
    int32_t* box = nullptr;                /* [8]: box, count, spread bits, 2 unused; the list follows */
    uint32_t* unc_list = nullptr;
    uint32_t unc_cap = 0;
    std::vector<int32_t> got;              /* the read-back of box and list */
};

int make_parts(csm_ctx* ctx, const csm_map_builder_params* prm, const MapBuild& whole,
               const std::vector<int32_t>& part_of, std::vector<Part>& parts)
{
    parts.clear();
    for (int k = 0; k < whole.n_nodes;) {
        int last = k;
        while (last < whole.n_nodes && part_of[last] == part_of[k])
            ++last;
        parts.emplace_back();
        Part& p = parts.back();
        p.first = k;
        p.map_id = whole.map_id;
        p.shape = whole.shape;
        p.map_pose = whole.map_pose;
        p.nodes = whole.nodes + k;
        p.n_nodes = last - k;
        if (int rc = map_node_table(ctx, prm, p))
            return rc;
        k = last;
    }
    return CSM_OK;
}

/* The hit points of one part in s.rays and its box in p (map_take_projection, map_patch_rays): one
 * launch, one read-back (box, count and the listed beams together). */
int project_part(csm_ctx* ctx, Part& p, Scratch& s, int scale)
{
    const int n_rays = p.n_beams;
    std::vector<double> stage;
    if (p.device_projection) {
        stage.resize(2 * (size_t)n_rays);
        for (int k = 0; k < p.n_nodes; ++k) {
            std::memcpy(stage.data() + p.table[k].beam_base, p.nodes[k].scan.angles,
                        (size_t)p.table[k].n_beams * sizeof(double));
            std::memcpy(stage.data() + n_rays + p.table[k].beam_base, p.nodes[k].scan.ranges,
                        (size_t)p.table[k].n_beams * sizeof(double));
        }
        double* d_scan = reinterpret_cast<double*>(ctx->scan_dev.p);
        const int32_t init_box[8] = { 0x7fffffff, 0x7fffffff, -0x7fffffff - 1, -0x7fffffff - 1, 0, 0, 0, 0 };
        HIP_TRY(ctx, hipMemcpyAsync(d_scan, stage.data(), stage.size() * sizeof(double), hipMemcpyHostToDevice,
                                    ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(s.nodes, p.table.data(), p.table.size() * sizeof(MapNode),
                                    hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(s.box, init_box, sizeof(init_box), hipMemcpyHostToDevice, ctx->stream));
        MapProjJob pj;
        std::memset(&pj, 0, sizeof(pj));
        pj.angles = d_scan;
        pj.ranges = d_scan + n_rays;
        pj.nodes = s.nodes;
        pj.n_nodes = p.n_nodes;
        pj.n_beams = n_rays;
        pj.rays = s.rays;
        pj.off_x = p.shape->offset_x;       /* the frame BEFORE the resize, in both phases */
        pj.off_y = p.shape->offset_y;
        pj.res = p.shape->resolution;
        pj.scaled_res = p.shape->resolution / scale;
        pj.box = s.box;
        pj.unc_count = reinterpret_cast<uint32_t*>(s.box + 4);
        pj.unc_list = s.unc_list;
        pj.unc_cap = s.unc_cap;
        int e;
        {
            ScopedTimer tm(ctx, "gmap_project");
            e = launch(k_gmap_project, dim3((unsigned)ceil_div(n_rays, 256)), dim3(256), ctx->stream, pj);
        }
        if (int rc = launched_ok(ctx, e, "global map project"))
            return rc;
        const size_t words = 8 + std::min<size_t>(s.unc_cap, (size_t)n_rays);
        HIP_TRY(ctx, hipMemcpyAsync(s.got.data(), s.box, words * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (int k = 0; k < 4; ++k)
            p.box[k] = k < 2 ? 0x7fffffff : -0x7fffffff - 1;
        map_take_projection(p, s.got.data(), s.unc_cap);
    }
    std::vector<MapRay> patch;              /* source of asynchronous uploads */
    bool uploads = false;
    if (int rc = map_patch_rays(ctx, p, reinterpret_cast<const uint32_t*>(s.got.data() + 8), s.rays, patch, uploads))
        return rc;
    if (uploads)
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CSM_OK;
}

int cut(const std::vector<int64_t>& beams, int64_t n_cells, int64_t limit, std::vector<int32_t>& part_of)
{
    std::vector<int64_t> bytes(beams.size());
    int32_t n_parts = 0;
    part_of.resize(beams.size());
    return csm_host_global_map_parts(beams.data(), (int32_t)beams.size(), n_cells, limit, part_of.data(),
                                     bytes.data(), &n_parts);
}

} /* namespace */

extern "C" {

int csm_host_global_map_parts(const int64_t* n_beams, int32_t n_nodes, int64_t n_cells,
                              int64_t scratch_limit_bytes, int32_t* part_of, int64_t* part_bytes,
                              int32_t* n_parts)
{
    if (!n_beams || n_nodes < 1 || scratch_limit_bytes < 0 || n_cells < 0 || n_cells > kGmapCellsMax || !part_of ||
        !part_bytes || !n_parts)
        return CSM_EINVAL;
    for (int k = 0; k < n_nodes; ++k)
        if (n_beams[k] < 0 || n_beams[k] > kGmapBeamsMax)
            return CSM_EINVAL;
    const int64_t limit = scratch_limit_bytes ? scratch_limit_bytes : kGmapDefaultLimit;
    int part = 0, held_nodes = 0;
    int64_t held = 0;
    for (int k = 0; k < n_nodes; ++k) {
        if (held_nodes && (held + n_beams[k] > kGmapBeamsMax || part_scratch(held + n_beams[k], n_cells) > limit)) {
            part_bytes[part++] = part_scratch(held, n_cells);
            held = 0;
            held_nodes = 0;
        }
        held += n_beams[k];
        ++held_nodes;
        part_of[k] = part;
    }
    part_bytes[part++] = part_scratch(held, n_cells);
    *n_parts = part;
    return CSM_OK;
}

/* ConstructMapFromAllScans's pose of a scan node (grid_map_builder.cpp:698-817):
 * Compound(LocalMapNode::mGlobalPose, ScanNode::mLocalPose) */
int csm_host_global_scan_poses(const double local_map_pose[3], const double* local_poses, int32_t n,
                               double* out_global_poses)
{
    if (!local_map_pose || n < 0 || (n > 0 && (!local_poses || !out_global_poses)))
        return CSM_EINVAL;
    for (int i = 0; i < n; ++i)
        csm_host_compound(local_map_pose, local_poses + 3 * (size_t)i, out_global_poses + 3 * (size_t)i);
    return CSM_OK;
}

int csm_construct_global_map(csm_ctx* ctx, uint64_t map_id, csm_map_shape* shape,
                             const double global_map_pose[3], const csm_scan_node* nodes, int32_t n_nodes,
                             const csm_map_builder_params* prm, const csm_global_map_params* gp,
                             csm_map_build_info* info, csm_global_map_info* ginfo)
{
    if (!ctx || !shape || !global_map_pose || !prm || prm->subpixel_scale < 1 || prm->subpixel_scale > 1024)
        return fail(ctx, CSM_EINVAL, "map build: bad arguments");
    const int64_t limit = gp ? gp->scratch_limit_bytes : 0;
    const int32_t direct_max = gp && gp->rank_direct_max ? gp->rank_direct_max : kGmapDirectDefault;
    const int32_t tile = gp && gp->rank_tile ? gp->rank_tile : kGmapTileDefault;
    if (limit < 0 || direct_max < 1 || tile < 4 || tile > kGmapTileMax || (tile & (tile - 1)))
        return fail(ctx, CSM_EINVAL, "global map: bad scratch limit or rank settings");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const double t0 = clock_us();
    const int scale = prm->subpixel_scale;
    int rc = 0;

    MapBuild whole;
    whole.map_id = map_id;
    whole.shape = shape;
    whole.map_pose = global_map_pose;
    whole.nodes = nodes;
    whole.n_nodes = n_nodes;
    if (!nodes || n_nodes < 1)
        return fail(ctx, CSM_EINVAL, "map build: bad arguments");

    /* ---- the pieces of the bounds phase: cut by the beams alone, the cells are not known yet ---- */
    std::vector<int64_t> beams((size_t)n_nodes);
    int64_t beams_all = 0;
    for (int k = 0; k < n_nodes; ++k) {
        if (!nodes[k].scan.angles || !nodes[k].scan.ranges || nodes[k].scan.n_points < 0)
            return fail(ctx, CSM_EINVAL, "scan node %d has no scan", k);
        beams[k] = nodes[k].scan.n_points;
        beams_all += beams[k];
    }
    std::vector<int32_t> piece_of, part_of;
    if (cut(beams, 0, limit, piece_of) != CSM_OK)
        return fail(ctx, CSM_EINVAL, "%lld beams in one scan node", (long long)*std::max_element(beams.begin(), beams.end()));
    std::vector<Part> pieces, recut;
    if ((rc = make_parts(ctx, prm, whole, piece_of, pieces))) return rc;

    size_t rays_max = 1, nodes_max = 1;
    for (const Part& p : pieces) {
        rays_max = std::max(rays_max, (size_t)p.n_beams);
        nodes_max = std::max(nodes_max, (size_t)p.n_nodes);
    }
    Scratch s;
    s.unc_cap = map_unc_cap(ctx);
    s.got.assign(8 + (size_t)s.unc_cap, 0);
    auto take_scratch = [&]() -> int {
        int rc2 = 0;
        if ((rc2 = ensure(ctx, ctx->m_rays, rays_max * sizeof(MapRay) + nodes_max * sizeof(MapNode) + 64))) return rc2;
        if ((rc2 = ensure(ctx, ctx->m_cnt, kGmapCounters * sizeof(unsigned long long) + 64 + (size_t)kMapUncCap * 4))) return rc2;
        if ((rc2 = ensure(ctx, ctx->scan_dev, 2 * rays_max * sizeof(double)))) return rc2;
        s.rays = reinterpret_cast<MapRay*>(ctx->m_rays.p);
        s.nodes = reinterpret_cast<MapNode*>(s.rays + rays_max);
        s.counters = reinterpret_cast<unsigned long long*>(ctx->m_cnt.p);
        s.box = reinterpret_cast<int32_t*>(s.counters + kGmapCounters);
        s.unc_list = reinterpret_cast<uint32_t*>(s.box + 8);
        return CSM_OK;
    };
    if ((rc = take_scratch())) return rc;

    /* ---- bounds: every piece's box, merged ---- */
    whole.min_x = whole.min_y = std::numeric_limits<double>::max();
    whole.max_x = whole.max_y = std::numeric_limits<double>::min();   /* as the reference: smallest positive */
    for (int k = 0; k < 4; ++k)
        whole.box[k] = k < 2 ? 0x7fffffff : -0x7fffffff - 1;
    whole.device_projection = true;
    for (Part& p : pieces) {
        if ((rc = project_part(ctx, p, s, scale))) return rc;
        whole.add_point(p.min_x, p.min_y);
        whole.add_point(p.max_x, p.max_y);
        whole.box[0] = std::min(whole.box[0], p.box[0]);
        whole.box[1] = std::min(whole.box[1], p.box[1]);
        whole.box[2] = std::max(whole.box[2], p.box[2]);
        whole.box[3] = std::max(whole.box[3], p.box[3]);
        whole.spread_known |= p.spread_known;
        whole.device_projection &= p.device_projection;
        whole.usable += p.usable;
        whole.table.insert(whole.table.end(), p.table.begin(), p.table.end());
    }

    /* ---- one resize, one destination grid ---- */
    if ((rc = map_resize(ctx, whole, scale))) return rc;
    const size_t n_cells = whole.n_cells;
    if ((rc = cut(beams, (int64_t)n_cells, limit, part_of)))
        return fail(ctx, rc, "global map: internal: the plan was refused");
    const bool reproject = pieces.size() > 1 || part_of != piece_of;
    std::vector<Part>* parts = &pieces;
    if (part_of != piece_of) {
        if ((rc = make_parts(ctx, prm, whole, part_of, recut))) return rc;
        parts = &recut;
        /* every part is projected again: the buffers may move */
        for (const Part& p : recut) {
            rays_max = std::max(rays_max, (size_t)p.n_beams);
            nodes_max = std::max(nodes_max, (size_t)p.n_nodes);
        }
        if ((rc = take_scratch())) return rc;
    }
    for (Part& p : *parts)
        for (int k = 0; k < p.n_nodes; ++k) {
            p.table[k].sx = whole.table[(size_t)p.first + k].sx;
            p.table[k].sy = whole.table[(size_t)p.first + k].sy;
        }
    if ((rc = map_ensure_tables(ctx, prm))) return rc;
    bool synced = false;
    if ((rc = map_claim_grid(ctx, whole, ctx->m_alloc, synced))) return rc;

    /* the scratch of the largest part (the rays of an only part stay where the bounds phase left them) */
    size_t part_rays = 1;
    for (const Part& p : *parts)
        part_rays = std::max(part_rays, (size_t)p.n_beams);
    if ((rc = ensure(ctx, ctx->m_recs, part_rays * sizeof(MapRayRec)))) return rc;
    if ((rc = ensure(ctx, ctx->m_lists, (11 * part_rays + 20) * sizeof(uint32_t)))) return rc;
    if ((rc = ensure(ctx, ctx->m_cell, 3 * n_cells * sizeof(uint32_t)))) return rc;

    /* ---- cast: the update chain per part ---- */
    unsigned long long counters[kGmapCounters] = { 0 };
    counters[kMapKnownRow] = counters[kMapKnownCol] = ~0ull;
    const GmapRank rk = { (uint32_t)direct_max, (uint32_t)tile };
    const uint16_t* d_lut = reinterpret_cast<const uint16_t*>(ctx->m_lut.p);
    const double t1 = clock_us();
    double cast_host_us = 0.0;
    CallSpan span(ctx);
    if (!span.a || !span.b)
        return fail(ctx, CSM_EIO, "global map: no event for device_us");
    HIP_TRY(ctx, hipEventRecord(span.a, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(s.counters, counters, sizeof(counters), hipMemcpyHostToDevice, ctx->stream));
    for (size_t i = 0; i < parts->size(); ++i) {
        Part& p = (*parts)[i];
        if (i > 0 && p.usable == 0)
            continue;                        /* nothing to add to the cells */
        if (reproject) {
            /* the host waits here (staging, the projection's read-back, patches): host time, not device */
            const double h0 = clock_us();
            if ((rc = project_part(ctx, p, s, scale))) return rc;
            cast_host_us += clock_us() - h0;
        }
        p.keep_cells = i > 0;
        p.next = whole.next;
        p.dst = whole.dst;
        MapJob mj;
        std::memset(&mj, 0, sizeof(mj));
        mj.rays = s.rays;
        mj.nodes = s.nodes;
        mj.recs = reinterpret_cast<MapRayRec*>(ctx->m_recs.p);
        mj.n_hit = reinterpret_cast<uint32_t*>(ctx->m_cell.p);
        mj.n_miss = mj.n_hit + n_cells;
        mj.seg = mj.n_miss + n_cells;
        mj.lists = reinterpret_cast<uint32_t*>(ctx->m_lists.p);
        mj.counters = s.counters;
        map_fill_job(p, scale, d_lut, mj);
        const int n_rays = p.n_beams;
        HIP_TRY(ctx, hipMemcpyAsync(s.nodes, p.table.data(), p.table.size() * sizeof(MapNode), hipMemcpyHostToDevice,
                                    ctx->stream));
        if (i > 0) {
            /* the words of a part: list cursor, hit cells, long cells. The totals go on. */
            if ((rc = launched_ok(ctx, launch(k_gmap_next_part, dim3(1), dim3(64), ctx->stream, s.counters),
                                  "global map next part")))
                return rc;
        }
        HIP_TRY(ctx, hipMemsetAsync(mj.n_hit, 0, 2 * n_cells * sizeof(uint32_t), ctx->stream));
        const dim3 ray_blocks((unsigned)ceil_div(std::max(n_rays, 1), 256));
        const dim3 cell_blocks((unsigned)((n_cells + 255) / 256));
        const dim3 blk(256);
        int e = 0;
        if (n_rays) {
            {
                ScopedTimer tm(ctx, "gmap_hits");
                keep_first(e, launch(k_gmap_hits, ray_blocks, blk, ctx->stream, mj));
            }
            {
                ScopedTimer tm(ctx, "gmap_alloc");
                keep_first(e, launch(k_gmap_alloc, cell_blocks, blk, ctx->stream, mj, rk));
            }
            {
                ScopedTimer tm(ctx, "gmap_fill_hits");
                keep_first(e, launch(k_gmap_fill_hits, ray_blocks, blk, ctx->stream, mj));
            }
            {
                ScopedTimer tm(ctx, "gmap_rank_direct");
                keep_first(e, launch(k_gmap_rank_direct, ray_blocks, blk, ctx->stream, mj, rk));
            }
            /* a long cell has more than direct_max hits: at most this many of them */
            const unsigned long_max = (unsigned)(p.usable / ((long long)direct_max + 1));
            if (long_max) {
                ScopedTimer tm(ctx, "gmap_rank_sort");
                keep_first(e, launch_lds(ctx->device, k_gmap_rank_sort, dim3(long_max), blk,
                                         (size_t)tile * sizeof(uint32_t), ctx->stream, mj, rk));
            }
            {
                ScopedTimer tm(ctx, "gmap_walk");
                keep_first(e, launch(k_gmap_walk, dim3((unsigned)ceil_div(n_rays, kMapGroup)), dim3(512), ctx->stream,
                                     mj));
            }
        }
        {
            ScopedTimer tm(ctx, "gmap_apply");
            const dim3 apply_blocks((unsigned)(((size_t)mj.rows * mj.pitch + 255) / 256));
            keep_first(e, launch(k_gmap_apply, apply_blocks, blk, ctx->stream, mj));
        }
        if (p.usable > 0) {
            const unsigned wgs = (unsigned)std::min<long long>(
                256, ceil_div((int)std::min<long long>(p.usable, (long long)n_cells), 4));
            ScopedTimer tm(ctx, "gmap_apply_hits");
            keep_first(e, launch_lds(ctx->device, k_gmap_apply_hits, dim3(wgs), blk, 65536 * sizeof(uint16_t),
                                     ctx->stream, mj));
        }
        if ((rc = launched_ok(ctx, e, "global map cast"))) return rc;
    }
    /* the old allocation moved by the block shift, and every block that holds a known cell */
    if ((rc = map_carry_allocation(ctx, whole, ctx->m_alloc))) return rc;
    HIP_TRY(ctx, hipEventRecord(span.b, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(counters, s.counters, sizeof(counters), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float dev_ms = 0.f;
    (void)hipEventElapsedTime(&dev_ms, span.a, span.b);
    /* host_us: everything up to the first launch of the cast phase, plus each part's projection when the
     * parts are projected again; device_us: the event span of the cast phase less that */
    const double host_us = t1 - t0 + cast_host_us;
    const double device_us = std::max(0.0, dev_ms * 1e3 - cast_host_us);
    if (ginfo) {
        std::memset(ginfo, 0, sizeof(*ginfo));
        ginfo->parts = (int32_t)parts->size();
        ginfo->max_hits_per_cell = (int32_t)counters[kGmapMaxHits];
        ginfo->direct_cells = (int64_t)counters[kGmapDirect];
        ginfo->sorted_cells = (int64_t)counters[kGmapSorted];
        ginfo->tiled_cells = (int64_t)counters[kGmapTiled];
        ginfo->beams = beams_all;
        ginfo->host_us = host_us;
        ginfo->device_us = device_us;
    }
    if ((rc = map_finish(ctx, whole, counters, info))) return rc;
    if (info) {
        info->host_us = host_us;
        info->device_us = device_us;
    }
    return CSM_OK;
}

} /* extern "C" */
