/* csm_map_batch_api.hip -- host side of csm_construct_maps_from_scans and its planner
 * csm_host_map_batch_plan (include/csm_hip.h), with their kernels
 * (csm_map_batch_kernels.hip). A translation unit of libcsm_hip.so of its own.
 *
 * Per job the host steps are the functions map_build runs (csm_map_build.hpp, keep_cells = false);
 * each runs for a whole chunk of jobs before the next one starts, so that the device sees one
 * launch per step and the host two read-backs per chunk. What this file keeps: the chunk's
 * scratch layout, prefix tables and shared scans, the launches, one synchronise per chunk where
 * the single call has one per map, and a refused job leaving the chunk while the others go on. */
#include "csm_map_build.hpp"

#include "csm_map_batch_kernels.hip"

namespace {

constexpr int64_t kMapBatchDefaultLimit = 1ll << 30;
constexpr int64_t kMapCellsMax = 1ll << 28;      /* csm_host_map_resize refuses more */

int64_t map_list_words(int64_t n_rays)           /* a map's lists + hit-cell list, whole uint4s */
{
    return (11 * n_rays + 23) & ~3ll;
}

int64_t map_job_scratch(int64_t n_beams, int64_t n_cells)
{
    const int64_t n = std::max<int64_t>(n_beams, 1);
    return n * (int64_t)(sizeof(MapRay) + sizeof(MapRayRec)) + 4 * map_list_words(n_beams) + 12 * n_cells +
           8 * (int64_t)kMapCounters;
}

/* one job on its way through a chunk: the build's state and the job's places in the chunk's buffers */
struct BatchJob : MapBuild {
    int index = 0;                         /* in the caller's array */
    int64_t cells_upper = 0;
    size_t ray0 = 0, node0 = 0, unc0 = 0;  /* its first ray, node and uncertain-list word */
    size_t cell0 = 0, list0 = 0;
    DevBuf carried;                        /* the old map's allocation bitmap until the new one is built */
    bool live = true;
    std::string error;
};

/* a step refused the job (its message is in ctx->err): the chunk goes on without it */
int job_fail(csm_ctx* ctx, csm_map_build_job& job, BatchJob& b, int code)
{
    job.status = code;
    b.live = false;
    b.error = ctx->err;
    return code;
}

/* the checks and the node table, then the planner's bound on the cells */
void prepare_job(csm_ctx* ctx, csm_map_build_job& job, const csm_map_builder_params* prm, BatchJob& b)
{
    b.map_id = job.map_id;
    b.shape = &job.shape;
    b.map_pose = job.global_map_pose;
    b.nodes = job.nodes;
    b.n_nodes = job.n_nodes;
    if (int rc = map_node_table(ctx, prm, b)) {
        job_fail(ctx, job, b, rc);
        return;
    }
    /* csm_hip.h: every hit point lies within `reach` of its sensor */
    const double big = std::numeric_limits<double>::max();
    double reach = 0.0, lo_x = big, lo_y = big, hi_x = -big, hi_y = -big;
    for (const MapNode& t : b.table) {
        if (t.max_range > t.min_range)
            reach = std::max(reach, t.max_range);
        lo_x = std::min(lo_x, t.x);
        lo_y = std::min(lo_y, t.y);
        hi_x = std::max(hi_x, t.x);
        hi_y = std::max(hi_y, t.y);
    }
    const double block = (double)(1 << job.shape.log2_block_size), res = job.shape.resolution;
    const double cols = std::ceil((hi_x - lo_x + 2.0 * reach + 2.0 * res) / res) + 2.0 + 2.0 * block;
    const double rows = std::ceil((hi_y - lo_y + 2.0 * reach + 2.0 * res) / res) + 2.0 + 2.0 * block;
    const double cells = rows * cols;
    b.cells_upper = cells >= 1.0 && cells < (double)kMapCellsMax ? (int64_t)cells : kMapCellsMax;
}

/* One chunk: the jobs chunk[0 .. n) (all live) from the projection to the counters. */
int run_chunk(csm_ctx* ctx, csm_map_build_job* jobs, BatchJob** chunk, int n,
              const csm_map_builder_params* prm, csm_map_batch_info* binfo)
{
    const double t0 = clock_us();
    const int scale = prm->subpixel_scale;
    int rc = 0, e = 0;
    const uint32_t unc_cap = map_unc_cap(ctx);

    /* ---- the chunk's scratch that does not depend on the cell counts ---- */
    size_t n_rays_all = 0, n_nodes_all = 0, n_unc_words = 0, list_words_all = 0;
    for (int j = 0; j < n; ++j) {
        BatchJob& b = *chunk[j];
        b.ray0 = n_rays_all;
        b.node0 = n_nodes_all;
        b.unc0 = n_unc_words;
        b.list0 = list_words_all;
        n_rays_all += (size_t)std::max(b.n_beams, 1);
        n_nodes_all += (size_t)b.n_nodes;
        n_unc_words += std::min<size_t>(unc_cap, (size_t)std::max(b.n_beams, 1));
        list_words_all += (size_t)map_list_words(b.n_beams);
    }
    if ((rc = ensure(ctx, ctx->m_rays, n_rays_all * sizeof(MapRay) + n_nodes_all * (sizeof(MapNode) + 16) + 64))) return rc;
    if ((rc = ensure(ctx, ctx->m_recs, n_rays_all * sizeof(MapRayRec)))) return rc;
    if ((rc = ensure(ctx, ctx->m_lists, list_words_all * sizeof(uint32_t)))) return rc;
    if ((rc = ensure(ctx, ctx->m_cnt, (size_t)n * (kMapCounters * sizeof(unsigned long long) + 32) + n_unc_words * 4 + 64))) return rc;
    MapRay* d_rays = reinterpret_cast<MapRay*>(ctx->m_rays.p);
    MapNode* d_nodes = reinterpret_cast<MapNode*>(d_rays + n_rays_all);
    long long* d_node_src = reinterpret_cast<long long*>(d_nodes + n_nodes_all);
    unsigned long long* d_counters = reinterpret_cast<unsigned long long*>(ctx->m_cnt.p);
    int32_t* d_box = reinterpret_cast<int32_t*>(d_counters + (size_t)n * kMapCounters);   /* per map [4] + count + spread + 2 */
    uint32_t* d_unc_list = reinterpret_cast<uint32_t*>(d_box + (size_t)n * 8);

    /* the device tables: MapProjJob[n] MapJob[n], then six uint32 tables of n + 1 */
    const size_t tab_words = (size_t)(n + 1);
    const size_t tab_bytes = (size_t)n * (sizeof(MapProjJob) + sizeof(MapJob)) + 6 * tab_words * 4;
    if ((rc = ensure(ctx, ctx->m_btab, tab_bytes))) return rc;
    std::vector<unsigned char> tab_host(tab_bytes, 0);
    MapProjJob* h_proj = reinterpret_cast<MapProjJob*>(tab_host.data());
    MapJob* h_jobs = reinterpret_cast<MapJob*>(h_proj + n);
    uint32_t* h_pre = reinterpret_cast<uint32_t*>(h_jobs + n);      /* beam, ray, cell, group, apply */
    MapBatchTable tab;
    std::memset(&tab, 0, sizeof(tab));
    tab.proj = reinterpret_cast<const MapProjJob*>(ctx->m_btab.p);
    tab.jobs = reinterpret_cast<const MapJob*>(tab.proj + n);
    tab.n_maps = n;
    uint32_t* d_pre = reinterpret_cast<uint32_t*>(const_cast<MapJob*>(tab.jobs) + n);
    tab.pre_beam = d_pre;
    tab.pre_ray = d_pre + tab_words;
    tab.pre_cell = d_pre + 2 * tab_words;
    tab.pre_group = d_pre + 3 * tab_words;
    tab.pre_apply = d_pre + 4 * tab_words;
    tab.hit_prefix = d_pre + 5 * tab_words;

    /* all node tables of the chunk, one after the other */
    std::vector<MapNode> nodes_host(n_nodes_all);
    auto gather_nodes = [&]() {
        for (int j = 0; j < n; ++j)
            std::copy(chunk[j]->table.begin(), chunk[j]->table.end(), nodes_host.begin() + (long)chunk[j]->node0);
    };

    /* ---- hit points + bounding boxes (grid_map_builder.cpp:614-638), one launch ---- */
    std::vector<int32_t> boxes((size_t)n * 8);
    uint32_t beam_blocks = 0;
    {
        /* every distinct scan of the chunk once: angles, then ranges */
        ScanTable scans;                                /* its users are the chunk's nodes */
        std::vector<const csm_scan*> scan_of(n_nodes_all, nullptr);
        std::vector<long long> node_src(2 * n_nodes_all, 0);
        for (int j = 0; j < n; ++j) {
            BatchJob& b = *chunk[j];
            h_pre[j] = beam_blocks;
            if (!b.device_projection)
                continue;
            beam_blocks += (uint32_t)ceil_div(b.n_beams, 256);
            const csm_scan_node* nodes = jobs[b.index].nodes;
            for (int k = 0; k < b.n_nodes; ++k) {
                const csm_scan& sc = nodes[k].scan;
                const long long at = 2 * scans.slot(sc, (int)(b.node0 + k));
                scan_of[b.node0 + k] = &sc;
                node_src[2 * (b.node0 + k)] = at;
                node_src[2 * (b.node0 + k) + 1] = at + sc.n_points;
            }
        }
        std::vector<double> stage;
        stage.reserve(2 * (size_t)scans.beams);
        for (int node : scans.first_use) {
            const csm_scan& sc = *scan_of[node];
            stage.insert(stage.end(), sc.angles, sc.angles + sc.n_points);
            stage.insert(stage.end(), sc.ranges, sc.ranges + sc.n_points);
        }
        h_pre[n] = beam_blocks;
        if (beam_blocks) {
            if ((rc = ensure(ctx, ctx->scan_dev, stage.size() * sizeof(double) + 64))) return rc;
            double* d_scan = reinterpret_cast<double*>(ctx->scan_dev.p);
            for (int j = 0; j < n; ++j) {
                BatchJob& b = *chunk[j];
                int32_t* ib = boxes.data() + (size_t)j * 8;
                for (int k = 0; k < 8; ++k)
                    ib[k] = k < 4 ? b.box[k] : 0;
                MapProjJob& pj = h_proj[j];
                pj.angles = pj.ranges = d_scan;
                pj.nodes = d_nodes + b.node0;
                pj.n_nodes = b.n_nodes;
                pj.n_beams = b.n_beams;
                pj.rays = d_rays + b.ray0;
                pj.off_x = jobs[b.index].shape.offset_x;
                pj.off_y = jobs[b.index].shape.offset_y;
                pj.res = jobs[b.index].shape.resolution;
                pj.scaled_res = pj.res / scale;             /* ScaledGeometry, grid_map_geometry.cpp:46-58 */
                pj.box = d_box + (size_t)j * 8;
                pj.unc_count = reinterpret_cast<uint32_t*>(pj.box + 4);
                pj.unc_list = d_unc_list + b.unc0;
                pj.unc_cap = unc_cap;
                pj.node_src = d_node_src + 2 * b.node0;
            }
            gather_nodes();
            HIP_TRY(ctx, hipMemcpyAsync(d_scan, stage.data(), stage.size() * sizeof(double),
                                        hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(d_nodes, nodes_host.data(), nodes_host.size() * sizeof(MapNode),
                                        hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(d_node_src, node_src.data(), node_src.size() * sizeof(long long),
                                        hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(d_box, boxes.data(), boxes.size() * 4, hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(ctx->m_btab.p, tab_host.data(), tab_bytes, hipMemcpyHostToDevice, ctx->stream));
            {
                ScopedTimer tm(ctx, "map_batch_project");
                e = launch(k_mapb_project, dim3(beam_blocks), dim3(256), ctx->stream, tab);
            }
            if ((rc = launched_ok(ctx, e, "map batch project"))) return rc;
            /* the one read-back of the projection: every map's box, count and spread bits */
            HIP_TRY(ctx, hipMemcpyAsync(boxes.data(), d_box, boxes.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            if (binfo)
                binfo->scan_bytes_uploaded += (int64_t)(stage.size() * sizeof(double));
        }
    }
    /* each map under the single call's rules: projected on the host, or its uncertain beams listed */
    std::vector<std::vector<uint32_t>> unc_lists((size_t)n);
    bool any_unc = false;
    for (int j = 0; j < n; ++j) {
        BatchJob& b = *chunk[j];
        if (!b.device_projection)
            continue;
        map_take_projection(b, boxes.data() + (size_t)j * 8, unc_cap);
        if (b.n_unc) {
            unc_lists[j].resize(b.n_unc);
            HIP_TRY(ctx, hipMemcpyAsync(unc_lists[j].data(), d_unc_list + b.unc0, (size_t)b.n_unc * 4,
                                        hipMemcpyDeviceToHost, ctx->stream));
            any_unc = true;
        }
    }
    if (any_unc)
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<std::vector<MapRay>> patches((size_t)n);    /* sources of asynchronous uploads */
    bool uploads = false;
    for (int j = 0; j < n; ++j) {
        BatchJob& b = *chunk[j];
        if ((rc = map_patch_rays(ctx, b, unc_lists[j].data(), d_rays + b.ray0, patches[j], uploads))) return rc;
        if (!b.device_projection && binfo)
            ++binfo->host_projection_jobs;
    }
    if (uploads)
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    patches.clear();

    /* ---- resize every map on the host; a refused job leaves the chunk here ---- */
    for (int j = 0; j < n; ++j)
        if ((rc = map_resize(ctx, *chunk[j], scale)))
            job_fail(ctx, jobs[chunk[j]->index], *chunk[j], rc);

    if ((rc = map_ensure_tables(ctx, prm))) return rc;
    uint16_t* d_lut = reinterpret_cast<uint16_t*>(ctx->m_lut.p);
    if (!ctx->m_cus) {
        int cus = 0;
        HIP_TRY(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
        ctx->m_cus = std::max(cus, 1);
    }

    /* ---- per map: the carried allocation (it waits in the job's own buffer: many are alive at once)
     * and the destination grid; at most one synchronise for the chunk ---- */
    size_t n_cells_all = 0;
    bool synced = false;
    for (int j = 0; j < n; ++j) {
        BatchJob& b = *chunk[j];
        if (!b.live)
            continue;
        if ((rc = map_claim_grid(ctx, b, b.carried, synced))) return rc;
        b.cell0 = n_cells_all;
        n_cells_all += b.n_cells;
    }

    /* ---- the update chain, once for the chunk ---- */
    if ((rc = ensure(ctx, ctx->m_cell, 3 * std::max<size_t>(n_cells_all, 1) * sizeof(uint32_t)))) return rc;
    uint32_t* d_cell = reinterpret_cast<uint32_t*>(ctx->m_cell.p);
    std::vector<unsigned long long> counters((size_t)n * kMapCounters, 0ull);
    uint32_t ray_blocks = 0, cell_blocks = 0, groups = 0, apply_blocks = 0;
    long long usable_all = 0;
    int n_live = 0;
    for (int j = 0; j < n; ++j) {
        BatchJob& b = *chunk[j];
        uint32_t* pre = h_pre + tab_words;      /* ray, cell, group, apply follow the beam table */
        pre[j] = ray_blocks;
        pre[tab_words + j] = cell_blocks;
        pre[2 * tab_words + j] = groups;
        pre[3 * tab_words + j] = apply_blocks;
        counters[(size_t)j * kMapCounters + kMapKnownRow] = counters[(size_t)j * kMapCounters + kMapKnownCol] = ~0ull;
        /* a job refused above stays in the tables with no workgroup of any step and no cell with hits,
         * but k_mapb_hit_prefix reads every map's count: its counter block must be a real one */
        h_jobs[j].counters = d_counters + (size_t)j * kMapCounters;
        if (!b.live)
            continue;
        ++n_live;
        MapJob& mj = h_jobs[j];
        mj.rays = d_rays + b.ray0;
        mj.nodes = d_nodes + b.node0;
        mj.recs = reinterpret_cast<MapRayRec*>(ctx->m_recs.p) + b.ray0;
        mj.n_hit = d_cell + 2 * b.cell0;        /* n_hit and n_miss of all maps first (one memset), then seg */
        mj.n_miss = mj.n_hit + b.n_cells;
        mj.seg = d_cell + 2 * n_cells_all + b.cell0;
        mj.lists = reinterpret_cast<uint32_t*>(ctx->m_lists.p) + b.list0;
        map_fill_job(b, scale, d_lut, mj);      /* ray numbers, cell ids and slots are local to the map */
        if (b.n_beams) {
            ray_blocks += (uint32_t)ceil_div(b.n_beams, 256);
            cell_blocks += (uint32_t)((b.n_cells + 255) / 256);
            groups += (uint32_t)ceil_div(b.n_beams, kMapGroup);
        }
        apply_blocks += (uint32_t)(((size_t)mj.rows * mj.pitch + 255) / 256);
        usable_all += b.usable;
    }
    {
        uint32_t* pre = h_pre + tab_words;
        pre[n] = ray_blocks;
        pre[tab_words + n] = cell_blocks;
        pre[2 * tab_words + n] = groups;
        pre[3 * tab_words + n] = apply_blocks;
    }
    const double t1 = clock_us();
    float dev_ms = 0.f;
    if (n_live) {
        CallSpan span(ctx);
        if (!span.a || !span.b)
            return fail(ctx, CSM_EIO, "map batch: no event for device_us");
        gather_nodes();
        HIP_TRY(ctx, hipEventRecord(span.a, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_nodes, nodes_host.data(), nodes_host.size() * sizeof(MapNode),
                                    hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_counters, counters.data(), counters.size() * sizeof(unsigned long long),
                                    hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->m_btab.p, tab_host.data(), tab_bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(d_cell, 0, 2 * n_cells_all * sizeof(uint32_t), ctx->stream));
        {
            ScopedTimer tm(ctx, "map_batch_build");
            if (ray_blocks) {
                keep_first(e, launch(k_mapb_hits, dim3(ray_blocks), dim3(256), ctx->stream, tab));
                keep_first(e, launch(k_mapb_alloc, dim3(cell_blocks), dim3(256), ctx->stream, tab));
                keep_first(e, launch(k_mapb_fill_hits, dim3(ray_blocks), dim3(256), ctx->stream, tab));
                keep_first(e, launch(k_mapb_rank_hits, dim3(ray_blocks), dim3(256), ctx->stream, tab));
                keep_first(e, launch(k_mapb_walk, dim3(groups), dim3(512), ctx->stream, tab));
            }
            keep_first(e, launch(k_mapb_apply, dim3(apply_blocks), dim3(256), ctx->stream, tab));
            if (usable_all > 0) {
                /* one workgroup per CU at most, the hit table loaded once each; the kernel spreads the
                 * chunk's cells with hits over their wavefronts */
                const unsigned wgs = (unsigned)std::min<long long>(
                    ctx->m_cus, (std::min<long long>(usable_all, (long long)n_cells_all) + 3) / 4);
                keep_first(e, launch(k_mapb_hit_prefix, dim3(1), dim3(256), ctx->stream, tab));
                keep_first(e, launch_lds(ctx->device, k_mapb_apply_hits, dim3(wgs), dim3(256), 65536 * sizeof(uint16_t),
                                         ctx->stream, tab, (const uint16_t*)d_lut));
            }
            if ((rc = launched_ok(ctx, e, "map batch build"))) return rc;
            for (int j = 0; j < n; ++j)
                if (chunk[j]->live && (rc = map_carry_allocation(ctx, *chunk[j], chunk[j]->carried))) return rc;
        }
        HIP_TRY(ctx, hipEventRecord(span.b, ctx->stream));
        /* the one read-back of the update: every map's counter block */
        HIP_TRY(ctx, hipMemcpyAsync(counters.data(), d_counters, counters.size() * sizeof(unsigned long long),
                                    hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        (void)hipEventElapsedTime(&dev_ms, span.a, span.b);
    }
    const double host_us = t1 - t0;
    if (binfo) {
        ++binfo->chunks;
        binfo->host_us += host_us;
        binfo->device_us += dev_ms * 1e3;
    }
    for (int j = 0; j < n; ++j) {
        BatchJob& b = *chunk[j];
        if (!b.live)
            continue;
        csm_map_build_job& job = jobs[b.index];
        if ((rc = map_finish(ctx, b, counters.data() + (size_t)j * kMapCounters, &job.info))) {
            job_fail(ctx, job, b, rc);
            continue;
        }
        job.info.host_us = host_us / std::max(n_live, 1);
        job.info.device_us = dev_ms * 1e3 / std::max(n_live, 1);
        job.status = CSM_OK;
    }
    return CSM_OK;
}

} /* namespace */

extern "C" {

int csm_host_map_batch_plan(const int64_t* n_beams, const int64_t* n_cells_upper, int32_t n_jobs,
                            int64_t scratch_limit_bytes, int32_t* chunk_of, int64_t* chunk_bytes,
                            int32_t* n_chunks)
{
    if (!n_beams || !n_cells_upper || n_jobs < 1 || scratch_limit_bytes < 0 || !chunk_of || !chunk_bytes || !n_chunks)
        return CSM_EINVAL;
    for (int j = 0; j < n_jobs; ++j)
        if (n_beams[j] < 0 || n_cells_upper[j] < 0 || n_beams[j] > (1ll << 24) || n_cells_upper[j] > kMapCellsMax)
            return CSM_EINVAL;
    const int64_t limit = scratch_limit_bytes ? scratch_limit_bytes : kMapBatchDefaultLimit;
    int chunk = 0;
    int64_t held = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const int64_t need = map_job_scratch(n_beams[j], n_cells_upper[j]);
        if (j > 0 && held + need > limit) {
            chunk_bytes[chunk++] = held;
            held = 0;
        }
        held += need;
        chunk_of[j] = chunk;
    }
    chunk_bytes[chunk++] = held;
    *n_chunks = chunk;
    return CSM_OK;
}

int csm_construct_maps_from_scans(csm_ctx* ctx, csm_map_build_job* jobs, int32_t n_jobs,
                                  const csm_map_builder_params* prm, const csm_map_batch_params* bp,
                                  csm_map_batch_info* info)
{
    if (!ctx || !jobs || n_jobs < 1 || !prm || prm->subpixel_scale < 1 || prm->subpixel_scale > 1024 ||
        (bp && bp->scratch_limit_bytes < 0))
        return fail(ctx, CSM_EINVAL, "map batch: bad arguments");
    {
        std::vector<uint64_t> ids((size_t)n_jobs);
        for (int j = 0; j < n_jobs; ++j)
            ids[j] = jobs[j].map_id;
        std::sort(ids.begin(), ids.end());
        if (std::adjacent_find(ids.begin(), ids.end()) != ids.end())
            return fail(ctx, CSM_EINVAL, "map batch: the same map_id in two jobs");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    csm_map_batch_info local;
    std::memset(&local, 0, sizeof(local));
    std::vector<BatchJob> state((size_t)n_jobs);
    std::vector<BatchJob*> live;
    for (int j = 0; j < n_jobs; ++j) {
        state[j].index = j;
        jobs[j].status = CSM_OK;
        std::memset(&jobs[j].info, 0, sizeof(jobs[j].info));
        prepare_job(ctx, jobs[j], prm, state[j]);
        if (state[j].live)
            live.push_back(&state[j]);
    }
    int rc = CSM_OK;
    if (!live.empty()) {
        const int n = (int)live.size();
        std::vector<int64_t> beams((size_t)n), cells((size_t)n), chunk_bytes((size_t)n);
        std::vector<int32_t> chunk_of((size_t)n);
        int32_t n_chunks = 0;
        for (int j = 0; j < n; ++j) {
            beams[j] = live[j]->n_beams;
            cells[j] = live[j]->cells_upper;
        }
        rc = csm_host_map_batch_plan(beams.data(), cells.data(), n, bp ? bp->scratch_limit_bytes : 0,
                                     chunk_of.data(), chunk_bytes.data(), &n_chunks);
        if (rc != CSM_OK)
            return fail(ctx, rc, "map batch: internal: the plan was refused");
        for (int first = 0; first < n;) {
            int last = first;
            while (last < n && chunk_of[last] == chunk_of[first])
                ++last;
            if ((rc = run_chunk(ctx, jobs, live.data() + first, last - first, prm, &local))) {
                /* a device or allocation failure: the jobs of this chunk that had not been refused and
                 * those of the chunks behind it were not built (their maps may be gone) */
                for (int j = first; j < n; ++j)
                    if (live[j]->live)
                        jobs[live[j]->index].status = rc;
                if (info)
                    *info = local;
                return rc;
            }
            first = last;
        }
    }
    if (info)
        *info = local;
    /* as the loop of single calls: the first status that is not CSM_OK, the last failure's message */
    for (int j = n_jobs - 1; j >= 0; --j)
        if (jobs[j].status != CSM_OK) {
            ctx->err = state[j].error;
            break;
        }
    for (int j = 0; j < n_jobs; ++j)
        if (jobs[j].status != CSM_OK)
            return jobs[j].status;
    return CSM_OK;
}

} /* extern "C" */
