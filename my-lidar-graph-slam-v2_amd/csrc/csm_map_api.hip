/* csm_map_api.hip -- host side of the map updates: csm_construct_map_from_scans
 * and csm_update_map_with_scan (include/csm_hip.h), with their kernels
 * (csm_map_kernels.hip). A translation unit of libcsm_hip.so of its own. */
#include "csm_map_build.hpp"

#include "csm_map_kernels.hip"

/* ---- map building ---- */

namespace {

/* GridBinaryBayes's conversions (src/grid_map_new/grid_binary_bayes.cpp:345-383,
 * inc/grid_map_new/grid_values.hpp:11-46) with its constants: values 1..65535
 * stand for probabilities 0.001..0.999, 0 = unknown. */
const double kBayesProbMin = 1e-3;
const double kBayesProbMax = 1.0 - 1e-3;

double bayes_probability_to_odds(double prob)
{
    if (prob == 0.0)
        return 1.0;
    if (prob < kBayesProbMin)
        return kBayesProbMin / (1.0 - kBayesProbMin);
    if (prob > kBayesProbMax)
        return kBayesProbMax / (1.0 - kBayesProbMax);
    return prob / (1.0 - prob);
}

uint16_t bayes_value_after(uint32_t value, double odds)
{
    /* GridBinaryBayes::UpdateOddsUnchecked (grid_binary_bayes.cpp:302-321) */
    double now = odds;
    if (value != 0) {
        const double p = kBayesProbMin + (kBayesProbMax - kBayesProbMin) *
                         static_cast<double>(static_cast<int>(value) - 1) / 65534.0;
        now = (p / (1.0 - p)) * odds;
    }
    double prob = 0.0;
    if (!(now < 0.0))
        prob = std::min(std::max(now / (1.0 + now), kBayesProbMin), kBayesProbMax);
    if (prob == 0.0)
        return 0;
    if (prob < kBayesProbMin)
        return 1;
    if (prob > kBayesProbMax)
        return 65535;
    return static_cast<uint16_t>(1 + (prob - kBayesProbMin) * 65534.0 / (kBayesProbMax - kBayesProbMin));
}

/* GridMap<T>::IndexToBlock (src/grid_map_new/grid_map.cpp:804-814): a negative
 * index lands one block further out than a floor would put it */
int map_index_to_block(int idx, int log2_block)
{
    return idx >= 0 ? (idx >> log2_block) : ((idx >> log2_block) - 1);
}

} /* namespace */

namespace csm_host {

/* the two value -> value tables of the cell update, in ctx->m_lut, for prm's probabilities */
int map_ensure_tables(csm_ctx* ctx, const csm_map_builder_params* prm)
{
    if (int rc = ensure(ctx, ctx->m_lut, 2 * 65536 * sizeof(uint16_t)))
        return rc;
    uint16_t* d_lut = reinterpret_cast<uint16_t*>(ctx->m_lut.p);
    if (ctx->m_lut_hit != prm->prob_hit || ctx->m_lut_miss != prm->prob_miss) {
        std::vector<uint16_t> tab(2 * 65536);
        const double odds_hit = bayes_probability_to_odds(prm->prob_hit);     /* grid_map_builder.cpp:95-96 */
        const double odds_miss = bayes_probability_to_odds(prm->prob_miss);
        for (uint32_t v = 0; v < 65536; ++v) {
            tab[v] = bayes_value_after(v, odds_hit);
            tab[65536 + v] = bayes_value_after(v, odds_miss);
        }
        HIP_TRY(ctx, hipMemcpyAsync(d_lut, tab.data(), tab.size() * 2, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        ctx->m_lut_hit = prm->prob_hit;
        ctx->m_lut_miss = prm->prob_miss;
    }
    return CSM_OK;
}

/* ---- the steps of a build, on one map (csm_map_build.hpp) ---- */

int map_node_table(csm_ctx* ctx, const csm_map_builder_params* prm, MapBuild& m)
{
    const csm_map_shape& shape = *m.shape;
    if (!m.nodes || m.n_nodes < 1 || !(shape.resolution > 0.0) || shape.log2_block_size < 0 ||
        shape.log2_block_size > 12)
        return fail(ctx, CSM_EINVAL, "map build: bad arguments");
    if (m.keep_cells) {
        const DeviceGrid* have = find_grid(ctx, m.map_id);
        if (!have || have->levels.empty())
            return fail(ctx, CSM_ENOENT, "map %llu not resident", (unsigned long long)m.map_id);
        if (have->rows != shape.rows || have->cols != shape.cols)
            return fail(ctx, CSM_EINVAL, "shape %d x %d does not match the resident map %d x %d",
                        shape.rows, shape.cols, have->rows, have->cols);
    }
    /* grid_map_builder.cpp:583-612: sensor poses, usable ranges */
    m.table.resize((size_t)m.n_nodes);
    long long n_beams_ll = 0, usable = 0;
    for (int k = 0; k < m.n_nodes; ++k) {
        const csm_scan_node& nd = m.nodes[k];
        if (!nd.scan.angles || !nd.scan.ranges || nd.scan.n_points < 0)
            return fail(ctx, CSM_EINVAL, "scan node %d has no scan", k);
        double global_sensor[3], local_sensor[3];
        csm_host_compound(nd.global_pose, nd.scan.relative_sensor_pose, global_sensor);
        csm_host_inverse_compound(m.map_pose, global_sensor, local_sensor);
        MapNode& t = m.table[k];
        t.x = local_sensor[0];
        t.y = local_sensor[1];
        t.theta = local_sensor[2];
        t.min_range = std::max(prm->usable_range_min, nd.min_range);
        t.max_range = std::min(prm->usable_range_max, nd.max_range);
        t.beam_base = (int32_t)n_beams_ll;
        t.n_beams = nd.scan.n_points;
        t.sx = t.sy = 0;
        n_beams_ll += nd.scan.n_points;
        for (int i = 0; i < nd.scan.n_points; ++i) {
            const double r = nd.scan.ranges[i];
            usable += !(r >= t.max_range || r <= t.min_range);
        }
    }
    if (n_beams_ll > (1ll << 24))
        return fail(ctx, CSM_EINVAL, "%lld beams in one map build", n_beams_ll);
    m.n_beams = (int)n_beams_ll;
    m.usable = usable;
    /* ---- hit points + bounding box (grid_map_builder.cpp:614-638) ----
     * In index form: Resize(BoundingBox<double>) (grid_map.cpp:892-913) takes
     * floor((min - res - off) / res) and floor((max + res - off) / res), and that
     * expression is monotone, so the box is the min / max of it over the points. */
    m.min_x = m.min_y = std::numeric_limits<double>::max();
    m.max_x = m.max_y = std::numeric_limits<double>::min();   /* as the reference: smallest positive */
    if (m.keep_cells) {
        /* ComputeBoundingBoxAndScanPointsMapLocal starts from the sensor position (:835-841) */
        m.min_x = m.max_x = m.table[0].x;
        m.min_y = m.max_y = m.table[0].y;
    }
    for (const MapNode& t : m.table)
        m.add_point(t.x, t.y);
    for (int k = 0; k < 4; ++k)
        m.box[k] = k < 2 ? 0x7fffffff : -0x7fffffff - 1;
    m.device_projection = m.n_beams > 0 && !ctx->tune.map_host_projection;
    return CSM_OK;
}

void map_take_projection(MapBuild& m, const int32_t got[8], uint32_t unc_cap)
{
    m.n_unc = (uint32_t)got[4];
    m.spread_known = ((uint32_t)got[5] & 3u) == 3u;     /* the box of the certified beams is certainly not degenerate */
    if (m.n_unc > unc_cap || !m.spread_known) {
        m.device_projection = false;        /* too many beams on cell edges, or a degenerate box: all on the host */
        m.n_unc = 0;
        return;
    }
    for (int k = 0; k < 4; ++k)
        m.box[k] = got[k];
}

int map_patch_rays(csm_ctx* ctx, MapBuild& m, const uint32_t* list, MapRay* d_rays, std::vector<MapRay>& src,
                   bool& uploads)
{
    /* ScanData::HitPoint with glibc (csm_certify.hpp) */
    auto hit_point = [&m](int k, int i, MapRay& ray) {
        const MapNode& t = m.table[k];
        host_hit_point(t.x, t.y, t.theta, m.nodes[k].scan.ranges[i], m.nodes[k].scan.angles[i], &ray.hx, &ray.hy);
        ray.node = k;
        ray.usable = 1;
        m.add_point(ray.hx, ray.hy);
    };
    if (m.device_projection) {
        /* the beams the device could not certify: exactly as the reference, and patched in */
        src.resize(m.n_unc);
        for (uint32_t u = 0; u < m.n_unc; ++u) {
            const uint32_t b = list[u];
            int k = 0;
            while (k + 1 < m.n_nodes && m.table[k + 1].beam_base <= (int32_t)b)
                ++k;
            hit_point(k, (int)b - m.table[k].beam_base, src[u]);
            HIP_TRY(ctx, hipMemcpyAsync(d_rays + b, &src[u], sizeof(MapRay), hipMemcpyHostToDevice, ctx->stream));
        }
        uploads |= m.n_unc > 0;
        return CSM_OK;
    }
    /* host projection */
    src.resize((size_t)std::max(m.n_beams, 1));
    for (int k = 0; k < m.n_nodes; ++k) {
        const MapNode& t = m.table[k];
        for (int i = 0; i < t.n_beams; ++i) {
            MapRay& ray = src[(size_t)t.beam_base + i];
            ray.hx = ray.hy = 0.0;
            ray.node = k;
            ray.usable = 0;
            const double r = m.nodes[k].scan.ranges[i];
            if (!(r >= t.max_range || r <= t.min_range))
                hit_point(k, i, ray);
        }
    }
    for (int k = 0; k < 4; ++k)
        m.box[k] = k < 2 ? 0x7fffffff : -0x7fffffff - 1;
    m.spread_known = false;
    if (m.n_beams) {
        HIP_TRY(ctx, hipMemcpyAsync(d_rays, src.data(), (size_t)m.n_beams * sizeof(MapRay), hipMemcpyHostToDevice,
                                    ctx->stream));
        uploads = true;
    }
    return CSM_OK;
}

int map_resize(csm_ctx* ctx, MapBuild& m, int scale)
{
    const csm_map_shape& shape = *m.shape;
    const double res = shape.resolution, scaled_res = res / scale;   /* ScaledGeometry, grid_map_geometry.cpp:46-58 */
    auto to_index = [res](double p, double off) { return cell_index(p, off, res); };
    /* Assert(min < max) of Resize: the host-side points decide unless the certified
     * beams are known to spread in both axes */
    if (!m.spread_known && (!(m.min_x < m.max_x) || !(m.min_y < m.max_y)))
        return fail(ctx, CSM_EINVAL, "empty bounding box (the reference asserts)");
    if (m.min_x <= m.max_x) {               /* points the host holds as doubles (always: the sensors) */
        m.box[0] = std::min(m.box[0], to_index(m.min_x - res, shape.offset_x));
        m.box[1] = std::min(m.box[1], to_index(m.min_y - res, shape.offset_y));
        m.box[2] = std::max(m.box[2], to_index(m.max_x + res, shape.offset_x));
        m.box[3] = std::max(m.box[3], to_index(m.max_y + res, shape.offset_y));
    }
    /* GridMap::Resize(BoundingBox<int>) / GridMap::Expand on the CURRENT geometry */
    m.next = shape;
    if (csm_host_map_resize(&m.next, m.box, m.keep_cells ? 1 : 0, m.shift) != CSM_OK)
        return fail(ctx, CSM_EINVAL, "resized map is out of range");
    m.resized = !m.keep_cells || m.shift[0] != 0 || m.shift[1] != 0 || m.next.rows != shape.rows ||
                m.next.cols != shape.cols;
    for (MapNode& t : m.table) {
        t.sx = cell_index(t.x, m.next.offset_x, scaled_res);
        t.sy = cell_index(t.y, m.next.offset_y, scaled_res);
    }
    m.n_cells = (size_t)m.next.rows * m.next.cols;
    return CSM_OK;
}

int map_claim_grid(csm_ctx* ctx, MapBuild& m, DevBuf& carried, bool& synced)
{
    int rc = 0;
    /* The old map's block allocation, which Resize / Expand move and ResetValues keeps
     * (grid_map.cpp:278-287, 841-889, 915-936): the resident map_id's, if its rows and cols
     * are the shape's; its bitmap if that is on the shape's blocks, else the rule "a block with a
     * known cell is allocated" on them. Otherwise nothing was allocated. */
    const int lb = m.shape->log2_block_size;
    if (DeviceGrid* old = find_grid(ctx, m.map_id)) {
        if (!old->levels.empty() && old->rows == m.shape->rows && old->cols == m.shape->cols) {
            if (old->alloc_derived || old->alloc_log2 != lb) {
                old->alloc_stale |= old->alloc_log2 != lb || !old->alloc_derived;
                old->alloc_derived = true;
                old->alloc_log2 = lb;
            }
            if ((rc = ensure_allocation(ctx, *old))) return rc;
            m.has_carried = true;
            m.carried_brows = (old->rows + (1 << lb) - 1) >> lb;
            m.carried_bcols = old->alloc_bcols;
        }
        std::swap(carried, old->alloc);
        old->alloc_derived = true;          /* until the build has finished */
        old->alloc_stale = true;
    }

    /* the destination grid: keep the old allocation when it is large enough; a new one is
     * built here and registered once the build has succeeded */
    const int rows = m.next.rows, cols = m.next.cols;
    const int pitch = (cols + 7) & ~7;
    const size_t bytes = (size_t)rows * pitch * 2;
    m.dst = find_grid(ctx, m.map_id);
    if (!m.keep_cells && (!m.dst || m.dst->levels.empty() || !m.dst->levels[0].owned() ||
                          m.dst->levels[0].own.cap < bytes)) {
        if (!synced)
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        synced = true;
        m.fresh = take_grid(ctx, m.map_id);
        m.dst = &m.fresh;
        Level base;
        if ((rc = grow(ctx, base.own, bytes + bytes / 2, bytes + bytes / 2, false))) return rc;
        base.cells = base.own.as<uint16_t>();
        m.fresh.levels.push_back(std::move(base));
    }
    DeviceGrid& g = *m.dst;
    if (m.keep_cells && m.resized) {
        /* GridMap::Resize moves the blocks (grid_map.cpp:866-879): the old cells, shifted */
        Level base;
        if ((rc = grow(ctx, base.own, bytes + bytes / 2, bytes + bytes / 2, false))) return rc;
        base.cells = base.own.as<uint16_t>();
        const int shift_r = -m.shift[0], shift_c = -m.shift[1];
        HIP_TRY(ctx, hipMemsetAsync(base.cells, 0, bytes, ctx->stream));
        HIP_TRY(ctx, hipMemcpy2DAsync(base.cells + (size_t)shift_r * pitch + shift_c, (size_t)pitch * 2,
                                      g.levels[0].cells, (size_t)g.pitch * 2, (size_t)g.cols * 2, g.rows,
                                      hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        g.levels[0] = std::move(base);
    }
    for (size_t i = 1; i < g.levels.size(); ++i) {
        if (g.levels[i].owned())
            g.levels[i].stale = true;
        else
            g.levels[i].cells = g.levels[0].cells;     /* an alias of the base (window 1) */
    }
    /* level 0 changes in place or moves: the phase-major copies of the box-max levels would
     * otherwise be taken for current (same level buffer, same epoch) */
    if (!g.phase.empty() && !synced) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        synced = true;
    }
    base_changed(g);
    g.xg_stale = true;         /* the pair-row copy follows the base */
    g.rows = rows;
    g.cols = cols;
    g.pitch = pitch;
    g.known_r0 = 0;
    g.known_c0 = 0;
    return CSM_OK;
}

void map_fill_job(const MapBuild& m, int scale, const uint16_t* d_lut, MapJob& mj)
{
    mj.n_rays = m.n_beams;
    mj.off_x = m.next.offset_x;
    mj.off_y = m.next.offset_y;
    mj.res = m.shape->resolution;
    mj.scaled_res = mj.res / scale;
    mj.scale = scale;
    mj.rows = m.dst->rows;
    mj.cols = m.dst->cols;
    mj.pitch = m.dst->pitch;
    /* per hit cell at most 3n + 7 words (csm_device.hpp: map_block_words), then the hit-cell list */
    mj.hit_cells = mj.lists + 10 * (size_t)m.n_beams + 16;
    mj.lut_hit = d_lut;
    mj.lut_miss = d_lut + 65536;
    mj.cells = m.dst->levels[0].cells;
    mj.keep_cells = m.keep_cells ? 1 : 0;
}

int map_carry_allocation(csm_ctx* ctx, MapBuild& m, const DevBuf& carried)
{
    const int lb = m.shape->log2_block_size;
    return build_allocation(ctx, *m.dst, lb, m.has_carried ? carried.as<uint8_t>() : nullptr, m.carried_brows,
                            m.carried_bcols, m.shift[0] / (1 << lb), m.shift[1] / (1 << lb));
}

int map_finish(csm_ctx* ctx, MapBuild& m, const unsigned long long* counters, csm_map_build_info* info)
{
    if (counters[kMapError]) {
        ctx->grids.erase(m.map_id);         /* the cells may be half updated: drop the map */
        m.fresh = DeviceGrid();
        return fail(ctx, CSM_EINVAL, "a ray leaves the resized map (flags %llu): the reference asserts",
                    counters[kMapError]);
    }
    DeviceGrid& g = *m.dst;
    g.known_r0 = counters[kMapKnownRow] == ~0ull ? g.rows : (int)counters[kMapKnownRow];
    g.known_c0 = counters[kMapKnownCol] == ~0ull ? g.cols : (int)counters[kMapKnownCol];
    m.shape->rows = g.rows;
    m.shape->cols = g.cols;
    m.shape->offset_x = m.next.offset_x;
    m.shape->offset_y = m.next.offset_y;
    if (info) {
        info->rays = m.usable;
        info->cell_updates = info->saturated_reads = 0;
        for (int k = 0; k < kMapStripes; ++k) {
            info->cell_updates += (int64_t)counters[kMapStripedUpdates + k];
            info->saturated_reads += (int64_t)counters[kMapStripedSaturated + k];
        }
        info->first_known_row = g.known_r0;
        info->first_known_col = g.known_c0;
        info->device_projection = m.device_projection ? 1 : 0;
    }
    if (m.dst == &m.fresh)
        ctx->grids[m.map_id] = std::move(m.fresh);
    return CSM_OK;
}

} /* namespace csm_host */

extern "C" {

/* GridMap<T>::Resize(BoundingBox<int>) (src/grid_map_new/grid_map.cpp:841-889) and, with
 * expand != 0, GridMap<T>::Expand (:915-936) in front of it, on index boxes: host only. */
int csm_host_map_resize(csm_map_shape* shape, const int32_t box[4], int32_t expand, int32_t shift_out[2])
{
    if (!shape || !box || shape->log2_block_size < 0 || shape->log2_block_size > 12 ||
        !(shape->resolution > 0.0))
        return CSM_EINVAL;
    const int lb = shape->log2_block_size, block = 1 << lb;
    long long i_min_x = box[0], i_min_y = box[1], i_max_x = (long long)box[2] + 1, i_max_y = (long long)box[3] + 1;
    if (shift_out)
        shift_out[0] = shift_out[1] = 0;
    if (i_min_x >= i_max_x || i_min_y >= i_max_y)
        return CSM_EINVAL;                  /* the reference asserts */
    if (expand) {
        auto inside = [shape](long long row, long long col) {
            return row >= 0 && row < shape->rows && col >= 0 && col < shape->cols;
        };
        if (inside(i_min_y, i_min_x) && inside(i_max_y - 1, i_max_x - 1))
            return CSM_OK;                  /* the box fits: nothing changes */
        i_min_x = std::min(0ll, i_min_x);
        i_min_y = std::min(0ll, i_min_y);
        i_max_x = std::max((long long)shape->cols, i_max_x);
        i_max_y = std::max((long long)shape->rows, i_max_y);
    }
    if (i_min_x < -(1ll << 30) || i_min_y < -(1ll << 30) || i_max_x > (1ll << 30) || i_max_y > (1ll << 30))
        return CSM_EINVAL;
    const int b_min_x = map_index_to_block((int)i_min_x, lb), b_min_y = map_index_to_block((int)i_min_y, lb);
    const int b_max_x = map_index_to_block((int)i_max_x + block - 1, lb);
    const int b_max_y = map_index_to_block((int)i_max_y + block - 1, lb);
    const long long rows = (long long)(b_max_y - b_min_y) << lb, cols = (long long)(b_max_x - b_min_x) << lb;
    if (rows < 1 || cols < 1 || rows * cols > (1ll << 28))
        return CSM_EINVAL;
    shape->rows = (int32_t)rows;
    shape->cols = (int32_t)cols;
    /* GridMapGeometry::Resize (src/grid_map_new/grid_map_geometry.cpp:61-72) */
    shape->offset_x += shape->resolution * (b_min_x * block);      /* b_min may be negative: no shift */
    shape->offset_y += shape->resolution * (b_min_y * block);
    if (shift_out) {
        shift_out[0] = b_min_y * block;
        shift_out[1] = b_min_x * block;
    }
    return CSM_OK;
}

/* Both map updates of GridMapBuilder. keep_cells = false: ConstructMapFromScans
 * (src/mapping/grid_map_builder.cpp:561-695): resize to the scans' bounding box,
 * reset, integrate. keep_cells = true: UpdateGridMap (:389-494): expand only if
 * the scan does not fit, keep the cells, integrate one scan on top. The steps are
 * those of csm_map_build.hpp; here are the launches, one map at a time. */
static int map_build(csm_ctx* ctx, uint64_t map_id, csm_map_shape* shape,
                     const double global_map_pose[3], const csm_scan_node* nodes,
                     int32_t n_nodes, const csm_map_builder_params* prm,
                     csm_map_build_info* info, bool keep_cells)
{
    if (!ctx || !shape || !global_map_pose || !prm || prm->subpixel_scale < 1 || prm->subpixel_scale > 1024)
        return fail(ctx, CSM_EINVAL, "map build: bad arguments");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const double t0 = clock_us();
    const int scale = prm->subpixel_scale;
    int rc = 0, e = 0;
    MapBuild m;
    m.map_id = map_id;
    m.shape = shape;
    m.map_pose = global_map_pose;
    m.nodes = nodes;
    m.n_nodes = n_nodes;
    m.keep_cells = keep_cells;
    if ((rc = map_node_table(ctx, prm, m))) return rc;
    const int n_rays = m.n_beams;

    if ((rc = ensure(ctx, ctx->m_rays, (size_t)std::max(n_rays, 1) * sizeof(MapRay) +
                                           (size_t)n_nodes * sizeof(MapNode) + 64))) return rc;
    if ((rc = ensure(ctx, ctx->m_recs, (size_t)std::max(n_rays, 1) * sizeof(MapRayRec)))) return rc;
    const size_t list_words = 10 * (size_t)n_rays + 16;
    if ((rc = ensure(ctx, ctx->m_lists, (list_words + (size_t)n_rays + 4) * sizeof(uint32_t)))) return rc;
    if ((rc = ensure(ctx, ctx->m_cnt, kMapCounters * sizeof(unsigned long long) + 64 + kMapUncCap * 4))) return rc;
    MapRay* d_rays = reinterpret_cast<MapRay*>(ctx->m_rays.p);
    MapNode* d_nodes = reinterpret_cast<MapNode*>(d_rays + std::max(n_rays, 1));
    unsigned long long* d_counters = reinterpret_cast<unsigned long long*>(ctx->m_cnt.p);
    int32_t* d_box = reinterpret_cast<int32_t*>(d_counters + kMapCounters);   /* [4] + count + spread */
    uint32_t* d_unc = reinterpret_cast<uint32_t*>(d_box + 4);                  /* [0] count, [1] spread bits */
    uint32_t* d_unc_list = d_unc + 4;

    /* ---- hit points + bounding box ---- */
    const uint32_t unc_cap = map_unc_cap(ctx);
    if (m.device_projection) {
        /* scans to the device (one staging copy), projection there */
        std::vector<double> stage(2 * (size_t)n_rays);
        for (int k = 0; k < n_nodes; ++k) {
            std::memcpy(stage.data() + m.table[k].beam_base, nodes[k].scan.angles,
                        (size_t)m.table[k].n_beams * sizeof(double));
            std::memcpy(stage.data() + n_rays + m.table[k].beam_base, nodes[k].scan.ranges,
                        (size_t)m.table[k].n_beams * sizeof(double));
        }
        if ((rc = ensure(ctx, ctx->scan_dev, stage.size() * sizeof(double)))) return rc;
        double* d_scan = reinterpret_cast<double*>(ctx->scan_dev.p);
        const int32_t init_box[8] = { m.box[0], m.box[1], m.box[2], m.box[3], 0, 0, 0, 0 };
        HIP_TRY(ctx, hipMemcpyAsync(d_scan, stage.data(), stage.size() * sizeof(double),
                                    hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_nodes, m.table.data(), m.table.size() * sizeof(MapNode),
                                    hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_box, init_box, sizeof(init_box), hipMemcpyHostToDevice, ctx->stream));
        MapProjJob pj;
        std::memset(&pj, 0, sizeof(pj));
        pj.angles = d_scan;
        pj.ranges = d_scan + n_rays;
        pj.nodes = d_nodes;
        pj.n_nodes = n_nodes;
        pj.n_beams = n_rays;
        pj.rays = d_rays;
        pj.off_x = shape->offset_x;
        pj.off_y = shape->offset_y;
        pj.res = shape->resolution;
        pj.scaled_res = shape->resolution / scale;          /* ScaledGeometry, grid_map_geometry.cpp:46-58 */
        pj.box = d_box;
        pj.unc_count = d_unc;
        pj.unc_list = d_unc_list;
        pj.unc_cap = unc_cap;
        {
            ScopedTimer tm(ctx, "map_project");
            e = launch(k_map_project, dim3((unsigned)ceil_div(n_rays, 256)), dim3(256), ctx->stream, pj);
        }
        if ((rc = launched_ok(ctx, e, "map project"))) return rc;
        int32_t got[8];
        HIP_TRY(ctx, hipMemcpyAsync(got, d_box, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        map_take_projection(m, got, unc_cap);
    }
    {
        std::vector<uint32_t> list(m.n_unc);
        std::vector<MapRay> patch;          /* source of asynchronous uploads */
        bool uploads = false;
        if (m.n_unc)
            HIP_TRY(ctx, hipMemcpy(list.data(), d_unc_list, (size_t)m.n_unc * 4, hipMemcpyDeviceToHost));
        if ((rc = map_patch_rays(ctx, m, list.data(), d_rays, patch, uploads))) return rc;
        if (uploads)
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   /* `patch` goes out of scope */
    }
    if ((rc = map_resize(ctx, m, scale))) return rc;
    const size_t n_cells = m.n_cells;

    /* the two value -> value tables of the cell update */
    if ((rc = map_ensure_tables(ctx, prm))) return rc;

    /* the carried bitmap waits in ctx->m_alloc until the new one is built */
    bool synced = false;
    if ((rc = map_claim_grid(ctx, m, ctx->m_alloc, synced))) return rc;

    if ((rc = ensure(ctx, ctx->m_cell, 3 * n_cells * sizeof(uint32_t)))) return rc;
    MapJob mj;
    std::memset(&mj, 0, sizeof(mj));
    mj.rays = d_rays;
    mj.nodes = d_nodes;
    mj.recs = reinterpret_cast<MapRayRec*>(ctx->m_recs.p);
    mj.n_hit = reinterpret_cast<uint32_t*>(ctx->m_cell.p);
    mj.n_miss = mj.n_hit + n_cells;
    mj.seg = mj.n_miss + n_cells;
    mj.lists = reinterpret_cast<uint32_t*>(ctx->m_lists.p);
    mj.counters = d_counters;
    map_fill_job(m, scale, reinterpret_cast<const uint16_t*>(ctx->m_lut.p), mj);
    unsigned long long counters[kMapCounters] = { 0 };
    counters[kMapKnownRow] = counters[kMapKnownCol] = ~0ull;
    const double t1 = clock_us();
    CallSpan span(ctx, info != nullptr);    /* device_us: events only for a caller who asks */
    if (info) {
        if (!span.a || !span.b)
            return fail(ctx, CSM_EIO, "map build: no event for device_us");
        HIP_TRY(ctx, hipEventRecord(span.a, ctx->stream));
    }
    HIP_TRY(ctx, hipMemcpyAsync(d_nodes, m.table.data(), m.table.size() * sizeof(MapNode),
                                hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(mj.counters, counters, sizeof(counters), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(mj.n_hit, 0, 2 * n_cells * sizeof(uint32_t), ctx->stream));
    {
        ScopedTimer tm(ctx, "map_build");
        const unsigned ray_blocks = (unsigned)ceil_div(std::max(n_rays, 1), 256);
        const unsigned cell_blocks = (unsigned)((n_cells + 255) / 256);
        if (n_rays) {
            keep_first(e, launch(k_map_hits, dim3(ray_blocks), dim3(256), ctx->stream, mj));
            keep_first(e, launch(k_map_alloc, dim3(cell_blocks), dim3(256), ctx->stream, mj));
            keep_first(e, launch(k_map_fill_hits, dim3(ray_blocks), dim3(256), ctx->stream, mj));
            keep_first(e, launch(k_map_rank_hits, dim3(ray_blocks), dim3(256), ctx->stream, mj));
            keep_first(e, launch(k_map_walk, dim3((unsigned)ceil_div(n_rays, kMapGroup)), dim3(512), ctx->stream, mj));
        }
        keep_first(e, launch(k_map_apply, dim3((unsigned)(((size_t)mj.rows * mj.pitch + 255) / 256)), dim3(256),
                             ctx->stream, mj));
        if (m.usable > 0) {
            /* one workgroup per CU at most; the kernel spreads the cells with hits over
             * their wavefronts (each has at least one usable ray) */
            const unsigned wgs = (unsigned)std::min<long long>(
                256, ceil_div((int)std::min<long long>(m.usable, (long long)n_cells), 4));
            keep_first(e, launch_lds(ctx->device, k_map_apply_hits, dim3(wgs), dim3(256), 65536 * sizeof(uint16_t),
                                     ctx->stream, mj));
        }
        if ((rc = launched_ok(ctx, e, "map build"))) return rc;
        /* the old allocation moved by the block shift, and every block a cell update touched
         * (each leaves a known cell) */
        if ((rc = map_carry_allocation(ctx, m, ctx->m_alloc))) return rc;
    }
    if (info)
        HIP_TRY(ctx, hipEventRecord(span.b, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(counters, mj.counters, sizeof(counters), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float dev_ms = 0.f;
    if (info)
        (void)hipEventElapsedTime(&dev_ms, span.a, span.b);
    if ((rc = map_finish(ctx, m, counters, info))) return rc;
    if (info) {
        info->host_us = t1 - t0;
        info->device_us = dev_ms * 1e3;
    }
    return CSM_OK;
}

/* GridMapBuilder::ConstructMapFromScans (src/mapping/grid_map_builder.cpp:561-695) */
int csm_construct_map_from_scans(csm_ctx* ctx, uint64_t map_id, csm_map_shape* shape,
                                 const double global_map_pose[3], const csm_scan_node* nodes,
                                 int32_t n_nodes, const csm_map_builder_params* prm,
                                 csm_map_build_info* info)
{
    return map_build(ctx, map_id, shape, global_map_pose, nodes, n_nodes, prm, info, false);
}

/* the grid half of GridMapBuilder::UpdateGridMap (src/mapping/grid_map_builder.cpp:389-494) */
int csm_update_map_with_scan(csm_ctx* ctx, uint64_t map_id, csm_map_shape* shape,
                             const double global_map_pose[3], const csm_scan_node* node,
                             const csm_map_builder_params* prm, csm_map_build_info* info)
{
    return map_build(ctx, map_id, shape, global_map_pose, node, node ? 1 : 0, prm, info, true);
}

} /* extern "C" */
