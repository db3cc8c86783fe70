/* csm_map_build.hpp -- the host steps of a map build, each on ONE map, defined in csm_map_api.hip.
 * map_build (csm_map_api.hip) runs them on its one map; run_chunk (csm_map_batch_api.hip) runs each
 * in a loop over the chunk's jobs before the next one starts. What stays with the callers: the
 * launches, the sizes and carving of the scratch buffers, where the carried bitmap waits, the
 * synchronises behind asynchronous uploads, and host_us / device_us.
 *
 * Every step fails through fail(ctx, ...) and returns the code. map_node_table, map_resize and
 * map_finish refuse a MAP (CSM_EINVAL, CSM_ENOENT): a batch goes on with its other jobs.
 * map_patch_rays and map_claim_grid fail only on the device or on an allocation: that ends the call. */
#ifndef CSM_MAP_BUILD_HPP
#define CSM_MAP_BUILD_HPP

#include "csm_internal.hpp"

namespace csm_host {

/* one map on its way through a build */
struct MapBuild {
    uint64_t map_id = 0;
    csm_map_shape* shape = nullptr;        /* the caller's: the frame before the build, written by map_finish */
    const double* map_pose = nullptr;
    const csm_scan_node* nodes = nullptr;
    int n_nodes = 0;
    bool keep_cells = false;               /* csm_update_map_with_scan */
    std::vector<MapNode> table;
    long long usable = 0;
    int n_beams = 0;                       /* = rays: a ray's number is its beam's place in the update order */
    double min_x = 0, min_y = 0, max_x = 0, max_y = 0;   /* of the points the host holds as doubles */
    int box[4] = { 0, 0, 0, 0 };           /* of the beams the device certified, in indices */
    bool device_projection = false, spread_known = false;
    uint32_t n_unc = 0;
    csm_map_shape next = {};
    int32_t shift[2] = { 0, 0 };           /* first row / column of the new map in the old frame */
    bool resized = false;
    size_t n_cells = 0;
    bool has_carried = false;
    int carried_brows = 0, carried_bcols = 0;
    DeviceGrid fresh;                      /* a new grid until the build has succeeded */
    DeviceGrid* dst = nullptr;

    void add_point(double x, double y)
    {
        min_x = std::min(min_x, x);
        min_y = std::min(min_y, y);
        max_x = std::max(max_x, x);
        max_y = std::max(max_y, y);
    }
};

/* csm_config.map_uncertain_cap: tests of the overflow path */
inline uint32_t map_unc_cap(const csm_ctx* ctx)
{
    return ctx->tune.map_unc_cap > 0 ? (uint32_t)std::min<long>(ctx->tune.map_unc_cap, kMapUncCap) : kMapUncCap;
}

/* m's map_id ... keep_cells are set. The per-map argument checks (update mode: the map is resident with
 * the shape given), then table (sx = sy = 0), usable, n_beams, the bounds over the sensors, the empty
 * box, and whether the device projects. */
int map_node_table(csm_ctx* ctx, const csm_map_builder_params* prm, MapBuild& m);
/* the eight words of the device projection (box, count, spread bits): m.box, n_unc and spread_known,
 * or device_projection = false when the map has to be projected on the host */
void map_take_projection(MapBuild& m, const int32_t got[8], uint32_t unc_cap);
/* The hit points the device did not leave in d_rays (m's first ray): the n_unc beams of `list`
 * recomputed exactly, each with a copy of its own, or after a refused device projection all of them.
 * `src` is filled with the sources of the copies queued on ctx->stream, `uploads` set if there are
 * any: the caller keeps src until it has synchronised. */
int map_patch_rays(csm_ctx* ctx, MapBuild& m, const uint32_t* list, MapRay* d_rays, std::vector<MapRay>& src,
                   bool& uploads);
/* Resize (keep_cells: Expand) to the bounds: next, shift, resized, n_cells, and the table's sx / sy */
int map_resize(csm_ctx* ctx, MapBuild& m, int scale);
/* The old map's block allocation moves to `carried` (empty, or the context's spare: the grid's bitmap
 * buffer takes its place) until build_allocation has run; m.dst = the grid to build into, in place
 * or m.fresh, with the old cells shifted in update mode, its levels and copies marked as behind.
 * `synced`: the stream has been synchronised since the last launch; set where this step does it. */
int map_claim_grid(csm_ctx* ctx, MapBuild& m, DevBuf& carried, bool& synced);
/* mj's geometry, tables and output cells; its scratch pointers other than hit_cells are the caller's */
void map_fill_job(const MapBuild& m, int scale, const uint16_t* d_lut, MapJob& mj);
/* build_allocation for m.dst behind the update chain: the bitmap in `carried` moved by the block shift */
int map_carry_allocation(csm_ctx* ctx, MapBuild& m, const DevBuf& carried);
/* The counter block read back: a ray that left the map drops the map; otherwise the first known row /
 * column, the caller's shape, info (null, or all but host_us / device_us), and a fresh grid registered. */
int map_finish(csm_ctx* ctx, MapBuild& m, const unsigned long long* counters, csm_map_build_info* info);

} /* namespace csm_host */

#endif
