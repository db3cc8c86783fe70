/* csm_map_kernels.hip -- the kernels of the one-map updates
 * (csm_construct_map_from_scans, csm_update_map_with_scan): one launch per step
 * and map, the workgroup number is the place in the map. Their bodies are in
 * csm_map.hpp, shared with the many-map kernels. Included by csm_map_api.hip (its
 * own translation unit). gfx950 only. */
#ifndef CSM_MAP_KERNELS_HIP
#define CSM_MAP_KERNELS_HIP

#include "csm_map.hpp"

namespace csm {

__global__ __launch_bounds__(256) void k_map_project(MapProjJob job)
{
    map_project_beam(job, blockIdx.x * 256 + threadIdx.x);
}

/* hit cell + sub-pixel end of every ray; the cell's hit counter hands out slots */
__global__ __launch_bounds__(256) void k_map_hits(MapJob job)
{
    map_hits_ray(job, blockIdx.x * 256 + threadIdx.x);
}

__global__ __launch_bounds__(256) void k_map_alloc(MapJob job)
{
    map_alloc_cell(job, blockIdx.x * 256 + threadIdx.x);
}

__global__ __launch_bounds__(256) void k_map_fill_hits(MapJob job)
{
    map_fill_ray(job, blockIdx.x * 256 + threadIdx.x);
}

/* rank of each hit among its cell's hits = its place in ray order */
__global__ __launch_bounds__(256) void k_map_rank_hits(MapJob job)
{
    map_rank_ray(job, blockIdx.x * 256 + threadIdx.x);
}

__global__ __launch_bounds__(512) void k_map_walk(MapJob job)
{
    map_walk_group(job, blockIdx.x);
}

/* cells no ray ends in: their miss count through the miss table; clears the rest */
__global__ __launch_bounds__(256) void k_map_apply(MapJob job)
{
    map_apply_cell(job, blockIdx.x);
}

/* cells with hits (csm_map.hpp, map_apply_hit_cell) */
__global__ __launch_bounds__(256) void k_map_apply_hits(MapJob job)
{
    extern __shared__ uint16_t hit_table[];
    const uint32_t n_cells = (uint32_t)job.counters[kMapHitCells];
    const uint32_t waves = gridDim.x * 4u;
    const uint32_t per_wave = min(max((n_cells + waves - 1u) / waves, 1u), 64u);
    if (blockIdx.x * 4u * per_wave >= n_cells)
        return;                              /* fewer cells than workgroups (uniform exit) */
    map_load_hit_table(job.lut_hit, hit_table);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * 4u + (threadIdx.x >> 6);
    for (uint32_t first = 0; first < n_cells; first += waves * per_wave) {
        const uint32_t idx = first + wave * per_wave + lane;
        uint32_t v = 0, sat = 0, updates = 0;
        int row = 0, col = 0;
        if (lane < per_wave && idx < n_cells)
            map_apply_hit_cell(job, hit_table, (int)job.hit_cells[idx], v, sat, updates, row, col);
        map_apply_totals(job, v, row, col, sat, updates, blockIdx.x);
    }
}

} /* namespace csm */
#endif
