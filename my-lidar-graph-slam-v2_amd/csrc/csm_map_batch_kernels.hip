/* csm_map_batch_kernels.hip -- the kernels of csm_construct_maps_from_scans: every
 * step of the map build once per chunk of maps instead of once per map. The bodies
 * are those of the one-map kernels (csm_map.hpp); what is new here is the schedule.
 *
 * Flat schedule: the host uploads, per step, the prefix sums of the maps' workgroup
 * counts (MapBatchTable). A workgroup finds its map by a binary search on its own
 * number -- uniform, so the table and the map's MapJob come in through scalar loads
 * -- and then does what workgroup (number - prefix) of the one-map kernel does. A
 * map's rays, beams and cells round up to whole workgroups (and whole groups of
 * k_map_walk), so no workgroup holds parts of two maps, and maps that differ 30 x in
 * size cost what they hold, not what the largest holds.
 *
 * k_mapb_apply_hits is the exception: its items (cells with hits) are known only on
 * the device. k_mapb_hit_prefix sums the maps' counts, and one persistent workgroup
 * per CU loads the hit table into LDS once and walks the chunk-wide item list; lanes
 * of one wavefront may hold cells of different maps, so the per-map totals are
 * reduced map by map. Included by csm_map_batch_api.hip. gfx950 only. */
#ifndef CSM_MAP_BATCH_KERNELS_HIP
#define CSM_MAP_BATCH_KERNELS_HIP

#include "csm_map.hpp"

namespace csm {

/* the map of workgroup (or item) w is prefix_find(pre, n, w) (csm_score_common.hpp); maps without
 * work have pre[m] == pre[m + 1] and are never found. */

__global__ __launch_bounds__(256) void k_mapb_project(MapBatchTable tab)
{
    const int m = prefix_find(tab.pre_beam, tab.n_maps, blockIdx.x);
    map_project_beam(tab.proj[m], (int)(blockIdx.x - tab.pre_beam[m]) * 256 + (int)threadIdx.x);
}

__global__ __launch_bounds__(256) void k_mapb_hits(MapBatchTable tab)
{
    const int m = prefix_find(tab.pre_ray, tab.n_maps, blockIdx.x);
    map_hits_ray(tab.jobs[m], (int)(blockIdx.x - tab.pre_ray[m]) * 256 + (int)threadIdx.x);
}

__global__ __launch_bounds__(256) void k_mapb_alloc(MapBatchTable tab)
{
    const int m = prefix_find(tab.pre_cell, tab.n_maps, blockIdx.x);
    map_alloc_cell(tab.jobs[m], (int)(blockIdx.x - tab.pre_cell[m]) * 256 + (int)threadIdx.x);
}

__global__ __launch_bounds__(256) void k_mapb_fill_hits(MapBatchTable tab)
{
    const int m = prefix_find(tab.pre_ray, tab.n_maps, blockIdx.x);
    map_fill_ray(tab.jobs[m], (int)(blockIdx.x - tab.pre_ray[m]) * 256 + (int)threadIdx.x);
}

/* the rank is the hit's place among ITS map's rays: ray numbers are local to the map */
__global__ __launch_bounds__(256) void k_mapb_rank_hits(MapBatchTable tab)
{
    const int m = prefix_find(tab.pre_ray, tab.n_maps, blockIdx.x);
    map_rank_ray(tab.jobs[m], (int)(blockIdx.x - tab.pre_ray[m]) * 256 + (int)threadIdx.x);
}

__global__ __launch_bounds__(512) void k_mapb_walk(MapBatchTable tab)
{
    const int m = prefix_find(tab.pre_group, tab.n_maps, blockIdx.x);
    map_walk_group(tab.jobs[m], (int)(blockIdx.x - tab.pre_group[m]));
}

__global__ __launch_bounds__(256) void k_mapb_apply(MapBatchTable tab)
{
    const int m = prefix_find(tab.pre_apply, tab.n_maps, blockIdx.x);
    map_apply_cell(tab.jobs[m], blockIdx.x - tab.pre_apply[m]);
}

/* hit_prefix[m] = cells with hits in the maps before m, [n_maps] = all of them. One workgroup. */
__global__ __launch_bounds__(256) void k_mapb_hit_prefix(MapBatchTable tab)
{
    __shared__ uint32_t wave_sum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t carry = 0;
    for (int m0 = 0; m0 < tab.n_maps; m0 += 256) {
        const int m = m0 + tid;
        const uint32_t c = m < tab.n_maps ? (uint32_t)tab.jobs[m].counters[kMapHitCells] : 0u;
        uint32_t incl = c;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off);
            if (lane >= off)
                incl += up;
        }
        if (lane == 63)
            wave_sum[wave] = incl;
        __syncthreads();
        uint32_t before = 0;
        for (int w = 0; w < wave; ++w)
            before += wave_sum[w];
        if (m < tab.n_maps)
            tab.hit_prefix[m] = carry + before + incl - c;
        carry += wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
        __syncthreads();
    }
    if (tid == 0)
        tab.hit_prefix[tab.n_maps] = carry;
}

/* Cells with hits of all maps of the chunk: item i is cell hit_cells[i - hit_prefix[m]] of the map m
 * that prefix_find gives. One workgroup per CU at most (128 KB of LDS each), the table loaded once; as in
 * k_map_apply_hits, as few lanes per wavefront carry a cell as the chunk's total allows. */
__global__ __launch_bounds__(256) void k_mapb_apply_hits(MapBatchTable tab, const uint16_t* lut_hit)
{
    extern __shared__ uint16_t hit_table[];
    const uint32_t n_items = tab.hit_prefix[tab.n_maps];
    const uint32_t waves = gridDim.x * 4u;
    const uint32_t per_wave = min(max((n_items + waves - 1u) / waves, 1u), 64u);
    if (blockIdx.x * 4u * per_wave >= n_items)
        return;                              /* fewer cells than workgroups (uniform exit) */
    map_load_hit_table(lut_hit, hit_table);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * 4u + (threadIdx.x >> 6);
    for (uint32_t first = 0; first < n_items; first += waves * per_wave) {
        const uint32_t idx = first + wave * per_wave + lane;
        const bool have = lane < per_wave && idx < n_items;
        uint32_t v = 0, sat = 0, updates = 0;
        int row = 0, col = 0, m = -1;
        if (have) {
            m = prefix_find(tab.hit_prefix, tab.n_maps, idx);
            const MapJob& job = tab.jobs[m];
            map_apply_hit_cell(job, hit_table, (int)job.hit_cells[idx - tab.hit_prefix[m]], v, sat, updates, row, col);
        }
        /* the totals are per map: one reduction for each map this wavefront holds (mostly one) */
        unsigned long long todo = __ballot(have);
        while (todo) {
            const int mm = __builtin_amdgcn_readfirstlane(__shfl(m, __ffsll((long long)todo) - 1));
            const bool mine = have && m == mm;
            map_apply_totals(tab.jobs[mm], mine ? v : 0u, row, col, mine ? sat : 0u, mine ? updates : 0u, blockIdx.x);
            todo &= ~__ballot(mine);
        }
    }
}

} /* namespace csm */
#endif
