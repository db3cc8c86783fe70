/* csm_map_global_kernels.hip -- the kernels of csm_construct_global_map: one map of
 * many scans, cast in parts. The chain is the one-map chain (project, hits, alloc,
 * fill, rank, walk, apply, apply_hits) on the bodies of csm_map.hpp; only the rank
 * step differs. After k_gmap_fill_hits a cell's arrival list holds its ray numbers in
 * atomic arrival order and k_gmap_walk needs them ascending behind it. Per cell, by
 * its number of hits n:
 *   n <= direct_max          k_gmap_rank_direct: each hit counts the earlier arrivals
 *                            (map_rank_ray, as the one-map chain)
 *   direct_max < n <= tile   k_gmap_rank_sort, one workgroup per cell: the list into LDS,
 *                            padded with 0xffffffff to a power of two, a bitonic sort
 *   n > tile                 the same workgroup sorts the list tile by tile, each sorted
 *                            tile written back over its part of the arrival list; a
 *                            hit's rank is then the sum over the tiles of the number of
 *                            smaller entries (a binary search per tile)
 * Ray numbers of a map are distinct: no tie rule. k_gmap_alloc lists the cells with
 * n > direct_max ("long cells") from the END of the hit-cell list downwards: a long
 * cell has at least two hits, so cells with hits + long cells <= rays and the two
 * lists never meet. Wave64, integer atomics only, no scratch memory.
 * Included by csm_map_global_api.hip (its own translation unit). gfx950 only. */
#ifndef CSM_MAP_GLOBAL_KERNELS_HIP
#define CSM_MAP_GLOBAL_KERNELS_HIP

#include "csm_map.hpp"

namespace csm {

/* the counter block of a global build: the one-map block, then these. They are never cleared
 * between the parts of a build except kGmapLong (with kMapCursor and kMapHitCells). */
enum GmapCounter {
    kGmapLong = kMapCounters,   /* long cells of this part */
    kGmapMaxHits,               /* largest n of any cell of any part */
    kGmapDirect, kGmapSorted, kGmapTiled,   /* hit cells by rank path, all parts */
    kGmapCounters
};

struct GmapRank {
    uint32_t direct_max;        /* >= 1 */
    uint32_t tile;              /* a power of two >= 4: entries (words of dynamic LDS) per sort */
};

/* between two parts: the words of one part cleared, the totals go on */
__global__ void k_gmap_next_part(unsigned long long* counters)
{
    if (threadIdx.x == 0) {
        counters[kMapCursor] = 0;
        counters[kMapHitCells] = 0;
        counters[kGmapLong] = 0;
    }
}

__global__ __launch_bounds__(256) void k_gmap_project(MapProjJob job)
{
    map_project_beam(job, blockIdx.x * 256 + threadIdx.x);
}

__global__ __launch_bounds__(256) void k_gmap_hits(MapJob job)
{
    map_hits_ray(job, blockIdx.x * 256 + threadIdx.x);
}

/* the one-map allocation, then the long cells listed and the cells counted by rank path */
__global__ __launch_bounds__(256) void k_gmap_alloc(MapJob job, GmapRank rk)
{
    const int cell = blockIdx.x * 256 + threadIdx.x;
    map_alloc_cell(job, cell);
    const uint32_t n = cell < job.rows * job.cols ? job.n_hit[cell] : 0u;
    if (n > rk.direct_max) {
        const uint32_t pos = (uint32_t)atomicAdd(&job.counters[kGmapLong], 1ull);
        job.hit_cells[(uint32_t)job.n_rays - 1u - pos] = (uint32_t)cell;
    }
    uint32_t direct = n && n <= rk.direct_max, sorted = n > rk.direct_max && n <= rk.tile, tiled = n > rk.tile;
    uint32_t most = n;
    for (int off = 32; off; off >>= 1) {
        direct += __shfl_xor(direct, off);
        sorted += __shfl_xor(sorted, off);
        tiled += __shfl_xor(tiled, off);
        most = max(most, (uint32_t)__shfl_xor(most, off));
    }
    if ((threadIdx.x & 63) == 0 && most) {
        if (direct)
            atomicAdd(&job.counters[kGmapDirect], (unsigned long long)direct);
        if (sorted)
            atomicAdd(&job.counters[kGmapSorted], (unsigned long long)sorted);
        if (tiled)
            atomicAdd(&job.counters[kGmapTiled], (unsigned long long)tiled);
        if ((unsigned long long)most > job.counters[kGmapMaxHits])    /* only ever rises */
            atomicMax(&job.counters[kGmapMaxHits], (unsigned long long)most);
    }
}

__global__ __launch_bounds__(256) void k_gmap_fill_hits(MapJob job)
{
    map_fill_ray(job, blockIdx.x * 256 + threadIdx.x);
}

/* the hits of short cells: the one-map rank */
__global__ __launch_bounds__(256) void k_gmap_rank_direct(MapJob job, GmapRank rk)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= job.n_rays)
        return;
    const int cell = job.recs[r].hit_cell;
    if (cell >= 0 && job.n_hit[cell] <= rk.direct_max)
        map_rank_ray(job, r);
}

/* s[0 .. p), p a power of two, ascending; 256 threads, all of them call */
__device__ __forceinline__ void gmap_bitonic(uint32_t* s, uint32_t p)
{
    for (uint32_t k = 2; k <= p; k <<= 1) {
        for (uint32_t j = k >> 1; j; j >>= 1) {
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < p; i += 256) {
                const uint32_t q = i ^ j;
                if (q > i) {
                    const uint32_t a = s[i], b = s[q];
                    if ((a > b) == ((i & k) == 0)) {
                        s[i] = b;
                        s[q] = a;
                    }
                }
            }
        }
    }
    __syncthreads();
}

/* One workgroup per long cell. The launch covers an upper bound of their number (rays / (direct_max +
 * 1)): workgroups past the count leave at once. Dynamic LDS: rk.tile words. */
__global__ __launch_bounds__(256) void k_gmap_rank_sort(MapJob job, GmapRank rk)
{
    extern __shared__ uint32_t keys[];
    if ((unsigned long long)blockIdx.x >= job.counters[kGmapLong])
        return;                              /* uniform */
    const uint32_t cell = job.hit_cells[(uint32_t)job.n_rays - 1u - blockIdx.x];
    const uint32_t n = job.n_hit[cell];
    uint32_t* arrival = job.lists + job.seg[cell];
    uint32_t* sorted = arrival + n;
    const uint32_t tid = threadIdx.x;
    for (uint32_t t0 = 0; t0 < n; t0 += rk.tile) {
        const uint32_t count = min(rk.tile, n - t0);
        uint32_t p = 4;
        while (p < count)
            p <<= 1;
        __syncthreads();                     /* the previous tile has been written out */
        for (uint32_t i = tid; i < p; i += 256)
            keys[i] = i < count ? arrival[t0 + i] : 0xffffffffu;
        gmap_bitonic(keys, p);
        /* one tile: the result. Several: each sorted tile over its own part of the arrival list */
        uint32_t* out = n <= rk.tile ? sorted : arrival + t0;
        for (uint32_t i = tid; i < count; i += 256)
            out[i] = keys[i];
    }
    if (n <= rk.tile)
        return;
    __syncthreads();                         /* the tiles, written by this workgroup, are visible to it */
    for (uint32_t i = tid; i < n; i += 256) {
        const uint32_t r = arrival[i];
        uint32_t rank = 0;
        for (uint32_t t0 = 0; t0 < n; t0 += rk.tile) {
            uint32_t lo = 0, hi = min(rk.tile, n - t0);
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (arrival[t0 + mid] < r)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            rank += lo;
        }
        sorted[rank] = r;
    }
}

__global__ __launch_bounds__(512) void k_gmap_walk(MapJob job)
{
    map_walk_group(job, blockIdx.x);
}

__global__ __launch_bounds__(256) void k_gmap_apply(MapJob job)
{
    map_apply_cell(job, blockIdx.x);
}

/* cells with hits (csm_map.hpp, map_apply_hit_cell), handed out as the one-map chain does */
__global__ __launch_bounds__(256) void k_gmap_apply_hits(MapJob job)
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
