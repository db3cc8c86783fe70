/* csm_ray_kernels.hip -- the free-space check of loop candidates (included by csm_ray_api.hip; the
 * definition is in include/csm_hip.h, csm_ray_check_batch). gfx950 only.
 *
 * RayRec, the projection body and the patch body are csm_ray.hpp's, shared with the ray cast.
 *
 *   k_ray_project  one thread per beam of a chunk of queries: the hit point with the device's sin / cos,
 *                  its four integers (sub-pixel end, hit cell) and the map builder's certificate
 *                  (certified, csm_certify.hpp) at both resolutions on both axes. The frame is fixed here
 *                  (no resize follows), so the certificate speaks about exactly the integers stored. A
 *                  beam that is not certified is listed for the host.
 *   k_ray_patch    the listed beams' records as glibc gives them, scattered into place.
 *   k_ray_walk     256 threads = 4 wavefronts, kRayGroup consecutive rays of ONE query per workgroup, one
 *                  wavefront per ray, lanes over the ray's cells (ray_cells_closed_form, csm_map.hpp: the
 *                  text map_walk_ray runs). The ray is first moved by whole cells so that its coordinates
 *                  are non-negative (the floored reading of the reference's / and %), and the enumeration
 *                  is clipped to the map: a ray that starts far outside walks no empty column. Each lane
 *                  reads its cells from level 0 and classifies them; classes are summed per lane over the
 *                  wavefront's rays and reduced across the wave once; the workgroup sums in LDS and adds
 *                  each non-zero counter once to the query's record. max_depth goes through atomicMax.
 *                  Integer sums and maxima are order-free: no ordering between threads is assumed. Lane 0
 *                  writes the per-beam word. Nothing but the records and the words is written. */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csm_ray.hpp"

namespace csm {

constexpr int kRayGroup = 16;                /* rays per workgroup of k_ray_walk: 4 per wavefront */
/* one query of a chunk */
struct RayQuery {
    const uint16_t* cells;     /* level 0 of its map */
    int32_t rows, cols, pitch;
    int32_t n_beams;
    long long angles_at, ranges_at;   /* its scan in the chunk's staged doubles */
    double  x, y, theta;       /* S, the sensor pose (host) */
    double  off_x, off_y, res, scaled_res;
    int32_t sx, sy;            /* sub-pixel index of the sensor position (host) */
    int32_t pad[2];
};

struct RayChunk {
    const RayQuery* queries;
    const uint32_t* pre_beam;  /* [n_queries + 1] beams before each query */
    const uint32_t* pre_group; /* [n_queries + 1] workgroups of k_ray_walk before each query */
    const double* scans;
    RayRec* recs;              /* [n_beams] */
    int32_t* words;            /* [n_beams] per-beam words */
    unsigned char* records;    /* [n_queries] csm_ray_check_result */
    uint32_t* unc;             /* [0] count, [1 ..] the listed beams */
    uint32_t unc_cap;
    int32_t n_queries, n_beams;
    double  min_range, max_range;
    int32_t scale, tolerance;
    uint32_t occupied_min, free_max;
};

/* the record's layout as the kernel adds to it (csm_ray_check_result: 8 int32, 5 int64, 2 int32) */
enum RayCounter {
    kRayUsable = 1, kRayWalked, kRayBlocked, kRayEndInside, kRayEndOccupied, kRayEndFree, kRayEndUnknown,
    kRayCells, kRayCellsFree, kRayCellsUnknown, kRayCellsNear, kRayCellsBlocking, kRayCounters
};
constexpr int kRayRecordBytes = 80, kRayMaxDepthAt = 72;

__global__ __launch_bounds__(256) void k_ray_project(RayChunk ch)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= ch.n_beams)
        return;
    const int qi = prefix_find(ch.pre_beam, ch.n_queries, (uint32_t)b);
    const RayQuery& q = ch.queries[qi];
    const int i = b - (int)ch.pre_beam[qi];
    const double r = ch.scans[q.ranges_at + i];
    RayRec rec = { kRayUnusable, 0, 0, 0 };
    if (r > ch.min_range && r < ch.max_range) {
        bool sure;
        rec = ray_project<true>(q.x, q.y, q.theta, r, ch.scans[q.angles_at + i], q.off_x, q.off_y, q.res, q.scaled_res,
                                sure);
        if (!sure)
            ray_list(ch.unc, ch.unc_cap, (uint32_t)b);
    }
    ch.recs[b] = rec;
}

__global__ __launch_bounds__(256) void k_ray_patch(const RayPatch* patches, int n, RayRec* recs)
{
    ray_patch_one(patches, n, recs, blockIdx.x * 256 + threadIdx.x);
}

__global__ __launch_bounds__(256) void k_ray_walk(RayChunk ch)
{
    __shared__ uint32_t total[kRayCounters];
    __shared__ int depth_max;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < kRayCounters)
        total[tid] = 0;
    if (tid == 0)
        depth_max = 0;
    __syncthreads();

    const int qi = prefix_find(ch.pre_group, ch.n_queries, blockIdx.x);     /* uniform */
    const RayQuery& q = ch.queries[qi];
    const int first = ((int)blockIdx.x - (int)ch.pre_group[qi]) * kRayGroup;
    const int beam0 = (int)ch.pre_beam[qi];
    const int scale = ch.scale;

    /* per lane, over this wavefront's rays */
    uint32_t n_cells = 0, n_free = 0, n_unknown = 0, n_near = 0, n_blocking = 0;
    /* per wavefront (uniform) */
    uint32_t usable = 0, walked = 0, blocked = 0, end_inside = 0, end_occupied = 0, end_free = 0, end_unknown = 0;
    int wave_depth = 0;

    for (int k = wave; k < kRayGroup; k += 4) {
        const int i = first + k;
        if (i >= q.n_beams)
            break;
        const RayRec rec = ch.recs[beam0 + i];
        int word = -2;
        if (rec.ex != kRayUnusable) {
            ++usable;
            /* the same ray moved by whole cells into non-negative coordinates */
            const int bx = floor_div(min(q.sx, rec.ex), scale), by = floor_div(min(q.sy, rec.ey), scale);
            const int end_x = floor_div(rec.ex, scale), end_y = floor_div(rec.ey, scale);
            const RayClip clip = { -bx, q.cols - 1 - bx, -by, q.rows - 1 - by };
            uint32_t ray_cells = 0;
            int ray_depth = 0;
            ray_cells_closed_form<true>(
                q.sx - bx * scale, q.sy - by * scale, rec.ex - bx * scale, rec.ey - by * scale, scale, lane, clip,
                [&](int x, int y) {
                    const int cx = x + bx, cy = y + by;      /* inside the map: the clip */
                    if (cx == end_x && cy == end_y)
                        return;                              /* the end cell is no missed cell */
                    const uint32_t v = q.cells[(size_t)cy * q.pitch + cx];
                    ++ray_cells;
                    if (v == 0) {
                        ++n_unknown;
                    } else if (v <= ch.free_max) {
                        ++n_free;
                    } else if (v >= ch.occupied_min) {
                        const int d = max(abs(cx - rec.hx), abs(cy - rec.hy));
                        if (d > ch.tolerance) {
                            ++n_blocking;
                            ray_depth = max(ray_depth, d);
                        } else {
                            ++n_near;
                        }
                    }
                });
            n_cells += ray_cells;
            const bool any_cell = __ballot(ray_cells != 0) != 0ull;
            for (int off = 32; off; off >>= 1)
                ray_depth = max(ray_depth, __shfl_xor(ray_depth, off));
            const bool inside = rec.hx >= 0 && rec.hx < q.cols && rec.hy >= 0 && rec.hy < q.rows;
            if (inside) {
                const uint32_t v = q.cells[(size_t)rec.hy * q.pitch + rec.hx];
                ++end_inside;
                end_unknown += v == 0;
                end_free += v != 0 && v <= ch.free_max;
                end_occupied += v >= ch.occupied_min;
            }
            word = -1;
            if (any_cell || inside) {
                ++walked;
                word = ray_depth;           /* 0: walked and not blocked (a blocking depth is > tolerance >= 0) */
                blocked += ray_depth > 0;
                wave_depth = max(wave_depth, ray_depth);
            }
        }
        if (lane == 0)
            ch.words[beam0 + i] = word;
    }

    for (int off = 32; off; off >>= 1) {
        n_cells += __shfl_xor(n_cells, off);
        n_free += __shfl_xor(n_free, off);
        n_unknown += __shfl_xor(n_unknown, off);
        n_near += __shfl_xor(n_near, off);
        n_blocking += __shfl_xor(n_blocking, off);
    }
    if (lane == 0) {
        const uint32_t mine[kRayCounters] = { 0, usable, walked, blocked, end_inside, end_occupied, end_free,
                                              end_unknown, n_cells, n_free, n_unknown, n_near, n_blocking };
#pragma unroll
        for (int c = 1; c < kRayCounters; ++c)
            if (mine[c])
                atomicAdd(&total[c], mine[c]);
        if (wave_depth)
            atomicMax(&depth_max, wave_depth);
    }
    __syncthreads();

    unsigned char* const record = ch.records + (size_t)qi * kRayRecordBytes;
    if (tid >= 1 && tid < kRayCounters && total[tid]) {
        if (tid < kRayCells)
            atomicAdd(reinterpret_cast<int*>(record) + tid, (int)total[tid]);
        else
            atomicAdd(reinterpret_cast<unsigned long long*>(record + 32) + (tid - kRayCells),
                      (unsigned long long)total[tid]);
    }
    if (tid == 0 && depth_max)
        atomicMax(reinterpret_cast<int*>(record + kRayMaxDepthAt), depth_max);
}

} /* namespace csm */
