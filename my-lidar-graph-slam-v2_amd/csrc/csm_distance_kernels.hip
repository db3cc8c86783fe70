/* csm_distance_kernels.hip -- distance fields: every cell's nearest obstacle, exactly, in two separable
 * passes (included by csm_distance_api.hip; the definition is in include/csm_hip.h, the argument for the
 * two tie rules in DESIGN.md 4p).
 *
 *   k_distance_columns  grid = (64-column strips, 1, maps), 64 threads: one lane per column, so every load
 *                       and store of a row is contiguous. A sweep down writes the signed row offset to the
 *                       last obstacle above (or on) the cell, a sweep up replaces it where the obstacle
 *                       below is STRICTLY nearer: of two equally near the upper one stays. No obstacle in
 *                       the column: kDtNone. The sweeps are serial over the rows; the loads do not depend
 *                       on the carried row, so they pipeline.
 *   k_distance_rows<T>  grid = (1, runs of kDtRun rows, maps), 256 threads, dynamic LDS: the offsets of
 *                       `per_pass` rows staged per trip (4: one wavefront per row; 1 for maps too wide for
 *                       that: the whole workgroup on one row). Every lane owns the columns lane, lane +
 *                       width, ..; from its column it walks outwards (c - k, c + k) over the staged row
 *                       and keeps min (d2 << 32 | nearest), until k^2 > d2: at k^2 == d2 an obstacle of the
 *                       cell's own row ties and may have the smaller index. T = false (the build): looks
 *                       T[min(d2, R^2)] up in global memory (read-only, L2-resident), applies keep_unknown,
 *                       writes the cell, pad columns 0, and reduces the first known row / column: wave
 *                       shuffles, LDS, one atomicMin pair per workgroup. T = true (csm_distance_transform):
 *                       writes d2 and nearest to dense buffers instead; no map is written.
 *
 * Maps of any shapes share a launch: one job per map, a workgroup outside its map returns at once, as in
 * k_likelihood_batch. Every index is checked against the map's own rows / cols / pitch. */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csm_device.hpp"

namespace csm {

constexpr int kDtRun = 4;                       /* rows of one workgroup of the row pass */
constexpr int kDtWide = 8192;                   /* widest map with one wavefront per row: 4 rows x 16 KB of LDS */
constexpr int kDtNone = -32768;                 /* offset: the column holds no obstacle */
constexpr uint32_t kDtFar = 0xFFFFFFFFu;        /* CSM_DISTANCE_NONE */
constexpr int kDtHead = 16;                     /* bytes ahead of the staged rows: the workgroup's two counters */

struct DtJob {
    const uint16_t* src;        /* rows * pitch */
    int16_t*  off;              /* rows * cols: scratch of the column pass */
    uint16_t* dst;              /* rows * pitch, pad columns included (build) */
    uint32_t* d2;               /* rows * cols, or null (transform) */
    uint32_t* nearest;          /* rows * cols, or null (transform) */
    int32_t*  known;            /* [2]: first known row, column of dst; rows, cols before the launch (build) */
    int32_t   rows, cols, pitch, pad;
};

struct DtParams {
    const uint16_t* table;      /* device copy of T[0 .. radius^2] (build) */
    int32_t  radius;
    uint32_t occupied_min;      /* >= 1 */
    int32_t  keep_unknown;
    int32_t  per_pass;          /* rows staged per trip of the row pass: 4 or 1 */
    int32_t  lds_cols;          /* int16 slots per staged row: >= the widest map of the launch, even */
    int32_t  pad;
};

__global__ __launch_bounds__(64) void k_distance_columns(const DtJob* jobs, DtParams prm)
{
    const DtJob j = jobs[blockIdx.z];
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= j.cols)
        return;
    const uint16_t* __restrict__ src = j.src + c;
    int16_t* __restrict__ off = j.off + c;
    int last = -1;
#pragma unroll 4
    for (int r = 0; r < j.rows; ++r) {
        if (src[(size_t)r * j.pitch] >= prm.occupied_min)
            last = r;
        off[(size_t)r * j.cols] = (int16_t)(last < 0 ? kDtNone : last - r);
    }
    last = -1;
#pragma unroll 4
    for (int r = j.rows - 1; r >= 0; --r) {
        const int up = off[(size_t)r * j.cols];         /* <= 0, or none */
        if (up == 0)
            last = r;
        else if (last >= 0 && (up == kDtNone || last - r < -up))
            off[(size_t)r * j.cols] = (int16_t)(last - r);
    }
}

__device__ __forceinline__ unsigned long long dt_key(int k2, int o, int r, int cols, int at)
{
    return (unsigned long long)(uint32_t)(k2 + o * o) << 32 | (uint32_t)((r + o) * cols + at);
}

template <bool kTransform>
__global__ __launch_bounds__(256) void k_distance_rows(const DtJob* jobs, DtParams prm)
{
    extern __shared__ __attribute__((aligned(16))) char dt_lds[];
    const DtJob j = jobs[blockIdx.z];
    const int r0 = blockIdx.y * kDtRun;
    if (r0 >= j.rows)
        return;
    int* const s_known = reinterpret_cast<int*>(dt_lds);
    int16_t* const stage = reinterpret_cast<int16_t*>(dt_lds + kDtHead);
    const int tid = threadIdx.x, lane = tid & 63;
    const int width = 256 / prm.per_pass;               /* lanes of one row */
    const int slot = tid / width, first = tid - slot * width;
    const int R2 = prm.radius * prm.radius;
    const int out_cols = kTransform ? j.cols : j.pitch;
    if (tid == 0)
        s_known[0] = s_known[1] = 0x7fffffff;
    int kr = 0x7fffffff, kc = 0x7fffffff;
    const int r_end = min(r0 + kDtRun, j.rows);
    for (int rb = r0; rb < r_end; rb += prm.per_pass) {
        __syncthreads();                                /* the rows of the last trip are read; s_known is set */
        const int nr = min(prm.per_pass, r_end - rb);
        for (int i = tid; i < nr * j.cols; i += 256) {
            const int rr = i / j.cols, cc = i - rr * j.cols;
            stage[rr * prm.lds_cols + cc] = j.off[(size_t)(rb + rr) * j.cols + cc];
        }
        __syncthreads();
        const int r = rb + slot;
        if (r >= r_end)
            continue;
        const int16_t* g = stage + slot * prm.lds_cols;
        for (int c = first; c < out_cols; c += width) {
            if (c >= j.cols) {                          /* a pad column (build only) */
                j.dst[(size_t)r * j.pitch + c] = 0;
                continue;
            }
            unsigned long long best = ~0ull;
            const int own = g[c];
            if (own != kDtNone)
                best = dt_key(0, own, r, j.cols, c);
            const int reach = max(c, j.cols - 1 - c);
            for (int k = 1; k <= reach; ++k) {
                const int k2 = k * k;
                if ((unsigned long long)k2 > (best >> 32))
                    break;
                if (c - k >= 0) {
                    const int o = g[c - k];
                    if (o != kDtNone)
                        best = min(best, dt_key(k2, o, r, j.cols, c - k));
                }
                if (c + k < j.cols) {
                    const int o = g[c + k];
                    if (o != kDtNone)
                        best = min(best, dt_key(k2, o, r, j.cols, c + k));
                }
            }
            const uint32_t d2 = (uint32_t)(best >> 32);
            if (kTransform) {
                if (j.d2)
                    j.d2[(size_t)r * j.cols + c] = d2;
                if (j.nearest)
                    j.nearest[(size_t)r * j.cols + c] = (uint32_t)best;
            } else {
                uint32_t o = prm.table[min(d2, (uint32_t)R2)];
                if (prm.keep_unknown && j.src[(size_t)r * j.pitch + c] == 0)
                    o = 0;
                j.dst[(size_t)r * j.pitch + c] = (uint16_t)o;
                if (o != 0) {
                    kr = min(kr, r);
                    kc = min(kc, c);
                }
            }
        }
    }
    if (kTransform)
        return;
    for (int s = 32; s >= 1; s >>= 1) {
        kr = min(kr, __shfl_xor(kr, s));
        kc = min(kc, __shfl_xor(kc, s));
    }
    if (lane == 0 && kr != 0x7fffffff) {
        atomicMin(&s_known[0], kr);
        atomicMin(&s_known[1], kc);
    }
    __syncthreads();
    if (tid == 0 && s_known[0] != 0x7fffffff) {
        atomicMin(&j.known[0], s_known[0]);
        atomicMin(&j.known[1], s_known[1]);
    }
}

} /* namespace csm */
