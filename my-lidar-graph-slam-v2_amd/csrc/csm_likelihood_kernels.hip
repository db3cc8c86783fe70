/* csm_likelihood_kernels.hip -- likelihood-field maps: every obstacle of a grid spread by an integer
 * Gaussian table (included by csm_likelihood_api.hip; the definition is in include/csm_hip.h).
 *
 *   k_likelihood_batch  grid = (column tiles, row tiles, maps), 256 threads: one 32 x 64 output tile of one
 *                       map per workgroup, any number of maps of any shapes in one launch (a workgroup
 *                       whose tile lies outside its map returns at once, as in k_boxmax_batch).
 *
 * Obstacles are sparse (walls one or two cells wide), so the workgroup does not visit the (2R + 1)^2 taps of
 * every cell. It stages the tile plus a halo of R cells into LDS (coalesced row reads, zeros outside the
 * map) and, while staging, compacts the obstacles it sees into an LDS list by wave ballot and prefix: one
 * word per obstacle, halo row << 23 | halo column << 16 | value. Then
 *   - no obstacle: the tile is copied through;
 *   - at most (2R + 1)^2 obstacles: every thread walks the list for its 8 cells (one column, 8 consecutive
 *     rows: the squared column distance is shared and rejects most entries with one compare). The list
 *     entry is a broadcast read; a hit costs one read of the LDS copy of the table, a multiply, a shift
 *     and a max;
 *   - more (a dense tile): the list is dropped -- it holds (2R + 1)^2 entries, and entries past that are
 *     counted but not stored -- and every thread visits the taps of the disc in the staged tile instead,
 *     which bounds the work per cell by the size of the disc.
 * An integer maximum does not depend on the order, so both paths and every list order give the same bytes.
 * Pad columns (cols..pitch) are written 0. The first known row / column of the new cells go through one
 * atomicMin per workgroup on the map's two counters (initialised to rows / cols by the host). */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csm_device.hpp"

namespace csm {

constexpr int kLfTR = 32, kLfTC = 64;                        /* output tile */
constexpr int kLfMaxR = 16;                                  /* CSM_LIKELIHOOD_MAX_RADIUS */
constexpr int kLfHC = kLfTC + 2 * kLfMaxR;                   /* LDS row pitch of the staged tile */
constexpr int kLfHR = kLfTR + 2 * kLfMaxR;
constexpr int kLfListCap = (2 * kLfMaxR + 1) * (2 * kLfMaxR + 1);
constexpr int kLfRows = 8;                                   /* consecutive rows of one thread */
static_assert(kLfRows * 4 == kLfTR && kLfTC == 64, "256 threads: 4 wavefronts of 64 columns, 8 rows each");
static_assert(kLfHR <= 64 && kLfHC <= 128, "a list entry packs the halo row in 6 bits, the column in 7");

struct LfJob {
    const uint16_t* src;
    uint16_t* dst;              /* rows * pitch, pad columns included */
    int32_t*  known;            /* [2]: first known row, column of dst; rows, cols before the launch */
    int32_t   rows, cols, pitch, pad;
};

struct LfParams {
    const uint32_t* kernel;     /* device copy of T[0 .. radius^2] */
    int32_t  radius;
    uint32_t occupied_min;      /* >= 1 */
    int32_t  keep_unknown;
    int32_t  pad;
};

__device__ __forceinline__ uint32_t lf_spread(uint32_t value_minus_1, uint32_t weight)
{
    return 1u + ((value_minus_1 * weight) >> 15);
}

__global__ __launch_bounds__(256) void k_likelihood_batch(const LfJob* jobs, LfParams prm)
{
    __shared__ uint16_t tile[kLfHR * kLfHC];
    __shared__ uint32_t list[kLfListCap];
    __shared__ uint32_t tab[kLfMaxR * kLfMaxR + 1];
    __shared__ uint32_t s_count;
    __shared__ int s_known[2];
    const LfJob j = jobs[blockIdx.z];
    const int r0 = blockIdx.y * kLfTR, c0 = blockIdx.x * kLfTC;
    if (r0 >= j.rows || c0 >= j.pitch)
        return;
    const int R = prm.radius, R2 = R * R;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) {
        s_count = 0;
        s_known[0] = s_known[1] = 0x7fffffff;
    }
    for (int i = tid; i <= R2; i += 256)
        tab[i] = prm.kernel[i];
    __syncthreads();

    /* stage tile + halo; compact its obstacles (every wavefront runs every trip: the ballot is whole) */
    const int nr = kLfTR + 2 * R, nc = kLfTC + 2 * R, total = nr * nc;
    for (int base = 0; base < total; base += 256) {
        const int i = base + tid;
        uint32_t v = 0;
        int r = 0, c = 0;
        if (i < total) {
            r = i / nc;
            c = i - r * nc;
            const int gr = r0 - R + r, gc = c0 - R + c;
            if (gr >= 0 && gr < j.rows && gc >= 0 && gc < j.cols)
                v = j.src[(size_t)gr * j.pitch + gc];
            tile[r * kLfHC + c] = (uint16_t)v;
        }
        const bool obstacle = v >= prm.occupied_min;        /* occupied_min >= 1: never an unknown cell */
        const unsigned long long m = __ballot(obstacle);
        if (m) {
            uint32_t first = 0;
            if (lane == 0)
                first = atomicAdd(&s_count, (uint32_t)__popcll(m));
            first = __shfl(first, 0);
            const uint32_t slot = first + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (obstacle && slot < (uint32_t)kLfListCap)
                list[slot] = v | (uint32_t)c << 16 | (uint32_t)r << 23;
        }
    }
    __syncthreads();

    const uint32_t n = s_count;
    const int tr0 = (tid >> 6) * kLfRows;       /* this thread's first row of the tile; its column is `lane` */
    const int hc = lane + R;                    /* ... and its column of the staged tile */
    uint32_t best[kLfRows];
#pragma unroll
    for (int k = 0; k < kLfRows; ++k)
        best[k] = 0;
    if (n != 0 && n <= (uint32_t)((2 * R + 1) * (2 * R + 1))) {
        for (uint32_t e = 0; e < n; ++e) {
            const uint32_t p = list[e];
            const int dc = (int)((p >> 16) & 127u) - hc;
            const int dc2 = dc * dc;
            if (dc2 > R2)
                continue;
            const int orow = (int)(p >> 23) - R - tr0;      /* the obstacle's row, from this thread's first */
            const uint32_t vm1 = (p & 0xffffu) - 1u;
#pragma unroll
            for (int k = 0; k < kLfRows; ++k) {
                const int dr = orow - k;
                const int d2 = dc2 + dr * dr;
                if (d2 <= R2)
                    best[k] = max(best[k], lf_spread(vm1, tab[d2]));
            }
        }
    } else if (n != 0) {
        for (int dr = -R; dr <= R; ++dr)
            for (int dc = -R; dc <= R; ++dc) {
                const int d2 = dr * dr + dc * dc;
                if (d2 > R2)
                    continue;
                const uint32_t w = tab[d2];
#pragma unroll
                for (int k = 0; k < kLfRows; ++k) {
                    const uint32_t v = tile[(tr0 + k + R + dr) * kLfHC + hc + dc];
                    if (v >= prm.occupied_min)
                        best[k] = max(best[k], lf_spread(v - 1u, w));
                }
            }
    }

    const int gc = c0 + lane;
    int kr = 0x7fffffff, kc = 0x7fffffff;
    if (gc < j.pitch) {
#pragma unroll
        for (int k = 0; k < kLfRows; ++k) {
            const int gr = r0 + tr0 + k;
            if (gr >= j.rows)
                break;
            const uint32_t g = tile[(tr0 + k + R) * kLfHC + hc];
            uint32_t o = 0;
            if (gc < j.cols && !(prm.keep_unknown && g == 0))
                o = max(g, best[k]);
            j.dst[(size_t)gr * j.pitch + gc] = (uint16_t)o;
            if (o != 0) {
                kr = min(kr, gr);
                kc = gc;
            }
        }
    }
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
