/* csm_loopsearch_kernels.hip -- the candidate pairs of a pose graph (included by csm_loopsearch_api.hip; the
 * rule is in include/csm_hip.h, csm_loop_search). gfx950 only.
 *
 *   k_loop_search  256 threads = 4 wavefronts, one workgroup per query. Every thread finds the query's prefix
 *                  length by the same binary search on travel (uniform: scalar loads). Then one pass over
 *                  the prefix: every lane strides over it with coalesced f64 loads of x and y and appends
 *                  each eligible pair's key (d2 bits, r) and map to a list in LDS (an LDS counter hands out
 *                  the slots; it ends as the number of eligible pairs, whether they fitted or not). Then one
 *                  round per record: every lane keeps the least key that is greater than the key selected
 *                  last -- from the list, or, when the eligible pairs outnumber the list's kLoopListCap
 *                  slots, from another pass over the prefix; with one_per_map it skips a pair whose map has
 *                  its bit set in the LDS bitset of maps already taken. The 96-bit key is reduced across the
 *                  wave by xor shuffles, across the four waves through LDS, and thread 0 writes the record.
 *                  Rounds end with the first that finds nothing; the unused slots are filled by all threads.
 *                  The order of the keys is total, so nothing depends on which lane met a key or on the
 *                  order of the list; no sort. d2 is formed as the host forms it: two subtractions, two
 *                  products, one sum, each rounded on its own (the unit is compiled with -ffp-contract=off,
 *                  and no fma is written). Only the query's records, count, prefix length and eligible count
 *                  are written. */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/csm_hip.h"

namespace csm {

constexpr int kLoopBlock = 256;
constexpr int kLoopWaves = kLoopBlock / 64;
constexpr int kLoopMapWords = CSM_LOOP_SEARCH_MAX_MAPS / 32;
constexpr int kLoopListCap = 1024;     /* eligible pairs of a query kept in LDS: 16 bytes each */

struct LoopSearchJob {
    const double*  x;              /* [n_scan] */
    const double*  y;
    const double*  travel;
    const int32_t* map;            /* [n_scan] */
    const int32_t* query_index;    /* [n_q] */
    const double*  query_travel;   /* [n_q] */
    csm_loop_candidate* out;       /* [n_q * k] */
    int32_t* counts;               /* [n_q] records used */
    int32_t* prefix;               /* [n_q] p_q */
    int32_t* eligible;             /* [n_q] eligible pairs */
    double  travel_threshold, t2;
    int32_t n_ref, n_maps, k, one_per_map;
};

struct LoopKey {
    uint64_t d;                    /* bits of d2 */
    int32_t  r;                    /* -1 with d = ~0: no candidate */
};

__device__ __forceinline__ bool loop_key_less(uint64_t ad, int32_t ar, uint64_t bd, int32_t br)
{
    return ad < bd || (ad == bd && ar < br);
}

__device__ __forceinline__ LoopKey loop_key_min_wave(LoopKey k)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)k.d, m, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(k.d >> 32), m, 64);
        const int32_t r = __shfl_xor(k.r, m, 64);
        const uint64_t d = ((uint64_t)hi << 32) | lo;
        if (loop_key_less(d, r, k.d, k.r)) {
            k.d = d;
            k.r = r;
        }
    }
    return k;
}

__global__ __launch_bounds__(kLoopBlock) void k_loop_search(LoopSearchJob job)
{
    __shared__ uint32_t taken[kLoopMapWords];
    __shared__ uint64_t list_d[kLoopListCap];
    __shared__ int32_t  list_r[kLoopListCap];
    __shared__ int32_t  list_m[kLoopListCap];
    __shared__ int32_t  list_n;
    __shared__ uint64_t wave_d[kLoopWaves];
    __shared__ int32_t  wave_r[kLoopWaves];
    __shared__ uint64_t last_d;
    __shared__ int32_t  last_r;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qi = blockIdx.x;
    const int32_t q = job.query_index[qi];
    const double qt = job.query_travel[qi];
    const double qx = job.x[q], qy = job.y[q];
    const int32_t qmap = job.map[q];
    const bool per_map = job.one_per_map != 0;

    /* p = the first r in [0, n_ref) with query_travel - travel[r] < threshold, or n_ref */
    int lo = 0, hi = job.n_ref;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (qt - job.travel[mid] < job.travel_threshold)
            hi = mid;
        else
            lo = mid + 1;
    }
    const int p = lo;

    if (per_map) {
        const int words = (job.n_maps + 31) >> 5;
        for (int w = tid; w < words; w += kLoopBlock)
            taken[w] = 0;
    }
    if (tid == 0) {
        list_n = 0;
        last_d = 0;
        last_r = -1;                /* every key (d >= 0, r >= 0) is above it */
    }
    __syncthreads();

    /* d2 of (q, r) as the host forms it; false: not eligible */
    auto pair_key = [&](int r, uint64_t& d, int32_t& m) {
        const double dx = job.x[r] - qx;
        const double dy = job.y[r] - qy;
        const double xx = dx * dx;
        const double yy = dy * dy;
        const double d2 = xx + yy;
        if (!(d2 < job.t2))
            return false;
        m = job.map[r];
        if (m == qmap)
            return false;
        d = (uint64_t)__double_as_longlong(d2);
        return true;
    };

    for (int r = tid; r < p; r += kLoopBlock) {
        uint64_t d;
        int32_t m;
        if (!pair_key(r, d, m))
            continue;
        const int slot = atomicAdd(&list_n, 1);
        if (slot < kLoopListCap) {
            list_d[slot] = d;
            list_r[slot] = r;
            list_m[slot] = m;
        }
    }
    __syncthreads();
    const int n_eligible = list_n;              /* <= p <= 2^20 */
    const bool listed = n_eligible <= kLoopListCap;
    if (tid == 0) {
        job.eligible[qi] = n_eligible;
        job.prefix[qi] = p;
    }

    csm_loop_candidate* const rec = job.out + (size_t)qi * job.k;
    const int rounds = per_map ? job.k : min(job.k, n_eligible);
    int used = 0;
    for (; used < rounds; ++used) {
        const uint64_t ld = last_d;
        const int32_t lr = last_r;
        LoopKey best = { ~0ull, -1 };
        auto consider = [&](uint64_t d, int32_t r, int32_t m) {
            if (!loop_key_less(ld, lr, d, r) || !loop_key_less(d, r, best.d, best.r))
                return;
            if (per_map && ((taken[m >> 5] >> (m & 31)) & 1u))
                return;
            best.d = d;
            best.r = r;
        };
        if (listed) {
            for (int i = tid; i < n_eligible; i += kLoopBlock)
                consider(list_d[i], list_r[i], list_m[i]);
        } else {
            for (int r = tid; r < p; r += kLoopBlock) {
                uint64_t d;
                int32_t m;
                if (pair_key(r, d, m))
                    consider(d, r, m);
            }
        }
        best = loop_key_min_wave(best);
        if (lane == 0) {
            wave_d[wave] = best.d;
            wave_r[wave] = best.r;
        }
        __syncthreads();
        LoopKey all = { wave_d[0], wave_r[0] };
#pragma unroll
        for (int w = 1; w < kLoopWaves; ++w)
            if (loop_key_less(wave_d[w], wave_r[w], all.d, all.r)) {
                all.d = wave_d[w];
                all.r = wave_r[w];
            }
        const bool found = all.r >= 0;
        if (found && tid == 0) {
            const int32_t m = job.map[all.r];
            csm_loop_candidate c;
            c.query_scan_index = q;
            c.ref_scan_index = all.r;
            c.ref_map_index = m;
            c.reserved = 0;
            c.dist_sq = __longlong_as_double((long long)all.d);
            rec[used] = c;
            last_d = all.d;
            last_r = all.r;
            if (per_map)
                taken[m >> 5] |= 1u << (m & 31);
        }
        __syncthreads();            /* last_*, taken and wave_* are settled before the next round reads or writes them */
        if (!found)
            break;
    }
    for (int s = used + tid; s < job.k; s += kLoopBlock) {
        csm_loop_candidate c;
        c.query_scan_index = q;
        c.ref_scan_index = -1;
        c.ref_map_index = -1;
        c.reserved = 0;
        c.dist_sq = 0.0;
        rec[s] = c;
    }
    if (tid == 0)
        job.counts[qi] = used;
}

} /* namespace csm */
