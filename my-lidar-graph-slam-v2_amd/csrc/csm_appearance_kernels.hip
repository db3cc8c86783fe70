/* csm_appearance_kernels.hip -- scan descriptors and the loop search by appearance (included by
 * csm_appearance_api.hip; the rule is in include/csm_hip.h, "loop search by appearance"). gfx950 only. All
 * results are integers, so nothing depends on which lane met a beam or a pair.
 *
 *   k_scan_descriptors       256 threads, one workgroup per scan. The two edge tables and a histogram of the
 *                            cells (32 bits per cell) in LDS; every lane strides over the scan's beams with
 *                            coalesced f64 loads, finds ring and sector by ap_greatest_le (a binary search on
 *                            the table: comparisons only) and counts with one LDS atomic. The cells leave as
 *                            min(count, 255).
 *   k_appearance_ring_sums   one thread per (node, ring): the ring's byte sum, four bytes per v_sad_u8
 *                            against zero.
 *   k_appearance_pairs       256 threads = 4 wavefronts; workgroup (x, y) takes query x of the chunk and
 *                            reference nodes [y, y + 1) * CSM_APPEARANCE_REF_CHUNK of its prefix. The query's
 *                            descriptor is staged in LDS with its sector axis doubled, once per byte phase:
 *                            image[ph][ring][j] = Q[ring][(j + ph) mod S] for j in [0, 2 S), so the four
 *                            bytes Q[ring][(4 w + s + 0..3) mod S] are the aligned dword w + s / 4 of row ring
 *                            of image s mod 4. The images are kApPhasePad dwords apart modulo 32, so the 32
 *                            lanes of a half wave (4 phases x 8 dword offsets) read 32 different banks. A
 *                            wavefront takes one reference node at a time: ring sums and ring distance by a
 *                            wave reduction; a pair that fails a gate costs nothing more; otherwise lane l
 *                            scores shifts l and l + 64 (lanes at or above S idle), one v_sad_u8 per dword
 *                            of the image against the reference's dword. The reference node is wave-uniform
 *                            (readfirstlane) and the descriptors and the pair table come in as __restrict__
 *                            kernel arguments of their own, which is what lets the compiler read the
 *                            reference through scalar loads (s_load_dwordx8 per eight v_sad_u8) and not
 *                            through the LDS or the vector memory path. The minimum of L1 << 8 | s goes
 *                            across the wave by xor shuffles; lane 0 writes the pair's word into the pair
 *                            table: that minimum, or kApNoPair.
 *   k_appearance_select      256 threads, one workgroup per query of the chunk: the rounds of k_loop_search
 *                            over the key distance << 32 | r, read from the pair table (no LDS list: a
 *                            round's pass over the prefix reads 4 bytes per pair). Every thread ends a round
 *                            with the same winner in registers; thread 0 writes the record.
 *
 * Every kernel recomputes a query's prefix length by the same uniform binary search as k_loop_search. */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/csm_hip.h"

namespace csm {

constexpr int kApBlock = 256;
constexpr int kApWaves = kApBlock / 64;
constexpr int kApMapWords = CSM_LOOP_SEARCH_MAX_MAPS / 32;
constexpr int kApMaxCells = CSM_DESCRIPTOR_MAX_RINGS * CSM_DESCRIPTOR_MAX_SECTORS;
constexpr int kApPhasePad = 8;              /* the phase images' pitch is this modulo 32 dwords */
constexpr uint32_t kApNoPair = 0xffffffffu; /* above every L1 << 8 | s (L1 < 2^20) */

/* dwords between two phase images of a query: rings * (2 S / 4) rounded up to kApPhasePad modulo 32 */
__host__ __device__ inline int ap_phase_pitch(int n_rings, int n_sectors)
{
    const int base = n_rings * (n_sectors / 2);
    return base + ((kApPhasePad - base % 32 + 32) % 32);
}

/* the greatest k in [0, n) with edge[k] <= v; the caller has checked edge[0] <= v < edge[n] */
__host__ __device__ inline int ap_greatest_le(const double* edge, int n, double v)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (edge[mid] <= v)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__host__ __device__ inline bool ap_finite(double v)
{
    uint64_t b;
    __builtin_memcpy(&b, &v, 8);
    return (b & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

struct DescriptorJob {
    const double*  ring_edge;      /* [n_rings + 1] */
    const double*  sector_edge;    /* [n_sectors + 1] */
    const int32_t* offsets;        /* [n_scans + 1] */
    const double*  angles;
    const double*  ranges;
    uint8_t*       out;            /* [n_scans][n_rings * n_sectors] */
    int32_t*       beams_used;     /* [n_scans] */
    int32_t n_rings, n_sectors;
};

struct AppearanceJob {
    const uint32_t* desc;          /* [n_scan][cells / 4]: four sectors per dword */
    uint16_t*       ring_sum;      /* [n_scan][n_rings] */
    const double*   travel;        /* [n_scan] */
    const int32_t*  map;           /* [n_scan] */
    const int32_t*  query_index;   /* [n_q] */
    const double*   query_travel;  /* [n_q] */
    uint32_t*       table;         /* [queries of the chunk][n_ref]: L1 << 8 | s, or kApNoPair */
    csm_appearance_candidate* out; /* [n_q * k] */
    int32_t* counts;               /* [n_q] records used */
    int32_t* prefix;               /* [n_q] p_q */
    int32_t* eligible;             /* [n_q] eligible pairs */
    double   travel_threshold;
    uint32_t max_distance, min_cell_sum;
    int32_t  n_scan, n_ref, n_maps, k, one_per_map, n_rings, n_sectors;
    int32_t  q0;                   /* the chunk's first query */
    int32_t  phase_pitch;          /* ap_phase_pitch(n_rings, n_sectors) */
};

__device__ __forceinline__ uint32_t ap_wave_sum(uint32_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
        v += (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}

__device__ __forceinline__ uint32_t ap_wave_min(uint32_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
        v = min(v, (uint32_t)__shfl_xor((int)v, m, 64));
    return v;
}

__device__ __forceinline__ uint64_t ap_wave_min64(uint64_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

/* p = the first r in [0, n_ref) with query_travel - travel[r] < threshold, or n_ref (uniform: scalar loads) */
__device__ __forceinline__ int ap_prefix(const AppearanceJob& job, double qt)
{
    int lo = 0, hi = job.n_ref;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (qt - job.travel[mid] < job.travel_threshold)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(kApBlock) void k_scan_descriptors(DescriptorJob job)
{
    __shared__ double   ring_edge[CSM_DESCRIPTOR_MAX_RINGS + 1];
    __shared__ double   sector_edge[CSM_DESCRIPTOR_MAX_SECTORS + 1];
    __shared__ uint32_t hist[kApMaxCells];
    __shared__ int32_t  used;

    const int tid = threadIdx.x;
    const int scan = blockIdx.x;
    const int nr = job.n_rings, ns = job.n_sectors, cells = nr * ns;
    for (int i = tid; i <= nr; i += kApBlock)
        ring_edge[i] = job.ring_edge[i];
    for (int i = tid; i <= ns; i += kApBlock)
        sector_edge[i] = job.sector_edge[i];
    for (int i = tid; i < cells; i += kApBlock)
        hist[i] = 0;
    if (tid == 0)
        used = 0;
    __syncthreads();

    const int b0 = job.offsets[scan], b1 = job.offsets[scan + 1];
    uint32_t mine = 0;
    for (int b = b0 + tid; b < b1; b += kApBlock) {
        const double a = job.angles[b], r = job.ranges[b];
        if (!ap_finite(a) || !ap_finite(r))
            continue;
        if (!(ring_edge[0] <= r && r < ring_edge[nr]) || !(sector_edge[0] <= a && a < sector_edge[ns]))
            continue;
        const int ring = ap_greatest_le(ring_edge, nr, r);
        const int sec = ap_greatest_le(sector_edge, ns, a);
        atomicAdd(&hist[ring * ns + sec], 1u);
        ++mine;
    }
    mine = ap_wave_sum(mine);
    if ((tid & 63) == 0)
        atomicAdd(&used, (int32_t)mine);
    __syncthreads();
    uint8_t* const out = job.out + (size_t)scan * cells;
    for (int i = tid; i < cells; i += kApBlock)
        out[i] = (uint8_t)min(hist[i], 255u);
    if (tid == 0)
        job.beams_used[scan] = used;
}

__global__ __launch_bounds__(kApBlock) void k_appearance_ring_sums(AppearanceJob job)
{
    const size_t idx = (size_t)blockIdx.x * kApBlock + threadIdx.x;
    if (idx >= (size_t)job.n_scan * job.n_rings)
        return;
    const int s4 = job.n_sectors >> 2;
    const uint32_t* const row = job.desc + idx * s4;    /* node-major, ring-minor: row idx of all rows */
    uint32_t acc = 0;
    for (int w = 0; w < s4; ++w)
        acc = __builtin_amdgcn_sad_u8(row[w], 0u, acc);
    job.ring_sum[idx] = (uint16_t)acc;                  /* <= 128 * 255 */
}

__global__ __launch_bounds__(kApBlock) void k_appearance_pairs(AppearanceJob job, const uint32_t* __restrict__ desc,
                                                               uint32_t* __restrict__ table)
{
    extern __shared__ uint32_t q_image[];               /* [4 phases][phase_pitch] */
    __shared__ uint32_t q_ring[CSM_DESCRIPTOR_MAX_RINGS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qi = job.q0 + blockIdx.x;
    const int32_t q = job.query_index[qi];
    const int p = ap_prefix(job, job.query_travel[qi]);
    const int r0 = blockIdx.y * CSM_APPEARANCE_REF_CHUNK;
    if (r0 >= p)
        return;
    const int r1 = min(p, r0 + CSM_APPEARANCE_REF_CHUNK);
    const int nr = job.n_rings, ns = job.n_sectors, s4 = ns >> 2, s2 = ns >> 1, cells4 = nr * s4;
    const int pitch = job.phase_pitch;

    const uint8_t* const qb = reinterpret_cast<const uint8_t*>(job.desc + (size_t)q * cells4);
    for (int i = tid; i < 4 * nr * s2; i += kApBlock) {
        const int ph = i / (nr * s2), rem = i - ph * (nr * s2), ring = rem / s2, jw = rem - ring * s2;
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b)
            v |= (uint32_t)qb[ring * ns + (4 * jw + ph + b) % ns] << (8 * b);
        q_image[ph * pitch + ring * s2 + jw] = v;
    }
    if (tid < nr)
        q_ring[tid] = job.ring_sum[(size_t)q * nr + tid];
    __syncthreads();
    uint32_t q_sum = 0;
    for (int i = 0; i < nr; ++i)
        q_sum += q_ring[i];
    const bool q_ok = q_sum >= job.min_cell_sum;
    const int32_t q_map = job.map[q];
    const uint32_t q_mine = lane < nr ? q_ring[lane] : 0u;
    uint32_t* const row_out = table + (size_t)blockIdx.x * job.n_ref;

    for (int rr = r0 + wave; rr < r1; rr += kApWaves) {
        const int r = __builtin_amdgcn_readfirstlane(rr);
        const uint32_t r_mine = lane < nr ? (uint32_t)job.ring_sum[(size_t)r * nr + lane] : 0u;
        const uint32_t r_sum = ap_wave_sum(r_mine);
        const uint32_t ring_dist = ap_wave_sum(r_mine > q_mine ? r_mine - q_mine : q_mine - r_mine);
        uint32_t key = kApNoPair;
        if (q_ok && job.map[r] != q_map && r_sum >= job.min_cell_sum && ring_dist <= job.max_distance) {
            const uint32_t* const rd = desc + (size_t)r * cells4;
            for (int s = lane; s < ns; s += 64) {
                const uint32_t* const ql = q_image + (s & 3) * pitch + (s >> 2);
                uint32_t acc = 0;
                for (int ring = 0; ring < nr; ++ring) {
                    const uint32_t* const qrow = ql + ring * s2;
                    const uint32_t* const rrow = rd + ring * s4;
#pragma unroll 8
                    for (int w = 0; w < s4; ++w)
                        acc = __builtin_amdgcn_sad_u8(qrow[w], rrow[w], acc);
                }
                key = min(key, (acc << 8) | (uint32_t)s);
            }
            key = ap_wave_min(key);
            if ((key >> 8) > job.max_distance)
                key = kApNoPair;
        }
        if (lane == 0)
            row_out[r] = key;
    }
}

__global__ __launch_bounds__(kApBlock) void k_appearance_select(AppearanceJob job)
{
    __shared__ uint32_t taken[kApMapWords];
    __shared__ uint64_t wave_key[kApWaves];
    __shared__ int32_t  n_listed;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qi = job.q0 + blockIdx.x;
    const int32_t q = job.query_index[qi];
    const int p = ap_prefix(job, job.query_travel[qi]);
    const bool per_map = job.one_per_map != 0;
    const uint32_t* const row = job.table + (size_t)blockIdx.x * job.n_ref;

    if (per_map) {
        const int words = (job.n_maps + 31) >> 5;
        for (int w = tid; w < words; w += kApBlock)
            taken[w] = 0;
    }
    if (tid == 0)
        n_listed = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (int r = tid; r < p; r += kApBlock)
        mine += row[r] != kApNoPair;
    mine = ap_wave_sum(mine);
    if (lane == 0)
        atomicAdd(&n_listed, (int32_t)mine);
    __syncthreads();
    const int n_eligible = n_listed;
    if (tid == 0) {
        job.eligible[qi] = n_eligible;
        job.prefix[qi] = p;
    }

    csm_appearance_candidate* const rec = job.out + (size_t)qi * job.k;
    const int rounds = per_map ? job.k : min(job.k, n_eligible);
    uint64_t last = 0;                          /* the key selected last; none before the first round */
    int used = 0;
    for (; used < rounds; ++used) {
        uint64_t best = ~0ull;
        for (int r = tid; r < p; r += kApBlock) {
            const uint32_t v = row[r];
            if (v == kApNoPair)
                continue;
            const uint64_t key = ((uint64_t)(v >> 8) << 32) | (uint32_t)r;
            if ((used > 0 && key <= last) || key >= best)
                continue;
            if (per_map) {
                const int32_t m = job.map[r];
                if ((taken[m >> 5] >> (m & 31)) & 1u)
                    continue;
            }
            best = key;
        }
        best = ap_wave_min64(best);
        if (lane == 0)
            wave_key[wave] = best;
        __syncthreads();
        uint64_t all = wave_key[0];
#pragma unroll
        for (int w = 1; w < kApWaves; ++w)
            all = wave_key[w] < all ? wave_key[w] : all;
        const bool found = all != ~0ull;
        if (found && tid == 0) {
            const int32_t r = (int32_t)(uint32_t)all;
            const uint32_t v = row[r];
            const int32_t m = job.map[r];
            uint32_t ring_dist = 0;
            for (int i = 0; i < job.n_rings; ++i) {
                const uint32_t a = job.ring_sum[(size_t)q * job.n_rings + i];
                const uint32_t b = job.ring_sum[(size_t)r * job.n_rings + i];
                ring_dist += a > b ? a - b : b - a;
            }
            csm_appearance_candidate c;
            c.query_scan_index = q;
            c.ref_scan_index = r;
            c.ref_map_index = m;
            c.shift = (int32_t)(v & 0xffu);
            c.distance = v >> 8;
            c.ring_distance = ring_dist;
            rec[used] = c;
            if (per_map)
                taken[m >> 5] |= 1u << (m & 31);
        }
        __syncthreads();            /* taken and wave_key are settled before the next round reads or writes them */
        if (!found)
            break;
        last = all;
    }
    for (int s = used + tid; s < job.k; s += kApBlock) {
        csm_appearance_candidate c;
        c.query_scan_index = q;
        c.ref_scan_index = -1;
        c.ref_map_index = -1;
        c.shift = 0;
        c.distance = 0;
        c.ring_distance = 0;
        rec[s] = c;
    }
    if (tid == 0)
        job.counts[qi] = used;
}

} /* namespace csm */
