/* csm_consistency_kernels.hip -- pairwise consistency of loop edges and the largest consistent set (included by
 * csm_consistency_api.hip; the rule is in include/csm_hip.h, csm_loop_consistency, and DESIGN.md 4o). gfx950 only.
 *
 * lc_pair is THE pair function: __host__ __device__, the host restatement and k_lc_pairs call the same text. It
 * uses +, -, *, / and fmod in f64 and nothing else (no trigonometry: every cosine and sine arrives in the
 * records, taken by glibc on the host), every sum and product in the order written, and the unit is compiled
 * with -ffp-contract=off: chi^2 has the same bits on both sides.
 *
 *   k_lc_pairs   256 threads = 4 wavefronts; a workgroup owns a tile of 64 row edges x 64 column edges. The 64
 *                column records are gathered once, coalesced, into LDS (field-major: lane-contiguous reads); a
 *                lane keeps its column's record in registers. A wavefront takes every fourth row of the tile;
 *                the row's record is wave-uniform. The lane of (row i, column j) evaluates the pair (min, max),
 *                so both triangles hold the same bits without atomics or a transpose; the wave's ballot is the
 *                adjacency word of (i, j / 64), stored by lane 0. Lanes past M and the diagonal give zero bits.
 *                Bad pivots are counted over i < j, per tile, into tile_bad (no atomics, nothing to clear).
 *   k_lc_degree  a wavefront per row: popcounts of its words.
 *   k_lc_rank    a thread per vertex: its rank by (degree descending, index ascending) by counting; the
 *                vertices of rank < n_seeds are the seeds, in rank order.
 *   k_lc_greedy  a workgroup per seed. The candidate set C is a bitset in LDS, and so are the counts |N(u) & C|
 *                of its members (32 KB at the cap). They are summed once (a group of G lanes per candidate, G =
 *                the row's words rounded up to a power of two, at most 64, popcount(A[u] & C) over the row's
 *                words) and then kept current: per step the key (count + 1) << 13 | (8191 - u) is reduced by
 *                maximum across the wave and the four waves, the winner joins the clique, C &= A[u], and every
 *                vertex that stays loses its neighbours among those that left -- read from the words of C \ A[u]
 *                that are not zero, one word in most steps. (Recounting every candidate in every step, the first
 *                form of this kernel, took 5.4 s at 8 192 edges and 8 seeds.)
 *   k_lc_finish  one workgroup: the winning seed (size descending, rank ascending), selected[], the info record. */
#ifndef CSM_CONSISTENCY_KERNELS_HIP
#define CSM_CONSISTENCY_KERNELS_HIP

#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include <stdint.h>

#include "../../include/csm_hip.h"
#include "csm_pg_math.hpp"

namespace csm {

static_assert(CSM_LOOP_CONSISTENCY_MAX_EDGES == 8192, "the 13-bit index fields of the reduction keys");

constexpr int kLcBlock = 256;
constexpr int kLcWaves = kLcBlock / 64;
constexpr int kLcTile = 64;                     /* rows and columns of a tile of k_lc_pairs */
constexpr int kLcMaxWords = CSM_LOOP_CONSISTENCY_MAX_EDGES / 64;

/* an edge's record: everything lc_pair reads of it, as doubles */
enum {
    kLcZx, kLcZy, kLcZt, kLcZc, kLcZs,                        /* z and cos / sin of z.theta */
    kLcS00, kLcS10, kLcS11, kLcS20, kLcS21, kLcS22,           /* Sigma = Lambda^-1, lower triangle */
    kLcSx, kLcSy, kLcSc, kLcSs, kLcSt, kLcSl,                 /* local map node: p, cos, sin, theta, travel */
    kLcTx, kLcTy, kLcTc, kLcTs, kLcTt, kLcTl,                 /* scan node: the same */
    kLcPad,
    kLcRec                                                    /* = 24 doubles */
};
static_assert(kLcRec == 24, "192-byte records");

/* J S J^T of a 3x3 J = [[a, b, g0], [c, d, g1], [0, 0, w]] and a symmetric S given by its lower triangle, lower
 * triangle out (m00 m10 m11 m20 m21 m22). T = J S first (every entry T_rk = (J_r0 S_0k + J_r1 S_1k) + J_r2 S_2k),
 * then M_rc = (T_r0 J_c0 + T_r1 J_c1) + T_r2 J_c2 for r >= c. J's last row is (0, 0, w): its products with the
 * zeros are written out, so the text is one generic 3x3 congruence and every implementation rounds alike. */
__host__ __device__ inline void lc_congruence(const double J[9], const double* S, double m[6])
{
    const double s[9] = { S[0], S[1], S[3], S[1], S[2], S[4], S[3], S[4], S[5] };
    double t[9];
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k)
            t[3 * r + k] = (J[3 * r] * s[k] + J[3 * r + 1] * s[3 + k]) + J[3 * r + 2] * s[6 + k];
    int q = 0;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c <= r; ++c)
            m[q++] = (t[3 * r] * J[3 * c] + t[3 * r + 1] * J[3 * c + 1]) + t[3 * r + 2] * J[3 * c + 2];
}

/* The cycle test of the pair (a, b) = (edge i, edge j), i < j. Returns 0 and chi^2, or 1 when a
 * pivot of M is not positive and finite (chi^2 is not written). drift: the three variances per metre. */
__host__ __device__ inline int lc_pair(const double* a, const double* b, const double* drift, double* chi2)
{
    /* t_B = R_ti^T (p_tj - p_ti), R_B = R_ti^T R_tj */
    const double bx = b[kLcTx] - a[kLcTx], by = b[kLcTy] - a[kLcTy];
    const double tbx = a[kLcTc] * bx + a[kLcTs] * by;
    const double tby = a[kLcTc] * by - a[kLcTs] * bx;
    const double cb = a[kLcTc] * b[kLcTc] + a[kLcTs] * b[kLcTs];
    const double sb = a[kLcTc] * b[kLcTs] - a[kLcTs] * b[kLcTc];
    /* t_C = -R_zj^T t_zj, R_C = R_zj^T */
    const double tcx = -(b[kLcZc] * b[kLcZx] + b[kLcZs] * b[kLcZy]);
    const double tcy = -(b[kLcZc] * b[kLcZy] - b[kLcZs] * b[kLcZx]);
    const double cc = b[kLcZc], sc = -b[kLcZs];
    /* t_D = R_sj^T (p_si - p_sj) */
    const double dx = a[kLcSx] - b[kLcSx], dy = a[kLcSy] - b[kLcSy];
    const double tdx = b[kLcSc] * dx + b[kLcSs] * dy;
    const double tdy = b[kLcSc] * dy - b[kLcSs] * dx;
    /* u = t_B + R_B (t_C + R_C t_D) */
    const double wx = tcx + (cc * tdx - sc * tdy);
    const double wy = tcy + (sc * tdx + cc * tdy);
    const double ux = tbx + (cb * wx - sb * wy);
    const double uy = tby + (sb * wx + cb * wy);
    /* e */
    double e[3];
    e[0] = a[kLcZx] + (a[kLcZc] * ux - a[kLcZs] * uy);
    e[1] = a[kLcZy] + (a[kLcZs] * ux + a[kLcZc] * uy);
    e[2] = pg_normalize_angle(((a[kLcZt] + (b[kLcTt] - a[kLcTt])) - b[kLcZt]) + (a[kLcSt] - b[kLcSt]));
    /* J_i = [[I, R_zi J u], [0, 1]], J u = (-u_y, u_x) */
    const double ji[9] = { 1.0, 0.0, a[kLcZc] * (-uy) - a[kLcZs] * ux,
                           0.0, 1.0, a[kLcZs] * (-uy) + a[kLcZc] * ux,
                           0.0, 0.0, 1.0 };
    /* R_Q = (R_zi R_B) R_C; J_j = [[-R_Q, R_Q J (t_zj - t_D)], [0, -1]] */
    const double c1 = a[kLcZc] * cb - a[kLcZs] * sb, s1 = a[kLcZs] * cb + a[kLcZc] * sb;
    const double cq = c1 * cc - s1 * sc, sq = s1 * cc + c1 * sc;
    const double vx = b[kLcZx] - tdx, vy = b[kLcZy] - tdy;
    const double jj[9] = { -cq, sq, cq * (-vy) - sq * vx,
                           -sq, -cq, sq * (-vy) + cq * vx,
                           0.0, 0.0, -1.0 };
    double mi[6], mj[6];
    lc_congruence(ji, a + kLcS00, mi);
    lc_congruence(jj, b + kLcS00, mj);
    /* the drift term, unrotated: l_ij diag(drift) */
    const double l = fabs(a[kLcTl] - b[kLcTl]) + fabs(a[kLcSl] - b[kLcSl]);
    double M[9];
    M[0] = (mi[0] + mj[0]) + l * drift[0];
    M[3] = mi[1] + mj[1];
    M[4] = (mi[2] + mj[2]) + l * drift[1];
    M[6] = mi[3] + mj[3];
    M[7] = mi[4] + mj[4];
    M[8] = (mi[5] + mj[5]) + l * drift[2];
    M[1] = M[3];
    M[2] = M[6];
    M[5] = M[7];
    double f[6], x[3];
    pg_ldl3(M, f);
    for (int k = 0; k < 3; ++k)
        if (!(f[k] > 0.0) || !(f[k] <= DBL_MAX))
            return 1;
    pg_ldl3_solve(f, e[0], e[1], e[2], x);
    *chi2 = (e[0] * x[0] + e[1] * x[1]) + e[2] * x[2];
    return 0;
}

struct LcJob {
    const double* rec;            /* [M][kLcRec] */
    uint64_t* adj;                /* [M][W] */
    double*   chi2;               /* [M][M] or null */
    uint32_t* tile_bad;           /* [W * W] bad pivots over i < j of each tile */
    int32_t*  degree;             /* [M] */
    int32_t*  seeds;              /* [n_seeds] vertices in rank order */
    int32_t*  seed_size;          /* [n_seeds] */
    uint64_t* seed_bits;          /* [n_seeds][W] */
    int32_t*  selected;           /* [M] */
    csm_loop_consistency_info* info;
    double gate;
    double drift[3];
    int32_t M, W, n_seeds, group; /* group: lanes per candidate in k_lc_greedy */
};

__global__ __launch_bounds__(kLcBlock) void k_lc_pairs(LcJob job)
{
    __shared__ double col[kLcRec * kLcTile];
    __shared__ uint32_t wave_bad[kLcWaves];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     /* the row's loads are scalar loads */
    const int M = job.M;
    const int j0 = blockIdx.x * kLcTile, i0 = blockIdx.y * kLcTile;
    for (int q = tid; q < kLcRec * kLcTile; q += kLcBlock) {
        const int c = q / kLcRec, k = q - c * kLcRec;
        col[k * kLcTile + c] = j0 + c < M ? job.rec[(size_t)(j0 + c) * kLcRec + k] : 0.0;
    }
    __syncthreads();
    const int j = j0 + lane;
    double cj[kLcRec];
#pragma unroll
    for (int k = 0; k < kLcRec; ++k)
        cj[k] = col[k * kLcTile + lane];
    uint32_t bad = 0;
    const int i_end = min(i0 + kLcTile, M);
    for (int i = i0 + wave; i < i_end; i += kLcWaves) {
        const double* const ri = job.rec + (size_t)i * kLcRec;     /* wave-uniform */
        const bool swap = i > j;
        double a[kLcRec], b[kLcRec];
#pragma unroll
        for (int k = 0; k < kLcRec; ++k) {
            const double r = ri[k];
            a[k] = swap ? cj[k] : r;
            b[k] = swap ? r : cj[k];
        }
        double chi = 0.0;
        bool ok = false;
        if (j < M && j != i) {
            const int pivot = lc_pair(a, b, job.drift, &chi);
            if (pivot) {
                chi = (double)INFINITY;
                bad += i < j ? 1u : 0u;
            } else {
                ok = chi <= job.gate;
            }
        }
        const uint64_t word = __ballot(ok);
        if (lane == 0)
            job.adj[(size_t)i * job.W + blockIdx.x] = word;
        if (job.chi2 && j < M)
            job.chi2[(size_t)i * M + j] = chi;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
        bad += (uint32_t)__shfl_xor((int)bad, m, 64);
    if (lane == 0)
        wave_bad[wave] = bad;
    __syncthreads();
    if (tid == 0) {
        uint32_t s = 0;
        for (int w = 0; w < kLcWaves; ++w)
            s += wave_bad[w];
        job.tile_bad[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(kLcBlock) void k_lc_degree(LcJob job)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kLcWaves + (threadIdx.x >> 6);
    if (i >= job.M)
        return;
    int d = 0;
    for (int w = lane; w < job.W; w += 64)
        d += __popcll(job.adj[(size_t)i * job.W + w]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
        d += __shfl_xor(d, m, 64);
    if (lane == 0)
        job.degree[i] = d;
}

__global__ __launch_bounds__(kLcBlock) void k_lc_rank(LcJob job)
{
    const int v = blockIdx.x * kLcBlock + threadIdx.x;
    if (v >= job.M)
        return;
    const int dv = job.degree[v];
    int rank = 0;
    for (int u = 0; u < job.M; ++u) {
        const int du = job.degree[u];
        rank += (du > dv || (du == dv && u < v)) ? 1 : 0;
    }
    if (rank < job.n_seeds)
        job.seeds[rank] = v;
}

/* the maximum of a key over the workgroup, on every thread; `slot` is kLcWaves words of LDS */
__device__ __forceinline__ uint32_t lc_block_max(uint32_t key, uint32_t* slot)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
        key = max(key, (uint32_t)__shfl_xor((int)key, m, 64));
    __syncthreads();                /* the last round's readers are done with slot */
    if ((threadIdx.x & 63) == 0)
        slot[threadIdx.x >> 6] = key;
    __syncthreads();
    uint32_t all = slot[0];
#pragma unroll
    for (int w = 1; w < kLcWaves; ++w)
        all = max(all, slot[w]);
    return all;
}

__global__ __launch_bounds__(kLcBlock) void k_lc_greedy(LcJob job)
{
    __shared__ uint64_t C[kLcMaxWords];
    __shared__ uint64_t K[kLcMaxWords];
    __shared__ uint64_t gone[kLcMaxWords];      /* the words of C \ N(u) that are not zero, and which they are */
    __shared__ int32_t gone_w[kLcMaxWords];
    __shared__ int32_t n_gone;
    __shared__ int32_t cnt[CSM_LOOP_CONSISTENCY_MAX_EDGES];
    __shared__ uint32_t slot[kLcWaves];
    const int tid = threadIdx.x;
    const int M = job.M, W = job.W, G = job.group;
    const int seed = blockIdx.x;
    const int v0 = job.seeds[seed];
    for (int w = tid; w < W; w += kLcBlock) {
        C[w] = job.adj[(size_t)v0 * W + w];
        K[w] = w == (v0 >> 6) ? 1ull << (v0 & 63) : 0ull;
    }
    __syncthreads();
    /* cnt[u] = |N(u) & C| of every u in C: summed once over the rows' words by groups of G lanes ... */
    const int sub = tid & (G - 1);              /* this lane's place in its group */
    const int n_groups = kLcBlock / G;
    for (int u = tid / G; u < M; u += n_groups) {
        if (!((C[u >> 6] >> (u & 63)) & 1ull))
            continue;               /* uniform across the group */
        int n = 0;
        for (int w = sub; w < W; w += G)
            n += __popcll(job.adj[(size_t)u * W + w] & C[w]);
        for (int m = G >> 1; m >= 1; m >>= 1)
            n += __shfl_xor(n, m, 64);
        if (sub == 0)
            cnt[u] = n;
    }
    __syncthreads();
    int size = 1;
    /* ... and then kept current: a step takes the vertices R = C \ N(u) out of C, and every u that stays loses
     * its neighbours in R. Only the words of R that are not zero are visited (most steps remove u alone), so
     * a search costs O(M W) words in all and not per step. Integers: the counts are those a recount would give.
     * At most M - 1 steps: every step takes a vertex out of C. */
    for (int step = 1; step < M; ++step) {
        uint32_t key = 0;
        for (int u = tid; u < M; u += kLcBlock)
            if ((C[u >> 6] >> (u & 63)) & 1ull)
                key = max(key, ((uint32_t)(cnt[u] + 1) << 13) | (uint32_t)(CSM_LOOP_CONSISTENCY_MAX_EDGES - 1 - u));
        key = lc_block_max(key, slot);
        if (!key)
            break;                  /* C is empty */
        const int u = CSM_LOOP_CONSISTENCY_MAX_EDGES - 1 - (int)(key & (CSM_LOOP_CONSISTENCY_MAX_EDGES - 1));
        if (tid == 0) {
            K[u >> 6] |= 1ull << (u & 63);
            n_gone = 0;
        }
        __syncthreads();
        if (tid < W) {              /* W <= kLcMaxWords <= kLcBlock: one word per thread */
            const uint64_t c = C[tid];
            const uint64_t stay = c & job.adj[(size_t)u * W + tid];
            C[tid] = stay;
            if (c != stay) {
                const int s = atomicAdd(&n_gone, 1);        /* the list's order does not matter: a sum */
                gone_w[s] = tid;
                gone[s] = c & ~stay;
            }
        }
        __syncthreads();
        const int ng = n_gone;
        for (int v = tid; v < M; v += kLcBlock) {
            if (!((C[v >> 6] >> (v & 63)) & 1ull))
                continue;
            int d = 0;
            for (int s = 0; s < ng; ++s)
                d += __popcll(job.adj[(size_t)v * W + gone_w[s]] & gone[s]);
            cnt[v] -= d;
        }
        ++size;
        __syncthreads();
    }
    __syncthreads();
    for (int w = tid; w < W; w += kLcBlock)
        job.seed_bits[(size_t)seed * W + w] = K[w];
    if (tid == 0)
        job.seed_size[seed] = size;
}

__global__ __launch_bounds__(kLcBlock) void k_lc_finish(LcJob job, int n_tiles)
{
    __shared__ uint32_t slot[kLcWaves];
    __shared__ long long sum_deg[kLcBlock], sum_bad[kLcBlock];
    const int tid = threadIdx.x;
    /* the largest clique, ties to the seed of better rank */
    uint32_t key = 0;
    for (int s = tid; s < job.n_seeds; s += kLcBlock)
        key = max(key, ((uint32_t)job.seed_size[s] << 13) | (uint32_t)(CSM_LOOP_CONSISTENCY_MAX_EDGES - 1 - s));
    key = lc_block_max(key, slot);
    const int win = CSM_LOOP_CONSISTENCY_MAX_EDGES - 1 - (int)(key & (CSM_LOOP_CONSISTENCY_MAX_EDGES - 1));
    for (int u = tid; u < job.M; u += kLcBlock)
        job.selected[u] = (int32_t)((job.seed_bits[(size_t)win * job.W + (u >> 6)] >> (u & 63)) & 1ull);
    long long d = 0, b = 0;
    for (int u = tid; u < job.M; u += kLcBlock)
        d += job.degree[u];
    for (int t = tid; t < n_tiles; t += kLcBlock)
        b += job.tile_bad[t];
    sum_deg[tid] = d;
    sum_bad[tid] = b;
    __syncthreads();
    if (tid == 0) {
        for (int t = 1; t < kLcBlock; ++t) {
            d += sum_deg[t];
            b += sum_bad[t];
        }
        csm_loop_consistency_info r;
        r.consistent_pairs = d / 2;
        r.bad_pivots = b;
        r.clique_size = (int32_t)(key >> 13);
        r.winning_seed = job.seeds[win];
        r.seeds_run = job.n_seeds;
        r.reserved = 0;
        *job.info = r;
    }
}

} /* namespace csm */
#endif
