/* csm_prior_kernels.hip -- the winner of a scored window under a motion prior (included by
 * csm_prior_api.hip).
 *
 * Input: the window's S / K dumps and coarse known counts (PeakJob, csm_peaks.hpp) and the six quantised
 * prior terms Q (PriorJob). A candidate at offsets d = (x, y, t) from the window centre pays
 * pen = max(0, (sum Q_ab d_a d_b) >> 8) key units: pk = key - pen. Two winners come out of one pass:
 *   best        the greatest (pk, key), then the greatest f64 beam-order score, then the first in sweep order;
 *   unweighted  the greatest key, then as above: peak 0 of the peaks entries.
 *   k_prior_argmax  (blocks of the window, window): one pass over a contiguous chunk of the volume ->
 *                   one PriorBest per workgroup (both arg-max records with their tie counts);
 *   k_prior_pick    (1, window): reduces the window's records; a tied winner is replayed in f64 over the
 *                   chunks that hold it; both records, the penalty and the penalised key are written.
 * A lane takes kPriorRun candidates that are consecutive in y per step (one 16-byte load of S, one 8-byte
 * load of K) and carries the quadratic form along: a step in y adds `inc` and `inc` grows by 2 Q_yy, so
 * only a run's first candidate and a carry into x or t pay the multiplies. All sums are integers: the
 * result does not depend on how the volume is cut. No atomics. */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csm_score_common.hpp"
#include "csm_peaks.hpp"

namespace csm {

constexpr int kPriorBlock = 256;    /* threads per workgroup (4 wave64) */
constexpr int kPriorRun = 4;        /* candidates of one lane and step; a chunk is a multiple of it */

struct PriorBest {
    long long pk;               /* penalised key of the best candidate; meaningful when count > 0 */
    unsigned long long key;     /* its key */
    unsigned long long rank;    /* traversal rank of the first candidate holding (pk, key) */
    unsigned long long ukey;    /* greatest key + 1; 0 = no eligible candidate */
    unsigned long long urank;
    uint32_t count;             /* candidates sharing (pk, key); 0 = no eligible candidate */
    uint32_t ucount;            /* candidates sharing ukey */
};

struct PriorJob {
    long long Q[6];             /* xx xy xt yy yt tt */
    csm_prior_result* out;      /* zero before the launch */
    PriorBest* partial;         /* [blocks] */
    int32_t blocks, chunk;      /* blocks * chunk >= n_theta nx ny, chunk % kPriorRun == 0 */
};

/* sum_{a<=b} Q_ab d_a d_b: below 2^62 in magnitude by the entry's range check */
__device__ __forceinline__ long long prior_quad(const long long* Q, int x, int y, int t)
{
    const long long lx = x, ly = y, lt = t;
    return Q[0] * (lx * lx) + Q[1] * (lx * ly) + Q[2] * (lx * lt) + Q[3] * (ly * ly) + Q[4] * (ly * lt) +
           Q[5] * (lt * lt);
}

__device__ __forceinline__ long long prior_pen(long long quad)
{
    const long long p = quad >> 8;
    return p > 0 ? p : 0;
}

/* (pk, key, rank, count): greater pk first, then the greater key, then the smaller rank; count = 0: none */
__device__ __forceinline__ void prior_combine(long long& pk, unsigned long long& key, unsigned long long& rank,
                                              uint32_t& count, long long pk2, unsigned long long key2,
                                              unsigned long long rank2, uint32_t count2)
{
    if (count2 == 0)
        return;
    if (count == 0 || pk2 > pk || (pk2 == pk && key2 > key)) {
        pk = pk2;
        key = key2;
        rank = rank2;
        count = count2;
    } else if (pk2 == pk && key2 == key) {
        rank = rank2 < rank ? rank2 : rank;
        count += count2;
    }
}

/* The two running winners of a lane, a wave or a workgroup (prior_none(): no candidate yet). */
struct PriorAcc {
    long long pk;
    unsigned long long key, rank, ukey, urank;
    uint32_t count, ucount;

    __device__ __forceinline__ void take(const PriorAcc& o)
    {
        prior_combine(pk, key, rank, count, o.pk, o.key, o.rank, o.count);
        best_combine(ukey, urank, ucount, o.ukey, o.urank, o.ucount);
    }
    __device__ __forceinline__ PriorAcc shuffled(int m) const
    {
        PriorAcc o;
        o.pk = (long long)shfl_xor_u64((unsigned long long)pk, m);
        o.key = shfl_xor_u64(key, m);
        o.rank = shfl_xor_u64(rank, m);
        o.ukey = shfl_xor_u64(ukey, m);
        o.urank = shfl_xor_u64(urank, m);
        o.count = __shfl_xor(count, m, 64);
        o.ucount = __shfl_xor(ucount, m, 64);
        return o;
    }
};

__device__ __forceinline__ PriorAcc prior_none()
{
    PriorAcc a;
    a.pk = 0;
    a.key = 0;
    a.rank = ~0ull;
    a.ukey = 0;
    a.urank = ~0ull;
    a.count = 0;
    a.ucount = 0;
    return a;
}

/* Reduces `a` over the workgroup; every thread returns with the result. red: [kPriorBlock / 64]. */
__device__ __forceinline__ void prior_block_reduce(PriorAcc& a, PriorAcc* red, int tid)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
        a.take(a.shuffled(m));
    if ((tid & 63) == 0)
        red[tid >> 6] = a;
    __syncthreads();
    a = red[0];
    for (int w = 1; w < kPriorBlock / 64; ++w)
        a.take(red[w]);
    __syncthreads();
}

__global__ __launch_bounds__(kPriorBlock) void k_prior_argmax(const PeakJob* jobs, const PriorJob* pjobs)
{
    __shared__ PriorAcc red[kPriorBlock / 64];
    const PeakJob& job = jobs[blockIdx.y];
    const PriorJob& pj = pjobs[blockIdx.y];
    if ((int)blockIdx.x >= pj.blocks)
        return;
    const int tid = threadIdx.x;
    const int nx = job.nx, ny = job.ny, L = job.L, nxc = nx / L, nyc = ny / L;
    const long total = (long)job.n_theta * nx * ny;
    const long lo = (long)blockIdx.x * pj.chunk, hi = min(total, lo + pj.chunk);
    long long Q[6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
        Q[i] = pj.Q[i];

    /* the digits of a step of kPriorBlock runs in the mixed radix (t | xq, fx | yq, fy) */
    int s_fy, s_yq, s_fx, s_xq, s_t;
    {
        int q = kPriorBlock * kPriorRun;
        s_fy = q % L; q /= L;
        s_yq = q % nyc; q /= nyc;
        s_fx = q % L; q /= L;
        s_xq = q % nxc; q /= nxc;
        s_t = q;
    }
    long ci = lo + (long)tid * kPriorRun;
    int fy, yq, fx, xq, t;
    {
        long q = ci;
        fy = (int)(q % L); q /= L;
        yq = (int)(q % nyc); q /= nyc;
        fx = (int)(q % L); q /= L;
        xq = (int)(q % nxc); q /= nxc;
        t = (int)q;
    }
    const uint16_t* const ck = job.ck;
    const int min_known = job.min_known;
    const long long two_qyy = 2 * Q[3];
    PriorAcc acc = prior_none();
    for (; ci < hi; ci += kPriorBlock * kPriorRun) {
        uint32_t sv[kPriorRun];
        uint32_t kv[kPriorRun];
        const int nrun = (int)min((long)kPriorRun, hi - ci);
        if (nrun == kPriorRun) {        /* ci % 4 == 0 and the volumes start on 256 bytes: aligned */
            const uint4 a = *reinterpret_cast<const uint4*>(job.s + ci);
            const ushort4 b = *reinterpret_cast<const ushort4*>(job.k + ci);
            sv[0] = a.x, sv[1] = a.y, sv[2] = a.z, sv[3] = a.w;
            kv[0] = b.x, kv[1] = b.y, kv[2] = b.z, kv[3] = b.w;
        } else {
#pragma unroll
            for (int r = 0; r < kPriorRun; ++r) {
                sv[r] = r < nrun ? job.s[ci + r] : 0u;
                kv[r] = r < nrun ? job.k[ci + r] : 0u;
            }
        }
        /* the run's walk: its own copy of the digits */
        int wfy = fy, wyq = yq, wfx = fx, wxq = xq, wt = t;
        long long quad = 0, inc = 0;
        bool fresh = true;              /* the row (x, t) changed: recompute the form */
#pragma unroll
        for (int r = 0; r < kPriorRun; ++r) {
            if (r < nrun) {
                if (fresh) {
                    const int x = job.x_lo + wxq * L + wfx, y = job.y_lo + wyq * L + wfy, th = wt - job.win_theta;
                    quad = prior_quad(Q, x, y, th);
                    inc = Q[3] * (long long)(2 * y + 1) + Q[1] * (long long)x + Q[4] * (long long)th;
                    fresh = false;
                }
                const size_t node = ((size_t)wt * nxc + wxq) * nyc + wyq;
                if (!ck || (int)ck[node] >= min_known) {
                    PriorAcc c;
                    c.key = 32268ull * kv[r] + 499ull * (unsigned long long)sv[r];
                    c.pk = (long long)c.key - prior_pen(quad);
                    c.rank = (node * L + wfx) * L + wfy;
                    c.count = 1;
                    c.ukey = c.key + 1ull;
                    c.urank = c.rank;
                    c.ucount = 1;
                    acc.take(c);
                }
                /* one step in y; a carry out of y leaves the row */
                quad += inc;
                inc += two_qyy;
                if (++wfy == L) {
                    wfy = 0;
                    if (++wyq == nyc) {
                        wyq = 0;
                        fresh = true;
                        if (++wfx == L) {
                            wfx = 0;
                            if (++wxq == nxc) {
                                wxq = 0;
                                ++wt;
                            }
                        }
                    }
                }
            }
        }
        /* advance the run's start by kPriorBlock runs: add the step digit by digit, carrying upwards */
        fy += s_fy;
        int c = fy >= L;
        fy -= c ? L : 0;
        yq += s_yq + c;
        c = yq >= nyc;
        yq -= c ? nyc : 0;
        fx += s_fx + c;
        c = fx >= L;
        fx -= c ? L : 0;
        xq += s_xq + c;
        c = xq >= nxc;
        xq -= c ? nxc : 0;
        t += s_t + c;
    }
    prior_block_reduce(acc, red, tid);
    if (tid == 0) {
        PriorBest pb;
        pb.pk = acc.pk;
        pb.key = acc.key;
        pb.rank = acc.rank;
        pb.ukey = acc.ukey;
        pb.urank = acc.urank;
        pb.count = acc.count;
        pb.ucount = acc.ucount;
        pj.partial[blockIdx.x] = pb;
    }
}

/* One of the two records of a window. weighted: the winner holds (wpk, wkey) among `wcnt` candidates, the
 * first of them at `wrank`; else: key wkey among wcnt, first at wrank. A tie is replayed in f64 over the
 * chunks whose record carries the winner's pair. The whole workgroup calls it; thread 0 writes. */
__device__ __forceinline__ void prior_write_record(const PeakJob& job, const PriorJob& pj, bool weighted, long long wpk,
                                                   unsigned long long wkey, unsigned long long wrank, uint32_t wcnt,
                                                   double* red_score, unsigned long long* red_rank,
                                                   uint32_t* red_cnt, double* sm_p, int tid)
{
    if (wcnt == 0)              /* nothing eligible: the record stays zero */
        return;
    const int L = job.L, nxc = job.nx / L, nyc = job.ny / L;
    uint32_t same = 1;
    if (wcnt > 1) {
        const long total = (long)job.n_theta * job.nx * job.ny;
        double ts = 0.0;
        unsigned long long tr = ~0ull;
        uint32_t tsame = 0;
        for (int b = 0; b < pj.blocks; ++b) {
            const PriorBest pb = pj.partial[b];
            if (weighted ? (pb.count == 0 || pb.pk != wpk || pb.key != wkey) : pb.ukey != wkey + 1ull)
                continue;
            const long lo = (long)b * pj.chunk, hi = min(total, lo + pj.chunk);
            for (long ci = lo + tid; ci < hi; ci += kPriorBlock) {
                const int yi = (int)(ci % job.ny);
                const int xi = (int)((ci / job.ny) % job.nx);
                const int t = (int)(ci / ((long)job.ny * job.nx));
                const int xq = xi / L, yq = yi / L;
                const size_t node = ((size_t)t * nxc + xq) * nyc + yq;
                if (job.ck && (int)job.ck[node] < job.min_known)
                    continue;
                const unsigned long long key = 32268ull * job.k[ci] + 499ull * (unsigned long long)job.s[ci];
                if (key != wkey)
                    continue;
                const int x = job.x_lo + xi, y = job.y_lo + yi;
                if (weighted && (long long)key - prior_pen(prior_quad(pj.Q, x, y, t - job.win_theta)) != wpk)
                    continue;
                const unsigned long long rank = (node * L + (xi - xq * L)) * L + (yi - yq * L);
                tie_combine(ts, tr, tsame, replay_score(job, t, x, y), rank, 1u);
            }
        }
        red_score[tid] = ts;
        red_rank[tid] = tr;
        red_cnt[tid] = tsame;
        __syncthreads();
        for (int s = kPriorBlock / 2; s >= 1; s >>= 1) {
            if (tid < s) {
                tie_combine(ts, tr, tsame, red_score[tid + s], red_rank[tid + s], red_cnt[tid + s]);
                red_score[tid] = ts;
                red_rank[tid] = tr;
                red_cnt[tid] = tsame;
            }
            __syncthreads();
        }
        wrank = red_rank[0];
        same = red_cnt[0];
        __syncthreads();
    }
    /* decode the traversal rank */
    unsigned long long q = wrank;
    const int fy = (int)(q % L); q /= L;
    const int fx = (int)(q % L); q /= L;
    const int yc = (int)(q % nyc); q /= nyc;
    const int xc = (int)(q % nxc); q /= nxc;
    const int t = (int)q;
    const int xi = xc * L + fx, yi = yc * L + fy;
    const size_t ci = ((size_t)t * job.nx + xi) * job.ny + yi;
    const int x = job.x_lo + xi, y = job.y_lo + yi;
    /* the winner's f64 score as k_finalize replays a winner: gather in parallel, sum in beam order */
    {
        const int32_t* col = job.hit_col + (size_t)t * job.n_points;
        const int32_t* row = job.hit_row + (size_t)t * job.n_points;
        for (int i = tid; i < job.n_points; i += kPriorBlock) {
            const int r = row[i] + y, c = col[i] + x;
            uint32_t v = 0;
            if (r >= 0 && r < job.rows && c >= 0 && c < job.cols)
                v = job.cells[(size_t)r * job.pitch + c];
            sm_p[i] = job.lut[v];
        }
    }
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int i = 0; i < job.n_points; ++i)
            sum += sm_p[i];
        const double score = sum / (double)job.n_points;
        if (score > job.score_thr) {        /* the comparison of `found`, on the raw score */
            csm_result r;
            r.found = 1;
            r.best_x = x;
            r.best_y = y;
            r.best_theta = t - job.win_theta;
            r.key = wkey;
            r.sum_values = job.s[ci];
            r.known = job.k[ci];
            r.tie_count = wcnt;
            r.flags = (job.chain->flags & CSM_FLAG_EDGE_BAND) |
                      (wcnt > 1 ? CSM_FLAG_KEY_TIE | (same > 1 ? CSM_FLAG_F64_TIE : 0u) : 0u);
            r.score = score;
            if (weighted) {
                pj.out->best = r;
                pj.out->penalty = (long long)wkey - wpk;
                pj.out->penalised_key = wpk;
            } else {
                pj.out->unweighted = r;
            }
        }
    }
    __syncthreads();            /* sm_p and the reduction arrays are free again */
}

__global__ __launch_bounds__(kPriorBlock) void k_prior_pick(const PeakJob* jobs, const PriorJob* pjobs)
{
    __shared__ PriorAcc red[kPriorBlock / 64];
    __shared__ unsigned long long red_rank[kPriorBlock];
    __shared__ uint32_t red_cnt[kPriorBlock];
    __shared__ double red_score[kPriorBlock];
    extern __shared__ double sm_p[];            /* [n_points] probabilities of a winner's hit cells */
    const PeakJob& job = jobs[blockIdx.x];
    const PriorJob& pj = pjobs[blockIdx.x];
    const int tid = threadIdx.x;
    PriorAcc acc = prior_none();
    if (tid < pj.blocks) {                      /* blocks <= kPeakBlocksMax == kPriorBlock */
        const PriorBest pb = pj.partial[tid];
        acc.pk = pb.pk;
        acc.key = pb.key;
        acc.rank = pb.rank;
        acc.ukey = pb.ukey;
        acc.urank = pb.urank;
        acc.count = pb.count;
        acc.ucount = pb.ucount;
    }
    prior_block_reduce(acc, red, tid);
    prior_write_record(job, pj, true, acc.pk, acc.key, acc.rank, acc.count, red_score, red_rank, red_cnt, sm_p, tid);
    prior_write_record(job, pj, false, 0, acc.ukey - 1ull, acc.urank, acc.ucount, red_score, red_rank, red_cnt, sm_p,
                       tid);
}

} /* namespace csm */
