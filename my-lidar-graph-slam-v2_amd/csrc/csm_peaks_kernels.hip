/* csm_peaks_kernels.hip -- the K best distinct poses of a scored window (included by csm_peaks_api.hip).
 *
 * Input: every candidate's exact integer sums as the exhaustive chains dump them (S uint32, K uint16,
 * [n_theta][nx][ny]). Peak j is the eligible candidate, outside the exclusion boxes of peaks 0..j-1, with
 * the greatest key 32268 K + 499 S; among equal keys the greatest f64 beam-order score; among those the
 * first in traversal rank. One round per peak, two launches per round, all windows of a chunk in each:
 *   k_peaks_argmax   (blocks of the window, window): masked arg-max of (key, -rank) with the tie count
 *                    over a contiguous chunk of the volume -> one BlockBest per workgroup;
 *   k_peaks_pick     (1, window): reduces the window's records; a tied key is replayed in f64 over the
 *                    chunks that hold it; the peak's record is written, or the window's list is closed.
 * A round reads the earlier peaks from the records in device memory; nothing returns to the host in between.
 * Keys are carried as key + 1 so that 0 means "no candidate left". */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csm_score_common.hpp"
#include "csm_peaks.hpp"

namespace csm {

/* Known count of every coarse node: hit cells that are known on the box-max(L) level at the node's
 * offset (reads outside the map are unknown), as ComputeScore on the coarse map counts them. One lane
 * per node; the lanes of a wave share the slice, so the hit indices are broadcast reads. */
__global__ __launch_bounds__(kPeakBlock) void k_peaks_coarse_known(const PeakJob* jobs)
{
    const PeakJob& job = jobs[blockIdx.y];
    uint16_t* const ck = job.ck;
    if (!ck)
        return;
    const int nxc = job.nx / job.L, nyc = job.ny / job.L, n = job.n_points;
    const long nodes = (long)job.n_theta * nxc * nyc;
    for (long gid = (long)blockIdx.x * kPeakBlock + threadIdx.x; gid < nodes; gid += (long)gridDim.x * kPeakBlock) {
        /* neighbouring lanes take neighbouring columns of one node row: their reads of a beam's cell
         * fall into the same few cache lines of one grid row */
        const int xc = (int)(gid % nxc);
        const int yc = (int)((gid / nxc) % nyc);
        const int t = (int)(gid / ((long)nyc * nxc));
        const int x = job.x_lo + xc * job.L, y = job.y_lo + yc * job.L;
        const int32_t* col = job.hit_col + (size_t)t * n;
        const int32_t* row = job.hit_row + (size_t)t * n;
        uint32_t known = 0;
        for (int i = 0; i < n; ++i) {
            const int r = row[i] + y, c = col[i] + x;
            if (r >= 0 && r < job.rows && c >= 0 && c < job.cols)
                known += job.coarse[(size_t)r * job.pitch + c] != 0;
        }
        ck[((size_t)t * nxc + xc) * nyc + yc] = (uint16_t)known;
    }
}

/* The peaks chosen so far, as candidate indices (t, xi, yi). */
struct PeakSet {
    int n;
    int t[kPeaksMax], x[kPeaksMax], y[kPeaksMax];
};

__device__ __forceinline__ void load_peaks(const PeakJob& job, int round, PeakSet& ps)
{
    ps.n = round;
    for (int j = 0; j < round; ++j) {
        const csm_result& r = job.out[j];
        ps.t[j] = r.best_theta + job.win_theta;
        ps.x[j] = r.best_x - job.x_lo;
        ps.y[j] = r.best_y - job.y_lo;
    }
}

/* key + 1 and traversal rank of candidate ci = (t nx + xi) ny + yi, or 0 when it is not eligible or
 * lies in the exclusion box of an earlier peak. */
__device__ __forceinline__ unsigned long long masked_key(const PeakJob& job, const PeakSet& ps, long ci,
                                                         unsigned long long* rank)
{
    const int yi = (int)(ci % job.ny);
    const long q = ci / job.ny;
    const int xi = (int)(q % job.nx);
    const int t = (int)(q / job.nx);
    const int L = job.L, nxc = job.nx / L, nyc = job.ny / L;
    const int xq = xi / L, yq = yi / L;
    if (job.ck && (int)job.ck[((size_t)t * nxc + xq) * nyc + yq] < job.min_known)
        return 0ull;
    for (int j = 0; j < ps.n; ++j)
        if (abs(t - ps.t[j]) <= job.excl_theta && abs(xi - ps.x[j]) <= job.excl_x && abs(yi - ps.y[j]) <= job.excl_y)
            return 0ull;
    *rank = ((((unsigned long long)t * nxc + xq) * nyc + yq) * L + (xi - xq * L)) * L + (yi - yq * L);
    return 32268ull * job.k[ci] + 499ull * (unsigned long long)job.s[ci] + 1ull;
}

__global__ __launch_bounds__(kPeakBlock) void k_peaks_argmax(const PeakJob* jobs, int round)
{
    __shared__ PeakSet ps;
    __shared__ unsigned long long red_key[kPeakBlock / 64], red_rank[kPeakBlock / 64];
    __shared__ uint32_t red_cnt[kPeakBlock / 64];
    const PeakJob& job = jobs[blockIdx.y];
    if ((int)blockIdx.x >= job.blocks || round >= job.k_max || job.state[1])
        return;
    const int tid = threadIdx.x;
    if (tid == 0)
        load_peaks(job, round, ps);
    __syncthreads();
    const long total = (long)job.n_theta * job.nx * job.ny;
    const long lo = (long)blockIdx.x * job.chunk, hi = min(total, lo + job.chunk);
    unsigned long long bkey = 0, brank = ~0ull;
    uint32_t bcnt = 0;
    for (long ci = lo + tid; ci < hi; ci += kPeakBlock) {
        unsigned long long rank = 0;
        const unsigned long long key = masked_key(job, ps, ci, &rank);
        if (key)
            best_combine(bkey, brank, bcnt, key, rank, 1u);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long k2 = shfl_xor_u64(bkey, m);
        const unsigned long long r2 = shfl_xor_u64(brank, m);
        const uint32_t c2 = __shfl_xor(bcnt, m, 64);
        best_combine(bkey, brank, bcnt, k2, r2, c2);
    }
    if ((tid & 63) == 0) {
        red_key[tid >> 6] = bkey;
        red_rank[tid >> 6] = brank;
        red_cnt[tid >> 6] = bcnt;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kPeakBlock / 64; ++w)
            best_combine(bkey, brank, bcnt, red_key[w], red_rank[w], red_cnt[w]);
        BlockBest bb;
        bb.key = bkey;
        bb.rank = brank;
        bb.count = bcnt;
        bb.pad = 0;
        job.partial[blockIdx.x] = bb;
    }
}

__global__ __launch_bounds__(kPeakBlock) void k_peaks_pick(const PeakJob* jobs, int round)
{
    __shared__ PeakSet ps;
    __shared__ unsigned long long red_key[kPeakBlock], red_rank[kPeakBlock];
    __shared__ uint32_t red_cnt[kPeakBlock];
    __shared__ double red_score[kPeakBlock];
    extern __shared__ double sm_p[];            /* [n_points] probabilities of the peak's hit cells */
    const PeakJob& job = jobs[blockIdx.x];
    if (round >= job.k_max || job.state[1])
        return;
    const int tid = threadIdx.x;
    if (tid == 0)
        load_peaks(job, round, ps);

    unsigned long long bkey = 0, brank = ~0ull;
    uint32_t bcnt = 0;
    if (tid < job.blocks) {
        const BlockBest bb = job.partial[tid];
        bkey = bb.key;
        brank = bb.rank;
        bcnt = bb.count;
    }
    red_key[tid] = bkey;
    red_rank[tid] = brank;
    red_cnt[tid] = bcnt;
    __syncthreads();
    for (int s = kPeakBlock / 2; s >= 1; s >>= 1) {
        if (tid < s) {
            best_combine(bkey, brank, bcnt, red_key[tid + s], red_rank[tid + s], red_cnt[tid + s]);
            red_key[tid] = bkey;
            red_rank[tid] = brank;
            red_cnt[tid] = bcnt;
        }
        __syncthreads();
    }
    bkey = red_key[0];
    brank = red_rank[0];
    bcnt = red_cnt[0];
    __syncthreads();
    if (bkey == 0) {                /* no candidate left */
        if (tid == 0)
            job.state[1] = 1;
        return;
    }

    const int L = job.L, nxc = job.nx / L, nyc = job.ny / L;
    uint32_t same = 1;
    if (bcnt > 1) {
        /* f64 replay of the tie set: only the chunks whose record carries the key hold a member */
        const long total = (long)job.n_theta * job.nx * job.ny;
        double ts = 0.0;
        unsigned long long tr = ~0ull;
        uint32_t tsame = 0;
        for (int b = 0; b < job.blocks; ++b) {
            if (job.partial[b].key != bkey)
                continue;
            const long lo = (long)b * job.chunk, hi = min(total, lo + job.chunk);
            for (long ci = lo + tid; ci < hi; ci += kPeakBlock) {
                unsigned long long rank = 0;
                if (masked_key(job, ps, ci, &rank) != bkey)
                    continue;
                const int yi = (int)(ci % job.ny);
                const int xi = (int)((ci / job.ny) % job.nx);
                const int t = (int)(ci / ((long)job.ny * job.nx));
                tie_combine(ts, tr, tsame, replay_score(job, t, job.x_lo + xi, job.y_lo + yi), rank, 1u);
            }
        }
        red_score[tid] = ts;
        red_rank[tid] = tr;
        red_cnt[tid] = tsame;
        __syncthreads();
        for (int s = kPeakBlock / 2; s >= 1; s >>= 1) {
            if (tid < s) {
                tie_combine(ts, tr, tsame, red_score[tid + s], red_rank[tid + s], red_cnt[tid + s]);
                red_score[tid] = ts;
                red_rank[tid] = tr;
                red_cnt[tid] = tsame;
            }
            __syncthreads();
        }
        brank = red_rank[0];
        same = red_cnt[0];
    }
    /* decode the traversal rank */
    unsigned long long q = brank;
    const int fy = (int)(q % L); q /= L;
    const int fx = (int)(q % L); q /= L;
    const int yc = (int)(q % nyc); q /= nyc;
    const int xc = (int)(q % nxc); q /= nxc;
    const int t = (int)q;
    const int xi = xc * L + fx, yi = yc * L + fy;
    const size_t ci = ((size_t)t * job.nx + xi) * job.ny + yi;
    /* the peak's f64 score as k_finalize replays a winner: gather in parallel, sum in beam order */
    {
        const int x = job.x_lo + xi, y = job.y_lo + yi;
        const int32_t* col = job.hit_col + (size_t)t * job.n_points;
        const int32_t* row = job.hit_row + (size_t)t * job.n_points;
        for (int i = tid; i < job.n_points; i += kPeakBlock) {
            const int r = row[i] + y, c = col[i] + x;
            uint32_t v = 0;
            if (r >= 0 && r < job.rows && c >= 0 && c < job.cols)
                v = job.cells[(size_t)r * job.pitch + c];
            sm_p[i] = job.lut[v];
        }
    }
    __syncthreads();
    if (tid != 0)
        return;
    double sum = 0.0;
    for (int i = 0; i < job.n_points; ++i)
        sum += sm_p[i];
    const double score = sum / (double)job.n_points;
    if (!(score > job.score_thr)) {     /* the comparison of `found` */
        job.state[1] = 1;
        return;
    }
    csm_result r;
    r.found = 1;
    r.best_x = job.x_lo + xi;
    r.best_y = job.y_lo + yi;
    r.best_theta = t - job.win_theta;
    r.key = bkey - 1ull;
    r.sum_values = job.s[ci];
    r.known = job.k[ci];
    r.tie_count = bcnt;
    r.flags = (job.chain->flags & CSM_FLAG_EDGE_BAND) |
              (bcnt > 1 ? CSM_FLAG_KEY_TIE | (same > 1 ? CSM_FLAG_F64_TIE : 0u) : 0u);
    r.score = score;
    job.out[round] = r;
    job.state[0] = round + 1;
}

} /* namespace csm */
