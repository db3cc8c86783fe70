/* csm_volume_kernels.hip -- integer moments of a scored window's whole volume around its winner (included
 * by csm_volume_api.hip).
 *
 * Input: the window's S / K dumps and coarse known counts (PeakJob, csm_peaks.hpp) and the winner that one
 * selection round left in job.out[0]. An eligible candidate weighs W[(key_b - key) >> bin_shift] (a
 * fixed-point table the host computed; 0 past its last bin), and the sums of w, w d, w d_a d_b over
 * the offsets d = (x - x_b, y - y_b, t - t_b) are exact int64: integer adds commute, so the result does
 * not depend on how the volume is cut over lanes and workgroups.
 *   k_volume_moments  (blocks of the window, window): streams a contiguous chunk of the volume ->
 *                     one VolSums per workgroup;
 *   k_volume_reduce   (1, window): adds the window's records and writes its csm_volume_moments.
 * A lane decomposes its first candidate index once; after that t, x, y and the coarse node follow from
 * running counters (a stride of kVolBlock candidates is a fixed step in every digit), so the loop holds
 * no integer division. No atomics. */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csm_score_common.hpp"
#include "csm_peaks.hpp"

namespace csm {

constexpr int kVolBlock = 256;      /* threads per workgroup (4 wave64) */
constexpr int kVolSums = 12;        /* m0, m1[3], m2[6], support, border support */

struct VolSums {
    long long v[kVolSums];
};

struct VolJob {
    const uint32_t* table;      /* [CSM_VOLUME_BINS] weights of this window's beam count */
    VolSums* partial;           /* [blocks of the window's PeakJob] */
    csm_volume_moments* out;
    int32_t bin_shift, pad;
};

__device__ __forceinline__ long long shfl_xor_i64(long long v, int m)
{
    return (long long)shfl_xor_u64((unsigned long long)v, m);
}

__global__ __launch_bounds__(kVolBlock) void k_volume_moments(const PeakJob* jobs, const VolJob* vjobs)
{
    __shared__ uint32_t sm_w[CSM_VOLUME_BINS];
    __shared__ long long sm_red[kVolBlock / 64][kVolSums];
    const PeakJob& job = jobs[blockIdx.y];
    const VolJob& vj = vjobs[blockIdx.y];
    if ((int)blockIdx.x >= job.blocks || job.state[0] == 0)     /* no winner: k_volume_reduce writes zeros */
        return;
    const int tid = threadIdx.x;
    for (int i = tid; i < CSM_VOLUME_BINS; i += kVolBlock)
        sm_w[i] = vj.table[i];
    __syncthreads();

    const csm_result best = job.out[0];
    const int bx = best.best_x - job.x_lo, by = best.best_y - job.y_lo, bt = best.best_theta + job.win_theta;
    const unsigned long long bkey = best.key;
    const int shift = vj.bin_shift;
    const int nx = job.nx, ny = job.ny, L = job.L, nxc = nx / L, nyc = ny / L, nt = job.n_theta;
    const long total = (long)nt * nx * ny;
    const long lo = (long)blockIdx.x * job.chunk, hi = min(total, lo + job.chunk);

    /* the digits of kVolBlock in the mixed radix (t | xq, fx | yq, fy): the step between a lane's candidates */
    int s_fy, s_yq, s_fx, s_xq, s_t;
    {
        int q = kVolBlock;
        s_fy = q % L; q /= L;
        s_yq = q % nyc; q /= nyc;
        s_fx = q % L; q /= L;
        s_xq = q % nxc; q /= nxc;
        s_t = q;
    }
    long ci = lo + tid;
    int fy, yq, fx, xq, t;
    {
        long q = ci;
        fy = (int)(q % L); q /= L;
        yq = (int)(q % nyc); q /= nyc;
        fx = (int)(q % L); q /= L;
        xq = (int)(q % nxc); q /= nxc;
        t = (int)q;
    }
    long long a[kVolSums];
#pragma unroll
    for (int i = 0; i < kVolSums; ++i)
        a[i] = 0;
    const uint16_t* const ck = job.ck;
    const int min_known = job.min_known;
    for (; ci < hi; ci += kVolBlock) {
        const unsigned long long key = 32268ull * job.k[ci] + 499ull * (unsigned long long)job.s[ci];
        const bool eligible = !ck || (int)ck[((size_t)t * nxc + xq) * nyc + yq] >= min_known;
        /* the winner holds the greatest key of the eligible candidates: the difference is >= 0 */
        const unsigned long long bin = (bkey - key) >> shift;
        if (eligible && key <= bkey && bin < (unsigned long long)CSM_VOLUME_BINS) {
            const uint32_t w = sm_w[(int)bin];
            if (w) {
                const int xi = xq * L + fx, yi = yq * L + fy;
                const int dx = xi - bx, dy = yi - by, dt = t - bt;
                const long long wl = (long long)w;
                a[0] += wl;
                a[1] += wl * dx;
                a[2] += wl * dy;
                a[3] += wl * dt;
                a[4] += wl * (dx * dx);         /* |d| < 2^13 (the entry's range check): 32-bit products */
                a[5] += wl * (dx * dy);
                a[6] += wl * (dx * dt);
                a[7] += wl * (dy * dy);
                a[8] += wl * (dy * dt);
                a[9] += wl * (dt * dt);
                a[10] += 1;
                a[11] += (xi == 0 || xi == nx - 1 || yi == 0 || yi == ny - 1 || t == 0 || t == nt - 1) ? 1 : 0;
            }
        }
        /* advance by kVolBlock candidates: add the step digit by digit, carrying upwards */
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
#pragma unroll
    for (int i = 0; i < kVolSums; ++i) {
        long long v = a[i];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
            v += shfl_xor_i64(v, m);
        a[i] = v;
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int i = 0; i < kVolSums; ++i)
            sm_red[tid >> 6][i] = a[i];
    }
    __syncthreads();
    if (tid < kVolSums) {
        long long v = 0;
        for (int w = 0; w < kVolBlock / 64; ++w)
            v += sm_red[w][tid];
        vj.partial[blockIdx.x].v[tid] = v;
    }
}

__global__ __launch_bounds__(kVolBlock) void k_volume_reduce(const PeakJob* jobs, const VolJob* vjobs)
{
    __shared__ long long sm_red[kVolBlock / 64][kVolSums];
    const PeakJob& job = jobs[blockIdx.x];
    const VolJob& vj = vjobs[blockIdx.x];
    const int tid = threadIdx.x;
    const bool found = job.state[0] != 0;
    long long a[kVolSums];
#pragma unroll
    for (int i = 0; i < kVolSums; ++i)
        a[i] = 0;
    if (found && tid < job.blocks) {        /* blocks <= kPeakBlocksMax == kVolBlock */
        const VolSums p = vj.partial[tid];
#pragma unroll
        for (int i = 0; i < kVolSums; ++i)
            a[i] = p.v[i];
    }
#pragma unroll
    for (int i = 0; i < kVolSums; ++i) {
        long long v = a[i];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
            v += shfl_xor_i64(v, m);
        a[i] = v;
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int i = 0; i < kVolSums; ++i)
            sm_red[tid >> 6][i] = a[i];
    }
    __syncthreads();
    if (tid != 0)
        return;
    long long v[kVolSums];
    for (int i = 0; i < kVolSums; ++i) {
        v[i] = 0;
        for (int w = 0; w < kVolBlock / 64; ++w)
            v[i] += sm_red[w][i];
    }
    csm_volume_moments r;
    r.best = job.out[0];            /* zero when no winner was written */
    r.m0 = v[0];
    for (int i = 0; i < 3; ++i)
        r.m1[i] = v[1 + i];
    for (int i = 0; i < 6; ++i)
        r.m2[i] = v[4 + i];
    r.support = v[10];
    r.border_support = v[11];
    r.bin_shift = vj.bin_shift;
    r.reserved = 0;
    *vj.out = r;
}

} /* namespace csm */
