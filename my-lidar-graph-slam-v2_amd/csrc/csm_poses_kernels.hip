/* csm_poses_kernels.hip -- a scan scored at the poses of a set, and the measurement update of a particle set
 * (included by csm_poses_api.hip; the definitions are in include/csm_hip.h, csm_score_pose_sets and
 * csm_pose_set_update). gfx950 only.
 *
 *   k_pose_prep      one thread per beam of the call's distinct scans: (cos a, sin a, r), the device's libm.
 *   k_pose_score     256 threads = 4 wavefronts, up to kPoseGroupMax consecutive poses of ONE set per
 *                    workgroup. The first threads take cos / sin of their pose's theta once; the set's beam
 *                    triples are staged in LDS kPoseTile at a time (structure of arrays: consecutive lanes
 *                    read consecutive doubles); a wavefront owns a pose at a time, its lanes the beams.
 *                    cos / sin(theta + a) come from the addition theorems, the cell index counts only under
 *                    the certificate proj_body uses (csm_certify.hpp, reciprocal form): the same two library
 *                    calls, two products and one sum, the same bound and margin. Lanes gather their cells
 *                    and add integers; the wavefront reduces by shuffles (integer sums have no order). A
 *                    pose with any beam inside the margin is marked and listed once: the list has a slot
 *                    per pose and cannot overflow.
 *   k_pose_rescore   one wavefront per listed pose, from the indices the host computed with glibc.
 *   k_pose_weights   ONE workgroup of 1024 threads over the poses of a set: keys and eligibility, the
 *                    greatest key with its first index (packed, one maximum), then tiles of 1024 poses:
 *                    the weight from the table (in LDS), an inclusive wavefront scan of the u64 weights,
 *                    the wavefronts' totals through LDS, a running carry. Writes weights, prefix sums and
 *                    the update record.
 *   k_pose_resample  one thread per output: T_j and a binary search in the prefix sums.
 * Nothing here orders threads beyond the barriers written out. */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/csm_hip.h"
#include "csm_score_common.hpp"     /* prefix_find; the certificate (csm_certify.hpp) */

namespace csm {

constexpr int kPoseBlock = 256;
constexpr int kPoseGroupMax = 16;            /* poses per workgroup of k_pose_score, at most (measured: DESIGN 4k) */
constexpr int kPoseTile = 1024;              /* beams staged per pass: 3 x 8 KiB of LDS */
constexpr int kPoseUpdateBlock = 1024;

struct PoseTriple {
    double c, s, r;                          /* cos a_i, sin a_i, r_i */
};

/* one set of a call */
struct PoseJob {
    const uint16_t* cells;                   /* level 0 of its map */
    int32_t rows, cols, pitch, n_points;
    long long trip_at;                       /* its scan's first triple */
    long long pose_at;                       /* its first pose = its first record */
    int32_t n_poses, pad;
    double  off_x, off_y, inv_res;
    double  ang_max;                         /* max |a_i|: the angle term of the bound, taken per set */
};

struct PoseChunk {
    const PoseJob*  jobs;
    const uint32_t* pre_group;               /* [n_sets + 1] workgroups of k_pose_score before each set */
    const double*   angles;                  /* [n_beams] the distinct scans, one after the other */
    const double*   ranges;
    PoseTriple*     trips;                   /* [n_beams] */
    const double*   poses;                   /* [poses][3] */
    csm_pose_record* records;                /* [poses] */
    uint32_t*       unc;                     /* [0] marked poses, [1] records the rescore changed, [2 ..] the list */
    int32_t n_sets, n_beams, group_poses, pad;
};

/* a listed pose for k_pose_rescore */
struct PoseFix {
    uint32_t pose;                           /* its record */
    int32_t  set;
    long long hit_at;                        /* [n_points] columns, then [n_points] rows */
};

struct PoseUpdate {
    const csm_pose_record* records;
    const uint32_t* table;                   /* [CSM_VOLUME_BINS] */
    uint32_t* weights;                       /* [n_poses] */
    unsigned long long* prefix;              /* [n_poses] inclusive */
    int32_t* ancestors;                      /* [n_out] */
    csm_pose_update_info* info;
    int32_t n_poses, n_out, min_known, bin_shift;
    unsigned long long offset;
};

__device__ __forceinline__ unsigned long long pose_key(uint32_t s, uint32_t k)
{
    return 32268ull * k + 499ull * s;
}

__global__ __launch_bounds__(kPoseBlock) void k_pose_prep(PoseChunk ch)
{
    const int b = blockIdx.x * kPoseBlock + threadIdx.x;
    if (b >= ch.n_beams)
        return;
    const double a = ch.angles[b];
    PoseTriple t;
    t.c = cos(a);
    t.s = sin(a);
    t.r = ch.ranges[b];
    ch.trips[b] = t;
}

__global__ __launch_bounds__(kPoseBlock) void k_pose_score(PoseChunk ch)
{
    __shared__ double t_c[kPoseTile], t_s[kPoseTile], t_r[kPoseTile];
    __shared__ double p_x[kPoseGroupMax], p_y[kPoseGroupMax], p_c[kPoseGroupMax], p_s[kPoseGroupMax],
                      p_e[kPoseGroupMax];
    __shared__ uint32_t acc_s[kPoseGroupMax], acc_k[kPoseGroupMax], acc_u[kPoseGroupMax];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    const int si = prefix_find(ch.pre_group, ch.n_sets, blockIdx.x);        /* uniform */
    const PoseJob& job = ch.jobs[si];
    const uint16_t* const cells = job.cells;
    const int rows = job.rows, cols = job.cols, pitch = job.pitch, n_points = job.n_points;
    const long long trip_at = job.trip_at;
    const double off_x = job.off_x, off_y = job.off_y, inv_res = job.inv_res;
    const int first = ((int)blockIdx.x - (int)ch.pre_group[si]) * ch.group_poses;
    const int np = min(ch.group_poses, job.n_poses - first);              /* >= 1 */
    const long long pose0 = job.pose_at + first;

    if (tid < np) {
        const double* const p = ch.poses + 3 * (pose0 + tid);
        const double th = p[2];
        p_x[tid] = p[0];
        p_y[tid] = p[1];
        p_c[tid] = cos(th);
        p_s[tid] = sin(th);
        p_e[tid] = addition_trig_err(fabs(th) + job.ang_max);
        acc_s[tid] = acc_k[tid] = acc_u[tid] = 0u;
    }
    for (int tile0 = 0; tile0 < n_points; tile0 += kPoseTile) {
        __syncthreads();                     /* the pose table is written; the last tile is consumed */
        const int nt = min(kPoseTile, n_points - tile0);
        for (int i = tid; i < nt; i += kPoseBlock) {
            const PoseTriple t = ch.trips[trip_at + tile0 + i];
            t_c[i] = t.c;
            t_s[i] = t.s;
            t_r[i] = t.r;
        }
        __syncthreads();
        for (int p = wave; p < np; p += kPoseBlock / 64) {
            const double x = p_x[p], y = p_y[p], ct = p_c[p], st = p_s[p], trig_err = p_e[p];
            uint32_t s = 0, k = 0;
            bool uncertain = false;
            for (int i = lane; i < nt; i += 64) {
                const double ca = t_c[i], sa = t_s[i], r = t_r[i];
                const double hx = x + r * (ct * ca - st * sa);
                const double hy = y + r * (st * ca + ct * sa);
                const double qx = (hx - off_x) * inv_res, qy = (hy - off_y) * inv_res;
                const double fx = floor(qx), fy = floor(qy);
                const double mx = kCertSafety * proj_err_bound_recip(r, hx, off_x, inv_res, qx, trig_err);
                const double my = kCertSafety * proj_err_bound_recip(r, hy, off_y, inv_res, qy, trig_err);
                uncertain |= !(off_cell_edge(qx - fx, mx) && off_cell_edge(qy - fy, my));
                const int col = (int)fx, row = (int)fy;          /* |q| < 2^30 + 1: the call's check */
                if ((unsigned)col < (unsigned)cols && (unsigned)row < (unsigned)rows) {
                    const uint32_t v = cells[(size_t)row * pitch + col];
                    s += v;
                    k += v != 0u;
                }
            }
            for (int off = 32; off; off >>= 1) {
                s += __shfl_xor(s, off);
                k += __shfl_xor(k, off);
            }
            const bool any = __ballot(uncertain) != 0ull;
            if (lane == 0) {                 /* pose p belongs to this wavefront alone */
                acc_s[p] += s;
                acc_k[p] += k;
                acc_u[p] |= any ? 1u : 0u;
            }
        }
    }
    __syncthreads();
    if (tid < np) {
        csm_pose_record rec;
        rec.sum_values = acc_s[tid];
        rec.known = acc_k[tid];
        rec.flags = acc_u[tid] ? CSM_POSE_UNCERTAIN : 0u;
        rec.reserved = 0;
        ch.records[pose0 + tid] = rec;
        if (acc_u[tid]) {
            const uint32_t pos = atomicAdd(ch.unc, 1u);          /* < poses of the call: a slot per pose */
            ch.unc[2 + pos] = (uint32_t)(pose0 + tid);
        }
    }
}

__global__ __launch_bounds__(kPoseBlock) void k_pose_rescore(PoseChunk ch, const PoseFix* fixes, const int32_t* hits,
                                                             int n_fixes)
{
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * (kPoseBlock / 64) + (threadIdx.x >> 6);    /* uniform per wavefront */
    if (f >= n_fixes)
        return;
    const PoseFix fix = fixes[f];
    const PoseJob& job = ch.jobs[fix.set];
    const uint16_t* const cells = job.cells;
    const int rows = job.rows, cols = job.cols, pitch = job.pitch, n_points = job.n_points;
    const int32_t* const hit_col = hits + fix.hit_at;
    const int32_t* const hit_row = hit_col + n_points;
    uint32_t s = 0, k = 0;
    for (int i = lane; i < n_points; i += 64) {
        const int col = hit_col[i], row = hit_row[i];
        if ((unsigned)col < (unsigned)cols && (unsigned)row < (unsigned)rows) {
            const uint32_t v = cells[(size_t)row * pitch + col];
            s += v;
            k += v != 0u;
        }
    }
    for (int off = 32; off; off >>= 1) {
        s += __shfl_xor(s, off);
        k += __shfl_xor(k, off);
    }
    if (lane == 0) {
        csm_pose_record rec = ch.records[fix.pose];
        if (rec.sum_values != s || rec.known != k)
            atomicAdd(ch.unc + 1, 1u);
        rec.sum_values = s;
        rec.known = k;
        rec.flags = CSM_POSE_UNCERTAIN | CSM_POSE_HOST_PROJECTED;
        ch.records[fix.pose] = rec;
    }
}

__global__ __launch_bounds__(kPoseUpdateBlock) void k_pose_weights(PoseUpdate u)
{
    constexpr int kWaves = kPoseUpdateBlock / 64;
    __shared__ uint32_t table[CSM_VOLUME_BINS];
    __shared__ unsigned long long wave_val[kWaves];
    __shared__ unsigned long long best_sh;
    __shared__ uint32_t support_sh[kWaves];
    static_assert(CSM_VOLUME_BINS == kPoseUpdateBlock, "one table entry per thread");
    static_assert(CSM_POSE_SET_MAX_POSES == (1 << 18), "the packed maximum keeps 18 bits for the index");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = u.n_poses;
    table[tid] = u.table[tid];

    /* the greatest key of an eligible pose and the first pose that has it: bit 62 | key << 18 | (2^18 - 1 - i),
     * key < 2^42 */
    unsigned long long best = 0;
    for (int i = tid; i < n; i += kPoseUpdateBlock) {
        const csm_pose_record rec = u.records[i];
        if ((int)rec.known >= u.min_known) {
            const unsigned long long packed = (1ull << 62) | (pose_key(rec.sum_values, rec.known) << 18) |
                                              (unsigned long long)(0x3FFFF - i);
            best = best > packed ? best : packed;
        }
    }
    for (int off = 32; off; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off);
        best = best > o ? best : o;
    }
    if (lane == 0)
        wave_val[wave] = best;
    __syncthreads();
    if (tid == 0) {
        unsigned long long b = 0;
        for (int w = 0; w < kWaves; ++w)
            b = b > wave_val[w] ? b : wave_val[w];
        best_sh = b;
    }
    __syncthreads();
    best = best_sh;
    const bool found = best != 0ull;
    const unsigned long long key_max = (best & ~(1ull << 62)) >> 18;

    unsigned long long carry = 0;            /* the same in every thread */
    uint32_t support = 0;
    for (int base = 0; base < n; base += kPoseUpdateBlock) {
        const int i = base + tid;
        uint32_t w = 0;
        if (i < n && found) {
            const csm_pose_record rec = u.records[i];
            if ((int)rec.known >= u.min_known) {
                const unsigned long long bin = (key_max - pose_key(rec.sum_values, rec.known)) >> u.bin_shift;
                w = bin < (unsigned long long)CSM_VOLUME_BINS ? table[bin] : 0u;
            }
        }
        support += w != 0u;
        unsigned long long v = w;            /* inclusive scan over the wavefront */
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long o = __shfl_up(v, off);
            if (lane >= off)
                v += o;
        }
        __syncthreads();                     /* wave_val of the last tile (or of the maximum) is consumed */
        if (lane == 63)
            wave_val[wave] = v;
        __syncthreads();
        unsigned long long before = 0, total = 0;
        for (int w2 = 0; w2 < kWaves; ++w2) {
            const unsigned long long t = wave_val[w2];
            before += w2 < wave ? t : 0ull;
            total += t;
        }
        if (i < n) {
            u.weights[i] = w;
            u.prefix[i] = carry + before + v;
        }
        carry += total;
    }
    for (int off = 32; off; off >>= 1)
        support += __shfl_xor(support, off);
    if (lane == 0)
        support_sh[wave] = support;
    __syncthreads();
    if (tid == 0) {
        uint32_t sup = 0;
        for (int w = 0; w < kWaves; ++w)
            sup += support_sh[w];
        csm_pose_update_info out;
        out.m0 = carry;
        out.key_max = found ? key_max : 0ull;
        out.best_index = found ? (int32_t)(0x3FFFF - (int)(best & 0x3FFFFull)) : -1;
        out.support = (int32_t)sup;
        out.bin_shift = u.bin_shift;
        out.found = found ? 1 : 0;
        *u.info = out;
    }
}

__global__ __launch_bounds__(kPoseBlock) void k_pose_resample(PoseUpdate u)
{
    const int j = blockIdx.x * kPoseBlock + threadIdx.x;
    if (j >= u.n_out)
        return;
    const unsigned long long m0 = u.info->m0;
    if (!u.info->found || m0 == 0ull) {
        u.ancestors[j] = -1;
        return;
    }
    /* j m0 + offset mod m0 < 2^18 2^42 + 2^42: no overflow; T < m0 = prefix[n_poses - 1] */
    const unsigned long long T = ((unsigned long long)j * m0 + u.offset % m0) / (unsigned long long)u.n_out;
    int lo = 0, hi = u.n_poses - 1;          /* the smallest i with prefix[i] > T */
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (u.prefix[mid] > T)
            hi = mid;
        else
            lo = mid + 1;
    }
    u.ancestors[j] = lo;
}

} /* namespace csm */
