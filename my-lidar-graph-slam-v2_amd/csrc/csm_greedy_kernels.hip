/* csm_greedy_kernels.hip -- device side of the greedy-endpoint cost and the hill-climbing matcher
 * (CostGreedyEndpoint, src/my_lidar_graph_slam/mapping/cost_function_greedy_endpoint.cpp;
 * ScanMatcherHillClimbing::OptimizePose, src/my_lidar_graph_slam/mapping/scan_matcher_hill_climbing.cpp:72-180).
 * Included by csm_greedy_api.hip (its own translation unit); the certificate's margin comes from
 * csm_certify.hpp, wave_sum from csm_score_common.hpp. gfx950 only.
 *
 * One workgroup per query runs the whole OptimizePose loop. An evaluation of up to six poses projects
 * every beam once per pose (lanes over beams, the six moves side by side in registers; the four x / y
 * moves share the trig of the current angle) and keeps each beam's result as a RANK: an index into the
 * ascending table of the distinct values of { LUT_cost, default }. A pose's cost is the literal
 * beam-order double sum of vals[rank], times ScalingFactor. Decisions (`localCost < minLocalCost`) are
 * taken from a wave-reduced sum with an error bound when the two intervals are apart, otherwise from the
 * literal sums, replayed one lane per pose from the ranks kept in LDS. */
#ifndef CSM_GREEDY_KERNELS_HIP
#define CSM_GREEDY_KERNELS_HIP

#include "csm_score_common.hpp"

namespace csm {

constexpr int kGreedyBlock = 256;
constexpr int kGreedyMaxVals = 64;            /* distinct cost values: <= 45 + 1 for KernelSize 8 */
constexpr int kGreedyMaxOff = 17 * 17;        /* (2 KernelSize + 1)^2 */
constexpr int kGreedySlots = 7;               /* the best pose + six candidates */
constexpr int kGreedyLdsBeams = 4096;         /* longer scans keep their ranks in global scratch */

/* the cost tables and search parameters of one call, built on the host (glibc exp) */
struct GreedyTab {
    double  vals[kGreedyMaxVals];     /* ascending distinct values of { LUT_cost, default } */
    double  hit_missed_dist, scaling, linear_step, angular_step;
    int32_t k, n_vals, default_rank;
    int32_t vh_lo;                    /* hit cell passes iff v >= vh_lo (>= 1: LUT[v] >= OccupancyThreshold) */
    int32_t vm_hi;                    /* missed cell passes iff 1 <= v <= vm_hi (LUT[v] <= OccupancyThreshold) */
    int32_t max_iterations, max_refinements, literal;
    uint8_t off_rank[kGreedyMaxOff + 3];   /* rank of LUT_cost[(k + ky) (2k + 1) + k + kx] */
};

struct GreedyJob {
    const uint16_t* cells;            /* level 0, pitched */
    const double*   angles;
    const double*   ranges;
    uint8_t*        scratch;          /* kGreedySlots * stride bytes when n > kGreedyLdsBeams */
    int32_t rows, cols, pitch, n;
    int32_t mode;                     /* 0: OptimizePose + covariance; 1: cost + covariance at `start` */
    int32_t stride;                   /* rank slot stride in scratch */
    double  res, off_x, off_y;
    double  start[3];                 /* sensor pose */
};

struct GreedyOut {
    double  initial_cost, cost;       /* Cost(), ScalingFactor applied */
    double  best[3];
    double  cov[9];
    int32_t iterations, refinements, replays, uncertain;
    int64_t evals;
};

/* floor((h - off) / res) as PositionToIndex computes it, and whether the host's glibc sin / cos could
 * give another integer: the margin of `certified` (csm_certify.hpp). Its own: a quotient no int holds is
 * never certified, and the index comes back. */
__device__ __forceinline__ bool greedy_index(double r, double h, double off, double res, int& idx)
{
    const double q = (h - off) / res;
    if (!(fabs(q) < 1.0e9)) {
        idx = 0;
        return false;
    }
    const double m = direct_margin(r, h, off, res, q);
    const double fq = floor(q);
    const double frac = q - fq;
    idx = (int)fq;
    return off_cell_edge(frac, m);
}

__device__ __forceinline__ uint32_t greedy_cell(const GreedyJob& j, int row, int col)
{
    return ((unsigned)row < (unsigned)j.rows && (unsigned)col < (unsigned)j.cols)
               ? (uint32_t)j.cells[(size_t)row * j.pitch + col] : 0u;
}

/* the beam's min over the surviving kernel offsets, as a rank (cost_function_greedy_endpoint.cpp:57-87) */
__device__ __forceinline__ int greedy_beam_rank(const GreedyJob& j, int hc, int hr, int mc, int mr, int k,
                                                uint32_t vh_lo, uint32_t vm_hi, const uint8_t* off_rank, int def)
{
    int best = def;
    int t = 0;
    for (int ky = -k; ky <= k; ++ky) {
        for (int kx = -k; kx <= k; ++kx, ++t) {
            const uint32_t vh = greedy_cell(j, hr + ky, hc + kx);
            if (vh < vh_lo)
                continue;
            const uint32_t vm = greedy_cell(j, mr + ky, mc + kx);
            if (vm == 0u || vm > vm_hi)
                continue;
            best = min(best, (int)off_rank[t]);
        }
    }
    return best;
}

struct GreedyIv {
    double lo, hi;
};

/* strict `a < b` of the scaled costs: 1 yes, 0 no, -1 undecided */
__device__ __forceinline__ int greedy_less(GreedyIv a, GreedyIv b)
{
    if (a.hi < b.lo)
        return 1;
    if (a.lo >= b.hi)
        return 0;
    return -1;
}

__global__ __launch_bounds__(kGreedyBlock) void k_greedy(const GreedyTab* __restrict__ tab,
                                                         const GreedyJob* __restrict__ jobs,
                                                         GreedyOut* __restrict__ outs)
{
    __shared__ double  s_vals[kGreedyMaxVals];
    __shared__ uint8_t s_off[kGreedyMaxOff + 3];
    __shared__ uint8_t s_rank[kGreedySlots * kGreedyLdsBeams];
    __shared__ double  s_cpose[6][3];           /* candidate poses of the evaluation */
    __shared__ int     s_phys[6];               /* their rank slots */
    __shared__ double  s_red[kGreedyBlock / 64][12];
    __shared__ double  s_A[6], s_M[6];          /* reduced sum / sum of |v| per candidate */
    __shared__ double  s_lit[kGreedySlots];     /* literal sums per slot */
    __shared__ int     s_want;                  /* slots to replay (bit mask) */
    __shared__ int     s_unc;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const GreedyJob job = jobs[blockIdx.x];
    const int n = job.n, k = tab->k, def = tab->default_rank;
    const uint32_t vh_lo = (uint32_t)tab->vh_lo, vm_hi = (uint32_t)tab->vm_hi;
    const double hmd = tab->hit_missed_dist, scaling = tab->scaling;
    for (int i = tid; i < kGreedyMaxVals; i += kGreedyBlock)
        s_vals[i] = tab->vals[i];
    for (int i = tid; i < kGreedyMaxOff + 3; i += kGreedyBlock)
        s_off[i] = tab->off_rank[i];
    uint8_t* const ranks = n <= kGreedyLdsBeams ? s_rank : job.scratch;
    const int stride = n <= kGreedyLdsBeams ? kGreedyLdsBeams : job.stride;
    if (tid == 0) {
        s_unc = 0;
        for (int p = 0; p < 3; ++p)
            s_cpose[0][p] = job.start[p];
        s_phys[0] = 0;
    }
    __syncthreads();

    /* Cost() of candidates 0..np-1 (np = 1 or 6): ranks into their slots, s_A / s_M. Candidates 0..3
     * share the angle of candidate 0 (theta + 0.0 * step, bit for bit up to the sign of a zero, which
     * changes no index); 4 and 5 have their own. */
    auto evaluate = [&](int np) {
        double sum[6], asum[6];
#pragma unroll
        for (int p = 0; p < 6; ++p)
            sum[p] = asum[p] = 0.0;
        double px[6], py[6];
        int slot[6];
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            px[p] = s_cpose[p][0];
            py[p] = s_cpose[p][1];
            slot[p] = s_phys[p];
        }
        const double t0 = s_cpose[0][2], t4 = s_cpose[4][2], t5 = s_cpose[5][2];
        bool unc = false;
        for (int i = tid; i < n; i += kGreedyBlock) {
            const double a = job.angles[i], r = job.ranges[i], rm = r - hmd;
            double c[3], s[3];
            sincos(t0 + a, &s[0], &c[0]);
            if (np > 1) {
                sincos(t4 + a, &s[1], &c[1]);
                sincos(t5 + a, &s[2], &c[2]);
            } else {
                c[1] = c[2] = c[0];
                s[1] = s[2] = s[0];
            }
#pragma unroll
            for (int p = 0; p < 6; ++p) {
                if (p < np) {
                    const int g = p < 4 ? 0 : p - 3;
                    const double cs = c[g], sn = s[g];
                    /* ScanData::HitAndMissedPoint (sensor_data.hpp:252-273) + PositionToIndex */
                    const double hx = px[p] + r * cs, hy = py[p] + r * sn;
                    const double mx = px[p] + rm * cs, my = py[p] + rm * sn;
                    int hc, hr, mc, mr;
                    bool ok = greedy_index(r, hx, job.off_x, job.res, hc);
                    ok &= greedy_index(r, hy, job.off_y, job.res, hr);
                    ok &= greedy_index(rm, mx, job.off_x, job.res, mc);
                    ok &= greedy_index(rm, my, job.off_y, job.res, mr);
                    unc |= !ok;
                    const int rk = ok ? greedy_beam_rank(job, hc, hr, mc, mr, k, vh_lo, vm_hi, s_off, def) : def;
                    ranks[(size_t)slot[p] * stride + i] = (uint8_t)rk;
                    const double v = s_vals[rk];
                    sum[p] += v;
                    asum[p] += fabs(v);
                }
            }
        }
        if (unc)
            atomicOr(&s_unc, 1);
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            if (p < np) {
                const double a = wave_sum(sum[p]), m = wave_sum(asum[p]);
                if (lane == 0) {
                    s_red[wave][2 * p] = a;
                    s_red[wave][2 * p + 1] = m;
                }
            }
        }
        __syncthreads();
        if (tid < np) {
            double a = 0.0, m = 0.0;
            for (int w = 0; w < kGreedyBlock / 64; ++w) {
                a += s_red[w][2 * tid];
                m += s_red[w][2 * tid + 1];
            }
            s_A[tid] = a;
            s_M[tid] = m;
        }
        __syncthreads();
    };
    /* literal beam-order sums of the slots in s_want, one lane per slot (Cost(): sumCostValue) */
    auto replay = [&]() {
        if (tid < kGreedySlots && (s_want >> tid & 1)) {
            const uint8_t* rk = ranks + (size_t)tid * stride;
            double acc = 0.0;
            for (int i = 0; i < n; ++i)
                acc += s_vals[rk[i]];
            s_lit[tid] = acc;
        }
        __syncthreads();
    };
    /* the scaled cost of candidate p as an interval: the literal sum lies within 2 (n-1) u M of the
     * wave-reduced one (both orders' error bounds), then one rounding by ScalingFactor */
    auto cand_iv = [&](int p) {
        const double e = 2.05 * (double)n * 1.12e-16 * s_M[p] + 1e-300;
        const double x1 = (s_A[p] - e) * scaling, x2 = (s_A[p] + e) * scaling;
        const double pad = 4.5e-16 * fmax(fabs(x1), fabs(x2)) + 1e-300;
        return GreedyIv { fmin(x1, x2) - pad, fmax(x1, x2) + pad };
    };

    /* Cost at the start pose (scan_matcher_hill_climbing.cpp:97-99) */
    evaluate(1);
    const bool literal = tab->literal != 0;
    int best = 0, iterations = 0, refinements = 0, replays = 0;
    int64_t evals = 1;
    double bx = job.start[0], by = job.start[1], bt = job.start[2];
    double initial_cost = 0.0, min_cost = 0.0;
    GreedyIv min_iv { 0.0, 0.0 };
    bool min_exact = true;
    if (tid == 0)
        s_want = 1;
    __syncthreads();
    replay();
    initial_cost = min_cost = s_lit[0] * scaling;
    min_iv = GreedyIv { min_cost, min_cost };
    bool unc = s_unc != 0;

    if (job.mode == 0 && !unc) {
        double lin = tab->linear_step, ang = tab->angular_step;
        const int max_it = tab->max_iterations, max_ref = tab->max_refinements;
        for (;;) {
            /* scan_matcher_hill_climbing.cpp:123-151: six moves from the current best pose */
            if (tid < 6) {
                /* moveX / moveY / moveTheta = { 1, -1, 0, 0, 0, 0 }, { 0, 0, 1, -1, 0, 0 }, { 0, 0, 0, 0, 1, -1 } */
                const double mx = tid == 0 ? 1.0 : tid == 1 ? -1.0 : 0.0;
                const double my = tid == 2 ? 1.0 : tid == 3 ? -1.0 : 0.0;
                const double mt = tid == 4 ? 1.0 : tid == 5 ? -1.0 : 0.0;
                s_cpose[tid][0] = bx + mx * lin;
                s_cpose[tid][1] = by + my * lin;
                s_cpose[tid][2] = bt + mt * ang;
                s_phys[tid] = tid < best ? tid : tid + 1;
            }
            __syncthreads();
            evaluate(6);
            evals += 6;
            if (s_unc) {
                unc = true;
                break;
            }
            /* every thread takes the same decisions from the same LDS values (uniform control flow) */
            int winner = -1;
            bool need = literal;
            GreedyIv local = min_iv;
            if (!need) {
                for (int p = 0; p < 6; ++p) {
                    const GreedyIv c = cand_iv(p);
                    const int lt = greedy_less(c, local);
                    if (lt < 0) {
                        need = true;
                        break;
                    }
                    if (lt) {
                        local = c;
                        winner = p;
                    }
                }
            }
            if (need) {
                ++replays;
                if (tid == 0) {
                    int w = 0;
                    for (int p = 0; p < 6; ++p)
                        w |= 1 << (p < best ? p : p + 1);
                    if (!min_exact)
                        w |= 1 << best;
                    s_want = w;
                }
                __syncthreads();
                replay();
                if (!min_exact) {
                    min_cost = s_lit[best] * scaling;
                    min_iv = GreedyIv { min_cost, min_cost };
                    min_exact = true;
                }
                local = min_iv;
                winner = -1;
                for (int p = 0; p < 6; ++p) {
                    const double c = s_lit[p < best ? p : p + 1] * scaling;
                    if (c < local.lo) {
                        local = GreedyIv { c, c };
                        winner = p;
                    }
                }
            }
            if (winner >= 0) {
                bx = s_cpose[winner][0];
                by = s_cpose[winner][1];
                bt = s_cpose[winner][2];
                best = winner < best ? winner : winner + 1;
                min_iv = local;
                min_exact = min_iv.lo == min_iv.hi;
                min_cost = min_iv.lo;
            } else {
                ++refinements;
                lin *= 0.5;
                ang *= 0.5;
            }
            const bool cont = (winner >= 0 || refinements < max_ref) && (++iterations < max_it);
            __syncthreads();     /* s_cpose / s_lit are rewritten by the next pass */
            if (!cont)
                break;
        }
        if (!unc && !min_exact) {
            if (tid == 0)
                s_want = 1 << best;
            __syncthreads();
            replay();
            min_cost = s_lit[best] * scaling;
        }
    }

    /* ComputeCovariance at the best sensor pose (cost_function_greedy_endpoint.cpp:101-157) */
    double cov[9] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    if (!unc) {
        const double dl = job.res, da = 1e-2;
        if (tid < 6) {
            /* pose +- deltaX, +- deltaY, +- deltaTheta, component-wise (inc/pose.hpp:65-79) */
            const int p = tid;
            const double dx = p < 2 ? dl : 0.0, dy = p == 2 || p == 3 ? dl : 0.0, dt = p >= 4 ? da : 0.0;
            const bool plus = (p & 1) == 0;
            s_cpose[p][0] = plus ? bx + dx : bx - dx;
            s_cpose[p][1] = plus ? by + dy : by - dy;
            s_cpose[p][2] = plus ? bt + dt : bt - dt;
            s_phys[p] = p < best ? p : p + 1;
        }
        __syncthreads();
        evaluate(6);
        evals += 6;
        unc = s_unc != 0;
        if (!unc) {
            if (tid == 0) {
                int w = 0;
                for (int p = 0; p < 6; ++p)
                    w |= 1 << (p < best ? p : p + 1);
                s_want = w;
            }
            __syncthreads();
            replay();
            double c[6];
            for (int p = 0; p < 6; ++p)
                c[p] = s_lit[p < best ? p : p + 1] * scaling;
            const double g[3] = { 0.5 * (c[0] - c[1]) / dl, 0.5 * (c[2] - c[3]) / dl, 0.5 * (c[4] - c[5]) / da };
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j)
                    cov[3 * i + j] = g[i] * g[j];
            cov[0] += 0.1;
            cov[4] += 0.1;
            cov[8] += 0.1;
        }
    }
    if (tid == 0) {
        GreedyOut o;
        o.initial_cost = initial_cost;
        o.cost = job.mode == 0 ? min_cost : initial_cost;
        o.best[0] = bx;
        o.best[1] = by;
        o.best[2] = bt;
        for (int i = 0; i < 9; ++i)
            o.cov[i] = cov[i];
        o.iterations = iterations;
        o.refinements = refinements;
        o.replays = replays;
        o.uncertain = unc ? 1 : 0;
        o.evals = evals;
        outs[blockIdx.x] = o;
    }
}

} /* namespace csm */
#endif
