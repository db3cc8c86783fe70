/* csm_posegraph_kernels.hip -- PoseGraphOptimizerLM (src/my_lidar_graph_slam/mapping/pose_graph_optimizer_lm.cpp)
 * with the ConjugateGradient solver: the per-edge / per-block arithmetic that the host restatement and the
 * device share (__host__ __device__, glibc's sin / cos / fmod on the host, the device library's on the
 * device), and the kernel. Included by csm_posegraph_api.hip (its own translation unit). gfx950 only.
 *
 * H is kept as a block-CSR of 3x3 blocks holding both triangles: slot k < n_nodes is
 * the diagonal block of node k (all nine entries, mirrored from its lower triangle), slot n_nodes + u
 * the lower cross block of the u-th distinct (scan node, local map node) pair. Every stored value is
 * the sum of its setFromTriplets contributions in triplet order: [1e9] + lambda + edges in edge order
 * on a diagonal, edges in edge order elsewhere. A row of H walks its blocks in ascending column order;
 * the upper cross blocks are read transposed.
 *
 * One workgroup of kPgBlock threads runs every LM step of one Optimize call. Vectors live in global
 * memory (L2-resident); the dot products and the total error are reduced in a fixed shape (per-thread
 * strided sums, a wave butterfly, then the 8 wave partials in order on every thread), so the result
 * is deterministic. 512 threads: the kernel needs 196 VGPRs, which 1024 threads (128 each) would
 * spill. Every loop is bounded by NumOfIterationsMax, 2n or a host-built list length. */
#ifndef CSM_POSEGRAPH_KERNELS_HIP
#define CSM_POSEGRAPH_KERNELS_HIP

#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "csm_pg_math.hpp"

namespace csm {

constexpr int kPgBlock = 512;
constexpr int kPgWaves = kPgBlock / 64;
constexpr int kPgEdgeVals = 27;   /* A[6] = JsT L Js lower, B[6] = JeT L Je lower, C[9], bs[3], be[3] */

/* row entry flags (slot = entry >> 2) */
constexpr int kPgTransposed = 1;  /* an upper cross block: read the stored lower block transposed */
constexpr int kPgDiagOnly = 2;    /* diagonal block of a node without edges: only its diagonal exists */

struct PgJob {
    int n_local, n_nodes, n_vars, n_edges, n_cross;
    int iterations_max, loss_type, cg_max;
    double error_tolerance, loss_scale, lambda;
    double* pose;                 /* [n_vars]: local map nodes, then scan nodes */
    const double* rel;            /* [3 E] */
    const double* info;           /* [9 E] */
    const int32_t* enode;         /* [2 E]: start node, end node (node indices) */
    const int32_t* is_loop;       /* [E] */
    const int32_t* node_ptr;      /* [n_nodes + 1] into node_edges: incident edges in edge order */
    const int32_t* node_edges;
    const int32_t* cross_ptr;     /* [n_cross + 1] into cross_edges: the pair's edges in edge order */
    const int32_t* cross_edges;
    const int32_t* row_ptr;       /* [n_nodes + 1] into row_col / row_ent, ascending column node */
    const int32_t* row_col;
    const int32_t* row_ent;       /* slot << 2 | flags */
    double* ev;                   /* [kPgEdgeVals E] */
    double* bv;                   /* [9 (n_nodes + n_cross)] */
    double *b, *invd, *x, *r, *z, *p, *ap;   /* [n_vars] each */
    double* out;                  /* [4 + 5 iterations_max]: steps, initial, final, lambda; per step
                                     total, lambda, |b|^2, |r|^2, cg iterations */
};

/* ------------------------------------------------------------------ shared arithmetic */

/* pg_normalize_angle, pg_ldl3 and pg_ldl3_solve are in csm_pg_math.hpp */

/* LossFunction::Loss / Weight (src/mapping/robust_loss_function.cpp, inc/.../robust_loss_function.hpp) */
__host__ __device__ inline double pg_loss(int type, double s, double t)
{
    switch (type) {
    case 1: return (t <= s) ? t : (2.0 * sqrt(s * t) - s);
    case 2: return s * log1p(t / s);
    case 3: { const double q = sqrt(t / s); return 2.0 * s * (q - log1p(q)); }
    case 4: return s * t / (s + t);
    case 5: return s * (-expm1(-t / s));
    default: return t;
    }
}

__host__ __device__ inline double pg_weight(int type, double s, double t)
{
    switch (type) {
    case 1: return (t <= s) ? 1.0 : sqrt(s / t);
    case 2: return s / (s + t);
    case 3: { const double q = sqrt(t / s); return 1.0 / (1.0 + q); }
    case 4: { const double ss = s * s; const double st = s + t; return ss / (st * st); }
    case 5: return exp(-t / s);
    default: return 1.0;
    }
}

/* e = h(c_i, c_j) - z (ComputeErrorAndJacobians :381-415 and ComputeErrorFunction / InverseCompound
 * :362-378, pose_eigen.hpp:29-42: the same expressions); returns cos, sin and the relative x, y */
__host__ __device__ inline void pg_error(const double* ps, const double* pe, const double* z, double e[3],
                                         double& c, double& s, double& x, double& y)
{
    s = sin(ps[2]);
    c = cos(ps[2]);
    const double d0 = pe[0] - ps[0], d1 = pe[1] - ps[1], d2 = pe[2] - ps[2];
    x = c * d0 + s * d1;
    y = -s * d0 + c * d1;
    e[0] = x - z[0];
    e[1] = y - z[1];
    e[2] = pg_normalize_angle(d2 - z[2]);
}

/* e^T Lambda e as (e^T Lambda) e, every three-term sum left to right */
__host__ __device__ inline double pg_quad(const double e[3], const double* L)
{
    double u[3];
    for (int j = 0; j < 3; ++j)
        u[j] = e[0] * L[j] + e[1] * L[3 + j] + e[2] * L[6 + j];
    return u[0] * e[0] + u[1] * e[1] + u[2] * e[2];
}

/* ComputeTotalError's term of one edge (:418-452) */
__host__ __device__ inline double pg_edge_loss(const double* ps, const double* pe, const double* z, const double* L,
                                               int loss, double scale)
{
    double e[3], c, s, x, y;
    pg_error(ps, pe, z, e, c, s, x, y);
    return pg_loss(loss, scale, pg_quad(e, L));
}

/* OptimizeStep's per-edge work (:150-232): the triplet values of the edge and its two b terms */
__host__ __device__ inline void pg_edge_values(const double* ps, const double* pe, const double* z, const double* L,
                                               int is_loop, int loss, double scale, double* v)
{
    double e[3], c, s, x, y;
    pg_error(ps, pe, z, e, c, s, x, y);
    const double Js[9] = { -c, -s, y, s, -c, -x, 0.0, 0.0, -1.0 };
    const double Je[9] = { c, s, 0.0, -s, c, 0.0, 0.0, 0.0, 1.0 };
    const double w = is_loop ? pg_weight(loss, scale, pg_quad(e, L)) : 1.0;
    double Ts[9], Te[9];     /* Js^T Lambda w, Je^T Lambda w */
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            Ts[3 * i + j] = (Js[i] * L[j] + Js[3 + i] * L[3 + j] + Js[6 + i] * L[6 + j]) * w;
            Te[3 * i + j] = (Je[i] * L[j] + Je[3 + i] * L[3 + j] + Je[6 + i] * L[6 + j]) * w;
        }
    auto prod = [](const double* T, const double* J, int i, int j) {
        return T[3 * i] * J[j] + T[3 * i + 1] * J[3 + j] + T[3 * i + 2] * J[6 + j];
    };
    int k = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j <= i; ++j, ++k) {
            v[k] = prod(Ts, Js, i, j);
            v[6 + k] = prod(Te, Je, i, j);
        }
    /* C(i, j) = H(end + i, start + j) = (Js^T Lambda Je)(j, i) */
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            v[12 + 3 * i + j] = prod(Ts, Je, j, i);
    for (int i = 0; i < 3; ++i) {
        v[21 + i] = Ts[3 * i] * e[0] + Ts[3 * i + 1] * e[1] + Ts[3 * i + 2] * e[2];
        v[24 + i] = Te[3 * i] * e[0] + Te[3 * i + 1] * e[1] + Te[3 * i + 2] * e[2];
    }
}

/* edge e of a job: its two node poses, its measurement and its information matrix. Every site that walks the
 * edges goes through these two, but for step 1 of k_pose_graph_lm (see there). */
__host__ __device__ inline double pg_edge_loss_at(const PgJob& J, int e)
{
    return pg_edge_loss(J.pose + 3 * (size_t)J.enode[2 * e], J.pose + 3 * (size_t)J.enode[2 * e + 1],
                        J.rel + 3 * (size_t)e, J.info + 9 * (size_t)e, J.loss_type, J.loss_scale);
}

__host__ __device__ inline void pg_edge_values_at(const PgJob& J, int e)
{
    pg_edge_values(J.pose + 3 * (size_t)J.enode[2 * e], J.pose + 3 * (size_t)J.enode[2 * e + 1],
                   J.rel + 3 * (size_t)e, J.info + 9 * (size_t)e, J.is_loop[e], J.loss_type, J.loss_scale,
                   J.ev + (size_t)kPgEdgeVals * e);
}

/* lower-triangle index (i >= j) of a 3x3 block in the per-edge value order (0,0) (1,0) (1,1) (2,0) ... */
__host__ __device__ inline int pg_tri(int i, int j) { return i * (i + 1) / 2 + j; }

/* diagonal block of node k: its nine H entries, the three b entries and the Jacobi inverse diagonal */
__host__ __device__ inline void pg_assemble_node(const PgJob& J, int k, double lambda)
{
    const int e0 = J.node_ptr[k], e1 = J.node_ptr[k + 1];
    const int off = k < J.n_local ? 0 : 6;          /* start nodes take A, end nodes B */
    const int boff = k < J.n_local ? 21 : 24;
    double* blk = J.bv + 9 * (size_t)k;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j <= i; ++j) {
            double h;
            int t = e0;
            if (i == j) {
                h = (k == 0) ? 1e9 : lambda;
                if (k == 0)
                    h += lambda;
            } else {
                h = (e0 < e1) ? J.ev[(size_t)kPgEdgeVals * J.node_edges[t++] + off + pg_tri(i, j)] : 0.0;
            }
            for (; t < e1; ++t)
                h += J.ev[(size_t)kPgEdgeVals * J.node_edges[t] + off + pg_tri(i, j)];
            blk[3 * i + j] = h;
            blk[3 * j + i] = h;
        }
    }
    for (int a = 0; a < 3; ++a) {
        double bb = 0.0;
        for (int t = e0; t < e1; ++t)
            bb -= J.ev[(size_t)kPgEdgeVals * J.node_edges[t] + boff + a];
        J.b[3 * k + a] = bb;
        const double d = blk[4 * a];
        J.invd[3 * k + a] = (d != 0.0) ? 1.0 / d : 1.0;   /* DiagonalPreconditioner::factorize */
    }
}

/* lower cross block u: the sum of its edges' C blocks in edge order */
__host__ __device__ inline void pg_assemble_cross(const PgJob& J, int u)
{
    const int e0 = J.cross_ptr[u], e1 = J.cross_ptr[u + 1];
    double* blk = J.bv + 9 * ((size_t)J.n_nodes + u);
    for (int q = 0; q < 9; ++q) {
        double h = J.ev[(size_t)kPgEdgeVals * J.cross_edges[e0] + 12 + q];
        for (int t = e0 + 1; t < e1; ++t)
            h += J.ev[(size_t)kPgEdgeVals * J.cross_edges[t] + 12 + q];
        blk[q] = h;
    }
}

/* (H v)_row, the row's stored entries in ascending column order, summed left to right from 0 */
__host__ __device__ inline double pg_row_times(const PgJob& J, int row, const double* v)
{
    const int node = row / 3, a = row - 3 * node;
    double s = 0.0;
    for (int t = J.row_ptr[node]; t < J.row_ptr[node + 1]; ++t) {
        const int ent = J.row_ent[t];
        const double* blk = J.bv + 9 * (size_t)(ent >> 2);
        const double* vc = v + 3 * (size_t)J.row_col[t];
        if (ent & kPgDiagOnly) {
            s += blk[4 * a] * vc[a];
        } else if (ent & kPgTransposed) {
            for (int c = 0; c < 3; ++c)
                s += blk[3 * c + a] * vc[c];
        } else {
            for (int c = 0; c < 3; ++c)
                s += blk[3 * a + c] * vc[c];
        }
    }
    return s;
}

/* ------------------------------------------------------------------ device */

/* sum of N values per thread over a workgroup of Waves waves (8 in k_pose_graph_lm, 4 in the k_pgs_*
 * kernels): wave butterfly (every lane ends with the same bits), the wave sums through LDS buffer `buf`,
 * added in wave order by every thread. One barrier; a caller that reduces again alternates two buffers,
 * which keeps a buffer's next writes behind the following reduction's barrier. */
template <int N, int Waves>
__device__ inline void pg_block_sum(double (&v)[N], double (*buf)[N])
{
    for (int m = 32; m >= 1; m >>= 1)
        for (int q = 0; q < N; ++q)
            v[q] += __shfl_xor(v[q], m, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int q = 0; q < N; ++q)
            buf[wave][q] = v[q];
    __syncthreads();
    for (int q = 0; q < N; ++q) {
        double s = buf[0][q];
        for (int w = 1; w < Waves; ++w)
            s += buf[w][q];
        v[q] = s;
    }
}

__device__ inline double pg_total_error(const PgJob& J, double (*buf)[1])
{
    double v[1] = { 0.0 };
    for (int e = threadIdx.x; e < J.n_edges; e += kPgBlock)
        v[0] += pg_edge_loss_at(J, e);
    pg_block_sum<1, kPgWaves>(v, buf);
    return v[0];
}

__global__ __launch_bounds__(kPgBlock) void k_pose_graph_lm(PgJob J)
{
    __shared__ double red1[2][kPgWaves][1];
    __shared__ double red2[2][kPgWaves][2];
    int flip = 0;
    auto sum1 = [&](double x) {
        double v[1] = { x };
        pg_block_sum<1, kPgWaves>(v, red1[flip]);
        flip ^= 1;
        return v[0];
    };
    const int tid = threadIdx.x, n = J.n_vars;
    double lambda = J.lambda;
    double prev = DBL_MAX, total = DBL_MAX;
    const double initial = pg_total_error(J, red1[flip]);
    flip ^= 1;
    int steps = 0;
    for (int it = 0; it < J.iterations_max; ++it) {
        /* 1. per-edge error, Jacobians, weight and blocks */
        /* spelled out, not pg_edge_values_at: through the helper the compiler emits this loop two
         * instructions longer, and the kernel measured 0.7 % slower at 1000 scan nodes */
        for (int e = tid; e < J.n_edges; e += kPgBlock)
            pg_edge_values(J.pose + 3 * (size_t)J.enode[2 * e], J.pose + 3 * (size_t)J.enode[2 * e + 1],
                           J.rel + 3 * (size_t)e, J.info + 9 * (size_t)e, J.is_loop[e], J.loss_type, J.loss_scale,
                           J.ev + (size_t)kPgEdgeVals * e);
        __syncthreads();
        /* 2. assembly in triplet order, b, the preconditioner */
        for (int k = tid; k < J.n_nodes; k += kPgBlock)
            pg_assemble_node(J, k, lambda);
        for (int u = tid; u < J.n_cross; u += kPgBlock)
            pg_assemble_cross(J, u);
        __syncthreads();
        /* 3. conjugate_gradient (Eigen/src/IterativeLinearSolvers/ConjugateGradient.h), x0 = 0 */
        double part = 0.0;
        for (int i = tid; i < n; i += kPgBlock) {
            const double bi = J.b[i];
            J.x[i] = 0.0;
            J.r[i] = bi;
            part += bi * bi;
        }
        const double rhs2 = sum1(part);
        double r2 = rhs2;
        int cg = 0;
        if (rhs2 != 0.0) {
            const double a = DBL_EPSILON * DBL_EPSILON * rhs2;
            const double thr = (a < DBL_MIN) ? DBL_MIN : a;      /* numext::maxi */
            if (!(r2 < thr)) {
                part = 0.0;
                for (int i = tid; i < n; i += kPgBlock) {
                    const double pi = J.invd[i] * J.r[i];
                    J.p[i] = pi;
                    part += J.r[i] * pi;
                }
                double abs_new = sum1(part);
                __syncthreads();
                for (; cg < J.cg_max; ++cg) {
                    part = 0.0;
                    for (int i = tid; i < n; i += kPgBlock) {
                        const double t = pg_row_times(J, i, J.p);
                        J.ap[i] = t;
                        part += J.p[i] * t;
                    }
                    const double alpha = abs_new / sum1(part);
                    double v[2] = { 0.0, 0.0 };
                    for (int i = tid; i < n; i += kPgBlock) {
                        J.x[i] += alpha * J.p[i];
                        const double ri = J.r[i] - alpha * J.ap[i];
                        J.r[i] = ri;
                        const double zi = J.invd[i] * ri;
                        J.z[i] = zi;
                        v[0] += ri * ri;
                        v[1] += ri * zi;
                    }
                    pg_block_sum<2, kPgWaves>(v, red2[flip]);
                    flip ^= 1;
                    r2 = v[0];
                    if (r2 < thr)
                        break;
                    const double abs_old = abs_new;
                    abs_new = v[1];
                    const double beta = abs_new / abs_old;
                    for (int i = tid; i < n; i += kPgBlock)
                        J.p[i] = J.z[i] + beta * J.p[i];
                    __syncthreads();
                }
            }
        } else {
            r2 = 0.0;
        }
        /* 4. node += delta, the total error, the LM decision */
        for (int i = tid; i < n; i += kPgBlock)
            J.pose[i] += J.x[i];
        __syncthreads();
        total = pg_total_error(J, red1[flip]);
        flip ^= 1;
        steps = it + 1;
        if (tid == 0) {
            double* o = J.out + 4 + 5 * (size_t)it;
            o[0] = total;
            o[1] = lambda;
            o[2] = rhs2;
            o[3] = r2;
            o[4] = (double)cg;
        }
        if (steps >= J.iterations_max || fabs(prev - total) < J.error_tolerance)
            break;
        lambda = (total < prev) ? lambda * 0.5 : lambda * 2.0;
        prev = total;
    }
    if (tid == 0) {
        J.out[0] = (double)steps;
        J.out[1] = initial;
        J.out[2] = total;
        J.out[3] = lambda;
    }
}

/* ================================================================== Schur-complement Cholesky solver
 * CSM_PG_SOLVER_SCHUR_CHOLESKY: every edge joins a local map node to a scan node, so
 * D (the scan nodes' diagonal blocks) is block diagonal. Per LM step: D_t = L D L^T (3x3, unpivoted),
 * g_t = D_t^-1 b_t and W_ts = D_t^-1 B_ts per scan node; S = A - B^T W and c = b_local - B^T g from
 * host-built ordered lists; a dense unpivoted scalar LDL^T of S (lower triangle, row-major, each
 * entry's inner product over k ascending); substitutions; x_t = g_t - sum_s W_ts x_s. The per-entry
 * arithmetic below is shared by the host restatement and the kernels; the device's blocked
 * factorization subtracts every entry's terms in the same ascending k order, one after the other. */

constexpr int kPgsTile = 48;      /* panel width = tile edge of the blocked LDL^T: a multiple of 3 */
constexpr int kPgsSmall = 96;     /* 3 n_local up to here: S lives in the LDS of one workgroup */
constexpr int kPgsBlock = 256;    /* threads of the grid-wide kernels and of the reductions */
constexpr int kPgsWaves = kPgsBlock / 64;
constexpr int kPgsSolveBlock = 1024;

/* what the LM loop carries from step to step on the device */
struct PgState {
    double lambda, prev, total, initial;
    int32_t steps, done;
};

struct PgSchurJob {
    PgJob J;                      /* J.x is delta; J.r, J.z, J.p, J.ap are unused */
    int n_s, np;                  /* 3 n_local; n_s rounded up to whole tiles (= the row stride of S) */
    int n_sblk;                   /* stored 3x3 blocks of S: the n_local diagonal ones, then the others */
    int nb_vars, nb_edges;        /* workgroups (= partial sums) of k_pgs_update / k_pgs_error */
    const int32_t* sb_rc;         /* [2 n_sblk]: s1 >= s2 */
    const int32_t* sb_ptr;        /* [n_sblk + 1] into sb_pair */
    const int32_t* sb_pair;       /* cross blocks (t, s1), (t, s2) of every common scan node t, ascending t */
    double* g;                    /* [3 n_scan] */
    double* w;                    /* [9 n_cross] */
    double* S;                    /* [np * np] (blocked path) */
    double* wp;                   /* [np * kPgsTile]: (L d) of the current panel */
    double* y;                    /* [np]: c, then the substitutions in place */
    double* part;                 /* [2 nb_vars + nb_edges]: |r|^2, |b|^2, total-error partial sums */
    PgState* st;
};

/* step 1 for scan node t (a node index >= n_local): g_t and W of each of its cross blocks */
__host__ __device__ inline void pg_eliminate_scan(const PgJob& J, double* g, double* w, int t)
{
    double f[6];
    pg_ldl3(J.bv + 9 * (size_t)t, f);
    const double* bt = J.b + 3 * (size_t)t;
    pg_ldl3_solve(f, bt[0], bt[1], bt[2], g + 3 * (size_t)(t - J.n_local));
    for (int q = J.row_ptr[t]; q < J.row_ptr[t + 1]; ++q) {
        if (J.row_col[q] == t)
            continue;
        const int slot = J.row_ent[q] >> 2;
        const double* B = J.bv + 9 * (size_t)slot;
        double* W = w + 9 * (size_t)(slot - J.n_nodes);
        for (int j = 0; j < 3; ++j) {
            double x[3];
            pg_ldl3_solve(f, B[j], B[3 + j], B[6 + j], x);
            W[j] = x[0];
            W[3 + j] = x[1];
            W[6 + j] = x[2];
        }
    }
}

/* step 2: entry (i, j) of stored S block q */
__host__ __device__ inline double pg_schur_entry(const PgJob& J, const int32_t* sb_rc, const int32_t* sb_ptr,
                                                 const int32_t* sb_pair, const double* w, int q, int i, int j)
{
    const int s1 = sb_rc[2 * q], s2 = sb_rc[2 * q + 1];
    double acc = (s1 == s2) ? J.bv[9 * (size_t)s1 + 3 * i + j] : 0.0;
    for (int m = sb_ptr[q]; m < sb_ptr[q + 1]; ++m) {
        const double* B = J.bv + 9 * ((size_t)J.n_nodes + sb_pair[2 * m]);
        const double* W = w + 9 * (size_t)sb_pair[2 * m + 1];
        acc -= B[i] * W[j] + B[3 + i] * W[3 + j] + B[6 + i] * W[6 + j];
    }
    return acc;
}

/* step 2: entry a of the reduced right-hand side of local map node s */
__host__ __device__ inline double pg_schur_rhs(const PgJob& J, const double* g, int s, int a)
{
    double acc = J.b[3 * (size_t)s + a];
    for (int q = J.row_ptr[s]; q < J.row_ptr[s + 1]; ++q) {
        if (!(J.row_ent[q] & kPgTransposed))
            continue;
        const double* B = J.bv + 9 * (size_t)(J.row_ent[q] >> 2);
        const double* gt = g + 3 * (size_t)(J.row_col[q] - J.n_local);
        acc -= B[a] * gt[0] + B[3 + a] * gt[1] + B[6 + a] * gt[2];
    }
    return acc;
}

/* step 4 for scan node t: its three entries of delta (x holds the local map nodes' already) */
__host__ __device__ inline void pg_back_scan(const PgJob& J, const double* g, const double* w, double* x, int t)
{
    double acc[3];
    for (int i = 0; i < 3; ++i)
        acc[i] = g[3 * (size_t)(t - J.n_local) + i];
    for (int q = J.row_ptr[t]; q < J.row_ptr[t + 1]; ++q) {
        if (J.row_col[q] == t)
            continue;
        const double* W = w + 9 * (size_t)((J.row_ent[q] >> 2) - J.n_nodes);
        const double* xs = x + 3 * (size_t)J.row_col[q];
        for (int i = 0; i < 3; ++i)
            acc[i] -= W[3 * i] * xs[0] + W[3 * i + 1] * xs[1] + W[3 * i + 2] * xs[2];
    }
    for (int i = 0; i < 3; ++i)
        x[3 * (size_t)t + i] = acc[i];
}

/* ------------------------------------------------------------------ device: the launch chain of one LM step.
 * Every kernel returns at once when the state's done flag is set; none waits on another workgroup. */

__global__ __launch_bounds__(kPgsBlock) void k_pgs_edges(PgSchurJob Q)
{
    const PgJob& J = Q.J;
    const int e = blockIdx.x * kPgsBlock + threadIdx.x;
    if (Q.st->done || e >= J.n_edges)
        return;
    pg_edge_values_at(J, e);
}

__global__ __launch_bounds__(kPgsBlock) void k_pgs_assemble(PgSchurJob Q)
{
    const PgJob& J = Q.J;
    const int k = blockIdx.x * kPgsBlock + threadIdx.x;
    if (Q.st->done)
        return;
    if (k < J.n_nodes)
        pg_assemble_node(J, k, Q.st->lambda);
    else if (k - J.n_nodes < J.n_cross)
        pg_assemble_cross(J, k - J.n_nodes);
}

__global__ __launch_bounds__(kPgsBlock) void k_pgs_eliminate(PgSchurJob Q)
{
    const int t = Q.J.n_local + blockIdx.x * kPgsBlock + threadIdx.x;
    if (Q.st->done || t >= Q.J.n_nodes)
        return;
    pg_eliminate_scan(Q.J, Q.g, Q.w, t);
}

/* S = 0 with a unit diagonal in the padding rows (they factor to L = 0, d = 1) */
__global__ __launch_bounds__(kPgsBlock) void k_pgs_clear(PgSchurJob Q)
{
    if (Q.st->done)
        return;
    const size_t total = (size_t)Q.np * Q.np;
    for (size_t i = (size_t)blockIdx.x * kPgsBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kPgsBlock) {
        const int r = (int)(i / Q.np), c = (int)(i - (size_t)r * Q.np);
        Q.S[i] = (r == c && r >= Q.n_s) ? 1.0 : 0.0;
    }
}

/* a thread per scalar of a stored S block, then a thread per entry of c */
__global__ __launch_bounds__(kPgsBlock) void k_pgs_schur(PgSchurJob Q)
{
    if (Q.st->done)
        return;
    const int id = blockIdx.x * kPgsBlock + threadIdx.x;
    if (id < 9 * Q.n_sblk) {
        const int q = id / 9, ij = id - 9 * q, i = ij / 3, j = ij - 3 * i;
        const size_t r = 3 * (size_t)Q.sb_rc[2 * q] + i, c = 3 * (size_t)Q.sb_rc[2 * q + 1] + j;
        Q.S[r * Q.np + c] = pg_schur_entry(Q.J, Q.sb_rc, Q.sb_ptr, Q.sb_pair, Q.w, q, i, j);
    } else if (id - 9 * Q.n_sblk < Q.np) {
        const int a = id - 9 * Q.n_sblk;
        Q.y[a] = (a < Q.n_s) ? pg_schur_rhs(Q.J, Q.g, a / 3, a % 3) : 0.0;
    }
}

/* blocked right-looking LDL^T, panel p: the diagonal tile by one workgroup in LDS */
__global__ __launch_bounds__(kPgsBlock) void k_pgs_ldl_diag(PgSchurJob Q, int p)
{
    __shared__ double A[kPgsTile][kPgsTile + 1];
    __shared__ double Lk[kPgsTile], Wk[kPgsTile];
    if (Q.st->done)
        return;
    const int tid = threadIdx.x;
    double* T = Q.S + ((size_t)p * kPgsTile) * Q.np + (size_t)p * kPgsTile;
    for (int q = tid; q < kPgsTile * kPgsTile; q += kPgsBlock)
        A[q / kPgsTile][q % kPgsTile] = T[(size_t)(q / kPgsTile) * Q.np + q % kPgsTile];
    for (int k = 0; k < kPgsTile; ++k) {
        __syncthreads();
        if (tid > k && tid < kPgsTile) {
            const double d = A[k][k], l = A[tid][k] / d;
            A[tid][k] = l;
            Lk[tid] = l;
            Wk[tid] = l * d;
        }
        __syncthreads();
        for (int q = tid; q < kPgsTile * kPgsTile; q += kPgsBlock) {
            const int i = q / kPgsTile, j = q % kPgsTile;
            if (j > k && j <= i)
                A[i][j] -= Wk[i] * Lk[j];
        }
    }
    __syncthreads();
    for (int q = tid; q < kPgsTile * kPgsTile; q += kPgsBlock)
        if (q % kPgsTile <= q / kPgsTile)
            T[(size_t)(q / kPgsTile) * Q.np + q % kPgsTile] = A[q / kPgsTile][q % kPgsTile];
}

/* panel p: a thread per row below the diagonal tile; its (L d) values stay in registers */
__global__ __launch_bounds__(64) void k_pgs_ldl_panel(PgSchurJob Q, int p)
{
    __shared__ double Ld[kPgsTile][kPgsTile];
    __shared__ double dd[kPgsTile];
    if (Q.st->done)
        return;
    const int j0 = p * kPgsTile;
    for (int q = threadIdx.x; q < kPgsTile * kPgsTile; q += 64)
        Ld[q / kPgsTile][q % kPgsTile] = Q.S[(size_t)(j0 + q / kPgsTile) * Q.np + j0 + q % kPgsTile];
    __syncthreads();
    if (threadIdx.x < kPgsTile)
        dd[threadIdx.x] = Ld[threadIdx.x][threadIdx.x];
    __syncthreads();
    const int r = j0 + kPgsTile + blockIdx.x * 64 + threadIdx.x;
    if (r >= Q.np)
        return;
    double* row = Q.S + (size_t)r * Q.np + j0;
    double* wrow = Q.wp + (size_t)r * kPgsTile;
    double w[kPgsTile];
#pragma unroll
    for (int j = 0; j < kPgsTile; ++j) {
        double v = row[j];
#pragma unroll
        for (int k = 0; k < j; ++k)
            v -= w[k] * Ld[j][k];
        const double l = v / dd[j];
        w[j] = l * dd[j];
        row[j] = l;
        wrow[j] = w[j];
    }
}

/* trailing update behind panel p: tile (ti, tj), ti >= tj > p, S_ij -= sum_k (L d)_ik L_jk with k
 * ascending, a 3x3 register tile per thread, both operand tiles staged k-major in LDS */
__global__ __launch_bounds__(kPgsBlock) void k_pgs_ldl_update(PgSchurJob Q, int p)
{
    __shared__ double Wt[kPgsTile][kPgsTile + 1];
    __shared__ double Lt[kPgsTile][kPgsTile + 1];
    if (Q.st->done || blockIdx.x > blockIdx.y)
        return;
    const int ti = p + 1 + blockIdx.y, tj = p + 1 + blockIdx.x;
    const int i0 = ti * kPgsTile, c0 = tj * kPgsTile, j0 = p * kPgsTile;
    for (int q = threadIdx.x; q < kPgsTile * kPgsTile; q += kPgsBlock) {
        const int r = q / kPgsTile, k = q % kPgsTile;
        Wt[k][r] = Q.wp[(size_t)(i0 + r) * kPgsTile + k];
        Lt[k][r] = Q.S[(size_t)(c0 + r) * Q.np + j0 + k];
    }
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    double acc[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b)
            acc[a][b] = Q.S[(size_t)(i0 + ty + 16 * a) * Q.np + c0 + tx + 16 * b];
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < kPgsTile; ++k) {
        double wv[3], lv[3];
        for (int a = 0; a < 3; ++a) {
            wv[a] = Wt[k][ty + 16 * a];
            lv[a] = Lt[k][tx + 16 * a];
        }
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b)
                acc[a][b] -= wv[a] * lv[b];
    }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b)
            Q.S[(size_t)(i0 + ty + 16 * a) * Q.np + c0 + tx + 16 * b] = acc[a][b];
}

/* forward, diagonal and backward substitution on the factored S by one workgroup: per panel the
 * diagonal tile on one wave (row i on lane i), then a thread per remaining row (forward) or
 * column (backward). Forward subtracts in ascending k, backward in descending k. */
__global__ __launch_bounds__(kPgsSolveBlock) void k_pgs_solve(PgSchurJob Q)
{
    __shared__ double blk[kPgsTile][kPgsTile + 1];
    __shared__ double pan[kPgsTile];
    if (Q.st->done)
        return;
    const int tid = threadIdx.x, nt = Q.np / kPgsTile, n = Q.n_s;
    double* y = Q.y;
    for (int p = 0; p < nt; ++p) {
        const int j0 = p * kPgsTile;
        for (int q = tid; q < kPgsTile * kPgsTile; q += kPgsSolveBlock)
            blk[q / kPgsTile][q % kPgsTile] = Q.S[(size_t)(j0 + q / kPgsTile) * Q.np + j0 + q % kPgsTile];
        __syncthreads();
        if (tid < 64) {
            double yi = (tid < kPgsTile) ? y[j0 + tid] : 0.0;
            for (int j = 0; j < kPgsTile; ++j) {
                const double yj = __shfl(yi, j, 64);
                if (tid > j && tid < kPgsTile)
                    yi -= blk[tid][j] * yj;
            }
            if (tid < kPgsTile) {
                pan[tid] = yi;
                y[j0 + tid] = yi;
            }
        }
        __syncthreads();
        for (int r = j0 + kPgsTile + tid; r < n; r += kPgsSolveBlock) {
            const double* row = Q.S + (size_t)r * Q.np + j0;
            double v = y[r];
            for (int k = 0; k < kPgsTile; ++k)
                v -= row[k] * pan[k];
            y[r] = v;
        }
        __syncthreads();
    }
    for (int i = tid; i < n; i += kPgsSolveBlock)
        y[i] = y[i] / Q.S[(size_t)i * Q.np + i];
    __syncthreads();
    for (int p = nt - 1; p >= 0; --p) {
        const int j0 = p * kPgsTile;
        for (int q = tid; q < kPgsTile * kPgsTile; q += kPgsSolveBlock)
            blk[q / kPgsTile][q % kPgsTile] = Q.S[(size_t)(j0 + q / kPgsTile) * Q.np + j0 + q % kPgsTile];
        __syncthreads();
        if (tid < 64) {
            double xi = (tid < kPgsTile) ? y[j0 + tid] : 0.0;
            for (int j = kPgsTile - 1; j >= 0; --j) {
                const double xj = __shfl(xi, j, 64);
                if (tid < j && j0 + j < n)
                    xi -= blk[j][tid] * xj;
            }
            if (tid < kPgsTile) {
                pan[tid] = xi;
                y[j0 + tid] = xi;
            }
        }
        __syncthreads();
        const int kmax = (n - j0 < kPgsTile) ? n - j0 : kPgsTile;
        for (int i = tid; i < j0; i += kPgsSolveBlock) {
            double v = y[i];
            for (int k = kmax - 1; k >= 0; --k)
                v -= Q.S[(size_t)(j0 + k) * Q.np + i] * pan[k];
            y[i] = v;
        }
        __syncthreads();
    }
    for (int i = tid; i < n; i += kPgsSolveBlock)
        Q.J.x[i] = y[i];
}

/* 3 n_local <= kPgsSmall: steps 2 and 3 in one workgroup, S in LDS */
__global__ __launch_bounds__(kPgsBlock) void k_pgs_small(PgSchurJob Q)
{
    __shared__ double A[kPgsSmall][kPgsSmall + 1];
    __shared__ double y[kPgsSmall], Lk[kPgsSmall], Wk[kPgsSmall];
    if (Q.st->done)
        return;
    const int tid = threadIdx.x, n = Q.n_s;
    for (int q = tid; q < n * n; q += kPgsBlock)
        A[q / n][q % n] = 0.0;
    __syncthreads();
    for (int id = tid; id < 9 * Q.n_sblk; id += kPgsBlock) {
        const int q = id / 9, ij = id - 9 * q, i = ij / 3, j = ij - 3 * i;
        A[3 * Q.sb_rc[2 * q] + i][3 * Q.sb_rc[2 * q + 1] + j] =
            pg_schur_entry(Q.J, Q.sb_rc, Q.sb_ptr, Q.sb_pair, Q.w, q, i, j);
    }
    if (tid < n)
        y[tid] = pg_schur_rhs(Q.J, Q.g, tid / 3, tid % 3);
    for (int k = 0; k < n; ++k) {
        __syncthreads();
        if (tid > k && tid < n) {
            const double d = A[k][k], l = A[tid][k] / d;
            A[tid][k] = l;
            Lk[tid] = l;
            Wk[tid] = l * d;
        }
        __syncthreads();
        const int m = n - k - 1;              /* rows and columns k + 1 .. n - 1 */
        for (int q = tid; q < m * m; q += kPgsBlock) {
            const int i = k + 1 + q / m, j = k + 1 + q % m;
            if (j <= i)
                A[i][j] -= Wk[i] * Lk[j];
        }
    }
    for (int k = 0; k < n; ++k) {
        __syncthreads();
        if (tid > k && tid < n)
            y[tid] -= A[tid][k] * y[k];
    }
    __syncthreads();
    if (tid < n)
        y[tid] = y[tid] / A[tid][tid];
    for (int k = n - 1; k >= 0; --k) {
        __syncthreads();
        if (tid < k)
            y[tid] -= A[k][tid] * y[k];
    }
    __syncthreads();
    if (tid < n)
        Q.J.x[tid] = y[tid];
}

__global__ __launch_bounds__(kPgsBlock) void k_pgs_back(PgSchurJob Q)
{
    const int t = Q.J.n_local + blockIdx.x * kPgsBlock + threadIdx.x;
    if (Q.st->done || t >= Q.J.n_nodes)
        return;
    pg_back_scan(Q.J, Q.g, Q.w, Q.J.x, t);
}

/* the true residual b - H delta and |b|^2 as per-workgroup partial sums; node += delta */
__global__ __launch_bounds__(kPgsBlock) void k_pgs_update(PgSchurJob Q)
{
    __shared__ double red[kPgsWaves][2];
    if (Q.st->done)
        return;
    const PgJob& J = Q.J;
    const int i = blockIdx.x * kPgsBlock + threadIdx.x;
    double v[2] = { 0.0, 0.0 };
    if (i < J.n_vars) {
        const double bi = J.b[i], r = bi - pg_row_times(J, i, J.x);
        v[0] = r * r;
        v[1] = bi * bi;
        J.pose[i] += J.x[i];
    }
    pg_block_sum<2, kPgsWaves>(v, red);
    if (threadIdx.x == 0) {
        Q.part[blockIdx.x] = v[0];
        Q.part[Q.nb_vars + blockIdx.x] = v[1];
    }
}

__global__ __launch_bounds__(kPgsBlock) void k_pgs_error(PgSchurJob Q)
{
    __shared__ double red[kPgsWaves][1];
    if (Q.st->done)
        return;
    const PgJob& J = Q.J;
    const int e = blockIdx.x * kPgsBlock + threadIdx.x;
    double v[1] = { 0.0 };
    if (e < J.n_edges)
        v[0] = pg_edge_loss_at(J, e);
    pg_block_sum<1, kPgsWaves>(v, red);
    if (threadIdx.x == 0)
        Q.part[2 * Q.nb_vars + blockIdx.x] = v[0];
}

/* one workgroup: the partial sums in a fixed shape, the step's trace record and the LM decision.
 * first != 0: only the initial total error. */
__global__ __launch_bounds__(kPgsBlock) void k_pgs_decide(PgSchurJob Q, int first)
{
    __shared__ double red[kPgsWaves][3];
    PgState& st = *Q.st;
    if (st.done)
        return;
    double v[3] = { 0.0, 0.0, 0.0 };
    if (!first)
        for (int q = threadIdx.x; q < Q.nb_vars; q += kPgsBlock) {
            v[0] += Q.part[q];
            v[1] += Q.part[Q.nb_vars + q];
        }
    for (int q = threadIdx.x; q < Q.nb_edges; q += kPgsBlock)
        v[2] += Q.part[2 * Q.nb_vars + q];
    pg_block_sum<3, kPgsWaves>(v, red);
    if (threadIdx.x != 0)
        return;
    const double total = v[2];
    if (first) {
        st.initial = total;
        Q.J.out[1] = total;
        return;
    }
    double* o = Q.J.out + 4 + 5 * (size_t)st.steps;
    o[0] = total;
    o[1] = st.lambda;
    o[2] = v[1];
    o[3] = v[0];
    o[4] = 0.0;
    const int steps = st.steps + 1;
    st.steps = steps;
    st.total = total;
    if (steps >= Q.J.iterations_max || fabs(st.prev - total) < Q.J.error_tolerance) {
        st.done = 1;
    } else {
        st.lambda = (total < st.prev) ? st.lambda * 0.5 : st.lambda * 2.0;
        st.prev = total;
    }
    Q.J.out[0] = (double)steps;
    Q.J.out[2] = total;
    Q.J.out[3] = st.lambda;
}

/* ================================================================== marginal covariances of node pairs
 * csm_pose_graph_marginals ("marginals"): H at lambda = 0 is eliminated and factored by
 * the kernels above; X = S^-1 is solved for the block columns C that the pairs need, every column by
 * itself (forward k ascending, division by d, backward k descending), and a pair's four 3x3 blocks are
 * put together from X, W and D_t^-1. X[r, c] is always the entry in row r of the solved column c. The
 * per-pair arithmetic is shared by the host restatement and the kernel.
 *
 * X is row-major [np][ldx]: column 3 m + j belongs to C[m]; sixteen nodes of C (kPgcGroup, 48 columns =
 * one tile) are a column group. The sweep is grid-wide with launches per panel, as the factorization's:
 * k_pgc_diag solves the panel's 48 rows of every group in LDS, k_pgc_update takes the panel out of every
 * row tile below (forward) or above (backward), a workgroup per (row tile, group). A group starts at
 * the panel of its first unit row; the host knows which groups are in play. */

constexpr int kPgcGroup = 16;     /* nodes of C per column group: 3 * 16 = kPgsTile columns */
static_assert(3 * kPgcGroup == kPgsTile, "a column group is one tile wide");

struct PgCovJob {
    PgSchurJob Q;
    int n_cols, ldx;              /* 3 |C|; n_cols rounded up to whole column groups (= the row stride of X) */
    int n_pairs;
    const int32_t* col_node;      /* [|C|]: ascending local map nodes */
    const int32_t* col_of;        /* [n_local]: position in C, or -1 */
    const int32_t* pairs;         /* [2 n_pairs]: local map node, scan node as a node index or -1 */
    double* X;                    /* [np * ldx] */
    double* out;                  /* [36 n_pairs]: local, scan, cross, relative */
};

/* (A B)(i, j) and (A B^T)(i, j) of row-major 3x3 blocks, left to right */
__host__ __device__ inline double pg_mul3(const double* A, const double* B, int i, int j)
{
    return A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

__host__ __device__ inline double pg_mul3t(const double* A, const double* B, int i, int j)
{
    return A[3 * i] * B[3 * j] + A[3 * i + 1] * B[3 * j + 1] + A[3 * i + 2] * B[3 * j + 2];
}

/* the record of pair (s, t): v = Sigma_ss, Sigma_tt, Sigma_st, relative (9 each, row-major). t is a node
 * index, or -1 for the local map node alone. Symmetric blocks are computed for i >= j and mirrored. */
__host__ __device__ inline void pg_marginal_pair(const PgJob& J, const double* w, const double* X, size_t ldx,
                                                 const int32_t* col_of, int s, int t, double* v)
{
    for (int q = 0; q < 36; ++q)
        v[q] = 0.0;
    const double* Xs = X + 3 * (size_t)s * ldx;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j <= i; ++j) {
            const double x = Xs[i * ldx + 3 * (size_t)col_of[s] + j];
            v[3 * i + j] = x;
            v[3 * j + i] = x;
        }
    if (t < 0)
        return;
    double *stt = v + 9, *sst = v + 18, *rel = v + 27;
    double f[6], Dinv[9];
    pg_ldl3(J.bv + 9 * (size_t)t, f);
    for (int j = 0; j < 3; ++j) {
        double x[3];
        pg_ldl3_solve(f, j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0, x);
        for (int i = 0; i < 3; ++i)
            Dinv[3 * i + j] = x[i];
    }
    const int q0 = J.row_ptr[t], q1 = J.row_ptr[t + 1];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double acc = 0.0;
            for (int a = q0; a < q1; ++a) {
                if (J.row_col[a] == t)
                    continue;
                const double* W = w + 9 * (size_t)((J.row_ent[a] >> 2) - J.n_nodes);
                const double* x = Xs + i * ldx + 3 * (size_t)col_of[J.row_col[a]];
                acc -= x[0] * W[3 * j] + x[1] * W[3 * j + 1] + x[2] * W[3 * j + 2];
            }
            sst[3 * i + j] = acc;
        }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j <= i; ++j) {
            double acc = Dinv[3 * i + j];
            for (int a = q0; a < q1; ++a) {
                if (J.row_col[a] == t)
                    continue;
                const double* Wa = w + 9 * (size_t)((J.row_ent[a] >> 2) - J.n_nodes);
                const double* Xa = X + 3 * (size_t)J.row_col[a] * ldx;
                for (int b = q0; b < q1; ++b) {
                    if (J.row_col[b] == t)
                        continue;
                    const double* Wb = w + 9 * (size_t)((J.row_ent[b] >> 2) - J.n_nodes);
                    const double* x = Xa + 3 * (size_t)col_of[J.row_col[b]];
                    double m[3];
                    for (int k = 0; k < 3; ++k)
                        m[k] = Wa[3 * i] * x[k] + Wa[3 * i + 1] * x[ldx + k] + Wa[3 * i + 2] * x[2 * ldx + k];
                    acc += m[0] * Wb[3 * j] + m[1] * Wb[3 * j + 1] + m[2] * Wb[3 * j + 2];
                }
            }
            stt[3 * i + j] = acc;
            stt[3 * j + i] = acc;
        }
    /* first-order covariance of InverseCompound(x_s, x_t): the Jacobians of pg_edge_values */
    const double zero[3] = { 0.0, 0.0, 0.0 };
    double e[3], c, sn, x, y;
    pg_error(J.pose + 3 * (size_t)s, J.pose + 3 * (size_t)t, zero, e, c, sn, x, y);
    const double Js[9] = { -c, -sn, y, sn, -c, -x, 0.0, 0.0, -1.0 };
    const double Je[9] = { c, sn, 0.0, -sn, c, 0.0, 0.0, 0.0, 1.0 };
    double sts[9], T1[9], T2[9], T3[9], T4[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            sts[3 * i + j] = sst[3 * j + i];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            T1[3 * i + j] = pg_mul3(Js, v, i, j);
            T2[3 * i + j] = pg_mul3(Js, sst, i, j);
            T3[3 * i + j] = pg_mul3(Je, sts, i, j);
            T4[3 * i + j] = pg_mul3(Je, stt, i, j);
        }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j <= i; ++j) {
            const double r = pg_mul3t(T1, Js, i, j) + pg_mul3t(T2, Je, i, j) + pg_mul3t(T3, Js, i, j) +
                             pg_mul3t(T4, Je, i, j);
            rel[3 * i + j] = r;
            rel[3 * j + i] = r;
        }
}

/* X = the unit columns of C, zeros in the padding rows and columns */
__global__ __launch_bounds__(kPgsBlock) void k_pgc_init(PgCovJob C)
{
    const size_t total = (size_t)C.Q.np * C.ldx;
    for (size_t i = (size_t)blockIdx.x * kPgsBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kPgsBlock) {
        const int r = (int)(i / C.ldx), c = (int)(i - (size_t)r * C.ldx);
        C.X[i] = (c < C.n_cols && r == 3 * C.col_node[c / 3] + c % 3) ? 1.0 : 0.0;
    }
}

/* z = y / d on the rows of S */
__global__ __launch_bounds__(kPgsBlock) void k_pgc_scale(PgCovJob C)
{
    const size_t total = (size_t)C.Q.n_s * C.ldx;
    for (size_t i = (size_t)blockIdx.x * kPgsBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kPgsBlock) {
        const size_t r = i / C.ldx;
        C.X[i] = C.X[i] / C.Q.S[r * C.Q.np + r];
    }
}

/* panel p, column group blockIdx.x: the triangular solve on the panel's own rows, in LDS. Forward: row i
 * takes rows j < i in ascending j; backward: rows j > i in descending j. Rows past n_s take no part. */
template <bool Fwd>
__global__ __launch_bounds__(kPgsBlock) void k_pgc_diag(PgCovJob C, int p)
{
    __shared__ double Lt[kPgsTile][kPgsTile + 1];
    __shared__ double Yt[kPgsTile][kPgsTile + 1];
    const PgSchurJob& Q = C.Q;
    const int tid = threadIdx.x, j0 = p * kPgsTile;
    const double* T = Q.S + (size_t)j0 * Q.np + j0;
    double* Y = C.X + (size_t)j0 * C.ldx + (size_t)blockIdx.x * kPgsTile;
    for (int q = tid; q < kPgsTile * kPgsTile; q += kPgsBlock) {
        const int r = q / kPgsTile, c = q % kPgsTile;
        Lt[r][c] = T[(size_t)r * Q.np + c];
        Yt[r][c] = Y[(size_t)r * C.ldx + c];
    }
    const int kmax = (Q.n_s - j0 < kPgsTile) ? Q.n_s - j0 : kPgsTile;
    if (Fwd) {
        for (int j = 0; j < kmax - 1; ++j) {
            __syncthreads();
            for (int q = tid; q < kPgsTile * kPgsTile; q += kPgsBlock) {
                const int i = q / kPgsTile, c = q % kPgsTile;
                if (i > j && i < kmax)
                    Yt[i][c] -= Lt[i][j] * Yt[j][c];
            }
        }
    } else {
        for (int j = kmax - 1; j >= 1; --j) {
            __syncthreads();
            for (int q = tid; q < kPgsTile * kPgsTile; q += kPgsBlock) {
                const int i = q / kPgsTile, c = q % kPgsTile;
                if (i < j)
                    Yt[i][c] -= Lt[j][i] * Yt[j][c];
            }
        }
    }
    __syncthreads();
    for (int q = tid; q < kmax * kPgsTile; q += kPgsBlock)
        Y[(size_t)(q / kPgsTile) * C.ldx + q % kPgsTile] = Yt[q / kPgsTile][q % kPgsTile];
}

/* panel p out of row tile ti of column group blockIdx.y: X_ic -= sum_k L_(i, j0 + k) X_(j0 + k, c) with k
 * ascending for the tiles below (forward), sum_k L_(j0 + k, i) X_(j0 + k, c) with k descending for the
 * tiles above (backward); a 3x3 register tile per thread, both operand tiles k-major in LDS */
template <bool Fwd>
__global__ __launch_bounds__(kPgsBlock) void k_pgc_update(PgCovJob C, int p)
{
    __shared__ double Lt[kPgsTile][kPgsTile + 1];
    __shared__ double Pt[kPgsTile][kPgsTile + 1];
    const PgSchurJob& Q = C.Q;
    const int ti = Fwd ? p + 1 + blockIdx.x : blockIdx.x;
    const int i0 = ti * kPgsTile, j0 = p * kPgsTile;
    const size_t c0 = (size_t)blockIdx.y * kPgsTile;
    for (int q = threadIdx.x; q < kPgsTile * kPgsTile; q += kPgsBlock) {
        const int a = q / kPgsTile, b = q % kPgsTile;
        if (Fwd)
            Lt[b][a] = Q.S[(size_t)(i0 + a) * Q.np + j0 + b];
        else
            Lt[a][b] = Q.S[(size_t)(j0 + a) * Q.np + i0 + b];
        Pt[a][b] = C.X[(size_t)(j0 + a) * C.ldx + c0 + b];
    }
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    double acc[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b)
            acc[a][b] = C.X[(size_t)(i0 + ty + 16 * a) * C.ldx + c0 + tx + 16 * b];
    __syncthreads();
    const int kmax = (Q.n_s - j0 < kPgsTile) ? Q.n_s - j0 : kPgsTile;
    for (int kk = 0; kk < kmax; ++kk) {
        const int k = Fwd ? kk : kmax - 1 - kk;
        double lv[3], pv[3];
        for (int a = 0; a < 3; ++a) {
            lv[a] = Lt[k][ty + 16 * a];
            pv[a] = Pt[k][tx + 16 * a];
        }
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b)
                acc[a][b] -= lv[a] * pv[b];
    }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b)
            C.X[(size_t)(i0 + ty + 16 * a) * C.ldx + c0 + tx + 16 * b] = acc[a][b];
}

__global__ __launch_bounds__(kPgsBlock) void k_pgc_pairs(PgCovJob C)
{
    const int q = blockIdx.x * kPgsBlock + threadIdx.x;
    if (q >= C.n_pairs)
        return;
    pg_marginal_pair(C.Q.J, C.Q.w, C.X, (size_t)C.ldx, C.col_of, C.pairs[2 * q], C.pairs[2 * q + 1],
                     C.out + 36 * (size_t)q);
}

} /* namespace csm */
#endif
