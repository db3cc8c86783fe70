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

/* NormalizeAngle (include/my_lidar_graph_slam/util.hpp:282-292) */
__host__ __device__ inline double pg_normalize_angle(double theta)
{
    const double pi = 3.14159265358979323846;
    double t = fmod(theta, 2.0 * pi);
    if (t > pi)
        t -= 2.0 * pi;
    else if (t < -pi)
        t += 2.0 * pi;
    return t;
}

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

/* sum of one value per thread: wave butterfly (every lane ends with the same bits), the wave sums
 * through LDS buffer `buf`, added in wave order by every thread. One barrier; the two alternating
 * buffers keep a buffer's next writes behind the following reduction's barrier. */
template <int N>
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
        for (int w = 1; w < kPgWaves; ++w)
            s += buf[w][q];
        v[q] = s;
    }
}

__device__ inline double pg_total_error(const PgJob& J, double (*buf)[1])
{
    double v[1] = { 0.0 };
    for (int e = threadIdx.x; e < J.n_edges; e += kPgBlock) {
        const double* ps = J.pose + 3 * (size_t)J.enode[2 * e];
        const double* pe = J.pose + 3 * (size_t)J.enode[2 * e + 1];
        v[0] += pg_edge_loss(ps, pe, J.rel + 3 * (size_t)e, J.info + 9 * (size_t)e, J.loss_type, J.loss_scale);
    }
    pg_block_sum<1>(v, buf);
    return v[0];
}

__global__ __launch_bounds__(kPgBlock) void k_pose_graph_lm(PgJob J)
{
    __shared__ double red1[2][kPgWaves][1];
    __shared__ double red2[2][kPgWaves][2];
    int flip = 0;
    auto sum1 = [&](double x) {
        double v[1] = { x };
        pg_block_sum<1>(v, red1[flip]);
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
        for (int e = tid; e < J.n_edges; e += kPgBlock) {
            const double* ps = J.pose + 3 * (size_t)J.enode[2 * e];
            const double* pe = J.pose + 3 * (size_t)J.enode[2 * e + 1];
            pg_edge_values(ps, pe, J.rel + 3 * (size_t)e, J.info + 9 * (size_t)e, J.is_loop[e], J.loss_type,
                           J.loss_scale, J.ev + (size_t)kPgEdgeVals * e);
        }
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
                    pg_block_sum<2>(v, red2[flip]);
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

} /* namespace csm */
#endif
