/* csm_pg_math.hpp -- the three pieces of the pose-graph arithmetic that more than one unit calls, __host__
 * __device__ so that a host restatement and a kernel share the text: NormalizeAngle and the unpivoted 3x3
 * LDL^T with its substitution. Included by csm_posegraph_kernels.hip (the optimizer, the marginals, the
 * loop gate) and csm_consistency_kernels.hip (the cycle test of two loop edges). */
#ifndef CSM_PG_MATH_HPP
#define CSM_PG_MATH_HPP

#include <hip/hip_runtime.h>
#include <cmath>

namespace csm {

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

/* unpivoted LDL^T of a self-adjoint 3x3 block read from its lower triangle (row-major, 9 entries):
 * f = d0 d1 d2 l10 l20 l21; the same formulas as the dense factorization of S */
__host__ __device__ inline void pg_ldl3(const double* D, double f[6])
{
    f[0] = D[0];
    f[3] = D[3] / f[0];
    f[4] = D[6] / f[0];
    f[1] = D[4] - (f[3] * f[0]) * f[3];
    f[5] = (D[7] - (f[4] * f[0]) * f[3]) / f[1];
    f[2] = D[8] - (f[4] * f[0]) * f[4] - (f[5] * f[1]) * f[5];
}

/* forward (k ascending), diagonal, backward (k descending) */
__host__ __device__ inline void pg_ldl3_solve(const double f[6], double v0, double v1, double v2, double x[3])
{
    const double y1 = v1 - f[3] * v0;
    const double y2 = v2 - f[4] * v0 - f[5] * y1;
    const double z0 = v0 / f[0], z1 = y1 / f[1], z2 = y2 / f[2];
    x[2] = z2;
    x[1] = z1 - f[5] * x[2];
    x[0] = z0 - f[4] * x[2] - f[3] * x[1];
}

} /* namespace csm */
#endif
