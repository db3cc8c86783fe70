/* csm_certify.hpp -- the projection certificate, in one place.
 *
 * The reference turns a beam into a cell with ScanData::HitPoint (inc/sensor/sensor_data.hpp:189-203) and
 * PositionToIndex (src/grid_map_new/grid_map_geometry.cpp:113-122): floor((pose + r trig - off) / res), with
 * glibc's sin / cos. The device evaluates the same quotient q with its own libm and trusts floor(q) only where q
 * is farther from a cell edge than a bound on |q_host - q_device|; everything else is listed and recomputed on
 * the host by host_hit_point + cell_index below, exactly as the reference does. Every build uses
 * -ffp-contract=off: these functions inline to the operations written here, in this order. */
#ifndef CSM_CERTIFY_HPP
#define CSM_CERTIFY_HPP

#include <hip/hip_runtime.h>

#include <cmath>

namespace csm {

/* Every bound below is multiplied by this before it is used: the bounds are first-order. */
constexpr double kCertSafety = 64.0;
/* |device trig - glibc trig| when both take the same argument: 3 ulp between the two libms, values <= 1. */
constexpr double kLibmTrigErr = 8e-16;
/* ... when the device forms cos(B + D) from the addition theorems: four library results at <= 3 ulp, two
 * products and one sum. The angle roundings come on top (addition_trig_err). */
constexpr double kAdditionTrigErr = 2.4e-15;
/* One rounding on either side, relative: of an angle sum, of the hit coordinate, of h - off. */
constexpr double kRoundErr = 4e-16;
/* The quotient's own roundings, relative to |q|: a division, or (h - off) * (1 / res) with two roundings more. */
constexpr double kQuotDivErr = 4e-16;
constexpr double kQuotRecipErr = 8e-16;
/* Division form only: the integers taken from a hit point are used in a frame moved by a whole number of cells
 * (a resize); q there is q here plus an integer up to roundings of the coordinates, never measured against
 * less than 1e3 m. */
constexpr double kFrameSlack = 2.3e-16;
constexpr double kFrameFloor = 1.0e3;
/* Branch and bound's per-node margins (proj_body, the only user): the node offset adds a rounding to the
 * coordinate and one to the quotient. */
constexpr double kNodeRoundErr = 8e-16;
constexpr double kNodeQuotErr = 1.2e-15;

/* PositionToIndex, IEEE double, no contraction: bit-identical on host and device. */
__host__ __device__ __forceinline__ int cell_index(double pos, double off, double res)
{
    return (int)floor((pos - off) / res);
}

/* Division form. Bound on |q_host - q_device| for q = (sensor + r*trig - off) / res, in cells. `trig_err`:
 * absolute error of the device's cosine / sine against the host's; then one rounding per arithmetic step on
 * either side; the caller multiplies by kCertSafety. */
__device__ __forceinline__ double proj_err_bound(double r, double hit, double off, double res,
                                                 double q, double trig_err)
{
    return (fabs(r) * trig_err + (fabs(hit) + fabs(off)) * kRoundErr) / res + fabs(q) * kQuotDivErr;
}

/* Reciprocal form: the same for q = (sensor + r*trig - off) * inv_res. */
__device__ __forceinline__ double proj_err_bound_recip(double r, double hit, double off, double inv_res,
                                                       double q, double trig_err)
{
    return (fabs(r) * trig_err + (fabs(hit) + fabs(off)) * kRoundErr) * inv_res + fabs(q) * kQuotRecipErr;
}

/* trig_err of the addition-theorem path; angle_sum = the |angles| whose sum the host rounds. */
__device__ __forceinline__ double addition_trig_err(double angle_sum)
{
    return kAdditionTrigErr + kRoundErr * angle_sum;
}

/* The decision: frac = q - floor(q) is farther than m from both cell edges. */
__device__ __forceinline__ bool off_cell_edge(double frac, double m)
{
    return frac > m && frac < 1.0 - m;
}

/* The margin of a hit coordinate h = sensor + r * trig(arg), both libms on the same arg, whose integers may be
 * used in a frame a resize moves: division form plus the frame slack. q = (h - off) / res. */
__device__ __forceinline__ double direct_margin(double r, double h, double off, double res, double q)
{
    return kCertSafety * proj_err_bound(r, h, off, res, q, kLibmTrigErr) +
           kCertSafety * kFrameSlack * (fabs(h) + fabs(off) + kFrameFloor) / res;
}

/* Does floor((h - off) / res) equal what the host gets with glibc? */
__device__ __forceinline__ bool certified(double r, double h, double off, double res)
{
    const double q = (h - off) / res;
    const double m = direct_margin(r, h, off, res, q);
    const double frac = q - floor(q);
    return off_cell_edge(frac, m);
}

/* ---- host: what a listed item is recomputed with ---- */

/* The products of ScanData::HitPoint with glibc: r cos(theta + a), r sin(theta + a). */
inline void host_hit_products(double theta, double r, double a, double* rc, double* rs)
{
    *rc = r * std::cos(theta + a);
    *rs = r * std::sin(theta + a);
}

/* ScanData::HitPoint at sensor pose (x, y, theta): the products, then the sums. */
inline void host_hit_point(double x, double y, double theta, double r, double a, double* hx, double* hy)
{
    double rc, rs;
    host_hit_products(theta, r, a, &rc, &rs);
    *hx = x + rc;
    *hy = y + rs;
}

} /* namespace csm */
#endif
