/* csm_ray.hpp -- what the two units that walk single rays through a resident map share: the free-space
 * check of loop candidates (csm_ray_api.hip, csm_ray_kernels.hip) and the ray cast (csm_cast_api.hip,
 * csm_cast_kernels.hip). One text each of
 *   device  RayRec / RayPatch, ray_project (a beam's end point with the device's sin / cos, its integers and
 *           the map builder's certificate), ray_list (the list of beams the host recomputes), ray_patch_one;
 *   host    ray_unc_cap, ray_frame (the limits that keep the closed form within 64 bits, and the sensor's
 *           sub-pixel index), ray_host_rec (ScanData::HitPoint with glibc), host_floor_div and ray_step_cells
 *           (BresenhamScaled step by step).
 * The cells of a ray come from ray_cells_closed_form / ray_column_rows (csm_map.hpp). gfx950 only. */
#ifndef CSM_RAY_HPP
#define CSM_RAY_HPP

#include "csm_internal.hpp"
#include "csm_map.hpp"

namespace csm {

constexpr int32_t kRayUnusable = (int32_t)0x80000000;   /* RayRec.ex of an unusable beam (no index reaches it) */

struct RayRec {
    int32_t ex, ey;            /* sub-pixel index of the hit point; ex = kRayUnusable: the beam is not usable */
    int32_t hx, hy;            /* the hit cell H (the ray check; the cast leaves 0) */
};

struct RayPatch {
    uint32_t beam;
    RayRec   rec;
};

/* The beam of range r at angle a from the sensor pose (x, y, theta): its record, and in `sure` whether every
 * integer of it is certified (csm_certify.hpp). kCell: the hit cell H is wanted too, and certified with the rest. */
template <bool kCell>
__device__ __forceinline__ RayRec ray_project(double x, double y, double theta, double r, double a, double off_x,
                                              double off_y, double res, double scaled_res, bool& sure)
{
    const double arg = theta + a;
    const double hx = x + r * cos(arg);
    const double hy = y + r * sin(arg);
    RayRec rec;
    rec.ex = cell_index(hx, off_x, scaled_res);
    rec.ey = cell_index(hy, off_y, scaled_res);
    rec.hx = kCell ? cell_index(hx, off_x, res) : 0;
    rec.hy = kCell ? cell_index(hy, off_y, res) : 0;
    sure = (!kCell || (certified(r, hx, off_x, res) && certified(r, hy, off_y, res))) &&
           certified(r, hx, off_x, scaled_res) && certified(r, hy, off_y, scaled_res);
    return rec;
}

/* beam b goes onto the list of the host: unc[0] counts, unc[1 ..] holds the first `cap` of them */
__device__ __forceinline__ void ray_list(uint32_t* unc, uint32_t cap, uint32_t b)
{
    const uint32_t pos = atomicAdd(unc, 1u);
    if (pos < cap)
        unc[1 + pos] = b;
}

/* thread i of a launch over n patches: the host's record into its place */
__device__ __forceinline__ void ray_patch_one(const RayPatch* patches, int n, RayRec* recs, int i)
{
    if (i < n)
        recs[patches[i].beam] = patches[i].rec;
}

} /* namespace csm */

namespace csm_host {

constexpr double kRayMaxCells = 1048576.0;           /* 2^20: the 64-bit bound of the closed form */
constexpr int64_t kRayDefaultScratch = 1ll << 30;

inline uint32_t ray_unc_cap(const csm_ctx* ctx)      /* csm_config.map_uncertain_cap, as the map builder */
{
    return ctx->tune.map_unc_cap > 0 ? (uint32_t)std::min<long>(ctx->tune.map_unc_cap, kMapUncCap) : kMapUncCap;
}

/* The sensor pose S in the frame of `geom` (finite, checked by the caller) with rays of at most range_max:
 * false where a coordinate could leave the bound of the closed form (include/csm_hip.h, "64 bits");
 * otherwise s = the sub-pixel index of the sensor position. */
inline bool ray_frame(const csm_geometry* geom, const double S[3], double range_max, int scale, int32_t s[2])
{
    const double res = geom->resolution;
    if (!(std::fabs((S[0] - geom->offset_x) / res) <= kRayMaxCells) ||
        !(std::fabs((S[1] - geom->offset_y) / res) <= kRayMaxCells) || !(range_max / res <= kRayMaxCells))
        return false;
    const double scaled_res = res / scale;
    s[0] = cell_index(S[0], geom->offset_x, scaled_res);
    s[1] = cell_index(S[1], geom->offset_y, scaled_res);
    return true;
}

/* ScanData::HitPoint with glibc (host_hit_point, csm_certify.hpp), and its four integers */
inline RayRec ray_host_rec(const double S[3], const csm_geometry* geom, double scaled_res, double r, double a)
{
    double hx, hy;
    host_hit_point(S[0], S[1], S[2], r, a, &hx, &hy);
    RayRec rec;
    rec.ex = cell_index(hx, geom->offset_x, scaled_res);
    rec.ey = cell_index(hy, geom->offset_y, scaled_res);
    rec.hx = cell_index(hx, geom->offset_x, geom->resolution);
    rec.hy = cell_index(hy, geom->offset_y, geom->resolution);
    return rec;
}

inline int host_floor_div(int a, int b)
{
    const int q = a / b;
    return q * b > a ? q - 1 : q;
}

typedef std::pair<int, int> Cell;   /* (x = column, y = row) */

/* BresenhamScaled (src/bresenham.cpp:58-237) step by step, on non-negative coordinates: the error term is
 * carried from column to column as the reference carries it. The falling case runs the rising loop on the
 * mirrored sub-row position (subY < 0 <-> subY > denominator, subY == 0 <-> subY == denominator). */
inline void ray_step_cells(int sx, int sy, int ex, int ey, int scale, std::vector<Cell>& out)
{
    out.clear();
    if (sx > ex) {
        std::swap(sx, ex);
        std::swap(sy, ey);
    }
    const int start_x = sx / scale, start_y = sy / scale, end_x = ex / scale, end_y = ey / scale;
    auto visit = [&out](int x, int y) {
        if (out.empty() || out.back() != Cell(x, y))
            out.emplace_back(x, y);
    };
    if (start_x == end_x) {
        for (int y = std::min(start_y, end_y); y <= std::max(start_y, end_y); ++y)
            visit(start_x, y);
        return;
    }
    const int64_t dx = ex - sx, dy = ey - sy;
    const int64_t denom = 2 * static_cast<int64_t>(scale) * dx;
    const int up = dy > 0 ? 1 : -1;
    const int64_t rise = dy > 0 ? dy : -dy;
    int64_t sub = (2 * (sy % scale) + 1) * dx;
    if (up < 0)
        sub = denom - sub;
    int x = start_x, y = start_y;
    visit(x, y);
    sub += rise * (2 * scale - (2 * (sx % scale) + 1));
    for (;;) {
        visit(x, y);
        while (sub > denom) {
            sub -= denom;
            y += up;
            visit(x, y);
        }
        if (sub == denom) {                 /* exactly through a corner: a diagonal step */
            sub -= denom;
            y += up;
        }
        if (++x == end_x)
            break;
        sub += 2 * rise * scale;
    }
    sub += rise * (2 * (ex % scale) + 1);
    visit(x, y);
    while (sub > denom) {
        sub -= denom;
        y += up;
        visit(x, y);
    }
}

} /* namespace csm_host */

#endif
