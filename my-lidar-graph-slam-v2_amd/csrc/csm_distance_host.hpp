/* csm_distance_host.hpp -- the host restatements of the distance fields (csm_host_distance_kernel,
 * csm_host_distance_transform, csm_host_distance_map of include/csm_hip.h) and the argument checks the device
 * entries share with them. Plain C++ without a HIP call: included by csm_distance_api.hip, which makes them
 * part of libcsm_hip.so, and by tools/distance_host_check.cpp, which runs them under the sanitizers. It
 * DEFINES the three functions: one translation unit of a program includes it. */
#ifndef CSM_DISTANCE_HOST_HPP
#define CSM_DISTANCE_HOST_HPP

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/csm_hip.h"

namespace csm_distance_host {

constexpr int kMaxSide = 32767;         /* d2 < 2^31, a row offset fits 16 bits */

inline bool shape_ok(int rows, int cols) { return rows >= 1 && cols >= 1 && rows <= kMaxSide && cols <= kMaxSide; }

inline bool params_ok(const csm_distance_params* p)
{
    if (!p || !p->table || p->radius < 1 || p->radius > CSM_DISTANCE_MAX_RADIUS || p->occupied_min < 1)
        return false;
    for (int i = 0; i <= p->radius * p->radius; ++i)
        if (p->table[i] > 65534u)
            return false;
    return true;
}

/* The two passes on the host, sequentially. Pass 1 as on the device: per column the offset to the nearest
 * obstacle of the column, the upper of two equally near. Pass 2 walks, per cell, over the COLUMNS THAT HOLD
 * AN OBSTACLE (ascending list, the same for every row) to the right and to the left of the cell while the
 * squared column distance, plus the squared distance of the row to its nearest obstacle row-wise, does not
 * exceed the best d2: the tie rule of the device (an equal d2 is still visited), on a list instead of on every
 * column, so an empty map costs nothing, a sparse one little, and a wall along a far row one step per cell. */
inline void transform(const uint16_t* grid, int rows, int cols, uint32_t occupied_min, uint32_t* d2_out,
                      uint32_t* nearest_out)
{
    constexpr int32_t none = INT32_MIN;
    std::vector<int32_t> off((size_t)rows * cols, none);
    std::vector<int> occupied_cols;
    for (int c = 0; c < cols; ++c) {
        int last = -1;
        for (int r = 0; r < rows; ++r) {
            if (grid[(size_t)r * cols + c] >= occupied_min)
                last = r;
            if (last >= 0)
                off[(size_t)r * cols + c] = last - r;
        }
        if (last >= 0)
            occupied_cols.push_back(c);
        last = -1;
        for (int r = rows - 1; r >= 0; --r) {
            int32_t& o = off[(size_t)r * cols + c];
            if (o == 0)
                last = r;
            else if (last >= 0 && (o == none || last - r < -o))
                o = last - r;
        }
    }
    const int n_occ = (int)occupied_cols.size();
    for (int r = 0; r < rows; ++r) {
        const int32_t* g = off.data() + (size_t)r * cols;
        /* no obstacle is nearer to this row than `near2` (squared), whatever its column: a listed column at
         * distance dc holds nothing below dc^2 + near2, which ends the walk early under a far wall */
        int64_t near2 = INT64_MAX;
        for (int i = 0; i < n_occ; ++i)
            near2 = std::min(near2, (int64_t)g[occupied_cols[i]] * g[occupied_cols[i]]);
        int at = 0;                                 /* the first listed column >= c */
        for (int c = 0; c < cols; ++c) {
            while (at < n_occ && occupied_cols[at] < c)
                ++at;
            uint64_t best = ~(uint64_t)0;
            auto visit = [&](int cc) {
                const int64_t dc = cc - c, o = g[cc];
                if ((uint64_t)(dc * dc + near2) > (best >> 32))
                    return false;
                best = std::min(best, (uint64_t)(dc * dc + o * o) << 32 | (uint64_t)((r + o) * cols + cc));
                return true;
            };
            for (int i = at; i < n_occ && visit(occupied_cols[i]); ++i) { }
            for (int i = at - 1; i >= 0 && visit(occupied_cols[i]); --i) { }
            if (d2_out)
                d2_out[(size_t)r * cols + c] = (uint32_t)(best >> 32);
            if (nearest_out)
                nearest_out[(size_t)r * cols + c] = (uint32_t)best;
        }
    }
}

} /* namespace csm_distance_host */

extern "C" {

int csm_host_distance_kernel(double sigma, double resolution, int32_t radius, uint32_t peak, uint32_t floor_value,
                             uint16_t* table)
{
    if (!(std::isfinite(sigma) && std::isfinite(resolution) && sigma > 0.0 && resolution > 0.0) || radius < 1 ||
        radius > CSM_DISTANCE_MAX_RADIUS || peak > 65534u || floor_value > peak || !table)
        return CSM_EINVAL;
    for (int d2 = 0; d2 <= radius * radius; ++d2)
        table[d2] = (uint16_t)(floor_value + (uint16_t)std::floor(
            (double)(peak - floor_value) * std::exp(-((double)d2 * (resolution * resolution)) / (2.0 * (sigma * sigma))) +
            0.5));
    return CSM_OK;
}

int csm_host_distance_transform(const uint16_t* grid, int32_t rows, int32_t cols, uint32_t occupied_min,
                                uint32_t* d2, uint32_t* nearest)
{
    if (!grid || !csm_distance_host::shape_ok(rows, cols) || occupied_min < 1 || (!d2 && !nearest))
        return CSM_EINVAL;
    csm_distance_host::transform(grid, rows, cols, occupied_min, d2, nearest);
    return CSM_OK;
}

int csm_host_distance_map(const uint16_t* grid, int32_t rows, int32_t cols, const csm_distance_params* prm,
                          uint16_t* out)
{
    if (!grid || !out || !csm_distance_host::shape_ok(rows, cols) || !csm_distance_host::params_ok(prm))
        return CSM_EINVAL;
    std::vector<uint32_t> d2((size_t)rows * cols);
    csm_distance_host::transform(grid, rows, cols, prm->occupied_min, d2.data(), nullptr);
    const uint32_t R2 = (uint32_t)(prm->radius * prm->radius);
    for (size_t i = 0; i < d2.size(); ++i)
        out[i] = prm->keep_unknown && grid[i] == 0 ? 0 : prm->table[std::min(d2[i], R2)];
    return CSM_OK;
}

} /* extern "C" */

#endif
