/* csm_cast_kernels.hip -- rays cast through a resident map (included by csm_cast_api.hip; the definition is
 * in include/csm_hip.h, csm_ray_cast). gfx950 only.
 *
 *   k_cast_project  one thread per ray of a chunk: the beam's limit, its end point with the device's sin / cos
 *                   and the certificate at the sub-pixel resolution on both axes (ray_project, csm_ray.hpp:
 *                   the text k_ray_project runs). A ray that is not certified is listed for the host.
 *   k_cast_patch    the listed rays' records as glibc gives them, scattered into place (ray_patch_one).
 *   k_cast_walk     256 threads = 4 wavefronts, kCastGroup consecutive rays of ONE pose per workgroup, one
 *                   wavefront per ray. The cells of the ray are those of the closed form of csm_map.hpp
 *                   (ray_column_rows: the one text of a column's rows), enumerated FROM THE SENSOR'S END:
 *                   rounds of 64 columns in travel order (descending columns when the reference would have
 *                   swapped its end points), each column's rows in travel order, cell number t of a round on
 *                   lane t mod 64. After every 64 cells one ballot of the stop predicate; its lowest lane is
 *                   the first stopping cell seen from the sensor, and the wavefront leaves the loops there.
 *                   The enumeration is clipped to the map first: the cells of a straight walk that lie inside
 *                   a rectangle are consecutive, so a ray that has left the map is finished. Every trip count
 *                   is fixed before its loop starts; the one early exit is wave-uniform. Lane 0 writes the
 *                   ray's record; threads 0 and 1 write the workgroup's two cell counts. No atomics, nothing read
 *                   that another workgroup writes. */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csm_ray.hpp"

namespace csm {

constexpr int kCastGroup = 16;               /* rays per workgroup of k_cast_walk: 4 per wavefront */
constexpr int kCastRecordBytes = 24;         /* csm_ray_cast_record */

/* consecutive poses of one set, as far as they lie in the chunk */
struct CastSeg {
    const uint16_t* cells;     /* level 0 of its map */
    int32_t rows, cols, pitch;
    int32_t n_beams;
    long long angles_at, ranges_at;   /* its scan in the chunk's staged doubles; ranges_at < 0: no limits */
    long long pose_at;         /* its first pose among the chunk's */
    int32_t n_poses, groups;   /* workgroups of k_cast_walk per pose */
    double  off_x, off_y, res, scaled_res;
    long long min_dist2;       /* at this set's resolution */
};

struct CastPose {
    double  x, y, theta;       /* the sensor pose */
    int32_t sx, sy;            /* sub-pixel index of the sensor position (host) */
};

struct CastRecord {            /* csm_ray_cast_record */
    int32_t cell_x, cell_y;
    uint32_t value;
    int32_t kind;
    long long dist2;
};

struct CastChunk {
    const CastSeg* segs;
    const uint32_t* pre_ray;   /* [n_segs + 1] rays before each segment */
    const uint32_t* pre_group; /* [n_segs + 1] workgroups of k_cast_walk before each segment */
    const CastPose* poses;
    const double* scans;
    RayRec* recs;              /* [n_rays] */
    CastRecord* records;       /* [n_rays] */
    uint32_t* group_cells;     /* [workgroups][2]: cells read, cells up to the stop */
    uint32_t* unc;             /* [0] count, [1 ..] the listed rays */
    uint32_t unc_cap;
    int32_t n_segs, n_rays;
    double  range_max;
    int32_t scale, unknown_stops;
    uint32_t occupied_min;
    int32_t pad;
};

__global__ __launch_bounds__(256) void k_cast_project(CastChunk ch)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= ch.n_rays)
        return;
    const int si = prefix_find(ch.pre_ray, ch.n_segs, (uint32_t)b);
    const CastSeg& q = ch.segs[si];
    const int local = b - (int)ch.pre_ray[si];
    const int p = local / q.n_beams, i = local - p * q.n_beams;
    const CastPose pose = ch.poses[q.pose_at + p];
    const double r = q.ranges_at < 0 ? ch.range_max : ch.scans[q.ranges_at + i];
    RayRec rec = { kRayUnusable, 0, 0, 0 };
    if (q.ranges_at < 0 || r > 0.0) {
        const double limit = r < ch.range_max ? r : ch.range_max;
        bool sure;
        rec = ray_project<false>(pose.x, pose.y, pose.theta, limit, ch.scans[q.angles_at + i], q.off_x, q.off_y, q.res,
                                 q.scaled_res, sure);
        if (!sure)
            ray_list(ch.unc, ch.unc_cap, (uint32_t)b);
    }
    ch.recs[b] = rec;
}

__global__ __launch_bounds__(256) void k_cast_patch(const RayPatch* patches, int n, RayRec* recs)
{
    ray_patch_one(patches, n, recs, blockIdx.x * 256 + threadIdx.x);
}

/* what a wavefront needs of its ray's map and rules */
struct CastRule {
    const uint16_t* cells;
    int pitch, scale;
    long long sx2, sy2;        /* 2 s + 1 - scale per axis: D = 2 c scale - this */
    long long min_dist2;
    uint32_t occupied_min;
    bool unknown_stops;
};

/* One group of up to 64 cells in travel order, cell (x, y) on this lane if `valid` (inside the map: the clip).
 * True: the ray stops in this group, and `stop` holds its record on every lane. */
__device__ __forceinline__ bool cast_probe(const CastRule& rule, bool valid, int x, int y, int lane, CastRecord& stop,
                                           int& stop_lane)
{
    uint32_t v = 0;
    long long d2 = 0;
    int kind = CSM_CAST_NONE;
    if (valid) {
        v = rule.cells[(ptrdiff_t)y * rule.pitch + x];
        const long long dx = 2ll * x * rule.scale - rule.sx2, dy = 2ll * y * rule.scale - rule.sy2;
        d2 = dx * dx + dy * dy;
        if (d2 >= rule.min_dist2)
            kind = v >= rule.occupied_min ? CSM_CAST_OCCUPIED : (rule.unknown_stops && v == 0) ? CSM_CAST_UNKNOWN
                                                                                               : CSM_CAST_NONE;
    }
    const unsigned long long hit = __ballot(kind != CSM_CAST_NONE);
    if (hit == 0ull)
        return false;
    stop_lane = __ffsll((long long)hit) - 1;       /* lanes hold the group's cells in travel order */
    stop.cell_x = __shfl(x, stop_lane);
    stop.cell_y = __shfl(y, stop_lane);
    stop.value = (uint32_t)__shfl((int)v, stop_lane);
    stop.kind = __shfl(kind, stop_lane);
    stop.dist2 = __shfl(d2, stop_lane);
    return true;
}

/* The ray from sub-pixel (sx, sy) to (ex, ey) on one wavefront: true and its record in `stop` if it stops.
 * n_read += the cells read, n_upto += the cells up to and including the stop (all of them without one). */
__device__ __forceinline__ bool cast_walk_ray(const CastSeg& q, const CastChunk& ch, int sx, int sy, int ex, int ey,
                                              int lane, CastRecord& stop, uint32_t& n_read, uint32_t& n_upto)
{
    const int scale = ch.scale;
    /* the same ray moved by whole cells into non-negative coordinates */
    const int bx = floor_div(min(sx, ex), scale), by = floor_div(min(sy, ey), scale);
    const RayClip clip = { -bx, q.cols - 1 - bx, -by, q.rows - 1 - by };
    /* the rule reads the map and measures from the sensor in the moved frame */
    const CastRule rule = { q.cells + (ptrdiff_t)by * q.pitch + bx, q.pitch, scale,
                            2ll * sx + 1 - scale - 2ll * bx * scale, 2ll * sy + 1 - scale - 2ll * by * scale,
                            q.min_dist2, ch.occupied_min, ch.unknown_stops != 0 };
    int ax = sx - bx * scale, ay = sy - by * scale, cx = ex - bx * scale, cy = ey - by * scale;
    const int sensor_row = ay / scale, end_row = cy / scale;
    const bool swapped = ax > cx;             /* bresenham.cpp:67-70: the reference walks from the other end */
    if (swapped) {
        int t = ax; ax = cx; cx = t;
        t = ay; ay = cy; cy = t;
    }
    const int x0 = ax / scale, y0 = ay / scale, x1 = cx / scale, y1 = cy / scale;
    int stop_lane = 0;
    auto stopped = [&]() {                    /* the walk runs in the moved frame */
        stop.cell_x += bx;
        stop.cell_y += by;
        n_upto += (uint32_t)stop_lane + 1u;
        return true;
    };
    if (x0 == x1) {                           /* bresenham.cpp:87-99: one column, rows from the sensor's */
        if (x0 < clip.x_lo || x0 > clip.x_hi)
            return false;
        const int lo = max(min(y0, y1), clip.y_lo), hi = min(max(y0, y1), clip.y_hi);
        const bool up = sensor_row <= end_row;
        const int total = hi - lo + 1;
        for (int t0 = 0; t0 < total; t0 += 64) {
            const int t = t0 + lane;
            const uint32_t here = (uint32_t)min(64, total - t0);
            n_read += here;
            if (cast_probe(rule, t < total, x0, up ? lo + t : hi - t, lane, stop, stop_lane))
                return stopped();
            n_upto += here;
        }
        return false;
    }
    const long long dx = cx - ax, dy = cy - ay;
    const long long den = 2ll * scale * dx;
    const long long n0 = (long long)y0 * den + (2ll * (ay % scale) + 1) * dx;
    const long long first_part = 2ll * scale - (2ll * (ax % scale) + 1), last_part = 2ll * (cx % scale) + 1;
    const int m = x1 - x0;
    const int j_lo = max(0, clip.x_lo - x0), j_hi = min(m, clip.x_hi - x0);
    const int n_cols = j_hi - j_lo + 1;
    const bool up = (dy > 0) != swapped;      /* rows of a column in travel order */
    for (int u0 = 0; u0 < n_cols; u0 += 64) { /* rounds of 64 columns in travel order */
        const int u = u0 + lane;
        int from = 0, to = -1;
        if (u < n_cols) {
            ray_column_rows(swapped ? j_hi - u : j_lo + u, m, y0, scale, n0, dy, den, first_part, last_part, from,
                            to);
            from = max(from, clip.y_lo);
            to = min(to, clip.y_hi);
        }
        const int count = max(to - from + 1, 0);
        const int first = up ? from : to;     /* the column's first row in travel order */
        int incl = count;
        for (int off = 1; off < 64; off <<= 1) {
            const int below = __shfl_up(incl, off);
            if (lane >= off)
                incl += below;
        }
        const int excl = incl - count;
        const int total = __shfl(incl, 63);
        for (int t0 = 0; t0 < total; t0 += 64) {
            const int t = t0 + lane;
            int c = 0;                        /* last column whose first cell number is <= t */
            for (int step = 32; step; step >>= 1) {
                const int e = __shfl(excl, min(c + step, 63));
                if (c + step < 64 && e <= t)
                    c += step;
            }
            const int o = t - __shfl(excl, c);
            const int f = __shfl(first, c);
            const int x = x0 + (swapped ? j_hi - (u0 + c) : j_lo + u0 + c);
            const uint32_t here = (uint32_t)min(64, total - t0);
            n_read += here;
            if (cast_probe(rule, t < total, x, up ? f + o : f - o, lane, stop, stop_lane))
                return stopped();
            n_upto += here;
        }
    }
    return false;
}

__global__ __launch_bounds__(256) void k_cast_walk(CastChunk ch)
{
    __shared__ uint32_t wave_cells[4][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    const int si = prefix_find(ch.pre_group, ch.n_segs, blockIdx.x);        /* uniform */
    const CastSeg& q = ch.segs[si];
    const int local = (int)blockIdx.x - (int)ch.pre_group[si];
    const int p = local / q.groups, first = (local - p * q.groups) * kCastGroup;
    const CastPose pose = ch.poses[q.pose_at + p];
    const size_t ray0 = (size_t)ch.pre_ray[si] + (size_t)p * q.n_beams;

    uint32_t n_read = 0, n_upto = 0;          /* per wavefront (uniform) */
    for (int k = wave; k < kCastGroup; k += 4) {
        const int i = first + k;
        if (i >= q.n_beams)
            break;
        const RayRec rec = ch.recs[ray0 + i];
        CastRecord stop = { 0, 0, 0u, CSM_CAST_NONE, 0ll };
        if (rec.ex != kRayUnusable)
            cast_walk_ray(q, ch, pose.sx, pose.sy, rec.ex, rec.ey, lane, stop, n_read, n_upto);
        if (lane == 0)
            ch.records[ray0 + i] = stop;
    }
    if (lane == 0) {
        wave_cells[wave][0] = n_read;
        wave_cells[wave][1] = n_upto;
    }
    __syncthreads();
    if (tid < 2)
        ch.group_cells[2 * (size_t)blockIdx.x + tid] =
            wave_cells[0][tid] + wave_cells[1][tid] + wave_cells[2][tid] + wave_cells[3][tid];
}

} /* namespace csm */
