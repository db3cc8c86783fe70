/* csm_distance_api.hip -- distance fields (csm_distance_transform, csm_build_distance_map,
 * csm_build_distance_maps of include/csm_hip.h) with their kernels (csm_distance_kernels.hip), and the host
 * restatements csm_host_distance_kernel / csm_host_distance_transform / csm_host_distance_map, which
 * csm_distance_host.hpp defines. A translation unit of libcsm_hip.so of its own.
 *
 * A build call checks everything and allocates every new base level first (the field helpers of
 * csm_internal.hpp, shared with csm_likelihood_api.hip), uploads one block ([table][one job per map][two
 * counters per map], from dt_pin into dt_tab), runs the two passes over chunks of maps whose offsets fit
 * CSM_DISTANCE_SCRATCH_LIMIT (dt_work), reads the counters back and only then replaces the destination
 * grids: a call that is refused or fails has changed nothing. */
#include "csm_internal.hpp"
#include "csm_distance_host.hpp"

#include "csm_distance_kernels.hip"

static_assert(kDtFar == CSM_DISTANCE_NONE, "the kernel's empty key is the header's constant");

namespace {

constexpr int kDtMaxSide = csm_distance_host::kMaxSide;
constexpr size_t kDtTableBytes =
    align256((size_t)(CSM_DISTANCE_MAX_RADIUS * CSM_DISTANCE_MAX_RADIUS + 1) * 2);
using csm_distance_host::shape_ok;

/* the launch chain of the maps jobs[0 .. n) (device copies; the host's in `host`), which share ctx->dt_work */
template <bool kTransform>
int run_passes(csm_ctx* ctx, const DtJob* jobs_dev, const DtJob* host, int n, DtParams dp)
{
    int rows_max = 0, cols_max = 0;
    for (int i = 0; i < n; ++i) {
        rows_max = std::max(rows_max, host[i].rows);
        cols_max = std::max(cols_max, host[i].cols);
    }
    dp.per_pass = cols_max <= kDtWide ? 4 : 1;
    dp.lds_cols = (cols_max + 7) & ~7;
    const size_t lds = (size_t)kDtHead + (size_t)dp.per_pass * dp.lds_cols * 2;
    for (int first = 0; first < n; first += 65535) {      /* grid.z limit */
        const unsigned nz = (unsigned)std::min(65535, n - first);
        {
            ScopedTimer tm(ctx, "distance_columns");
            const int e = launch(k_distance_columns, dim3(ceil_div(cols_max, 64), 1, nz), dim3(64), ctx->stream,
                                 jobs_dev + first, dp);
            if (int rc = launched_ok(ctx, e, "distance field (columns)"))
                return rc;
        }
        ScopedTimer tm(ctx, "distance_rows");
        const int e = launch_lds(ctx->device, k_distance_rows<kTransform>, dim3(1, ceil_div(rows_max, kDtRun), nz),
                                 dim3(256), lds, ctx->stream, jobs_dev + first, dp);
        if (int rc = launched_ok(ctx, e, "distance field (rows)"))
            return rc;
    }
    return CSM_OK;
}

size_t offsets_bytes(const DeviceGrid& s) { return align256((size_t)s.rows * s.cols * 2); }

} /* namespace */

extern "C" {

int csm_distance_transform(csm_ctx* ctx, uint64_t map_id, uint32_t occupied_min, uint32_t* d2, uint32_t* nearest)
{
    if (!ctx || occupied_min < 1 || (!d2 && !nearest))
        return fail(ctx, CSM_EINVAL, "csm_distance_transform: occupied_min >= 1 and at least one output");
    const DeviceGrid* s = find_grid(ctx, map_id);
    if (!s || s->levels.empty())
        return fail(ctx, CSM_ENOENT, "map %llu not resident", (unsigned long long)map_id);
    if (!shape_ok(s->rows, s->cols))
        return fail(ctx, CSM_EINVAL, "distance transform: at most %d rows and columns", kDtMaxSide);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t cells = (size_t)s->rows * s->cols;
    Carve w;
    const size_t off_at = w.take(cells * 2), d2_at = w.take(d2 ? cells * 4 : 0),
                 near_at = w.take(nearest ? cells * 4 : 0);
    if (int rc = reserve(ctx, ctx->dt_work, w.off))
        return rc;
    if (int rc = reserve(ctx, ctx->dt_tab, sizeof(DtJob)))
        return rc;
    if (int rc = reserve(ctx, ctx->dt_pin, sizeof(DtJob)))
        return rc;
    char* const work = ctx->dt_work.as<char>();
    DtJob& J = *ctx->dt_pin.as<DtJob>();
    J = DtJob {};
    J.src = s->levels[0].cells;
    J.off = reinterpret_cast<int16_t*>(work + off_at);
    J.d2 = d2 ? reinterpret_cast<uint32_t*>(work + d2_at) : nullptr;
    J.nearest = nearest ? reinterpret_cast<uint32_t*>(work + near_at) : nullptr;
    J.rows = s->rows;
    J.cols = s->cols;
    J.pitch = s->pitch;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->dt_tab.p, &J, sizeof(DtJob), hipMemcpyHostToDevice, ctx->stream));
    DtParams dp {};
    dp.radius = 1;
    dp.occupied_min = occupied_min;
    if (int rc = run_passes<true>(ctx, ctx->dt_tab.as<DtJob>(), &J, 1, dp))
        return rc;
    if (d2)
        HIP_TRY(ctx, hipMemcpyAsync(d2, J.d2, cells * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (nearest)
        HIP_TRY(ctx, hipMemcpyAsync(nearest, J.nearest, cells * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CSM_OK;
}

int csm_build_distance_maps(csm_ctx* ctx, const uint64_t* src_ids, const uint64_t* dst_ids, int32_t n,
                            const csm_distance_params* prm)
{
    if (!ctx || !src_ids || !dst_ids || n < 1)
        return fail(ctx, CSM_EINVAL, "csm_build_distance_maps: bad arguments");
    if (!csm_distance_host::params_ok(prm))
        return fail(ctx, CSM_EINVAL,
                    "distance field: radius must be 1..%d, occupied_min >= 1 and every table entry <= 65534",
                    CSM_DISTANCE_MAX_RADIUS);
    if (int rc = field_ids_ok(ctx, "distance field", src_ids, dst_ids, n))
        return rc;
    for (int i = 0; i < n; ++i) {
        const DeviceGrid& s = *find_grid(ctx, src_ids[i]);
        if (!shape_ok(s.rows, s.cols))
            return fail(ctx, CSM_EINVAL, "distance field: map %llu has more than %d rows or columns",
                        (unsigned long long)src_ids[i], kDtMaxSide);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    /* the new base levels, owned here until every one of them is built */
    std::vector<Level> bases;
    if (int rc = alloc_field_bases(ctx, src_ids, n, bases))
        return rc;

    /* chunks of maps whose offsets fit the limit (a map beyond it goes alone); dt_work holds the largest */
    std::vector<int> chunk_first { 0 };
    size_t work_bytes = 0, in_chunk = 0;
    for (int i = 0; i < n; ++i) {
        const size_t b = offsets_bytes(*find_grid(ctx, src_ids[i]));
        if (in_chunk != 0 && in_chunk + b > (size_t)CSM_DISTANCE_SCRATCH_LIMIT) {
            chunk_first.push_back(i);
            in_chunk = 0;
        }
        in_chunk += b;
        work_bytes = std::max(work_bytes, in_chunk);
    }
    chunk_first.push_back(n);
    if (int rc = reserve(ctx, ctx->dt_work, work_bytes))
        return rc;

    /* [table][jobs][counters]: one upload */
    Carve c;
    c.take(kDtTableBytes);
    const size_t jobs_at = c.take((size_t)n * sizeof(DtJob)), known_at = c.off, block = known_at + (size_t)n * 8;
    if (int rc = reserve(ctx, ctx->dt_tab, block))
        return rc;
    if (int rc = reserve(ctx, ctx->dt_pin, block))
        return rc;
    char* const pin = ctx->dt_pin.as<char>();
    char* const dev = ctx->dt_tab.as<char>();
    std::memcpy(pin, prm->table, (size_t)(prm->radius * prm->radius + 1) * 2);
    DtJob* const jobs_pin = reinterpret_cast<DtJob*>(pin + jobs_at);
    int32_t* const known_pin = reinterpret_cast<int32_t*>(pin + known_at);
    int32_t* const known_dev = reinterpret_cast<int32_t*>(dev + known_at);
    for (size_t k = 0; k + 1 < chunk_first.size(); ++k) {
        size_t at = 0;
        for (int i = chunk_first[k]; i < chunk_first[k + 1]; ++i) {
            const DeviceGrid& s = *find_grid(ctx, src_ids[i]);
            DtJob& J = jobs_pin[i];
            J = DtJob {};
            J.src = s.levels[0].cells;
            J.off = reinterpret_cast<int16_t*>(ctx->dt_work.as<char>() + at);
            J.dst = bases[i].cells;
            J.known = known_dev + 2 * i;
            J.rows = s.rows;
            J.cols = s.cols;
            J.pitch = s.pitch;
            known_pin[2 * i] = s.rows;          /* "no known cell": what csm_upload_grid reports */
            known_pin[2 * i + 1] = s.cols;
            at += offsets_bytes(s);
        }
    }
    HIP_TRY(ctx, hipMemcpyAsync(dev, pin, block, hipMemcpyHostToDevice, ctx->stream));
    DtParams dp {};
    dp.table = reinterpret_cast<const uint16_t*>(dev);
    dp.radius = prm->radius;
    dp.occupied_min = prm->occupied_min;
    dp.keep_unknown = prm->keep_unknown ? 1 : 0;
    const DtJob* const jobs_dev = reinterpret_cast<const DtJob*>(dev + jobs_at);
    for (size_t k = 0; k + 1 < chunk_first.size(); ++k)     /* in stream order: a chunk reuses the last one's offsets */
        if (int rc = run_passes<false>(ctx, jobs_dev + chunk_first[k], jobs_pin + chunk_first[k],
                                       chunk_first[k + 1] - chunk_first[k], dp))
            return rc;
    HIP_TRY(ctx, hipMemcpyAsync(known_pin, known_dev, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    /* also: nothing queued reads an old destination any more */
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    register_fields(ctx, src_ids, dst_ids, n, bases, known_pin);
    return CSM_OK;
}

int csm_build_distance_map(csm_ctx* ctx, uint64_t src_map_id, uint64_t dst_map_id, const csm_distance_params* prm)
{
    return csm_build_distance_maps(ctx, &src_map_id, &dst_map_id, 1, prm);
}

} /* extern "C" */
