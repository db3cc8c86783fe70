/* csm_likelihood_api.hip -- likelihood-field maps (csm_build_likelihood_map, csm_build_likelihood_maps and
 * the host restatements csm_host_likelihood_radius / csm_host_likelihood_kernel / csm_host_likelihood_map of
 * include/csm_hip.h), with their kernel (csm_likelihood_kernels.hip). A translation unit of libcsm_hip.so
 * of its own.
 *
 * A build call checks everything and allocates every new base level first, uploads one block ([table][one
 * job per map][two counters per map], from lf_pin into lf_tab), launches k_likelihood_batch over all maps,
 * reads the counters back and only then replaces the destination grids (register_fields): a call that is
 * refused or fails has changed nothing. The id checks, the new base levels and the registration are the
 * field helpers of csm_internal.hpp, shared with csm_distance_api.hip. */
#include "csm_internal.hpp"

#include "csm_likelihood_kernels.hip"

static_assert(kLfMaxR == CSM_LIKELIHOOD_MAX_RADIUS, "the kernel's LDS tile is sized for the largest radius");

namespace {

constexpr size_t kLfTableBytes = align256((size_t)(kLfMaxR * kLfMaxR + 1) * 4);

bool likelihood_params_ok(const csm_likelihood_params* p)
{
    if (!p || !p->kernel || p->radius < 1 || p->radius > CSM_LIKELIHOOD_MAX_RADIUS || p->occupied_min < 1)
        return false;
    for (int i = 0; i <= p->radius * p->radius; ++i)
        if (p->kernel[i] > 32768u)
            return false;
    return true;
}

bool sigma_ok(double sigma, double resolution)
{
    return std::isfinite(sigma) && std::isfinite(resolution) && sigma > 0.0 && resolution > 0.0;
}

} /* namespace */

extern "C" {

int csm_host_likelihood_radius(double sigma, double resolution)
{
    if (!sigma_ok(sigma, resolution))
        return CSM_EINVAL;
    const double r = std::ceil(3.0 * (sigma / resolution));
    return r < 1.0 ? 1 : r > (double)CSM_LIKELIHOOD_MAX_RADIUS ? CSM_LIKELIHOOD_MAX_RADIUS : (int)r;
}

int csm_host_likelihood_kernel(double sigma, double resolution, int32_t radius, uint32_t* table)
{
    if (!sigma_ok(sigma, resolution) || radius < 1 || radius > CSM_LIKELIHOOD_MAX_RADIUS || !table)
        return CSM_EINVAL;
    for (int d2 = 0; d2 <= radius * radius; ++d2)
        table[d2] = (uint32_t)std::floor(
            32768.0 * std::exp(-((double)d2 * (resolution * resolution)) / (2.0 * (sigma * sigma))) + 0.5);
    return CSM_OK;
}

int csm_host_likelihood_map(const uint16_t* grid, int32_t rows, int32_t cols, const csm_likelihood_params* prm,
                            uint16_t* out)
{
    if (!grid || !out || rows < 1 || cols < 1 || !likelihood_params_ok(prm))
        return CSM_EINVAL;
    const int R = prm->radius;
    std::memcpy(out, grid, (size_t)rows * cols * 2);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            const uint32_t v = grid[(size_t)r * cols + c];
            if (v < prm->occupied_min)
                continue;
            /* the obstacle (r, c) raises every cell of its disc */
            for (int dr = -R; dr <= R; ++dr)
                for (int dc = -R; dc <= R; ++dc) {
                    const int d2 = dr * dr + dc * dc, rr = r + dr, cc = c + dc;
                    if (d2 > R * R || rr < 0 || rr >= rows || cc < 0 || cc >= cols)
                        continue;
                    const size_t at = (size_t)rr * cols + cc;
                    if (prm->keep_unknown && grid[at] == 0)
                        continue;
                    const uint32_t s = 1u + (((v - 1u) * prm->kernel[d2]) >> 15);
                    if (s > out[at])
                        out[at] = (uint16_t)s;
                }
        }
    return CSM_OK;
}

int csm_build_likelihood_maps(csm_ctx* ctx, const uint64_t* src_ids, const uint64_t* dst_ids, int32_t n,
                              const csm_likelihood_params* prm)
{
    if (!ctx || !src_ids || !dst_ids || n < 1)
        return fail(ctx, CSM_EINVAL, "csm_build_likelihood_maps: bad arguments");
    if (!likelihood_params_ok(prm))
        return fail(ctx, CSM_EINVAL,
                    "likelihood field: radius must be 1..%d, occupied_min >= 1 and every table entry <= 32768",
                    CSM_LIKELIHOOD_MAX_RADIUS);
    if (int rc = field_ids_ok(ctx, "likelihood field", src_ids, dst_ids, n))
        return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    /* the new base levels, owned here until every one of them is built */
    std::vector<Level> bases;
    if (int rc = alloc_field_bases(ctx, src_ids, n, bases))
        return rc;

    /* [table][jobs][counters]: one upload */
    Carve c;
    c.take(kLfTableBytes);
    const size_t jobs_at = c.take((size_t)n * sizeof(LfJob)), known_at = c.off, block = known_at + (size_t)n * 8;
    if (int rc = reserve(ctx, ctx->lf_tab, block))
        return rc;
    if (int rc = reserve(ctx, ctx->lf_pin, block))
        return rc;
    char* const pin = ctx->lf_pin.as<char>();
    char* const dev = ctx->lf_tab.as<char>();
    std::memset(pin, 0, kLfTableBytes);
    std::memcpy(pin, prm->kernel, (size_t)(prm->radius * prm->radius + 1) * 4);
    LfJob* const jobs_pin = reinterpret_cast<LfJob*>(pin + jobs_at);
    int32_t* const known_pin = reinterpret_cast<int32_t*>(pin + known_at);
    int32_t* const known_dev = reinterpret_cast<int32_t*>(dev + known_at);
    int rows_max = 0, pitch_max = 0;
    for (int i = 0; i < n; ++i) {
        const DeviceGrid& s = *find_grid(ctx, src_ids[i]);
        LfJob& J = jobs_pin[i];
        J.src = s.levels[0].cells;
        J.dst = bases[i].cells;
        J.known = known_dev + 2 * i;
        J.rows = s.rows;
        J.cols = s.cols;
        J.pitch = s.pitch;
        J.pad = 0;
        known_pin[2 * i] = s.rows;          /* "no known cell": what csm_upload_grid reports */
        known_pin[2 * i + 1] = s.cols;
        rows_max = std::max(rows_max, s.rows);
        pitch_max = std::max(pitch_max, s.pitch);
    }
    HIP_TRY(ctx, hipMemcpyAsync(dev, pin, block, hipMemcpyHostToDevice, ctx->stream));
    LfParams lp;
    lp.kernel = reinterpret_cast<const uint32_t*>(dev);
    lp.radius = prm->radius;
    lp.occupied_min = prm->occupied_min;
    lp.keep_unknown = prm->keep_unknown ? 1 : 0;
    lp.pad = 0;
    {
        ScopedTimer tm(ctx, "likelihood");
        const LfJob* const jobs_dev = reinterpret_cast<const LfJob*>(dev + jobs_at);
        for (int first = 0; first < n; first += 65535) {      /* grid.z limit */
            const unsigned nz = (unsigned)std::min(65535, n - first);
            const int e = launch(k_likelihood_batch, dim3(ceil_div(pitch_max, kLfTC), ceil_div(rows_max, kLfTR), nz),
                                 dim3(256), ctx->stream, jobs_dev + first, lp);
            if (int rc = launched_ok(ctx, e, "likelihood field"))
                return rc;
        }
    }
    HIP_TRY(ctx, hipMemcpyAsync(known_pin, known_dev, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    /* also: nothing queued reads an old destination any more */
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

    register_fields(ctx, src_ids, dst_ids, n, bases, known_pin);
    return CSM_OK;
}

int csm_build_likelihood_map(csm_ctx* ctx, uint64_t src_map_id, uint64_t dst_map_id,
                             const csm_likelihood_params* prm)
{
    return csm_build_likelihood_maps(ctx, &src_map_id, &dst_map_id, 1, prm);
}

} /* extern "C" */
