/* csm_loopsearch_api.hip -- the candidate pairs of a pose graph: csm_loop_search and the host functions
 * csm_host_loop_search (its CPU reference), csm_host_travel_distances and csm_host_loop_candidates_nearest
 * (include/csm_hip.h), with the kernel (csm_loopsearch_kernels.hip). A translation unit of libcsm_hip.so of
 * its own.
 *
 * A call is checked first (a refused call has run nothing). Then one upload ([x | y | travel | query travel |
 * map | query index], from ls_pin into ls_dev), k_loop_search over the queries, one read-back of [records |
 * counts | prefix lengths | eligible counts]; the two totals of csm_loop_search_info are summed on the host.
 * Nothing the context keeps between calls is touched but these two workspaces, and nothing in them is read
 * before the call has written it. */
#include "csm_internal.hpp"

#include "csm_loopsearch_kernels.hip"

static_assert(sizeof(csm_loop_candidate) == 24 && offsetof(csm_loop_candidate, dist_sq) == 16,
              "k_loop_search writes whole records; the host compares them byte for byte");

namespace {

/* what is wrong with a call, or null */
const char* loop_search_refusal(const double* poses, const int32_t* map, const double* travel, int32_t n_scan,
                                int32_t n_maps, int32_t n_ref, const int32_t* query_index, const double* query_travel,
                                int32_t n_q, const csm_loop_search_params* p, const csm_loop_candidate* out,
                                const int32_t* counts)
{
    if (!poses || !map || !travel || !query_index || !query_travel || !p || !out || !counts)
        return "a null pointer";
    if (n_scan < 1 || n_scan > CSM_LOOP_SEARCH_MAX_NODES)
        return "n_scan outside 1..CSM_LOOP_SEARCH_MAX_NODES";
    if (n_maps < 1 || n_maps > CSM_LOOP_SEARCH_MAX_MAPS)
        return "n_maps outside 1..CSM_LOOP_SEARCH_MAX_MAPS";
    if (n_ref < 0 || n_ref > n_scan)
        return "n_ref outside [0, n_scan]";
    if (n_q < 1)
        return "n_q < 1";
    if (p->n_per_query < 1 || p->n_per_query > CSM_LOOP_SEARCH_MAX_K)
        return "n_per_query outside 1..CSM_LOOP_SEARCH_MAX_K";
    if (p->one_per_map != 0 && p->one_per_map != 1)
        return "one_per_map is neither 0 nor 1";
    if (!std::isfinite(p->travel_dist_threshold) || !std::isfinite(p->node_dist_threshold))
        return "a threshold that is not finite";
    for (int32_t i = 0; i < n_scan; ++i) {
        if (!std::isfinite(poses[3 * (size_t)i]) || !std::isfinite(poses[3 * (size_t)i + 1]) || !std::isfinite(travel[i]))
            return "a pose coordinate or travel value that is not finite";
        if (map[i] < 0 || map[i] >= n_maps)
            return "a map index outside [0, n_maps)";
        if (i > 0 && (travel[i] < travel[i - 1] || map[i] < map[i - 1]))
            return "travel or scan_map_index decreasing";
    }
    std::vector<bool> seen((size_t)n_scan, false);
    for (int32_t i = 0; i < n_q; ++i) {
        const int32_t q = query_index[i];
        if (q < 0 || q >= n_scan)
            return "a query index out of range";
        if (seen[(size_t)q])
            return "a query index repeated";
        seen[(size_t)q] = true;
        if (!std::isfinite(query_travel[i]))
            return "a query_travel value that is not finite";
    }
    return nullptr;
}

csm_loop_candidate loop_unused(int32_t q)
{
    csm_loop_candidate c;
    std::memset(&c, 0, sizeof(c));
    c.query_scan_index = q;
    c.ref_scan_index = c.ref_map_index = -1;
    return c;
}

} /* namespace */

extern "C" {

int csm_host_travel_distances(const double* scan_poses, int32_t n, double* out)
{
    if (!scan_poses || !out || n < 0)
        return CSM_EINVAL;
    double acc = 0.0;
    for (int32_t i = 0; i < n; ++i) {
        if (i > 0)
            acc += std::hypot(scan_poses[3 * (size_t)(i - 1)] - scan_poses[3 * (size_t)i],
                              scan_poses[3 * (size_t)(i - 1) + 1] - scan_poses[3 * (size_t)i + 1]);
        out[i] = acc;
    }
    return CSM_OK;
}

int csm_host_loop_search(const double* scan_poses, const int32_t* scan_map_index, const double* travel,
                         int32_t n_scan, int32_t n_maps, int32_t n_ref, const int32_t* query_index,
                         const double* query_travel, int32_t n_q, const csm_loop_search_params* prm,
                         csm_loop_candidate* out, int32_t* counts, csm_loop_search_info* info)
{
    if (loop_search_refusal(scan_poses, scan_map_index, travel, n_scan, n_maps, n_ref, query_index, query_travel, n_q,
                            prm, out, counts))
        return CSM_EINVAL;
    const double t2 = std::pow(prm->node_dist_threshold, 2.0);
    const int k = prm->n_per_query;
    int64_t evaluated = 0, eligible = 0;
    std::vector<std::pair<uint64_t, int32_t>> keys;
    std::vector<bool> taken;
    for (int32_t i = 0; i < n_q; ++i) {
        const int32_t q = query_index[i];
        const double qx = scan_poses[3 * (size_t)q], qy = scan_poses[3 * (size_t)q + 1];
        keys.clear();
        for (int32_t r = 0; r < n_ref; ++r) {
            if (query_travel[i] - travel[r] < prm->travel_dist_threshold)
                break;
            ++evaluated;
            if (scan_map_index[r] == scan_map_index[q])
                continue;
            const double dx = scan_poses[3 * (size_t)r] - qx;
            const double dy = scan_poses[3 * (size_t)r + 1] - qy;
            const double xx = dx * dx;
            const double yy = dy * dy;
            const double d2 = xx + yy;
            if (!(d2 < t2))
                continue;
            uint64_t bits;
            std::memcpy(&bits, &d2, 8);
            keys.emplace_back(bits, r);
        }
        eligible += (int64_t)keys.size();
        std::sort(keys.begin(), keys.end());
        if (prm->one_per_map)
            taken.assign((size_t)n_maps, false);
        int used = 0;
        for (const auto& key : keys) {
            if (used == k)
                break;
            const int32_t m = scan_map_index[key.second];
            if (prm->one_per_map) {
                if (taken[(size_t)m])
                    continue;
                taken[(size_t)m] = true;
            }
            csm_loop_candidate c = loop_unused(q);
            c.ref_scan_index = key.second;
            c.ref_map_index = m;
            std::memcpy(&c.dist_sq, &key.first, 8);
            out[(size_t)i * k + used++] = c;
        }
        counts[i] = used;
        for (int s = used; s < k; ++s)
            out[(size_t)i * k + s] = loop_unused(q);
    }
    if (info) {
        info->pairs_evaluated = evaluated;
        info->pairs_eligible = eligible;
    }
    return CSM_OK;
}

int csm_host_loop_candidates_nearest(const csm_loop_candidate* cands, const int32_t* counts, int32_t n_q,
                                     int32_t n_per_query, int32_t n_total, csm_loop_candidate* out, int32_t* n_out)
{
    if (!cands || !counts || !out || !n_out || n_q < 1 || n_per_query < 1 || n_per_query > CSM_LOOP_SEARCH_MAX_K ||
        n_total < 0)
        return CSM_EINVAL;
    std::vector<csm_loop_candidate> all;
    for (int32_t i = 0; i < n_q; ++i) {
        if (counts[i] < 0 || counts[i] > n_per_query)
            return CSM_EINVAL;
        all.insert(all.end(), cands + (size_t)i * n_per_query, cands + (size_t)i * n_per_query + counts[i]);
    }
    std::sort(all.begin(), all.end(), [](const csm_loop_candidate& a, const csm_loop_candidate& b) {
        return std::tie(a.dist_sq, a.ref_scan_index, a.query_scan_index) <
               std::tie(b.dist_sq, b.ref_scan_index, b.query_scan_index);
    });
    const size_t n = std::min(all.size(), (size_t)n_total);
    std::copy(all.begin(), all.begin() + n, out);
    *n_out = (int32_t)n;
    return CSM_OK;
}

int csm_loop_search(csm_ctx* ctx, const double* scan_poses, const int32_t* scan_map_index, const double* travel,
                    int32_t n_scan, int32_t n_maps, int32_t n_ref, const int32_t* query_index,
                    const double* query_travel, int32_t n_q, const csm_loop_search_params* prm,
                    csm_loop_candidate* out, int32_t* counts, csm_loop_search_info* info)
{
    if (!ctx)
        return CSM_EINVAL;
    if (const char* why = loop_search_refusal(scan_poses, scan_map_index, travel, n_scan, n_maps, n_ref, query_index,
                                              query_travel, n_q, prm, out, counts))
        return fail(ctx, CSM_EINVAL, "csm_loop_search: %s", why);
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    const int k = prm->n_per_query;
    const size_t ns = (size_t)n_scan, nq = (size_t)n_q;
    /* up: [x | y | travel | query travel | map | query index]; back: [records | counts | prefix | eligible] */
    Carve up;
    const size_t x_at = up.take(ns * 8), y_at = up.take(ns * 8), t_at = up.take(ns * 8), qt_at = up.take(nq * 8),
                 m_at = up.take(ns * 4), qi_at = up.take(nq * 4);
    Carve back;
    const size_t rec_at = back.take(nq * k * sizeof(csm_loop_candidate)), cnt_at = back.take(nq * 4),
                 pre_at = back.take(nq * 4), eli_at = back.take(nq * 4);
    int rc;
    if ((rc = reserve(ctx, ctx->ls_dev, up.off + back.off))) return rc;
    if ((rc = reserve(ctx, ctx->ls_pin, std::max(up.off, back.off)))) return rc;
    char* const pin = ctx->ls_pin.as<char>();
    char* const dev = ctx->ls_dev.as<char>();
    char* const dev_back = dev + up.off;

    double* const px = reinterpret_cast<double*>(pin + x_at);
    double* const py = reinterpret_cast<double*>(pin + y_at);
    for (size_t i = 0; i < ns; ++i) {
        px[i] = scan_poses[3 * i];
        py[i] = scan_poses[3 * i + 1];
    }
    std::memcpy(pin + t_at, travel, ns * 8);
    std::memcpy(pin + qt_at, query_travel, nq * 8);
    std::memcpy(pin + m_at, scan_map_index, ns * 4);
    std::memcpy(pin + qi_at, query_index, nq * 4);
    HIP_TRY(ctx, hipMemcpyAsync(dev, pin, up.off, hipMemcpyHostToDevice, ctx->stream));

    LoopSearchJob job;
    job.x = reinterpret_cast<const double*>(dev + x_at);
    job.y = reinterpret_cast<const double*>(dev + y_at);
    job.travel = reinterpret_cast<const double*>(dev + t_at);
    job.map = reinterpret_cast<const int32_t*>(dev + m_at);
    job.query_index = reinterpret_cast<const int32_t*>(dev + qi_at);
    job.query_travel = reinterpret_cast<const double*>(dev + qt_at);
    job.out = reinterpret_cast<csm_loop_candidate*>(dev_back + rec_at);
    job.counts = reinterpret_cast<int32_t*>(dev_back + cnt_at);
    job.prefix = reinterpret_cast<int32_t*>(dev_back + pre_at);
    job.eligible = reinterpret_cast<int32_t*>(dev_back + eli_at);
    job.travel_threshold = prm->travel_dist_threshold;
    job.t2 = std::pow(prm->node_dist_threshold, 2.0);
    job.n_ref = n_ref;
    job.n_maps = n_maps;
    job.k = k;
    job.one_per_map = prm->one_per_map;
    int e;
    {
        ScopedTimer tm(ctx, "loop_search");
        e = launch(k_loop_search, dim3((unsigned)n_q), dim3(kLoopBlock), ctx->stream, job);
    }
    if ((rc = launched_ok(ctx, e, "loop search"))) return rc;
    /* the upload has been read by the time the kernel has run: the pinned block is free for the way back */
    HIP_TRY(ctx, hipMemcpyAsync(pin, dev_back, back.off, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(out, pin + rec_at, nq * k * sizeof(csm_loop_candidate));
    std::memcpy(counts, pin + cnt_at, nq * 4);
    if (info) {
        const int32_t* const pre = reinterpret_cast<const int32_t*>(pin + pre_at);
        const int32_t* const eli = reinterpret_cast<const int32_t*>(pin + eli_at);
        info->pairs_evaluated = info->pairs_eligible = 0;
        for (size_t i = 0; i < nq; ++i) {
            info->pairs_evaluated += pre[i];
            info->pairs_eligible += eli[i];
        }
    }
    return CSM_OK;
}

} /* extern "C" */
