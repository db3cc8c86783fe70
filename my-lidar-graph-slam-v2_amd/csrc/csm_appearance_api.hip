/* csm_appearance_api.hip -- scan descriptors and the loop search by appearance: csm_scan_descriptors and
 * csm_appearance_search with their CPU references csm_host_scan_descriptors and csm_host_appearance_search, and
 * csm_host_descriptor_shift_angle (include/csm_hip.h), with the kernels (csm_appearance_kernels.hip). A
 * translation unit of libcsm_hip.so of its own.
 *
 * A call is checked first (a refused call has run nothing). csm_scan_descriptors: one upload ([ring edges |
 * sector edges | offsets | angles | ranges], from ap_pin into ap_dev), k_scan_descriptors over the scans, one
 * read-back of [descriptors | beams used]. csm_appearance_search: one upload ([descriptors | travel | query
 * travel | map | query index]), k_appearance_ring_sums, then per chunk of queries k_appearance_pairs into the
 * pair table (ap_table, at most CSM_APPEARANCE_TABLE_BYTES unless one query's row alone is larger) and
 * k_appearance_select; one read-back of [records | counts | prefix lengths | eligible counts]; the two totals
 * of csm_loop_search_info are summed on the host. Nothing the context keeps between calls is touched but these
 * three workspaces, and nothing in them is read before the call has written it. */
#include "csm_internal.hpp"

#include "csm_appearance_kernels.hip"

static_assert(sizeof(csm_appearance_candidate) == 24 && offsetof(csm_appearance_candidate, distance) == 16,
              "k_appearance_select writes whole records; the host compares them byte for byte");

namespace {

const char* descriptor_refusal(const csm_descriptor_params* p)
{
    if (p->n_rings < 1 || p->n_rings > CSM_DESCRIPTOR_MAX_RINGS)
        return "n_rings outside 1..CSM_DESCRIPTOR_MAX_RINGS";
    if (p->n_sectors < 4 || p->n_sectors > CSM_DESCRIPTOR_MAX_SECTORS || p->n_sectors % 4 != 0)
        return "n_sectors is no multiple of 4 in 4..CSM_DESCRIPTOR_MAX_SECTORS";
    if (!std::isfinite(p->range_min) || !std::isfinite(p->range_max) || !(p->range_min < p->range_max))
        return "range_min and range_max must be finite with range_min < range_max";
    return nullptr;
}

/* the edge tables, by the expressions of the header */
void descriptor_edges(const csm_descriptor_params* p, double* ring_edge, double* sector_edge)
{
    for (int k = 0; k <= p->n_rings; ++k)
        ring_edge[k] = p->range_min + ((p->range_max - p->range_min) * k) / p->n_rings;
    ring_edge[p->n_rings] = p->range_max;
    for (int k = 0; k <= p->n_sectors; ++k)
        sector_edge[k] = -M_PI + (2.0 * M_PI * k) / p->n_sectors;
    sector_edge[p->n_sectors] = M_PI;
}

const char* scans_refusal(const double* angles, const double* ranges, const int32_t* offsets, int32_t n_scans,
                          const csm_descriptor_params* p, const uint8_t* out, const int32_t* beams_used)
{
    if (!angles || !ranges || !offsets || !p || !out || !beams_used)
        return "a null pointer";
    if (n_scans < 1 || n_scans > CSM_LOOP_SEARCH_MAX_NODES)
        return "n_scans outside 1..CSM_LOOP_SEARCH_MAX_NODES";
    if (const char* why = descriptor_refusal(p))
        return why;
    if (offsets[0] != 0)
        return "offsets[0] is not 0";
    for (int32_t i = 0; i < n_scans; ++i) {
        if (offsets[i + 1] < offsets[i])
            return "offsets decreasing";
        if (offsets[i + 1] - offsets[i] > CSM_DESCRIPTOR_MAX_BEAMS)
            return "a scan of more than CSM_DESCRIPTOR_MAX_BEAMS beams";
    }
    return nullptr;
}

const char* appearance_refusal(const uint8_t* desc, const int32_t* map, const double* travel, int32_t n_scan,
                               int32_t n_maps, int32_t n_ref, const int32_t* query_index, const double* query_travel,
                               int32_t n_q, const csm_appearance_params* p, const csm_appearance_candidate* out,
                               const int32_t* counts)
{
    if (!desc || !map || !travel || !query_index || !query_travel || !p || !out || !counts)
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
    if (!std::isfinite(p->travel_dist_threshold))
        return "a threshold that is not finite";
    if (const char* why = descriptor_refusal(&p->descriptor))
        return why;
    if ((int64_t)n_scan * p->descriptor.n_rings * p->descriptor.n_sectors > ((int64_t)1 << 30))
        return "n_scan * n_rings * n_sectors above 2^30";
    for (int32_t i = 0; i < n_scan; ++i) {
        if (!std::isfinite(travel[i]))
            return "a travel value that is not finite";
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

csm_appearance_candidate appearance_unused(int32_t q)
{
    csm_appearance_candidate c;
    std::memset(&c, 0, sizeof(c));
    c.query_scan_index = q;
    c.ref_scan_index = c.ref_map_index = -1;
    return c;
}

inline uint32_t abs_diff(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }

/* sum of |a[i] - b[i]| over n bytes */
inline uint32_t l1_bytes(const uint8_t* a, const uint8_t* b, int n)
{
    uint32_t acc = 0;
    for (int i = 0; i < n; ++i)
        acc += (uint32_t)std::abs((int)a[i] - (int)b[i]);
    return acc;
}

} /* namespace */

extern "C" {

int csm_host_scan_descriptors(const double* angles, const double* ranges, const int32_t* offsets, int32_t n_scans,
                              const csm_descriptor_params* prm, uint8_t* out, int32_t* beams_used)
{
    if (scans_refusal(angles, ranges, offsets, n_scans, prm, out, beams_used))
        return CSM_EINVAL;
    double ring_edge[CSM_DESCRIPTOR_MAX_RINGS + 1], sector_edge[CSM_DESCRIPTOR_MAX_SECTORS + 1];
    descriptor_edges(prm, ring_edge, sector_edge);
    const int nr = prm->n_rings, ns = prm->n_sectors, cells = nr * ns;
    std::vector<uint32_t> hist((size_t)cells);
    for (int32_t i = 0; i < n_scans; ++i) {
        std::fill(hist.begin(), hist.end(), 0u);
        int32_t used = 0;
        for (int32_t b = offsets[i]; b < offsets[i + 1]; ++b) {
            const double a = angles[b], r = ranges[b];
            if (!ap_finite(a) || !ap_finite(r))
                continue;
            if (!(ring_edge[0] <= r && r < ring_edge[nr]) || !(sector_edge[0] <= a && a < sector_edge[ns]))
                continue;
            ++hist[(size_t)ap_greatest_le(ring_edge, nr, r) * ns + ap_greatest_le(sector_edge, ns, a)];
            ++used;
        }
        for (int c = 0; c < cells; ++c)
            out[(size_t)i * cells + c] = (uint8_t)std::min(hist[(size_t)c], 255u);
        beams_used[i] = used;
    }
    return CSM_OK;
}

int csm_host_descriptor_shift_angle(int32_t shift, int32_t n_sectors, double* out)
{
    if (!out || n_sectors < 4 || n_sectors > CSM_DESCRIPTOR_MAX_SECTORS || n_sectors % 4 != 0 || shift < 0 ||
        shift >= n_sectors)
        return CSM_EINVAL;
    double t = std::fmod((-(double)shift * (2.0 * M_PI)) / (double)n_sectors, 2.0 * M_PI);
    if (t > M_PI)
        t -= 2.0 * M_PI;
    else if (t < -M_PI)
        t += 2.0 * M_PI;
    *out = t;
    return CSM_OK;
}

int csm_host_appearance_search(const uint8_t* descriptors, const int32_t* scan_map_index, const double* travel,
                               int32_t n_scan, int32_t n_maps, int32_t n_ref, const int32_t* query_index,
                               const double* query_travel, int32_t n_q, const csm_appearance_params* prm,
                               csm_appearance_candidate* out, int32_t* counts, csm_loop_search_info* info)
{
    if (appearance_refusal(descriptors, scan_map_index, travel, n_scan, n_maps, n_ref, query_index, query_travel, n_q,
                           prm, out, counts))
        return CSM_EINVAL;
    const int nr = prm->descriptor.n_rings, ns = prm->descriptor.n_sectors, cells = nr * ns;
    const int k = prm->n_per_query;
    std::vector<uint32_t> ring_sum((size_t)n_scan * nr), total((size_t)n_scan, 0u);
    for (size_t i = 0; i < (size_t)n_scan * nr; ++i) {
        uint32_t acc = 0;
        for (int s = 0; s < ns; ++s)
            acc += descriptors[i * ns + s];
        ring_sum[i] = acc;
        total[i / nr] += acc;
    }
    struct Pair {
        uint64_t key;               /* distance << 32 | r */
        int32_t shift;
        uint32_t ring_distance;
        bool operator<(const Pair& o) const { return key < o.key; }
    };
    int64_t evaluated = 0, eligible = 0;
    std::vector<Pair> pairs;
    std::vector<bool> taken;
    std::vector<uint8_t> q2((size_t)nr * 2 * ns);
    for (int32_t i = 0; i < n_q; ++i) {
        const int32_t q = query_index[i];
        /* the query with its sector axis doubled: Q[ring][(sec + s) mod S] is q2[ring][sec + s] */
        for (int g = 0; g < nr; ++g) {
            std::memcpy(&q2[(size_t)g * 2 * ns], descriptors + (size_t)q * cells + g * ns, (size_t)ns);
            std::memcpy(&q2[(size_t)g * 2 * ns + ns], descriptors + (size_t)q * cells + g * ns, (size_t)ns);
        }
        pairs.clear();
        for (int32_t r = 0; r < n_ref; ++r) {
            if (query_travel[i] - travel[r] < prm->travel_dist_threshold)
                break;
            ++evaluated;
            if (scan_map_index[r] == scan_map_index[q] || total[(size_t)q] < prm->min_cell_sum ||
                total[(size_t)r] < prm->min_cell_sum)
                continue;
            uint32_t ring_distance = 0;
            for (int g = 0; g < nr; ++g)
                ring_distance += abs_diff(ring_sum[(size_t)q * nr + g], ring_sum[(size_t)r * nr + g]);
            if (ring_distance > prm->max_distance)
                continue;           /* distance >= ring_distance: not eligible at any shift */
            const uint8_t* const rd = descriptors + (size_t)r * cells;
            uint32_t distance = 0;
            int32_t shift = 0;
            for (int s = 0; s < ns; ++s) {
                uint32_t l1 = 0;
                for (int g = 0; g < nr; ++g)
                    l1 += l1_bytes(&q2[(size_t)g * 2 * ns + s], rd + g * ns, ns);
                if (s == 0 || l1 < distance) {
                    distance = l1;
                    shift = s;
                }
            }
            if (distance > prm->max_distance)
                continue;
            pairs.push_back({ ((uint64_t)distance << 32) | (uint32_t)r, shift, ring_distance });
        }
        eligible += (int64_t)pairs.size();
        std::sort(pairs.begin(), pairs.end());
        if (prm->one_per_map)
            taken.assign((size_t)n_maps, false);
        int used = 0;
        for (const Pair& pr : pairs) {
            if (used == k)
                break;
            const int32_t r = (int32_t)(uint32_t)pr.key;
            const int32_t m = scan_map_index[r];
            if (prm->one_per_map) {
                if (taken[(size_t)m])
                    continue;
                taken[(size_t)m] = true;
            }
            csm_appearance_candidate c = appearance_unused(q);
            c.ref_scan_index = r;
            c.ref_map_index = m;
            c.shift = pr.shift;
            c.distance = (uint32_t)(pr.key >> 32);
            c.ring_distance = pr.ring_distance;
            out[(size_t)i * k + used++] = c;
        }
        counts[i] = used;
        for (int s = used; s < k; ++s)
            out[(size_t)i * k + s] = appearance_unused(q);
    }
    if (info) {
        info->pairs_evaluated = evaluated;
        info->pairs_eligible = eligible;
    }
    return CSM_OK;
}

int csm_scan_descriptors(csm_ctx* ctx, const double* angles, const double* ranges, const int32_t* offsets,
                         int32_t n_scans, const csm_descriptor_params* prm, uint8_t* out, int32_t* beams_used)
{
    if (!ctx)
        return CSM_EINVAL;
    if (const char* why = scans_refusal(angles, ranges, offsets, n_scans, prm, out, beams_used))
        return fail(ctx, CSM_EINVAL, "csm_scan_descriptors: %s", why);
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    const size_t n = (size_t)n_scans, beams = (size_t)offsets[n_scans];
    const size_t cells = (size_t)prm->n_rings * prm->n_sectors;
    /* up: [ring edges | sector edges | offsets | angles | ranges]; back: [descriptors | beams used] */
    Carve up;
    const size_t re_at = up.take((CSM_DESCRIPTOR_MAX_RINGS + 1) * 8), se_at = up.take((CSM_DESCRIPTOR_MAX_SECTORS + 1) * 8),
                 of_at = up.take((n + 1) * 4), an_at = up.take(beams * 8), rg_at = up.take(beams * 8);
    Carve back;
    const size_t de_at = back.take(n * cells), bu_at = back.take(n * 4);
    int rc;
    if ((rc = reserve(ctx, ctx->ap_dev, up.off + back.off))) return rc;
    if ((rc = reserve(ctx, ctx->ap_pin, std::max(up.off, back.off)))) return rc;
    char* const pin = ctx->ap_pin.as<char>();
    char* const dev = ctx->ap_dev.as<char>();
    char* const dev_back = dev + up.off;

    descriptor_edges(prm, reinterpret_cast<double*>(pin + re_at), reinterpret_cast<double*>(pin + se_at));
    std::memcpy(pin + of_at, offsets, (n + 1) * 4);
    std::memcpy(pin + an_at, angles, beams * 8);
    std::memcpy(pin + rg_at, ranges, beams * 8);
    HIP_TRY(ctx, hipMemcpyAsync(dev, pin, up.off, hipMemcpyHostToDevice, ctx->stream));

    DescriptorJob job;
    job.ring_edge = reinterpret_cast<const double*>(dev + re_at);
    job.sector_edge = reinterpret_cast<const double*>(dev + se_at);
    job.offsets = reinterpret_cast<const int32_t*>(dev + of_at);
    job.angles = reinterpret_cast<const double*>(dev + an_at);
    job.ranges = reinterpret_cast<const double*>(dev + rg_at);
    job.out = reinterpret_cast<uint8_t*>(dev_back + de_at);
    job.beams_used = reinterpret_cast<int32_t*>(dev_back + bu_at);
    job.n_rings = prm->n_rings;
    job.n_sectors = prm->n_sectors;
    int e;
    {
        ScopedTimer tm(ctx, "scan_descriptors");
        e = launch(k_scan_descriptors, dim3((unsigned)n_scans), dim3(kApBlock), ctx->stream, job);
    }
    if ((rc = launched_ok(ctx, e, "scan descriptor"))) return rc;
    /* the upload has been read by the time the kernel has run: the pinned block is free for the way back */
    HIP_TRY(ctx, hipMemcpyAsync(pin, dev_back, back.off, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(out, pin + de_at, n * cells);
    std::memcpy(beams_used, pin + bu_at, n * 4);
    return CSM_OK;
}

int csm_appearance_search(csm_ctx* ctx, const uint8_t* descriptors, const int32_t* scan_map_index,
                          const double* travel, int32_t n_scan, int32_t n_maps, int32_t n_ref,
                          const int32_t* query_index, const double* query_travel, int32_t n_q,
                          const csm_appearance_params* prm, csm_appearance_candidate* out, int32_t* counts,
                          csm_loop_search_info* info)
{
    if (!ctx)
        return CSM_EINVAL;
    if (const char* why = appearance_refusal(descriptors, scan_map_index, travel, n_scan, n_maps, n_ref, query_index,
                                             query_travel, n_q, prm, out, counts))
        return fail(ctx, CSM_EINVAL, "csm_appearance_search: %s", why);
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    const int k = prm->n_per_query, nr = prm->descriptor.n_rings, ns = prm->descriptor.n_sectors;
    const size_t n = (size_t)n_scan, nq = (size_t)n_q, cells = (size_t)nr * ns;
    /* up: [descriptors | travel | query travel | map | query index]; then the ring sums; back: [records |
     * counts | prefix | eligible] */
    Carve up;
    const size_t d_at = up.take(n * cells), t_at = up.take(n * 8), qt_at = up.take(nq * 8), m_at = up.take(n * 4),
                 qi_at = up.take(nq * 4);
    Carve work;
    const size_t rs_at = work.take(n * nr * 2);
    Carve back;
    const size_t rec_at = back.take(nq * k * sizeof(csm_appearance_candidate)), cnt_at = back.take(nq * 4),
                 pre_at = back.take(nq * 4), eli_at = back.take(nq * 4);
    /* queries per chunk: the pair table's rows are n_ref words each */
    const size_t row_bytes = std::max((size_t)n_ref, (size_t)1) * 4;
    const size_t chunk = std::min(nq, std::max((size_t)CSM_APPEARANCE_TABLE_BYTES / row_bytes, (size_t)1));
    int rc;
    if ((rc = reserve(ctx, ctx->ap_dev, up.off + work.off + back.off))) return rc;
    if ((rc = reserve(ctx, ctx->ap_pin, std::max(up.off, back.off)))) return rc;
    if ((rc = reserve(ctx, ctx->ap_table, chunk * row_bytes))) return rc;
    char* const pin = ctx->ap_pin.as<char>();
    char* const dev = ctx->ap_dev.as<char>();
    char* const dev_back = dev + up.off + work.off;

    std::memcpy(pin + d_at, descriptors, n * cells);
    std::memcpy(pin + t_at, travel, n * 8);
    std::memcpy(pin + qt_at, query_travel, nq * 8);
    std::memcpy(pin + m_at, scan_map_index, n * 4);
    std::memcpy(pin + qi_at, query_index, nq * 4);
    HIP_TRY(ctx, hipMemcpyAsync(dev, pin, up.off, hipMemcpyHostToDevice, ctx->stream));

    AppearanceJob job;
    job.desc = reinterpret_cast<const uint32_t*>(dev + d_at);
    job.ring_sum = reinterpret_cast<uint16_t*>(dev + up.off + rs_at);
    job.travel = reinterpret_cast<const double*>(dev + t_at);
    job.map = reinterpret_cast<const int32_t*>(dev + m_at);
    job.query_index = reinterpret_cast<const int32_t*>(dev + qi_at);
    job.query_travel = reinterpret_cast<const double*>(dev + qt_at);
    job.table = ctx->ap_table.as<uint32_t>();
    job.out = reinterpret_cast<csm_appearance_candidate*>(dev_back + rec_at);
    job.counts = reinterpret_cast<int32_t*>(dev_back + cnt_at);
    job.prefix = reinterpret_cast<int32_t*>(dev_back + pre_at);
    job.eligible = reinterpret_cast<int32_t*>(dev_back + eli_at);
    job.travel_threshold = prm->travel_dist_threshold;
    job.max_distance = prm->max_distance;
    job.min_cell_sum = prm->min_cell_sum;
    job.n_scan = n_scan;
    job.n_ref = n_ref;
    job.n_maps = n_maps;
    job.k = k;
    job.one_per_map = prm->one_per_map;
    job.n_rings = nr;
    job.n_sectors = ns;
    job.q0 = 0;
    job.phase_pitch = ap_phase_pitch(nr, ns);
    const size_t lds = (size_t)4 * job.phase_pitch * sizeof(uint32_t);
    const unsigned ref_chunks = (unsigned)ceil_div(n_ref, CSM_APPEARANCE_REF_CHUNK);
    int e = 0;
    {
        ScopedTimer tm(ctx, "appearance_search");
        keep_first(e, launch(k_appearance_ring_sums, dim3((unsigned)((n * nr + kApBlock - 1) / kApBlock)),
                             dim3(kApBlock), ctx->stream, job));
        for (size_t q0 = 0; q0 < nq && !e; q0 += chunk) {
            const unsigned nc = (unsigned)std::min(chunk, nq - q0);
            job.q0 = (int32_t)q0;
            if (ref_chunks)
                keep_first(e, launch_lds(ctx->device, k_appearance_pairs, dim3(nc, ref_chunks), dim3(kApBlock), lds,
                                         ctx->stream, job, job.desc, job.table));
            keep_first(e, launch(k_appearance_select, dim3(nc), dim3(kApBlock), ctx->stream, job));
        }
    }
    if ((rc = launched_ok(ctx, e, "appearance search"))) return rc;
    /* the upload has been read by the time the kernels have run: the pinned block is free for the way back */
    HIP_TRY(ctx, hipMemcpyAsync(pin, dev_back, back.off, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(out, pin + rec_at, nq * k * sizeof(csm_appearance_candidate));
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
