/* csm_consistency_api.hip -- do the loop edges agree with each other: csm_loop_consistency and its CPU reference
 * csm_host_loop_consistency (include/csm_hip.h), with the kernels (csm_consistency_kernels.hip). A translation
 * unit of libcsm_hip.so of its own.
 *
 * A call is checked first (a refused call has run nothing) and its tables are built on the host: per edge z,
 * cos / sin of z.theta (glibc), Sigma = Lambda^-1 (csm_host_information_from_covariance), and the two nodes'
 * p, cos, sin, theta and travel -- one cos / sin per node an edge names, copied into every record that names it.
 * Then one upload of the records, the chain k_lc_pairs -> k_lc_degree -> k_lc_rank -> k_lc_greedy -> k_lc_finish
 * without a host round trip, and one read-back of [selected | degree | info] (the adjacency and the chi^2 matrix
 * only where the caller asks for them). Nothing the context keeps between calls is touched but lc_dev / lc_pin,
 * and nothing in them is read before the call has written it. */
#include "csm_internal.hpp"

#include "csm_consistency_kernels.hip"

static_assert(sizeof(csm_loop_consistency_info) == 32, "k_lc_finish writes the whole record");

namespace {

struct LcTables {
    std::vector<double> rec;      /* [M][kLcRec] */
    double drift[3];
    int n_seeds;                  /* the seeds that run */
};

/* what is wrong with a call, or null; the tables of a call that is not refused */
const char* lc_prepare(const double* local_poses, int32_t n_local, const double* scan_poses, int32_t n_scan,
                       const csm_pose_graph_edge* edges, int32_t n_edges, double gate, const double* drift,
                       const double* local_travel, const double* scan_travel, int32_t n_seeds,
                       const int32_t* selected, const int32_t* degree, const csm_loop_consistency_info* info,
                       const double* chi2, LcTables& T)
{
    if (!local_poses || !scan_poses || !edges || !selected || !degree || !info)
        return "a null pointer";
    if (n_local < 1 || n_scan < 1)
        return "a graph without local map nodes or without scan nodes";
    if (n_edges < 1 || n_edges > CSM_LOOP_CONSISTENCY_MAX_EDGES)
        return "n_edges outside 1..CSM_LOOP_CONSISTENCY_MAX_EDGES";
    if (chi2 && n_edges > CSM_LOOP_CONSISTENCY_MAX_CHI2_EDGES)
        return "the chi-square matrix of more than CSM_LOOP_CONSISTENCY_MAX_CHI2_EDGES edges";
    if (std::isnan(gate) || gate < 0.0)
        return "a gate that is negative or not a number";
    if (n_seeds < 0)
        return "n_seeds < 0";
    if ((drift != nullptr) != (local_travel != nullptr) || (drift != nullptr) != (scan_travel != nullptr))
        return "a drift model needs drift_var_per_metre, local_travel and scan_travel together";
    for (int a = 0; a < 3; ++a) {
        T.drift[a] = drift ? drift[a] : 0.0;
        if (!std::isfinite(T.drift[a]) || T.drift[a] < 0.0)
            return "a drift variance that is negative or not finite";
    }
    for (size_t q = 0; q < 3 * (size_t)n_local; ++q)
        if (!std::isfinite(local_poses[q]))
            return "a local map pose that is not finite";
    for (size_t q = 0; q < 3 * (size_t)n_scan; ++q)
        if (!std::isfinite(scan_poses[q]))
            return "a scan pose that is not finite";
    if (drift) {
        for (int32_t q = 0; q < n_local; ++q)
            if (!std::isfinite(local_travel[q]))
                return "a travel distance that is not finite";
        for (int32_t q = 0; q < n_scan; ++q)
            if (!std::isfinite(scan_travel[q]))
                return "a travel distance that is not finite";
    }
    for (int32_t e = 0; e < n_edges; ++e) {
        const csm_pose_graph_edge& E = edges[e];
        if (E.local_map_index < 0 || E.local_map_index >= n_local || E.scan_index < 0 || E.scan_index >= n_scan)
            return "an edge's node index out of range";
        for (int q = 0; q < 3; ++q)
            if (!std::isfinite(E.relative_pose[q]))
                return "a relative pose that is not finite";
        for (int q = 0; q < 9; ++q)
            if (!std::isfinite(E.information[q]))
                return "an information entry that is not finite";
    }
    /* one cos / sin per node that an edge names */
    std::vector<double> lcs(2 * (size_t)n_local), scs(2 * (size_t)n_scan);
    std::vector<bool> lseen((size_t)n_local, false), sseen((size_t)n_scan, false);
    T.rec.assign((size_t)n_edges * kLcRec, 0.0);
    for (int32_t e = 0; e < n_edges; ++e) {
        const csm_pose_graph_edge& E = edges[e];
        const size_t s = (size_t)E.local_map_index, t = (size_t)E.scan_index;
        if (!lseen[s]) {
            lseen[s] = true;
            lcs[2 * s] = cos(local_poses[3 * s + 2]);
            lcs[2 * s + 1] = sin(local_poses[3 * s + 2]);
        }
        if (!sseen[t]) {
            sseen[t] = true;
            scs[2 * t] = cos(scan_poses[3 * t + 2]);
            scs[2 * t + 1] = sin(scan_poses[3 * t + 2]);
        }
        double* r = &T.rec[(size_t)e * kLcRec];
        r[kLcZx] = E.relative_pose[0];
        r[kLcZy] = E.relative_pose[1];
        r[kLcZt] = E.relative_pose[2];
        r[kLcZc] = cos(E.relative_pose[2]);
        r[kLcZs] = sin(E.relative_pose[2]);
        double sigma[9];
        if (csm_host_information_from_covariance(E.information, sigma) != CSM_OK)
            return "an information matrix whose LDL^T has a pivot that is not positive and finite";
        r[kLcS00] = sigma[0];
        r[kLcS10] = sigma[3];
        r[kLcS11] = sigma[4];
        r[kLcS20] = sigma[6];
        r[kLcS21] = sigma[7];
        r[kLcS22] = sigma[8];
        r[kLcSx] = local_poses[3 * s];
        r[kLcSy] = local_poses[3 * s + 1];
        r[kLcSc] = lcs[2 * s];
        r[kLcSs] = lcs[2 * s + 1];
        r[kLcSt] = local_poses[3 * s + 2];
        r[kLcSl] = drift ? local_travel[s] : 0.0;
        r[kLcTx] = scan_poses[3 * t];
        r[kLcTy] = scan_poses[3 * t + 1];
        r[kLcTc] = scs[2 * t];
        r[kLcTs] = scs[2 * t + 1];
        r[kLcTt] = scan_poses[3 * t + 2];
        r[kLcTl] = drift ? scan_travel[t] : 0.0;
    }
    T.n_seeds = (n_seeds == 0 || n_seeds >= n_edges) ? n_edges : n_seeds;
    return nullptr;
}

int lc_words(int m) { return (m + 63) / 64; }

} /* namespace */

extern "C" {

int csm_host_loop_consistency(const double* local_poses, int32_t n_local, const double* scan_poses, int32_t n_scan,
                              const csm_pose_graph_edge* edges, int32_t n_edges, double gate,
                              const double* drift_var_per_metre, const double* local_travel,
                              const double* scan_travel, int32_t n_seeds, int32_t* selected, int32_t* degree,
                              csm_loop_consistency_info* info, uint64_t* adjacency, double* chi2)
{
    LcTables T;
    if (lc_prepare(local_poses, n_local, scan_poses, n_scan, edges, n_edges, gate, drift_var_per_metre, local_travel,
                   scan_travel, n_seeds, selected, degree, info, chi2, T))
        return CSM_EINVAL;
    const int M = n_edges, W = lc_words(M);
    std::vector<uint64_t> own;
    if (!adjacency) {
        own.resize((size_t)M * W);
        adjacency = own.data();
    }
    std::fill(adjacency, adjacency + (size_t)M * W, (uint64_t)0);
    int64_t bad = 0, pairs = 0;
    for (int i = 0; i < M; ++i) {
        if (chi2)
            chi2[(size_t)i * M + i] = 0.0;
        for (int j = i + 1; j < M; ++j) {
            double chi = 0.0;
            bool ok = false;
            if (lc_pair(&T.rec[(size_t)i * kLcRec], &T.rec[(size_t)j * kLcRec], T.drift, &chi)) {
                chi = (double)INFINITY;
                ++bad;
            } else {
                ok = chi <= gate;
            }
            if (ok) {
                adjacency[(size_t)i * W + (j >> 6)] |= 1ull << (j & 63);
                adjacency[(size_t)j * W + (i >> 6)] |= 1ull << (i & 63);
                ++pairs;
            }
            if (chi2)
                chi2[(size_t)i * M + j] = chi2[(size_t)j * M + i] = chi;
        }
    }
    for (int i = 0; i < M; ++i) {
        int d = 0;
        for (int w = 0; w < W; ++w)
            d += __builtin_popcountll(adjacency[(size_t)i * W + w]);
        degree[i] = d;
    }
    /* the seeds: by degree descending, ties to the lower index */
    std::vector<int32_t> order((size_t)M);
    for (int i = 0; i < M; ++i)
        order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return degree[a] > degree[b]; });
    std::vector<uint64_t> C((size_t)W), K((size_t)W), best_k((size_t)W);
    int best_size = 0, best_seed = -1;
    for (int s = 0; s < T.n_seeds; ++s) {
        const int v0 = order[(size_t)s];
        std::fill(K.begin(), K.end(), (uint64_t)0);
        K[(size_t)(v0 >> 6)] = 1ull << (v0 & 63);
        std::copy(adjacency + (size_t)v0 * W, adjacency + (size_t)(v0 + 1) * W, C.begin());
        int size = 1;
        for (;;) {
            int pick = -1, pick_n = -1;
            for (int u = 0; u < M; ++u) {
                if (!((C[(size_t)(u >> 6)] >> (u & 63)) & 1ull))
                    continue;
                int n = 0;
                for (int w = 0; w < W; ++w)
                    n += __builtin_popcountll(adjacency[(size_t)u * W + w] & C[(size_t)w]);
                if (n > pick_n) {
                    pick_n = n;
                    pick = u;
                }
            }
            if (pick < 0)
                break;
            for (int w = 0; w < W; ++w)
                C[(size_t)w] &= adjacency[(size_t)pick * W + w];
            K[(size_t)(pick >> 6)] |= 1ull << (pick & 63);
            ++size;
        }
        if (size > best_size) {
            best_size = size;
            best_seed = v0;
            best_k = K;
        }
    }
    for (int u = 0; u < M; ++u)
        selected[u] = (int32_t)((best_k[(size_t)(u >> 6)] >> (u & 63)) & 1ull);
    std::memset(info, 0, sizeof(*info));
    info->consistent_pairs = pairs;
    info->bad_pivots = bad;
    info->clique_size = best_size;
    info->winning_seed = best_seed;
    info->seeds_run = T.n_seeds;
    return CSM_OK;
}

int csm_loop_consistency(csm_ctx* ctx, const double* local_poses, int32_t n_local, const double* scan_poses,
                         int32_t n_scan, const csm_pose_graph_edge* edges, int32_t n_edges, double gate,
                         const double* drift_var_per_metre, const double* local_travel, const double* scan_travel,
                         int32_t n_seeds, int32_t* selected, int32_t* degree, csm_loop_consistency_info* info,
                         uint64_t* adjacency, double* chi2)
{
    if (!ctx)
        return CSM_EINVAL;
    LcTables T;
    if (const char* why = lc_prepare(local_poses, n_local, scan_poses, n_scan, edges, n_edges, gate,
                                     drift_var_per_metre, local_travel, scan_travel, n_seeds, selected, degree, info,
                                     chi2, T))
        return fail(ctx, CSM_EINVAL, "csm_loop_consistency: %s", why);
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    const size_t M = (size_t)n_edges, W = (size_t)lc_words(n_edges), S = (size_t)T.n_seeds;
    /* [records | adjacency | tile counts | seeds | clique sizes | clique bitsets | chi^2] and, read back in one
     * piece, [selected | degree | info] */
    Carve c;
    const size_t rec_at = c.take(M * kLcRec * 8), adj_at = c.take(M * W * 8), bad_at = c.take(W * W * 4),
                 seed_at = c.take(S * 4), size_at = c.take(S * 4), bits_at = c.take(S * W * 8),
                 chi_at = c.take(chi2 ? M * M * 8 : 0);
    const size_t back_at = c.off;
    Carve back;
    const size_t sel_at = back.take(M * 4), deg_at = back.take(M * 4), info_at = back.take(sizeof(*info));
    int rc;
    if ((rc = reserve(ctx, ctx->lc_dev, back_at + back.off))) return rc;
    if ((rc = reserve(ctx, ctx->lc_pin, std::max(M * kLcRec * 8, back.off)))) return rc;
    char* const pin = ctx->lc_pin.as<char>();
    char* const dev = ctx->lc_dev.as<char>();
    char* const dev_back = dev + back_at;
    std::memcpy(pin, T.rec.data(), M * kLcRec * 8);
    HIP_TRY(ctx, hipMemcpyAsync(dev + rec_at, pin, M * kLcRec * 8, hipMemcpyHostToDevice, ctx->stream));

    LcJob job;
    job.rec = reinterpret_cast<const double*>(dev + rec_at);
    job.adj = reinterpret_cast<uint64_t*>(dev + adj_at);
    job.chi2 = chi2 ? reinterpret_cast<double*>(dev + chi_at) : nullptr;
    job.tile_bad = reinterpret_cast<uint32_t*>(dev + bad_at);
    job.degree = reinterpret_cast<int32_t*>(dev_back + deg_at);
    job.seeds = reinterpret_cast<int32_t*>(dev + seed_at);
    job.seed_size = reinterpret_cast<int32_t*>(dev + size_at);
    job.seed_bits = reinterpret_cast<uint64_t*>(dev + bits_at);
    job.selected = reinterpret_cast<int32_t*>(dev_back + sel_at);
    job.info = reinterpret_cast<csm_loop_consistency_info*>(dev_back + info_at);
    job.gate = gate;
    for (int a = 0; a < 3; ++a)
        job.drift[a] = T.drift[a];
    job.M = n_edges;
    job.W = (int32_t)W;
    job.n_seeds = T.n_seeds;
    int g = 1;
    while (g < (int)W && g < 64)
        g <<= 1;
    job.group = g;
    int e = 0;
    {
        ScopedTimer tm(ctx, "loop_consistency");
        const dim3 blk(kLcBlock);
        {
            ScopedTimer tp(ctx, "loop_consistency_pairs");
            keep_first(e, launch(k_lc_pairs, dim3((unsigned)W, (unsigned)W), blk, ctx->stream, job));
            keep_first(e, launch(k_lc_degree, dim3((unsigned)ceil_div(n_edges, kLcWaves)), blk, ctx->stream, job));
        }
        {
            ScopedTimer ts(ctx, "loop_consistency_select");
            keep_first(e, launch(k_lc_rank, dim3((unsigned)ceil_div(n_edges, kLcBlock)), blk, ctx->stream, job));
            keep_first(e, launch(k_lc_greedy, dim3((unsigned)S), blk, ctx->stream, job));
            keep_first(e, launch(k_lc_finish, dim3(1), blk, ctx->stream, job, (int)(W * W)));
        }
    }
    if ((rc = launched_ok(ctx, e, "loop consistency"))) return rc;
    /* the upload has been read by the time the kernels have run: the pinned block is free for the way back */
    HIP_TRY(ctx, hipMemcpyAsync(pin, dev_back, back.off, hipMemcpyDeviceToHost, ctx->stream));
    if (adjacency)
        HIP_TRY(ctx, hipMemcpyAsync(adjacency, dev + adj_at, M * W * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (chi2)
        HIP_TRY(ctx, hipMemcpyAsync(chi2, dev + chi_at, M * M * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(selected, pin + sel_at, M * 4);
    std::memcpy(degree, pin + deg_at, M * 4);
    std::memcpy(info, pin + info_at, sizeof(*info));
    return CSM_OK;
}

} /* extern "C" */
