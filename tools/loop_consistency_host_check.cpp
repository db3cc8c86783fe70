/* loop_consistency_host_check.cpp -- the host code of the loop-edge consistency unit (csm_host_loop_consistency,
 * with csm_host_information_from_covariance of the pose-graph unit under it) in a stand-alone program, for a run
 * under AddressSanitizer and UndefinedBehaviorSanitizer on a machine without a GPU. It builds a walk of 120
 * scan nodes in 12 local maps with 200 loop edges of which every fourth is off by metres, runs the M ladder 1, 2,
 * 3, 63, 64, 65, 127, 128, 129, 200 with and without the optional outputs and the drift model, and every
 * refusal; it checks the invariants a reader can state without a second implementation. From the repository
 * root:
 *
 *   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
 *       -Xarch_host -fno-sanitize-recover=undefined tools/loop_consistency_host_check.cpp \
 *       my-lidar-graph-slam-v2_amd/csrc/csm_consistency_api.hip my-lidar-graph-slam-v2_amd/csrc/csm_posegraph_api.hip \
 *       -fsanitize=address,undefined -o loop_consistency_host_check
 *   ./loop_consistency_host_check
 *
 * No device call is made: the device entries of the two units are linked and never called. */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/csm_hip.h"

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "check failed: %s (line %d)\n", #cond, __LINE__);    \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

namespace {

/* a small generator of its own: the program depends on no library's random numbers */
struct Lcg {
    unsigned long long s;
    double uniform()
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(s >> 11) / 9007199254740992.0;
    }
    double normal() { return std::sqrt(-2.0 * std::log(1.0 - uniform())) * std::cos(6.283185307179586 * uniform()); }
};

void inverse_compound(const double* a, const double* b, double* out)
{
    const double c = std::cos(a[2]), s = std::sin(a[2]);
    const double dx = b[0] - a[0], dy = b[1] - a[1];
    out[0] = c * dx + s * dy;
    out[1] = -s * dx + c * dy;
    out[2] = std::remainder(b[2] - a[2], 6.283185307179586);
}

bool bit(const std::vector<uint64_t>& adj, int W, int i, int j) { return (adj[(size_t)i * W + (j >> 6)] >> (j & 63)) & 1; }

} /* namespace */

int main()
{
    const int n_scan = 120, n_local = 12, n_all = 200;
    Lcg rng { 12345 };
    std::vector<double> scan(3 * n_scan, 0.0), local(3 * n_local);
    for (int i = 1; i < n_scan; ++i) {
        const double th = scan[3 * (i - 1) + 2] + 0.35 * rng.normal();
        scan[3 * i] = scan[3 * (i - 1)] + 0.5 * std::cos(th);
        scan[3 * i + 1] = scan[3 * (i - 1) + 1] + 0.5 * std::sin(th);
        scan[3 * i + 2] = std::remainder(th, 6.283185307179586);
    }
    for (int m = 0; m < n_local; ++m)
        std::memcpy(&local[3 * m], &scan[30 * m], 24);
    std::vector<double> scan_travel(n_scan, 0.0), local_travel(n_local);
    for (int i = 1; i < n_scan; ++i)
        scan_travel[i] = scan_travel[i - 1] + std::hypot(scan[3 * i] - scan[3 * i - 3], scan[3 * i + 1] - scan[3 * i - 2]);
    for (int m = 0; m < n_local; ++m)
        local_travel[m] = scan_travel[10 * m];
    const double sigma[3] = { 0.05, 0.05, 0.02 };
    std::vector<csm_pose_graph_edge> edges(n_all);
    for (int k = 0; k < n_all; ++k) {
        csm_pose_graph_edge& e = edges[k];
        std::memset(&e, 0, sizeof(e));
        e.local_map_index = (int32_t)(rng.uniform() * n_local);
        e.scan_index = (int32_t)(rng.uniform() * n_scan);
        inverse_compound(&local[3 * e.local_map_index], &scan[3 * e.scan_index], e.relative_pose);
        for (int a = 0; a < 3; ++a)
            e.relative_pose[a] += sigma[a] * rng.normal();
        if (k % 4 == 3) {
            e.relative_pose[0] += 3.0 + rng.uniform();
            e.relative_pose[1] -= 2.0 + rng.uniform();
        }
        double cov[9] = { 0 };
        for (int a = 0; a < 3; ++a)
            cov[4 * a] = sigma[a] * sigma[a];
        CHECK(csm_host_information_from_covariance(cov, e.information) == CSM_OK);
    }
    const double gate = 11.34, drift[3] = { 0.01, 0.01, 1e-4 };
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();

    const int ladder[] = { 1, 2, 3, 63, 64, 65, 127, 128, 129, 200 };
    for (int M : ladder)
        for (int variant = 0; variant < 3; ++variant) {
            const int W = (M + 63) / 64;
            const bool with_drift = variant == 1, plain = variant == 2;
            /* exactly sized: a write past an output's end is a heap overflow the sanitizer sees */
            std::vector<int32_t> sel(M, -1), deg(M, -1);
            std::vector<uint64_t> adj(plain ? 0 : (size_t)M * W, ~0ull);
            std::vector<double> chi(plain ? 0 : (size_t)M * M, -1.0);
            csm_loop_consistency_info info;
            std::memset(&info, 0xff, sizeof(info));
            const int n_seeds = variant == 0 ? 0 : 3;
            CHECK(csm_host_loop_consistency(local.data(), n_local, scan.data(), n_scan, edges.data(), M, gate,
                                            with_drift ? drift : nullptr, with_drift ? local_travel.data() : nullptr,
                                            with_drift ? scan_travel.data() : nullptr, n_seeds, sel.data(), deg.data(),
                                            &info, plain ? nullptr : adj.data(), plain ? nullptr : chi.data()) == CSM_OK);
            long long deg_sum = 0;
            int n_sel = 0;
            for (int i = 0; i < M; ++i) {
                CHECK(sel[i] == 0 || sel[i] == 1);
                CHECK(deg[i] >= 0 && deg[i] < M);
                deg_sum += deg[i];
                n_sel += sel[i];
            }
            CHECK(info.consistent_pairs * 2 == deg_sum && info.bad_pivots == 0 && info.reserved == 0);
            CHECK(info.clique_size == n_sel && n_sel >= 1);
            CHECK(info.winning_seed >= 0 && info.winning_seed < M && sel[info.winning_seed] == 1);
            CHECK(info.seeds_run == (n_seeds == 0 || n_seeds >= M ? M : n_seeds));
            if (plain)
                continue;
            for (int i = 0; i < M; ++i) {
                int d = 0;
                CHECK(chi[(size_t)i * M + i] == 0.0 && !bit(adj, W, i, i));
                for (int j = 0; j < M; ++j) {
                    CHECK(bit(adj, W, i, j) == bit(adj, W, j, i));
                    CHECK(std::memcmp(&chi[(size_t)i * M + j], &chi[(size_t)j * M + i], 8) == 0);
                    if (i != j)
                        CHECK(bit(adj, W, i, j) == (chi[(size_t)i * M + j] <= gate));
                    d += bit(adj, W, i, j);
                    if (sel[i] && sel[j] && i != j)
                        CHECK(bit(adj, W, i, j));       /* the selection is a clique */
                }
                CHECK(d == deg[i]);
                for (int j = M; j < 64 * W; ++j)
                    CHECK(!bit(adj, W, i, j));          /* no bit past M */
            }
        }

    /* the outliers do not make it into the largest set of the whole case */
    {
        std::vector<int32_t> sel(n_all), deg(n_all);
        csm_loop_consistency_info info;
        CHECK(csm_host_loop_consistency(local.data(), n_local, scan.data(), n_scan, edges.data(), n_all, gate, nullptr,
                                        nullptr, nullptr, 4, sel.data(), deg.data(), &info, nullptr, nullptr) == CSM_OK);
        int outliers = 0;
        for (int k = 3; k < n_all; k += 4)
            outliers += sel[k];
        CHECK(outliers == 0 && info.clique_size > 50);
    }

    /* refusals */
    {
        const int M = 8;
        std::vector<int32_t> sel(M), deg(M);
        std::vector<double> chi((size_t)M * M);
        csm_loop_consistency_info info;
        auto run = [&](const double* lp, const double* sp, const csm_pose_graph_edge* e, int m, double g, const double* dv,
                       const double* lt, const double* st, int seeds) {
            return csm_host_loop_consistency(lp, n_local, sp, n_scan, e, m, g, dv, lt, st, seeds, sel.data(), deg.data(),
                                             &info, nullptr, nullptr);
        };
        const double *L = local.data(), *S = scan.data(), *LT = local_travel.data(), *ST = scan_travel.data();
        CHECK(run(L, S, edges.data(), M, gate, drift, LT, ST, 0) == CSM_OK);
        CHECK(run(L, S, edges.data(), 0, gate, nullptr, nullptr, nullptr, 0) == CSM_EINVAL);
        CHECK(run(nullptr, S, edges.data(), M, gate, nullptr, nullptr, nullptr, 0) == CSM_EINVAL);
        CHECK(run(L, S, edges.data(), M, -1.0, nullptr, nullptr, nullptr, 0) == CSM_EINVAL);
        CHECK(run(L, S, edges.data(), M, nan, nullptr, nullptr, nullptr, 0) == CSM_EINVAL);
        CHECK(run(L, S, edges.data(), M, inf, nullptr, nullptr, nullptr, 0) == CSM_OK);
        CHECK(run(L, S, edges.data(), M, gate, drift, nullptr, ST, 0) == CSM_EINVAL);
        CHECK(run(L, S, edges.data(), M, gate, drift, LT, nullptr, 0) == CSM_EINVAL);
        CHECK(run(L, S, edges.data(), M, gate, nullptr, LT, ST, 0) == CSM_EINVAL);
        CHECK(run(L, S, edges.data(), M, gate, nullptr, nullptr, nullptr, -1) == CSM_EINVAL);
        const double neg[3] = { 0.01, -0.01, 0.0 };
        CHECK(run(L, S, edges.data(), M, gate, neg, LT, ST, 0) == CSM_EINVAL);
        std::vector<csm_pose_graph_edge> bad(edges.begin(), edges.begin() + M);
        bad[3].scan_index = n_scan;
        CHECK(run(L, S, bad.data(), M, gate, nullptr, nullptr, nullptr, 0) == CSM_EINVAL);
        bad[3] = edges[3];
        bad[5].relative_pose[1] = nan;
        CHECK(run(L, S, bad.data(), M, gate, nullptr, nullptr, nullptr, 0) == CSM_EINVAL);
        bad[5] = edges[5];
        bad[7].information[4] = -1.0;
        CHECK(run(L, S, bad.data(), M, gate, nullptr, nullptr, nullptr, 0) == CSM_EINVAL);
        std::vector<double> sp(scan);
        sp[3 * 17] = inf;
        CHECK(run(L, sp.data(), edges.data(), M, gate, nullptr, nullptr, nullptr, 0) == CSM_EINVAL);
        std::vector<csm_pose_graph_edge> many(CSM_LOOP_CONSISTENCY_MAX_EDGES + 1, edges[0]);
        CHECK(run(L, S, many.data(), (int)many.size(), gate, nullptr, nullptr, nullptr, 1) == CSM_EINVAL);
        CHECK(csm_host_loop_consistency(L, n_local, S, n_scan, many.data(), CSM_LOOP_CONSISTENCY_MAX_CHI2_EDGES + 1, gate,
                                        nullptr, nullptr, nullptr, 1, sel.data(), deg.data(), &info, nullptr,
                                        chi.data()) == CSM_EINVAL);
        /* an information matrix of 1e-308: Sigma is finite, the sum of two is not -- bad pivots, counted */
        bad.assign(edges.begin(), edges.begin() + M);
        for (int q = 0; q < 9; ++q)
            bad[2].information[q] = q % 4 == 0 ? 1e-308 : 0.0;
        CHECK(run(L, S, bad.data(), M, inf, nullptr, nullptr, nullptr, 0) == CSM_OK);
        CHECK(info.bad_pivots == M - 1 && deg[2] == 0 && sel[2] == 0);
    }
    std::printf("loop_consistency_host_check: ok\n");
    return 0;
}
