/* loop_search_host_check.cpp -- the host code of the loop search unit (csm_host_travel_distances,
 * csm_host_loop_search, csm_host_loop_candidates_nearest) in a stand-alone program, for a run under
 * AddressSanitizer and UndefinedBehaviorSanitizer on a machine without a GPU. It builds the laps family of
 * tests/loop_search_cases.py (three laps of a 10 m x 6 m rectangle on a 0.25 m lattice, maps of 10 nodes),
 * runs every node as a query at K = 1, 2, 16 with both one_per_map values, the online form behind
 * csm_host_loop_candidates_nearest, and every refusal; it checks the invariants a reader can state without a
 * second implementation. From the repository root:
 *
 *   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
 *       -Xarch_host -fno-sanitize-recover=undefined tools/loop_search_host_check.cpp \
 *       my-lidar-graph-slam-v2_amd/csrc/csm_loopsearch_api.hip -fsanitize=address,undefined -o loop_search_host_check
 *   ./loop_search_host_check
 *
 * No device call is made: the device entry of the unit is linked and never called. */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/csm_hip.h"

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "check failed: %s (line %d)\n", #cond, __LINE__);    \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

int main()
{
    std::vector<double> poses;
    for (int lap = 0; lap < 3; ++lap) {
        double x = 0.0, y = 0.0;
        const int side[4][3] = { { 1, 0, 40 }, { 0, 1, 24 }, { -1, 0, 40 }, { 0, -1, 24 } };
        for (const auto& s : side)
            for (int i = 0; i < s[2]; ++i) {
                poses.insert(poses.end(), { x, y, std::atan2((double)s[1], (double)s[0]) });
                x += 0.25 * s[0];
                y += 0.25 * s[1];
            }
    }
    const int n = (int)poses.size() / 3;
    CHECK(n == 384);
    std::vector<int32_t> map(n), query(n);
    for (int i = 0; i < n; ++i) {
        map[i] = i / 10;
        query[i] = n - 1 - i;                       /* descending */
    }
    const int n_maps = map[n - 1] + 1;
    std::vector<double> travel(n), qt(n);
    CHECK(csm_host_travel_distances(poses.data(), n, travel.data()) == CSM_OK);
    CHECK(travel[0] == 0.0 && travel[n - 1] == 0.25 * (n - 1));
    CHECK(csm_host_travel_distances(poses.data(), 0, travel.data()) == CSM_OK);
    for (int i = 0; i < n; ++i)
        qt[i] = travel[query[i]];

    const int ks[3] = { 1, 2, 16 };
    for (int k : ks)
        for (int per_map = 0; per_map < 2; ++per_map) {
            csm_loop_search_params prm = { 10.0, 2.0, k, per_map };
            std::vector<csm_loop_candidate> out((size_t)n * k);
            std::vector<int32_t> counts(n);
            csm_loop_search_info info = { -1, -1 };
            CHECK(csm_host_loop_search(poses.data(), map.data(), travel.data(), n, n_maps, n, query.data(), qt.data(),
                                       n, &prm, out.data(), counts.data(), &info) == CSM_OK);
            CHECK(info.pairs_eligible > 0 && info.pairs_evaluated > info.pairs_eligible);
            int64_t used = 0;
            for (int i = 0; i < n; ++i) {
                CHECK(counts[i] >= 0 && counts[i] <= k);
                used += counts[i];
                for (int s = 0; s < k; ++s) {
                    const csm_loop_candidate& c = out[(size_t)i * k + s];
                    CHECK(c.query_scan_index == query[i] && c.reserved == 0);
                    if (s >= counts[i]) {
                        CHECK(c.ref_scan_index == -1 && c.ref_map_index == -1 && c.dist_sq == 0.0);
                        continue;
                    }
                    CHECK(c.ref_scan_index >= 0 && c.ref_scan_index < n && c.ref_map_index == map[c.ref_scan_index]);
                    CHECK(c.ref_map_index != map[query[i]] && c.dist_sq < 4.0);
                    CHECK(!(qt[i] - travel[c.ref_scan_index] < 10.0));
                    if (s > 0) {
                        const csm_loop_candidate& b = out[(size_t)i * k + s - 1];
                        CHECK(b.dist_sq < c.dist_sq || (b.dist_sq == c.dist_sq && b.ref_scan_index < c.ref_scan_index));
                        if (per_map)
                            for (int t = 0; t < s; ++t)
                                CHECK(out[(size_t)i * k + t].ref_map_index != c.ref_map_index);
                    }
                }
            }
            CHECK(used > 0 && used <= info.pairs_eligible);
            /* the nearest form: all, some, none */
            for (int total : { 0, 5, 4 * n * k }) {
                std::vector<csm_loop_candidate> kept((size_t)total + 1);
                int32_t n_kept = -1;
                CHECK(csm_host_loop_candidates_nearest(out.data(), counts.data(), n, k, total, kept.data(), &n_kept) ==
                      CSM_OK);
                CHECK(n_kept == (used < total ? used : total));
                for (int i = 1; i < n_kept; ++i)
                    CHECK(kept[i - 1].dist_sq <= kept[i].dist_sq);
            }
        }

    /* the online form: the last map's nodes against the maps before it, one travel distance for all */
    {
        csm_loop_search_params prm = { 10.0, 2.0, 16, 0 };
        std::vector<int32_t> q = { 380, 381, 382, 383 }, counts(4);
        std::vector<double> t(4, travel[n - 1]);
        std::vector<csm_loop_candidate> out(4 * 16), kept(16);
        int32_t n_kept = 0;
        CHECK(csm_host_loop_search(poses.data(), map.data(), travel.data(), n, n_maps, 380, q.data(), t.data(), 4, &prm,
                                   out.data(), counts.data(), nullptr) == CSM_OK);
        CHECK(csm_host_loop_candidates_nearest(out.data(), counts.data(), 4, 16, 16, kept.data(), &n_kept) == CSM_OK);
        CHECK(n_kept == 16 && kept[0].dist_sq == 0.0);
    }

    /* refusals: nothing is read past what the arguments say, nothing is written */
    {
        csm_loop_search_params prm = { 10.0, 2.0, 2, 0 };
        std::vector<csm_loop_candidate> out((size_t)n * 16);
        std::vector<int32_t> counts(n);
        auto run = [&](const std::vector<double>& p, const std::vector<int32_t>& m, const std::vector<double>& t,
                       int maps, int n_ref, const std::vector<int32_t>& q, int n_q, const csm_loop_search_params& pr) {
            return csm_host_loop_search(p.data(), m.data(), t.data(), n, maps, n_ref, q.data(), qt.data(), n_q, &pr,
                                        out.data(), counts.data(), nullptr);
        };
        CHECK(run(poses, map, travel, n_maps, n, query, n, prm) == CSM_OK);
        std::vector<double> bad = poses;
        bad[3 * 7] = NAN;
        CHECK(run(bad, map, travel, n_maps, n, query, n, prm) == CSM_EINVAL);
        bad = travel;
        bad[100] = 0.0;
        CHECK(run(poses, map, bad, n_maps, n, query, n, prm) == CSM_EINVAL);
        bad[100] = INFINITY;
        CHECK(run(poses, map, bad, n_maps, n, query, n, prm) == CSM_EINVAL);
        std::vector<int32_t> worse = map;
        worse[100] = 3;
        CHECK(run(poses, worse, travel, n_maps, n, query, n, prm) == CSM_EINVAL);
        CHECK(run(poses, map, travel, n_maps - 1, n, query, n, prm) == CSM_EINVAL);
        CHECK(run(poses, map, travel, n_maps, n + 1, query, n, prm) == CSM_EINVAL);
        CHECK(run(poses, map, travel, n_maps, -1, query, n, prm) == CSM_EINVAL);
        CHECK(run(poses, map, travel, n_maps, n, query, 0, prm) == CSM_EINVAL);
        worse = query;
        worse[5] = worse[6];
        CHECK(run(poses, map, travel, n_maps, n, worse, n, prm) == CSM_EINVAL);
        worse[5] = n;
        CHECK(run(poses, map, travel, n_maps, n, worse, n, prm) == CSM_EINVAL);
        for (int k : { 0, 17 }) {
            csm_loop_search_params p2 = prm;
            p2.n_per_query = k;
            CHECK(run(poses, map, travel, n_maps, n, query, n, p2) == CSM_EINVAL);
        }
        csm_loop_search_params p3 = prm;
        p3.node_dist_threshold = NAN;
        CHECK(run(poses, map, travel, n_maps, n, query, n, p3) == CSM_EINVAL);
    }
    std::puts("loop search host check: ok");
    return 0;
}
