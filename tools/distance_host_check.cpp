/* distance_host_check.cpp -- the host code of the distance unit (csm_host_distance_kernel,
 * csm_host_distance_transform, csm_host_distance_map: my-lidar-graph-slam-v2_amd/csrc/csm_distance_host.hpp,
 * which this file includes and thereby defines) in a stand-alone program, for a run under AddressSanitizer and
 * UndefinedBehaviorSanitizer on a machine without a GPU. It runs the three functions over the edge shapes
 * (1 x 1, 1 x N, N x 1, no obstacle, every cell an obstacle, the value 65535, thresholds above every value),
 * the tie cases of DESIGN.md 4p, random grids against a brute force over the obstacles, every radius limit,
 * null outputs and every refusal. From the repository root:
 *
 *   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
 *       tools/distance_host_check.cpp -o distance_host_check
 *   ./distance_host_check
 *
 * No HIP header is read and no device call is made. Never loaded into Python, never run on a GPU machine. */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../my-lidar-graph-slam-v2_amd/csrc/csm_distance_host.hpp"

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "check failed: %s (line %d)\n", #cond, __LINE__);    \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

static uint32_t g_state = 12345u;
static uint32_t next_u32()
{
    g_state = g_state * 1664525u + 1013904223u;
    return g_state >> 8;
}

/* the definition: every obstacle in ascending index order, a strict < */
static void brute(const std::vector<uint16_t>& g, int rows, int cols, uint32_t occ, std::vector<uint32_t>& d2,
                  std::vector<uint32_t>& nearest)
{
    d2.assign(g.size(), CSM_DISTANCE_NONE);
    nearest.assign(g.size(), CSM_DISTANCE_NONE);
    for (int o = 0; o < rows * cols; ++o) {
        if (g[o] < occ)
            continue;
        const int orow = o / cols, ocol = o % cols;
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) {
                const uint32_t d = (uint32_t)((orow - r) * (orow - r) + (ocol - c) * (ocol - c));
                if (d < d2[(size_t)r * cols + c]) {
                    d2[(size_t)r * cols + c] = d;
                    nearest[(size_t)r * cols + c] = (uint32_t)o;
                }
            }
    }
}

static int check_grid(const std::vector<uint16_t>& g, int rows, int cols, uint32_t occ)
{
    std::vector<uint32_t> want_d2, want_near, d2(g.size(), 7u), near(g.size(), 7u), only(g.size(), 7u);
    brute(g, rows, cols, occ, want_d2, want_near);
    CHECK(csm_host_distance_transform(g.data(), rows, cols, occ, d2.data(), near.data()) == CSM_OK);
    CHECK(d2 == want_d2 && near == want_near);
    CHECK(csm_host_distance_transform(g.data(), rows, cols, occ, only.data(), nullptr) == CSM_OK && only == want_d2);
    CHECK(csm_host_distance_transform(g.data(), rows, cols, occ, nullptr, only.data()) == CSM_OK && only == want_near);
    for (int R : { 1, 2, 16, CSM_DISTANCE_MAX_RADIUS })
        for (int keep = 0; keep < 2; ++keep) {
            std::vector<uint16_t> table((size_t)R * R + 1), out(g.size(), 0xabcd);
            for (size_t i = 0; i < table.size(); ++i)
                table[i] = (uint16_t)(65534u - i % 65533u);
            const csm_distance_params p = { R, occ, keep, 0, table.data() };
            CHECK(csm_host_distance_map(g.data(), rows, cols, &p, out.data()) == CSM_OK);
            for (size_t i = 0; i < g.size(); ++i) {
                const uint32_t at = want_d2[i] < (uint32_t)(R * R) ? want_d2[i] : (uint32_t)(R * R);
                CHECK(out[i] == (keep && g[i] == 0 ? 0 : table[at]));
            }
        }
    return 0;
}

static std::vector<uint16_t> with(int rows, int cols, std::initializer_list<std::pair<int, int>> cells)
{
    std::vector<uint16_t> g((size_t)rows * cols, 700);
    for (const auto& rc : cells)
        g[(size_t)rc.first * cols + rc.second] = 50000;
    return g;
}

static int check_shapes()
{
    CHECK(check_grid({ 50000 }, 1, 1, 32768) == 0);
    CHECK(check_grid({ 900 }, 1, 1, 32768) == 0);
    for (int pass = 0; pass < 2; ++pass) {      /* 1 x 200, then 200 x 1 */
        std::vector<uint16_t> line(200);
        for (int i = 0; i < 200; ++i)
            line[i] = i % 7 < 4 ? 700 : 0;
        for (int i : { 0, 199, 63, 64, 65 })
            line[i] = 40000;
        CHECK(check_grid(line, pass ? 200 : 1, pass ? 1 : 200, 32768) == 0);
    }
    CHECK(check_grid(std::vector<uint16_t>(20 * 33, 900), 20, 33, 32768) == 0);        /* no obstacle */
    CHECK(check_grid(std::vector<uint16_t>(20 * 33, 45000), 20, 33, 32768) == 0);      /* every cell */
    std::vector<uint16_t> top = with(24, 40, { { 3, 3 } });
    top[7 * 40 + 9] = 65535;
    CHECK(check_grid(top, 24, 40, 65535) == 0);
    CHECK(check_grid(top, 24, 40, 70000) == 0);
    CHECK(check_grid(top, 24, 40, 1) == 0);
    return 0;
}

static int check_ties()
{
    std::vector<uint32_t> d2, near;
    auto run = [&](const std::vector<uint16_t>& g, int rows, int cols) {
        d2.assign(g.size(), 0);
        near.assign(g.size(), 0);
        return csm_host_distance_transform(g.data(), rows, cols, 32768, d2.data(), near.data());
    };
    const auto cross = with(11, 11, { { 5, 0 }, { 0, 5 }, { 10, 5 }, { 5, 10 } });
    CHECK(run(cross, 11, 11) == CSM_OK && d2[5 * 11 + 5] == 25 && near[5 * 11 + 5] == 5);
    CHECK(check_grid(cross, 11, 11, 32768) == 0);
    const auto pyth = with(12, 12, { { 10, 5 }, { 8, 9 }, { 2, 1 }, { 9, 2 }, { 5, 10 } });
    CHECK(run(pyth, 12, 12) == CSM_OK && d2[5 * 12 + 5] == 25 && near[5 * 12 + 5] == 25);
    CHECK(check_grid(pyth, 12, 12, 32768) == 0);
    const auto column = with(9, 5, { { 1, 2 }, { 7, 2 } });
    CHECK(run(column, 9, 5) == CSM_OK && d2[4 * 5 + 2] == 9 && near[4 * 5 + 2] == 1 * 5 + 2);
    const auto row = with(5, 9, { { 2, 1 }, { 2, 7 } });
    CHECK(run(row, 5, 9) == CSM_OK && d2[2 * 9 + 4] == 9 && near[2 * 9 + 4] == 2 * 9 + 1);
    /* an obstacle of the cell's own row at k^2 == best, with the smaller index */
    const auto own = with(11, 11, { { 5, 2 }, { 8, 3 } });
    CHECK(run(own, 11, 11) == CSM_OK && d2[5 * 11 + 7] == 25 && near[5 * 11 + 7] == 5 * 11 + 2);
    CHECK(check_grid(own, 11, 11, 32768) == 0);
    return 0;
}

static int check_random()
{
    static const uint32_t densities[5] = { 0, 2, 30, 500, 1000 };       /* obstacles per thousand cells */
    for (int trial = 0; trial < 40; ++trial) {
        const int rows = 1 + (int)(next_u32() % 48), cols = 1 + (int)(next_u32() % 48);
        const uint32_t per_mille = densities[trial % 5];
        std::vector<uint16_t> g((size_t)rows * cols);
        for (auto& v : g)
            v = next_u32() % 1000 < per_mille ? (uint16_t)(32768 + next_u32() % 32767) : (uint16_t)(next_u32() % 32768);
        CHECK(check_grid(g, rows, cols, 32768) == 0);
    }
    /* the far corner of a 200 x 200 map: d2(0, 0) = 79202, 765 cells beyond 255 */
    std::vector<uint16_t> far((size_t)200 * 200, 0);
    far.back() = 50000;
    std::vector<uint32_t> d2(far.size());
    CHECK(csm_host_distance_transform(far.data(), 200, 200, 32768, d2.data(), nullptr) == CSM_OK);
    int beyond = 0;
    for (uint32_t v : d2)
        beyond += v > 255u * 255u;
    CHECK(d2[0] == 79202u && beyond == 765);
    return 0;
}

static int check_table_and_refusals()
{
    std::vector<uint16_t> t((size_t)CSM_DISTANCE_MAX_RADIUS * CSM_DISTANCE_MAX_RADIUS + 1, 0xabcd);
    CHECK(csm_host_distance_kernel(1.0, 0.05, CSM_DISTANCE_MAX_RADIUS, 65534, 1, t.data()) == CSM_OK);
    CHECK(t[0] == 65534 && t.back() >= 1);
    for (size_t i = 1; i < t.size(); ++i)
        CHECK(t[i] <= t[i - 1] && t[i] >= 1);
    std::vector<uint16_t> one(2, 0xabcd);
    CHECK(csm_host_distance_kernel(0.01, 0.05, 1, 7, 7, one.data()) == CSM_OK && one[0] == 7 && one[1] == 7);
    CHECK(csm_host_distance_kernel(0.01, 0.05, 1, 65534, 0, one.data()) == CSM_OK && one[0] == 65534 && one[1] == 0);
    CHECK(csm_host_distance_kernel(0.0, 0.05, 1, 65534, 1, one.data()) == CSM_EINVAL);
    CHECK(csm_host_distance_kernel(0.1, -1.0, 1, 65534, 1, one.data()) == CSM_EINVAL);
    CHECK(csm_host_distance_kernel(NAN, 0.05, 1, 65534, 1, one.data()) == CSM_EINVAL);
    CHECK(csm_host_distance_kernel(0.1, 0.05, 0, 65534, 1, one.data()) == CSM_EINVAL);
    CHECK(csm_host_distance_kernel(0.1, 0.05, CSM_DISTANCE_MAX_RADIUS + 1, 65534, 1, t.data()) == CSM_EINVAL);
    CHECK(csm_host_distance_kernel(0.1, 0.05, 1, 65535, 1, one.data()) == CSM_EINVAL);
    CHECK(csm_host_distance_kernel(0.1, 0.05, 1, 10, 11, one.data()) == CSM_EINVAL);
    CHECK(csm_host_distance_kernel(0.1, 0.05, 1, 65534, 1, nullptr) == CSM_EINVAL);

    const std::vector<uint16_t> g(20, 40000);
    std::vector<uint32_t> out32(20);
    std::vector<uint16_t> out16(20);
    CHECK(csm_host_distance_transform(nullptr, 4, 5, 32768, out32.data(), nullptr) == CSM_EINVAL);
    CHECK(csm_host_distance_transform(g.data(), 4, 5, 32768, nullptr, nullptr) == CSM_EINVAL);
    CHECK(csm_host_distance_transform(g.data(), 4, 5, 0, out32.data(), nullptr) == CSM_EINVAL);
    CHECK(csm_host_distance_transform(g.data(), 0, 5, 32768, out32.data(), nullptr) == CSM_EINVAL);
    CHECK(csm_host_distance_transform(g.data(), 4, 0, 32768, out32.data(), nullptr) == CSM_EINVAL);
    CHECK(csm_host_distance_transform(g.data(), 32768, 5, 32768, out32.data(), nullptr) == CSM_EINVAL);
    CHECK(csm_host_distance_transform(g.data(), 4, 32768, 32768, out32.data(), nullptr) == CSM_EINVAL);
    csm_distance_params p = { 2, 32768, 0, 0, t.data() };
    CHECK(csm_host_distance_map(g.data(), 4, 5, &p, out16.data()) == CSM_OK);
    CHECK(csm_host_distance_map(g.data(), 4, 5, nullptr, out16.data()) == CSM_EINVAL);
    CHECK(csm_host_distance_map(g.data(), 4, 5, &p, nullptr) == CSM_EINVAL);
    CHECK(csm_host_distance_map(nullptr, 4, 5, &p, out16.data()) == CSM_EINVAL);
    CHECK(csm_host_distance_map(g.data(), 32768, 5, &p, out16.data()) == CSM_EINVAL);
    p.radius = 0;
    CHECK(csm_host_distance_map(g.data(), 4, 5, &p, out16.data()) == CSM_EINVAL);
    p.radius = CSM_DISTANCE_MAX_RADIUS + 1;
    CHECK(csm_host_distance_map(g.data(), 4, 5, &p, out16.data()) == CSM_EINVAL);
    p.radius = 2;
    p.occupied_min = 0;
    CHECK(csm_host_distance_map(g.data(), 4, 5, &p, out16.data()) == CSM_EINVAL);
    p.occupied_min = 32768;
    p.table = nullptr;
    CHECK(csm_host_distance_map(g.data(), 4, 5, &p, out16.data()) == CSM_EINVAL);
    std::vector<uint16_t> over(5, 100);
    over[4] = 65535;
    p.table = over.data();
    CHECK(csm_host_distance_map(g.data(), 4, 5, &p, out16.data()) == CSM_EINVAL);
    /* the widest and the tallest map the entries accept: one row / one column of 32767 cells */
    std::vector<uint16_t> wide(32767, 0);
    wide[32766] = 50000;
    std::vector<uint32_t> d2(32767), near(32767);
    CHECK(csm_host_distance_transform(wide.data(), 1, 32767, 32768, d2.data(), near.data()) == CSM_OK);
    CHECK(d2[0] == 32766u * 32766u && near[0] == 32766u);
    CHECK(csm_host_distance_transform(wide.data(), 32767, 1, 32768, d2.data(), near.data()) == CSM_OK);
    CHECK(d2[0] == 32766u * 32766u && near[0] == 32766u);
    return 0;
}

int main()
{
    if (check_shapes() || check_ties() || check_random() || check_table_and_refusals())
        return 1;
    std::printf("distance_host_check ok\n");
    return 0;
}
