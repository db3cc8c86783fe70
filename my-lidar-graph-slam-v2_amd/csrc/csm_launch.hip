/* csm_launch.hip -- the translation unit of the per-slice kernels (csm_kernels.hip) and their launch
 * wrappers (csm_launch.hpp): dispatch of the scoring kernels over the shape tables (row pitch, rows per lane,
 * stride kind) and the weighted flag, plain wrappers for everything else. */
#include <hip/hip_runtime.h>

#include "csm_kernels.hip"
#include "csm_launch.hpp"

namespace csm_launch {

/* The strided kernels (coarser levels): kStridedLS x kStridedR, stride a power of two (MODE 1) or any
 * (MODE 2), always on weighted entries. The stride-1 level is always a pair kernel. */
int score_strided(const ScoreLaunch& a, const ScoreJob& job)
{
    return match_strided_shape(a, [&](auto ls, auto r, auto mode) {
        return launch_lds(a.device, k_score<ls, r, mode>, a.grid, dim3(kBlock), a.lds, a.stream, job, a.cbx,
                          a.groups, a.n_buf);
    });
}

int score_strided_batch(const ScoreLaunch& a, const ScoreJob* jobs)
{
    return match_strided_shape(a, [&](auto ls, auto r, auto mode) {
        return launch_lds(a.device, k_score_batch<ls, r, mode>, a.grid, dim3(kBlock), a.lds, a.stream, jobs,
                          a.cbx, a.groups, a.n_slices, a.n_buf);
    });
}

/* The pair-row fine kernels: kPairLS (slots per pair row) x kPairR x weighted. */
template <class F>
int match_pairs(const ScoreLaunch& a, F f)
{
    return match_pair_shape(a, [&](auto ls, auto r) {
        return a.weighted ? f(ls, r, std::true_type()) : f(ls, r, std::false_type());
    });
}

int score_pairs(const ScoreLaunch& a, const ScoreJob& job)
{
    return match_pairs(a, [&](auto ls, auto r, auto w) {
        return launch_lds(a.device, k_score_pairs<ls, r, w>, a.theta_major ? dim3(a.grid.y, a.grid.x, 1) : a.grid,
                          dim3(kBlock), a.lds, a.stream, job, a.cbx, a.groups, a.theta_major, a.lane_map);
    });
}

int score_pairs_batch(const ScoreLaunch& a, const ScoreJob* jobs)
{
    return match_pairs(a, [&](auto ls, auto r, auto w) {
        if (a.lists == 2)
            return launch_lds(a.device, k_score_pairs2_batch<ls, r, w>, dim3(a.grid.x, (a.grid.y + 1) / 2, a.grid.z),
                              dim3(kBlock), a.lds, a.stream, jobs, a.cbx, a.groups, a.lane_map, a.xcd_map, a.bb);
        return launch_lds(a.device, k_score_pairs_batch<ls, r, w>, a.grid, dim3(kBlock), a.lds, a.stream, jobs, a.cbx,
                          a.groups, a.lane_map, a.xcd_map, a.bb);
    });
}

int score_pairs_list(const ScoreLaunch& a, const ScoreJob& job)
{
    return match_pairs(a, [&](auto ls, auto r, auto w) {
        return launch_lds(a.device, k_score_pairs_list<ls, r, w>, dim3(a.blocks), dim3(kBlock), a.lds, a.stream, job,
                          a.cbx, a.groups, a.ncb, a.lane_map, a.items, a.count);
    });
}

/* the arg-max pass over the sums of a tile-split launch: the fine plan's lane <-> candidate mapping (cbx, groups, R) */
int argmax(const ScoreLaunch& a, const ScoreJob& job, uint32_t* sum_s, uint32_t* sum_k)
{
    return match<kPairR>(a.R, [&](auto r) {
        return launch(k_argmax<r>, a.grid, dim3(kBlock), a.stream, job, sum_s, sum_k, a.cbx, a.groups);
    });
}

/* ---- the other kernels ---- */

int bin(hipStream_t s, int device, int n_theta, size_t lds, const BinJob& job)
{
    return launch_lds(device, k_bin, dim3(n_theta), dim3(kBinBlock), lds, s, job);
}

int bin_batch(hipStream_t s, int device, int n_theta_max, int n_jobs, size_t lds, const BinJob* jobs)
{
    return launch_lds(device, k_bin_batch, dim3(n_theta_max, n_jobs), dim3(kBinBlock), lds, s, jobs);
}

int zero_if_band(hipStream_t s, int blocks, const ZeroJob& job)
{
    return launch(k_zero_if_band, dim3(blocks, 1), dim3(256), s, job);
}

int zero_if_band_batch(hipStream_t s, int blocks, int n_jobs, const ZeroJob* jobs)
{
    return launch(k_zero_if_band_batch, dim3(blocks, n_jobs), dim3(256), s, jobs);
}

int finalize(hipStream_t s, int device, size_t lds, const FinalJob& job)
{
    return launch_lds(device, k_finalize, dim3(1), dim3(kBlock), lds, s, job);
}

int finalize_batch(hipStream_t s, int device, int n_jobs, size_t lds, const FinalJob* jobs)
{
    return launch_lds(device, k_finalize_batch, dim3(n_jobs), dim3(kBlock), lds, s, jobs);
}

int tie_replay_pick(hipStream_t s, int device, unsigned n, size_t lds, const TieJob& job)
{
    if (int e = launch_lds(device, k_tie_replay, dim3(n), dim3(kBlock), lds, s, job))
        return e;
    return launch(k_tie_pick, dim3(1), dim3(64), s, job);
}

int exact_scores(hipStream_t s, unsigned blocks, const ExactJob& job)
{
    return launch(k_exact_scores, dim3(blocks), dim3(kBlock), s, job);
}

int literal_scan(hipStream_t s, const LiteralJob& job)
{
    return launch(k_csm_literal_scan, dim3(1), dim3(64), s, job);
}

int boxmax_batch(hipStream_t s, dim3 grid, const BoxJob* jobs)
{
    return launch(k_boxmax_batch, grid, dim3(256), s, jobs);
}

int expand_pairs(hipStream_t s, int blocks, const uint16_t* cells, int rows, int cols, int pitch, uint32_t* xg,
                 int prows, int xp, int pad)
{
    return launch(k_expand_pairs, dim3(blocks), dim3(256), s, cells, rows, cols, pitch, reinterpret_cast<uint2*>(xg),
                  prows, xp, pad);
}

int deblock(hipStream_t s, int blocks, const uint16_t* packed, const int32_t* slot, int log2_block, int block_cols,
            int rows, int cols, int pitch, uint16_t* cells, uint8_t* alloc, int n_blocks, int32_t* known_first)
{
    return launch(k_deblock, dim3(blocks), dim3(256), s, packed, slot, log2_block, block_cols, rows, cols, pitch, cells,
                  alloc, n_blocks, known_first);
}

int project(hipStream_t s, dim3 grid, const ProjJob& job)
{
    return launch(k_project, grid, dim3(kBlock), s, job);
}

int project_batch(hipStream_t s, dim3 grid, const ProjJob* jobs)
{
    return launch(k_project_batch, grid, dim3(kBlock), s, jobs);
}

int grid_scores_pick(hipStream_t s, int blocks, const GridSearchJob& job)
{
    if (int e = launch(k_grid_scores, dim3(blocks), dim3(kBlock), s, job))
        return e;
    return launch(k_grid_pick, dim3(blocks), dim3(kBlock), s, job);
}

int scatter_records(hipStream_t s, const csm_result* src, const int32_t* idx, csm_result* dst, int n)
{
    return launch(k_scatter_records, dim3((n + 255) / 256), dim3(256), s, src, idx, dst, n);
}

} /* namespace csm_launch */
