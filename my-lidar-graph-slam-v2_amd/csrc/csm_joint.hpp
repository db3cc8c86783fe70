/* csm_joint.hpp -- the wrappers of csm_joint_kernels.hip (a translation unit of its own): joint
 * two-slice binning, the batched fine kernels that consume it (bound pass, exact pass, exact pass over a
 * work list), the selection between them. Part of the launch layer of csm_launch.hpp: same namespace,
 * same descriptor, same return values. */
#ifndef CSM_JOINT_HPP
#define CSM_JOINT_HPP

#include "csm_launch.hpp"

namespace csm_launch {

/* slots of k_binj's hash table for n_points beams per slice (>= 4/3 * 2 * n_points, any size) and the
 * LDS bytes of k_binj for a frame of `tiles` endpoint tiles with that table */
int binj_hash_size(int n_points);
size_t binj_lds_bytes(int tiles, int n_points, int hash_size);

/* grid = (ceil(max slices / 2), jobs); BinJob.sorted_pb / sorted_rc hold 2 * n_points entries
 * per PAIR of slices, BinJob.tiles max_tiles records per pair, n_tiles one count per pair */
int binj_batch(hipStream_t s, int device, int n_pairs_max, int n_jobs, size_t lds, const BinJob* jobs);

/* k_score_joint_batch, or a.fp32: k_score_jointf_batch, over a.grid = (candidate blocks of this launch,
 * slices, jobs); a.items: the exact kernel over a work list instead (k_score_joint_list: items / count
 * as bound_select wrote them, a.blocks workgroups share them) */
int joint_batch(const ScoreLaunch& a, const ScoreJob* jobs);

/* One window with its jobs by value (no job array in device memory): joint binning over n_pairs pairs of
 * slices, then the exact joint kernel over a.grid.x candidate blocks x n_pairs (grid.y / z, fp32 and the
 * list fields are not used). The coarse pass of a coarse-first search. */
int binj_one(hipStream_t s, int device, int n_pairs, size_t lds, const BinJob& job);
int joint_one(const ScoreLaunch& a, const ScoreJob& job, int n_pairs);

/* After the bound pass (approx_best of every job written): clears every job's BlockBest records and
 * lists the candidate blocks the exact kernel has to score: item = job << 18 | pair << 8 | block;
 * blocks >= split_cb go to items1 (the row block of the R = 6 launch). counts[2] must be zero.
 * round 1: as described; round 2 (two-round exact pass, ScoreJob.round1_record): the blocks not listed
 * in round 1 that can still reach the best eligible key of round 1. */
int bound_select(hipStream_t s, const ScoreJob* jobs, int n_jobs, int ncb, int split_cb, uint32_t* items0,
                 uint32_t* items1, uint32_t* counts, uint32_t cap, int round);

/* Coarse-first window batches. coarse_joint_batch: the strided level of every job (ScoreJob of the level,
 * joint entry lists in sorted_pb) scored node by node straight from the level's cells, every node's exact
 * (S, K) stored to acc_s / acc_k; `nodes` = nx * ny of the level. unit_bounds (fine jobs, after it): the
 * greatest node key over each (slice, candidate block) of the fine plan, rounded up, to approx_best --
 * what bound_select reads in place of the fp32 pass's block maxima; units_max = max slices * ncb, the
 * blocks cbx x cby candidates, ncbx per row of blocks. */
int coarse_joint_batch(hipStream_t s, int nodes, int n_pairs_max, int n_jobs, const ScoreJob* jobs);
int unit_bounds(hipStream_t s, const ScoreJob* jobs, int n_jobs, int units_max, int cbx, int cby, int ncbx, int ncb);

/* xgf = the level's fp32 key copy in the layout of its pair-row copy (k_expand_pairs_f) */
int expand_pairs_f(hipStream_t s, const uint16_t* cells, int rows, int cols, int pitch, float* xgf, int xg_prows,
                   int xg_pitch, int pad);

} /* namespace csm_launch */
#endif
