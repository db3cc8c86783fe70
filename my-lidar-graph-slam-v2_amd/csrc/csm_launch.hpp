/* csm_launch.hpp -- the launch layer between the host code and the kernels. Three translation units
 * hold kernels and the wrappers that launch them, all in namespace csm_launch: csm_launch.hip (this
 * header: the per-slice kernels of csm_kernels.hip -- binning, strided and pair-row scoring, box maximum,
 * finalize, exact paths, projection, grid search), csm_joint_kernels.hip (csm_joint.hpp) and
 * csm_phase_kernels.hip (csm_phase.hpp). The host units (planner, batch staging, C ABI) compile without
 * device code and launch through the wrappers. Every wrapper returns a HIP error code (0 = launched), or
 * -1 where no kernel is instantiated for the requested shape; the host hands that to launched_ok().
 *
 * What the three units share is here too: THE tables of instantiated launch shapes (the planner picks
 * from them, the dispatch expands them), the one launch descriptor, and the helpers the wrappers are
 * written in (match, grant_lds, launch / launch_lds). The units that compile their kernels with their host
 * code (maps, cost, greedy, pose graph, peaks, volume, prior, likelihood, ray check, pose sets) launch through
 * launch / launch_lds directly: no kernel is launched, and no dynamic-LDS limit raised, anywhere else. */
#ifndef CSM_LAUNCH_HPP
#define CSM_LAUNCH_HPP

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <iterator>
#include <map>
#include <mutex>
#include <type_traits>
#include <utility>

#include "csm_device.hpp"
#include "../../include/csm_hip.h"

namespace csm_launch {

using namespace csm;

/* ---- the launch shapes that are instantiated ----
 * One definition each: plan_pass / plan_pass_pairs (csm_plan.hip) choose from these tables and the
 * wrappers dispatch over them, so a shape the planner picks is a shape that is built, and adding one
 * is a one-line change. CSM_FAST_BUILD (tuning builds, tools/build_variant.sh): only the shapes
 * bench.py's configs[1] uses.
 *
 * kPairLS: row pitches of the pair-row and joint kernels = slots per pair row of the LDS region =
 * alignment column + 64-cell tile + cbx - 1 candidates, even (16-byte rows for the LDS-DMA pieces),
 * ascending; a candidate block may be any width cbx <= LS - 65 (124: the conflict-free pitch of R = 6,
 * cbx = 52, the branch-and-bound detector's default window; 156: that of R = 6, cbx = 84, the 36-row
 * tail block of the frontend window). kPairR: their candidate rows per lane, in the planner's order of
 * preference. kStrided*: the strided kernels of the coarser levels, row pitch x rows per lane x stride
 * kind (1 = a power of two, 2 = any). */
#ifdef CSM_FAST_BUILD
inline constexpr int kPairLS[] = { 150, 156 };
inline constexpr int kStridedLS[] = { 192 }, kStridedR[] = { 1 }, kStridedMode[] = { 1 };
#else
inline constexpr int kPairLS[] = { 86, 98, 118, 124, 130, 150, 156, 162, 182 };
inline constexpr int kStridedLS[] = { 128, 192 }, kStridedR[] = { 1, 2, 4 }, kStridedMode[] = { 1, 2 };
#endif
inline constexpr int kPairR[] = { 8, 6 };

/* which scoring kernel instantiation, and how it is launched */
struct ScoreLaunch {
    hipStream_t stream = nullptr;
    int device = 0;
    int lstride = 0, R = 0;
    int mode = 0;               /* strided kernels: 1 = power-of-two stride, 2 = any */
    bool weighted = true;
    int lists = 1;              /* pair batch kernels: 2 = two theta slices per workgroup */
    bool fp32 = false;          /* joint batch kernels: the packed-fp32 bound pass (k_score_jointf_batch) */
    int cbx = 0, groups = 0;
    dim3 grid;                  /* (candidate blocks of this launch, theta slices, jobs [x tile slices]) */
    size_t lds = 0;
    int n_buf = 1, n_slices = 1;
    int theta_major = 0, xcd_map = 0;
    const uint16_t* lane_map = nullptr;
    BlockBase bb = { 0, 0, 0 }; /* where this launch sits among the window's row blocks */
    int ncb = 0;                /* list launches: candidate blocks of the window */
    const uint32_t* items = nullptr;    /* list launches: the work list and its length, on the device */
    const uint32_t* count = nullptr;
    int blocks = 0;             /* list launches: workgroups sharing the list */
};

/* ---- what the wrappers are written in ---- */

template <int V>
using int_c = std::integral_constant<int, V>;

/* Run-time value -> compile-time constant: f(int_c<T[i]>()) for the entry of the constexpr table T that
 * equals v, and what f returned; -1 where T has no such entry (no kernel for that shape). */
template <const auto& T, class F, size_t... I>
int match_entry(int v, F& f, std::index_sequence<I...>)
{
    int rc = -1;
    ((v == T[I] ? (void)(rc = f(int_c<T[I]>())) : (void)0), ...);
    return rc;
}

template <const auto& T, class F>
int match(int v, F f)
{
    return match_entry<T>(v, f, std::make_index_sequence<std::size(T)>());
}

/* f(int_c<LS>, int_c<R>) of a pair-row or joint launch; f(int_c<LS>, int_c<R>, int_c<MODE>) of a strided one */
template <class F>
int match_pair_shape(const ScoreLaunch& a, F f)
{
    return match<kPairLS>(a.lstride, [&](auto ls) { return match<kPairR>(a.R, [&](auto r) { return f(ls, r); }); });
}

template <class F>
int match_strided_shape(const ScoreLaunch& a, F f)
{
    return match<kStridedLS>(a.lstride, [&](auto ls) {
        return match<kStridedR>(a.R, [&](auto r) {
            return match<kStridedMode>(a.mode, [&](auto mode) { return f(ls, r, mode); });
        });
    });
}

/* Dynamic LDS above 64 KB needs the function attribute. It is a driver call and
 * it belongs to the function on a device, not to a context: one process-wide
 * table, only ever raised (a smaller value set by another context would make
 * a larger launch of this one fail). Inline with function-local statics: one table
 * in the library, whichever translation unit asks. */
inline hipError_t grant_lds(int device, const void* fn, size_t bytes)
{
    if (bytes <= 64 * 1024)
        return hipSuccess;
    static std::mutex guard;
    static std::map<std::pair<int, const void*>, size_t> granted;
    std::lock_guard<std::mutex> lock(guard);
    size_t& have = granted[{ device, fn }];
    if (bytes > have) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess)
            return e;
        have = bytes;
    }
    return hipSuccess;
}

/* One kernel launch and its error code; launch_lds: with dynamic LDS, granted first. */
template <class... P, class... A>
int launch_lds(int device, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, const A&... args)
{
    const hipError_t e = grant_lds(device, reinterpret_cast<const void*>(kernel), lds);
    if (e != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
    return (int)hipGetLastError();
}

template <class... P, class... A>
int launch(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t s, const A&... args)
{
    hipLaunchKernelGGL(kernel, grid, block, 0, s, args...);
    return (int)hipGetLastError();
}

/* A chain of launches that is checked once, where it ends: `e` keeps the first code that is not 0. */
inline void keep_first(int& e, int code)
{
    if (!e)
        e = code;
}

/* ---- the wrappers of csm_launch.hip ---- */

/* the scoring kernels; grid.y counts theta slices: the kernels that take two per workgroup
 * (pair batch with lists == 2, joint batch) are launched over ceil(grid.y / 2) */
int score_strided(const ScoreLaunch& a, const ScoreJob& job);             /* k_score<LS, R, MODE> */
int score_strided_batch(const ScoreLaunch& a, const ScoreJob* jobs);      /* k_score_batch */
int score_pairs(const ScoreLaunch& a, const ScoreJob& job);               /* k_score_pairs */
int score_pairs_batch(const ScoreLaunch& a, const ScoreJob* jobs);        /* k_score_pairs_batch / pairs2_batch */
int score_pairs_list(const ScoreLaunch& a, const ScoreJob& job);          /* k_score_pairs_list */
int argmax(const ScoreLaunch& a, const ScoreJob& job, uint32_t* sum_s, uint32_t* sum_k);    /* k_argmax<R> */

/* the other kernels: grid / block / dynamic LDS as the caller decides; those that take `device` and
 * `lds` raise the kernel's dynamic-LDS limit first (grant_lds) */
int bin(hipStream_t s, int device, int n_theta, size_t lds, const BinJob& job);
int bin_batch(hipStream_t s, int device, int n_theta_max, int n_jobs, size_t lds, const BinJob* jobs);
int zero_if_band(hipStream_t s, int blocks, const ZeroJob& job);
int zero_if_band_batch(hipStream_t s, int blocks, int n_jobs, const ZeroJob* jobs);
int finalize(hipStream_t s, int device, size_t lds, const FinalJob& job);
int finalize_batch(hipStream_t s, int device, int n_jobs, size_t lds, const FinalJob* jobs);
int tie_replay_pick(hipStream_t s, int device, unsigned n, size_t lds, const TieJob& job);
int exact_scores(hipStream_t s, unsigned blocks, const ExactJob& job);
int literal_scan(hipStream_t s, const LiteralJob& job);
int boxmax_batch(hipStream_t s, dim3 grid, const BoxJob* jobs);
int expand_pairs(hipStream_t s, int blocks, const uint16_t* cells, int rows, int cols, int pitch, uint32_t* xg,
                 int prows, int xp, int pad);
int deblock(hipStream_t s, int blocks, const uint16_t* packed, const int32_t* slot, int log2_block, int block_cols,
            int rows, int cols, int pitch, uint16_t* cells, uint8_t* alloc, int n_blocks, int32_t* known_first);
int project(hipStream_t s, dim3 grid, const ProjJob& job);
int project_batch(hipStream_t s, dim3 grid, const ProjJob* jobs);
int grid_scores_pick(hipStream_t s, int blocks, const GridSearchJob& job);
int scatter_records(hipStream_t s, const csm_result* src, const int32_t* idx, csm_result* dst, int n);

} /* namespace csm_launch */
#endif
