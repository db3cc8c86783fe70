/* csm_window.hip -- one search window at a time (host code only): three launch chains over the stages of
 * WindowRun (run_exhaustive; the coarse-first search_window of large windows = run_level_pass, then
 * run_fine_under_level), tie / literal resolution, and the single-query entry points of the C ABI, the
 * only names visible outside: csm_score_window*, csm_correlative_match (query block, graph cache,
 * uncertified projection entries), csm_grid_search_match, csm_project_scan. */
#include "csm_matchers.hpp"
#include "csm_certify.hpp"

namespace {

/* Every candidate's sums of a scored level, [n_theta][nxs][nys]: the eligibility of the level below. */
struct StoredLevel {
    uint32_t *s = nullptr, *k = nullptr;
    int nxs = 0, nys = 0;
};

/* Can the level pass run on JOINT entries of slice pairs (k_binj_one + k_score_joint_one)? On the
 * phase-major copy a tile holds the beams of one phase only (configs[4]: ~6 entries per staged window
 * against ~53 at the fine level), so the pass is bound by staging, and a pair of neighbouring slices
 * shares every staged window. Not where the joint tables do not fit (then: the per-slice pair kernel). */
bool joint_level_plan(const csm_ctx* ctx, const Plan& p, PassPlan* jp)
{
    if (!ctx->tune.joint || !ctx->tune.two_slices || !p.fine.pairs || p.L != 1)
        return false;
    const size_t binj_lds = csm_launch::binj_lds_bytes(p.tiles_x * p.tiles_y, p.n, csm_launch::binj_hash_size(p.n));
    /* the exact joint kernel keeps kJRec entry words next to the window copy (not two kPbMax lists) */
    if (binj_lds > 150 * 1024 || !plan_pass_pairs(ctx->tune, p.nx, p.ny, jp, true, kJRec * 4) || jp->lists != 2)
        return false;
    jp->joint = true;
    jp->weighted = true;
    return true;
}

/* Tile-split fine launch when the window gives fewer than ~1.5 workgroups per CU (config 2: 246);
 * CSM_TUNE_NO_TILE_SPLIT: never. *fine_slices > 1: the accumulators are sized and zero. */
int tile_split_slices(csm_ctx* ctx, const Plan& p, int* fine_slices)
{
    int rc;
    const long blocks = (long)p.fine.ncb() * p.n_theta;
    *fine_slices = 1;
    if (blocks < 384)
        *fine_slices = (int)std::min<long>(4, std::max<long>(1, 492 / std::max<long>(1, blocks)));
    if (!ctx->tune.tile_split)
        *fine_slices = 1;
    else if (ctx->tune.fine_slices)
        *fine_slices = std::max(1, std::min(8, ctx->tune.fine_slices));
    if (*fine_slices <= 1)
        return CSM_OK;
    /* the accumulators are zero between queries: cleared once when
     * (re)allocated, then by the arg-max pass as it reads them. A buffer that grew is told by its
     * capacity: the allocator may hand the freed address out again, with other contents behind it */
    const size_t words = (size_t)p.n_theta * p.nx * p.ny;
    const size_t old_s = ctx->fine_s.cap, old_k = ctx->fine_k.cap;
    if ((rc = ensure(ctx, ctx->fine_s, words * 4))) return rc;
    if ((rc = ensure(ctx, ctx->fine_k, words * 4))) return rc;
    if (ctx->fine_s.cap != old_s || ctx->fine_acc_dirty)
        HIP_TRY(ctx, hipMemsetAsync(ctx->fine_s.p, 0, ctx->fine_s.cap, ctx->stream));
    if (ctx->fine_k.cap != old_k || ctx->fine_acc_dirty)
        HIP_TRY(ctx, hipMemsetAsync(ctx->fine_k.p, 0, ctx->fine_k.cap, ctx->stream));
    ctx->fine_acc_dirty = false;
    return CSM_OK;
}

/* One window's launch chain in the making: what its stages share. A driver calls the stages it
 * needs top to bottom; each stage queues its work on ctx->stream and returns a CSM_* code. */
struct WindowRun {
    csm_ctx* ctx;
    DeviceGrid& g;
    const csm_window* w;
    const Plan& p;
    const int32_t *hit_col, *hit_row;   /* device */
    uint32_t *flags = nullptr, *flags_next = nullptr;   /* this chain's flag word; the word its finalize clears for the next */
    BinJob bj;                          /* the entry lists the scoring stages read (bin, bin_joint) */

    /* The window's level checked, then the workspaces every chain sizes for its window (a graph is
     * recorded on a shape's third query: by then none may grow). */
    int workspaces()
    {
        if (w->coarse_level < 0 || w->coarse_level >= (int)g.levels.size())
            return fail(ctx, CSM_ENOENT, "coarse level %d not built", w->coarse_level);
        if (g.levels[w->coarse_level].stale)
            return fail(ctx, CSM_ENOENT, "coarse level %d is stale: the map was rebuilt", w->coarse_level);
        if (g.levels[w->coarse_level].win != p.L)
            return fail(ctx, CSM_EINVAL, "level %d holds box-max(%d), window asks L=%d",
                        w->coarse_level, g.levels[w->coarse_level].win, p.L);
        int rc;
        const size_t nt = p.n_theta;
        if ((rc = ensure(ctx, ctx->sorted, nt * p.n * 4 + 256))) return rc;   /* + 64 entries: the LDS-DMA of a
                                                                                 tile's list reads whole 64-entry pieces */
        if (p.fine.pairs && (rc = ensure_xgrid(ctx, g, xgrid_pad_for(p.nx, p.ny)))) return rc;
        if ((rc = ensure(ctx, ctx->tiles, nt * p.max_tiles * sizeof(TileRec)))) return rc;
        if ((rc = ensure(ctx, ctx->ntiles, nt * 8))) return rc;
        if ((rc = ensure(ctx, ctx->misc, 256))) return rc;
        if ((rc = ensure(ctx, ctx->coarse_s, nt * p.nxc * p.nyc * 4))) return rc;
        if ((rc = ensure(ctx, ctx->coarse_k, nt * p.nxc * p.nyc * 4))) return rc;
        if ((rc = ensure(ctx, ctx->best, nt * p.fine.ncb() * sizeof(BlockBest)))) return rc;
        return ensure(ctx, ctx->sorted_rc, nt * p.n * 4);
    }

    /* Two flag words of ctx->misc used alternately: k_finalize of query i clears the word of query
     * i + 1, so only a chain that ends in a finalize moves on to the next word. */
    int take_flags(bool finalize_follows)
    {
        uint32_t* flag_words = reinterpret_cast<uint32_t*>(ctx->misc.p);
        if (!ctx->flags_ready && !ctx->capturing) {
            HIP_TRY(ctx, hipMemsetAsync(flag_words, 0, 16, ctx->stream));
            ctx->flags_ready = true;
        }
        flags = flag_words + (ctx->flag_toggle & 1u);
        flags_next = flag_words + ((ctx->flag_toggle + 1u) & 1u);
        if (ctx->capturing) {
            /* a graph bakes its pointers: a flag word of its own, cleared by a node of the graph */
            flags = flag_words + 2;
            flags_next = nullptr;
            HIP_TRY(ctx, hipMemsetAsync(flags, 0, 4, ctx->stream));
        } else if (finalize_follows) {
            ctx->flag_toggle++;
        }
        return CSM_OK;
    }

    /* Per-slice entry lists (row pairs for the pair-row fine kernel); L > 1: also the coarse level's
     * lists and the edge-band flag. */
    int bin()
    {
        bj = bin_job(g, p, p.n_theta, p.n, p.max_tiles, hit_col, hit_row, ctx->sorted.as<uint32_t>(),
                     ctx->tiles.as<TileRec>(), ctx->ntiles.as<int32_t>(), flags, p.fine.pairs ? 1 : 0);
        bj.hash_size = bin_hash_size(p.n);
        bj.max_mult = p.fine.weighted ? kMaxMult : 1;
        bj.lstride = p.fine.lstride;
        bj.sorted_rc = p.L > 1 ? ctx->sorted_rc.as<uint32_t>() : nullptr;
        if (p.L > 1) {
            bj.n_band = 1;
            bj.band_win[0] = p.L;
            bj.band_nx[0] = p.nxc;
            bj.band_ny[0] = p.nyc;
        }
        ScopedTimer tm(ctx, "bin");
        return launched_ok(ctx, csm_launch::bin(ctx->stream, ctx->device, p.n_theta,
                                                bin_lds_bytes(p.tiles_x * p.tiles_y, p.n), bj), "binning");
    }

    /* Joint entry lists of slice pairs, for score_joint. */
    int bin_joint(const PassPlan& jp)
    {
        int rc;
        const int n_pairs = (p.n_theta + 1) / 2;
        const int max_tiles = std::min(2 * p.n, p.tiles_x * p.tiles_y) + 2 * p.n / kJRec + 1;
        if ((rc = ensure(ctx, ctx->sorted, (size_t)n_pairs * 2 * p.n * 4 + 256))) return rc;
        if ((rc = ensure(ctx, ctx->tiles, (size_t)n_pairs * max_tiles * sizeof(TileRec)))) return rc;
        if ((rc = ensure(ctx, ctx->ntiles, (size_t)n_pairs * 8))) return rc;
        bj = bin_job(g, p, p.n_theta, p.n, max_tiles, hit_col, hit_row, ctx->sorted.as<uint32_t>(),
                     ctx->tiles.as<TileRec>(), ctx->ntiles.as<int32_t>(), flags, 2);
        bj.hash_size = csm_launch::binj_hash_size(p.n);
        bj.max_mult = kMaxMult;
        bj.lstride = jp.lstride;
        const size_t lds = csm_launch::binj_lds_bytes(p.tiles_x * p.tiles_y, p.n, bj.hash_size);
        ScopedTimer tm(ctx, "bin");
        return launched_ok(ctx, csm_launch::binj_one(ctx->stream, ctx->device, n_pairs, lds, bj), "joint binning");
    }

    /* The coarse level of an exhaustive window (L > 1), its sums into ctx->coarse_s / coarse_k. With
     * `exits` it only runs when a beam reaches the edge band (rare). */
    int coarse(bool exits)
    {
        /* the coarse pass accumulates with atomics: its sums are cleared first, but
         * only when it is going to run (k_zero_if_band reads the band flag k_bin set) */
        const ZeroJob zj = { ctx->coarse_s.as<uint32_t>(), ctx->coarse_k.as<uint32_t>(),
                             (size_t)p.n_theta * p.nxc * p.nyc, flags, exits ? 0 : 1, 0 };
        const int zb = (int)std::min<size_t>(256, (zj.words + 255) / 256);
        if (int rc = launched_ok(ctx, csm_launch::zero_if_band(ctx->stream, std::max(1, zb), zj), "edge-band clear")) return rc;
        ScoreJob cj = score_job(g, g.levels[w->coarse_level].cells, p.L, bj, w->min_known);
        cj.sorted_pb = bj.sorted_rc;
        cj.acc_s = ctx->coarse_s.as<uint32_t>();
        cj.acc_k = ctx->coarse_k.as<uint32_t>();
        cj.rank_l = 1;
        cj.skip_unless_band = exits;
        ScopedTimer tm(ctx, "score_coarse");
        /* few candidates per slice: split the tile list over blockIdx.z so enough workgroups are in flight
         * to hide the staging latency -- unless the pass only runs when a beam reaches the edge band
         * (rare): then one slice, so that the launch that normally exits at once stays small */
        return launch_score(ctx, cj, p.coarse, p.n_theta, exits ? 1 : kCoarseSlices);
    }

    /* THE fine-level job over the entry lists of bj; the caller sets where its results go. L > 1: only
     * candidates under an eligible node of `elig` (only_if_band: consulted only when a beam reaches the band). */
    ScoreJob fine_job(const StoredLevel& elig, bool only_if_band) const
    {
        ScoreJob fj = score_job(g, g.levels[0].cells, 1, bj, w->min_known);
        fj.xg = g.xg.as<uint32_t>();
        fj.xg_pitch = g.xg_pitch;
        fj.xg_pad = g.xg_pad;
        fj.rank_l = p.L;
        if (p.L > 1) {
            fj.n_elig = 1;
            fj.elig[0].k = elig.k;
            fj.elig[0].s = elig.s;
            fj.elig[0].div = p.L;
            fj.elig[0].nxc = elig.nxs;
            fj.elig[0].nyc = elig.nys;
            fj.elig_only_if_band = only_if_band;
        } else {
            fj.check_own_known = 1;
        }
        return fj;
    }

    /* Small windows: too few workgroups to fill the chip, so the tile list is split over blockIdx.z,
     * the slices add their exact integer sums with atomics, and a second pass does the arg-max. */
    int score_tile_split(const ScoreJob& fj, int fine_slices)
    {
        int rc;
        ScoreJob sj = fj;
        sj.block_best = nullptr;
        sj.dump_s = nullptr;
        sj.dump_k = nullptr;
        sj.acc_s = ctx->fine_s.as<uint32_t>();
        sj.acc_k = ctx->fine_k.as<uint32_t>();
        sj.acc_x_major = 1;
        ctx->fine_acc_dirty = true;
        {
            ScopedTimer tm(ctx, "score_fine");
            if ((rc = launch_score(ctx, sj, p.fine, p.n_theta, fine_slices)))
                return rc;
        }
        ScopedTimer tm(ctx, "argmax");
        if ((rc = launch_argmax(ctx, fj, p.fine, p.n_theta, sj.acc_s, sj.acc_k)))
            return rc;
        ctx->fine_acc_dirty = false;
        return CSM_OK;
    }

    /* The work list (J.items, J.count of J.cap): the blocks whose coarse bound reaches the best fine key under
     * the best coarse node. ctx->tp_items = [best pair | count | pad to 64][*reduced records][items][keep bytes]. */
    int select_blocks(const StoredLevel& level, csm::TwoPhaseJob& J, BlockBest** reduced)
    {
        const size_t n_blocks = (size_t)p.n_theta * p.fine.ncb();
        if (int rc = ensure(ctx, ctx->tp_items, 64 + csm::kReducedBest * sizeof(BlockBest) + n_blocks * 5))
            return rc;
        std::memset(&J, 0, sizeof(J));
        J.best = ctx->tp_items.as<unsigned long long>();
        J.count = reinterpret_cast<uint32_t*>(J.best + 2);
        *reduced = reinterpret_cast<BlockBest*>(ctx->tp_items.as<char>() + 64);
        J.items = reinterpret_cast<uint32_t*>(*reduced + csm::kReducedBest);
        J.keep = reinterpret_cast<unsigned char*>(J.items + n_blocks);
        J.cap = (uint32_t)n_blocks;
        HIP_TRY(ctx, hipMemsetAsync(ctx->tp_items.p, 0, 64, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(J.keep, 0, n_blocks, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(ctx->best.p, 0, n_blocks * sizeof(BlockBest), ctx->stream));
        J.coarse_s = level.s;
        J.coarse_k = level.k;
        J.n_theta = p.n_theta;
        J.nxc = p.nxc;
        J.nyc = p.nyc;
        J.nxs = level.nxs;
        J.nys = level.nys;
        J.L = p.L;
        J.min_known = w->min_known;
        J.cells = g.levels[0].cells;
        J.rows = g.rows;
        J.cols = g.cols;
        J.pitch = g.pitch;
        J.hit_col = hit_col;
        J.hit_row = hit_row;
        J.n_points = p.n;
        J.x_lo = p.x_lo;
        J.y_lo = p.y_lo;
        J.nx = p.nx;
        J.ny = p.ny;
        J.cbx = p.fine.cbx;
        J.cby = p.fine.groups * p.fine.R;
        J.ncbx = p.fine.ncbx;
        J.ncb = p.fine.ncb();
        J.flags = flags;
        ScopedTimer tm(ctx, "select");
        int e = csm_launch::coarse_best(ctx->stream, J);
        if (!e) e = csm_launch::fine_under_best(ctx->stream, J);
        if (!e) e = csm_launch::mark_blocks(ctx->stream, J);
        return launched_ok(ctx, e, "two-phase select");
    }

    /* The window's record from n_records block records of the fine job; clears the next chain's flag word. */
    int finalize(const ScoreJob& fj, const BlockBest* records, int n_records, csm_result* out_dev)
    {
        FinalJob fin = final_job(fj, n_records, hit_col, hit_row, w->score_threshold, ctx->lut_dev.as<double>(), out_dev);
        fin.block_best = records;
        fin.flags_clear = flags_next;
        ScopedTimer tm(ctx, "finalize");
        return launched_ok(ctx, csm_launch::finalize(ctx->stream, ctx->device, (size_t)p.n * 8, fin), "finalize");
    }
};

/* The exhaustive chain: every candidate at the fine level (L > 1: under an eligible node of the coarse
 * level, scored first). force_coarse: the coarse level always runs (csm_score_window_dump reads its sums). */
int run_exhaustive(csm_ctx* ctx, DeviceGrid& g, const csm_window* w, const Plan& p, const int32_t* hit_col,
                   const int32_t* hit_row, csm_result* out_dev, uint32_t* dump_s = nullptr,
                   uint16_t* dump_k = nullptr, bool force_coarse = false)
{
    WindowRun r = { ctx, g, w, p, hit_col, hit_row };
    int rc, fine_slices = 1;
    if ((rc = r.workspaces())) return rc;
    if ((rc = tile_split_slices(ctx, p, &fine_slices))) return rc;
    if ((rc = r.take_flags(true))) return rc;
    if ((rc = r.bin())) return rc;
    const bool coarse_exits = w->min_known <= 1 && !force_coarse;   /* unless a beam reaches the band */
    if (p.L > 1 && (rc = r.coarse(coarse_exits))) return rc;
    ScoreJob fj = r.fine_job({ ctx->coarse_s.as<uint32_t>(), ctx->coarse_k.as<uint32_t>(), p.nxc, p.nyc }, coarse_exits);
    fj.block_best = ctx->best.as<BlockBest>();
    fj.dump_s = dump_s;
    fj.dump_k = dump_k;
    if (fine_slices > 1) {
        if ((rc = r.score_tile_split(fj, fine_slices))) return rc;
    } else {
        ScopedTimer tm(ctx, "score_fine");
        if ((rc = launch_score(ctx, fj, p.fine, p.n_theta, 1))) return rc;
    }
    ctx->last_run.fine = fj;
    return r.finalize(fj, fj.block_best, p.n_theta * p.fine.ncb(), out_dev);
}

/* The level pass: the window (one of L = 1, on a phase-major copy) scored and every candidate's
 * sums STORED as *level in ctx->coarse_s / coarse_k; no arg-max, no record, so no flag to pass on. */
int run_level_pass(csm_ctx* ctx, DeviceGrid& g, const csm_window* w, const Plan& p, const int32_t* hit_col,
                   const int32_t* hit_row, StoredLevel* level)
{
    WindowRun r = { ctx, g, w, p, hit_col, hit_row };
    int rc;
    PassPlan jp;
    if ((rc = r.workspaces())) return rc;
    if ((rc = r.take_flags(false))) return rc;
    const bool joint = joint_level_plan(ctx, p, &jp);
    if ((rc = joint ? r.bin_joint(jp) : r.bin())) return rc;
    *level = { ctx->coarse_s.as<uint32_t>(), ctx->coarse_k.as<uint32_t>(), p.nx, p.ny };
    ScoreJob fj = r.fine_job(StoredLevel(), false);
    fj.joint = joint;
    fj.check_own_known = 0;
    fj.acc_s = level->s;
    fj.acc_k = level->k;
    fj.acc_x_major = 2;
    const uint16_t* lane_map = nullptr;
    if (joint && (rc = lane_map_for(ctx, jp, &lane_map))) return rc;
    ScopedTimer tm(ctx, "score_coarse");
    if (!joint)
        return launch_score(ctx, fj, p.fine, p.n_theta, 1);
    csm_launch::ScoreLaunch a = score_launch(ctx, jp, dim3(jp.ncb(), 1, 1), pass_lds_bytes(jp));
    a.lane_map = lane_map;
    a.bb = BlockBase{ 0, 0, jp.ncb() };
    return launched_ok(ctx, csm_launch::joint_one(a, fj, (p.n_theta + 1) / 2), "joint level pass");
}

/* The fine level of a large window (L > 1) under a stored level: eligibility from the level's
 * sums, only the blocks of the work list scored, the record from kReducedBest reduced records. */
int run_fine_under_level(csm_ctx* ctx, DeviceGrid& g, const csm_window* w, const Plan& p, const int32_t* hit_col,
                         const int32_t* hit_row, const StoredLevel& level, csm_result* out_dev)
{
    WindowRun r = { ctx, g, w, p, hit_col, hit_row };
    int rc;
    csm::TwoPhaseJob list;
    BlockBest* reduced = nullptr;
    if ((rc = r.workspaces())) return rc;
    if ((rc = r.take_flags(true))) return rc;
    if ((rc = r.bin())) return rc;
    ScoreJob fj = r.fine_job(level, false);
    fj.block_best = ctx->best.as<BlockBest>();
    if (p.fine.ncb() > 4096 || (size_t)p.n_theta * level.nxs * level.nys >= (1u << 26) || p.n > 4096)
        return fail(ctx, CSM_EINVAL, "internal: window too large for the two-phase work list");
    if ((rc = r.select_blocks(level, list, &reduced))) return rc;
    {
        ScopedTimer tm(ctx, "score_fine");
        if ((rc = launch_score_list(ctx, fj, p.fine, list.items, list.count, (int)std::min<uint32_t>(list.cap, 2048))))
            return rc;
    }
    /* k_finalize reads kReducedBest records instead of one per block of the window */
    if ((rc = launched_ok(ctx, csm_launch::reduce_items(ctx->stream, fj.block_best, list.items, list.count,
                                                         list.cap, p.fine.ncb(), reduced),
                          "record reduction")))
        return rc;
    ctx->last_run.fine = fj;
    ctx->last_run.coarse_nodes = (int64_t)p.n_theta * p.nxc * p.nyc;
    ctx->last_run.fine_candidates = -1;           /* from the device counters, on request (csm_last_search_info) */
    ctx->last_run.kept_dev = list.count;
    ctx->last_run.blocks_total = (int64_t)list.cap;
    ctx->last_run.block_candidates = (int64_t)p.fine.cbx * p.fine.groups * p.fine.R;
    return r.finalize(fj, reduced, csm::kReducedBest, out_dev);
}

/* The phase-major copy of box-max level `level` of g for coarse windows of up to `need` candidates
 * per axis (its zero padding), built on first use and whenever the level changed. */
int ensure_phase_map(csm_ctx* ctx, DeviceGrid& g, int level, int need, PhaseMap** out)
{
    const int L = g.levels[level].win;
    PhaseMap& pm = g.phase[L];
    const uint16_t* src = g.levels[level].cells;
    if (pm.grid && pm.built_from == src && pm.from_rows == g.rows && pm.from_cols == g.cols &&
        pm.from_pitch == g.pitch && pm.epoch == g.base_epoch && pm.pad >= need + 2) {
        *out = &pm;
        return CSM_OK;
    }
    const int pad = std::max(need + 2, pm.pad);
    const int rows_c = ceil_div(g.rows, L), cols_c = ceil_div(g.cols, L);
    const int hp = rows_c + 2 * pad, wp = cols_c + 2 * pad;
    if (!pm.grid)
        pm.grid.reset(new DeviceGrid());
    DeviceGrid& pg = *pm.grid;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    free_levels(pg, false);
    pg.rows = L * hp;
    pg.cols = L * wp;
    pg.pitch = (pg.cols + 7) & ~7;
    pg.known_r0 = 0;
    pg.known_c0 = 0;
    Level base;
    const size_t bytes = (size_t)pg.rows * pg.pitch * 2;
    if (int rc = grow(ctx, base.own, bytes, bytes, false))
        return rc;
    base.cells = base.own.as<uint16_t>();
    pg.levels.push_back(std::move(base));
    if (int rc = launched_ok(ctx, csm_launch::phase_map(ctx->stream, src, g.rows, g.cols, g.pitch, L, hp, wp, pad,
                                                         pg.levels[0].cells, pg.pitch), "phase-major copy"))
        return rc;
    pm.hp = hp;
    pm.wp = wp;
    pm.pad = pad;
    pm.built_from = src;
    pm.from_rows = g.rows;
    pm.from_cols = g.cols;
    pm.from_pitch = g.pitch;
    pm.epoch = g.base_epoch;
    *out = &pm;
    return CSM_OK;
}

/* Is this window searched coarse-first? Large windows only (the coarse pass, the selection and a
 * second binning cost more than they save on a window the exhaustive kernel finishes in 50 us). */
bool wants_two_phase(const csm_ctx* ctx, const Plan& p)
{
    if (ctx->tune.two_phase < 0 || p.L < 2 || !p.fine.pairs || p.fine.ncb() > 4096 || p.n > 4096)
        return false;
    const size_t nodes = (size_t)p.n_theta * (p.nxc + 1) * (p.nyc + 1);
    if (nodes >= (1u << 26))
        return false;
    return ctx->tune.two_phase > 0 || (double)p.n_theta * p.nx * p.ny >= 3.0e7;
}

/* ctx->last_run of an exhaustive search of the window (its fine job: set by the chain, or restored
 * from the recorded graph). */
void note_exhaustive_search(csm_ctx* ctx, const Plan& p)
{
    ctx->last_run.nominal = (int64_t)p.n_theta * p.nx * p.ny;
    ctx->last_run.coarse_nodes = 0;
    ctx->last_run.fine_candidates = ctx->last_run.nominal;
    ctx->last_run.kept_dev = nullptr;
}

/* One window, device-resident hit indices: exhaustive, or coarse-first (the level pass on the
 * phase-major copy of the coarse level, then the fine level under what it stored). */
int search_window(csm_ctx* ctx, DeviceGrid& g, const csm_window* w, const Plan& p, const int32_t* col_dev,
                  const int32_t* row_dev, csm_result* out_dev)
{
    note_exhaustive_search(ctx, p);
    if (!wants_two_phase(ctx, p))
        return run_exhaustive(ctx, g, w, p, col_dev, row_dev, out_dev);
    int rc;
    PhaseMap* pm = nullptr;
    if ((rc = ensure_phase_map(ctx, g, w->coarse_level, std::max(p.nxc, p.nyc) + 1, &pm))) return rc;
    /* the coarse window on the phase-major copy: candidate (xc, yc) = offsets (xc - wcx, yc - wcy) */
    csm_window wc = *w;
    wc.win_x = p.nxc / 2;
    wc.win_y = p.nyc / 2;
    wc.low_resolution = 1;
    wc.coarse_level = 0;
    Plan pc;
    if ((rc = make_plan(ctx, *pm->grid, &wc, &pc))) return rc;
    const size_t hn = (size_t)p.n_theta * p.n;
    if ((rc = ensure(ctx, ctx->ph_hits, hn * 8 + 256))) return rc;
    int32_t* pcol = reinterpret_cast<int32_t*>(ctx->ph_hits.p);
    int32_t* prow = pcol + hn;
    {
        ScopedTimer tm(ctx, "project");
        if ((rc = launched_ok(ctx, csm_launch::phase_hits(ctx->stream, col_dev, row_dev, hn, p.x_lo, p.y_lo, p.L, pm->hp,
                                                          pm->wp, pm->pad, ceil_div(g.rows, p.L), ceil_div(g.cols, p.L),
                                                          wc.win_x, wc.win_y, pcol, prow), "phase hits")))
            return rc;
    }
    StoredLevel level;
    if ((rc = run_level_pass(ctx, *pm->grid, &wc, pc, pcol, prow, &level))) return rc;
    return run_fine_under_level(ctx, g, w, p, col_dev, row_dev, level, out_dev);
}

const uint32_t kTieCap = 1u << 16;
const uint32_t kUncCap = 4096;

/* Several candidates share the best integer key: collect them with a second
 * fine pass, replay each in f64, pick like the reference's strict `<`. */
int resolve_ties(csm_ctx* ctx, DeviceGrid& g, const csm_window* w, const Plan& p,
                 const int32_t* col_dev, const int32_t* row_dev, csm_result* out_dev)
{
    int rc;
    if ((rc = ensure(ctx, ctx->tie, (size_t)kTieCap * 16 + 64))) return rc;
    unsigned long long* list = reinterpret_cast<unsigned long long*>(ctx->tie.p);
    double* score = reinterpret_cast<double*>(list + kTieCap);
    uint32_t* count = reinterpret_cast<uint32_t*>(score + kTieCap);
    HIP_TRY(ctx, hipMemsetAsync(count, 0, 4, ctx->stream));
    ScoreJob cj = ctx->last_run.fine;
    cj.block_best = nullptr;
    cj.dump_s = nullptr;
    cj.dump_k = nullptr;
    cj.collect_key = reinterpret_cast<const unsigned long long*>(
        reinterpret_cast<const char*>(out_dev) + offsetof(csm_result, key));
    cj.tie_list = list;
    cj.tie_count = count;
    cj.tie_cap = kTieCap;
    if ((rc = launch_score(ctx, cj, p.fine, p.n_theta, 1)))
        return rc;
    TieJob tj;
    std::memset(&tj, 0, sizeof(tj));
    tj.tie_list = list;
    tj.tie_count = count;
    tj.tie_cap = kTieCap;
    tj.tie_score = score;
    tj.nx = p.nx;
    tj.ny = p.ny;
    tj.rank_l = p.L;
    tj.x_lo = p.x_lo;
    tj.y_lo = p.y_lo;
    tj.win_theta = (p.n_theta - 1) / 2;
    tj.cells = g.levels[0].cells;
    tj.rows = g.rows;
    tj.cols = g.cols;
    tj.pitch = g.pitch;
    tj.hit_col = col_dev;
    tj.hit_row = row_dev;
    tj.n_points = p.n;
    tj.score_thr = w->score_threshold;
    tj.lut = ctx->lut_dev.as<double>();
    tj.out = out_dev;
    uint32_t n = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&n, count, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    n = std::min(n, kTieCap);
    if (n == 0)
        return CSM_OK;
    const size_t lds = (size_t)p.n * 8;
    return launched_ok(ctx, csm_launch::tie_replay_pick(ctx->stream, ctx->device, (unsigned)n, lds, tj), "tie replay");
}

/* The reference's sequential sweep over device-computed exact scores: used
 * when some coarse node fails to bound its fine candidates (negative edge
 * band) or the tie list overflows. */
int resolve_literal(csm_ctx* ctx, DeviceGrid& g, const csm_window* w, const Plan& p,
                    const int32_t* col_dev, const int32_t* row_dev, csm_result* out_dev)
{
    int rc;
    const size_t nf = (size_t)p.n_theta * p.nx * p.ny;
    const size_t nc = (size_t)p.n_theta * p.nxc * p.nyc;
    if ((rc = ensure(ctx, ctx->ex_fine, nf * 8))) return rc;
    if ((rc = ensure(ctx, ctx->ex_fine_k, nf * 4))) return rc;
    if ((rc = ensure(ctx, ctx->ex_coarse, nc * 8))) return rc;
    if ((rc = ensure(ctx, ctx->ex_coarse_k, nc * 4))) return rc;
    auto exact = [&](const uint16_t* cells, int nx, int ny, int stride, size_t n, DevBuf& score, DevBuf& known) {
        ExactJob j = exact_job(g, cells, p.n_theta, p.n, p.x_lo, p.y_lo, nx, ny, stride, ctx->lut_dev.as<double>(),
                               score.as<double>(), known.as<uint32_t>());
        j.hit_col = col_dev;
        j.hit_row = row_dev;
        return launched_ok(ctx, csm_launch::exact_scores(ctx->stream, (unsigned)((n + kBlock - 1) / kBlock), j), "exact score");
    };
    if ((rc = exact(g.levels[w->coarse_level].cells, p.nxc, p.nyc, p.L, nc, ctx->ex_coarse, ctx->ex_coarse_k))) return rc;
    if ((rc = exact(g.levels[0].cells, p.nx, p.ny, 1, nf, ctx->ex_fine, ctx->ex_fine_k))) return rc;
    LiteralJob lj;
    std::memset(&lj, 0, sizeof(lj));
    lj.coarse_score = ctx->ex_coarse.as<double>();
    lj.coarse_k = ctx->ex_coarse_k.as<uint32_t>();
    lj.fine_score = ctx->ex_fine.as<double>();
    lj.n_theta = p.n_theta;
    lj.nxc = p.nxc;
    lj.nyc = p.nyc;
    lj.L = p.L;
    lj.x_lo = p.x_lo;
    lj.y_lo = p.y_lo;
    lj.win_theta = (p.n_theta - 1) / 2;
    lj.min_known = w->min_known;
    lj.score_thr = w->score_threshold;
    lj.out = out_dev;
    return launched_ok(ctx, csm_launch::literal_scan(ctx->stream, lj), "literal sweep");
}

/* Finish a window whose fast-path record carries a tie or an edge-band flag. */
int resolve_window(csm_ctx* ctx, DeviceGrid& g, const csm_window* w, const Plan& p,
                   const int32_t* col_dev, const int32_t* row_dev, csm_result* out_dev,
                   const csm_result* have = nullptr, bool* changed = nullptr)
{   /* have: the record as already read back by the caller (saves a copy and a wait per query) */
    csm_result r;
    if (have) {
        r = *have;
    } else {
        HIP_TRY(ctx, hipMemcpyAsync(&r, out_dev, sizeof(r), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (changed)
        *changed = (!(r.flags & CSM_FLAG_EDGE_BAND) && r.tie_count > 1) || (r.flags & CSM_FLAG_EDGE_BAND);
    int rc;
    if (!(r.flags & CSM_FLAG_EDGE_BAND) && r.tie_count > 1) {
        if ((rc = resolve_ties(ctx, g, w, p, col_dev, row_dev, out_dev))) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(&r, out_dev, sizeof(r), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (r.flags & CSM_FLAG_EDGE_BAND)
        if ((rc = resolve_literal(ctx, g, w, p, col_dev, row_dev, out_dev))) return rc;
    return CSM_OK;
}

/* result record and the uncertified-entry count sit side by side: one read-back */
struct Tail {
    csm_result res;
    uint32_t n_unc, pad[3];
};

/* Where one query's data lives. Up from `pin` to `dev` in one copy of up_bytes: [projection job, padded to
 * job_bytes | angles | ranges]; back into the pinned block: the Tail behind the hit indices of ctx->hits. */
struct QueryBlock {
    int n = 0;                  /* beams */
    size_t hn = 0;              /* hit indices per axis: n_theta * n */
    size_t job_bytes = 0, up_bytes = 0;
    char *pin = nullptr, *dev = nullptr;
    double *ang_dev = nullptr, *rng_dev = nullptr;
    int32_t *col_dev = nullptr, *row_dev = nullptr;     /* ctx->hits */
    Tail *tail_dev = nullptr, *tail_pin = nullptr;
    uint32_t* unc_list = nullptr;       /* device: indices of the entries the projection could not certify */
};

int query_block(csm_ctx* ctx, int n_theta, int n, QueryBlock* q)
{
    int rc;
    q->n = n;
    q->hn = (size_t)n_theta * n;
    if ((rc = ensure(ctx, ctx->hits, q->hn * 8 + 256))) return rc;
    if ((rc = ensure(ctx, ctx->unc, 16 + (size_t)kUncCap * 4))) return rc;
    q->job_bytes = align256(sizeof(ProjJob));
    q->up_bytes = q->job_bytes + (size_t)n * 16;
    const size_t pin_bytes = q->up_bytes + 256;
    if ((rc = grow(ctx, ctx->q_pin, pin_bytes, pin_bytes + pin_bytes / 4, true))) return rc;
    if ((rc = ensure(ctx, ctx->q_dev, q->up_bytes))) return rc;
    q->pin = ctx->q_pin.as<char>();
    q->dev = ctx->q_dev.as<char>();
    q->ang_dev = reinterpret_cast<double*>(q->dev + q->job_bytes);
    q->rng_dev = q->ang_dev + n;
    q->col_dev = ctx->hits.as<int32_t>();
    q->row_dev = q->col_dev + q->hn;
    q->tail_dev = reinterpret_cast<Tail*>(q->row_dev + q->hn);
    q->tail_pin = reinterpret_cast<Tail*>(q->pin + ((q->up_bytes + 63) & ~(size_t)63));
    q->unc_list = ctx->unc.as<uint32_t>() + 4;
    return CSM_OK;
}

/* One query's stream work: [projection job | angles | ranges] up from the pinned block, the
 * projection, the search, [record | uncertified count] back into the pinned block. The same
 * sequence for every query of one launch shape, so from the third query of a shape on it is
 * replayed as a HIP graph (one launch instead of nine; every varying input lives in the pinned
 * block or in device memory the nodes point at). */
int enqueue_query(csm_ctx* ctx, DeviceGrid& g, const csm_window& w, const Plan& p, const QueryBlock& q)
{
    HIP_TRY(ctx, hipMemcpyAsync(q.dev, q.pin, q.up_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(&q.tail_dev->n_unc, 0, 16, ctx->stream));
    {
        ScopedTimer tm(ctx, "project");
        const int pb = ceil_div(q.n, kBlock);
        if (int e = csm_launch::project_batch(ctx->stream, dim3(pb, proj_theta_groups(w.n_theta, pb), 1),
                                              reinterpret_cast<const ProjJob*>(q.dev)))
            return launched_ok(ctx, e, "projection");
    }
    if (int rc = search_window(ctx, g, &w, p, q.col_dev, q.row_dev, &q.tail_dev->res))
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(q.tail_pin, q.tail_dev, sizeof(Tail), hipMemcpyDeviceToHost, ctx->stream));
    return CSM_OK;
}

/* What a graph of the query's chain has baked in. */
std::vector<uint64_t> graph_key(const csm_ctx* ctx, const DeviceGrid& g, int level, const csm_window& w, int n)
{
    std::vector<uint64_t> key = {
        ctx->alloc_epoch, (uint64_t)(uintptr_t)ctx->stream, (uint64_t)(uintptr_t)g.levels[0].cells,
        (uint64_t)(uintptr_t)g.levels[level].cells, (uint64_t)(uintptr_t)g.xg.p, (uint64_t)g.xg_pad,
        (uint64_t)g.rows, (uint64_t)g.cols, (uint64_t)g.known_r0, (uint64_t)g.known_c0,
        (uint64_t)w.n_theta, (uint64_t)n, (uint64_t)w.win_x, (uint64_t)w.win_y, (uint64_t)w.low_resolution,
        (uint64_t)(uint32_t)w.min_known, (uint64_t)w.merge_mode, 0 };
    std::memcpy(&key.back(), &w.score_threshold, 8);
    return key;
}

/* Launches the recorded chain of `key`, if there is one (*launched). */
int replay_graph(csm_ctx* ctx, const std::vector<uint64_t>& key, const Plan& p, bool* launched)
{
    auto it = ctx->graphs.find(key);
    if (it == ctx->graphs.end())
        return CSM_OK;
    HIP_TRY(ctx, hipGraphLaunch(it->second.exec, ctx->stream));
    note_exhaustive_search(ctx, p);
    /* no driver ran: the tie pass must see the job this chain was recorded with (its map, plan and
     * flag word), not that of the last plain launch */
    ctx->last_run.fine = it->second.fine;
    ctx->last_graph_replayed = true;
    *launched = true;
    return CSM_OK;
}

/* A sighting of a shape without a graph. The third: every workspace has its size, so the chain is captured,
 * kept and launched (a failed capture leaves the plain launch to the caller); at eight graphs all are dropped first. */
int record_graph(csm_ctx* ctx, const std::vector<uint64_t>& key, DeviceGrid& g, const csm_window& w, const Plan& p,
                 const QueryBlock& q, bool* launched)
{
    if (++ctx->graph_seen[key] < 3)
        return CSM_OK;
    if (ctx->graphs.size() >= 8) {
        for (auto& kv : ctx->graphs)
            (void)hipGraphExecDestroy(kv.second.exec);
        ctx->graphs.clear();
        ctx->graph_seen.clear();
    }
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    if (hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeRelaxed) != hipSuccess)
        return CSM_OK;
    ctx->capturing = true;
    const int rc_cap = enqueue_query(ctx, g, w, p, q);
    ctx->capturing = false;
    const hipError_t e_end = hipStreamEndCapture(ctx->stream, &graph);
    if (rc_cap == CSM_OK && e_end == hipSuccess && graph &&
        hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess) {
        ctx->graphs[key] = { exec, ctx->last_run.fine };   /* last_run.fine: set while capturing */
        HIP_TRY(ctx, hipGraphLaunch(exec, ctx->stream));
        *launched = true;
    }
    if (graph)
        (void)hipGraphDestroy(graph);
    (void)hipGetLastError();
    return CSM_OK;
}

/* The n_unc hit indices the device projection could not certify (listed up to kUncCap) recomputed exactly as
 * the reference does, with glibc. *patched: some entry differed and the corrected indices are on the device. */
int patch_uncertified(csm_ctx* ctx, const csm_geometry* geom, const csm_scan* scan, const csm_summary* out,
                      const QueryBlock& q, uint32_t n_unc, bool* patched)
{
    const size_t hn = q.hn;
    std::vector<int32_t> col(hn), row(hn);
    HIP_TRY(ctx, hipMemcpy(col.data(), q.col_dev, hn * 4, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(row.data(), q.row_dev, hn * 4, hipMemcpyDeviceToHost));
    *patched = false;
    if (n_unc > kUncCap) {
        std::vector<int32_t> c2(hn), r2(hn);
        csm_host_project(geom, out->sensor_pose, out->step_theta, out->win_theta, scan->angles,
                         scan->ranges, q.n, c2.data(), r2.data(), nullptr, nullptr);
        *patched = c2 != col || r2 != row;
        col.swap(c2);
        row.swap(r2);
    } else {
        std::vector<uint32_t> list(n_unc);
        HIP_TRY(ctx, hipMemcpy(list.data(), q.unc_list, (size_t)n_unc * 4, hipMemcpyDeviceToHost));
        for (uint32_t idx : list) {
            const int t = (int)(idx / (uint32_t)q.n) - out->win_theta;
            const int i = (int)(idx % (uint32_t)q.n);
            const double theta = out->sensor_pose[2] + out->step_theta * t;
            double hx, hy;
            host_hit_point(out->sensor_pose[0], out->sensor_pose[1], theta, scan->ranges[i], scan->angles[i], &hx, &hy);
            const int32_t c = cell_index(hx, geom->offset_x, geom->resolution);
            const int32_t r = cell_index(hy, geom->offset_y, geom->resolution);
            if (c != col[idx] || r != row[idx]) {
                col[idx] = c;
                row[idx] = r;
                *patched = true;
            }
        }
    }
    if (*patched) {
        HIP_TRY(ctx, hipMemcpy(q.col_dev, col.data(), hn * 4, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(q.row_dev, row.data(), hn * 4, hipMemcpyHostToDevice));
    }
    return CSM_OK;
}

} /* namespace */

extern "C" {

int csm_score_window_dev(csm_ctx* ctx, uint64_t map_id, const csm_window* w,
                         const int32_t* hit_col_dev, const int32_t* hit_row_dev, csm_result* out_dev)
{
    if (!ctx || !w || !hit_col_dev || !hit_row_dev || !out_dev)
        return fail(ctx, CSM_EINVAL, "csm_score_window_dev: bad arguments");
    DeviceGrid* g = find_grid(ctx, map_id);
    if (!g)
        return fail(ctx, CSM_ENOENT, "map %llu not resident", (unsigned long long)map_id);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Plan p;
    int rc = make_plan(ctx, *g, w, &p);
    if (rc)
        return rc;
    return run_exhaustive(ctx, *g, w, p, hit_col_dev, hit_row_dev, out_dev);
}

int csm_resolve_window_dev(csm_ctx* ctx, uint64_t map_id, const csm_window* w,
                           const int32_t* hit_col_dev, const int32_t* hit_row_dev,
                           csm_result* out_dev)
{
    if (!ctx || !w || !hit_col_dev || !hit_row_dev || !out_dev)
        return fail(ctx, CSM_EINVAL, "csm_resolve_window_dev: bad arguments");
    DeviceGrid* g = find_grid(ctx, map_id);
    if (!g)
        return fail(ctx, CSM_ENOENT, "map %llu not resident", (unsigned long long)map_id);
    Plan p;
    int rc = make_plan(ctx, *g, w, &p);
    if (rc)
        return rc;
    return resolve_window(ctx, *g, w, p, hit_col_dev, hit_row_dev, out_dev);
}

int csm_score_window_dump(csm_ctx* ctx, uint64_t map_id, const csm_window* w, const int32_t* hit_col,
                          const int32_t* hit_row, csm_result* out, uint32_t* dump_s,
                          uint16_t* dump_k, uint16_t* dump_coarse_k)
{
    if (!ctx || !w || !hit_col || !hit_row || !out)
        return fail(ctx, CSM_EINVAL, "csm_score_window: bad arguments");
    DeviceGrid* g = find_grid(ctx, map_id);
    if (!g)
        return fail(ctx, CSM_ENOENT, "map %llu not resident", (unsigned long long)map_id);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Plan p;
    int rc = make_plan(ctx, *g, w, &p);
    if (rc)
        return rc;
    const size_t hn = (size_t)p.n_theta * p.n;
    if ((rc = ensure(ctx, ctx->hits, hn * 8 + 256))) return rc;
    int32_t* col_dev = reinterpret_cast<int32_t*>(ctx->hits.p);
    int32_t* row_dev = col_dev + hn;
    csm_result* res_dev = reinterpret_cast<csm_result*>(row_dev + hn);
    HIP_TRY(ctx, hipMemcpyAsync(col_dev, hit_col, hn * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(row_dev, hit_row, hn * 4, hipMemcpyHostToDevice, ctx->stream));
    const size_t nc = (size_t)p.n_theta * p.nx * p.ny;
    if (dump_s && (rc = ensure(ctx, ctx->dump_s, nc * 4))) return rc;
    if (dump_k && (rc = ensure(ctx, ctx->dump_k, nc * 2))) return rc;
    uint32_t* dump_s_dev = dump_s ? ctx->dump_s.as<uint32_t>() : nullptr;
    uint16_t* dump_k_dev = dump_k ? ctx->dump_k.as<uint16_t>() : nullptr;
    if ((rc = run_exhaustive(ctx, *g, w, p, col_dev, row_dev, res_dev, dump_s_dev, dump_k_dev, dump_coarse_k != nullptr)))
        return rc;
    if ((rc = resolve_window(ctx, *g, w, p, col_dev, row_dev, res_dev)))
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out, res_dev, sizeof(csm_result), hipMemcpyDeviceToHost, ctx->stream));
    if (dump_s)
        HIP_TRY(ctx, hipMemcpyAsync(dump_s, dump_s_dev, nc * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (dump_k)
        HIP_TRY(ctx, hipMemcpyAsync(dump_k, dump_k_dev, nc * 2, hipMemcpyDeviceToHost, ctx->stream));
    std::vector<uint32_t> ck32;
    if (dump_coarse_k && p.L > 1) {
        ck32.resize((size_t)p.n_theta * p.nxc * p.nyc);
        HIP_TRY(ctx, hipMemcpyAsync(ck32.data(), ctx->coarse_k.p, ck32.size() * 4,
                                    hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < ck32.size(); ++i)
        dump_coarse_k[i] = (uint16_t)ck32[i];
    return CSM_OK;
}

int csm_score_window(csm_ctx* ctx, uint64_t map_id, const csm_window* w, const int32_t* hit_col,
                     const int32_t* hit_row, csm_result* out)
{
    return csm_score_window_dump(ctx, map_id, w, hit_col, hit_row, out, nullptr, nullptr, nullptr);
}

int csm_correlative_match(csm_ctx* ctx, uint64_t map_id, const csm_geometry* geom,
                          const csm_scan* scan, const double initial_pose[3],
                          const csm_correlative_params* prm, csm_summary* out)
{
    if (!ctx || !geom || !scan || !initial_pose || !prm || !out || scan->n_points < 1 ||
        prm->low_resolution < 1)
        return fail(ctx, CSM_EINVAL, "csm_correlative_match: bad arguments");
    if (!scan->angles || !scan->ranges || !scan_is_finite(scan))
        return fail(ctx, CSM_EINVAL, "csm_correlative_match: scan holds a non-finite range or angle");
    DeviceGrid* g = find_grid(ctx, map_id);
    if (!g)
        return fail(ctx, CSM_ENOENT, "map %llu not resident", (unsigned long long)map_id);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::memset(out, 0, sizeof(*out));
    const auto t0 = std::chrono::steady_clock::now();
    int level = 0;
    int rc = level_for_window(ctx, *g, prm->low_resolution, &level);
    if (rc)
        return rc;
    /* no wait here: a rebuilt coarse level is ordered before the search on the stream;
     * input_setup_us is the host side of the set-up */
    const auto t1 = std::chrono::steady_clock::now();

    csm_host_compound(initial_pose, scan->relative_sensor_pose, out->sensor_pose);
    csm_host_search_step(geom->resolution, scan->ranges, scan->n_points, &out->step_x,
                         &out->step_y, &out->step_theta);
    out->win_x = csm_host_window(prm->range_x, out->step_x);
    out->win_y = csm_host_window(prm->range_y, out->step_y);
    out->win_theta = csm_host_window(prm->range_theta, out->step_theta);
    csm_window w;
    std::memset(&w, 0, sizeof(w));
    w.n_theta = 2 * out->win_theta + 1;
    w.n_points = scan->n_points;
    w.win_x = out->win_x;
    w.win_y = out->win_y;
    w.low_resolution = prm->low_resolution;
    w.coarse_level = level;
    w.min_known = csm_host_min_known(scan->n_points, prm->known_rate_threshold);
    w.score_threshold = prm->score_threshold;
    w.merge_mode = merging_pays(scan->angles, scan->ranges, scan->n_points, geom->resolution) ? 0 : 1;
    /* Projection on the device with a per-entry certificate; the host
     * recomputes (glibc) only the entries that could not be certified. */
    const int n = scan->n_points;
    Plan p;
    QueryBlock q;
    if ((rc = make_plan(ctx, *g, &w, &p))) return rc;
    if ((rc = query_block(ctx, w.n_theta, n, &q))) return rc;
    ProjJob pj = proj_job(*geom, out->sensor_pose, out->step_theta, out->win_theta, n, q.ang_dev, q.rng_dev, q.col_dev,
                          q.row_dev);
    pj.unc_count = &q.tail_dev->n_unc;
    pj.unc_list = q.unc_list;
    pj.unc_cap = kUncCap;
    std::memcpy(q.pin, &pj, sizeof(pj));
    std::memcpy(q.pin + q.job_bytes, scan->angles, (size_t)n * 8);
    std::memcpy(q.pin + q.job_bytes + (size_t)n * 8, scan->ranges, (size_t)n * 8);

    bool launched = false;
    ctx->last_graph_replayed = false;
    if (!wants_two_phase(ctx, p) && !ctx->timing && ctx->tune.graphs && !g->xg_stale) {
        const std::vector<uint64_t> key = graph_key(ctx, *g, level, w, n);
        if ((rc = replay_graph(ctx, key, p, &launched))) return rc;
        if (!launched && (rc = record_graph(ctx, key, *g, w, p, q, &launched))) return rc;
    }
    if (!launched && (rc = enqueue_query(ctx, *g, w, p, q)))
        return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    Tail tail = *q.tail_pin;
    csm_result* res_dev = &q.tail_dev->res;
    bool changed = false, patched = false;
    if ((rc = resolve_window(ctx, *g, &w, p, q.col_dev, q.row_dev, res_dev, &tail.res, &changed))) return rc;
    if (changed) {
        HIP_TRY(ctx, hipMemcpyAsync(&tail.res, res_dev, sizeof(csm_result), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    out->raw = tail.res;
    if (tail.n_unc > 0 && (rc = patch_uncertified(ctx, geom, scan, out, q, tail.n_unc, &patched))) return rc;
    if (patched) {
        if ((rc = search_window(ctx, *g, &w, p, q.col_dev, q.row_dev, res_dev))) return rc;
        if ((rc = resolve_window(ctx, *g, &w, p, q.col_dev, q.row_dev, res_dev))) return rc;
        HIP_TRY(ctx, hipMemcpy(&out->raw, res_dev, sizeof(csm_result), hipMemcpyDeviceToHost));
    }
    const auto t2 = std::chrono::steady_clock::now();

    out->pose_found = out->raw.found;
    /* scan_matcher_correlative.cpp:203-206, 214-216 */
    out->best_sensor_pose[0] = out->sensor_pose[0] + out->raw.best_x * out->step_x;
    out->best_sensor_pose[1] = out->sensor_pose[1] + out->raw.best_y * out->step_y;
    out->best_sensor_pose[2] = out->sensor_pose[2] + out->raw.best_theta * out->step_theta;
    csm_host_move_backward(out->best_sensor_pose, scan->relative_sensor_pose, out->estimated_pose);
    out->candidates = (int64_t)w.n_theta * p.nx * p.ny;
    out->input_setup_us = std::chrono::duration<double, std::micro>(t1 - t0).count();
    out->optimization_us = std::chrono::duration<double, std::micro>(t2 - t1).count();
    return CSM_OK;
}

/* ScanMatcherGridSearch::OptimizePose (scan_matcher_grid_search.cpp:69-190) */
int csm_grid_search_match(csm_ctx* ctx, uint64_t map_id, const csm_geometry* geom,
                          const csm_scan* scan, const double initial_pose[3],
                          const csm_grid_search_params* prm, csm_summary* out)
{
    if (!ctx || !geom || !scan || !initial_pose || !prm || !out || scan->n_points < 1 ||
        !(prm->step_x > 0.0) || !(prm->step_y > 0.0) || !(prm->step_theta > 0.0))
        return fail(ctx, CSM_EINVAL, "csm_grid_search_match: bad arguments");
    if (!scan->angles || !scan->ranges || !scan_is_finite(scan))
        return fail(ctx, CSM_EINVAL, "csm_grid_search_match: scan holds a non-finite range or angle");
    DeviceGrid* g = find_grid(ctx, map_id);
    if (!g)
        return fail(ctx, CSM_ENOENT, "map %llu not resident", (unsigned long long)map_id);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::memset(out, 0, sizeof(*out));
    const auto t0 = std::chrono::steady_clock::now();
    csm_host_compound(initial_pose, scan->relative_sensor_pose, out->sensor_pose);
    /* the three loops of scan_matcher_grid_search.cpp:118-120: accumulated doubles */
    const double rx = prm->range_x / 2.0, ry = prm->range_y / 2.0, rt = prm->range_theta / 2.0;
    std::vector<double> px, py, th;
    for (double dy = -ry; dy <= ry; dy += prm->step_y)
        py.push_back(out->sensor_pose[1] + dy);
    for (double dx = -rx; dx <= rx; dx += prm->step_x)
        px.push_back(out->sensor_pose[0] + dx);
    for (double dt = -rt; dt <= rt; dt += prm->step_theta)
        th.push_back(out->sensor_pose[2] + dt);
    const int nx = (int)px.size(), ny = (int)py.size(), nt = (int)th.size(), n = scan->n_points;
    out->win_x = nx;
    out->win_y = ny;
    out->win_theta = nt;
    out->step_x = prm->step_x;
    out->step_y = prm->step_y;
    out->step_theta = prm->step_theta;
    for (int k = 0; k < 3; ++k)
        out->best_sensor_pose[k] = out->sensor_pose[k];
    out->raw.best_x = out->raw.best_y = out->raw.best_theta = -1;
    out->raw.score = prm->score_threshold;
    const size_t total = (size_t)nx * ny * nt;
    out->candidates = (int64_t)total;
    if (total > 0) {
        /* ScanData::HitPoint's products per theta value, with glibc */
        std::vector<double> prod(2 * (size_t)nt * n);
        double* rc = prod.data();
        double* rs = rc + (size_t)nt * n;
        for (int k = 0; k < nt; ++k)
            for (int i = 0; i < n; ++i)
                host_hit_products(th[k], scan->ranges[i], scan->angles[i], &rc[(size_t)k * n + i], &rs[(size_t)k * n + i]);
        int rc_ = 0;
        const size_t words = (size_t)nx + ny + prod.size();
        if ((rc_ = ensure(ctx, ctx->ex_coarse, words * 8 + 64))) return rc_;
        if ((rc_ = ensure(ctx, ctx->ex_fine, total * 8))) return rc_;
        if ((rc_ = ensure(ctx, ctx->ex_fine_k, total * 4))) return rc_;
        if ((rc_ = ensure(ctx, ctx->tie, 64))) return rc_;
        double* d_px = reinterpret_cast<double*>(ctx->ex_coarse.p);
        double* d_py = d_px + nx;
        double* d_rc = d_py + ny;
        double* d_rs = d_rc + (size_t)nt * n;
        unsigned long long* d_best = reinterpret_cast<unsigned long long*>(ctx->tie.p);
        const unsigned long long init_best[2] = { 0ull, ~0ull };
        HIP_TRY(ctx, hipMemcpyAsync(d_px, px.data(), (size_t)nx * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_py, py.data(), (size_t)ny * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_rc, prod.data(), prod.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_best, init_best, 16, hipMemcpyHostToDevice, ctx->stream));
        GridSearchJob gj;
        std::memset(&gj, 0, sizeof(gj));
        gj.cells = g->levels[0].cells;
        gj.rows = g->rows;
        gj.cols = g->cols;
        gj.pitch = g->pitch;
        gj.px = d_px;
        gj.py = d_py;
        gj.r_cos = d_rc;
        gj.r_sin = d_rs;
        gj.off_x = geom->offset_x;
        gj.off_y = geom->offset_y;
        gj.res = geom->resolution;
        gj.nx = nx;
        gj.ny = ny;
        gj.nt = nt;
        gj.n_points = n;
        gj.min_known = csm_host_min_known(n, prm->known_rate_threshold);
        gj.score_thr = prm->score_threshold;
        gj.lut = ctx->lut_dev.as<double>();
        gj.out_score = reinterpret_cast<double*>(ctx->ex_fine.p);
        gj.out_k = reinterpret_cast<uint32_t*>(ctx->ex_fine_k.p);
        gj.best_bits = d_best;
        gj.best_index = d_best + 1;
        const unsigned blocks = (unsigned)((total + kBlock - 1) / kBlock);
        {
            ScopedTimer tm(ctx, "grid_search");
            if (int e = csm_launch::grid_scores_pick(ctx->stream, blocks, gj))
                return launched_ok(ctx, e, "grid search");
        }
        unsigned long long best[2] = { 0, 0 };
        HIP_TRY(ctx, hipMemcpyAsync(best, d_best, 16, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (best[0] != 0ull && best[1] != ~0ull) {
            double score;
            const unsigned long long bits = best[0] - 1ull;
            std::memcpy(&score, &bits, 8);
            const size_t p = (size_t)best[1];
            const int it = (int)(p % nt), ix = (int)((p / nt) % nx), iy = (int)(p / ((size_t)nt * nx));
            out->pose_found = 1;
            out->raw.found = 1;
            out->raw.best_x = ix;
            out->raw.best_y = iy;
            out->raw.best_theta = it;
            out->raw.score = score;
            out->best_sensor_pose[0] = px[ix];
            out->best_sensor_pose[1] = py[iy];
            out->best_sensor_pose[2] = th[it];
        }
    }
    csm_host_move_backward(out->best_sensor_pose, scan->relative_sensor_pose, out->estimated_pose);
    out->optimization_us =
        std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    return CSM_OK;
}

/* The device projection (k_project) on its own, for parity tests of A3 */
int csm_project_scan(csm_ctx* ctx, const csm_geometry* geom, const double sensor_pose[3],
                     double step_theta, int32_t win_theta, const double* angles, const double* ranges,
                     int32_t n, int32_t* hit_col, int32_t* hit_row, uint32_t* uncertified,
                     int32_t uncertified_cap, int32_t* n_uncertified)
{
    if (!ctx || !geom || !sensor_pose || !angles || !ranges || n < 1 || win_theta < 0 || !hit_col ||
        !hit_row || !n_uncertified || uncertified_cap < 0 || (uncertified_cap > 0 && !uncertified))
        return fail(ctx, CSM_EINVAL, "csm_project_scan: bad arguments");
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(ranges[i]) || !std::isfinite(angles[i]))
            return fail(ctx, CSM_EINVAL, "csm_project_scan: beam %d is not finite", i);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int n_theta = 2 * win_theta + 1;
    const size_t hn = (size_t)n_theta * n;
    int rc;
    if ((rc = ensure(ctx, ctx->hits, hn * 8 + 256))) return rc;
    if ((rc = ensure(ctx, ctx->scan_dev, (size_t)n * 16))) return rc;
    if ((rc = ensure(ctx, ctx->unc, 16 + (size_t)std::max(uncertified_cap, 1) * 4))) return rc;
    int32_t* col_dev = reinterpret_cast<int32_t*>(ctx->hits.p);
    int32_t* row_dev = col_dev + hn;
    double* ang_dev = reinterpret_cast<double*>(ctx->scan_dev.p);
    double* rng_dev = ang_dev + n;
    uint32_t* unc_count = reinterpret_cast<uint32_t*>(ctx->unc.p);
    uint32_t* unc_list = unc_count + 4;
    HIP_TRY(ctx, hipMemcpyAsync(ang_dev, angles, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(rng_dev, ranges, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(unc_count, 0, 16, ctx->stream));
    ProjJob pj = proj_job(*geom, sensor_pose, step_theta, win_theta, n, ang_dev, rng_dev, col_dev, row_dev);
    pj.unc_count = unc_count;
    pj.unc_list = unc_list;
    pj.unc_cap = (uint32_t)uncertified_cap;
    if (int e = csm_launch::project(ctx->stream, dim3(ceil_div(n, kBlock), proj_theta_groups(n_theta, ceil_div(n, kBlock))), pj))
        return launched_ok(ctx, e, "projection");
    uint32_t count = 0;
    HIP_TRY(ctx, hipMemcpyAsync(hit_col, col_dev, hn * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(hit_row, row_dev, hn * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&count, unc_count, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *n_uncertified = (int32_t)count;
    const uint32_t have = std::min<uint32_t>(count, (uint32_t)uncertified_cap);
    if (have)
        HIP_TRY(ctx, hipMemcpy(uncertified, unc_list, (size_t)have * 4, hipMemcpyDeviceToHost));
    return CSM_OK;
}

} /* extern "C" */

