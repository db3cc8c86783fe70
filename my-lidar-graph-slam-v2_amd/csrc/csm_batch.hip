/* csm_batch.hip -- many windows in one launch chain (host code only): branch-and-bound and correlative
 * loop-detection batches (one driver, loop_batch), device-resident window batches (csm_score_windows_dev),
 * their entry points of the C ABI. run_batch_group takes one group of queries through its stages: plan,
 * scan staging, workspaces, job tables, upload, launch chain (joint binning, bound pass + exact rounds),
 * host finish with the exact fall-backs. */
#include "csm_matchers.hpp"

#include <optional>

#ifdef CSM_BIN_TIMING
static unsigned long long* g_bin_debug = nullptr;
static uint32_t* bin_debug_buffer()
{
    const size_t bytes = (size_t)kBinDebugRows * 128;
    if (!g_bin_debug && (hipMalloc(reinterpret_cast<void**>(&g_bin_debug), bytes) != hipSuccess ||
                         hipMemset(g_bin_debug, 0, bytes) != hipSuccess))
        g_bin_debug = nullptr;
    return reinterpret_cast<uint32_t*>(g_bin_debug);
}
#endif

namespace csm_host {


/* One query of a group: its window, frame and places in the group's workspaces. */
struct BatchPrep : WindowFrame {
    DeviceGrid* grid = nullptr;
    int level[kMaxElig] = { 0 };   /* index into grid->levels of box-max(2^h) */
    int n_theta = 0, n = 0;
    int win_x = 0, win_y = 0, win_t = 0;
    int max_tiles = 0;
    size_t hit_off = 0, tile_off = 0, theta_off = 0, best_off = 0;
    size_t lvl_off[kMaxElig] = { 0 };
};


/* Node of the reference's best-first search
 * (inc/mapping/scan_matcher_branch_bound.hpp:67-106): ordered by score only. */
struct HeapNode {
    int x, y, t, h;
    double score, known_rate;
    bool operator<(const HeapNode& o) const { return score < o.score; }
};

/* Exact resolution of one flagged branch-and-bound query. The device computes
 * the f64 score (beam order, per-node projection in double) and known count of
 * EVERY node of every level; the host then runs the reference's queue
 * discipline (std::priority_queue, same push / pop order as
 * src/mapping/scan_matcher_branch_bound.cpp:156-231) reading those scores
 * instead of calling Score(). No score is computed on the CPU. */
static int bnb_literal(csm_ctx* ctx, const csm_loop_query& q, const BatchPrep& p, const csm_summary& o,
                       const csm_bnb_params* prm, csm_result* res)
{
    const int H = prm->node_height_max;
    const int nx = p.nx, ny = p.ny;
    /* the exact path needs the host's own r*cos / r*sin (glibc) */
    const size_t hn = (size_t)p.n_theta * p.n;
    std::vector<double> prod(2 * hn);
    {
        std::vector<int32_t> col(hn), row(hn);
        int prc = csm_host_project(&q.geometry, o.sensor_pose, o.step_theta, p.win_t, q.scan.angles,
                                   q.scan.ranges, p.n, col.data(), row.data(), prod.data(),
                                   prod.data() + hn);
        if (prc)
            return fail(ctx, prc, "projection failed");
    }
    int rc0 = ensure(ctx, ctx->ex_coarse, 2 * hn * 8);
    if (rc0)
        return rc0;
    double* d_rc = reinterpret_cast<double*>(ctx->ex_coarse.p);
    double* d_rs = d_rc + hn;
    HIP_TRY(ctx, hipMemcpyAsync(d_rc, prod.data(), 2 * hn * 8, hipMemcpyHostToDevice, ctx->stream));
    std::vector<std::vector<double>> sc(H + 1);
    std::vector<std::vector<uint32_t>> kn(H + 1);
    int rc;
    for (int h = 0; h <= H; ++h) {
        const int nxh = nx >> h, nyh = ny >> h;
        const size_t n = (size_t)p.n_theta * nxh * nyh;
        if ((rc = ensure(ctx, ctx->ex_fine, n * 8))) return rc;
        if ((rc = ensure(ctx, ctx->ex_fine_k, n * 4))) return rc;
        ExactJob ej = exact_job(*p.grid, p.grid->levels[p.level[h]].cells, p.n_theta, p.n, -p.win_x, -p.win_y, nxh, nyh,
                                1 << h, ctx->lut_dev.as<double>(), ctx->ex_fine.as<double>(), ctx->ex_fine_k.as<uint32_t>());
        ej.r_cos = d_rc;
        ej.r_sin = d_rs;
        ej.sensor_x = o.sensor_pose[0];
        ej.sensor_y = o.sensor_pose[1];
        ej.step_x = o.step_x;
        ej.step_y = o.step_y;
        ej.off_x = q.geometry.offset_x;
        ej.off_y = q.geometry.offset_y;
        ej.res = q.geometry.resolution;
        if (int e = csm_launch::exact_scores(ctx->stream, (unsigned)((n + kBlock - 1) / kBlock), ej))
            return launched_ok(ctx, e, "exact score");
        sc[h].resize(n);
        kn[h].resize(n);
        HIP_TRY(ctx, hipMemcpyAsync(sc[h].data(), ej.out_score, n * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(kn[h].data(), ej.out_k, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }

    const int win_x = p.win_x, win_y = p.win_y, win_t = p.win_t;
    double score_max = prm->score_threshold;
    int best_x = 0, best_y = 0, best_t = 0;
    std::priority_queue<HeapNode> queue;
    const double n_points = static_cast<double>(p.n);
    auto append_node = [&](int x, int y, int t, int h) {
        const int xi = (x + win_x) >> h, yi = (y + win_y) >> h;
        const size_t i = ((size_t)(t + win_t) * (nx >> h) + xi) * (ny >> h) + yi;
        const double score = sc[h][i];
        if (score > score_max)
            queue.push(HeapNode { x, y, t, h, score, static_cast<double>(kn[h][i]) / n_points });
    };
    const int win_size_max = 1 << H;
    for (int x = -win_x; x <= win_x; x += win_size_max)
        for (int y = -win_y; y <= win_y; y += win_size_max)
            for (int t = -win_t; t <= win_t; ++t)
                append_node(x, y, t, H);
    while (!queue.empty()) {
        const HeapNode cur = queue.top();
        if (cur.score <= score_max || cur.known_rate <= prm->known_rate_threshold) {
            queue.pop();
            continue;
        }
        if (cur.h == 0) {
            best_x = cur.x;
            best_y = cur.y;
            best_t = cur.t;
            score_max = cur.score;
            queue.pop();
        } else {
            const int h = cur.h - 1;
            const int wsz = 1 << h;
            queue.pop();
            append_node(cur.x, cur.y, cur.t, h);
            append_node(cur.x + wsz, cur.y, cur.t, h);
            append_node(cur.x, cur.y + wsz, cur.t, h);
            append_node(cur.x + wsz, cur.y + wsz, cur.t, h);
        }
    }
    res->found = score_max > prm->score_threshold ? 1 : 0;
    res->best_x = best_x;
    res->best_y = best_y;
    res->best_theta = best_t;
    res->score = score_max;
    res->flags |= CSM_FLAG_LITERAL;
    return CSM_OK;
}

/* The device copy of a batch's final records: sized here, filled by
 * run_batch_group, handed out by csm_copy_last_batch_records. */
static int begin_batch_records(csm_ctx* ctx, int n_queries)
{
    ctx->rec_n = 0;
    int rc = ensure(ctx, ctx->rec_dev, (size_t)n_queries * sizeof(csm_result));
    if (rc)
        return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   /* patches of the previous call have landed */
    ctx->rec_patch.clear();
    ctx->rec_patch.reserve((size_t)n_queries);         /* no reallocation under a pending copy */
    ctx->rec_n = n_queries;
    return CSM_OK;
}

/* What distinguishes the two batched searches. */
struct BatchSpec {
    bool bnb = true;          /* branch and bound (leaf + 2^h levels) or correlative (fine + one
                                 box-max(L) level) */
    int H = 0;                /* number of coarser levels */
    int stride[kMaxElig] = { 1 };   /* stride[j] of level j (stride[0] = 1): its box-max window */
    int unit = 1;             /* candidate domain is padded to a multiple of this */
    double range_x = 0, range_y = 0, range_theta = 0;
    double score_thr = 0, known_thr = 0;
    const csm_bnb_params* bnb_params = nullptr;
    const csm_correlative_params* csm_params = nullptr;
    const double* max_range = nullptr;   /* [n_queries] largest range of each query's scan */
};

/* csm_score_windows_dev: the windows and hit indices are given (device
 * resident, already projected), the results stay on the device, nothing waits. */
struct ResidentBatch {
    const csm_window* windows;            /* [n] */
    const int32_t* const* hit_col;        /* [n] device pointers, [n_theta][n_points] each */
    const int32_t* const* hit_row;
    csm_result* out_dev;                  /* [n] device */
    uint32_t* const* dump_s = nullptr;    /* optional [n] device pointers (any may be null): every candidate's */
    uint16_t* const* dump_k = nullptr;    /* integer sums, [n_theta][nx][ny] (parity tests) */
    float* const* dump_f = nullptr;       /* optional: every candidate's fp32 key of the bound pass */
};

/* One group of queries that share (nx, ny) on its way through run_batch_group's stages: what each
 * stage decides or places, read by the stages after it. */
struct BatchGroup {
    csm_ctx* ctx;
    const csm_loop_query* queries;
    const std::vector<int>& idx;                  /* the group's queries */
    const std::vector<std::vector<int>>& levels;  /* [query][h] index into its grid's levels */
    const BatchSpec& spec;
    csm_summary* out;
    const ResidentBatch* resident;
    const int H, nq;

    /* host set-up and plan */
    std::vector<BatchPrep> pp;
    std::vector<csm_summary> scratch_out;         /* resident mode: no host summaries */
    int nx = 0, ny = 0, n_theta_max = 0, n_points_max = 0;
    std::vector<PassPlan> lp;                     /* [H + 1] launch geometry shared by the group */
    size_t bin_lds = 0, binj_lds = 0;
    bool joint = false, bound_pass = false, two_rounds = false;
    bool coarse_first = false;                    /* the box-max(L) level bounds the units of the exact pass */
    size_t hit_total = 0, tile_total = 0, theta_total = 0;
    /* scans */
    std::vector<size_t> scan_off;
    size_t scan_total = 0;
    double* scans = nullptr;                      /* pinned staging */
    /* workspaces */
    size_t lvl_total = 0, best_total = 0, blocks_total = 0, jobs_bytes = 0;
    double* d_scans = nullptr;
    csm_result* d_out = nullptr;
    uint32_t* d_flags = nullptr;                  /* [nq], behind the records */
    /* job tables, and where they were uploaded */
    std::vector<ProjJob> ij;
    std::vector<BinJob> bj;
    std::vector<FinalJob> fj;
    std::vector<std::vector<ScoreJob>> sj;        /* [h][query] */
    std::vector<ZeroJob> zj;                      /* [query][h - 1] */
    size_t zero_words_max = 0;
    PinBuf tables;                                /* from ctx->pin_free, back there after the chain */
    char *d_ij = nullptr, *d_bj = nullptr, *d_fj = nullptr, *d_idx = nullptr, *d_zj = nullptr;
    std::vector<char*> d_sj;

    BatchGroup(csm_ctx* c, const csm_loop_query* q, const std::vector<int>& i, const std::vector<std::vector<int>>& l,
               const BatchSpec& s, csm_summary* o, const ResidentBatch* r)
        : ctx(c), queries(q), idx(i), levels(l), spec(s), out(o), resident(r), H(s.H), nq((int)i.size())
    {
    }
    int plan();                                   /* the stages, in order */
    int stage_scans();
    int size_workspaces();
    int fill_job_tables();
    void build_jobs(int k);
    int upload_tables();
    int launch_chain();
    int finish();
    int min_known_of(int k) const
    {
        return resident ? resident->windows[idx[k]].min_known : csm_host_min_known(pp[k].n, spec.known_thr);
    }
    double score_thr(int k) const { return resident ? resident->windows[idx[k]].score_threshold : spec.score_thr; }
    /* CSM_TUNING host timing: time since the previous tick */
    void tick(const char* what) const
    {
        static thread_local std::chrono::steady_clock::time_point last;
        const auto now = std::chrono::steady_clock::now();
        if (ctx->tune.host_timing && what)
            fprintf(stderr, "[run_batch_group nq=%d] %-10s %8.3f ms\n", nq, what,
                    std::chrono::duration<double, std::milli>(now - last).count());
        last = now;
    }
};

/* Stage 1, host set-up and plan: each query's window and frame, the launch geometry shared by the
 * group, the joint / bound-pass / two-round decisions, the sizes of the per-query lists. */
int BatchGroup::plan()
{
    pp.resize(nq);
    if (resident) {
        scratch_out.assign((size_t)*std::max_element(idx.begin(), idx.end()) + 1, csm_summary {});
        out = scratch_out.data();
    }
    for (int k = 0; k < nq; ++k) {
        const csm_loop_query& q = queries[idx[k]];
        csm_summary& o = out[idx[k]];
        BatchPrep& p = pp[k];
        p.grid = find_grid(ctx, q.map_id);
        for (int h = 0; h <= H; ++h)
            p.level[h] = levels[idx[k]][h];
        if (resident) {
            const csm_window& w = resident->windows[idx[k]];
            p.win_x = w.win_x;
            p.win_y = w.win_y;
            p.win_t = (w.n_theta - 1) / 2;
            p.n_theta = w.n_theta;
            p.n = w.n_points;
        } else {
            csm_host_compound(q.initial_pose, q.scan.relative_sensor_pose, o.sensor_pose);
            search_step_from_max(q.geometry.resolution, spec.max_range[idx[k]], &o.step_x, &o.step_y,
                                 &o.step_theta);
            o.win_x = p.win_x = csm_host_window(spec.range_x, o.step_x);
            o.win_y = p.win_y = csm_host_window(spec.range_y, o.step_y);
            o.win_theta = p.win_t = csm_host_window(spec.range_theta, o.step_theta);
            p.n_theta = 2 * p.win_t + 1;
            p.n = q.scan.n_points;
        }
        static_cast<WindowFrame&>(p) = window_frame(*p.grid, p.win_x, p.win_y, spec.unit);
        if (p.n > kMaxPoints)
            return fail(ctx, CSM_EINVAL, "query %d: more than %d beams per scan", idx[k], kMaxPoints);
        n_theta_max = std::max(n_theta_max, p.n_theta);
        n_points_max = std::max(n_points_max, p.n);
    }
    nx = pp[0].nx;
    ny = pp[0].ny;

    lp.resize(H + 1);
    if (!plan_pass_pairs(ctx->tune, nx, ny, &lp[0], true))
        return fail(ctx, CSM_EINVAL, "no launch geometry for the fine level");
    for (int h = 1; h <= H; ++h)
        if (!plan_pass(ctx->tune, nx / spec.stride[h], ny / spec.stride[h], spec.stride[h], &lp[h]))
            return fail(ctx, CSM_EINVAL, "no launch geometry for level %d (stride %d)", h, spec.stride[h]);
    PassPlan& fine = lp[0];
    if (resident) {
        fine.weighted = resident->windows[idx[0]].merge_mode == 0;
    } else {
        const csm_loop_query& q0 = queries[idx[0]];
        fine.weighted = merging_pays(q0.scan.angles, q0.scan.ranges, q0.scan.n_points, q0.geometry.resolution);
    }
    /* Joint entry lists of slice pairs (k_binj + k_score_joint_batch, csm_joint_kernels.hip): the
     * two-slice plan with merged (weighted) entries, when the joint hash table of every query
     * fits a CU's LDS. Otherwise round 2's per-slice lists. */
    for (const BatchPrep& p : pp)
        binj_lds = std::max(binj_lds, csm_launch::binj_lds_bytes(p.tiles_x * p.tiles_y, p.n, csm_launch::binj_hash_size(p.n)));
    joint = ctx->tune.joint && fine.pairs && fine.lists == 2 && fine.weighted &&
              binj_lds <= 150 * 1024;     /* up to ~1,100 beams four binning workgroups share a CU, two up
                                               to ~2,200; one (the fine level's gain outweighs the slower
                                               binning) up to 4,248 beams per scan on maps of at most 32
                                               endpoint tiles (153,264 B with 16 tiles; 4,249 beams take
                                               154,036 B), 4,224 with 64 tiles: tests/beam_ladder_cases.py */
    fine.joint = joint;
    /* The packed-fp32 bound pass in front of the exact kernel: only where the arg-max is over ALL
     * candidates of the window -- the correlative sweep with a known-rate threshold that the coarse
     * level passes whenever a fine candidate scores at all (min_known <= 1; a touched edge band
     * switches the skipping off per query on the device). Branch and bound tests every leaf's own
     * known count: exact kernel only. */
    bound_pass = joint && ctx->tune.bound_pass && nq < (1 << 14) && fine.ncb() <= 256 &&
                   (n_theta_max + 1) / 2 <= 1024;       /* the work list's item format */
    /* Where the winner must pass a known-count test the bound pass does not see -- branch and bound:
     * every leaf's own count; the correlative sweep with a known-rate threshold above one beam: the
     * coarse node's count (the reference's loop detectors run with 0.6) -- the window's greatest
     * fp32 key may belong to a candidate that does not count, and the exact pass runs in two rounds
     * (k_bound_select). */
    two_rounds = spec.bnb;
    for (int k = 0; k < nq; ++k)
        two_rounds = two_rounds || min_known_of(k) > 1;
    /* Coarse first: the correlative sweep has a box-max(L) level whose nodes bound their L x L candidates,
     * at 1/L^2 of the fine level's reads. Its node keys, not an fp32 pass over every candidate, then bound
     * the units of the exact pass (k_coarse_joint_batch, k_unit_bounds). The greatest bound is not an
     * attained key, so the exact pass takes two rounds: the units near the greatest bound, then the units
     * whose bound reaches the best exact key of round 1. Windows that ask for every candidate's sums or
     * fp32 key keep the fp32 pass (for the whole group: one chain). */
    bool dumps = false;
    if (resident)
        for (int k = 0; k < nq; ++k)
            dumps = dumps || (resident->dump_s && resident->dump_s[idx[k]]) || (resident->dump_k && resident->dump_k[idx[k]]) ||
                    (resident->dump_f && resident->dump_f[idx[k]]);
    /* The level decides between units, a node between L x L candidates: a window of a handful of units
     * (few slices, one candidate block) lies inside one blurred peak of the level, every unit's bound
     * reaches the winner, and only the fp32 pass's per-candidate keys still tell units apart. */
    constexpr int kCoarseFirstMinUnits = 16;
    int min_units = INT_MAX;
    for (const BatchPrep& p : pp)
        min_units = std::min(min_units, (p.n_theta + 1) / 2 * fine.ncb());
    coarse_first = bound_pass && !spec.bnb && H >= 1 && spec.stride[1] >= 2 && !dumps && min_units >= kCoarseFirstMinUnits;
    two_rounds = two_rounds || coarse_first;
    for (BatchPrep& p : pp) {
        /* lists and records per slice, or per pair of slices (2 n entries each) */
        const int units = joint ? (p.n_theta + 1) / 2 : p.n_theta;
        const int per_unit = joint ? 2 * p.n : p.n;
        p.max_tiles = std::min(per_unit, p.tiles_x * p.tiles_y) + per_unit / (joint ? kJRec : kPbMax) + 1;
        bin_lds = std::max(bin_lds, bin_lds_bytes(p.tiles_x * p.tiles_y, p.n));
        p.hit_off = hit_total;
        p.tile_off = tile_total;
        p.theta_off = theta_total;
        hit_total += (size_t)(p.n_theta + 1) * p.n;         /* >= units * per_unit */
        tile_total += (size_t)units * p.max_tiles;
        theta_total += 2 * (size_t)p.n_theta;     /* record counts + merge flags */
    }
    if (bin_lds > 160 * 1024 - 64)
        return fail(ctx, CSM_EINVAL, "grid + window too large for the binning kernel (its per-tile words, hash table and cell list exceed the LDS)");
    return CSM_OK;
}

/* Stage 2: scans go to the device as they are (angles, ranges); the projection runs there with a
 * per-entry certificate (k_project). Queries that share a scan (one query scan node against many
 * local maps: the usual shape of a Detect() call) share its device copy. The staging buffer is
 * pinned and owned by the context: no clearing, one DMA. */
int BatchGroup::stage_scans()
{
    scan_off.resize(nq);
    if (resident) {                         /* no scan is staged and none is shared: the offsets only count */
        for (int k = 0; k < nq; ++k) {
            scan_off[k] = scan_total;
            scan_total += 2 * (size_t)pp[k].n;
        }
    } else {
        ScanTable table;                    /* scans are laid out in first-use order: [angles | ranges] each */
        for (int k = 0; k < nq; ++k)
            scan_off[k] = 2 * (size_t)table.slot(queries[idx[k]].scan, k);
        scan_total = 2 * (size_t)table.beams;
        const size_t need = scan_total * 8;
        if (int rc = grow(ctx, ctx->pin_scans, need, need + need / 4 + 64, false))
            return rc;
        scans = ctx->pin_scans.as<double>();
        host_parallel_for((int)table.first_use.size(), 128, [&](int lo, int hi) {
            for (int j = lo; j < hi; ++j) {
                const int k = table.first_use[j];
                const csm_loop_query& q = queries[idx[k]];
                std::memcpy(scans + scan_off[k], q.scan.angles, (size_t)pp[k].n * 8);
                std::memcpy(scans + scan_off[k] + pp[k].n, q.scan.ranges, (size_t)pp[k].n * 8);
            }
        });
    }
    tick("setup");
    return CSM_OK;
}

/* Stage 3: the context's workspaces sized for the group and carved up; the scans go up, the
 * per-query flag words are cleared. */
int BatchGroup::size_workspaces()
{
    const int ncb = lp[0].ncb();
    for (BatchPrep& p : pp) {
        for (int h = 1; h <= H; ++h) {
            p.lvl_off[h] = lvl_total;
            lvl_total += (size_t)p.n_theta * (nx / spec.stride[h]) * (ny / spec.stride[h]);
        }
        p.best_off = best_total;
        best_total += (size_t)p.n_theta * ncb;
        blocks_total += (size_t)((p.n_theta + 1) / 2) * ncb;
    }
    int rc;
    if ((rc = ensure(ctx, ctx->b_prod, (resident ? 0 : scan_total * 8) + 64))) return rc;
    if ((rc = ensure(ctx, ctx->b_hits, (resident ? 0 : hit_total * 8) + 64))) return rc;
    if ((rc = ensure(ctx, ctx->b_sorted, hit_total * 4 + 256))) return rc;
    if (lp[0].pairs)
        for (BatchPrep& p : pp)
            if ((rc = ensure_xgrid(ctx, *p.grid, xgrid_pad_for(nx, ny)))) return rc;
    if ((rc = ensure(ctx, ctx->b_sorted_rc, hit_total * 4))) return rc;
    if ((rc = ensure(ctx, ctx->b_tiles, tile_total * sizeof(TileRec)))) return rc;
    if ((rc = ensure(ctx, ctx->b_ntiles, theta_total * 4))) return rc;
    if ((rc = ensure(ctx, ctx->b_lvl, lvl_total * 8 + 16))) return rc;
    if ((rc = ensure(ctx, ctx->b_best, best_total * sizeof(BlockBest)))) return rc;
    if (bound_pass) {
        if (!ctx->bound_stats.p) {
            if ((rc = ensure(ctx, ctx->bound_stats, 64))) return rc;
            HIP_TRY(ctx, hipMemsetAsync(ctx->bound_stats.p, 0, 64, ctx->stream));
        }
        if ((rc = ensure(ctx, ctx->b_abest, best_total * sizeof(float)))) return rc;
        /* work lists of the exact kernel: [2 counts, pad][items 0][items 1], one item per (pair, block) */
        if ((rc = ensure(ctx, ctx->b_items, 64 + 2 * blocks_total * 4))) return rc;
        if (!coarse_first)
            for (BatchPrep& p : pp)
                if ((rc = ensure_xgrid_f(ctx, *p.grid))) return rc;
    }
    if ((rc = ensure(ctx, ctx->b_out, (size_t)nq * (sizeof(csm_result) + 4)))) return rc;
    jobs_bytes = (size_t)nq * (sizeof(ProjJob) + sizeof(BinJob) + sizeof(FinalJob) +
                                 (size_t)(H + 1) * sizeof(ScoreJob) + (size_t)H * sizeof(ZeroJob));
    if ((rc = ensure(ctx, ctx->b_jobs, jobs_bytes + 1024))) return rc;

    d_scans = ctx->b_prod.as<double>();
    d_out = ctx->b_out.as<csm_result>();
    d_flags = reinterpret_cast<uint32_t*>(d_out + nq);

    if (!resident)
        HIP_TRY(ctx, hipMemcpyAsync(d_scans, scans, scan_total * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_flags, 0, (size_t)nq * 4, ctx->stream));
    tick("workspace");
    return CSM_OK;
}

/* Stage 4, for query k: its projection, binning, level, fine and final records. */
void BatchGroup::build_jobs(int k)
{
    const int i = idx[k];
    const csm_loop_query& q = queries[i];
    const csm_summary& o = out[i];
    const BatchPrep& p = pp[k];
    const DeviceGrid& gr = *p.grid;
    const int min_known = min_known_of(k);
    uint32_t* const flags = d_flags + k;
    int32_t* const hits = ctx->b_hits.as<int32_t>() + p.hit_off;     /* [col | row] */
    uint32_t* const lvl_s = ctx->b_lvl.as<uint32_t>();
    uint32_t* const lvl_k = lvl_s + lvl_total;

    ProjJob& I = ij[k];
    I = proj_job(q.geometry, o.sensor_pose, o.step_theta, p.win_t, p.n, d_scans + scan_off[k],
                 d_scans + scan_off[k] + p.n, resident ? const_cast<int32_t*>(resident->hit_col[i]) : hits,
                 resident ? const_cast<int32_t*>(resident->hit_row[i]) : hits + hit_total);
    I.flags = flags;
    I.check_nodes = spec.bnb ? 1 : 0;
    I.flag_uncertain = 1;
    I.x_lo = p.x_lo;
    I.y_lo = p.y_lo;
    I.nx = p.nx;
    I.ny = p.ny;
    I.step_x = o.step_x;
    I.step_y = o.step_y;

    BinJob& B = bj[k];
    B = bin_job(gr, p, p.n_theta, p.n, p.max_tiles, I.hit_col, I.hit_row, ctx->b_sorted.as<uint32_t>() + p.hit_off,
                ctx->b_tiles.as<TileRec>() + p.tile_off, ctx->b_ntiles.as<int32_t>() + p.theta_off, flags,
                joint ? 2 : lp[0].pairs ? 1 : 0);
    B.sorted_rc = H > 0 ? ctx->b_sorted_rc.as<uint32_t>() + p.hit_off : nullptr;
    B.hash_size = joint ? csm_launch::binj_hash_size(p.n) : bin_hash_size(p.n);
    B.max_mult = lp[0].weighted ? kMaxMult : 1;
    B.lstride = lp[0].lstride;
#ifdef CSM_BIN_TIMING
    B.tuning_counters = bin_debug_buffer();
#endif
    B.n_band = H;

    ScoreJob& F = sj[0][k];
    F = score_job(gr, gr.levels[p.level[0]].cells, 1, B, min_known);
    F.joint = joint ? 1 : 0;
    F.rank_l = spec.bnb ? 1 : spec.unit;
    for (int h = 1; h <= H; ++h) {
        B.band_win[h - 1] = spec.stride[h];
        B.band_nx[h - 1] = p.nx / spec.stride[h];
        B.band_ny[h - 1] = p.ny / spec.stride[h];
        ScoreJob& S = sj[h][k];
        S = score_job(gr, gr.levels[p.level[h]].cells, spec.stride[h], B, min_known);
        S.joint = F.joint;
        S.rank_l = F.rank_l;
        /* a leaf's own known count bounds every ancestor's from below when
         * no read can fall in the edge band: the level passes are only
         * needed to detect (and then handle) that case */
        S.skip_unless_band = spec.bnb ? 1 : (min_known <= 1 && !coarse_first);
        S.sorted_pb = B.sorted_rc;
        S.acc_s = lvl_s + p.lvl_off[h];
        S.acc_k = lvl_k + p.lvl_off[h];
        F.elig[h - 1] = EligLevel { S.acc_k, S.acc_s, S.stride, S.nx, S.ny };
        /* the level's atomic accumulators: cleared only when the pass will run; the coarse-first pass
         * stores every node and needs no clear */
        ZeroJob& Z0 = zj[(size_t)k * H + (h - 1)];
        Z0 = ZeroJob { S.acc_s, S.acc_k, coarse_first ? 0 : (size_t)p.n_theta * S.nx * S.ny, flags,
                       S.skip_unless_band ? 0 : 1, 0 };
        zero_words_max = std::max(zero_words_max, Z0.words);
    }
    F.xg = gr.xg.as<uint32_t>();
    F.xg_pitch = gr.xg_pitch;
    F.xg_pad = gr.xg_pad;
    F.block_best = ctx->b_best.as<BlockBest>() + p.best_off;
    if (bound_pass) {
        if (!coarse_first)                      /* the fp32 key copy: read by the fp32 pass only */
            F.xgf = gr.xgf.as<float>();
        F.approx_best = ctx->b_abest.as<float>() + p.best_off;
        /* |fp32 key - key| <= (n + 2) 2^-24 * key for a sum of n non-negative terms (one rounding
         * per fused multiply-add, one for each cell's float, one for joining the two accumulator
         * sets), n <= beams. A candidate that reaches the winner's exact key has an fp32 key of at
         * least max_fp32 * (1 - 3 (n + 3) 2^-24); the kernel compares with 4 (n + 3) 2^-24. */
        F.approx_slack = 4.0f * (float)(p.n + 3) * 5.9604645e-08f;
        F.bound_stats = ctx->bound_stats.as<uint32_t>();
        /* found <=> sum of probabilities / n > threshold, and that sum is (0.998 / 65534 / 499) * key
         * up to the f64 rounding of the beam-order summation (1e-12 relative): a candidate below
         * this key cannot be reported */
        const double thr = score_thr(k);
        F.key_floor = thr > 0.0 ? (float)(thr * p.n * (65534.0 * 499.0 / 0.998) * (1.0 - 1e-9)) *
                                      (1.0f - F.approx_slack)
                                : 0.0f;
        F.round1_record = resident ? (const void*)(resident->out_dev + i) : (const void*)(d_out + k);
        if (resident && resident->dump_f)
            F.dump_f = resident->dump_f[i];
    }
    if (resident && resident->dump_s)
        F.dump_s = resident->dump_s[i];
    if (resident && resident->dump_k)
        F.dump_k = resident->dump_k[i];
    /* branch and bound tests every popped node, leaf included; the
     * correlative sweep tests the coarse node only */
    F.check_own_known = spec.bnb || H == 0;
    F.elig_only_if_band = spec.bnb ? 1 : (min_known <= 1);
    F.n_elig = H;

    FinalJob& Z = fj[k];
    Z = final_job(F, p.n_theta * lp[0].ncb(), I.hit_col, I.hit_row, score_thr(k), ctx->lut_dev.as<double>(),
                  resident ? resident->out_dev + i : d_out + k);
    if (spec.bnb) {
        /* scan_matcher_branch_bound.cpp:144-146 (scan_matcher_correlative.cpp:149-152: the first candidate) */
        Z.init_x = Z.init_y = Z.init_theta = 0;
    }
}

/* Stage 4: every query's job records. */
int BatchGroup::fill_job_tables()
{
    ij.resize(nq);
    bj.resize(nq);
    fj.resize(nq);
    sj.assign(H + 1, std::vector<ScoreJob>(nq));
    zj.resize((size_t)nq * H);
    for (int k = 0; k < nq; ++k)
        build_jobs(k);
    return CSM_OK;
}


/* A pinned block of at least `bytes` for a batch's job tables: the first in the pool that is large
 * enough, else a new one with room to grow. */
static int take_pinned(csm_ctx* ctx, size_t bytes, PinBuf* out)
{
    for (size_t b = 0; b < ctx->pin_free.size(); ++b)
        if (ctx->pin_free[b].cap >= bytes) {
            *out = std::move(ctx->pin_free[b]);
            ctx->pin_free.erase(ctx->pin_free.begin() + b);
            return CSM_OK;
        }
    return grow(ctx, *out, bytes, bytes + bytes / 4 + 4096, false);
}

/* Stage 5: upload the job tables: one device buffer with 256-byte aligned sections, filled from
 * one pinned block by ONE copy (five copies from pageable vectors cost 18 us per 64-window chain
 * and a staging pass each). */
int BatchGroup::upload_tables()
{
    const size_t tables_cap = jobs_bytes + (size_t)nq * 4 + 256 * (size_t)(H + 10);
    int rc;
    if ((rc = ensure(ctx, ctx->b_jobs, tables_cap))) return rc;
    if ((rc = take_pinned(ctx, tables_cap, &tables))) return rc;
    char* const jb0 = reinterpret_cast<char*>(ctx->b_jobs.p);
    char* const hb0 = tables.as<char>();
    Carve c;
    auto put = [&](const void* src, size_t bytes, char** dev) -> hipError_t {
        const size_t at = c.take(bytes);
        *dev = jb0 + at;
        std::memcpy(hb0 + at, src, bytes);
        return c.off <= tables_cap ? hipSuccess : hipErrorInvalidValue;
    };
    if (H > 0)
        HIP_TRY(ctx, put(zj.data(), zj.size() * sizeof(ZeroJob), &d_zj));
    if (!resident)
        HIP_TRY(ctx, put(idx.data(), (size_t)nq * sizeof(int), &d_idx));
    d_sj.resize(H + 1);
    HIP_TRY(ctx, put(ij.data(), nq * sizeof(ProjJob), &d_ij));
    HIP_TRY(ctx, put(bj.data(), nq * sizeof(BinJob), &d_bj));
    HIP_TRY(ctx, put(fj.data(), nq * sizeof(FinalJob), &d_fj));
    for (int h = 0; h <= H; ++h)
        HIP_TRY(ctx, put(sj[h].data(), nq * sizeof(ScoreJob), &d_sj[h]));
    HIP_TRY(ctx, hipMemcpyAsync(jb0, hb0, c.off, hipMemcpyHostToDevice, ctx->stream));
    tick("jobs");
    return CSM_OK;
}

/* Stage 6: projection, binning, edge-band clears, coarser levels, bound pass, exact fine level and
 * finalize, in one chain on the context's stream. */
int BatchGroup::launch_chain()
{
    const ScoreJob* fine_jobs = reinterpret_cast<const ScoreJob*>(d_sj[0]);
    int rc;
    if (!resident) {
        ScopedTimer tm(ctx, "project");
        const int pb = ceil_div(n_points_max, kBlock);
        if (int e = csm_launch::project_batch(ctx->stream, dim3(pb, proj_theta_groups(n_theta_max, (long)pb * nq), nq),
                                              reinterpret_cast<const ProjJob*>(d_ij)))
            return launched_ok(ctx, e, "projection");
    }
    if (joint) {
        ScopedTimer tm(ctx, "bin");
        if ((rc = launched_ok(ctx, csm_launch::binj_batch(ctx->stream, ctx->device, (n_theta_max + 1) / 2, nq, binj_lds,
                                                          reinterpret_cast<const BinJob*>(d_bj)), "joint binning")))
            return rc;
    } else {
        ScopedTimer tm(ctx, "bin");
        if ((rc = launched_ok(ctx, csm_launch::bin_batch(ctx->stream, ctx->device, n_theta_max, nq, bin_lds,
                                                         reinterpret_cast<const BinJob*>(d_bj)), "binning")))
            return rc;
    }
    if (H > 0 && zero_words_max > 0) {
        const int zb = (int)std::min<size_t>(64, (zero_words_max + 255) / 256);
        if ((rc = launched_ok(ctx, csm_launch::zero_if_band_batch(ctx->stream, std::max(1, zb), nq * H,
                                                                  reinterpret_cast<const ZeroJob*>(d_zj)), "edge-band clear")))
            return rc;
    }
    for (int h = H; h >= 1; --h) {
        if (coarse_first) {
            /* the level IS the bound pass of the fine level, and is timed as that */
            ScopedTimer tm(ctx, "score_bound");
            if ((rc = launched_ok(ctx, csm_launch::coarse_joint_batch(ctx->stream, lp[h].nx * lp[h].ny, (n_theta_max + 1) / 2, nq,
                                                                      reinterpret_cast<const ScoreJob*>(d_sj[h])), "coarse level")))
                return rc;
            continue;
        }
        /* keep >= ~2k workgroups in flight: split the tile list when the
         * level has few candidate blocks */
        const long blocks = (long)lp[h].ncb() * n_theta_max * nq;
        /* a level that only runs when a beam reaches the edge band (rare) is launched
         * unsplit: the launch that normally exits at once stays small */
        bool all_exit = true;
        for (int k = 0; k < nq; ++k)
            all_exit = all_exit && sj[h][k].skip_unless_band;
        const int n_slices = (blocks >= 2048 || all_exit)
                                 ? 1 : (int)std::min<long>(8, ceil_div(2048, (int)std::max<long>(1, blocks)));
        ScopedTimer tm(ctx, "score_coarse");
        if ((rc = launch_score_batch(ctx, reinterpret_cast<const ScoreJob*>(d_sj[h]), nq, lp[h],
                                     n_theta_max, n_slices, all_exit && nq >= 16 ? 4 : 0)))
            return rc;
    }
    if (coarse_first) {
        ScopedTimer tm(ctx, "score_bound");
        if ((rc = launched_ok(ctx, csm_launch::unit_bounds(ctx->stream, fine_jobs, nq, n_theta_max * lp[0].ncb(), lp[0].cbx,
                                                           lp[0].groups * lp[0].R, lp[0].ncbx, lp[0].ncb()), "unit bounds")))
            return rc;
    } else if (bound_pass) {
        PassPlan fp = lp[0];
        fp.fp32 = true;
        ScopedTimer tm(ctx, "score_bound");
        if ((rc = launch_score_batch(ctx, fine_jobs, nq, fp, n_theta_max, 1)))
            return rc;
    }
    auto finalize = [&]() -> int {
        const size_t lds = (size_t)n_points_max * 8;
        ScopedTimer tm(ctx, "finalize");
        return launched_ok(ctx, csm_launch::finalize_batch(ctx->stream, ctx->device, nq, lds,
                                                           reinterpret_cast<const FinalJob*>(d_fj)), "finalize");
    };
    if (!bound_pass) {
        {
            ScopedTimer tm(ctx, "score_fine");
            if ((rc = launch_score_batch(ctx, fine_jobs, nq, lp[0], n_theta_max, 1)))
                return rc;
        }
        return finalize();
    }
    const int ncb = lp[0].ncb();
    uint32_t* counts = reinterpret_cast<uint32_t*>(ctx->b_items.p);
    uint32_t* items0 = counts + 16;
    uint32_t* items1 = items0 + blocks_total;
    JointList list;
    list.items[0] = items0;
    list.items[1] = items1;
    list.counts = counts;
    list.blocks = (int)std::min<size_t>(blocks_total, 2048);
    const int split_cb = tail_split(ctx, lp[0]) ? lp[0].ncbx * (lp[0].ncby - 1) : ncb;
    /* coarse first: both rounds are one span of the exact pass (a chain counts once among the fine launches) */
    std::optional<ScopedTimer> exact_pass;
    if (coarse_first)
        exact_pass.emplace(ctx, "score_fine");
    for (int round = 1; round <= (two_rounds ? 2 : 1); ++round) {
        {
            std::optional<ScopedTimer> tm;
            if (!coarse_first)
                tm.emplace(ctx, "score_fine");
            HIP_TRY(ctx, hipMemsetAsync(counts, 0, 8, ctx->stream));
            if ((rc = launched_ok(ctx, csm_launch::bound_select(ctx->stream, fine_jobs, nq, ncb, split_cb, items0, items1,
                                                                counts, (uint32_t)blocks_total, round), "bound selection")))
                return rc;
            if ((rc = launch_score_batch(ctx, fine_jobs, nq, lp[0], n_theta_max, 1, 0, &list)))
                return rc;
        }
        if ((rc = finalize()))
            return rc;
    }
    return CSM_OK;
}

/* Stage 7. Resident mode: asynchronous, the records stay on the device and the pinned block of the
 * job tables is held until the chain has run. Otherwise the records in query order go to the
 * device copy (csm_copy_last_batch_records) and to the host, where flagged queries take the exact
 * path and the summaries are completed. */
int BatchGroup::finish()
{
    int rc;
    if (resident) {
        const hipEvent_t done = take_event(ctx);
        if (!done)
            return fail(ctx, CSM_EIO, "resident batch: no event to hold the job tables by");
        HIP_TRY(ctx, hipEventRecord(done, ctx->stream));
        ctx->resident_hold.emplace_back(done, std::move(tables));
        return CSM_OK;
    }
    csm_result* rec_dev = reinterpret_cast<csm_result*>(ctx->rec_dev.p);
    if (rec_dev) {
        if ((rc = launched_ok(ctx, csm_launch::scatter_records(ctx->stream, d_out, reinterpret_cast<const int32_t*>(d_idx),
                                                               rec_dev, nq), "record scatter")))
            return rc;
    }
    tick("launch");
    std::vector<csm_result> res(nq);
    HIP_TRY(ctx, hipMemcpyAsync(res.data(), d_out, (size_t)nq * sizeof(csm_result),
                                hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    tick("gpu wait");

    for (int k = 0; k < nq; ++k) {
        const csm_loop_query& q = queries[idx[k]];
        csm_summary& o = out[idx[k]];
        if (res[k].flags & (CSM_FLAG_EDGE_BAND | CSM_FLAG_KEY_TIE | CSM_FLAG_PROJ_DELTA)) {
            if (spec.bnb) {
                if ((rc = bnb_literal(ctx, q, pp[k], o, spec.bnb_params, &res[k])))
                    return rc;
            } else {
                /* exact single-query path (host-verified projection, tie replay,
                 * literal sweep) */
                const uint32_t why = res[k].flags;
                csm_summary one;
                if ((rc = csm_correlative_match(ctx, q.map_id, &q.geometry, &q.scan, q.initial_pose,
                                                spec.csm_params, &one)))
                    return rc;
                res[k] = one.raw;
                res[k].flags |= why & CSM_FLAG_PROJ_DELTA;
            }
            if (rec_dev) {
                /* fixed up on the host: patch the device copy (the source stays alive in the ctx) */
                ctx->rec_patch.push_back(res[k]);
                HIP_TRY(ctx, hipMemcpyAsync(rec_dev + idx[k], &ctx->rec_patch.back(), sizeof(csm_result),
                                            hipMemcpyHostToDevice, ctx->stream));
            }
        }
        o.raw = res[k];
        o.pose_found = o.raw.found;
        /* scan_matcher_branch_bound.cpp:238-247 */
        o.best_sensor_pose[0] = o.sensor_pose[0] + o.step_x * o.raw.best_x;
        o.best_sensor_pose[1] = o.sensor_pose[1] + o.step_y * o.raw.best_y;
        o.best_sensor_pose[2] = o.sensor_pose[2] + o.step_theta * o.raw.best_theta;
        csm_host_move_backward(o.best_sensor_pose, q.scan.relative_sensor_pose, o.estimated_pose);
        o.candidates = (int64_t)pp[k].n_theta * nx * ny;
    }
    tick("finish");
    return CSM_OK;
}

/* One group of queries that share (nx, ny): the whole device pipeline. */
static int run_batch_group(csm_ctx* ctx, const csm_loop_query* queries, const std::vector<int>& idx,
                           const std::vector<std::vector<int>>& levels, const BatchSpec& spec, csm_summary* out, const ResidentBatch* resident = nullptr)
{
    BatchGroup g(ctx, queries, idx, levels, spec, out, resident);
    g.tick(nullptr);
    int rc = g.plan();
    if (!rc) rc = g.stage_scans();
    if (!rc) rc = g.size_workspaces();
    if (!rc) rc = g.fill_job_tables();
    if (!rc) rc = g.upload_tables();
    if (!rc) rc = g.launch_chain();
    if (!rc) rc = g.finish();
    if (g.tables.p)                       /* not held by a resident chain: the copy has run (or failed) */
        ctx->pin_free.push_back(std::move(g.tables));
    return rc;
}

/* The loop-detection batches once their arguments are checked: pyramid levels built and cached
 * per map id, as mPrecompMaps does (loop_detector_branch_bound.cpp:83-89), all missing ones in
 * one launch; then one run_batch_group per leaf-window shape. */
static int loop_batch(csm_ctx* ctx, const csm_loop_query* queries, int n_queries, BatchSpec spec, csm_summary* out)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int H = spec.H;
    const bool host_timing = ctx->tune.host_timing && spec.bnb;   /* the branch-and-bound batch's ticks */
    const auto tb0 = std::chrono::steady_clock::now();
    if (int rc = begin_batch_records(ctx, n_queries))
        return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if (host_timing)
        fprintf(stderr, "[bnb batch] begin_records %8.3f ms\n", std::chrono::duration<double, std::milli>(t0 - tb0).count());
    std::vector<std::vector<int>> levels(n_queries, std::vector<int>(H + 1, 0));
    PendingBoxes pending_levels;      /* an error return before the launch leaves what it holds stale */
    std::vector<double> max_range(n_queries, 0.0);
    {
        const int i = scans_finite_max(queries, n_queries, max_range.data());
        if (i >= 0 && (!queries[i].scan.angles || !queries[i].scan.ranges || queries[i].scan.n_points < 1))
            return fail(ctx, CSM_EINVAL, "query %d: empty scan", i);
        if (i >= 0)
            return fail(ctx, CSM_EINVAL, "query %d: scan holds a non-finite range or angle", i);
    }
    for (int i = 0; i < n_queries; ++i) {
        DeviceGrid* g = find_grid(ctx, queries[i].map_id);
        if (!g)
            return fail(ctx, CSM_ENOENT, "query %d: map %llu not resident", i,
                        (unsigned long long)queries[i].map_id);
        for (int h = 0; h <= H; ++h)      /* h = 0: the map itself */
            if (int rc = level_for_window(ctx, *g, spec.stride[h], &levels[i][h], &pending_levels))
                return rc;
    }
    if (int rc = launch_box_jobs(ctx, pending_levels))
        return rc;
    const auto t1 = std::chrono::steady_clock::now();
    if (host_timing)
        fprintf(stderr, "[bnb batch] levels        %8.3f ms\n", std::chrono::duration<double, std::milli>(t1 - t0).count());

    /* group queries by leaf-window shape */
    std::memset(out, 0, sizeof(csm_summary) * (size_t)n_queries);
    std::map<std::pair<int, int>, std::vector<int>> groups;
    for (int i = 0; i < n_queries; ++i) {
        double sx, sy, st;
        search_step_from_max(queries[i].geometry.resolution, max_range[i], &sx, &sy, &st);
        groups[{ padded_extent(csm_host_window(spec.range_x, sx), spec.unit),
                 padded_extent(csm_host_window(spec.range_y, sy), spec.unit) }].push_back(i);
    }
    spec.max_range = max_range.data();
    for (auto& kv : groups) {
        if (host_timing)
            fprintf(stderr, "[bnb batch] grouping      %8.3f ms\n",
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
        if (int rc = run_batch_group(ctx, queries, kv.second, levels, spec, out))
            return rc;
    }
    const auto t2 = std::chrono::steady_clock::now();
    const double setup = std::chrono::duration<double, std::micro>(t1 - t0).count();
    const double opt = std::chrono::duration<double, std::micro>(t2 - t1).count();
    for (int i = 0; i < n_queries; ++i) {
        out[i].input_setup_us = setup / n_queries;
        out[i].optimization_us = opt / n_queries;
    }
    return CSM_OK;
}

} /* namespace csm_host */

extern "C" {


int csm_bnb_match_batch(csm_ctx* ctx, const csm_loop_query* queries, int32_t n_queries,
                        const csm_bnb_params* prm, csm_summary* out)
{
    if (!ctx || !queries || n_queries < 1 || !prm || !out || prm->node_height_max < 0 ||
        prm->node_height_max >= kMaxElig)
        return fail(ctx, CSM_EINVAL, "csm_bnb_match_batch: bad arguments");
    BatchSpec spec;
    spec.bnb = true;
    spec.H = prm->node_height_max;
    for (int h = 0; h <= spec.H; ++h)
        spec.stride[h] = 1 << h;
    spec.unit = 1 << spec.H;
    spec.range_x = prm->range_x;
    spec.range_y = prm->range_y;
    spec.range_theta = prm->range_theta;
    spec.score_thr = prm->score_threshold;
    spec.known_thr = prm->known_rate_threshold;
    spec.bnb_params = prm;
    return loop_batch(ctx, queries, n_queries, spec, out);
}

/* LoopDetectorCorrelative::Detect's search part for a batch of queries
 * (src/mapping/loop_detector_correlative.cpp:59-156 lines 68-108): one coarse
 * map per local map id, cached on the device like mPrecompMaps. */
int csm_correlative_match_batch(csm_ctx* ctx, const csm_loop_query* queries, int32_t n_queries,
                                const csm_correlative_params* prm, csm_summary* out)
{
    if (!ctx || !queries || n_queries < 1 || !prm || !out || prm->low_resolution < 1)
        return fail(ctx, CSM_EINVAL, "csm_correlative_match_batch: bad arguments");
    const int L = prm->low_resolution;
    BatchSpec spec;
    spec.bnb = false;
    spec.H = L > 1 ? 1 : 0;
    spec.stride[1] = L;
    spec.unit = L;
    spec.range_x = prm->range_x;
    spec.range_y = prm->range_y;
    spec.range_theta = prm->range_theta;
    spec.score_thr = prm->score_threshold;
    spec.known_thr = prm->known_rate_threshold;
    spec.csm_params = prm;
    return loop_batch(ctx, queries, n_queries, spec, out);
}

/* csm_score_window_dev for many windows at once: one launch chain (k_bin_batch,
 * the batched scoring kernels, k_finalize_batch) over all of them. */
int csm_score_windows_dev(csm_ctx* ctx, int32_t n, const uint64_t* map_ids, const csm_window* windows,
                          const int32_t* const* hit_col_dev, const int32_t* const* hit_row_dev,
                          csm_result* out_dev)
{
    return csm_score_windows_dump_dev(ctx, n, map_ids, windows, hit_col_dev, hit_row_dev, out_dev, nullptr,
                                      nullptr, nullptr);
}

int csm_score_windows_dump_dev(csm_ctx* ctx, int32_t n, const uint64_t* map_ids, const csm_window* windows,
                               const int32_t* const* hit_col_dev, const int32_t* const* hit_row_dev,
                               csm_result* out_dev, uint32_t* const* dump_s_dev, uint16_t* const* dump_k_dev,
                               float* const* dump_f_dev)
{
    if (!ctx || n < 1 || !map_ids || !windows || !hit_col_dev || !hit_row_dev || !out_dev)
        return fail(ctx, CSM_EINVAL, "csm_score_windows_dev: bad arguments");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<csm_loop_query> queries((size_t)n);
    std::vector<std::vector<int>> levels((size_t)n, std::vector<int>(2, 0));
    /* windows that share the candidate domain, the coarse window and the merge mode go together */
    std::map<std::array<int, 4>, std::vector<int>> groups;
    for (int i = 0; i < n; ++i) {
        const csm_window& w = windows[i];
        if (w.n_theta < 1 || (w.n_theta & 1) == 0 || w.n_points < 1 || w.win_x < 0 || w.win_y < 0 ||
            w.low_resolution < 1 || !hit_col_dev[i] || !hit_row_dev[i])
            return fail(ctx, CSM_EINVAL, "window %d: bad window", i);
        DeviceGrid* g = find_grid(ctx, map_ids[i]);
        if (!g)
            return fail(ctx, CSM_ENOENT, "window %d: map %llu not resident", i,
                        (unsigned long long)map_ids[i]);
        const int L = w.low_resolution;
        if (L > 1) {
            if (!level_holds(*g, w.coarse_level, L))
                return fail(ctx, CSM_ENOENT, "window %d: level %d does not hold box-max(%d)", i,
                            w.coarse_level, L);
            levels[i][1] = w.coarse_level;
        }
        std::memset(&queries[i], 0, sizeof(csm_loop_query));
        queries[i].map_id = map_ids[i];
        groups[{ padded_extent(w.win_x, L), padded_extent(w.win_y, L), L, w.merge_mode }].push_back(i);
    }
    ResidentBatch resident { windows, hit_col_dev, hit_row_dev, out_dev, dump_s_dev, dump_k_dev, dump_f_dev };
    /* drop the tables of earlier calls whose launch chains have completed */
    while (!ctx->resident_hold.empty()) {
        const bool full = ctx->resident_hold.size() >= 256;
        hipEvent_t ev = ctx->resident_hold.front().first;
        if (full)
            HIP_TRY(ctx, hipEventSynchronize(ev));
        else if (hipEventQuery(ev) != hipSuccess)
            break;
        ctx->event_pool.push_back(ev);
        ctx->pin_free.push_back(std::move(ctx->resident_hold.front().second));
        ctx->resident_hold.erase(ctx->resident_hold.begin());
    }
    for (auto& kv : groups) {
        const int L = kv.first[2];
        BatchSpec spec;
        spec.bnb = false;
        spec.H = L > 1 ? 1 : 0;
        spec.stride[1] = L;
        spec.unit = L;
        int rc = run_batch_group(ctx, queries.data(), kv.second, levels, spec, nullptr, &resident);
        if (rc)
            return rc;
    }
    return CSM_OK;
}

int csm_copy_last_batch_records(csm_ctx* ctx, csm_result* dst_dev)
{
    if (!ctx || !dst_dev)
        return fail(ctx, CSM_EINVAL, "csm_copy_last_batch_records: bad arguments");
    if (ctx->rec_n < 1 || !ctx->rec_dev.p)
        return fail(ctx, CSM_ENOENT, "no batch has been scored on this context");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(dst_dev, ctx->rec_dev.p, (size_t)ctx->rec_n * sizeof(csm_result),
                                hipMemcpyDeviceToDevice, ctx->stream));
    return CSM_OK;
}

int csm_bound_pass_stats(csm_ctx* ctx, uint64_t* blocks_scored, uint64_t* blocks_skipped)
{
    if (!ctx)
        return CSM_EINVAL;
    uint32_t h[2] = { 0, 0 };
    if (ctx->bound_stats.p) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipMemcpyAsync(h, ctx->bound_stats.p, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(ctx->bound_stats.p, 0, 8, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (blocks_scored) *blocks_scored = h[0];
    if (blocks_skipped) *blocks_skipped = h[1];
    return CSM_OK;
}

} /* extern "C" */

#ifdef CSM_BIN_TIMING
/* tuning builds only (tools/build_variant.sh NAME -DCSM_BIN_TIMING): reads and clears k_bin's phase counters */
extern "C" int csm_debug_bin_cycles(unsigned long long* out16)
{
    /* out16[0..5]: cycles per phase (8..11: parts of pass A) summed over the workgroups of the LAST launch
     * pattern (rows are overwritten by every launch), out16[15]: workgroups */
    if (!g_bin_debug)
        return CSM_ENOENT;
    std::vector<unsigned long long> rows((size_t)kBinDebugRows * 16);
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(rows.data(), g_bin_debug, rows.size() * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return CSM_EIO;
    for (int k = 0; k < 16; ++k)
        out16[k] = 0;
    for (int r = 0; r < kBinDebugRows; ++r) {
        if (!rows[(size_t)r * 16 + 7])
            continue;
        for (int k = 0; k < 12; ++k)
            if (k != 7)
                out16[k] += rows[(size_t)r * 16 + k];
        out16[15] += 1;
    }
    return CSM_OK;
}
#endif

