/* csm_posegraph_api.hip -- host side of the pose-graph optimizer (PoseGraphOptimizerLM with the
 * ConjugateGradient solver or the direct Schur-complement Cholesky solver): validation, the block
 * structure of H with the ordered contribution list of every stored block (and of every block of the
 * Schur complement), the host restatement csm_host_pose_graph_lm (the CPU reference) and the device
 * entry csm_pose_graph_lm, whose kernels are in csm_posegraph_kernels.hip; the marginal covariances of
 * node pairs from the Schur factor (csm_pose_graph_marginals, its host restatement) and the host helpers
 * that turn them into a search window, a gate and a prior. A translation unit of
 * libcsm_hip.so of its own. DESIGN.md 4e. */
#include "csm_internal.hpp"

#include "csm_posegraph_kernels.hip"

#include <unordered_map>

namespace {

constexpr int kPgMaxNodes = 1 << 24;     /* 2 * 3 * nodes stays an int (the CG's iteration cap) */

/* the graph as both solvers read it: inputs in node indices, the incidence lists, the distinct
 * cross blocks and the rows of H */
struct PgGraph {
    int n_local = 0, n_nodes = 0, n_vars = 0, n_edges = 0, n_cross = 0;
    std::vector<double> rel, info;
    std::vector<int32_t> enode, is_loop, node_ptr, node_edges, cross_ptr, cross_edges, row_ptr, row_col, row_ent;
    /* the Schur complement on the local map nodes (pg_build_schur): its stored 3x3 blocks (s1 >= s2,
     * the n_local diagonal ones first) and, per block, the cross-block pairs of the scan nodes adjacent
     * to both, in ascending scan node order */
    int n_sblk = 0;
    std::vector<int32_t> sb_rc, sb_ptr, sb_pair;
};

const char* pg_check(const double* local_poses, int n_local, const double* scan_poses, int n_scan,
                     const csm_pose_graph_edge* edges, int n_edges, const csm_pose_graph_lm_params* p,
                     const double* lambda)
{
    if (!p || !lambda || !local_poses || n_local < 1 || n_scan < 0 || (n_scan > 0 && !scan_poses) || n_edges < 0 ||
        (n_edges > 0 && !edges) || (int64_t)n_local + n_scan > kPgMaxNodes)
        return "bad arguments";
    if (p->solver_type == CSM_PG_SOLVER_SPARSE_CHOLESKY)
        return "SolverType SparseCholesky (SimplicialLDLT) is not provided; use ConjugateGradient";
    if (p->solver_type != CSM_PG_SOLVER_CONJUGATE_GRADIENT && p->solver_type != CSM_PG_SOLVER_SCHUR_CHOLESKY)
        return "unknown solver type";
    if (p->solver_type == CSM_PG_SOLVER_SCHUR_CHOLESKY && n_local > CSM_PG_SCHUR_MAX_LOCAL)
        return "n_local exceeds CSM_PG_SCHUR_MAX_LOCAL (the Schur complement is stored dense)";
    if (p->loss_type < CSM_PG_LOSS_SQUARED || p->loss_type > CSM_PG_LOSS_WELSCH)
        return "unknown loss type";
    if (p->iterations_max < 1)
        return "iterations_max < 1";
    if (std::isnan(p->error_tolerance) || !std::isfinite(p->loss_scale) || p->loss_scale < 0.0 ||
        !std::isfinite(*lambda))
        return "non-finite or negative parameter";
    for (int i = 0; i < 3 * n_local; ++i)
        if (!std::isfinite(local_poses[i]))
            return "non-finite local map node pose";
    for (int i = 0; i < 3 * n_scan; ++i)
        if (!std::isfinite(scan_poses[i]))
            return "non-finite scan node pose";
    for (int e = 0; e < n_edges; ++e) {
        const csm_pose_graph_edge& E = edges[e];
        if (E.local_map_index < 0 || E.local_map_index >= n_local || E.scan_index < 0 || E.scan_index >= n_scan)
            return "edge node index out of range";
        for (int j = 0; j < 3; ++j)
            if (!std::isfinite(E.relative_pose[j]))
                return "non-finite edge relative pose";
        for (int j = 0; j < 9; ++j)
            if (!std::isfinite(E.information[j]))
                return "non-finite edge information matrix";
    }
    return nullptr;
}

void pg_build(int n_local, int n_scan, const csm_pose_graph_edge* edges, int n_edges, PgGraph& G)
{
    const int N = n_local + n_scan;
    G.n_local = n_local;
    G.n_nodes = N;
    G.n_vars = 3 * N;
    G.n_edges = n_edges;
    G.rel.resize(3 * (size_t)n_edges);
    G.info.resize(9 * (size_t)n_edges);
    G.enode.resize(2 * (size_t)n_edges);
    G.is_loop.resize(n_edges);
    std::vector<int32_t> cross_of(n_edges);
    std::unordered_map<int64_t, int32_t> pair_id;
    std::vector<std::pair<int32_t, int32_t>> pairs;       /* (end node, start node) of cross block u */
    G.node_ptr.assign(N + 1, 0);
    for (int e = 0; e < n_edges; ++e) {
        const csm_pose_graph_edge& E = edges[e];
        const int s = E.local_map_index, t = n_local + E.scan_index;
        std::memcpy(&G.rel[3 * (size_t)e], E.relative_pose, 3 * sizeof(double));
        std::memcpy(&G.info[9 * (size_t)e], E.information, 9 * sizeof(double));
        G.enode[2 * e] = s;
        G.enode[2 * e + 1] = t;
        G.is_loop[e] = E.is_loop ? 1 : 0;
        ++G.node_ptr[s + 1];
        ++G.node_ptr[t + 1];
        const int64_t key = (int64_t)t * N + s;
        auto it = pair_id.find(key);
        if (it == pair_id.end()) {
            it = pair_id.emplace(key, (int32_t)pairs.size()).first;
            pairs.emplace_back(t, s);
        }
        cross_of[e] = it->second;
    }
    const int U = (int)pairs.size();
    G.n_cross = U;
    for (int k = 0; k < N; ++k)
        G.node_ptr[k + 1] += G.node_ptr[k];
    G.node_edges.resize(2 * (size_t)n_edges);
    G.cross_ptr.assign(U + 1, 0);
    for (int e = 0; e < n_edges; ++e)
        ++G.cross_ptr[cross_of[e] + 1];
    for (int u = 0; u < U; ++u)
        G.cross_ptr[u + 1] += G.cross_ptr[u];
    G.cross_edges.resize(n_edges);
    {
        std::vector<int32_t> fill(G.node_ptr.begin(), G.node_ptr.end() - 1);
        std::vector<int32_t> cfill(G.cross_ptr.begin(), G.cross_ptr.end() - 1);
        for (int e = 0; e < n_edges; ++e) {          /* edge order within every list */
            G.node_edges[fill[G.enode[2 * e]]++] = e;
            G.node_edges[fill[G.enode[2 * e + 1]]++] = e;
            G.cross_edges[cfill[cross_of[e]]++] = e;
        }
    }
    /* rows: per node its diagonal block and one block per distinct neighbour, ascending column */
    std::vector<std::vector<std::pair<int32_t, int32_t>>> rows(N);
    for (int k = 0; k < N; ++k)
        rows[k].emplace_back(k, (k << 2) | (G.node_ptr[k] == G.node_ptr[k + 1] ? kPgDiagOnly : 0));
    for (int u = 0; u < U; ++u) {
        const int t = pairs[u].first, s = pairs[u].second, slot = N + u;
        rows[t].emplace_back(s, slot << 2);
        rows[s].emplace_back(t, (slot << 2) | kPgTransposed);
    }
    G.row_ptr.assign(N + 1, 0);
    G.row_col.clear();
    G.row_ent.clear();
    G.row_col.reserve(N + 2 * (size_t)U);
    G.row_ent.reserve(N + 2 * (size_t)U);
    for (int k = 0; k < N; ++k) {
        std::sort(rows[k].begin(), rows[k].end());
        for (const auto& ce : rows[k]) {
            G.row_col.push_back(ce.first);
            G.row_ent.push_back(ce.second);
        }
        G.row_ptr[k + 1] = (int32_t)G.row_col.size();
    }
}

/* which scan nodes contribute to which block of S = A - B^T D^-1 B: a scan node with d distinct
 * neighbours contributes to d (d + 1) / 2 blocks. Returns false when the lists would not fit an int. */
bool pg_build_schur(PgGraph& G)
{
    const int nl = G.n_local;
    std::unordered_map<int64_t, int32_t> block_id;
    std::vector<std::vector<int32_t>> lists(nl);
    G.sb_rc.clear();
    for (int s = 0; s < nl; ++s) {
        G.sb_rc.push_back(s);
        G.sb_rc.push_back(s);
    }
    int64_t total = 0;
    for (int t = nl; t < G.n_nodes; ++t) {             /* ascending t: every list ends up in that order */
        const int q0 = G.row_ptr[t], q1 = G.row_ptr[t + 1];
        for (int a = q0; a < q1; ++a) {
            if (G.row_col[a] == t)
                continue;
            for (int b = q0; b <= a; ++b) {            /* columns ascend, so s1 = col[a] >= s2 = col[b] */
                const int s1 = G.row_col[a], s2 = G.row_col[b];
                int32_t id = s1;
                if (s1 != s2) {
                    const int64_t key = (int64_t)s1 * nl + s2;
                    auto it = block_id.find(key);
                    if (it == block_id.end()) {
                        it = block_id.emplace(key, (int32_t)lists.size()).first;
                        lists.emplace_back();
                        G.sb_rc.push_back(s1);
                        G.sb_rc.push_back(s2);
                    }
                    id = it->second;
                }
                lists[id].push_back((G.row_ent[a] >> 2) - G.n_nodes);
                lists[id].push_back((G.row_ent[b] >> 2) - G.n_nodes);
                if (++total > (INT32_MAX / 4))
                    return false;
            }
        }
    }
    G.n_sblk = (int)lists.size();
    G.sb_ptr.assign(G.n_sblk + 1, 0);
    G.sb_pair.clear();
    G.sb_pair.reserve(2 * (size_t)total);
    for (int q = 0; q < G.n_sblk; ++q) {
        G.sb_pair.insert(G.sb_pair.end(), lists[q].begin(), lists[q].end());
        G.sb_ptr[q + 1] = (int32_t)(G.sb_pair.size() / 2);
    }
    return true;
}

/* the n_s = 3 n_local rounded up to whole tiles of the blocked factorization */
int pg_schur_padded(int n_local) { return ceil_div(3 * n_local, kPgsTile) * kPgsTile; }

void pg_job_structure(const PgGraph& G, const csm_pose_graph_lm_params& p, double lambda, PgJob& J)
{
    J.n_local = G.n_local;
    J.n_nodes = G.n_nodes;
    J.n_vars = G.n_vars;
    J.n_edges = G.n_edges;
    J.n_cross = G.n_cross;
    J.iterations_max = p.iterations_max;
    J.loss_type = p.loss_type;
    J.cg_max = 2 * G.n_vars;              /* IterativeSolverBase::maxIterations(): 2 * cols */
    J.error_tolerance = p.error_tolerance;
    J.loss_scale = p.loss_scale;
    J.lambda = lambda;
}

/* the host job reads the graph's own lists */
void pg_host_lists(const PgGraph& G, PgJob& J)
{
    J.rel = G.rel.data();
    J.info = G.info.data();
    J.enode = G.enode.data();
    J.is_loop = G.is_loop.data();
    J.node_ptr = G.node_ptr.data();
    J.node_edges = G.node_edges.data();
    J.cross_ptr = G.cross_ptr.data();
    J.cross_edges = G.cross_edges.data();
    J.row_ptr = G.row_ptr.data();
    J.row_col = G.row_col.data();
    J.row_ent = G.row_ent.data();
}

/* step 2 on the host: the stored blocks of S into the dense row-major matrix (3 n_local square) */
void pg_host_schur_matrix(const PgGraph& G, const PgJob& J, const double* w, std::vector<double>& S)
{
    const int ns = 3 * G.n_local;
    std::fill(S.begin(), S.end(), 0.0);
    for (int q = 0; q < G.n_sblk; ++q)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                S[(3 * (size_t)G.sb_rc[2 * q] + i) * ns + 3 * (size_t)G.sb_rc[2 * q + 1] + j] =
                    pg_schur_entry(J, G.sb_rc.data(), G.sb_ptr.data(), G.sb_pair.data(), w, q, i, j);
}

/* step 3 on the host: the scalar LDL^T in place, L below the diagonal, d on it */
void pg_host_ldl(std::vector<double>& S, int ns, std::vector<double>& wrow)
{
    for (int i = 0; i < ns; ++i) {
        double* ri = &S[(size_t)i * ns];
        for (int j = 0; j <= i; ++j) {
            const double* rj = &S[(size_t)j * ns];
            double v = ri[j];
            for (int k = 0; k < j; ++k)
                v -= wrow[k] * rj[k];
            if (j < i) {
                const double l = v / rj[j];
                ri[j] = l;
                wrow[j] = l * rj[j];
            } else {
                ri[i] = v;
            }
        }
    }
}

/* Optimize, statement by statement and in sequence: the reference the device is held to */
void pg_host_run(const PgGraph& G, const csm_pose_graph_lm_params& p, std::vector<double>& pose, double& lambda,
                 csm_pose_graph_lm_info* info, csm_pose_graph_lm_step* trace)
{
    const int n = G.n_vars;
    const bool schur = p.solver_type == CSM_PG_SOLVER_SCHUR_CHOLESKY;
    std::vector<double> ev((size_t)kPgEdgeVals * G.n_edges), bv(9 * ((size_t)G.n_nodes + G.n_cross));
    std::vector<double> b(n), invd(n), x(n), r(n), z(n), pv(n), ap(n);
    PgJob J {};
    pg_job_structure(G, p, lambda, J);
    J.pose = pose.data();
    pg_host_lists(G, J);
    J.ev = ev.data();
    J.bv = bv.data();
    auto total_error = [&]() {
        double t = 0.0;
        for (int e = 0; e < G.n_edges; ++e)
            t += pg_edge_loss(&pose[3 * (size_t)G.enode[2 * e]], &pose[3 * (size_t)G.enode[2 * e + 1]],
                              &G.rel[3 * (size_t)e], &G.info[9 * (size_t)e], p.loss_type, p.loss_scale);
        return t;
    };
    auto dot = [n](const std::vector<double>& a, const std::vector<double>& c) {
        double s = 0.0;
        for (int i = 0; i < n; ++i)
            s += a[i] * c[i];
        return s;
    };
    J.b = b.data();
    J.invd = invd.data();
    /* conjugate_gradient with x0 = 0: residual = b. Returns |r|^2 and the iteration count. */
    auto solve_cg = [&](double rhs2, int& cg) {
        std::fill(x.begin(), x.end(), 0.0);
        r = b;
        double r2 = rhs2;
        cg = 0;
        if (rhs2 != 0.0) {
            const double a = DBL_EPSILON * DBL_EPSILON * rhs2;
            const double thr = (a < DBL_MIN) ? DBL_MIN : a;
            if (!(r2 < thr)) {
                for (int i = 0; i < n; ++i)
                    pv[i] = invd[i] * r[i];
                double abs_new = dot(r, pv);
                for (; cg < J.cg_max; ++cg) {
                    for (int i = 0; i < n; ++i)
                        ap[i] = pg_row_times(J, i, pv.data());
                    const double alpha = abs_new / dot(pv, ap);
                    for (int i = 0; i < n; ++i)
                        x[i] += alpha * pv[i];
                    for (int i = 0; i < n; ++i)
                        r[i] -= alpha * ap[i];
                    r2 = dot(r, r);
                    if (r2 < thr)
                        break;
                    for (int i = 0; i < n; ++i)
                        z[i] = invd[i] * r[i];
                    const double abs_old = abs_new;
                    abs_new = dot(r, z);
                    const double beta = abs_new / abs_old;
                    for (int i = 0; i < n; ++i)
                        pv[i] = z[i] + beta * pv[i];
                }
            }
        }
        return r2;
    };
    /* block elimination of the scan nodes, dense LDL^T of the Schur complement (steps 1 - 5 of
     * DESIGN.md 4e, "direct solver"). Returns the true |b - H x|^2. */
    const int ns = 3 * G.n_local;
    std::vector<double> S, g, w, wrow;
    if (schur) {
        S.resize((size_t)ns * ns);
        g.resize(3 * (size_t)(G.n_nodes - G.n_local));
        w.resize(9 * (size_t)G.n_cross);
        wrow.resize(ns);
    }
    auto solve_schur = [&]() {
        for (int t = G.n_local; t < G.n_nodes; ++t)
            pg_eliminate_scan(J, g.data(), w.data(), t);
        pg_host_schur_matrix(G, J, w.data(), S);
        for (int a = 0; a < ns; ++a)
            x[a] = pg_schur_rhs(J, g.data(), a / 3, a % 3);
        pg_host_ldl(S, ns, wrow);
        for (int i = 0; i < ns; ++i) {
            double v = x[i];
            for (int k = 0; k < i; ++k)
                v -= S[(size_t)i * ns + k] * x[k];
            x[i] = v;
        }
        for (int i = 0; i < ns; ++i)
            x[i] = x[i] / S[(size_t)i * ns + i];
        for (int i = ns - 1; i >= 0; --i) {
            double v = x[i];
            for (int k = ns - 1; k > i; --k)
                v -= S[(size_t)k * ns + i] * x[k];
            x[i] = v;
        }
        for (int t = G.n_local; t < G.n_nodes; ++t)
            pg_back_scan(J, g.data(), w.data(), x.data(), t);
        double r2 = 0.0;
        for (int i = 0; i < n; ++i) {
            const double ri = b[i] - pg_row_times(J, i, x.data());
            r2 += ri * ri;
        }
        return r2;
    };
    double prev = DBL_MAX, total = DBL_MAX;
    const double initial = total_error();
    int steps = 0;
    int64_t cg_total = 0;
    for (;;) {
        for (int e = 0; e < G.n_edges; ++e)
            pg_edge_values(&pose[3 * (size_t)G.enode[2 * e]], &pose[3 * (size_t)G.enode[2 * e + 1]],
                           &G.rel[3 * (size_t)e], &G.info[9 * (size_t)e], G.is_loop[e], p.loss_type, p.loss_scale,
                           &ev[(size_t)kPgEdgeVals * e]);
        for (int k = 0; k < G.n_nodes; ++k)
            pg_assemble_node(J, k, lambda);
        for (int u = 0; u < G.n_cross; ++u)
            pg_assemble_cross(J, u);
        const double rhs2 = dot(b, b);
        int cg = 0;
        const double r2 = schur ? solve_schur() : solve_cg(rhs2, cg);
        for (int i = 0; i < n; ++i)
            pose[i] += x[i];
        total = total_error();
        if (trace) {
            csm_pose_graph_lm_step& s = trace[steps];
            std::memset(&s, 0, sizeof(s));
            s.total_error = total;
            s.lambda = lambda;
            s.rhs_norm2 = rhs2;
            s.residual_norm2 = r2;
            s.cg_iterations = cg;
        }
        cg_total += cg;
        if (++steps >= p.iterations_max || std::fabs(prev - total) < p.error_tolerance)
            break;
        lambda = (total < prev) ? lambda * 0.5 : lambda * 2.0;
        prev = total;
    }
    if (info) {
        std::memset(info, 0, sizeof(*info));
        info->steps = steps;
        info->cg_iterations = cg_total;
        info->initial_error = initial;
        info->final_error = total;
        info->final_lambda = lambda;
    }
}

/* One launch of a chain on the context's stream. A chain keeps the first code that is not 0 in `e` and
 * hands it to launched_ok where the chain, or a step of it, ends. */
template <class... P, class... A>
void pg_launch(csm_ctx* ctx, int& e, void (*kernel)(P...), dim3 grid, dim3 block, const A&... args)
{
    keep_first(e, launch(kernel, grid, block, ctx->stream, args...));
}

/* grids of kPgsBlock threads: one thread per item; a grid-stride loop over the cells of a matrix */
dim3 pg_over(int64_t count) { return dim3((unsigned)((count + kPgsBlock - 1) / kPgsBlock)); }
dim3 pg_strided(int64_t cells) { return dim3((unsigned)std::min<int64_t>((cells + kPgsBlock - 1) / kPgsBlock, 16384)); }

/* the blocked LDL^T of S in place: per panel its diagonal tile, then the panel below it and the trailing update */
void pg_ldl_launches(csm_ctx* ctx, int& e, const PgSchurJob& Q)
{
    const int nt = Q.np / kPgsTile;
    for (int p = 0; p < nt; ++p) {
        pg_launch(ctx, e, k_pgs_ldl_diag, dim3(1), dim3(kPgsBlock), Q, p);
        const int below = nt - p - 1;
        if (below) {
            pg_launch(ctx, e, k_pgs_ldl_panel, dim3(ceil_div(below * kPgsTile, 64)), dim3(64), Q, p);
            pg_launch(ctx, e, k_pgs_ldl_update, dim3(below, below), dim3(kPgsBlock), Q, p);
        }
    }
}

/* the direct solver's launches for one Optimize call: the initial total error, then the chain of one
 * LM step iterations_max times (a step's kernels return at once after the step that stopped) */
int pg_schur_chain(csm_ctx* ctx, const PgSchurJob& Q, bool small)
{
    const PgJob& J = Q.J;
    const dim3 blk(kPgsBlock);
    const int n_scan = J.n_nodes - J.n_local;
    int e = 0;
    if (J.n_edges)
        pg_launch(ctx, e, k_pgs_error, pg_over(J.n_edges), blk, Q);
    pg_launch(ctx, e, k_pgs_decide, dim3(1), blk, Q, 1);
    for (int it = 0; it < J.iterations_max; ++it) {
        if (J.n_edges)
            pg_launch(ctx, e, k_pgs_edges, pg_over(J.n_edges), blk, Q);
        pg_launch(ctx, e, k_pgs_assemble, pg_over((int64_t)J.n_nodes + J.n_cross), blk, Q);
        if (n_scan)
            pg_launch(ctx, e, k_pgs_eliminate, pg_over(n_scan), blk, Q);
        if (small) {
            pg_launch(ctx, e, k_pgs_small, dim3(1), blk, Q);
        } else {
            pg_launch(ctx, e, k_pgs_clear, pg_strided((int64_t)Q.np * Q.np), blk, Q);
            pg_launch(ctx, e, k_pgs_schur, pg_over(9 * (int64_t)Q.n_sblk + Q.np), blk, Q);
            pg_ldl_launches(ctx, e, Q);
            pg_launch(ctx, e, k_pgs_solve, dim3(1), dim3(kPgsSolveBlock), Q);
        }
        if (n_scan)
            pg_launch(ctx, e, k_pgs_back, pg_over(n_scan), blk, Q);
        pg_launch(ctx, e, k_pgs_update, dim3(Q.nb_vars), blk, Q);
        if (J.n_edges)
            pg_launch(ctx, e, k_pgs_error, pg_over(J.n_edges), blk, Q);
        pg_launch(ctx, e, k_pgs_decide, dim3(1), blk, Q, 0);
        if (int rc = launched_ok(ctx, e, "pose-graph LM step"))
            return rc;
    }
    return CSM_OK;
}

/* one device call's set-up: the graph, its lists and the LM state staged and uploaded into pg_buf (on the
 * ctx stream), the work vectors carved behind them, pg_s grown for the blocked direct solver; Q.J alone
 * serves the conjugate-gradient kernel */
int pg_device_job(csm_ctx* ctx, const PgGraph& G, const double* local_poses, int n_local, const double* scan_poses,
                  int n_scan, const csm_pose_graph_lm_params* params, const double* lambda, bool schur, bool small,
                  PgSchurJob& Q)
{
    const int n = G.n_vars, E = G.n_edges, NB = G.n_nodes + G.n_cross, R = (int)G.row_col.size();
    const int n_out = 4 + 5 * params->iterations_max;
    /* inputs (uploaded): pose, rel, info, then the int lists; work and output after them */
    Carve c;
    const size_t o_pose = c.take(8 * (size_t)n), o_rel = c.take(24 * (size_t)E), o_info = c.take(72 * (size_t)E);
    const size_t o_enode = c.take(8 * (size_t)E), o_loop = c.take(4 * (size_t)E);
    const size_t o_nptr = c.take(4 * ((size_t)G.n_nodes + 1)), o_nedge = c.take(8 * (size_t)E);
    const size_t o_cptr = c.take(4 * ((size_t)G.n_cross + 1)), o_cedge = c.take(4 * (size_t)E);
    const size_t o_rptr = c.take(4 * ((size_t)G.n_nodes + 1)), o_rcol = c.take(4 * (size_t)R),
                 o_rent = c.take(4 * (size_t)R);
    /* the direct solver's lists and the LM state it keeps on the device */
    const size_t o_sbrc = c.take(schur ? 8 * (size_t)G.n_sblk : 0), o_sbptr = c.take(schur ? 4 * ((size_t)G.n_sblk + 1) : 0),
                 o_sbpair = c.take(schur ? 4 * G.sb_pair.size() : 0), o_state = c.take(schur ? sizeof(PgState) : 0);
    const size_t up_bytes = c.off;
    const size_t o_ev = c.take(8 * (size_t)kPgEdgeVals * E), o_bv = c.take(72 * (size_t)NB);
    size_t o_vec[7];
    for (size_t& o : o_vec)
        o = c.take(8 * (size_t)n);
    const size_t o_out = c.take(8 * (size_t)n_out);
    const int np = pg_schur_padded(n_local), nb_vars = ceil_div(n, kPgsBlock), nb_edges = ceil_div(E, kPgsBlock);
    const size_t o_g = c.take(schur ? 24 * (size_t)n_scan : 0), o_w = c.take(schur ? 72 * (size_t)G.n_cross : 0),
                 o_y = c.take(schur ? 8 * (size_t)np : 0), o_wp = c.take(schur && !small ? 8 * (size_t)np * kPgsTile : 0),
                 o_part = c.take(schur ? 8 * (2 * (size_t)nb_vars + nb_edges) : 0);
    int rc;
    if ((rc = ensure(ctx, ctx->pg_buf, c.off)))
        return rc;
    if (schur && !small && (rc = grow(ctx, ctx->pg_s, 8 * (size_t)np * np, 8 * (size_t)np * np, false)))
        return rc;
    std::vector<uint8_t>& st = ctx->pg_stage;
    st.assign(up_bytes, 0);
    auto put = [&](size_t off, const void* src, size_t bytes) {
        if (bytes)
            std::memcpy(st.data() + off, src, bytes);
    };
    put(o_pose, local_poses, 24 * (size_t)n_local);
    put(o_pose + 24 * (size_t)n_local, scan_poses, 24 * (size_t)n_scan);
    put(o_rel, G.rel.data(), 24 * (size_t)E);
    put(o_info, G.info.data(), 72 * (size_t)E);
    put(o_enode, G.enode.data(), 8 * (size_t)E);
    put(o_loop, G.is_loop.data(), 4 * (size_t)E);
    put(o_nptr, G.node_ptr.data(), 4 * ((size_t)G.n_nodes + 1));
    put(o_nedge, G.node_edges.data(), 8 * (size_t)E);
    put(o_cptr, G.cross_ptr.data(), 4 * ((size_t)G.n_cross + 1));
    put(o_cedge, G.cross_edges.data(), 4 * (size_t)E);
    put(o_rptr, G.row_ptr.data(), 4 * ((size_t)G.n_nodes + 1));
    put(o_rcol, G.row_col.data(), 4 * (size_t)R);
    put(o_rent, G.row_ent.data(), 4 * (size_t)R);
    if (schur) {
        const PgState st0 = { *lambda, DBL_MAX, DBL_MAX, 0.0, 0, 0 };
        put(o_sbrc, G.sb_rc.data(), 8 * (size_t)G.n_sblk);
        put(o_sbptr, G.sb_ptr.data(), 4 * ((size_t)G.n_sblk + 1));
        put(o_sbpair, G.sb_pair.data(), 4 * G.sb_pair.size());
        put(o_state, &st0, sizeof(st0));
    }

    uint8_t* d = reinterpret_cast<uint8_t*>(ctx->pg_buf.p);
    PgJob J {};
    pg_job_structure(G, *params, *lambda, J);
    J.pose = reinterpret_cast<double*>(d + o_pose);
    J.rel = reinterpret_cast<const double*>(d + o_rel);
    J.info = reinterpret_cast<const double*>(d + o_info);
    J.enode = reinterpret_cast<const int32_t*>(d + o_enode);
    J.is_loop = reinterpret_cast<const int32_t*>(d + o_loop);
    J.node_ptr = reinterpret_cast<const int32_t*>(d + o_nptr);
    J.node_edges = reinterpret_cast<const int32_t*>(d + o_nedge);
    J.cross_ptr = reinterpret_cast<const int32_t*>(d + o_cptr);
    J.cross_edges = reinterpret_cast<const int32_t*>(d + o_cedge);
    J.row_ptr = reinterpret_cast<const int32_t*>(d + o_rptr);
    J.row_col = reinterpret_cast<const int32_t*>(d + o_rcol);
    J.row_ent = reinterpret_cast<const int32_t*>(d + o_rent);
    J.ev = reinterpret_cast<double*>(d + o_ev);
    J.bv = reinterpret_cast<double*>(d + o_bv);
    double** vecs[7] = { &J.b, &J.invd, &J.x, &J.r, &J.z, &J.p, &J.ap };
    for (int v = 0; v < 7; ++v)
        *vecs[v] = reinterpret_cast<double*>(d + o_vec[v]);
    J.out = reinterpret_cast<double*>(d + o_out);

    HIP_TRY(ctx, hipMemcpyAsync(d, st.data(), up_bytes, hipMemcpyHostToDevice, ctx->stream));
    Q.J = J;
    Q.n_s = 3 * n_local;
    Q.np = np;
    Q.n_sblk = G.n_sblk;
    Q.nb_vars = nb_vars;
    Q.nb_edges = nb_edges;
    if (schur) {
        Q.sb_rc = reinterpret_cast<const int32_t*>(d + o_sbrc);
        Q.sb_ptr = reinterpret_cast<const int32_t*>(d + o_sbptr);
        Q.sb_pair = reinterpret_cast<const int32_t*>(d + o_sbpair);
        Q.g = reinterpret_cast<double*>(d + o_g);
        Q.w = reinterpret_cast<double*>(d + o_w);
        Q.S = small ? nullptr : ctx->pg_s.as<double>();
        Q.wp = reinterpret_cast<double*>(d + o_wp);
        Q.y = reinterpret_cast<double*>(d + o_y);
        Q.part = reinterpret_cast<double*>(d + o_part);
        Q.st = reinterpret_cast<PgState*>(d + o_state);
    }
    return CSM_OK;
}

/* ------------------------------------------------------------------ marginal covariances */

/* the LM parameters whose checks and structure the marginals share: one step, the direct solver */
csm_pose_graph_lm_params pg_cov_params(int32_t loss_type, double loss_scale)
{
    csm_pose_graph_lm_params p {};
    p.iterations_max = 1;
    p.solver_type = CSM_PG_SOLVER_SCHUR_CHOLESKY;
    p.loss_type = loss_type;
    p.loss_scale = loss_scale;
    return p;
}

/* what the pairs ask for: C (ascending), every node's position in it, the pairs in node indices */
struct PgCovPlan {
    std::vector<int32_t> col_node, col_of, pairs;
};

const char* pg_cov_check(const double* local_poses, int n_local, const double* scan_poses, int n_scan,
                         const csm_pose_graph_edge* edges, int n_edges, int32_t loss_type, double loss_scale,
                         const csm_pose_graph_pair* pairs, int n_pairs, const csm_pose_graph_marginal* out)
{
    const csm_pose_graph_lm_params p = pg_cov_params(loss_type, loss_scale);
    const double lambda = 0.0;
    if (const char* why = pg_check(local_poses, n_local, scan_poses, n_scan, edges, n_edges, &p, &lambda))
        return why;
    if (n_pairs < 1 || !pairs || !out)
        return "n_pairs < 1 or no pairs";
    for (int q = 0; q < n_pairs; ++q)
        if (pairs[q].local_map_index < 0 || pairs[q].local_map_index >= n_local || pairs[q].scan_index < -1 ||
            pairs[q].scan_index >= n_scan)
            return "pair node index out of range";
    return nullptr;
}

/* the refusals that need the graph, then C = {s of every pair} u adj(t of every pair) */
const char* pg_cov_plan(const PgGraph& G, const csm_pose_graph_pair* pairs, int n_pairs, PgCovPlan& P)
{
    const int nl = G.n_local;
    std::vector<int32_t> root(nl);
    for (int s = 0; s < nl; ++s)
        root[s] = s;
    auto find = [&](int s) {
        while (root[s] != s)
            s = root[s] = root[root[s]];
        return s;
    };
    for (int t = nl; t < G.n_nodes; ++t) {
        int first = -1;
        for (int q = G.row_ptr[t]; q < G.row_ptr[t + 1]; ++q) {
            if (G.row_col[q] == t)
                continue;
            if (first < 0)
                first = find(G.row_col[q]);
            else
                root[find(G.row_col[q])] = first;
        }
    }
    for (int s = 1; s < nl; ++s)
        if (find(s) != find(0))
            return "a local map node is not connected to local map node 0 (the Schur complement is singular)";
    std::vector<uint8_t> in(nl, 0);
    P.pairs.resize(2 * (size_t)n_pairs);
    for (int q = 0; q < n_pairs; ++q) {
        const int s = pairs[q].local_map_index, t = pairs[q].scan_index < 0 ? -1 : nl + pairs[q].scan_index;
        P.pairs[2 * q] = s;
        P.pairs[2 * q + 1] = t;
        in[s] = 1;
        if (t < 0)
            continue;
        if (G.node_ptr[t] == G.node_ptr[t + 1])
            return "a pair names a scan node without edges";
        for (int a = G.row_ptr[t]; a < G.row_ptr[t + 1]; ++a)
            if (G.row_col[a] != t)
                in[G.row_col[a]] = 1;
    }
    P.col_node.clear();
    P.col_of.assign(nl, -1);
    for (int s = 0; s < nl; ++s)
        if (in[s]) {
            P.col_of[s] = (int32_t)P.col_node.size();
            P.col_node.push_back(s);
        }
    return nullptr;
}

void pg_cov_record(const double* v, csm_pose_graph_marginal& m)
{
    std::memset(&m, 0, sizeof(m));
    std::memcpy(m.local_cov, v, 9 * sizeof(double));
    std::memcpy(m.scan_cov, v + 9, 9 * sizeof(double));
    std::memcpy(m.cross_cov, v + 18, 9 * sizeof(double));
    std::memcpy(m.relative_cov, v + 27, 9 * sizeof(double));
    m.finite = 1;
    for (int q = 0; q < 36; ++q)
        if (!std::isfinite(v[q]))
            m.finite = 0;
}

/* the marginals' launches behind the upload: H at lambda = 0 eliminated and factored by the LM step's
 * kernels (the state's done flag stays 0), then the columns of C and the pairs */
int pg_cov_chain(csm_ctx* ctx, const PgCovJob& C, const std::vector<int32_t>& col_node)
{
    const PgSchurJob& Q = C.Q;
    const PgJob& J = Q.J;
    const dim3 blk(kPgsBlock);
    const int n_scan = J.n_nodes - J.n_local, nt = Q.np / kPgsTile, ng = C.ldx / kPgsTile;
    int e = 0;
    if (J.n_edges)
        pg_launch(ctx, e, k_pgs_edges, pg_over(J.n_edges), blk, Q);
    pg_launch(ctx, e, k_pgs_assemble, pg_over((int64_t)J.n_nodes + J.n_cross), blk, Q);
    if (n_scan)
        pg_launch(ctx, e, k_pgs_eliminate, pg_over(n_scan), blk, Q);
    pg_launch(ctx, e, k_pgs_clear, pg_strided((int64_t)Q.np * Q.np), blk, Q);
    pg_launch(ctx, e, k_pgs_schur, pg_over(9 * (int64_t)Q.n_sblk + Q.np), blk, Q);
    {
        ScopedTimer tm(ctx, "pose_graph_marginals_factor");
        pg_ldl_launches(ctx, e, Q);
    }
    if (int rc = launched_ok(ctx, e, "pose-graph marginals factor"))
        return rc;
    ScopedTimer tm(ctx, "pose_graph_marginals_solve");
    pg_launch(ctx, e, k_pgc_init, pg_strided((int64_t)Q.np * C.ldx), blk, C);
    /* forward: the groups whose first unit row lies in panel p or above it (C ascends, so a prefix) */
    int live = 0;
    for (int p = 0; p < nt; ++p) {
        while (live < ng && 3 * col_node[(size_t)live * kPgcGroup] / kPgsTile <= p)
            ++live;
        if (!live)
            continue;
        pg_launch(ctx, e, k_pgc_diag<true>, dim3(live), blk, C, p);
        if (nt - p - 1)
            pg_launch(ctx, e, k_pgc_update<true>, dim3(nt - p - 1, live), blk, C, p);
    }
    pg_launch(ctx, e, k_pgc_scale, pg_strided((int64_t)Q.n_s * C.ldx), blk, C);
    for (int p = nt - 1; p >= 0; --p) {
        pg_launch(ctx, e, k_pgc_diag<false>, dim3(ng), blk, C, p);
        if (p)
            pg_launch(ctx, e, k_pgc_update<false>, dim3(p, ng), blk, C, p);
    }
    pg_launch(ctx, e, k_pgc_pairs, pg_over(C.n_pairs), blk, C);
    return launched_ok(ctx, e, "pose-graph marginals solve");
}

} /* namespace */

extern "C" {

int csm_host_pose_graph_loss(int32_t loss_type, double scale, double squared_error, double* loss, double* weight)
{
    if (loss_type < CSM_PG_LOSS_SQUARED || loss_type > CSM_PG_LOSS_WELSCH || !loss || !weight)
        return CSM_EINVAL;
    *loss = pg_loss(loss_type, scale, squared_error);
    *weight = pg_weight(loss_type, scale, squared_error);
    return CSM_OK;
}

int csm_host_pose_graph_lm(double* local_poses, int32_t n_local, double* scan_poses, int32_t n_scan,
                           const csm_pose_graph_edge* edges, int32_t n_edges, const csm_pose_graph_lm_params* params,
                           double* lambda, csm_pose_graph_lm_info* info, csm_pose_graph_lm_step* trace)
{
    if (pg_check(local_poses, n_local, scan_poses, n_scan, edges, n_edges, params, lambda))
        return CSM_EINVAL;
    PgGraph G;
    pg_build(n_local, n_scan, edges, n_edges, G);
    if (params->solver_type == CSM_PG_SOLVER_SCHUR_CHOLESKY && !pg_build_schur(G))
        return CSM_EINVAL;
    std::vector<double> pose(G.n_vars);
    std::memcpy(pose.data(), local_poses, 3 * (size_t)n_local * sizeof(double));
    if (n_scan)
        std::memcpy(pose.data() + 3 * (size_t)n_local, scan_poses, 3 * (size_t)n_scan * sizeof(double));
    pg_host_run(G, *params, pose, *lambda, info, trace);
    std::memcpy(local_poses, pose.data(), 3 * (size_t)n_local * sizeof(double));
    if (n_scan)
        std::memcpy(scan_poses, pose.data() + 3 * (size_t)n_local, 3 * (size_t)n_scan * sizeof(double));
    return CSM_OK;
}

int csm_pose_graph_lm(csm_ctx* ctx, double* local_poses, int32_t n_local, double* scan_poses, int32_t n_scan,
                      const csm_pose_graph_edge* edges, int32_t n_edges, const csm_pose_graph_lm_params* params,
                      double* lambda, csm_pose_graph_lm_info* info, csm_pose_graph_lm_step* trace)
{
    if (!ctx)
        return CSM_EINVAL;
    if (const char* why = pg_check(local_poses, n_local, scan_poses, n_scan, edges, n_edges, params, lambda))
        return fail(ctx, CSM_EINVAL, "csm_pose_graph_lm: %s", why);
    const bool schur = params->solver_type == CSM_PG_SOLVER_SCHUR_CHOLESKY;
    PgGraph G;
    pg_build(n_local, n_scan, edges, n_edges, G);
    if (schur && !pg_build_schur(G))
        return fail(ctx, CSM_EINVAL, "csm_pose_graph_lm: the Schur complement's contribution lists are too long");
    const bool small = 3 * n_local <= kPgsSmall;
    const int n = G.n_vars, n_out = 4 + 5 * params->iterations_max;
    PgSchurJob Q {};
    int rc;
    if ((rc = pg_device_job(ctx, G, local_poses, n_local, scan_poses, n_scan, params, lambda, schur, small, Q)))
        return rc;
    const PgJob& J = Q.J;
    if (!schur) {
        ScopedTimer tm(ctx, "pose_graph");
        if ((rc = launched_ok(ctx, launch(k_pose_graph_lm, dim3(1), dim3(kPgBlock), ctx->stream, J), "pose-graph LM")))
            return rc;
    } else {
        ScopedTimer tm(ctx, "pose_graph");
        if ((rc = pg_schur_chain(ctx, Q, small)))
            return rc;
    }
    std::vector<double> res(n + (size_t)n_out);
    HIP_TRY(ctx, hipMemcpyAsync(res.data(), J.pose, 8 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(res.data() + n, J.out, 8 * (size_t)n_out, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

    std::memcpy(local_poses, res.data(), 24 * (size_t)n_local);
    if (n_scan)
        std::memcpy(scan_poses, res.data() + 3 * (size_t)n_local, 24 * (size_t)n_scan);
    const double* o = res.data() + n;
    const int steps = (int)o[0];
    if (steps < 1 || steps > params->iterations_max)
        return fail(ctx, CSM_EIO, "csm_pose_graph_lm: the kernel reported %d steps", steps);
    *lambda = o[3];
    int64_t cg_total = 0;
    for (int s = 0; s < steps; ++s) {
        const double* t = o + 4 + 5 * s;
        cg_total += (int64_t)t[4];
        if (trace) {
            std::memset(&trace[s], 0, sizeof(trace[s]));
            trace[s].total_error = t[0];
            trace[s].lambda = t[1];
            trace[s].rhs_norm2 = t[2];
            trace[s].residual_norm2 = t[3];
            trace[s].cg_iterations = (int32_t)t[4];
        }
    }
    if (info) {
        std::memset(info, 0, sizeof(*info));
        info->steps = steps;
        info->cg_iterations = cg_total;
        info->initial_error = o[1];
        info->final_error = o[2];
        info->final_lambda = o[3];
    }
    return CSM_OK;
}

int csm_host_pose_graph_marginals(const double* local_poses, int32_t n_local, const double* scan_poses, int32_t n_scan,
                                  const csm_pose_graph_edge* edges, int32_t n_edges, int32_t loss_type,
                                  double loss_scale, const csm_pose_graph_pair* pairs, int32_t n_pairs,
                                  csm_pose_graph_marginal* out, csm_pose_graph_marginals_info* info)
{
    if (pg_cov_check(local_poses, n_local, scan_poses, n_scan, edges, n_edges, loss_type, loss_scale, pairs, n_pairs,
                     out))
        return CSM_EINVAL;
    PgGraph G;
    PgCovPlan P;
    pg_build(n_local, n_scan, edges, n_edges, G);
    if (!pg_build_schur(G) || pg_cov_plan(G, pairs, n_pairs, P))
        return CSM_EINVAL;
    const int n = G.n_vars, ns = 3 * n_local, nc = 3 * (int)P.col_node.size();
    std::vector<double> pose(n), ev((size_t)kPgEdgeVals * G.n_edges), bv(9 * ((size_t)G.n_nodes + G.n_cross));
    std::vector<double> b(n), invd(n), g(3 * (size_t)n_scan), w(9 * (size_t)G.n_cross), wrow(ns);
    std::vector<double> S((size_t)ns * ns), X((size_t)ns * nc, 0.0);
    std::memcpy(pose.data(), local_poses, 24 * (size_t)n_local);
    if (n_scan)
        std::memcpy(pose.data() + 3 * (size_t)n_local, scan_poses, 24 * (size_t)n_scan);
    PgJob J {};
    pg_job_structure(G, pg_cov_params(loss_type, loss_scale), 0.0, J);
    J.pose = pose.data();
    pg_host_lists(G, J);
    J.ev = ev.data();
    J.bv = bv.data();
    J.b = b.data();
    J.invd = invd.data();
    for (int e = 0; e < G.n_edges; ++e)
        pg_edge_values(&pose[3 * (size_t)G.enode[2 * e]], &pose[3 * (size_t)G.enode[2 * e + 1]], &G.rel[3 * (size_t)e],
                       &G.info[9 * (size_t)e], G.is_loop[e], loss_type, loss_scale, &ev[(size_t)kPgEdgeVals * e]);
    for (int k = 0; k < G.n_nodes; ++k)
        pg_assemble_node(J, k, 0.0);
    for (int u = 0; u < G.n_cross; ++u)
        pg_assemble_cross(J, u);
    for (int t = n_local; t < G.n_nodes; ++t)
        if (G.node_ptr[t] != G.node_ptr[t + 1])
            pg_eliminate_scan(J, g.data(), w.data(), t);
    pg_host_schur_matrix(G, J, w.data(), S);
    pg_host_ldl(S, ns, wrow);
    /* every column by itself; row k's terms reach the columns whose unit row is k or above it (a prefix) */
    std::vector<int32_t> reach(ns, 0);
    for (int c = 0; c < nc; ++c) {
        const int f = 3 * P.col_node[c / 3] + c % 3;
        X[(size_t)f * nc + c] = 1.0;
        ++reach[f];
    }
    for (int k = 1; k < ns; ++k)
        reach[k] += reach[k - 1];
    for (int i = 0; i < ns; ++i) {
        double* xi = &X[(size_t)i * nc];
        for (int k = 0; k < i; ++k) {
            const double l = S[(size_t)i * ns + k];
            const double* xk = &X[(size_t)k * nc];
            for (int c = 0; c < reach[k]; ++c)
                xi[c] -= l * xk[c];
        }
    }
    for (int i = 0; i < ns; ++i)
        for (int c = 0; c < nc; ++c)
            X[(size_t)i * nc + c] = X[(size_t)i * nc + c] / S[(size_t)i * ns + i];
    for (int i = ns - 1; i >= 0; --i) {
        double* xi = &X[(size_t)i * nc];
        for (int k = ns - 1; k > i; --k) {
            const double l = S[(size_t)k * ns + i];
            const double* xk = &X[(size_t)k * nc];
            for (int c = 0; c < nc; ++c)
                xi[c] -= l * xk[c];
        }
    }
    for (int q = 0; q < n_pairs; ++q) {
        double v[36];
        pg_marginal_pair(J, w.data(), X.data(), (size_t)nc, P.col_of.data(), P.pairs[2 * q], P.pairs[2 * q + 1], v);
        pg_cov_record(v, out[q]);
    }
    if (info) {
        std::memset(info, 0, sizeof(*info));
        info->n_columns = (int32_t)P.col_node.size();
    }
    return CSM_OK;
}

int csm_pose_graph_marginals(csm_ctx* ctx, const double* local_poses, int32_t n_local, const double* scan_poses,
                             int32_t n_scan, const csm_pose_graph_edge* edges, int32_t n_edges, int32_t loss_type,
                             double loss_scale, const csm_pose_graph_pair* pairs, int32_t n_pairs,
                             csm_pose_graph_marginal* out, csm_pose_graph_marginals_info* info)
{
    if (!ctx)
        return CSM_EINVAL;
    if (const char* why = pg_cov_check(local_poses, n_local, scan_poses, n_scan, edges, n_edges, loss_type, loss_scale,
                                       pairs, n_pairs, out))
        return fail(ctx, CSM_EINVAL, "csm_pose_graph_marginals: %s", why);
    PgGraph G;
    PgCovPlan P;
    pg_build(n_local, n_scan, edges, n_edges, G);
    if (!pg_build_schur(G))
        return fail(ctx, CSM_EINVAL, "csm_pose_graph_marginals: the Schur complement's contribution lists are too long");
    if (const char* why = pg_cov_plan(G, pairs, n_pairs, P))
        return fail(ctx, CSM_EINVAL, "csm_pose_graph_marginals: %s", why);
    const csm_pose_graph_lm_params prm = pg_cov_params(loss_type, loss_scale);
    const double lambda = 0.0;
    PgCovJob C {};
    int rc;
    if ((rc = pg_device_job(ctx, G, local_poses, n_local, scan_poses, n_scan, &prm, &lambda, true, false, C.Q)))
        return rc;
    const int n_c = (int)P.col_node.size();
    C.n_cols = 3 * n_c;
    C.ldx = ceil_div(n_c, kPgcGroup) * kPgsTile;
    C.n_pairs = n_pairs;
    /* X, then the uploaded lists, then the records */
    Carve c;
    const size_t o_x = c.take(8 * (size_t)C.Q.np * C.ldx), o_node = c.take(4 * (size_t)n_c),
                 o_of = c.take(4 * (size_t)n_local), o_pairs = c.take(8 * (size_t)n_pairs), o_lists = c.off,
                 o_out = c.take(8 * 36 * (size_t)n_pairs);
    if ((rc = grow(ctx, ctx->pg_cov, c.off, c.off, false)))
        return rc;
    std::vector<uint8_t>& st = ctx->pg_cov_stage;
    st.assign(o_lists - o_node, 0);
    std::memcpy(st.data(), P.col_node.data(), 4 * (size_t)n_c);
    std::memcpy(st.data() + (o_of - o_node), P.col_of.data(), 4 * (size_t)n_local);
    std::memcpy(st.data() + (o_pairs - o_node), P.pairs.data(), 8 * (size_t)n_pairs);
    uint8_t* d = reinterpret_cast<uint8_t*>(ctx->pg_cov.p);
    C.X = reinterpret_cast<double*>(d + o_x);
    C.col_node = reinterpret_cast<const int32_t*>(d + o_node);
    C.col_of = reinterpret_cast<const int32_t*>(d + o_of);
    C.pairs = reinterpret_cast<const int32_t*>(d + o_pairs);
    C.out = reinterpret_cast<double*>(d + o_out);
    HIP_TRY(ctx, hipMemcpyAsync(d + o_node, st.data(), st.size(), hipMemcpyHostToDevice, ctx->stream));
    {
        ScopedTimer tm(ctx, "pose_graph_marginals");
        if ((rc = pg_cov_chain(ctx, C, P.col_node)))
            return rc;
    }
    std::vector<double> res(36 * (size_t)n_pairs);
    HIP_TRY(ctx, hipMemcpyAsync(res.data(), C.out, 8 * res.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int q = 0; q < n_pairs; ++q)
        pg_cov_record(&res[36 * (size_t)q], out[q]);
    if (info) {
        std::memset(info, 0, sizeof(*info));
        info->n_columns = n_c;
    }
    return CSM_OK;
}

int csm_host_loop_search_ranges(const double relative_cov[9], double n_sigma, const double min_range[3],
                                const double max_range[3], double out_range[3])
{
    if (!relative_cov || !min_range || !max_range || !out_range || !std::isfinite(n_sigma) || n_sigma < 0.0)
        return CSM_EINVAL;
    for (int a = 0; a < 3; ++a) {
        const double d = relative_cov[4 * a];
        if (!std::isfinite(d) || d < 0.0 || std::isnan(min_range[a]) || std::isnan(max_range[a]) ||
            min_range[a] > max_range[a])
            return CSM_EINVAL;
    }
    for (int a = 0; a < 3; ++a) {
        double r = (2.0 * n_sigma) * sqrt(relative_cov[4 * a]);
        if (r < min_range[a])
            r = min_range[a];
        if (r > max_range[a])
            r = max_range[a];
        out_range[a] = r;
    }
    return CSM_OK;
}

int csm_host_loop_gate(const double relative_cov[9], const double match_cov[9], const double predicted[3],
                       const double measured[3], double* chi2)
{
    if (!relative_cov || !match_cov || !predicted || !measured || !chi2)
        return CSM_EINVAL;
    double M[9], f[6], x[3];
    for (int q = 0; q < 9; ++q)
        M[q] = relative_cov[q] + match_cov[q];
    pg_ldl3(M, f);
    for (int a = 0; a < 3; ++a)
        if (!(f[a] > 0.0) || !std::isfinite(f[a]))
            return CSM_EINVAL;
    const double d[3] = { measured[0] - predicted[0], measured[1] - predicted[1],
                          pg_normalize_angle(measured[2] - predicted[2]) };
    pg_ldl3_solve(f, d[0], d[1], d[2], x);
    *chi2 = d[0] * x[0] + d[1] * x[1] + d[2] * x[2];
    return CSM_OK;
}

int csm_host_information_from_covariance(const double cov[9], double out[9])
{
    if (!cov || !out)
        return CSM_EINVAL;
    double f[6];
    pg_ldl3(cov, f);
    for (int a = 0; a < 3; ++a)
        if (!(f[a] > 0.0) || !std::isfinite(f[a]))
            return CSM_EINVAL;
    for (int j = 0; j < 3; ++j) {
        double x[3];
        pg_ldl3_solve(f, j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0, x);
        for (int i = j; i < 3; ++i) {
            out[3 * i + j] = x[i];
            out[3 * j + i] = x[i];
        }
    }
    return CSM_OK;
}

} /* extern "C" */
