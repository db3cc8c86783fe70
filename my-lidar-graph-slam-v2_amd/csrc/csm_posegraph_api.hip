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

#include <optional>
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

/* local_poses, then scan_poses: the node poses as one vector, and back into the caller's two arrays */
std::vector<double> pg_join_poses(const double* local_poses, int n_local, const double* scan_poses, int n_scan)
{
    std::vector<double> pose(3 * ((size_t)n_local + n_scan));
    std::memcpy(pose.data(), local_poses, 24 * (size_t)n_local);
    if (n_scan)
        std::memcpy(pose.data() + 3 * (size_t)n_local, scan_poses, 24 * (size_t)n_scan);
    return pose;
}

void pg_split_poses(const double* pose, double* local_poses, int n_local, double* scan_poses, int n_scan)
{
    std::memcpy(local_poses, pose, 24 * (size_t)n_local);
    if (n_scan)
        std::memcpy(scan_poses, pose + 3 * (size_t)n_local, 24 * (size_t)n_scan);
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

/* The work set of the host restatements: the vectors of one linearization (and of the direct solver), and a job
 * bound to them and to the graph's own lists. */
struct PgHostWork {
    const PgGraph& G;
    PgJob J {};
    std::vector<double> pose, ev, bv, b, invd, x;
    std::vector<double> S, g, w, wrow;            /* the direct solver's: dense S (3 n_local square), g, W, a row of L d */

    PgHostWork(const PgGraph& graph, const csm_pose_graph_lm_params& p, double lambda, std::vector<double> poses)
        : G(graph), pose(std::move(poses)), ev((size_t)kPgEdgeVals * G.n_edges),
          bv(9 * ((size_t)G.n_nodes + G.n_cross)), b(G.n_vars), invd(G.n_vars), x(G.n_vars)
    {
        if (p.solver_type == CSM_PG_SOLVER_SCHUR_CHOLESKY) {
            const size_t ns = 3 * (size_t)G.n_local;
            S.resize(ns * ns);
            g.resize(3 * (size_t)(G.n_nodes - G.n_local));
            w.resize(9 * (size_t)G.n_cross);
            wrow.resize(ns);
        }
        pg_job_structure(G, p, lambda, J);
        J.pose = pose.data();
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
        J.ev = ev.data();
        J.bv = bv.data();
        J.b = b.data();
        J.invd = invd.data();
        J.x = x.data();
    }

    /* H and b at the current poses: per-edge values, the nodes' blocks, the cross blocks */
    void linearize(double lambda)
    {
        for (int e = 0; e < G.n_edges; ++e)
            pg_edge_values_at(J, e);
        for (int k = 0; k < G.n_nodes; ++k)
            pg_assemble_node(J, k, lambda);
        for (int u = 0; u < G.n_cross; ++u)
            pg_assemble_cross(J, u);
    }

    /* steps 1 - 3: the scan nodes eliminated, S put together and factored in place. The LM step eliminates
     * every scan node: with lambda on its diagonal a node without edges has D_t = lambda I, and the back
     * substitution reads its g_t = 0. The marginals linearize at lambda = 0, where that D_t is 0 and its
     * factor 0 / 0; nothing there reads g_t (pg_cov_plan refuses a pair that names such a node), so they
     * pass edgeless = false and skip it. */
    void factor_schur(bool edgeless)
    {
        for (int t = G.n_local; t < G.n_nodes; ++t)
            if (edgeless || G.node_ptr[t] != G.node_ptr[t + 1])
                pg_eliminate_scan(J, g.data(), w.data(), t);
        pg_host_schur_matrix(G, J, w.data(), S);
        pg_host_ldl(S, 3 * G.n_local, wrow);
    }
};

/* info zeroed, when the caller wants one */
template <class T>
T* pg_cleared(T* info)
{
    if (info)
        std::memset(info, 0, sizeof(*info));
    return info;
}

/* PgJob::out, as the kernels and pg_host_run write it, into the caller's lambda, info and trace. False, and
 * nothing written, when its step count is not in 1 .. iterations_max. */
bool pg_report(const double* out, int iterations_max, double* lambda, csm_pose_graph_lm_info* info,
               csm_pose_graph_lm_step* trace)
{
    const int steps = (int)out[0];
    if (steps < 1 || steps > iterations_max)
        return false;
    *lambda = out[3];
    int64_t cg_total = 0;
    for (int s = 0; s < steps; ++s) {
        const double* t = out + 4 + 5 * (size_t)s;
        cg_total += (int64_t)t[4];                /* a count: exact in a double */
        if (trace) {
            std::memset(&trace[s], 0, sizeof(trace[s]));
            trace[s].total_error = t[0];
            trace[s].lambda = t[1];
            trace[s].rhs_norm2 = t[2];
            trace[s].residual_norm2 = t[3];
            trace[s].cg_iterations = (int32_t)t[4];
        }
    }
    if (pg_cleared(info)) {
        info->steps = steps;
        info->cg_iterations = cg_total;
        info->initial_error = out[1];
        info->final_error = out[2];
        info->final_lambda = out[3];
    }
    return true;
}

/* Optimize, statement by statement and in sequence: the reference the device is held to. Leaves the poses in
 * W.pose and the report in out, laid out as PgJob::out. */
void pg_host_run(PgHostWork& W, const csm_pose_graph_lm_params& p, double lambda, double* out)
{
    const PgGraph& G = W.G;
    const PgJob& J = W.J;
    const int n = G.n_vars, ns = 3 * G.n_local;
    const bool schur = p.solver_type == CSM_PG_SOLVER_SCHUR_CHOLESKY;
    std::vector<double>&pose = W.pose, &b = W.b, &invd = W.invd, &x = W.x, &S = W.S;
    std::vector<double> r(n), z(n), pv(n), ap(n);
    auto total_error = [&]() {
        double t = 0.0;
        for (int e = 0; e < G.n_edges; ++e)
            t += pg_edge_loss_at(J, e);
        return t;
    };
    auto dot = [n](const std::vector<double>& a, const std::vector<double>& c) {
        double s = 0.0;
        for (int i = 0; i < n; ++i)
            s += a[i] * c[i];
        return s;
    };
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
    auto solve_schur = [&]() {
        W.factor_schur(true);
        for (int a = 0; a < ns; ++a)
            x[a] = pg_schur_rhs(J, W.g.data(), a / 3, a % 3);
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
            pg_back_scan(J, W.g.data(), W.w.data(), x.data(), t);
        double r2 = 0.0;
        for (int i = 0; i < n; ++i) {
            const double ri = b[i] - pg_row_times(J, i, x.data());
            r2 += ri * ri;
        }
        return r2;
    };
    double prev = DBL_MAX, total = DBL_MAX;
    out[1] = total_error();
    int steps = 0;
    for (;;) {
        W.linearize(lambda);
        const double rhs2 = dot(b, b);
        int cg = 0;
        const double r2 = schur ? solve_schur() : solve_cg(rhs2, cg);
        for (int i = 0; i < n; ++i)
            pose[i] += x[i];
        total = total_error();
        double* o = out + 4 + 5 * (size_t)steps;
        o[0] = total;
        o[1] = lambda;
        o[2] = rhs2;
        o[3] = r2;
        o[4] = (double)cg;
        if (++steps >= p.iterations_max || std::fabs(prev - total) < p.error_tolerance)
            break;
        lambda = (total < prev) ? lambda * 0.5 : lambda * 2.0;
        prev = total;
    }
    out[0] = (double)steps;
    out[2] = total;
    out[3] = lambda;
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

/* the head of a step's chain (steps 0 and 1): the per-edge values, the blocks of H with b, the scan nodes eliminated */
void pg_linearize_launches(csm_ctx* ctx, int& e, const PgSchurJob& Q)
{
    const PgJob& J = Q.J;
    const dim3 blk(kPgsBlock);
    if (J.n_edges)
        pg_launch(ctx, e, k_pgs_edges, pg_over(J.n_edges), blk, Q);
    pg_launch(ctx, e, k_pgs_assemble, pg_over((int64_t)J.n_nodes + J.n_cross), blk, Q);
    if (J.n_nodes - J.n_local)
        pg_launch(ctx, e, k_pgs_eliminate, pg_over(J.n_nodes - J.n_local), blk, Q);
}

/* the blocked path's steps 2 and 3: S and c from the ordered lists, then the LDL^T of S in place, per panel its
 * diagonal tile, the panel below it and the trailing update. ldl_timer: a timer around the LDL^T alone. */
void pg_factor_launches(csm_ctx* ctx, int& e, const PgSchurJob& Q, const char* ldl_timer = nullptr)
{
    const dim3 blk(kPgsBlock);
    pg_launch(ctx, e, k_pgs_clear, pg_strided((int64_t)Q.np * Q.np), blk, Q);
    pg_launch(ctx, e, k_pgs_schur, pg_over(9 * (int64_t)Q.n_sblk + Q.np), blk, Q);
    std::optional<ScopedTimer> tm;
    if (ldl_timer)
        tm.emplace(ctx, ldl_timer);
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
        pg_linearize_launches(ctx, e, Q);
        if (small) {
            pg_launch(ctx, e, k_pgs_small, dim3(1), blk, Q);
        } else {
            pg_factor_launches(ctx, e, Q);
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

/* The layout table of one device buffer: add() carves the next piece (Carve's 256-byte alignment) and notes the
 * pointer that will name it and, for an uploaded piece, its host source, so an array is stated once. `c.off`
 * is the size so far. The noted pointers and sources must outlive upload(). */
struct PgLayout {
    struct Piece {
        void* dst;
        void (*set)(void* dst, uint8_t* at);
        size_t off, bytes;
        const void* src;
    };
    Carve c;
    std::vector<Piece> pieces;

    template <class T>
    void add(T*& dst, size_t bytes, const void* src = nullptr)
    {
        pieces.push_back({ &dst, [](void* d, uint8_t* at) { *static_cast<T**>(d) = reinterpret_cast<T*>(at); },
                           c.take(bytes), bytes, src });
    }

    /* one pass once `buf` holds c.off bytes: every pointer set, the sources within bytes [from, to) copied
     * into the stage (zeros between them); then that range uploaded in one copy on the ctx stream */
    int upload(csm_ctx* ctx, const DevBuf& buf, std::vector<uint8_t>& stage, size_t from, size_t to) const
    {
        uint8_t* d = buf.as<uint8_t>();
        stage.assign(to - from, 0);
        for (const Piece& p : pieces) {
            p.set(p.dst, d + p.off);
            if (p.src && p.bytes)
                std::memcpy(stage.data() + (p.off - from), p.src, p.bytes);
        }
        HIP_TRY(ctx, hipMemcpyAsync(d + from, stage.data(), stage.size(), hipMemcpyHostToDevice, ctx->stream));
        return CSM_OK;
    }
};

/* one device call's set-up: the graph, its lists and the LM state staged and uploaded into pg_buf (on the
 * ctx stream), the work vectors carved behind them, pg_s grown for the blocked direct solver; Q.J alone
 * serves the conjugate-gradient kernel */
int pg_device_job(csm_ctx* ctx, const PgGraph& G, const double* local_poses, int n_local, const double* scan_poses,
                  int n_scan, const csm_pose_graph_lm_params* params, const double* lambda, bool schur, bool small,
                  PgSchurJob& Q)
{
    const size_t n = G.n_vars, E = G.n_edges, N = G.n_nodes, U = G.n_cross, R = G.row_col.size(), B = G.n_sblk;
    PgJob& J = Q.J;
    pg_job_structure(G, *params, *lambda, J);
    Q.n_s = 3 * n_local;
    Q.np = pg_schur_padded(n_local);
    Q.n_sblk = G.n_sblk;
    Q.nb_vars = ceil_div(G.n_vars, kPgsBlock);
    Q.nb_edges = ceil_div(G.n_edges, kPgsBlock);
    const size_t np = Q.np;
    const std::vector<double> pose = pg_join_poses(local_poses, n_local, scan_poses, n_scan);
    const PgState st0 = { *lambda, DBL_MAX, DBL_MAX, 0.0, 0, 0 };
    PgLayout lay;
    /* inputs (uploaded): pose, rel, info, the int lists, then the direct solver's lists and its LM state */
    lay.add(J.pose, 8 * n, pose.data());
    lay.add(J.rel, 24 * E, G.rel.data());
    lay.add(J.info, 72 * E, G.info.data());
    lay.add(J.enode, 8 * E, G.enode.data());
    lay.add(J.is_loop, 4 * E, G.is_loop.data());
    lay.add(J.node_ptr, 4 * (N + 1), G.node_ptr.data());
    lay.add(J.node_edges, 8 * E, G.node_edges.data());
    lay.add(J.cross_ptr, 4 * (U + 1), G.cross_ptr.data());
    lay.add(J.cross_edges, 4 * E, G.cross_edges.data());
    lay.add(J.row_ptr, 4 * (N + 1), G.row_ptr.data());
    lay.add(J.row_col, 4 * R, G.row_col.data());
    lay.add(J.row_ent, 4 * R, G.row_ent.data());
    lay.add(Q.sb_rc, schur ? 8 * B : 0, G.sb_rc.data());
    lay.add(Q.sb_ptr, schur ? 4 * (B + 1) : 0, G.sb_ptr.data());
    lay.add(Q.sb_pair, schur ? 4 * G.sb_pair.size() : 0, G.sb_pair.data());
    lay.add(Q.st, schur ? sizeof(PgState) : 0, &st0);
    const size_t up_bytes = lay.c.off;
    /* work and output */
    lay.add(J.ev, 8 * (size_t)kPgEdgeVals * E);
    lay.add(J.bv, 72 * (N + U));
    for (double** v : { &J.b, &J.invd, &J.x, &J.r, &J.z, &J.p, &J.ap })
        lay.add(*v, 8 * n);
    lay.add(J.out, 8 * (4 + 5 * (size_t)params->iterations_max));
    lay.add(Q.g, schur ? 24 * (size_t)n_scan : 0);
    lay.add(Q.w, schur ? 72 * U : 0);
    lay.add(Q.y, schur ? 8 * np : 0);
    lay.add(Q.wp, schur && !small ? 8 * np * kPgsTile : 0);
    lay.add(Q.part, schur ? 8 * (2 * (size_t)Q.nb_vars + Q.nb_edges) : 0);
    int rc;
    if ((rc = ensure(ctx, ctx->pg_buf, lay.c.off)))
        return rc;
    if (schur && !small && (rc = grow(ctx, ctx->pg_s, 8 * np * np, 8 * np * np, false)))
        return rc;
    Q.S = schur && !small ? ctx->pg_s.as<double>() : nullptr;
    return lay.upload(ctx, ctx->pg_buf, ctx->pg_stage, 0, up_bytes);
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
    const dim3 blk(kPgsBlock);
    const int nt = Q.np / kPgsTile, ng = C.ldx / kPgsTile;
    int e = 0;
    pg_linearize_launches(ctx, e, Q);
    pg_factor_launches(ctx, e, Q, "pose_graph_marginals_factor");
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

/* the LDL^T of a 3x3 (pg_ldl3) into f; false when a pivot is not positive and finite */
bool pg_ldl3_positive(const double* M, double f[6])
{
    pg_ldl3(M, f);
    for (int a = 0; a < 3; ++a)
        if (!(f[a] > 0.0) || !std::isfinite(f[a]))
            return false;
    return true;
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
    PgHostWork W(G, *params, *lambda, pg_join_poses(local_poses, n_local, scan_poses, n_scan));
    std::vector<double> out(4 + 5 * (size_t)params->iterations_max);
    pg_host_run(W, *params, *lambda, out.data());
    pg_split_poses(W.pose.data(), local_poses, n_local, scan_poses, n_scan);
    pg_report(out.data(), params->iterations_max, lambda, info, trace);
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
    {
        ScopedTimer tm(ctx, "pose_graph");
        rc = schur ? pg_schur_chain(ctx, Q, small)
                   : launched_ok(ctx, launch(k_pose_graph_lm, dim3(1), dim3(kPgBlock), ctx->stream, J), "pose-graph LM");
        if (rc)
            return rc;
    }
    std::vector<double> res(n + (size_t)n_out);
    HIP_TRY(ctx, hipMemcpyAsync(res.data(), J.pose, 8 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(res.data() + n, J.out, 8 * (size_t)n_out, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    pg_split_poses(res.data(), local_poses, n_local, scan_poses, n_scan);
    if (!pg_report(res.data() + n, params->iterations_max, lambda, info, trace))
        return fail(ctx, CSM_EIO, "csm_pose_graph_lm: the kernel reported %d steps", (int)res[n]);
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
    const int ns = 3 * n_local, nc = 3 * (int)P.col_node.size();
    PgHostWork W(G, pg_cov_params(loss_type, loss_scale), 0.0, pg_join_poses(local_poses, n_local, scan_poses, n_scan));
    W.linearize(0.0);
    W.factor_schur(false);
    const std::vector<double>& S = W.S;
    std::vector<double> X((size_t)ns * nc, 0.0);
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
        pg_marginal_pair(W.J, W.w.data(), X.data(), (size_t)nc, P.col_of.data(), P.pairs[2 * q], P.pairs[2 * q + 1], v);
        pg_cov_record(v, out[q]);
    }
    if (pg_cleared(info))
        info->n_columns = (int32_t)P.col_node.size();
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
    PgLayout lay;
    lay.add(C.X, 8 * (size_t)C.Q.np * C.ldx);
    const size_t o_lists = lay.c.off;
    lay.add(C.col_node, 4 * (size_t)n_c, P.col_node.data());
    lay.add(C.col_of, 4 * (size_t)n_local, P.col_of.data());
    lay.add(C.pairs, 8 * (size_t)n_pairs, P.pairs.data());
    const size_t o_out = lay.c.off;
    lay.add(C.out, 8 * 36 * (size_t)n_pairs);
    if ((rc = grow(ctx, ctx->pg_cov, lay.c.off, lay.c.off, false)) ||
        (rc = lay.upload(ctx, ctx->pg_cov, ctx->pg_cov_stage, o_lists, o_out)))
        return rc;
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
    if (pg_cleared(info))
        info->n_columns = n_c;
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
    if (!pg_ldl3_positive(M, f))
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
    if (!pg_ldl3_positive(cov, f))
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
