"""An independent Python restatement of PoseGraphOptimizerLM::Optimize with the direct
Schur-complement Cholesky solver (CSM_PG_SOLVER_SCHUR_CHOLESKY), in scalar float
arithmetic. The linearisation, the loss functions, `_sum` and the total error are those of
tests/pose_graph_literal.py (the ConjugateGradient restatement); this file adds the solve.

H is taken from `_linearize` as dense self-adjoint rows, so the 3x3 blocks are cut out of a matrix
here, not out of the library's block lists. Per LM step, in the order the library fixes:
  1. every scan node t: D_t = L D L^T (3x3, unpivoted, from the lower triangle), g_t = D_t^-1 b_t,
     W_ts = D_t^-1 B_ts for every stored cross block (three solves);
  2. S_(s1,s2), s1 >= s2: A_s1 [s1 = s2] - sum_t B_(t,s1)^T W_(t,s2), ascending t, every 3-term
     product left to right, subtracted one after the other; c_s = b_s - sum_t B_(t,s)^T g_t;
  3. scalar unpivoted LDL^T of S (lower triangle): S_ij - sum_{k<j} (L_ik d_k) L_jk, k ascending;
     forward substitution (k ascending), division by d, backward substitution (k descending);
  4. x_t = g_t - sum_s W_ts x_s, ascending s;
  5. residual_norm2 = |b - H delta|^2 with (H delta)_i as the conjugate-gradient restatement's
     product (ascending columns from 0.0), summed left to right.
`pairwise=True` runs the sums of steps 2 - 5 and the total error as "first value minus the
pairwise-tree sum of the terms" instead of one subtraction after the other: the spread between
the two orders sizes the device tolerances (tests/test_gpu_pose_graph_schur.py).
"""
from pose_graph_literal import DBL_MAX, _linearize, _rows, _sum, total_error


def _ldl3(D):
    d0 = D[0][0]
    l10 = D[1][0] / d0
    l20 = D[2][0] / d0
    d1 = D[1][1] - (l10 * d0) * l10
    l21 = (D[2][1] - (l20 * d0) * l10) / d1
    d2 = D[2][2] - (l20 * d0) * l20 - (l21 * d1) * l21
    return d0, d1, d2, l10, l20, l21


def _solve3(f, v):
    d0, d1, d2, l10, l20, l21 = f
    y1 = v[1] - l10 * v[0]
    y2 = v[2] - l20 * v[0] - l21 * y1
    z0, z1, z2 = v[0] / d0, y1 / d1, y2 / d2
    x2 = z2
    x1 = z1 - l21 * x2
    x0 = z0 - l20 * x2 - l10 * x1
    return [x0, x1, x2]


def _minus(first, terms, pairwise):
    """first - t0 - t1 - ..., or first - (pairwise sum of the terms)"""
    if pairwise:
        return first - _sum(terms, True) if terms else first
    for t in terms:
        first -= t
    return first


def solve(rows, b, nl, n_nodes, pairwise=False):
    """One direct solve of H delta = b. rows: the dense self-adjoint rows of `_linearize`."""
    Hd = [dict(rw) for rw in rows]

    def blk(r, c):
        """the stored 3x3 block (node r, node c), or None"""
        if not any((3 * c + j) in Hd[3 * r + i] for i in range(3) for j in range(3)):
            return None
        return [[Hd[3 * r + i].get(3 * c + j, 0.0) for j in range(3)] for i in range(3)]

    # the cross blocks exist per distinct (scan node, local map node) pair that has an edge; an entry
    # that sums to 0.0 is still stored, so adjacency comes from the keys, not from the values
    adj = {t: [s for s in range(nl) if blk(t, s) is not None] for t in range(nl, n_nodes)}
    B = {(t, s): blk(t, s) for t in adj for s in adj[t]}
    g, W = {}, {}
    for t in range(nl, n_nodes):
        f = _ldl3(blk(t, t))
        g[t] = _solve3(f, b[3 * t:3 * t + 3])
        for s in adj[t]:
            cols = [_solve3(f, [B[(t, s)][k][j] for k in range(3)]) for j in range(3)]
            W[(t, s)] = [[cols[j][k] for j in range(3)] for k in range(3)]
    ns = 3 * nl
    S = [[0.0] * ns for _ in range(ns)]
    c = [0.0] * ns
    of = [[t for t in range(nl, n_nodes) if s in adj[t]] for s in range(nl)]
    for s1 in range(nl):
        for s2 in range(s1 + 1):
            common = [t for t in of[s1] if s2 in adj[t]]
            if s1 != s2 and not common:
                continue
            A = blk(s1, s1) if s1 == s2 else None
            for i in range(3):
                for j in range(3):
                    terms = [B[(t, s1)][0][i] * W[(t, s2)][0][j] + B[(t, s1)][1][i] * W[(t, s2)][1][j] +
                             B[(t, s1)][2][i] * W[(t, s2)][2][j] for t in common]
                    S[3 * s1 + i][3 * s2 + j] = _minus(A[i][j] if A else 0.0, terms, pairwise)
        for a in range(3):
            terms = [B[(t, s1)][0][a] * g[t][0] + B[(t, s1)][1][a] * g[t][1] + B[(t, s1)][2][a] * g[t][2]
                     for t in of[s1]]
            c[3 * s1 + a] = _minus(b[3 * s1 + a], terms, pairwise)
    # LDL^T in place: L below the diagonal, d on it
    for i in range(ns):
        w = [0.0] * i
        for j in range(i + 1):
            v = _minus(S[i][j], [w[k] * S[j][k] for k in range(j)], pairwise)
            if j < i:
                S[i][j] = v / S[j][j]
                w[j] = S[i][j] * S[j][j]
            else:
                S[i][i] = v
    x = list(c) + [0.0] * (3 * n_nodes - ns)
    for i in range(ns):
        x[i] = _minus(x[i], [S[i][k] * x[k] for k in range(i)], pairwise)
    for i in range(ns):
        x[i] = x[i] / S[i][i]
    for i in range(ns - 1, -1, -1):
        x[i] = _minus(x[i], [S[k][i] * x[k] for k in range(ns - 1, i, -1)], pairwise)
    for t in range(nl, n_nodes):
        for i in range(3):
            terms = [W[(t, s)][i][0] * x[3 * s] + W[(t, s)][i][1] * x[3 * s + 1] + W[(t, s)][i][2] * x[3 * s + 2]
                     for s in adj[t]]
            x[3 * t + i] = _minus(g[t][i], terms, pairwise)
    return x


def residual_norm2(rows, b, x, pairwise=False):
    sq = []
    for i, rw in enumerate(rows):
        acc = 0.0
        for col, h in rw:
            acc += h * x[col]
        r = b[i] - acc
        sq.append(r * r)
    return _sum(sq, pairwise)


def optimize(local, scan, edges, lam, iterations_max=10, error_tolerance=1e-4, loss_kind="Huber",
             loss_scale=0.01, pairwise=False):
    """As pose_graph_literal.optimize: returns (local, scan, lambda, trace, initial_error) with
    trace = [(total, lambda, |b|^2, |b - H delta|^2, 0)]."""
    nl = len(local)
    nodes = [[float(v) for v in p] for p in local] + [[float(v) for v in p] for p in scan]
    n = 3 * len(nodes)
    E = []
    for d in edges:
        E.append((int(d["local"]), nl + int(d["scan"]), [float(v) for v in d["rel"]], _rows(d["info"]),
                  bool(d.get("loop"))))
    prev = DBL_MAX
    initial = total_error(nodes, E, loss_kind, loss_scale, pairwise)
    trace = []
    while True:
        rows, _, b = _linearize(nodes, E, lam, n, loss_kind, loss_scale)
        x = solve(rows, b, nl, len(nodes), pairwise)
        rhs2 = _sum([v * v for v in b], pairwise)
        r2 = residual_norm2(rows, b, x, pairwise)
        for k in range(len(nodes)):
            for j in range(3):
                nodes[k][j] += x[3 * k + j]
        total = total_error(nodes, E, loss_kind, loss_scale, pairwise)
        trace.append((total, lam, rhs2, r2, 0))
        if len(trace) >= iterations_max or abs(prev - total) < error_tolerance:
            break
        lam = lam * 0.5 if total < prev else lam * 2.0
        prev = total
    return nodes[:nl], nodes[nl:], lam, trace, initial
