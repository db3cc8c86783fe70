"""An independent Python restatement of the pose-graph marginals (csm_pose_graph_marginals, DESIGN.md 4e
"marginals"), in scalar float arithmetic. It runs on the dense self-adjoint rows of
pose_graph_literal._linearize(..., lam=0.0, ...), so the 3x3 blocks are cut out of a matrix, not out of
the library's block lists; the elimination of the scan nodes and the LDL^T of S are those of
pose_graph_schur_literal.solve, stated again here because that function keeps them to itself.

In the order the library fixes, with H = [A B^T; B D], W_ts = D_t^-1 B_ts and X = S^-1:
  columns   C = {s of every pair} u adj(t of every pair), ascending; column 3 m + j of X is solved from
            the unit vector of row 3 C[m] + j, by itself: y_i = e_i - sum_{k<i} L_ik y_k (k ascending,
            from the unit row on), z = y / d on every row, x_i = z_i - sum_{k>i} L_ki x_k (k descending).
            X[r, c] is always row r of the solved column c.
  Sigma_ss  X[s, s], entries i >= j mirrored
  Sigma_st  0.0 - sum_{s' in adj(t)} X[s, s'] W_ts'^T, ascending s', subtracted one after the other
  Sigma_tt  D_t^-1 (3x3 LDL^T, solved from the unit vectors) + sum_{s'} sum_{s''} (W_ts' X[s', s'']) W_ts''^T,
            entries i >= j mirrored
  relative  (Js Sigma_ss) Js^T + (Js Sigma_st) Je^T + (Je Sigma_st^T) Js^T + (Je Sigma_tt) Je^T, left to
            right, entries i >= j mirrored; Js, Je as in _linearize
Every 3-term product is summed left to right.
"""
from pose_graph_literal import _error, _linearize, _rows
from pose_graph_schur_literal import _ldl3, _solve3


def _mul(A, B, i, j):
    return A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j]


def _mult(A, B, i, j):
    """(A B^T)(i, j)"""
    return A[i][0] * B[j][0] + A[i][1] * B[j][1] + A[i][2] * B[j][2]


def marginals(local, scan, edges, pairs, loss_kind="Huber", loss_scale=0.01):
    """pairs: (local map index, scan index or None). Returns one dict per pair with local_cov, scan_cov,
    cross_cov, relative_cov as 3x3 lists of floats."""
    nl = len(local)
    nodes = [[float(v) for v in p] for p in local] + [[float(v) for v in p] for p in scan]
    n_nodes = len(nodes)
    n = 3 * n_nodes
    E = [(int(d["local"]), nl + int(d["scan"]), [float(v) for v in d["rel"]], _rows(d["info"]), bool(d.get("loop")))
         for d in edges]
    rows, _, _ = _linearize(nodes, E, 0.0, n, loss_kind, loss_scale)
    Hd = [dict(rw) for rw in rows]

    def blk(r, c):
        if not any((3 * c + j) in Hd[3 * r + i] for i in range(3) for j in range(3)):
            return None
        return [[Hd[3 * r + i].get(3 * c + j, 0.0) for j in range(3)] for i in range(3)]

    adj = {t: [s for s in range(nl) if blk(t, s) is not None] for t in range(nl, n_nodes)}
    B = {(t, s): blk(t, s) for t in adj for s in adj[t]}
    F, W = {}, {}
    for t in range(nl, n_nodes):
        if not adj[t]:
            continue                      # a scan node without edges takes no part
        F[t] = _ldl3(blk(t, t))
        for s in adj[t]:
            cols = [_solve3(F[t], [B[(t, s)][k][j] for k in range(3)]) for j in range(3)]
            W[(t, s)] = [[cols[j][k] for j in range(3)] for k in range(3)]
    ns = 3 * nl
    S = [[0.0] * ns for _ in range(ns)]
    of = [[t for t in range(nl, n_nodes) if s in adj[t]] for s in range(nl)]
    for s1 in range(nl):
        for s2 in range(s1 + 1):
            common = [t for t in of[s1] if s2 in adj[t]]
            if s1 != s2 and not common:
                continue
            A = blk(s1, s1) if s1 == s2 else None
            for i in range(3):
                for j in range(3):
                    v = A[i][j] if A else 0.0
                    for t in common:
                        v -= (B[(t, s1)][0][i] * W[(t, s2)][0][j] + B[(t, s1)][1][i] * W[(t, s2)][1][j] +
                              B[(t, s1)][2][i] * W[(t, s2)][2][j])
                    S[3 * s1 + i][3 * s2 + j] = v
    for i in range(ns):
        w = [0.0] * i
        Si = S[i]
        for j in range(i + 1):
            Sj = S[j]
            v = Si[j]
            for k in range(j):
                v -= w[k] * Sj[k]
            if j < i:
                Si[j] = v / Sj[j]
                w[j] = Si[j] * Sj[j]
            else:
                Si[i] = v
    # the columns
    need = set()
    for (s, t) in pairs:
        need.add(s)
        if t is not None and t >= 0:
            need.update(adj[nl + t])
    X = {}                                # (row, column) of S^-1, from the solved columns only
    for c in sorted(need):
        for j in range(3):
            f = 3 * c + j
            y = [0.0] * ns
            y[f] = 1.0
            for i in range(f + 1, ns):
                v = 0.0
                Si = S[i]
                for k in range(f, i):
                    v -= Si[k] * y[k]
                y[i] = v
            x = [y[i] / S[i][i] for i in range(ns)]
            for i in range(ns - 1, -1, -1):
                v = x[i]
                for k in range(ns - 1, i, -1):
                    v -= S[k][i] * x[k]
                x[i] = v
            for i in range(ns):
                X[(i, f)] = x[i]

    def xb(r, c):
        return [[X[(3 * r + i, 3 * c + j)] for j in range(3)] for i in range(3)]

    def mirrored(fn):
        out = [[0.0] * 3 for _ in range(3)]
        for i in range(3):
            for j in range(i + 1):
                out[i][j] = out[j][i] = fn(i, j)
        return out

    zero = [[0.0] * 3 for _ in range(3)]
    out = []
    for (s, t) in pairs:
        Xss = xb(s, s)
        sss = mirrored(lambda i, j: Xss[i][j])
        if t is None or t < 0:
            out.append(dict(local_cov=sss, scan_cov=zero, cross_cov=zero, relative_cov=zero))
            continue
        t = nl + t
        cols = [_solve3(F[t], [1.0 if k == j else 0.0 for k in range(3)]) for j in range(3)]
        Dinv = [[cols[j][i] for j in range(3)] for i in range(3)]
        sst = [[0.0] * 3 for _ in range(3)]
        for i in range(3):
            for j in range(3):
                acc = 0.0
                for s1 in adj[t]:
                    acc -= _mult(xb(s, s1), W[(t, s1)], i, j)
                sst[i][j] = acc

        def tt(i, j):
            acc = Dinv[i][j]
            for s1 in adj[t]:
                for s2 in adj[t]:
                    Xb = xb(s1, s2)
                    m = [[_mul(W[(t, s1)], Xb, i, k) for k in range(3)]]
                    acc += m[0][0] * W[(t, s2)][j][0] + m[0][1] * W[(t, s2)][j][1] + m[0][2] * W[(t, s2)][j][2]
            return acc
        stt = mirrored(tt)
        _, c, sn, x, y = _error(nodes[s], nodes[t], [0.0, 0.0, 0.0])
        Js = [[-c, -sn, y], [sn, -c, -x], [0.0, 0.0, -1.0]]
        Je = [[c, sn, 0.0], [-sn, c, 0.0], [0.0, 0.0, 1.0]]
        sts = [[sst[j][i] for j in range(3)] for i in range(3)]
        T1 = [[_mul(Js, sss, i, j) for j in range(3)] for i in range(3)]
        T2 = [[_mul(Js, sst, i, j) for j in range(3)] for i in range(3)]
        T3 = [[_mul(Je, sts, i, j) for j in range(3)] for i in range(3)]
        T4 = [[_mul(Je, stt, i, j) for j in range(3)] for i in range(3)]
        rel = mirrored(lambda i, j: _mult(T1, Js, i, j) + _mult(T2, Je, i, j) + _mult(T3, Js, i, j) +
                       _mult(T4, Je, i, j))
        out.append(dict(local_cov=sss, scan_cov=stt, cross_cov=sst, relative_cov=rel))
    return out


def dense_covariance(local, scan, edges, loss_kind="Huber", loss_scale=0.01):
    """numpy.linalg.inv of the dense H at lambda = 0: the yardstick that shares no arithmetic with the
    route above. Scan nodes without edges (zero rows) are left out; returns (Sigma, index of node -> row)."""
    import numpy as np
    from pose_graph_literal import dense_system
    H, _ = dense_system(local, scan, edges, 0.0, loss_kind, loss_scale)
    nl = len(local)
    used = set(range(nl)) | {nl + int(d["scan"]) for d in edges}
    keep = [k for k in range(nl + len(scan)) if k in used]
    idx = [3 * k + a for k in keep for a in range(3)]
    Sigma = np.linalg.inv(H[np.ix_(idx, idx)])
    return Sigma, {k: 3 * q for q, k in enumerate(keep)}
