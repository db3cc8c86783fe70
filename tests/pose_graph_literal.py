"""An independent Python restatement of PoseGraphOptimizerLM::Optimize with the ConjugateGradient
solver (src/my_lidar_graph_slam/mapping/pose_graph_optimizer_lm.cpp:38-452,
robust_loss_function.cpp, Eigen's conjugate_gradient()), in scalar float arithmetic with
math.sin / math.cos / math.fmod (the C library the C++ restatement calls).

It keeps H the way the reference builds it: a list of (row, col, value) triplets in insertion
order, summed per entry in that order (setFromTriplets), lower triangle only and read as
self-adjoint. The orders the C++ restatement fixes are spelled out here again:
  - every 3-term product sum left to right; (Js^T Lambda) times w; e^T Lambda e = (e^T Lambda) e;
  - (H v)_i = sum over the row's stored entries of the self-adjoint matrix in ascending column
    order, from 0.0;
  - dot products and the total error: left to right from 0.0, or (pairwise=True) in a pairwise
    tree, the switch that sizes the device tolerance.
"""
import math

import numpy as np

LOSSES = ("Squared", "Huber", "Cauchy", "Fair", "GemanMcClure", "Welsch")
DBL_EPSILON = 2.220446049250313e-16
DBL_MIN = 2.2250738585072014e-308
DBL_MAX = 1.7976931348623157e308


def loss(kind, s, t):
    if kind == "Huber":
        return t if t <= s else 2.0 * math.sqrt(s * t) - s
    if kind == "Cauchy":
        return s * math.log1p(t / s)
    if kind == "Fair":
        q = math.sqrt(t / s)
        return 2.0 * s * (q - math.log1p(q))
    if kind == "GemanMcClure":
        return s * t / (s + t)
    if kind == "Welsch":
        return s * (-math.expm1(-t / s))
    return t


def weight(kind, s, t):
    if kind == "Huber":
        return 1.0 if t <= s else math.sqrt(s / t)
    if kind == "Cauchy":
        return s / (s + t)
    if kind == "Fair":
        return 1.0 / (1.0 + math.sqrt(t / s))
    if kind == "GemanMcClure":
        return (s * s) / ((s + t) * (s + t))
    if kind == "Welsch":
        return math.exp(-t / s)
    return 1.0


def normalize_angle(theta):
    t = math.fmod(theta, 2.0 * math.pi)
    if t > math.pi:
        t -= 2.0 * math.pi
    elif t < -math.pi:
        t += 2.0 * math.pi
    return t


def _error(ps, pe, z):
    s = math.sin(ps[2])
    c = math.cos(ps[2])
    d = [pe[0] - ps[0], pe[1] - ps[1], pe[2] - ps[2]]
    x = c * d[0] + s * d[1]
    y = -s * d[0] + c * d[1]
    return [x - z[0], y - z[1], normalize_angle(d[2] - z[2])], c, s, x, y


def _quad(e, L):
    u = [e[0] * L[0][j] + e[1] * L[1][j] + e[2] * L[2][j] for j in range(3)]
    return u[0] * e[0] + u[1] * e[1] + u[2] * e[2]


def _mat(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def _vec(A, v):
    return [A[i][0] * v[0] + A[i][1] * v[1] + A[i][2] * v[2] for i in range(3)]


def _sum(vals, pairwise):
    if not pairwise:
        s = 0.0
        for v in vals:
            s += v
        return s

    def tree(lo, hi):
        if hi - lo == 1:
            return vals[lo]
        mid = (lo + hi) // 2
        return tree(lo, mid) + tree(mid, hi)
    return tree(0, len(vals)) if vals else 0.0


def total_error(nodes, edges, kind, scale, pairwise=False):
    """ComputeTotalError"""
    terms = []
    for (s, t, z, L, _) in edges:
        e = _error(nodes[s], nodes[t], z)[0]
        terms.append(loss(kind, scale, _quad(e, L)))
    return _sum(terms, pairwise)


def _linearize(nodes, E, lam, n, loss_kind, loss_scale):
    """OptimizeStep up to the solve: the rows of the self-adjoint H (ascending columns), its
    diagonal and b"""
    # OptimizeStep: triplets in insertion order
    trip = [(i, i, 1e9) for i in range(3)] + [(i, i, lam) for i in range(n)]
    b = [0.0] * n
    for (si, ti, z, L, is_loop) in E:
        e, c, s, x, y = _error(nodes[si], nodes[ti], z)
        Js = [[-c, -s, y], [s, -c, -x], [0.0, 0.0, -1.0]]
        Je = [[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]]
        w = weight(loss_kind, loss_scale, _quad(e, L)) if is_loop else 1.0
        JsT = [[Js[k][i] for k in range(3)] for i in range(3)]
        JeT = [[Je[k][i] for k in range(3)] for i in range(3)]
        Ts = [[v * w for v in row] for row in _mat(JsT, L)]
        Te = [[v * w for v in row] for row in _mat(JeT, L)]
        A, B, C = _mat(Ts, Js), _mat(Te, Je), _mat(Ts, Je)
        sb, tb = 3 * si, 3 * ti
        for i in range(3):
            for j in range(i + 1):
                trip.append((sb + i, sb + j, A[i][j]))
                trip.append((tb + i, tb + j, B[i][j]))
            for j in range(3):
                trip.append((tb + i, sb + j, C[j][i]))
        bs, be = _vec(Ts, e), _vec(Te, e)
        for i in range(3):
            b[sb + i] -= bs[i]
            b[tb + i] -= be[i]
    H = {}
    for (r, c, v) in trip:
        if (r, c) in H:
            H[(r, c)] += v
        else:
            H[(r, c)] = v
    rows = [dict() for _ in range(n)]
    for (r, c), v in H.items():
        rows[r][c] = v
        rows[c][r] = v
    rows = [sorted(rw.items()) for rw in rows]
    diag = [H[(i, i)] for i in range(n)]
    return rows, diag, b


def optimize(local, scan, edges, lam, iterations_max=10, error_tolerance=1e-4, loss_kind="Huber",
             loss_scale=0.01, pairwise=False):
    """local, scan: lists of [x, y, theta]; edges: dicts as synth.pose_graph_case makes. Returns
    (local, scan, lambda, trace, initial_error) with trace = [(total, lambda, |b|^2, |r|^2, cg iterations)]."""
    nl = len(local)
    nodes = [[float(v) for v in p] for p in local] + [[float(v) for v in p] for p in scan]
    n = 3 * len(nodes)
    E = []
    for d in edges:
        L = [[float(v) for v in row] for row in _rows(d["info"])]
        E.append((int(d["local"]), nl + int(d["scan"]), [float(v) for v in d["rel"]], L, bool(d.get("loop"))))

    def dot(a, b):
        return _sum([a[i] * b[i] for i in range(n)], pairwise)

    prev = DBL_MAX
    total = DBL_MAX
    initial = total_error(nodes, E, loss_kind, loss_scale, pairwise)
    trace = []
    while True:
        rows, diag, b = _linearize(nodes, E, lam, n, loss_kind, loss_scale)
        invd = [1.0 / d if d != 0.0 else 1.0 for d in diag]

        def mv(v):
            out = []
            for rw in rows:
                acc = 0.0
                for c, h in rw:
                    acc += h * v[c]
                out.append(acc)
            return out

        # conjugate_gradient, x0 = 0
        x = [0.0] * n
        r = list(b)
        rhs2 = dot(b, b)
        r2 = rhs2
        it = 0
        if rhs2 != 0.0:
            a = DBL_EPSILON * DBL_EPSILON * rhs2
            thr = DBL_MIN if a < DBL_MIN else a
            if not (r2 < thr):
                p = [invd[i] * r[i] for i in range(n)]
                abs_new = dot(r, p)
                while it < 2 * n:
                    ap = mv(p)
                    alpha = abs_new / dot(p, ap)
                    x = [x[i] + alpha * p[i] for i in range(n)]
                    r = [r[i] - alpha * ap[i] for i in range(n)]
                    r2 = dot(r, r)
                    if r2 < thr:
                        break
                    z = [invd[i] * r[i] for i in range(n)]
                    abs_old = abs_new
                    abs_new = dot(r, z)
                    beta = abs_new / abs_old
                    p = [z[i] + beta * p[i] for i in range(n)]
                    it += 1
        for k in range(len(nodes)):
            for j in range(3):
                nodes[k][j] += x[3 * k + j]
        total = total_error(nodes, E, loss_kind, loss_scale, pairwise)
        trace.append((total, lam, rhs2, r2, it))
        if len(trace) >= iterations_max or abs(prev - total) < error_tolerance:
            break
        lam = lam * 0.5 if total < prev else lam * 2.0
        prev = total
    return nodes[:nl], nodes[nl:], lam, trace, initial


def _rows(info):
    flat = [float(v) for v in np.asarray(info, dtype=np.float64).reshape(9)]
    return [flat[0:3], flat[3:6], flat[6:9]]


def dense_system(local, scan, edges, lam, loss_kind="Huber", loss_scale=0.01):
    """The dense H (both triangles) and b of one OptimizeStep at the given poses"""
    nl = len(local)
    nodes = [[float(v) for v in p] for p in local] + [[float(v) for v in p] for p in scan]
    n = 3 * len(nodes)
    E = [(int(d["local"]), nl + int(d["scan"]), [float(v) for v in d["rel"]], _rows(d["info"]), bool(d.get("loop")))
         for d in edges]
    rows, _, b = _linearize(nodes, E, lam, n, loss_kind, loss_scale)
    H = np.zeros((n, n))
    for i, rw in enumerate(rows):
        for c, h in rw:
            H[i, c] = h
    return H, np.array(b)
