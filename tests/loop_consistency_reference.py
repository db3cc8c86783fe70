"""An independent Python literal of the loop-edge consistency rule (include/csm_hip.h, csm_loop_consistency;
DESIGN.md 4o) and the cases its tests share. Plain Python floats (IEEE f64, one rounding per operation, no
fused multiply-add), math.cos / math.sin / math.fmod (the C library's), compound and inverse from products of
table entries, its own 3x3 LDL^T, and the greedy selection over Python sets. Every sum and product is written
in the order DESIGN.md 4o fixes, so chi^2 has the library's bits and everything after it is integers.

Cases (each seeded and small; `case(name)` builds and caches them, nothing modifies them):
  separated    a random walk of 120 scan nodes and 12 local maps; 40 edges whose noise is 0.3 sigma of their
               stated covariance, every fourth displaced by metres: the inliers form exactly one clique and no
               pair touching an outlier is consistent at gate 11.34 (asserted by the CPU test)
  ladder       200 edges on the same walk with full-sigma noise and every fourth displaced: a ragged relation;
               its prefixes are the M ladder
  peaks        several edges on the same (map, scan) pair, half a metre apart, among ordinary inliers
  duplicates   identical edges: e = 0, chi^2 = 0, consistent at gate 0
  drift        the estimates of the walk's second half are off by 0.5 m: a pair across the halves is
               inconsistent without the drift model and consistent with it
  two_cliques  the estimates of scan nodes 60.. are shifted rigidly: edges onto them agree with each other and
               with nobody else; cliques of 7 and 6. two_cliques_equal: 6 and 6, an edge of the second clique
               at index 0, so the tie goes to it
  bad_pivot    an information matrix of 1e-308 on the diagonal: Sigma = 1e308 is finite, the sum of two of them
               is not, so every pair with such an edge has a pivot that is not finite. (An indefinite M cannot
               be reached through the ABI: J Sigma J^T of a Sigma with positive pivots is positive
               semi-definite up to rounding; the literal's own test builds that one at the literal's level.)
  far_frame    `ladder`'s first 65 edges with every pose shifted by 1e5 m: parity only
"""
import math

import numpy as np

GATE = 11.34            # chi-square, 3 degrees of freedom, 99 %
PI = 3.14159265358979323846

_CACHE = {}


# ------------------------------------------------------------------ the literal

def normalize_angle(theta):
    t = math.fmod(theta, 2.0 * PI)
    if t > PI:
        t -= 2.0 * PI
    elif t < -PI:
        t += 2.0 * PI
    return t


def ldl3(m):
    """Unpivoted LDL^T of a 3x3 from its lower triangle: (d0, d1, d2, l10, l20, l21). A zero pivot divides:
    the quotient is what IEEE gives (the C code does not trap)."""
    def div(a, b):
        try:
            return a / b
        except ZeroDivisionError:
            if a != a or a == 0.0:
                return math.nan
            return math.copysign(math.inf, a) * math.copysign(1.0, b)
    d0 = m[0][0]
    l10 = div(m[1][0], d0)
    l20 = div(m[2][0], d0)
    d1 = m[1][1] - (l10 * d0) * l10
    l21 = div(m[2][1] - (l20 * d0) * l10, d1)
    d2 = m[2][2] - (l20 * d0) * l20 - (l21 * d1) * l21
    return d0, d1, d2, l10, l20, l21


def ldl3_solve(f, v0, v1, v2):
    d0, d1, d2, l10, l20, l21 = f
    y1 = v1 - l10 * v0
    y2 = v2 - l20 * v0 - l21 * y1
    z0, z1, z2 = v0 / d0, y1 / d1, y2 / d2
    x2 = z2
    x1 = z1 - l21 * x2
    x0 = z0 - l20 * x2 - l10 * x1
    return x0, x1, x2


def pivots_ok(f):
    return all(p > 0.0 and p <= 1.7976931348623157e308 for p in f[:3])


def inverse3(m):
    """The exactly symmetric inverse through the LDL^T: column j from e_j, entries i >= j mirrored. None when
    a pivot is not positive and finite."""
    f = ldl3(m)
    if not pivots_ok(f):
        return None
    out = [[0.0] * 3 for _ in range(3)]
    for j in range(3):
        x = ldl3_solve(f, 1.0 if j == 0 else 0.0, 1.0 if j == 1 else 0.0, 1.0 if j == 2 else 0.0)
        for i in range(j, 3):
            out[i][j] = x[i]
            out[j][i] = x[i]
    return out


def rot(c, s, x, y):
    return c * x - s * y, s * x + c * y


def rot_t(c, s, x, y):
    return c * x + s * y, c * y - s * x


def congruence(J, S):
    """Lower triangle of J S J^T, T = J S first, every three-term sum left to right."""
    T = [[(J[r][0] * S[0][k] + J[r][1] * S[1][k]) + J[r][2] * S[2][k] for k in range(3)] for r in range(3)]
    return [[(T[r][0] * J[c][0] + T[r][1] * J[c][1]) + T[r][2] * J[c][2] if c <= r else None for c in range(3)]
            for r in range(3)]


def edge_table(local_poses, scan_poses, e, local_travel, scan_travel):
    s, t = e["local"], e["scan"]
    z = [float(v) for v in e["rel"]]
    sigma = inverse3([[float(v) for v in row] for row in np.asarray(e["info"], dtype=np.float64).reshape(3, 3)])
    ps = [float(v) for v in local_poses[s]]
    pt = [float(v) for v in scan_poses[t]]
    return dict(z=z, cz=math.cos(z[2]), sz=math.sin(z[2]), sigma=sigma,
                ps=ps, cs=math.cos(ps[2]), ss=math.sin(ps[2]), ls=0.0 if local_travel is None else float(local_travel[s]),
                pt=pt, ct=math.cos(pt[2]), st=math.sin(pt[2]), lt=0.0 if scan_travel is None else float(scan_travel[t]))


def cycle(a, b):
    """(e, J_i, J_j) of the pair (a, b) = (edge i, edge j), i < j."""
    tb = rot_t(a["ct"], a["st"], b["pt"][0] - a["pt"][0], b["pt"][1] - a["pt"][1])
    cb = a["ct"] * b["ct"] + a["st"] * b["st"]
    sb = a["ct"] * b["st"] - a["st"] * b["ct"]
    r = rot_t(b["cz"], b["sz"], b["z"][0], b["z"][1])
    tc = (-r[0], -r[1])
    cc, sc = b["cz"], -b["sz"]
    td = rot_t(b["cs"], b["ss"], a["ps"][0] - b["ps"][0], a["ps"][1] - b["ps"][1])
    r = rot(cc, sc, td[0], td[1])
    w = (tc[0] + r[0], tc[1] + r[1])
    r = rot(cb, sb, w[0], w[1])
    u = (tb[0] + r[0], tb[1] + r[1])
    r = rot(a["cz"], a["sz"], u[0], u[1])
    e = [a["z"][0] + r[0], a["z"][1] + r[1],
         normalize_angle(((a["z"][2] + (b["pt"][2] - a["pt"][2])) - b["z"][2]) + (a["ps"][2] - b["ps"][2]))]
    g = rot(a["cz"], a["sz"], -u[1], u[0])
    Ji = [[1.0, 0.0, g[0]], [0.0, 1.0, g[1]], [0.0, 0.0, 1.0]]
    c1 = a["cz"] * cb - a["sz"] * sb
    s1 = a["sz"] * cb + a["cz"] * sb
    cq = c1 * cc - s1 * sc
    sq = s1 * cc + c1 * sc
    v = (b["z"][0] - td[0], b["z"][1] - td[1])
    h = rot(cq, sq, -v[1], v[0])
    Jj = [[-cq, sq, h[0]], [-sq, -cq, h[1]], [0.0, 0.0, -1.0]]
    return e, Ji, Jj


def pair_chi2(a, b, drift):
    """chi^2 of the pair, or None when a pivot of M is not positive and finite."""
    e, Ji, Jj = cycle(a, b)
    mi, mj = congruence(Ji, a["sigma"]), congruence(Jj, b["sigma"])
    length = abs(a["lt"] - b["lt"]) + abs(a["ls"] - b["ls"])
    M = [[None] * 3 for _ in range(3)]
    for r in range(3):
        for c in range(r + 1):
            M[r][c] = mi[r][c] + mj[r][c]
            if r == c:
                M[r][c] = M[r][c] + length * drift[r]
    f = ldl3(M)
    if not pivots_ok(f):
        return None
    x = ldl3_solve(f, e[0], e[1], e[2])
    return (e[0] * x[0] + e[1] * x[1]) + e[2] * x[2]


def chi2_matrix(local_poses, scan_poses, edges, drift=None, local_travel=None, scan_travel=None):
    """[M, M] float64: mirrored, zero diagonal, +inf where a pivot was bad; and the number of bad pivots."""
    d = [0.0, 0.0, 0.0] if drift is None else [float(v) for v in drift]
    tab = [edge_table(local_poses, scan_poses, e, local_travel if drift is not None else None,
                      scan_travel if drift is not None else None) for e in edges]
    m = len(edges)
    out = np.zeros((m, m))
    bad = 0
    for i in range(m):
        for j in range(i + 1, m):
            c = pair_chi2(tab[i], tab[j], d)
            if c is None:
                c = math.inf
                bad += 1
            out[i, j] = out[j, i] = c
    return out, bad


def select(chi2, gate, n_seeds=0):
    """The adjacency, degrees and the greedy selection from a chi^2 matrix (a NaN is not <= gate)."""
    m = chi2.shape[0]
    nb = [set(j for j in range(m) if j != i and chi2[min(i, j), max(i, j)] <= gate) for i in range(m)]
    degree = [len(s) for s in nb]
    n = m if n_seeds == 0 or n_seeds >= m else n_seeds
    seeds = sorted(range(m), key=lambda v: (-degree[v], v))[:n]
    best, best_seed = [], -1
    for v0 in seeds:
        K, C = [v0], set(nb[v0])
        while C:
            u = min(C, key=lambda w: (-len(nb[w] & C), w))
            K.append(u)
            C &= nb[u]
        if len(K) > len(best):
            best, best_seed = K, v0
    words = (m + 63) // 64
    adj = np.zeros((m, words), np.uint64)
    for i in range(m):
        for j in nb[i]:
            adj[i, j >> 6] |= np.uint64(1 << (j & 63))
    selected = np.zeros(m, np.int32)
    selected[best] = 1
    return dict(selected=selected, degree=np.array(degree, np.int32), adjacency=adj,
                info=dict(consistent_pairs=sum(degree) // 2, clique_size=len(best), winning_seed=best_seed,
                          seeds_run=n))


def literal(local_poses, scan_poses, edges, gate, drift=None, local_travel=None, scan_travel=None, n_seeds=0,
            chi2=None):
    """What loop_consistency returns with want_adjacency and want_chi2; chi2: a matrix computed before (with its
    count of bad pivots) to select from."""
    chi, bad = chi2 if chi2 is not None else chi2_matrix(local_poses, scan_poses, edges, drift, local_travel,
                                                          scan_travel)
    out = select(chi, gate, n_seeds)
    out["chi2"] = chi
    out["info"]["bad_pivots"] = bad
    return out


# ------------------------------------------------------------------ the cases

def inverse_compound(a, b):
    """InverseCompound(a, b): b in a's frame."""
    c, s = math.cos(a[2]), math.sin(a[2])
    dx, dy = b[0] - a[0], b[1] - a[1]
    return [c * dx + s * dy, -s * dx + c * dy, normalize_angle(b[2] - a[2])]


SIGMA = np.array([0.05, 0.05, 0.02])     # the stated standard deviations of a match


def walk(n=120, seed=5):
    """A random walk that stays in a 20 m box: many places are seen again."""
    rng = np.random.default_rng(seed)
    poses = np.zeros((n, 3))
    for i in range(1, n):
        th = poses[i - 1, 2] + rng.normal(0.0, 0.35)
        x, y = poses[i - 1, 0] + 0.5 * math.cos(th), poses[i - 1, 1] + 0.5 * math.sin(th)
        if abs(x) > 10.0 or abs(y) > 10.0:
            th += math.pi
            x, y = poses[i - 1, 0] + 0.5 * math.cos(th), poses[i - 1, 1] + 0.5 * math.sin(th)
        poses[i] = (x, y, normalize_angle(th))
    return poses


def travel_of(poses):
    d = np.hypot(np.diff(poses[:, 0]), np.diff(poses[:, 1]))
    return np.concatenate([[0.0], np.cumsum(d)])


def _graph(n_edges, noise, seed, outlier_every=4):
    truth = walk()
    rng = np.random.default_rng(seed)
    local = truth[::10].copy()                       # 12 local maps: the pose of their first scan node
    info = np.diag(1.0 / SIGMA ** 2)
    edges, outlier = [], []
    for k in range(n_edges):
        s, t = int(rng.integers(0, 12)), int(rng.integers(0, 120))
        z = np.array(inverse_compound(local[s], truth[t])) + noise * SIGMA * rng.normal(size=3)
        bad = outlier_every and k % outlier_every == 3
        if bad:
            a, r = rng.uniform(0.0, 2.0 * math.pi), rng.uniform(2.0, 5.0)
            z[:2] += (r * math.cos(a), r * math.sin(a))
        edges.append(dict(local=s, scan=t, rel=z.tolist(), info=info, loop=True))
        outlier.append(bool(bad))
    travel = travel_of(truth)
    return dict(local=local, scan=truth.copy(), edges=edges, outlier=np.array(outlier), gate=GATE,
                scan_travel=travel, local_travel=travel[::10].copy(), drift=None)


def _separated():
    return _graph(40, 0.3, 21)


def _ladder():
    return _graph(200, 1.0, 22)


def _peaks():
    c = _graph(12, 0.3, 23, outlier_every=0)
    base = c["edges"][0]
    for k in range(1, 4):               # three more peaks of edge 0's (map, scan) pair, half a metre apart
        z = list(base["rel"])
        z[0] += 0.5 * k
        c["edges"].append(dict(base, rel=z))
    c["peaks"] = [0, 12, 13, 14]
    c["outlier"] = np.zeros(len(c["edges"]), bool)
    return c


def _duplicates():
    c = _graph(6, 1.0, 24, outlier_every=0)
    c["edges"] = [dict(c["edges"][k]) for k in (0, 1, 0, 0, 2, 1)]
    c["same"] = [(0, 2), (0, 3), (2, 3), (1, 5)]
    c["outlier"] = np.zeros(6, bool)
    return c


def _drift():
    c = _graph(0, 0.0, 25)
    truth = c["scan"].copy()
    est = truth.copy()
    est[60:, 0] += 0.5                  # the second half's estimates have drifted
    info = np.diag(1.0 / SIGMA ** 2)
    c["scan"] = est
    c["edges"] = [dict(local=0, scan=5, rel=inverse_compound(c["local"][0], truth[5]), info=info, loop=True),
                  dict(local=1, scan=110, rel=inverse_compound(c["local"][1], truth[110]), info=info, loop=True),
                  dict(local=2, scan=20, rel=inverse_compound(c["local"][2], truth[20]), info=info, loop=True)]
    c["outlier"] = np.zeros(3, bool)
    c["drift"] = [0.01, 0.01, 1e-4]     # per metre; about 50 m lie between nodes 5 and 110
    c["flips"] = [(0, 1), (1, 2)]
    return c


def _two_cliques(equal):
    c = _graph(0, 0.0, 26)
    truth = c["scan"].copy()
    est = truth.copy()
    est[60:, :2] += (3.0, -2.0)         # a rigid shift: edges onto these nodes agree with each other only
    info = np.diag(1.0 / SIGMA ** 2)
    rng = np.random.default_rng(27)
    first = [int(v) for v in rng.choice(60, 6 if equal else 7, replace=False)]
    second = [int(v) + 60 for v in rng.choice(60, 6, replace=False)]
    order = ([("b", second[0])] if equal else []) + [("a", t) for t in first] + \
        [("b", t) for t in second[1 if equal else 0:]]
    c["scan"] = est
    c["edges"] = [dict(local=k % 6, scan=t, rel=inverse_compound(c["local"][k % 6], truth[t]), info=info, loop=True)
                  for k, (_, t) in enumerate(order)]
    c["groups"] = [g for g, _ in order]
    c["outlier"] = np.zeros(len(order), bool)
    return c


def _bad_pivot():
    c = _graph(8, 0.3, 28, outlier_every=0)
    for k in (2, 5):
        c["edges"][k] = dict(c["edges"][k], info=np.diag([1e-308, 1e-308, 1e-308]))
    c["overflowing"] = [2, 5]
    return c


def _far_frame():
    c = _ladder()
    c["edges"] = c["edges"][:65]
    c["outlier"] = c["outlier"][:65]
    c["local"] = c["local"] + (1e5, -1e5, 0.0)
    c["scan"] = c["scan"] + (1e5, -1e5, 0.0)
    return c


def end_to_end_graph():
    """60 scan nodes in 6 local maps whose estimates have drifted by 4 mm per node, the odometry edges that hold
    the graph together, and 12 loop edges of which every third is off by 4 to 6 metres. Returns the truth, the
    estimates, the odometry edges, the loop edges and the drift model under which the good loop edges agree."""
    if "e2e" in _CACHE:
        return _CACHE["e2e"]
    truth = walk(60, seed=31)
    est = truth.copy()
    est[:, 0] += 0.004 * np.arange(60)
    rng = np.random.default_rng(32)
    info = np.diag(1.0 / SIGMA ** 2)
    odo = []
    for m in range(6):
        for i in range(10 * m, 10 * m + 10):
            odo.append(dict(local=m, scan=i, rel=inverse_compound(est[10 * m], est[i]), info=info, loop=False))
        if m:
            odo.append(dict(local=m - 1, scan=10 * m, rel=inverse_compound(est[10 * m - 10], est[10 * m]), info=info,
                            loop=False))
    loops, outlier = [], []
    for k in range(12):
        s = int(rng.integers(0, 3))
        t = int(rng.integers(35, 60))
        z = np.array(inverse_compound(truth[10 * s], truth[t])) + 0.3 * SIGMA * rng.normal(size=3)
        if k % 3 == 2:
            a, r = rng.uniform(0.0, 2.0 * math.pi), rng.uniform(4.0, 6.0)
            z[:2] += (r * math.cos(a), r * math.sin(a))
        loops.append(dict(local=s, scan=t, rel=z.tolist(), info=info, loop=True))
        outlier.append(k % 3 == 2)
    travel = travel_of(est)
    _CACHE["e2e"] = dict(truth=truth, local=est[::10].copy(), scan=est, odometry=odo, loops=loops,
                         outlier=np.array(outlier), gate=GATE, drift=[0.005, 0.005, 1e-5],
                         local_travel=travel[::10].copy(), scan_travel=travel)
    return _CACHE["e2e"]


def position_error(scan_poses, truth):
    """Sum of the squared distances of the scan nodes from where they truly are."""
    d = np.asarray(scan_poses)[:, :2] - truth[:, :2]
    return float((d * d).sum())


_BUILDERS = dict(separated=_separated, ladder=_ladder, peaks=_peaks, duplicates=_duplicates, drift=_drift,
                 two_cliques=lambda: _two_cliques(False), two_cliques_equal=lambda: _two_cliques(True),
                 bad_pivot=_bad_pivot, far_frame=_far_frame)
CASES = tuple(_BUILDERS)
LADDER = (1, 2, 3, 63, 64, 65, 127, 128, 129, 200)


def case(name):
    if name not in _CACHE:
        _CACHE[name] = _BUILDERS[name]()
    return _CACHE[name]


def drift_args(c):
    """The drift model's three arguments of a case (None each without one)."""
    if c["drift"] is None:
        return dict(drift_var_per_metre=None, local_travel=None, scan_travel=None)
    return dict(drift_var_per_metre=c["drift"], local_travel=c["local_travel"], scan_travel=c["scan_travel"])


def case_chi2(name):
    """The literal's chi^2 matrix of a case (and its bad pivots), computed once."""
    key = ("chi2", name)
    if key not in _CACHE:
        c = case(name)
        _CACHE[key] = chi2_matrix(c["local"], c["scan"], c["edges"], c["drift"], c["local_travel"], c["scan_travel"])
    return _CACHE[key]


def prefix_chi2(name, m):
    """The chi^2 matrix of a case's first m edges: a pair's value does not depend on the other edges."""
    chi, _ = case_chi2(name)
    sub = chi[:m, :m].copy()
    return sub, int(np.isinf(np.triu(sub, 1)).sum())
