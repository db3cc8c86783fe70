"""The graphs, pair lists, error measure and recorded figures that test_cpu_pose_graph_marginals.py and
test_gpu_pose_graph_marginals.py share.

A case is (graph name, pair-list name). The graphs are synth.pose_graph_case chains and the connected
shapes of pose_graph_cases.py; every one is built once, shared and not to be changed by a test.

Error measure of every tolerance: |delta_ij| / sqrt(Sigma_ii Sigma_jj) with Sigma from the yardstick
(numpy.linalg.inv of the dense H; for relative_cov, J Sigma J^T of that inverse). Entries range from 1e-9
at the anchor to 0.4 elsewhere, so an absolute or a max-relative bound would test nothing.
"""
import math

import numpy as np

from csm_hip import synth
import pose_graph_cases as PC
import pose_graph_marginals_literal as ML

BLOCKS = ("local_cov", "scan_cov", "cross_cov", "relative_cov")
GROUP = 16      # kPgcGroup: local map nodes per column group of the substitution kernels

_SYNTH = {"synth%d" % s: (s, n, 10) for s, n in enumerate((40, 60, 80, 100, 120, 150))}
# 16 local maps: 3 n_local = 48, exactly one tile; 17: 51, padded to 96 (columns in the padded tile)
_SYNTH.update({"plain16": (916, 80, 5), "plain17": (917, 85, 5)})
_SHAPES = {"plain33": (330, None), "plain49": (490, None), "dense8": (40, "dense"), "dense33": (330, "dense"),
           "dense49": (490, "dense"), "dup8": (40, "dup"), "dup33": (330, "dup"), "wrapped8": (40, "wrapped"),
           "wrapped33": (330, "wrapped"), "one_local": (40, "one_local")}
_graphs = {}


def graph(name):
    if name not in _graphs:
        if name in _SYNTH:
            seed, n, spm = _SYNTH[name]
            c = synth.pose_graph_case(seed, n_scans=n, scans_per_map=spm, wrong_fraction=0.1)
        elif name == "alone":            # one local map node, n_scan = 0: 3 n_local = 3
            c = dict(PC.case(40, "no_scan"))
            c["local"] = c["local"][:1].copy()
        elif name == "star":             # one local map, every scan node tied to it by one edge, no loop edge
            c = dict(PC.case(40, "one_local"))
            seen, c["edges"] = set(), []
            for e in PC.case(40, "one_local")["edges"]:
                if e["scan"] not in seen:
                    seen.add(e["scan"])
                    c["edges"].append(dict(e, loop=0))
        else:
            c = PC.case(*_SHAPES[name])
        _graphs[name] = c
    return _graphs[name]


def adjacency(c):
    adj = {}
    for e in c["edges"]:
        adj.setdefault(e["scan"], set()).add(e["local"])
    return {t: sorted(s) for t, s in adj.items()}


def pairs(name, kind):
    """mixed: both end local maps alone (scan_index -1), then for some scan nodes (of every degree the graph
    has) a pair with an adjacent local map, one with a local map that is not adjacent, one with the anchor.
    one: a single local map (|C| = 1). all: every local map (|C| = n_local). cK: the first K local maps of
    an even spread (|C| = K: one below, at and one above the column-group width)."""
    c = graph(name)
    nl = len(c["local"])
    if kind == "one":
        return [(nl // 2, None)]
    if kind == "all":
        return [(s, None) for s in range(nl)]
    if kind[0] == "c":
        k = int(kind[1:])
        return [((s * nl) // k, None) for s in range(k)]
    adj = adjacency(c)
    out = [(0, None), (nl - 1, None)]
    by_degree = {}
    for t in sorted(adj):
        by_degree.setdefault(len(adj[t]), []).append(t)
    for deg in sorted(by_degree):
        for t in (by_degree[deg][0], by_degree[deg][-1]):
            non = [s for s in range(nl) if s not in adj[t]]
            out.append((adj[t][-1], t))
            if non:
                out.append((non[len(non) // 2], t))
            out.append((0, t))
    return out


# the CPU file's cases; the GPU file runs those named in its own list, against the figures below
CASES = ([("synth%d" % s, "mixed") for s in range(6)] +
         [("dense8", "mixed"), ("dense33", "mixed"), ("dense49", "mixed"), ("dup8", "mixed"), ("dup33", "mixed"),
          ("wrapped8", "mixed"), ("wrapped33", "mixed"), ("one_local", "mixed"), ("star", "mixed"), ("alone", "one"),
          ("plain16", "mixed"), ("plain16", "all"), ("plain17", "mixed"), ("plain17", "c15"), ("plain17", "c16"),
          ("plain17", "all"), ("plain33", "mixed"), ("plain33", "one"), ("plain33", "all"), ("plain49", "mixed"),
          ("plain49", "all")])

_literal, _yardstick = {}, {}


def literal(name, kind):
    if (name, kind) not in _literal:
        c = graph(name)
        _literal[(name, kind)] = ML.marginals(c["local"].tolist(), c["scan"].tolist(), c["edges"], pairs(name, kind))
    return _literal[(name, kind)]


def yardstick(name):
    if name not in _yardstick:
        c = graph(name)
        _yardstick[name] = ML.dense_covariance(c["local"].tolist(), c["scan"].tolist(), c["edges"])
    return _yardstick[name]


def expected(name, kind):
    """the four blocks of every pair from numpy's inverse"""
    c = graph(name)
    Sigma, at = yardstick(name)
    nl = len(c["local"])
    out = []
    for (s, t) in pairs(name, kind):
        a = at[s]
        rec = dict(local_cov=Sigma[a:a + 3, a:a + 3])
        if t is not None:
            b = at[nl + t]
            ps, pe = c["local"][s], c["scan"][t]
            sn, co = math.sin(ps[2]), math.cos(ps[2])
            d0, d1 = pe[0] - ps[0], pe[1] - ps[1]
            x, y = co * d0 + sn * d1, -sn * d0 + co * d1
            J = np.array([[-co, -sn, y, co, sn, 0.0], [sn, -co, -x, -sn, co, 0.0], [0.0, 0.0, -1.0, 0.0, 0.0, 1.0]])
            idx = list(range(a, a + 3)) + list(range(b, b + 3))
            rec.update(scan_cov=Sigma[b:b + 3, b:b + 3], cross_cov=Sigma[a:a + 3, b:b + 3],
                       relative_cov=J @ Sigma[np.ix_(idx, idx)] @ J.T)
        out.append(rec)
    return out


def error(records, name, kind):
    """the largest |delta_ij| / sqrt(Sigma_ii Sigma_jj) of the records against the yardstick"""
    c = graph(name)
    Sigma, at = yardstick(name)
    nl = len(c["local"])
    dg = np.diag(Sigma)
    worst = 0.0
    for (s, t), got, want in zip(pairs(name, kind), records, expected(name, kind)):
        ds = dg[at[s]:at[s] + 3]
        scale = dict(local_cov=(ds, ds))
        if t is not None:
            dt = dg[at[nl + t]:at[nl + t] + 3]
            dr = np.diag(want["relative_cov"])
            scale.update(scan_cov=(dt, dt), cross_cov=(ds, dt), relative_cov=(dr, dr))
        for k, (di, dj) in scale.items():
            delta = np.abs(np.asarray(got[k], dtype=np.float64) - want[k]) / np.sqrt(np.outer(di, dj))
            worst = max(worst, float(delta.max()))
    return worst


def same_bits(a, b):
    """two record lists, bit for bit"""
    return len(a) == len(b) and all(
        np.asarray(x[k], dtype=np.float64).tobytes() == np.asarray(y[k], dtype=np.float64).tobytes()
        for x, y in zip(a, b) for k in BLOCKS)


# The literal (pose_graph_marginals_literal.marginals) against the yardstick, `error` of every case:
# recorded from the literal itself, before any library or device run was compared. The host restatement is
# held to 10 x the figure of its case (the margin of the Schur solver's numpy check), the device to 100 x.
LITERAL_ERROR = {
    ("synth0", "mixed"): 1.2851729062801238e-14,
    ("synth1", "mixed"): 1.0588630190831411e-14,
    ("synth2", "mixed"): 5.181673079521378e-14,
    ("synth3", "mixed"): 3.7173756035063435e-14,
    ("synth4", "mixed"): 8.192957236024665e-14,
    ("synth5", "mixed"): 5.982740319066584e-14,
    ("dense8", "mixed"): 2.7016078240184338e-14,
    ("dense33", "mixed"): 1.891415679572242e-14,
    ("dense49", "mixed"): 1.4142617096177435e-14,
    ("dup8", "mixed"): 3.6392800339213424e-14,
    ("dup33", "mixed"): 2.93304883467978e-13,
    ("wrapped8", "mixed"): 3.9016085860327234e-14,
    ("wrapped33", "mixed"): 7.360833291999475e-13,
    ("one_local", "mixed"): 7.789513162880872e-16,
    ("star", "mixed"): 8.8249950143708e-16,
    ("alone", "one"): 0.0,
    ("plain16", "mixed"): 4.156353245249401e-14,
    ("plain16", "all"): 5.021604879691598e-14,
    ("plain17", "mixed"): 3.1012108802098855e-13,
    ("plain17", "c15"): 3.1012108802098855e-13,
    ("plain17", "c16"): 3.1012108802098855e-13,
    ("plain17", "all"): 3.1012108802098855e-13,
    ("plain33", "mixed"): 7.484113123825528e-13,
    ("plain33", "one"): 5.348455315945504e-13,
    ("plain33", "all"): 8.144174142997794e-13,
    ("plain49", "mixed"): 3.1173435237116837e-12,
    ("plain49", "all"): 3.1173435237116837e-12,
}


def bound(name, kind, factor):
    return factor * LITERAL_ERROR[(name, kind)]
