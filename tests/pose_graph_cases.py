"""Pose graphs of shapes that synth.pose_graph_case never makes, shared by the CPU and GPU tests
(test_cpu_pose_graph_cases.py pins the host restatement to the Python literals on them,
test_gpu_pose_graph_cases.py holds the device to the host).

A synth.pose_graph_case graph is a chain: each scan node has one to three edges, every local map node
has edges, no pair of nodes repeats and every heading grows without wrapping. Every function here
takes such a dict and returns a new one (the input is left alone) with local, scan, truth_local,
truth_scan and edges, plus the indices a test needs (`isolated_scans`, `idle_local`).

What each variant reaches in csm_posegraph_kernels.hip / csm_posegraph_api.hip:
  isolated     two scan nodes without edges: the kPgDiagOnly row entry, a lambda-only D_t in pg_ldl3
  idle_local   a local map node without edges, appended or inserted: a lambda-only block of S
  dense        every scan node tied to half of the local maps: every block of S stored, long sb_pair lists
  dup          every third edge twice: cross blocks that sum several edges (pg_assemble_cross)
  wrapped      headings in (-pi, pi]: d2 - z2 crosses +-pi in pg_normalize_angle
  zero         e = 0 on every edge (local map headings 0, so also with the device's sin / cos): b = 0,
               the conjugate-gradient loop's rhs2 == 0 branch
  one_local    a single local map node
  no_scan      no scan node and no edge: the launches that are skipped for an empty list
"""
import copy
import math

import numpy as np

from csm_hip import synth

VARIANTS = ("isolated", "idle_local_appended", "idle_local_inserted", "dense", "dup", "wrapped", "zero",
            "one_local", "no_scan")


def _spd_info(rng, sigma=(0.05, 0.05, 0.02)):
    """a random SPD covariance as synth.pose_graph_case draws it, and its inverse"""
    m = rng.randn(3, 3) * 0.3 + np.eye(3)
    sd = np.diag(sigma) * (0.5 + rng.rand())
    cov = sd @ (m @ m.T + 0.1 * np.eye(3)) @ sd
    info = np.linalg.inv(cov)
    return cov, 0.5 * (info + info.T)


def _truth_edge(rng, c, local, scan, loop):
    """an edge whose measurement is the true relative pose plus noise of a random SPD covariance"""
    cov, info = _spd_info(rng)
    rel = synth._inverse_compound(c["truth_local"][local], c["truth_scan"][scan])
    rel = np.asarray(rel) + np.linalg.cholesky(cov) @ rng.randn(3)
    return dict(local=int(local), scan=int(scan), rel=[float(v) for v in rel], info=info, loop=loop)


def isolated(c):
    """all edges of two scan nodes removed: one in the middle and the last one"""
    c = copy.deepcopy(c)
    gone = [len(c["scan"]) // 2, len(c["scan"]) - 1]
    c["edges"] = [e for e in c["edges"] if e["scan"] not in gone]
    c["isolated_scans"] = gone
    return c


def idle_local(c, inserted):
    """a local map node without an edge: appended, or inserted in the middle with the edges' local map
    indices shifted"""
    c = copy.deepcopy(c)
    nl = len(c["local"])
    at = nl // 2 if inserted else nl
    pose = np.array([0.3, -0.2, 0.7])
    c["local"] = np.insert(c["local"], at, pose, axis=0)
    c["truth_local"] = np.insert(c["truth_local"], at, pose, axis=0)
    for e in c["edges"]:
        if e["local"] >= at:
            e["local"] += 1
    c["idle_local"] = at
    return c


def dense(c, seed=7):
    """scan node k gets an extra loop edge to every local map s with (k + s) % 2 == 0"""
    c = copy.deepcopy(c)
    rng = np.random.RandomState(seed)
    for k in range(len(c["scan"])):
        for s in range(len(c["local"])):
            if (k + s) % 2 == 0:
                c["edges"].append(_truth_edge(rng, c, s, k, 1))
    return c


def dup(c):
    """every third edge appended again"""
    c = copy.deepcopy(c)
    c["edges"] += [copy.deepcopy(e) for e in c["edges"][::3]]
    return c


def wrap_angle(t):
    """into (-pi, pi]"""
    return -((-t + math.pi) % (2.0 * math.pi) - math.pi)


def wrapped(c):
    """all initial headings wrapped into (-pi, pi]"""
    c = copy.deepcopy(c)
    for key in ("local", "scan"):
        c[key][:, 2] = [wrap_angle(t) for t in c[key][:, 2]]
    return c


def zero_rhs(c, exact_trig=False):
    """every measurement equal to the relative pose of the initial estimate, computed with the same
    arithmetic: e = 0 exactly, so b = 0 and the CG returns at once.
    "The same arithmetic" is the host's: math.sin / math.cos are the C library's. The device library's
    sin / cos differ from them in the last place at some headings (at 330 scan nodes the device showed
    rhs_norm2 = 2.3e-23 where the host has 0.0), and then e is ~1e-16 on the device, not 0. With
    exact_trig every local map heading is set to 0.0 first, where sin = 0 and cos = 1 in any library,
    so e = 0 holds on the host and on the device alike."""
    c = copy.deepcopy(c)
    if exact_trig:
        c["local"][:, 2] = 0.0
    nodes = c["local"].tolist() + c["scan"].tolist()
    nl = len(c["local"])
    for e in c["edges"]:
        ps, pe = nodes[e["local"]], nodes[nl + e["scan"]]
        s, co = math.sin(ps[2]), math.cos(ps[2])
        d = [pe[0] - ps[0], pe[1] - ps[1], pe[2] - ps[2]]
        e["rel"] = [co * d[0] + s * d[1], -s * d[0] + co * d[1], d[2]]
    return c


def one_local(c, seed=11):
    """a single local map node: every edge tied to node 0, measured from the truth"""
    c = copy.deepcopy(c)
    rng = np.random.RandomState(seed)
    c["local"] = c["local"][:1].copy()
    c["truth_local"] = c["truth_local"][:1].copy()
    c["edges"] = [_truth_edge(rng, c, 0, e["scan"], e["loop"]) for e in c["edges"]]
    return c


def no_scan(c):
    """the local map nodes alone: n_scan = 0 and no edges"""
    c = copy.deepcopy(c)
    c["scan"] = np.zeros((0, 3))
    c["truth_scan"] = np.zeros((0, 3))
    c["edges"] = []
    return c


def variant(c, name):
    if name == "isolated":
        return isolated(c)
    if name == "idle_local_appended":
        return idle_local(c, False)
    if name == "idle_local_inserted":
        return idle_local(c, True)
    if name == "zero":
        return zero_rhs(c, exact_trig=True)
    return {"dense": dense, "dup": dup, "wrapped": wrapped, "one_local": one_local, "no_scan": no_scan}[name](c)


# ---------------------------------------------------------------- the structure, as the library builds it

def degrees(c):
    """edges per local map node and per scan node"""
    dl, ds = [0] * len(c["local"]), [0] * len(c["scan"])
    for e in c["edges"]:
        dl[e["local"]] += 1
        ds[e["scan"]] += 1
    return dl, ds


def pair_counts(c):
    """edges per distinct (scan node, local map node) pair: the cross blocks and their list lengths"""
    out = {}
    for e in c["edges"]:
        key = (e["scan"], e["local"])
        out[key] = out.get(key, 0) + 1
    return out


def schur_list_lengths(c):
    """per stored block (s1 >= s2) of the Schur complement, the number of scan nodes adjacent to both
    local map nodes: the length of its sb_pair list. Diagonal blocks are always stored."""
    adj = {}
    for (t, s) in pair_counts(c):
        adj.setdefault(t, set()).add(s)
    out = {(s, s): 0 for s in range(len(c["local"]))}
    for t, ss in adj.items():
        for s1 in ss:
            for s2 in ss:
                if s1 >= s2:
                    out[(s1, s2)] = out.get((s1, s2), 0) + 1
    return out


def counts(c):
    """(n_nodes, n_vars, n_edges, n_cross)"""
    n = len(c["local"]) + len(c["scan"])
    return n, 3 * n, len(c["edges"]), len(pair_counts(c))


def with_edge_count(c, n_edges):
    """trailing loop edges trimmed, or appended again in turn, until the graph has n_edges edges"""
    c = copy.deepcopy(c)
    loops = [i for i, e in enumerate(c["edges"]) if e["loop"]]
    assert loops
    while len(c["edges"]) > n_edges:
        del c["edges"][loops.pop()]
    k = 0
    while len(c["edges"]) < n_edges:
        k += 1
        c["edges"].append(copy.deepcopy(c["edges"][loops[-((k - 1) % len(loops)) - 1]]))
    return c


def with_block_count(c, total):
    """trailing loop edges trimmed until n_nodes + n_cross == total (a plain graph repeats no pair, so
    every trimmed edge takes one cross block with it)"""
    n_nodes, _, n_edges, n_cross = counts(c)
    assert n_cross == n_edges and n_nodes + n_cross >= total
    return with_edge_count(c, total - n_nodes)


# ---------------------------------------------------------------- the graphs both test files run

# n_scans -> (seed, scans per map): n_local 8 (3 n_local = 24: one workgroup, S in LDS), 33 (99: the
# blocked factorization, three tiles) and, for `dense` only, 49 (147: a fourth tile)
SIZES = {40: (940, 5), 330: (1230, 10), 490: (1390, 10)}
WRONG_FRACTION = 0.1
_cache = {}


def case(n_scans, name=None):
    """The plain graph of a size (name None) or one of its variants: built once, shared, not to be
    changed by a test."""
    key = (n_scans, name)
    if key not in _cache:
        if name is None:
            seed, spm = SIZES[n_scans]
            c = synth.pose_graph_case(seed, n_scans=n_scans, scans_per_map=spm, wrong_fraction=WRONG_FRACTION)
        else:
            c = variant(case(n_scans), name)
        for k in ("local", "scan", "truth_local", "truth_scan"):
            c[k].flags.writeable = False
        _cache[key] = c
    return _cache[key]
