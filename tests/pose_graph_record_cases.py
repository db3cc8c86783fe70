"""What the pose-graph unit COMPUTES on the device, bit for bit: csm_pose_graph_lm with both solvers and
csm_pose_graph_marginals on seeded graphs. tests/golden/make_pose_graph_records.py records the results with the
library of the commit it runs on, tests/test_gpu_pose_graph_records.py recomputes them with the built library
and compares: every double as its float.hex() string, every count as an integer. The parity tests hold the
device to the host within tolerances; a change that moves the device's bits inside them shows here.

Shapes, the smallest that reach every path of csm_posegraph_kernels.hip:
  cg / schur_small   rows 3 (24 scans, Huber, loops), 10 (duplicate edges), 13 (b = 0), 15 (stops early) and 20
                     (a scan node without edges) of test_cpu_pose_graph.CASES: 3 n_local <= 96, one workgroup
  cg                 wide765: n_vars = 765, more than one stride of the kernel's 512 threads
  schur_blocked      local33 (3 n_local = 99: three tiles, the last one padded), dense49 (147: a fourth tile)
  lm_at_its_steps    row 15 with iterations_max = the steps it took: the same result as with 10, where the
                     direct solver's chain launches the kernels of the remaining steps, which return at once
  marginals          local33: a local map alone, the last local map with the last scan node, a scan node tied
                     to two local maps; dense49: every local map with the last scan node (49 columns: four
                     column groups whose first unit rows lie in different panels)"""
import numpy as np

from csm_hip import synth
import pose_graph_cases as PC
from test_cpu_pose_graph import CASES, _case

ROWS = (3, 10, 13, 15, 20)
STOP_ROW, ZERO_ROW = 15, 13
DEFAULTS = dict(loss="Huber", loss_scale=0.01, iterations_max=10, error_tolerance=1e-4, lambda_=1e-4)
BLOCKS = ("local_cov", "scan_cov", "cross_cov", "relative_cov")
SOLVERS = {"cg": "ConjugateGradient", "schur": "SchurCholesky"}
_graphs = {}


def graph(name):
    """(graph dict, optimizer settings): built once, shared, not to be changed"""
    if name not in _graphs:
        if name.startswith("row"):
            seed, n, spm, wf, loss, scale, itmax, tol, lam, variant = CASES[int(name[3:]) - 1]
            assert seed == int(name[3:])
            _graphs[name] = (_case(seed, n, spm, wf, variant),
                             dict(loss=loss, loss_scale=scale, iterations_max=itmax, error_tolerance=tol, lambda_=lam))
        elif name == "wide765":
            _graphs[name] = (synth.pose_graph_case(1031, n_scans=231), DEFAULTS)
        elif name == "local33":
            _graphs[name] = (synth.pose_graph_case(733, n_scans=330), DEFAULTS)
        else:
            assert name == "dense49"
            _graphs[name] = (PC.case(490, "dense"), DEFAULTS)
    return _graphs[name]


LM_CASES = ([("cg", "row%d" % r) for r in ROWS] + [("cg", "wide765")] + [("schur", "row%d" % r) for r in ROWS] +
            [("schur", "local33"), ("schur", "dense49")])
BLOCKED = ("local33", "dense49")


def last_scan_with_edges(c):
    return max(e["scan"] for e in c["edges"])


def marginal_pairs(name):
    c = graph(name)[0]
    nl, last = len(c["local"]), last_scan_with_edges(c)
    if name == "dense49":
        return [(s, last) for s in range(nl)]
    touched = {}
    for e in c["edges"]:
        touched.setdefault(e["scan"], set()).add(e["local"])
    two = min(t for t, s in touched.items() if len(s) == 2)
    return [(0, None), (nl - 1, last), (min(touched[two]), two)]


def _hex(values):
    return [float(v).hex() for v in np.asarray(values, dtype=np.float64).ravel()]


def lm_record(result):
    lp, sp, info = result
    return dict(local=_hex(lp), scan=_hex(sp), steps=int(info["steps"]), cg_iterations=int(info["cg_iterations"]),
                initial_error=float(info["initial_error"]).hex(), final_error=float(info["final_error"]).hex(),
                final_lambda=float(info["lambda_"]).hex(),
                trace=[dict(total_error=float(t["total_error"]).hex(), lambda_=float(t["lambda_"]).hex(),
                            rhs_norm2=float(t["rhs_norm2"]).hex(), residual_norm2=float(t["residual_norm2"]).hex(),
                            cg_iterations=int(t["cg_iterations"])) for t in info["trace"]])


def run_lm(ctx, solver, name, iterations_max=None):
    c, kw = graph(name)
    kw = dict(kw, solver=SOLVERS[solver])
    if iterations_max is not None:
        kw["iterations_max"] = iterations_max
    lam = kw.pop("lambda_")
    return lm_record(ctx.pose_graph_lm(c["local"], c["scan"], c["edges"], lam, **kw))


def run_marginals(ctx, name):
    c = graph(name)[0]
    recs, info = ctx.pose_graph_marginals(c["local"], c["scan"], c["edges"], marginal_pairs(name))
    return dict(n_columns=int(info["n_columns"]),
                pairs=[dict({k: _hex(r[k]) for k in BLOCKS}, finite=int(r["finite"])) for r in recs])


def record(ctx):
    """Every case on context `ctx` (a Context for the device; anything with the same two methods otherwise)"""
    doc = {"lm": {}, "lm_at_its_steps": {}, "marginals": {}}
    for solver, name in LM_CASES:
        doc["lm"]["%s-%s" % (solver, name)] = run_lm(ctx, solver, name)
    for solver in SOLVERS:
        steps = doc["lm"]["%s-row%d" % (solver, STOP_ROW)]["steps"]
        doc["lm_at_its_steps"]["%s-row%d" % (solver, STOP_ROW)] = run_lm(ctx, solver, "row%d" % STOP_ROW, steps)
    for name in BLOCKED:
        doc["marginals"][name] = run_marginals(ctx, name)
    return doc
