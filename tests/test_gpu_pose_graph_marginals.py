"""csm_pose_graph_marginals on the device against the host restatement csm_host_pose_graph_marginals, which
tests/test_cpu_pose_graph_marginals.py pins to the Python literal bit for bit.

The device runs the host's arithmetic in the host's order (the elimination, the blocked LDL^T, every
column's substitutions, the pair formulas); it differs only through the device library's sin / cos, a
rounding-level perturbation of H that the conditioning of S amplifies as it amplifies the literal's own
rounding. Bound, fixed before any device run: 100 x the literal-against-numpy figure of the same case
(LITERAL_ERROR in pose_graph_marginals_cases.py), in the measure |delta_ij| / sqrt(Sigma_ii Sigma_jj).

Shapes: 3 n_local = 3 (one local map, n_scan = 0), 48 (exactly one tile), 51 (padded to 96: columns in
the padded tile), 99 and 147 (three and four tiles); pairs with s adjacent to t, not adjacent, s = 0 and
scan_index = -1; scan nodes of degree 1, 2, 3 and about n_local / 2; |C| = 1, n_local, and 15 / 16 / 17
around the kernels' column-group width of 16."""
import os
import subprocess

import numpy as np
import pytest

from csm_hip import _lib as L
from csm_hip import api
import pose_graph_cases as PC
import pose_graph_marginals_cases as MC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("alone", "one"), ("one_local", "mixed"), ("plain16", "mixed"), ("plain16", "all"), ("plain17", "mixed"),
         ("plain17", "c15"), ("plain17", "c16"), ("plain17", "all"), ("plain33", "mixed"), ("plain33", "one"),
         ("plain33", "all"), ("dense33", "mixed"), ("plain49", "mixed"), ("plain49", "all"), ("dense49", "mixed"),
         ("dup33", "mixed"), ("wrapped33", "mixed")]
IDS = ["%s-%s" % c for c in CASES]


def _args(name, kind):
    c = MC.graph(name)
    return c["local"], c["scan"], c["edges"], MC.pairs(name, kind)


def _difference(dev, host, name, kind):
    """|device - host| in the cases' measure: the yardstick only supplies the scale"""
    delta = [{k: np.asarray(a[k]) - np.asarray(b[k]) for k in MC.BLOCKS} for a, b in zip(dev, host)]
    zero = [{k: np.zeros((3, 3)) for k in MC.BLOCKS} for _ in dev]
    want = MC.expected(name, kind)
    shifted = [{k: d[k] + w.get(k, z[k]) for k in MC.BLOCKS} for d, w, z in zip(delta, want, zero)]
    return MC.error(shifted, name, kind)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_marginals_match_the_host(gpu_ctx, case):
    name, kind = case
    assert 3 * len(MC.graph("plain16")["local"]) == 48 and 3 * len(MC.graph("plain17")["local"]) == 51
    dev, dinfo = gpu_ctx.pose_graph_marginals(*_args(name, kind))
    host, hinfo = api.host_pose_graph_marginals(*_args(name, kind))
    assert dinfo == hinfo
    assert [r["finite"] for r in dev] == [r["finite"] for r in host]
    diff = _difference(dev, host, name, kind)
    print("device - host", diff, "bound", MC.bound(name, kind, 100.0), "bit-equal", MC.same_bits(dev, host))
    assert diff <= MC.bound(name, kind, 100.0)
    for (s, t), r in zip(MC.pairs(name, kind), dev):
        for k in ("local_cov", "scan_cov", "relative_cov"):
            assert np.array_equal(r[k], r[k].T)
        if t is None:
            assert not r["scan_cov"].any() and not r["cross_cov"].any() and not r["relative_cov"].any()


def test_column_group_widths_are_what_the_cases_say(gpu_ctx):
    for kind, n in (("c15", MC.GROUP - 1), ("c16", MC.GROUP), ("all", MC.GROUP + 1), ("one", 1)):
        name = "plain33" if kind == "one" else "plain17"
        assert gpu_ctx.pose_graph_marginals(*_args(name, kind))[1]["n_columns"] == n


@pytest.mark.parametrize("name", ["plain17", "dense33", "plain49"])
def test_a_pair_alone_among_all_and_reversed_has_the_same_bits(gpu_ctx, name):
    local, scan, edges, pairs = _args(name, "mixed")
    whole, _ = gpu_ctx.pose_graph_marginals(local, scan, edges, pairs)
    back, _ = gpu_ctx.pose_graph_marginals(local, scan, edges, pairs[::-1])
    assert MC.same_bits(whole, back[::-1])
    everything, _ = gpu_ctx.pose_graph_marginals(local, scan, edges, pairs + MC.pairs(name, "all"))
    assert MC.same_bits(whole, everything[:len(pairs)])
    for q in (0, 1, 2, 3, 4, len(pairs) - 2, len(pairs) - 1):
        alone, _ = gpu_ctx.pose_graph_marginals(local, scan, edges, [pairs[q]])
        assert MC.same_bits(alone, whole[q:q + 1])


def test_two_calls_agree_and_sizes_alternate_on_one_context(gpu_ctx):
    big, small = _args("plain49", "all"), _args("plain16", "mixed")
    first, _ = gpu_ctx.pose_graph_marginals(*big)
    assert MC.same_bits(first, gpu_ctx.pose_graph_marginals(*big)[0])
    little, _ = gpu_ctx.pose_graph_marginals(*small)
    assert MC.same_bits(first, gpu_ctx.pose_graph_marginals(*big)[0])
    assert MC.same_bits(little, gpu_ctx.pose_graph_marginals(*small)[0])


@pytest.mark.parametrize("solver", ["ConjugateGradient", "SchurCholesky"])
def test_pose_graph_lm_keeps_its_bits_around_a_marginals_call(solver):
    c = MC.graph("plain33")
    fresh = api.Context(0)
    try:
        want = fresh.pose_graph_lm(c["local"], c["scan"], c["edges"], 1e-4, solver=solver)
    finally:
        fresh.close()
    ctx = api.Context(0)
    try:
        before = ctx.pose_graph_lm(c["local"], c["scan"], c["edges"], 1e-4, solver=solver)
        ctx.pose_graph_marginals(*_args("plain49", "all"))
        ctx.pose_graph_marginals(*_args("plain33", "mixed"))
        after = ctx.pose_graph_lm(c["local"], c["scan"], c["edges"], 1e-4, solver=solver)
    finally:
        ctx.close()
    for got in (before, after):
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        assert got[2] == want[2]


def test_refusals_carry_their_reason(gpu_ctx):
    c = MC.graph("plain16")
    nl = len(c["local"])
    idle, lone = PC.case(40, "idle_local_appended"), PC.case(40, "isolated")
    for graph, pairs, why in ((c, [], "n_pairs"), (c, [(nl, None)], "out of range"), (c, [(0, len(c["scan"]))], "out of range"),
                              (idle, [(0, None)], "not connected"), (lone, [(0, lone["isolated_scans"][0])], "without edges")):
        with pytest.raises(api.CsmError) as ex:
            gpu_ctx.pose_graph_marginals(graph["local"], graph["scan"], graph["edges"], pairs)
        assert ex.value.code == L.CSM_EINVAL and why in str(ex.value), str(ex.value)
    dev, _ = gpu_ctx.pose_graph_marginals(lone["local"], lone["scan"], lone["edges"], [(0, 0), (1, None)])
    assert all(r["finite"] for r in dev)


def test_optimizer_wrapper_gives_the_plain_call(gpu_ctx):
    c = MC.graph("plain17")
    opt = api.PoseGraphOptimizerLMHIP("SchurCholesky", loss="Cauchy", loss_scale=0.05, ctx=gpu_ctx)
    lp, sp = opt.optimize(c["local"], c["scan"], c["edges"])
    pairs = MC.pairs("plain17", "mixed")
    got = opt.marginals(lp, sp, c["edges"], pairs)
    want, _ = gpu_ctx.pose_graph_marginals(lp, sp, c["edges"], pairs, loss="Cauchy", loss_scale=0.05)
    assert MC.same_bits(got, want)
    other, _ = gpu_ctx.pose_graph_marginals(lp, sp, c["edges"], pairs)       # Huber 0.01: another weight
    assert not MC.same_bits(got, other)


_CPP = r"""
#include <cstdio>
#include <vector>
#include "../my-lidar-graph-slam-v2_amd/host/csm_adapters.hpp"
using namespace CsmHip;
int main(int argc, char** argv)
{
    /* input: n_local n_scan n_edges n_pairs; local, scan poses; csm_pose_graph_edge records; pairs (2 x i32) */
    if (argc < 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    int hdr[4];
    if (!f || std::fread(hdr, 4, 4, f) != 4) return 2;
    std::vector<std::array<double, 3>> local(hdr[0]), scan(hdr[1]);
    std::vector<csm_pose_graph_edge> raw(hdr[2]);
    std::vector<NodePair> pairs(hdr[3]);
    if (std::fread(local.data(), 24, local.size(), f) != local.size() ||
        std::fread(scan.data(), 24, scan.size(), f) != scan.size() ||
        std::fread(raw.data(), sizeof(csm_pose_graph_edge), raw.size(), f) != raw.size() ||
        std::fread(pairs.data(), 8, pairs.size(), f) != pairs.size()) return 2;
    std::fclose(f);
    std::vector<EdgePose> edges(raw.size());
    for (std::size_t i = 0; i < raw.size(); ++i) {
        edges[i].mIsLoopConstraint = raw[i].is_loop != 0;
        edges[i].mLocalMapNodeIdx = raw[i].local_map_index;
        edges[i].mScanNodeIdx = raw[i].scan_index;
        for (int j = 0; j < 3; ++j) edges[i].mRelativePose[j] = raw[i].relative_pose[j];
        for (int j = 0; j < 9; ++j) edges[i].mInformationMat[j] = raw[i].information[j];
    }
    auto opt = PoseGraphOptimizerLMHIP::Create(PoseGraphOptimizerLMHIP::SolverType::SchurCholesky, 10, 1e-4, 1e-4,
                                               CSM_PG_LOSS_HUBER, 0.01);
    if (!opt) return 3;
    const std::vector<PairMarginal> got = opt->ComputeMarginals(local, scan, edges, pairs);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    for (const PairMarginal& m : got) {
        std::fwrite(m.localCov.data(), 8, 9, o);
        std::fwrite(m.scanCov.data(), 8, 9, o);
        std::fwrite(m.crossCov.data(), 8, 9, o);
        std::fwrite(m.relativeCov.data(), 8, 9, o);
        const double fin = m.finite ? 1.0 : 0.0;
        std::fwrite(&fin, 8, 1, o);
    }
    /* the free functions on the last pair's record */
    std::array<double, 3> ranges {};
    std::array<double, 9> match {};
    match[0] = match[4] = 1e-4;
    match[8] = 1e-5;
    double chi2 = -1.0;
    const bool ok = LoopSearchRanges(got.back().relativeCov, 3.0, { 0.1, 0.1, 0.01 }, { 2.5, 2.5, 0.5 }, ranges) &&
                    LoopGate(got.back().relativeCov, match, { 1.0, 2.0, 0.1 }, { 1.02, 1.97, 0.12 }, chi2);
    const double tail[5] = { ok ? 1.0 : 0.0, ranges[0], ranges[1], ranges[2], chi2 };
    std::fwrite(tail, 8, 5, o);
    std::fclose(o);
    return 0;
}
"""


def test_cpp_adapter_gives_the_python_binding_s_bits(gpu_ctx, tmp_path):
    src, exe = tmp_path / "marginals.cpp", tmp_path / "marginals"
    src.write_text(_CPP.replace("../my-lidar-graph-slam-v2_amd", os.path.join(ROOT, "my-lidar-graph-slam-v2_amd")))
    csrc = os.path.join(ROOT, "my-lidar-graph-slam-v2_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L" + csrc, "-lcsm_hip", "-Wl,-rpath," + csrc])
    local, scan, edges, pairs = _args("plain17", "mixed")
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([len(local), len(scan), len(edges), len(pairs)], np.int32).tobytes())
        f.write(np.ascontiguousarray(local, np.float64).tobytes())
        f.write(np.ascontiguousarray(scan, np.float64).tobytes())
        f.write(bytes(api.pose_graph_edges(edges))[:len(edges) * 112])
        f.write(np.array([[s, -1 if t is None else t] for s, t in pairs], np.int32).tobytes())
    subprocess.check_call([str(exe), str(inp), str(outp)], timeout=120)
    blob = np.frombuffer(outp.read_bytes(), np.float64)
    assert blob.size == 37 * len(pairs) + 5
    want, _ = gpu_ctx.pose_graph_marginals(local, scan, edges, pairs)
    for q, r in enumerate(want):
        rec = blob[37 * q:37 * q + 37]
        flat = np.concatenate([r[k].ravel() for k in MC.BLOCKS])
        assert rec[:36].tobytes() == flat.tobytes() and rec[36] == float(r["finite"])
    tail = blob[37 * len(pairs):]
    rel = want[-1]["relative_cov"]
    match = np.diag([1e-4, 1e-4, 1e-5])
    assert tail[0] == 1.0
    assert tail[1:4].tolist() == api.host_loop_search_ranges(rel, 3.0, [0.1, 0.1, 0.01], [2.5, 2.5, 0.5]).tolist()
    assert tail[4] == api.host_loop_gate(rel, match, [1.0, 2.0, 0.1], [1.02, 1.97, 0.12])
