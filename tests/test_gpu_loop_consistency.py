"""csm_loop_consistency on the device against csm_host_loop_consistency: every byte of every output, on the cases
and the M ladder of the CPU test (63 / 64 / 65 and 127 / 128 / 129: the edges of the ballot's word and of the
bitset; 200: several workgroups and a ragged last word); repeated calls, scratch growth, the resident state of
the pose-graph entries, the C++ adapter, and the chain into the optimizer."""
import math
import os
import subprocess

import numpy as np
import pytest

from csm_hip import api
import loop_consistency_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _call(fn, c, edges=None, gate=None, n_seeds=0, want_chi2=True, **kw):
    args = dict(R.drift_args(c))
    args.update(kw)
    return fn(c["local"], c["scan"], c["edges"] if edges is None else edges, c["gate"] if gate is None else gate,
              n_seeds=n_seeds, want_adjacency=True, want_chi2=want_chi2, **args)


def _same(got, want):
    assert sorted(got) == sorted(want)
    if "chi2" in want:
        assert got["chi2"].shape == want["chi2"].shape and got["chi2"].tobytes() == want["chi2"].tobytes()
    assert got["adjacency"].tobytes() == want["adjacency"].tobytes()
    assert got["degree"].tobytes() == want["degree"].tobytes()
    assert got["selected"].tobytes() == want["selected"].tobytes()
    assert got["info"] == want["info"]


def _agree(ctx, c, **kw):
    """The device's outputs are the host function's, byte for byte; returns them."""
    got = _call(ctx.loop_consistency, c, **kw)
    _same(got, _call(api.host_loop_consistency, c, **kw))
    return got


@pytest.mark.parametrize("name", [n for n in R.CASES if n != "ladder"])
def test_device_is_the_host_function(gpu_ctx, name):
    c = R.case(name)
    out = _agree(gpu_ctx, c)
    assert out["info"]["clique_size"] == int(out["selected"].sum()) >= 1
    if name == "bad_pivot":
        assert out["info"]["bad_pivots"] == 13 and np.isinf(out["chi2"][2, 0])
    if name == "drift":
        off = _agree(gpu_ctx, c, drift_var_per_metre=None, local_travel=None, scan_travel=None)
        assert off["info"]["clique_size"] == 2 and out["info"]["clique_size"] == 3


@pytest.mark.parametrize("m", R.LADDER)
def test_device_is_the_host_function_over_the_ladder(gpu_ctx, m):
    c = R.case("ladder")
    for n_seeds in (0, 1, 3):
        out = _agree(gpu_ctx, c, edges=c["edges"][:m], n_seeds=n_seeds)
        assert out["info"]["seeds_run"] == (n_seeds if 0 < n_seeds < m else m)
    if m >= 63:
        assert 0 < out["info"]["consistent_pairs"] < m * (m - 1) // 2


def test_gates_zero_and_infinity(gpu_ctx):
    c = R.case("ladder")
    e = c["edges"][:129]
    zero = _agree(gpu_ctx, c, edges=e, gate=0.0)
    assert zero["info"]["clique_size"] == 1 and zero["info"]["winning_seed"] == 0
    inf = _agree(gpu_ctx, c, edges=e, gate=math.inf)
    assert inf["selected"].all() and inf["info"]["consistent_pairs"] == 129 * 128 // 2
    assert not (int(inf["adjacency"][0, 2]) >> 1)           # lanes past M give zero bits


def test_two_calls_give_the_same_bytes(gpu_ctx):
    c = R.case("ladder")
    a = _call(gpu_ctx.loop_consistency, c, n_seeds=5)
    b = _call(gpu_ctx.loop_consistency, c, n_seeds=5)
    _same(a, b)


def test_chi2_output_does_not_change_the_adjacency(gpu_ctx):
    c = R.case("ladder")
    e = c["edges"][:129]
    a = _call(gpu_ctx.loop_consistency, c, edges=e, n_seeds=2, want_chi2=True)
    b = _call(gpu_ctx.loop_consistency, c, edges=e, n_seeds=2, want_chi2=False)
    assert "chi2" not in b
    del a["chi2"]
    _same(a, b)
    plain = gpu_ctx.loop_consistency(c["local"], c["scan"], e, c["gate"], n_seeds=2)
    assert sorted(plain) == ["degree", "info", "selected"]
    assert plain["selected"].tobytes() == a["selected"].tobytes() and plain["info"] == a["info"]


def test_a_larger_call_after_a_smaller_one_grows_the_scratch():
    before = api.debug_live_bytes()
    ctx = api.Context(0)
    try:
        c = R.case("ladder")
        _agree(ctx, c, edges=c["edges"][:3])
        small = api.debug_live_bytes()
        _agree(ctx, c, n_seeds=4)
        held = api.debug_live_bytes()
        assert held[0] > small[0]
        _agree(ctx, c, edges=c["edges"][:64])
        assert api.debug_live_bytes() == held       # the smaller call fits the larger one's workspaces
    finally:
        ctx.close()
    assert api.debug_live_bytes() == before


def test_pose_graph_entries_are_unharmed(gpu_ctx):
    g = R.end_to_end_graph()
    edges = g["odometry"] + [e for e, bad in zip(g["loops"], g["outlier"]) if not bad]
    pairs = [(0, 40), (1, 55), (2, 59)]

    def both():
        lp, sp, info = gpu_ctx.pose_graph_lm(g["local"], g["scan"], edges, 1e-4, solver="SchurCholesky",
                                             loss="Squared", iterations_max=4)
        recs, minfo = gpu_ctx.pose_graph_marginals(g["local"], g["scan"], edges, pairs, loss="Squared")
        return lp.tobytes(), sp.tobytes(), info, [r["relative_cov"].tobytes() for r in recs], minfo

    first = both()
    c = R.case("ladder")
    _agree(gpu_ctx, c, edges=c["edges"][:129], n_seeds=3)
    assert both() == first
    _agree(gpu_ctx, c, edges=c["edges"][:129], n_seeds=3)


def test_refusal_carries_its_reason_and_leaves_the_context_usable(gpu_ctx):
    c = R.case("separated")
    for kw, word in ((dict(gate=-1.0), "gate"), (dict(n_seeds=-1), "n_seeds"),
                     (dict(edges=[dict(c["edges"][0], scan=120)]), "range"),
                     (dict(drift_var_per_metre=[1.0, 1.0, 1.0]), "together")):
        with pytest.raises(api.CsmError) as e:
            _call(gpu_ctx.loop_consistency, c, **kw)
        assert e.value.code == api.L.CSM_EINVAL and word in str(e.value)
    _agree(gpu_ctx, c)


def test_kernel_timers_count_the_chain(gpu_ctx):
    c = R.case("separated")
    gpu_ctx.enable_kernel_timing(True)
    try:
        gpu_ctx.reset_kernel_timing()
        _call(gpu_ctx.loop_consistency, c)
        whole = gpu_ctx.kernel_time("loop_consistency")
        pairs = gpu_ctx.kernel_time("loop_consistency_pairs")
        select = gpu_ctx.kernel_time("loop_consistency_select")
    finally:
        gpu_ctx.enable_kernel_timing(False)
    assert whole[1] == pairs[1] == select[1] == 1
    assert 0.0 < pairs[0] < whole[0] and 0.0 < select[0] < whole[0]


_CPP = r"""
#include <cstdio>
#include <vector>
#include "../my-lidar-graph-slam-v2_amd/host/csm_adapters.hpp"
using namespace CsmHip;
int main(int argc, char** argv)
{
    /* input: n_local n_scan n_edges n_seeds; gate (f64); local poses; scan poses; per edge local, scan (i32),
     * z[3], cov[9], info[9] (f64) */
    if (argc < 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    int hdr[4];
    double gate;
    if (!f || std::fread(hdr, 4, 4, f) != 4 || std::fread(&gate, 8, 1, f) != 1) return 2;
    std::vector<std::array<double, 3>> local(hdr[0]), scan(hdr[1]);
    if (std::fread(local.data(), 24, local.size(), f) != local.size() ||
        std::fread(scan.data(), 24, scan.size(), f) != scan.size()) return 2;
    LoopDetectionResultVector results(hdr[2]);
    std::vector<EdgePose> edges(hdr[2]);
    for (int i = 0; i < hdr[2]; ++i) {
        int ids[2];
        double v[21];
        if (std::fread(ids, 4, 2, f) != 2 || std::fread(v, 8, 21, f) != 21) return 2;
        LoopDetectionResult& r = results[i];
        r.mRelativePose = RobotPose2D<double> { v[0], v[1], v[2] };
        r.mLocalMapNodeId = (std::uint64_t)ids[0];
        r.mScanNodeId = ids[1];
        r.mScoreValue = (double)i;
        for (int q = 0; q < 9; ++q) r.mEstimatedCovariance[q] = v[3 + q];
        EdgePose& e = edges[i];
        e.mIsLoopConstraint = true;
        e.mLocalMapNodeIdx = ids[0];
        e.mScanNodeIdx = ids[1];
        for (int q = 0; q < 3; ++q) e.mRelativePose[q] = v[q];
        for (int q = 0; q < 9; ++q) e.mInformationMat[q] = v[12 + q];
    }
    std::fclose(f);
    auto checker = LoopConsistencyHIP::Create(gate, hdr[3]);
    if (!checker || LoopConsistencyHIP::Create(-1.0)) return 3;
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 0) checker->Check(local, scan, results); else checker->Check(local, scan, edges);
        std::fwrite(checker->Selected().data(), 4, checker->Selected().size(), o);
        std::fwrite(checker->Degree().data(), 4, checker->Degree().size(), o);
        std::fwrite(&checker->LastInfo(), sizeof(csm_loop_consistency_info), 1, o);
    }
    const LoopDetectionResultVector kept = checker->SelectConsistent(results);
    const int n = (int)kept.size();
    std::fwrite(&n, 4, 1, o);
    for (const LoopDetectionResult& r : kept) std::fwrite(&r.mScoreValue, 8, 1, o);
    std::fclose(o);
    return 0;
}
"""


def test_cpp_adapter_gives_the_python_side_s_records(gpu_ctx, tmp_path):
    src, exe = tmp_path / "consistency.cpp", tmp_path / "consistency"
    src.write_text(_CPP.replace("../my-lidar-graph-slam-v2_amd", os.path.join(ROOT, "my-lidar-graph-slam-v2_amd")))
    csrc = os.path.join(ROOT, "my-lidar-graph-slam-v2_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L" + csrc, "-lcsm_hip", "-Wl,-rpath," + csrc])
    c = R.case("separated")
    cov = np.diag(R.SIGMA ** 2)
    edges = api.loop_edges_from_matches([dict(local=e["local"], scan=e["scan"], pose=e["rel"], covariance=cov)
                                         for e in c["edges"]])
    m, n_seeds = len(edges), 6
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([len(c["local"]), len(c["scan"]), m, n_seeds], np.int32).tobytes())
        f.write(np.array([c["gate"]]).tobytes())
        f.write(np.ascontiguousarray(c["local"]).tobytes())
        f.write(np.ascontiguousarray(c["scan"]).tobytes())
        for e in edges:
            f.write(np.array([e["local"], e["scan"]], np.int32).tobytes())
            f.write(np.concatenate([e["rel"], cov.reshape(9), np.asarray(e["info"]).reshape(9)]).tobytes())
    subprocess.check_call([str(exe), str(inp), str(outp)], timeout=120)
    blob = outp.read_bytes()
    want = gpu_ctx.loop_consistency(c["local"], c["scan"], edges, c["gate"], n_seeds=n_seeds)
    info = api.L.LoopConsistencyInfo(want["info"]["consistent_pairs"], want["info"]["bad_pivots"],
                                     want["info"]["clique_size"], want["info"]["winning_seed"],
                                     want["info"]["seeds_run"], 0)
    one = want["selected"].tobytes() + want["degree"].tobytes() + bytes(info)
    assert len(one) == 8 * m + 32 and blob[:2 * len(one)] == one + one
    at = 2 * len(one)
    n = int(np.frombuffer(blob, np.int32, 1, at)[0])
    kept = np.frombuffer(blob, np.float64, n, at + 4)
    assert kept.tolist() == np.flatnonzero(want["selected"]).astype(float).tolist()      # in their original order
    assert n == 30 and want["selected"].tolist() == (~c["outlier"]).astype(int).tolist()


def _optimized(lm, g, loops):
    lp, sp, info = lm(g["local"], g["scan"], g["odometry"] + loops, 1e-4, solver="SchurCholesky", loss="Squared",
                      iterations_max=10)
    return info["final_error"], R.position_error(sp, g["truth"])


def test_selected_edges_give_the_better_graph(gpu_ctx):
    g = R.end_to_end_graph()
    args = (g["local"], g["scan"], g["loops"], g["gate"], g["drift"], g["local_travel"], g["scan_travel"])
    # on the host functions first
    host = api.host_loop_consistency(*args)
    assert host["selected"].tolist() == (~g["outlier"]).astype(int).tolist()
    kept = [e for e, s in zip(g["loops"], host["selected"]) if s]
    err_kept, far_kept = _optimized(api.host_pose_graph_lm, g, kept)
    err_all, far_all = _optimized(api.host_pose_graph_lm, g, g["loops"])
    assert err_kept < err_all and far_kept < far_all
    assert far_kept < R.position_error(g["scan"], g["truth"])          # and better than not closing the loops
    # then on the device
    dev = gpu_ctx.loop_consistency(*args)
    assert dev["selected"].tobytes() == host["selected"].tobytes() and dev["info"] == host["info"]
    kept = [e for e, s in zip(g["loops"], dev["selected"]) if s]
    err_kept, far_kept = _optimized(gpu_ctx.pose_graph_lm, g, kept)
    err_all, far_all = _optimized(gpu_ctx.pose_graph_lm, g, g["loops"])
    assert err_kept < err_all and far_kept < far_all
