"""csm_loop_search on the device against csm_host_loop_search: every byte of records, counts and info, at the
smallest shapes at which the kernel can go wrong; the Python and C++ LoopSearcherNearestHIP; the chain into
pose_graph_marginals."""
import os
import subprocess

import numpy as np
import pytest

from csm_hip import api
import loop_search_cases as LC
import loop_search_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 2, 16)


def _args(c, q, qt, k, one_per_map, n_ref=None):
    return (c["poses"], c["map_index"], c["travel"], q, qt, n_ref, c["travel_dist_threshold"],
            c["node_dist_threshold"], k, one_per_map)


def _agree(ctx, c, q, qt, k, one_per_map, n_ref=None):
    """The device's records, counts and info are the host function's, byte for byte; returns them."""
    args = _args(c, np.asarray(q, np.int32), np.asarray(qt, np.float64), k, one_per_map, n_ref)
    rec, counts, info = ctx.loop_search(*args)
    hrec, hcounts, hinfo = api.host_loop_search(*args)
    assert rec.shape == hrec.shape and rec.tobytes() == hrec.tobytes()
    assert counts.tobytes() == hcounts.tobytes()
    assert info == hinfo
    return rec, counts, info


@pytest.mark.parametrize("one_per_map", (False, True))
@pytest.mark.parametrize("name", LC.FAMILIES)
def test_device_search_is_the_host_search(gpu_ctx, name, one_per_map):
    c = LC.family(name)
    q, qt = LC.all_queries(c)
    for k in KS:
        rec, counts, info = _agree(gpu_ctx, c, q, qt, k, one_per_map)
        assert 1 <= counts.max() <= k and (one_per_map or counts.max() == k)
        assert counts.min() == 0 and info["pairs_eligible"] > 0


def test_far_frame_records_are_the_laps_records(gpu_ctx):
    a, b = LC.family("laps"), LC.family("far_frame")
    q, qt = LC.all_queries(a)
    ra, ca, ia = gpu_ctx.loop_search(*_args(a, q, qt, 16, False))
    rb, cb, ib = gpu_ctx.loop_search(*_args(b, q, qt, 16, False))
    assert ra.tobytes() == rb.tobytes() and ca.tobytes() == cb.tobytes() and ia == ib


def _truncated_laps(n_ref):
    """Reference nodes [0, n_ref) of laps repeated to 1 000 nodes; the queries lie behind them."""
    base = LC.family("laps")["poses"]
    poses = np.concatenate([base, base, base])[:1100]
    sizes = [10] * 110
    return LC._finish(poses, sizes, 10.0, 2.0)


@pytest.mark.parametrize("n_ref", (0, 1, 63, 64, 65, 255, 256, 257, 1000))
def test_reference_counts_at_the_wave_and_block_edges(gpu_ctx, n_ref):
    c = _truncated_laps(n_ref)
    assert len(c["poses"]) == 1100
    rng = np.random.default_rng(n_ref)
    pool = np.arange(1000, 1100, dtype=np.int32)          # behind every reference node
    everywhere = rng.permutation(1100).astype(np.int32)
    total = 0
    for n_q, q in ((1, pool[:1]), (2, pool[5:7]), (300, everywhere[:300])):
        qt = c["travel"][q] if n_q == 300 else np.full(n_q, c["travel"][-1])
        for k in KS:
            for one_per_map in (False, True):
                _, counts, info = _agree(gpu_ctx, c, q, qt, k, one_per_map, n_ref)
                total += int(counts.sum())
                if n_q < 300:       # the gate is open: the prefix is all of n_ref
                    assert info["pairs_evaluated"] == n_q * n_ref
    assert total == 0 if n_ref == 0 else (total > 0 or n_ref < 63)


def test_empty_and_full_prefixes(gpu_ctx):
    c = LC.family("laps")
    n = len(c["poses"])
    q = np.array([383, 200, 100], np.int32)
    # travel 0: no reference node passes the gate; travel far ahead: all of n_ref do
    qt = np.array([0.0, c["travel"][-1] + 100.0, 9.99])
    rec, counts, info = _agree(gpu_ctx, c, q, qt, 16, False)
    assert counts.tolist()[0] == 0 and counts[1] > 0 and counts[2] == 0
    assert info["pairs_evaluated"] == n             # 0 + n + 0: node 0 (travel 0) fails 9.99 - 0 < 10
    assert rec[0]["ref_scan_index"].tolist() == [-1] * 16 and rec[0]["query_scan_index"].tolist() == [383] * 16


@pytest.mark.parametrize("k", KS)
def test_eligible_counts_of_exactly_k_and_one_less(gpu_ctx, k):
    c = LC.family("laps")
    q_all, qt_all = LC.all_queries(c)
    qi = LC.laps_properties(16)["more"]
    # the eligible reference nodes of one query on the third lap; a reference limit just behind the
    # want-th of them (by index) leaves exactly `want`
    refs = np.sort(R.eligible(c["poses"], c["map_index"], c["travel"], len(q_all), qi, qt_all[qi],
                              c["travel_dist_threshold"], c["node_dist_threshold"])[1])
    assert refs.size > 16
    for want in (k, k - 1):
        n_ref = int(refs[want - 1]) + 1 if want else int(refs[0])
        for one_per_map in (False, True):
            rec, counts, info = _agree(gpu_ctx, c, [qi], [qt_all[qi]], k, one_per_map, n_ref)
            assert info["pairs_eligible"] == want
            if not one_per_map:
                assert counts[0] == want


def test_one_identical_pose_orders_by_index(gpu_ctx):
    c = LC.one_pose_graph(300)
    for k in KS:
        rec, counts, info = _agree(gpu_ctx, c, [300], [100.0], k, False, 300)
        assert rec[0]["ref_scan_index"].tolist() == list(range(k)) and info["pairs_eligible"] == 300
        assert set(rec[0]["dist_sq"].tolist()) == {1.0}
        rec, counts, _ = _agree(gpu_ctx, c, [300], [100.0], k, True, 300)
        assert rec[0]["ref_scan_index"].tolist() == [7 * j for j in range(k)]


@pytest.mark.parametrize("n_ref", (1023, 1024, 1025, 3000))
def test_eligible_pairs_around_the_lds_list_s_capacity(gpu_ctx, n_ref):
    """Up to 1 024 eligible pairs of a query are kept in LDS; above that every record walks the prefix."""
    for c in (LC.dense_cloud_graph(n_ref), LC.one_pose_graph(n_ref)):
        for k in KS:
            for one_per_map in (False, True):
                rec, counts, info = _agree(gpu_ctx, c, [n_ref], [100.0], k, one_per_map, n_ref)
                assert info["pairs_eligible"] == n_ref and counts[0] == k
    # a second query whose gate closes after about 500 nodes rides along in the same launch
    c = LC.dense_cloud_graph(n_ref)
    gate = float(c["travel"][499]) + 10.0
    short = R.prefix_length(c["travel"], n_ref, gate, 10.0)
    assert 490 < short < 510
    rec, counts, info = _agree(gpu_ctx, c, [n_ref, 3], [100.0, gate], 16, False, n_ref)
    assert info["pairs_evaluated"] == n_ref + short


@pytest.mark.parametrize("n_maps", (33, 65))
def test_maps_at_the_edges_of_the_bitset_words(gpu_ctx, n_maps):
    c = LC.word_edge_graph(n_maps)
    q, qt = np.array([0], np.int32), np.array([0.0])
    rec, counts, _ = _agree(gpu_ctx, c, q, qt, 16, True)
    assert counts[0] == 16
    maps = rec[0]["ref_map_index"].tolist()
    assert maps[:len(c["edge_maps"])] == c["edge_maps"] and len(set(maps)) == 16
    assert {31, 32, n_maps - 1} <= set(maps) and (n_maps < 65 or {63, 64} <= set(maps))
    assert np.all(rec[0]["ref_scan_index"] % 2 == 0)            # the nearer node of each map
    every = np.arange(2 * n_maps, dtype=np.int32)
    _agree(gpu_ctx, c, every, np.zeros(every.size), 16, True)
    _agree(gpu_ctx, c, every, np.zeros(every.size), 2, False)


def test_query_order_moves_rows_and_nothing_else(gpu_ctx):
    c = LC.family("random_walk")
    q, qt = LC.all_queries(c)
    base, bcounts, binfo = _agree(gpu_ctx, c, q, qt, 2, True)
    rng = np.random.default_rng(11)
    for order in (q[::-1].copy(), rng.permutation(q).astype(np.int32)):
        rec, counts, info = _agree(gpu_ctx, c, order, c["travel"][order], 2, True)
        assert rec.tobytes() == base[order].tobytes() and counts.tobytes() == bcounts[order].tobytes()
        assert info == binfo


def test_a_larger_then_a_smaller_call_and_the_memory_goes_back():
    before = api.debug_live_bytes()
    ctx = api.Context(0)
    try:
        big, small = LC.family("random_walk"), LC.family("laps")
        q, qt = LC.all_queries(big)
        _agree(ctx, big, q, qt, 16, True)
        held = api.debug_live_bytes()
        s, st = LC.all_queries(small)
        first, fcounts, finfo = _agree(ctx, small, s[300:320], st[300:320], 2, False)
        assert api.debug_live_bytes() == held           # the smaller call fits the larger one's workspaces
        fresh = api.Context(0)
        try:
            again, acounts, ainfo = fresh.loop_search(*_args(small, s[300:320], st[300:320], 2, False))
        finally:
            fresh.close()
        assert first.tobytes() == again.tobytes() and fcounts.tobytes() == acounts.tobytes() and finfo == ainfo
    finally:
        ctx.close()
    assert api.debug_live_bytes() == before


def test_refusals_carry_their_reason(gpu_ctx):
    c = LC.family("laps")
    q, qt = LC.all_queries(c)
    for change, word in ((dict(k=0), "n_per_query"), (dict(k=17), "n_per_query"), (dict(n_ref=385), "n_ref"),
                         (dict(q=np.array([3, 3], np.int32)), "repeated"), (dict(q=np.array([384], np.int32)), "range")):
        qq = change.get("q", q[:4])
        with pytest.raises(api.CsmError) as e:
            gpu_ctx.loop_search(*_args(c, qq, c["travel"][np.minimum(qq, 383)], change.get("k", 2), False,
                                       change.get("n_ref")))
        assert word in str(e.value)
    bad = c["poses"].copy()
    bad[17, 1] = np.nan
    with pytest.raises(api.CsmError) as e:
        gpu_ctx.loop_search(bad, c["map_index"], c["travel"], q[:4], qt[:4])
    assert "finite" in str(e.value)
    _agree(gpu_ctx, c, q[:4], qt[:4], 2, False)         # a refused call leaves the context usable


def test_kernel_timer_counts_the_launch(gpu_ctx):
    c = LC.family("laps")
    q, qt = LC.all_queries(c)
    gpu_ctx.enable_kernel_timing(True)
    try:
        gpu_ctx.reset_kernel_timing()
        gpu_ctx.loop_search(*_args(c, q, qt, 2, False))
        ms, launches = gpu_ctx.kernel_time("loop_search")
    finally:
        gpu_ctx.enable_kernel_timing(False)
    assert launches == 1 and ms > 0.0


@pytest.mark.parametrize("name", LC.FAMILIES)
def test_python_searcher_is_the_reference_s_walk(gpu_ctx, name):
    c = LC.family(name)
    for k in KS:
        searcher = api.LoopSearcherNearestHIP(c["travel_dist_threshold"], c["node_dist_threshold"], k, ctx=gpu_ctx)
        for last in (len(c["runs"]) - 1, len(c["runs"]) // 2):
            accum = float(c["travel"][c["runs"][last][1]])
            got = searcher.search(c["poses"], c["runs"], accum, last)
            walk = R.reference_walk(c["poses"], c["runs"], accum, last, c["travel_dist_threshold"],
                                    c["node_dist_threshold"])
            assert set(got) == {(qq, rr, mm) for _, rr, qq, mm in walk[:k]} and len(got) == min(k, len(walk))
            assert searcher.last_metrics["NodeDist"] == [w[0] for w in walk[:k]]
            assert searcher.last_metrics["NumOfCandidateNodes"] == len(got)


def test_python_search_per_map(gpu_ctx):
    c = LC.family("laps")
    searcher = api.LoopSearcherNearestHIP(10.0, 2.0, 2, ctx=gpu_ctx)
    nodes = [383, 200, 5, 310]
    got = searcher.search_per_map(c["poses"], c["runs"], len(c["runs"]) - 1, nodes, 8)
    rec, counts, _ = api.host_loop_search(c["poses"], c["map_index"], c["travel"], nodes, None, None, 10.0, 2.0, 8, True)
    want = [(int(r["query_scan_index"]), int(r["ref_scan_index"]), int(r["ref_map_index"]))
            for row, n in zip(rec, counts) for r in row[:n]]
    assert got == want and len(got) > 8


_CPP = r"""
#include <cstdio>
#include <vector>
#include "../my-lidar-graph-slam-v2_amd/host/csm_adapters.hpp"
using namespace CsmHip;
static void put(FILE* o, const LoopCandidateVector& v)
{
    const int n = (int)v.size();
    std::fwrite(&n, 4, 1, o);
    for (const LoopCandidate& c : v) {
        const int ids[3] = { c.mQueryScanNodeId, c.mReferenceScanNodeId, c.mReferenceLocalMapId };
        std::fwrite(ids, 4, 3, o);
        std::fwrite(&c.mDistSq, 8, 1, o);
    }
}
int main(int argc, char** argv)
{
    /* input: n_scan n_maps last k n_queries n_per_query; accum (f64); poses; runs (2 x i32); query nodes (i32) */
    if (argc < 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    int hdr[6];
    double accum;
    if (!f || std::fread(hdr, 4, 6, f) != 6 || std::fread(&accum, 8, 1, f) != 1) return 2;
    std::vector<std::array<double, 3>> poses(hdr[0]);
    std::vector<std::pair<int, int>> runs(hdr[1]);
    std::vector<int> nodes(hdr[4]);
    if (std::fread(poses.data(), 24, poses.size(), f) != poses.size() ||
        std::fread(runs.data(), 8, runs.size(), f) != runs.size() ||
        std::fread(nodes.data(), 4, nodes.size(), f) != nodes.size()) return 2;
    std::fclose(f);
    auto searcher = LoopSearcherNearestHIP::Create(10.0, 2.0, hdr[3]);
    if (!searcher) return 3;
    LoopSearchHintView hint;
    hint.mScanNodePoses = poses.data();
    hint.mNumOfScanNodes = poses.size();
    hint.mLocalMapNodeRanges = runs.data();
    hint.mNumOfLocalMaps = runs.size();
    hint.mAccumTravelDist = accum;
    hint.mLastFinishedMapId = hdr[2];
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const LoopCandidateVector found = searcher->Search(hint);
    put(o, found);
    int observed = 0;
    double dist = 0.0, count = -1.0, travel = -1.0;
    searcher->ReportMetrics([&](const std::string& id, double v) {
        ++observed;
        if (id == "LoopSearcherNearest.NodeDist") dist += v;
        if (id == "LoopSearcherNearest.NumOfCandidateNodes") count = v;
        if (id == "LoopSearcherNearest.AccumTravelDist") travel = v;
    });
    put(o, searcher->SearchPerMap(hint, nodes, hdr[5]));
    /* the helpers: pairs for ComputeMarginals, and a candidate's predicted map-local pose */
    const std::vector<NodePair> pairs = ToNodePairs(found);
    for (const NodePair& p : pairs) {
        const int ids[2] = { p.mLocalMapNodeIdx, p.mScanNodeIdx };
        std::fwrite(ids, 4, 2, o);
    }
    const RobotPose2D<double> local = MapLocalScanPose(poses[runs[found[0].mReferenceLocalMapId].first],
                                                       poses[found[0].mQueryScanNodeId]);
    const double tail[7] = { (double)observed, dist, count, travel, local.mX, local.mY, local.mTheta };
    std::fwrite(tail, 8, 7, o);
    std::fclose(o);
    return 0;
}
"""


def test_cpp_adapter_gives_the_python_side_s_records(gpu_ctx, tmp_path):
    src, exe = tmp_path / "loopsearch.cpp", tmp_path / "loopsearch"
    src.write_text(_CPP.replace("../my-lidar-graph-slam-v2_amd", os.path.join(ROOT, "my-lidar-graph-slam-v2_amd")))
    csrc = os.path.join(ROOT, "my-lidar-graph-slam-v2_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L" + csrc, "-lcsm_hip", "-Wl,-rpath," + csrc])
    c = LC.family("laps")
    last, k, nodes, per = len(c["runs"]) - 1, 16, [383, 200, 5, 310], 8
    accum = float(c["travel"][-1])
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([len(c["poses"]), len(c["runs"]), last, k, len(nodes), per], np.int32).tobytes())
        f.write(np.array([accum]).tobytes())
        f.write(c["poses"].tobytes())
        f.write(np.array(c["runs"], np.int32).tobytes())
        f.write(np.array(nodes, np.int32).tobytes())
    subprocess.check_call([str(exe), str(inp), str(outp)], timeout=120)
    blob = outp.read_bytes()
    lists, at = [], 0
    for _ in range(2):
        n = int(np.frombuffer(blob, np.int32, 1, at)[0])
        rows = np.frombuffer(blob, np.dtype([("ids", np.int32, 3), ("d", np.float64)]), n, at + 4)
        lists.append([(tuple(int(v) for v in r["ids"]), float(r["d"])) for r in rows])
        at += 4 + 20 * n
    searcher = api.LoopSearcherNearestHIP(10.0, 2.0, k, ctx=gpu_ctx)
    want = searcher.search(c["poses"], c["runs"], accum, last)
    assert len(want) == k and [t for t, _ in lists[0]] == want
    assert [d for _, d in lists[0]] == searcher.last_metrics["NodeDist"]
    assert [t for t, _ in lists[1]] == searcher.search_per_map(c["poses"], c["runs"], last, nodes, per)
    pairs = np.frombuffer(blob, np.int32, 2 * k, at).reshape(k, 2)
    assert pairs.tolist() == [[m, q] for q, _, m in want]
    tail = np.frombuffer(blob, np.float64, 7, at + 8 * k)
    assert tail[0] == k + 2 and tail[1] == sum(searcher.last_metrics["NodeDist"]) and tail[2] == k
    assert tail[3] == accum
    q0, _, m0 = want[0]
    assert tail[4:].tolist() == api.host_inverse_compound(c["poses"][c["runs"][m0][0]], c["poses"][q0]).tolist()


def test_candidates_chain_into_the_marginals(gpu_ctx):
    """The smallest chain: candidates of the laps family as pairs of pose_graph_marginals, each with its
    predicted mapLocalScanPose. Only that the calls accept what the helpers produce and that the pair
    indices are the candidates'."""
    c = LC.family("laps")
    last = 20
    poses = c["poses"][:c["runs"][last][1] + 1]
    local = np.array([poses[a] for a, _ in c["runs"][:last + 1]])
    info = np.diag([400.0, 400.0, 900.0])
    edges = []
    for m, (a, b) in enumerate(c["runs"][:last + 1]):
        for i in range(a, b + 1):
            edges.append(dict(local=m, scan=i, rel=api.host_inverse_compound(local[m], poses[i]), info=info))
        if m > 0:
            edges.append(dict(local=m - 1, scan=a, rel=api.host_inverse_compound(local[m - 1], poses[a]), info=info))
    searcher = api.LoopSearcherNearestHIP(10.0, 2.0, 4, ctx=gpu_ctx)
    cands = searcher.search(poses, c["runs"], float(c["travel"][len(poses) - 1]), last)
    assert len(cands) == 4
    pairs = [(m, q) for q, _, m in cands]
    predicted = [api.host_inverse_compound(local[m], poses[q]) for q, _, m in cands]
    recs, minfo = gpu_ctx.pose_graph_marginals(local, poses, edges, pairs)
    assert len(recs) == len(cands) and all(r["finite"] for r in recs)
    assert minfo["n_columns"] >= len({m for m, _ in pairs})
    for (q, r, m), (pm, pq), pred in zip(cands, pairs, predicted):
        assert (pm, pq) == (m, q) and c["map_index"][r] == m and c["map_index"][q] == last
        assert np.all(np.isfinite(pred))
        rng3 = api.host_loop_search_ranges(recs[0]["relative_cov"], 3.0, [0.1, 0.1, 0.01], [2.5, 2.5, 0.5])
        assert np.all(rng3 > 0)
