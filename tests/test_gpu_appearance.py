"""csm_scan_descriptors and csm_appearance_search on the device against their host functions: every byte of
descriptors, beams_used, records, counts and info, at the smallest shapes at which the kernels can go wrong; the
Python and C++ LoopSearcherAppearanceHIP; buffer ownership."""
import math
import os
import subprocess

import numpy as np
import pytest

from csm_hip import _lib as L, api
import appearance_cases as AC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 2, 16)
U32_MAX = 0xffffffff


def _descriptors_agree(ctx, angles, ranges, offsets, shape):
    d, used = ctx.scan_descriptors(angles, ranges, offsets, shape[0], shape[1], AC.RANGE_MIN, AC.RANGE_MAX)
    hd, hused = api.host_scan_descriptors(angles, ranges, offsets, shape[0], shape[1], AC.RANGE_MIN, AC.RANGE_MAX)
    assert d.shape == hd.shape and d.tobytes() == hd.tobytes() and used.tobytes() == hused.tobytes()
    return d, used


def _agree(ctx, c, q, qt=None, n_ref=None, max_distance=U32_MAX, min_cell_sum=0, k=2, one_per_map=False, thr=10.0):
    """The device's records, counts and info are the host function's, byte for byte; returns them."""
    args = (c["desc"], c["map_index"], c["travel"], np.asarray(q, np.int32), qt, n_ref, thr, max_distance,
            min_cell_sum, k, one_per_map)
    rec, counts, info = ctx.appearance_search(*args)
    hrec, hcounts, hinfo = api.host_appearance_search(*args)
    assert rec.shape == hrec.shape and rec.tobytes() == hrec.tobytes()
    assert counts.tobytes() == hcounts.tobytes()
    assert info == hinfo
    return rec, counts, info


# ---- descriptor build ----

@pytest.mark.parametrize("shape", ((3, 12), (20, 64), (32, 128)))
def test_beam_counts_at_the_wave_and_block_edges_in_one_ragged_call(gpu_ctx, shape):
    angles, ranges, offsets = AC.ragged([1, 63, 64, 65, 0, 1024, 1025, 65536], seed=shape[0])
    d, used = _descriptors_agree(gpu_ctx, angles, ranges, offsets, shape)
    assert used[4] == 0 and d[4].sum() == 0 and 0 < used[7] < 65536
    assert (d[7].max() == 255) == (shape == (3, 12))        # 65536 beams saturate 36 cells, not 1280


def test_three_hundred_beams_in_one_cell_saturate(gpu_ctx):
    angles = np.concatenate([np.full(300, 0.1), np.full(255, -1.0), np.full(256, 2.0)])
    ranges = np.concatenate([np.full(300, 5.0), np.full(255, 7.0), np.full(256, 9.0)])
    d, used = _descriptors_agree(gpu_ctx, angles, ranges, [0, 811], (20, 64))
    assert used[0] == 811 and sorted(d[d > 0].tolist()) == [255, 255, 255] and d.sum() == 765


def test_a_call_of_three_hundred_scans(gpu_ctx):
    sizes = [(37 * i) % 400 for i in range(300)]
    angles, ranges, offsets = AC.ragged(sizes, seed=11)
    d, used = _descriptors_agree(gpu_ctx, angles, ranges, offsets, (20, 60))
    assert d.shape == (300, 20, 60) and used[0] == 0 and used.max() > 300
    # the edge beams: on a ring edge, at range_max, at pi, at -pi
    edge_a = np.array([0.1, 0.1, math.pi, -math.pi, np.nextafter(math.pi, 0.0)])
    edge_r = np.array([AC.RANGE_MIN, AC.RANGE_MAX, 1.0, 1.0, 1.0])
    d, used = _descriptors_agree(gpu_ctx, edge_a, edge_r, [0, 5], (20, 60))
    assert used[0] == 3


def test_descriptor_build_refusals_carry_their_reason(gpu_ctx):
    angles, ranges, offsets = AC.ragged([5, 6])
    for kw, word in ((dict(n_rings=33), "n_rings"), (dict(n_sectors=10), "n_sectors"),
                     (dict(range_min=3.0, range_max=3.0), "range_min")):
        with pytest.raises(api.CsmError) as e:
            gpu_ctx.scan_descriptors(angles, ranges, offsets, **kw)
        assert word in str(e.value)
    with pytest.raises(api.CsmError) as e:
        gpu_ctx.scan_descriptors(angles, ranges, [0, 7, 5])
    assert "decreasing" in str(e.value)
    _descriptors_agree(gpu_ctx, angles, ranges, offsets, (3, 12))       # a refused call leaves the context usable


# ---- search ----

@pytest.mark.parametrize("shape", AC.SHAPES)
def test_device_search_is_the_host_search_at_every_shape(gpu_ctx, shape):
    n = 96 if shape[0] * shape[1] > 1000 else 200
    c = AC.search_case(n, *shape)
    q = np.arange(n)
    for k in KS:
        for one_per_map in (False, True):
            rec, counts, info = _agree(gpu_ctx, c, q, k=k, one_per_map=one_per_map, thr=2.0)
            assert counts.max() <= k and (one_per_map or counts.max() == k)
            assert counts.min() == 0 and info["pairs_eligible"] > 0
    # a gate in the middle of the distances: some pairs pass it, some fail it, some fail the ring bound alone
    full, _, finfo = _agree(gpu_ctx, c, q, k=16, thr=2.0)
    used = full[full["ref_scan_index"] >= 0]
    gate = int(np.median(used["distance"]))
    rec, counts, info = _agree(gpu_ctx, c, q, k=16, thr=2.0, max_distance=gate)
    assert 0 < info["pairs_eligible"] < finfo["pairs_eligible"]
    assert shape[1] == 4 or (used["shift"] > 0).any()


@pytest.mark.parametrize("n_ref", (0, 1, 63, 64, 65, 255, 256, 257, 1100))
def test_reference_counts_at_the_wave_and_block_edges(gpu_ctx, n_ref):
    c = AC.search_case(1200, 3, 12)
    rng = np.random.default_rng(n_ref)
    pool = np.arange(1100, 1200, dtype=np.int32)            # behind every reference node
    everywhere = rng.permutation(1200).astype(np.int32)
    total = 0
    for n_q, q in ((1, pool[:1]), (2, pool[5:7]), (300, everywhere[:300])):
        qt = c["travel"][q] if n_q == 300 else np.full(n_q, c["travel"][-1] + 100.0)
        for k in KS:
            for one_per_map in (False, True):
                _, counts, info = _agree(gpu_ctx, c, q, qt, n_ref, k=k, one_per_map=one_per_map)
                total += int(counts.sum())
                if n_q < 300:       # the gate is open: the prefix is all of n_ref, and only a query's own map is out
                    assert info["pairs_evaluated"] == n_q * n_ref
                    own = sum(int((c["map_index"][:n_ref] == c["map_index"][i]).sum()) for i in q)
                    assert info["pairs_eligible"] == n_q * n_ref - own and own < 13 * n_q
    assert (total == 0) == (n_ref == 0)


@pytest.mark.parametrize("extra", (0, 1, 1025))
def test_a_query_with_more_eligible_pairs_than_a_workgroup_s_chunk(gpu_ctx, extra):
    """A workgroup of the scoring kernel takes CSM_APPEARANCE_REF_CHUNK reference nodes of a query."""
    n_ref = L.APPEARANCE_REF_CHUNK + extra
    c = AC.search_case(n_ref + 1, 3, 12)
    for k in KS:
        for one_per_map in (False, True):
            rec, counts, info = _agree(gpu_ctx, c, [n_ref], [1e6], n_ref, k=k, one_per_map=one_per_map)
            eligible = n_ref - int((c["map_index"][:n_ref] == c["map_index"][n_ref]).sum())
            assert info["pairs_eligible"] == eligible >= n_ref - 13 and counts[0] == k
    # a second query whose gate closes in the middle of a chunk (node 500) rides along in the same launch
    _, _, info = _agree(gpu_ctx, c, [n_ref, 3], [1e6, 0.25 * 499 + 10.0], n_ref, k=16)
    assert info["pairs_evaluated"] == n_ref + min(n_ref, 500)


def test_more_queries_than_the_pair_table_holds(gpu_ctx):
    """The host chunks the queries so that the pair table stays within CSM_APPEARANCE_TABLE_BYTES."""
    n = 4200
    assert 4 * n * n > L.APPEARANCE_TABLE_BYTES >= 4 * n
    c = AC.search_case(n, 1, 4)
    q = np.arange(n - 1, -1, -1)
    rec, counts, info = _agree(gpu_ctx, c, q, k=2, one_per_map=True, thr=3.0)
    assert counts[0] == 2 and counts[-1] == 0 and info["pairs_evaluated"] > n * n // 3


def test_all_identical_descriptors_order_by_index(gpu_ctx):
    c = AC.search_case(301, 20, 60)
    c["desc"] = np.broadcast_to(c["desc"][7], c["desc"].shape).copy()
    firsts = [a for a, _ in c["runs"]]
    own = int((c["map_index"][:300] == c["map_index"][300]).sum())      # the query's own map is no reference
    for k in KS:
        rec, counts, info = _agree(gpu_ctx, c, [300], [1e6], 300, k=k)
        assert rec[0]["ref_scan_index"].tolist() == list(range(k)) and info["pairs_eligible"] == 300 - own
        assert not rec[0]["distance"].any() and not rec[0]["shift"].any() and not rec[0]["ring_distance"].any()
        rec, counts, _ = _agree(gpu_ctx, c, [300], [1e6], 300, k=k, one_per_map=True)
        assert rec[0]["ref_scan_index"].tolist() == firsts[:k]


@pytest.mark.parametrize("shape", ((3, 12), (32, 128)))
def test_sector_constant_descriptors_tie_at_every_shift(gpu_ctx, shape):
    c = AC.search_case(120, *shape)
    rng = np.random.default_rng(2)
    c["desc"] = np.repeat(rng.integers(0, 9, (120, shape[0], 1)), shape[1], axis=2).astype(np.uint8)
    rec, counts, _ = _agree(gpu_ctx, c, np.arange(120), k=16, thr=1.0)
    used = rec[rec["ref_scan_index"] >= 0]
    assert len(used) > 500 and not used["shift"].any()
    assert np.array_equal(used["distance"], used["ring_distance"]) and (used["distance"] > 0).any()


def test_max_distance_zero_keeps_the_exact_revisits_only(gpu_ctx):
    c = AC.search_case(200, 20, 64)
    desc = np.random.default_rng(8).integers(0, 4, (200, 20, 64)).astype(np.uint8)
    desc[150] = np.roll(desc[3], 37, axis=1)
    desc[151] = np.roll(desc[3], 63, axis=1)
    desc[152] = desc[60]
    c["desc"] = desc
    rec, counts, info = _agree(gpu_ctx, c, np.arange(200), max_distance=0, k=16, thr=1.0)
    assert info["pairs_eligible"] == 3 and counts.sum() == 3
    assert [tuple(rec[i, 0])[1:] for i in (150, 151, 152)] == [
        (3, int(c["map_index"][3]), 37, 0, 0), (3, int(c["map_index"][3]), 63, 0, 0),
        (60, int(c["map_index"][60]), 0, 0, 0)]


def test_min_cell_sum_removes_references_and_queries(gpu_ctx):
    c = AC.search_case(200, 3, 12)
    desc = c["desc"].copy()
    desc[5] = 0
    desc[5, 0, 0] = 9
    desc[150] = 0
    c["desc"] = desc
    q = np.arange(140, 160)
    base, _, binfo = _agree(gpu_ctx, c, q, k=16, thr=1.0)
    rec, counts, info = _agree(gpu_ctx, c, q, k=16, thr=1.0, min_cell_sum=10)
    assert counts[10] == 0 and 5 not in rec["ref_scan_index"] and info["pairs_eligible"] < binfo["pairs_eligible"]
    assert info["pairs_evaluated"] == binfo["pairs_evaluated"]
    _agree(gpu_ctx, c, q, k=16, thr=1.0, min_cell_sum=9)


def test_query_order_moves_rows_and_nothing_else(gpu_ctx):
    c = AC.search_case(200, 20, 60)
    q = np.arange(200)
    base, bcounts, binfo = _agree(gpu_ctx, c, q, k=2, one_per_map=True, thr=2.0)
    order = np.random.default_rng(11).permutation(q).astype(np.int32)
    rec, counts, info = _agree(gpu_ctx, c, order, k=2, one_per_map=True, thr=2.0)
    assert rec.tobytes() == base[order].tobytes() and counts.tobytes() == bcounts[order].tobytes() and info == binfo


def test_search_refusals_carry_their_reason(gpu_ctx):
    c = AC.search_case(200, 3, 12)
    for kw, word in ((dict(k=0), "n_per_query"), (dict(k=17), "n_per_query"), (dict(n_ref=201), "n_ref"),
                     (dict(q=[3, 3]), "repeated"), (dict(q=[200]), "range"), (dict(thr=np.nan), "finite")):
        with pytest.raises(api.CsmError) as e:
            qq = kw.pop("q", [150, 151])
            _agree(gpu_ctx, c, qq, [100.0] * len(qq), **kw)
        assert word in str(e.value)
    with pytest.raises(api.CsmError) as e:
        gpu_ctx.appearance_search(c["desc"], c["map_index"], c["travel"], [150], n_sectors=10)
    assert "n_sectors" in str(e.value)
    _agree(gpu_ctx, c, [150, 151], k=2)                 # a refused call leaves the context usable


def test_kernel_timers_count_the_calls(gpu_ctx):
    c = AC.search_case(200, 3, 12)
    angles, ranges, offsets = AC.ragged([5, 6])
    gpu_ctx.enable_kernel_timing(True)
    try:
        gpu_ctx.reset_kernel_timing()
        gpu_ctx.appearance_search(c["desc"], c["map_index"], c["travel"], np.arange(200))
        gpu_ctx.scan_descriptors(angles, ranges, offsets)
        ms, launches = gpu_ctx.kernel_time("appearance_search")
        dms, dlaunches = gpu_ctx.kernel_time("scan_descriptors")
    finally:
        gpu_ctx.enable_kernel_timing(False)
    assert launches == 1 and ms > 0.0 and dlaunches == 1 and dms > 0.0


def test_a_larger_then_a_smaller_call_and_the_memory_goes_back():
    before = api.debug_live_bytes()
    ctx = api.Context(0)
    try:
        big, small = AC.search_case(1200, 3, 12), AC.search_case(200, 3, 12)
        angles, ranges, offsets = AC.ragged([1025, 64, 3000])
        _descriptors_agree(ctx, angles, ranges, offsets, (20, 64))
        _agree(ctx, big, np.arange(1200), k=16, one_per_map=True)
        held = api.debug_live_bytes()
        assert held[0] > before[0] and held[1] > before[1]
        first, fcounts, finfo = _agree(ctx, small, np.arange(100, 120), k=2)
        _descriptors_agree(ctx, angles[:1000], ranges[:1000], [0, 1000], (3, 12))
        assert api.debug_live_bytes() == held           # the smaller calls fit the larger ones' workspaces
        fresh = api.Context(0)
        try:
            again, acounts, ainfo = fresh.appearance_search(small["desc"], small["map_index"], small["travel"],
                                                            np.arange(100, 120))
        finally:
            fresh.close()
        assert first.tobytes() == again.tobytes() and fcounts.tobytes() == acounts.tobytes() and finfo == ainfo
    finally:
        ctx.close()
    assert api.debug_live_bytes() == before


# ---- adapters ----

SEARCHER = dict(travel_dist_threshold=5.0, max_distance=100000, num_of_candidate_nodes=8, n_rings=20, n_sectors=64,
                range_min=0.5, range_max=20.0, min_cell_sum=50)


def _host_walk(c, scans, last, accum, k):
    """What LoopSearcherAppearanceHIP.search states, from the host functions alone."""
    lo, hi = c["runs"][last]
    d, _ = api.host_scan_descriptors(*api.ragged_scans(list(scans[:hi + 1])), 20, 64, 0.5, 20.0)
    rec, counts, _ = api.host_appearance_search(d, c["map_index"][:hi + 1], c["travel"][:hi + 1], np.arange(lo, hi + 1),
                                                accum, lo, 5.0, 100000, 50, k)
    used = sorted((int(r["distance"]), int(r["ref_scan_index"]), int(r["query_scan_index"]), int(r["ref_map_index"]),
                   int(r["shift"])) for row, n in zip(rec, counts) for r in row[:n])
    return used[:k]


def test_python_searcher_keeps_its_descriptors_and_matches_the_host_walk(gpu_ctx):
    c, scans = AC.scene()
    searcher = api.LoopSearcherAppearanceHIP(ctx=gpu_ctx, **SEARCHER)
    gpu_ctx.enable_kernel_timing(True)
    try:
        for last, nodes in ((3, 40), (5, 60), (4, 60)):
            gpu_ctx.reset_kernel_timing()
            kept = searcher.descriptors.copy()
            accum = float(c["travel"][c["runs"][last][1]])
            got = searcher.search(c["poses"], c["runs"], accum, last, scans)
            walk = _host_walk(c, scans, last, accum, 8)
            assert got == [(q, r, m) for _, r, q, m, _ in walk] and len(got) == 8
            assert searcher.last_records["shift"].tolist() == [s for *_, s in walk]
            assert searcher.last_headings == [api.host_descriptor_shift_angle(s, 64) for *_, s in walk]
            # only the new nodes' descriptors were built, and in one call
            assert searcher.descriptors.shape[0] == nodes
            assert searcher.descriptors[:len(kept)].tobytes() == kept.tobytes()
            assert gpu_ctx.kernel_time("scan_descriptors")[1] == (1 if nodes > len(kept) else 0)
    finally:
        gpu_ctx.enable_kernel_timing(False)
    # the room is seen again from (nearly) the same places under another heading: the best candidate's shift
    # says by how much, to within a sector and a half
    q, r, _ = got[0]
    want = math.remainder(c["poses"][q, 2] - c["poses"][r, 2], 2.0 * math.pi)
    assert abs(math.remainder(searcher.last_headings[0] - want, 2.0 * math.pi)) < 1.5 * (2.0 * math.pi / 64)
    per_map = searcher.search_per_map(c["poses"], c["runs"], 5, [59, 31, 45], 3, scans)
    rec, counts, _ = api.host_appearance_search(searcher.descriptors, c["map_index"], c["travel"], [59, 31, 45], None,
                                                None, 5.0, 100000, 50, 3, True)
    assert per_map == [(int(x["query_scan_index"]), int(x["ref_scan_index"]), int(x["ref_map_index"]))
                       for row, n in zip(rec, counts) for x in row[:n]] and len(per_map) > 3


_CPP = r"""
#include <cstdio>
#include <vector>
#include "../my-lidar-graph-slam-v2_amd/host/csm_adapters.hpp"
using namespace CsmHip;
static void put(FILE* o, const LoopCandidateVector& v, const AppearanceCandidateVector& full)
{
    const int n = (int)v.size();
    std::fwrite(&n, 4, 1, o);
    for (int i = 0; i < n; ++i) {
        const int ids[4] = { v[i].mQueryScanNodeId, v[i].mReferenceScanNodeId, v[i].mReferenceLocalMapId, full[i].mShift };
        const double d[3] = { v[i].mDistSq, (double)full[i].mRingDistance, full[i].mHeadingDiff };
        std::fwrite(ids, 4, 4, o);
        std::fwrite(d, 8, 3, o);
    }
}
int main(int argc, char** argv)
{
    /* input: n_scan n_maps last k n_queries n_per_query n_beams; accum (f64); poses; runs (2 x i32); query nodes
     * (i32); per node n_beams angles then n_beams ranges */
    if (argc < 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    int hdr[7];
    double accum;
    if (!f || std::fread(hdr, 4, 7, f) != 7 || std::fread(&accum, 8, 1, f) != 1) return 2;
    std::vector<std::array<double, 3>> poses(hdr[0]);
    std::vector<std::pair<int, int>> runs(hdr[1]);
    std::vector<int> nodes(hdr[4]);
    std::vector<double> beams((size_t)hdr[0] * 2 * hdr[6]);
    if (std::fread(poses.data(), 24, poses.size(), f) != poses.size() ||
        std::fread(runs.data(), 8, runs.size(), f) != runs.size() ||
        std::fread(nodes.data(), 4, nodes.size(), f) != nodes.size() ||
        std::fread(beams.data(), 8, beams.size(), f) != beams.size()) return 2;
    std::fclose(f);
    std::vector<ScanView> scans(hdr[0]);
    for (int i = 0; i < hdr[0]; ++i)
        scans[i] = ScanView { beams.data() + (size_t)i * 2 * hdr[6], beams.data() + ((size_t)i * 2 + 1) * hdr[6],
                              (std::size_t)hdr[6] };
    const csm_descriptor_params desc = { 20, 64, 0.5, 20.0 };
    auto searcher = LoopSearcherAppearanceHIP::Create(5.0, 100000u, hdr[3], desc, 50u);
    if (!searcher) return 3;
    LoopSearchHintView hint;
    hint.mScanNodePoses = poses.data();
    hint.mNumOfScanNodes = poses.size();
    hint.mLocalMapNodeRanges = runs.data();
    hint.mNumOfLocalMaps = runs.size();
    hint.mAccumTravelDist = accum;
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    hint.mLastFinishedMapId = hdr[2] - 2;               /* an earlier search: its descriptors are kept */
    searcher->Search(hint, scans);
    const int kept = (int)searcher->NumOfDescriptors();
    hint.mLastFinishedMapId = hdr[2];
    put(o, searcher->Search(hint, scans), searcher->LastCandidates());
    put(o, searcher->SearchPerMap(hint, scans, nodes, hdr[5]), searcher->LastCandidates());
    const int tail[2] = { kept, (int)searcher->NumOfDescriptors() };
    std::fwrite(tail, 4, 2, o);
    std::fclose(o);
    return 0;
}
"""


def test_cpp_adapter_gives_the_python_side_s_records(gpu_ctx, tmp_path):
    src, exe = tmp_path / "appearance.cpp", tmp_path / "appearance"
    src.write_text(_CPP.replace("../my-lidar-graph-slam-v2_amd", os.path.join(ROOT, "my-lidar-graph-slam-v2_amd")))
    csrc = os.path.join(ROOT, "my-lidar-graph-slam-v2_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L" + csrc, "-lcsm_hip", "-Wl,-rpath," + csrc])
    c, scans = AC.scene()
    last, k, nodes, per = 5, 8, [59, 31, 45], 3
    accum = float(c["travel"][-1])
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([len(c["poses"]), len(c["runs"]), last, k, len(nodes), per, len(scans[0][0])], np.int32).tobytes())
        f.write(np.array([accum]).tobytes())
        f.write(c["poses"].tobytes())
        f.write(np.array(c["runs"], np.int32).tobytes())
        f.write(np.array(nodes, np.int32).tobytes())
        for a, r in scans:
            f.write(np.ascontiguousarray(a, np.float64).tobytes())
            f.write(np.ascontiguousarray(r, np.float64).tobytes())
    subprocess.check_call([str(exe), str(inp), str(outp)], timeout=120)
    blob = outp.read_bytes()
    row = np.dtype([("ids", np.int32, 4), ("d", np.float64, 3)])
    lists, at = [], 0
    for _ in range(2):
        n = int(np.frombuffer(blob, np.int32, 1, at)[0])
        lists.append(np.frombuffer(blob, row, n, at + 4))
        at += 4 + row.itemsize * n
    searcher = api.LoopSearcherAppearanceHIP(ctx=gpu_ctx, **SEARCHER)
    for got, run in ((lists[0], lambda: searcher.search(c["poses"], c["runs"], accum, last, scans)),
                     (lists[1], lambda: searcher.search_per_map(c["poses"], c["runs"], last, nodes, per, scans))):
        want = run()
        assert [tuple(int(v) for v in g["ids"][:3]) for g in got] == want and len(want) >= 8
        assert got["ids"][:, 3].tolist() == searcher.last_records["shift"].tolist()
        assert got["d"][:, 0].tolist() == searcher.last_records["distance"].astype(np.float64).tolist()
        assert got["d"][:, 1].tolist() == searcher.last_records["ring_distance"].astype(np.float64).tolist()
        assert got["d"][:, 2].tolist() == searcher.last_headings
    assert np.frombuffer(blob, np.int32, 2, at).tolist() == [40, 60]
