"""The host functions of the appearance unit (csm_host_scan_descriptors, csm_host_descriptor_shift_angle,
csm_host_appearance_search) against appearance_reference, byte for byte. No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from csm_hip import _lib as L, api
import appearance_cases as AC
import appearance_reference as R

U32_MAX = 0xffffffff


def _ref_records(rec):
    """reference records in the API's dtype (the same fields in the same order)"""
    assert R.CANDIDATE == api.APPEARANCE_CANDIDATE_DTYPE
    return rec


# ---- the descriptor ----

def _one(angles, ranges, n_rings=4, n_sectors=8, range_min=0.0, range_max=8.0):
    angles, ranges = np.asarray(angles, np.float64), np.asarray(ranges, np.float64)
    d, used = api.host_scan_descriptors(angles, ranges, [0, len(angles)], n_rings, n_sectors, range_min, range_max)
    want, want_used = R.descriptor(angles, ranges, n_rings, n_sectors, range_min, range_max)
    assert d[0].tobytes() == want.tobytes() and used[0] == want_used
    return d[0], int(used[0])


def test_a_range_on_a_ring_edge_goes_to_the_upper_ring():
    ring_edge, _ = R.edges(4, 8, 0.0, 8.0)
    assert ring_edge.tolist() == [0.0, 2.0, 4.0, 6.0, 8.0]
    d, used = _one([0.1, 0.1, 0.1], [2.0, np.nextafter(2.0, 0.0), 0.0])
    assert used == 3 and d[1, 4] == 1 and d[0, 4] == 2 and d.sum() == 3


def test_range_max_and_pi_are_excluded():
    d, used = _one([0.1, 0.1, math.pi, np.nextafter(math.pi, 0.0), -math.pi],
                   [8.0, np.nextafter(8.0, 0.0), 1.0, 1.0, 1.0])
    assert used == 3 and d[3, 4] == 1 and d[0, 7] == 1 and d[0, 0] == 1 and d.sum() == 3
    d, used = _one([0.1, -3.2, 3.2], [-0.1, 1.0, 1.0])
    assert used == 0 and d.sum() == 0


def test_nan_and_inf_beams_are_skipped_and_counted():
    d, used = _one([0.1, np.nan, 0.1, np.inf, 0.1, -np.inf, 0.2], [1.0, 1.0, np.nan, 1.0, np.inf, 1.0, -np.inf])
    assert used == 1 and d.sum() == 1 and d[0, 4] == 1


def test_three_hundred_beams_in_one_cell_give_255():
    d, used = _one(np.full(300, 0.1), np.full(300, 5.0))
    assert used == 300 and d[2, 4] == 255 and d.sum() == 255


@pytest.mark.parametrize("n", (0, 1, 65536))
def test_beam_counts_zero_one_and_the_most(n):
    rng = np.random.default_rng(n)
    angles, ranges = rng.uniform(-3.3, 3.3, n), rng.uniform(-0.5, 9.0, n)
    d, used = api.host_scan_descriptors(angles, ranges, [0, n], 4, 8, 0.0, 8.0)
    inside = (ranges >= 0.0) & (ranges < 8.0) & (angles >= -math.pi) & (angles < math.pi)
    assert used[0] == inside.sum()
    if n <= 1:
        assert d.sum() == used[0]
    else:
        want, want_used = R.descriptor(angles[:4000], ranges[:4000], 4, 8, 0.0, 8.0)
        part, part_used = api.host_scan_descriptors(angles[:4000], ranges[:4000], [0, 4000], 4, 8, 0.0, 8.0)
        assert part[0].tobytes() == want.tobytes() and part_used[0] == want_used
        assert d.max() == 255       # 65536 beams over 32 cells


def test_empty_scans_give_a_zero_descriptor():
    angles, ranges, offsets = AC.ragged([0, 5, 0, 0, 3, 0])
    d, used = api.host_scan_descriptors(angles, ranges, offsets, 3, 12, AC.RANGE_MIN, AC.RANGE_MAX)
    assert d.shape == (6, 3, 12) and used[[0, 2, 3, 5]].tolist() == [0] * 4
    assert d[[0, 2, 3, 5]].sum() == 0
    want, want_used = R.descriptors(angles, ranges, offsets, 3, 12, AC.RANGE_MIN, AC.RANGE_MAX)
    assert d.tobytes() == want.tobytes() and used.tolist() == want_used.tolist()


@pytest.mark.parametrize("shape", AC.SHAPES)
def test_ragged_scans_are_the_reference_s(shape):
    angles, ranges, offsets = AC.ragged([1, 63, 64, 65, 700], seed=shape[1])
    d, used = api.host_scan_descriptors(angles, ranges, offsets, shape[0], shape[1], AC.RANGE_MIN, AC.RANGE_MAX)
    want, want_used = R.descriptors(angles, ranges, offsets, shape[0], shape[1], AC.RANGE_MIN, AC.RANGE_MAX)
    assert d.tobytes() == want.tobytes() and used.tolist() == want_used.tolist()
    assert 0 < used.sum() < offsets[-1]


# ---- the shift ----

@pytest.mark.parametrize("shape", ((3, 12), (20, 64)))
def test_a_rolled_scan_has_distance_zero_at_its_shift(shape):
    n_rings, n_sectors = shape
    n = 6 * n_sectors
    rng = np.random.default_rng(n_sectors)
    angles = -math.pi + 2.0 * math.pi * (np.arange(n) + 0.5) / n      # no beam on a sector edge
    ranges_ref = rng.uniform(AC.RANGE_MIN, AC.RANGE_MAX - 0.01, n)
    _, sector_edge = R.edges(n_rings, n_sectors, AC.RANGE_MIN, AC.RANGE_MAX)
    assert not np.isin(angles, sector_edge).any()
    all_ranges = [ranges_ref] + [np.roll(ranges_ref, k * n // n_sectors) for k in range(n_sectors)]
    d, used = api.host_scan_descriptors(np.tile(angles, len(all_ranges)), np.concatenate(all_ranges),
                                        n * np.arange(len(all_ranges) + 1), n_rings, n_sectors, AC.RANGE_MIN,
                                        AC.RANGE_MAX)
    assert used.tolist() == [n] * len(all_ranges)
    # node 0 is the reference (map 0); node 1 + k is the query rolled by k sectors (map 1)
    m = np.array([0] + [1] * n_sectors, np.int32)
    travel = np.arange(len(m), dtype=np.float64)
    rec, counts, _ = api.host_appearance_search(d, m, travel, np.arange(1, len(m)), None, 1, -1.0, U32_MAX, 0, 1)
    assert counts.tolist() == [1] * n_sectors
    assert rec[:, 0]["distance"].tolist() == [0] * n_sectors
    assert rec[:, 0]["shift"].tolist() == list(range(n_sectors))
    assert rec[:, 0]["ring_distance"].tolist() == [0] * n_sectors
    for k in range(n_sectors):
        got = api.host_descriptor_shift_angle(k, n_sectors)
        want = math.fmod(-k * 2.0 * math.pi / n_sectors, 2.0 * math.pi)
        want = want + 2.0 * math.pi if want < -math.pi else want
        assert got == R.shift_angle(k, n_sectors) and abs(got - want) < 1e-12 and -math.pi <= got <= math.pi


def test_shift_angle_refusals():
    for shift, n_sectors in ((-1, 12), (12, 12), (0, 0), (0, 10), (0, 132)):
        with pytest.raises(api.CsmError) as e:
            api.host_descriptor_shift_angle(shift, n_sectors)
        assert e.value.code == L.CSM_EINVAL
    assert L.load().csm_host_descriptor_shift_angle(0, 12, None) == L.CSM_EINVAL


# ---- the search ----

def _args(c, q, qt=None, n_ref=None, max_distance=U32_MAX, min_cell_sum=0, k=2, one_per_map=False, thr=10.0):
    return (c["desc"], c["map_index"], c["travel"], np.asarray(q, np.int32), qt, n_ref, thr, max_distance,
            min_cell_sum, k, one_per_map)


def _host_is_reference(c, q, **kw):
    args = _args(c, q, **kw)
    rec, counts, info = api.host_appearance_search(*args)
    qt = c["travel"][args[3]] if args[4] is None else np.broadcast_to(np.asarray(args[4], np.float64), args[3].shape)
    n_ref = len(c["desc"]) if args[5] is None else args[5]
    want, wcounts, winfo = R.search(c["desc"], c["map_index"], c["travel"], n_ref, args[3], qt, *args[6:])
    assert rec.tobytes() == _ref_records(want).tobytes()
    assert counts.tolist() == wcounts.tolist() and info == winfo
    return rec, counts, info


@pytest.mark.parametrize("shape", ((1, 4), (3, 12), (20, 60)))
def test_search_is_the_reference_s(shape):
    c = AC.search_case(56, *shape)
    q = np.arange(56)
    for k in (1, 2, 16):
        for one_per_map in (False, True):
            rec, counts, info = _host_is_reference(c, q, k=k, one_per_map=one_per_map, thr=2.0)
            assert counts.max() <= k and (one_per_map or counts.max() == k)
            assert counts.min() == 0 and info["pairs_eligible"] > 0
    used = rec[rec["ref_scan_index"] >= 0]
    assert np.all(used["ring_distance"] <= used["distance"])
    assert shape[1] == 4 or (used["shift"] > 0).any()


def test_ring_distance_never_exceeds_distance():
    for shape in AC.SHAPES:
        d = AC.descriptor_set(24, *shape, seed=9)
        m = (np.arange(24) // 2).astype(np.int32)
        rec, counts, _ = api.host_appearance_search(d, m, np.zeros(24), np.arange(24), None, None, -1.0, U32_MAX, 0, 16)
        assert counts.tolist() == [16] * 24
        assert np.all(rec["ring_distance"] <= rec["distance"])
        q, r = int(rec[5, 3]["query_scan_index"]), int(rec[5, 3]["ref_scan_index"])
        assert R.distance(d[q], d[r]) == (int(rec[5, 3]["distance"]), int(rec[5, 3]["shift"]),
                                          int(rec[5, 3]["ring_distance"]))


def test_identical_descriptors_come_in_reference_order():
    c = AC.search_case(40, 3, 12)
    c["desc"] = np.broadcast_to(c["desc"][7], c["desc"].shape).copy()
    rec, counts, info = _host_is_reference(c, [39], qt=[100.0], k=16)
    assert rec[0]["ref_scan_index"].tolist() == list(range(16)) and rec[0]["distance"].tolist() == [0] * 16
    assert rec[0]["shift"].tolist() == [0] * 16
    rec, _, _ = _host_is_reference(c, [39], qt=[100.0], k=16, one_per_map=True)
    firsts = [a for a, _ in c["runs"]]
    assert rec[0]["ref_scan_index"][:5].tolist() == firsts[:5]


def test_sector_constant_descriptors_tie_at_every_shift():
    c = AC.search_case(40, 3, 12)
    rng = np.random.default_rng(2)
    c["desc"] = np.repeat(rng.integers(0, 9, (40, 3, 1)), 12, axis=2).astype(np.uint8)
    rec, counts, _ = _host_is_reference(c, np.arange(40), k=16, thr=1.0)
    used = rec[rec["ref_scan_index"] >= 0]
    assert len(used) > 100 and not used["shift"].any()
    # every ring sum is 12 times the ring's one value, so the bound is attained
    assert np.array_equal(used["distance"], used["ring_distance"]) and (used["distance"] > 0).any()


def test_max_distance_zero_and_the_largest():
    c = AC.search_case(48, 3, 12)
    desc = np.random.default_rng(8).integers(0, 4, (48, 3, 12)).astype(np.uint8)      # no two alike
    desc[40] = np.roll(desc[3], 5, axis=1)          # but for one exact revisit, rolled
    c["desc"] = desc
    rec, counts, info = _host_is_reference(c, np.arange(48), max_distance=0, k=16, thr=1.0)
    assert info["pairs_eligible"] == 1 and counts[40] == 1 and counts.sum() == 1
    assert tuple(rec[40, 0]) == (40, 3, int(c["map_index"][3]), 5, 0, 0)
    rec, counts, info = _host_is_reference(c, np.arange(48), max_distance=U32_MAX, k=16, thr=1.0)
    own_map = sum(int((c["map_index"][:R.prefix_length(c["travel"], 48, c["travel"][q], 1.0)] == c["map_index"][q]).sum())
                  for q in range(48))
    assert info["pairs_eligible"] == info["pairs_evaluated"] - own_map


def test_min_cell_sum_removes_a_reference_and_a_query():
    c = AC.search_case(48, 3, 12)
    desc = c["desc"].copy()
    desc[5] = 0
    desc[5, 0, 0] = 9                   # sum 9
    desc[44] = 0                        # sum 0
    c["desc"] = desc
    assert np.delete(desc.reshape(48, -1).astype(np.int64).sum(1), [5, 44]).min() > 10
    q = np.arange(40, 48)
    # twelve reference nodes and sixteen slots: every eligible pair is a record
    base, bcounts, binfo = _host_is_reference(c, q, n_ref=12, k=16, thr=1.0)
    assert bcounts.tolist() == [12] * 8 and binfo["pairs_eligible"] == 96
    rec, counts, info = _host_is_reference(c, q, n_ref=12, k=16, thr=1.0, min_cell_sum=10)
    assert 5 not in rec["ref_scan_index"] and counts.tolist() == [11] * 4 + [0] + [11] * 3
    assert rec[4]["ref_scan_index"].tolist() == [-1] * 16 and rec[4]["query_scan_index"].tolist() == [44] * 16
    assert info["pairs_evaluated"] == binfo["pairs_evaluated"] == 96 and info["pairs_eligible"] == 77
    rec, counts, _ = _host_is_reference(c, q, n_ref=12, k=16, thr=1.0, min_cell_sum=9)     # 9 >= 9 stays
    assert 5 in rec["ref_scan_index"] and counts.tolist() == [12] * 4 + [0] + [12] * 3


def test_one_per_map_and_the_cut():
    c = AC.search_case(56, 3, 12)
    full, fcounts, _ = _host_is_reference(c, [55], k=16, thr=1.0)
    for k in (1, 2, 15):
        rec, counts, _ = _host_is_reference(c, [55], k=k, thr=1.0)
        assert rec[0].tobytes() == full[0, :k].tobytes() and counts[0] == k
    rec, counts, _ = _host_is_reference(c, [55], k=16, thr=1.0, one_per_map=True)
    maps = rec[0]["ref_map_index"][:counts[0]].tolist()
    assert len(set(maps)) == len(maps) == min(16, len(c["runs"]) - 1)
    assert np.all(np.diff(rec[0]["distance"][:counts[0]].astype(np.int64)) >= 0)


def test_the_travel_prefix():
    c = AC.search_case(56, 3, 12)
    # travel is 0.25 i: from 9.99 node 0 fails the gate (9.99 - 0 < 10); from 10.0 node 0 alone passes
    rec, counts, info = _host_is_reference(c, [50, 51, 52], qt=[9.99, 10.0, 1e9], k=16)
    assert counts.tolist() == [0, 1, 16] and info["pairs_evaluated"] == 0 + 1 + 56
    rec, counts, info = _host_is_reference(c, [50, 51], qt=[1e9, 1e9], n_ref=7, k=16)
    assert info["pairs_evaluated"] == 14 and counts.tolist() == [7, 7]
    _, counts, info = _host_is_reference(c, [50], qt=[1e9], n_ref=0)
    assert counts.tolist() == [0] and info == dict(pairs_evaluated=0, pairs_eligible=0)


def _raw_search(c, **change):
    """csm_host_appearance_search with one argument changed; its return code."""
    a = dict(desc=np.ascontiguousarray(c["desc"]), map=c["map_index"].copy(), travel=c["travel"].copy(),
             n_scan=len(c["desc"]), n_maps=len(c["runs"]), n_ref=len(c["desc"]), q=np.array([50, 51], np.int32),
             qt=np.array([20.0, 30.0]), n_q=2, n_rings=3, n_sectors=12, range_min=0.5, range_max=20.0, thr=10.0, k=2,
             one_per_map=0, null=())
    a.update(change)
    p = L.AppearanceParams(L.DescriptorParams(a["n_rings"], a["n_sectors"], a["range_min"], a["range_max"]), a["thr"],
                           U32_MAX, 0, a["k"], a["one_per_map"])
    out = np.zeros((2, 16), api.APPEARANCE_CANDIDATE_DTYPE)
    counts = np.zeros(2, np.int32)
    ptr = lambda name, arr: None if name in a["null"] else arr.ctypes.data_as(C.c_void_p)
    return L.load().csm_host_appearance_search(
        ptr("desc", a["desc"]), ptr("map", a["map"]), ptr("travel", a["travel"]), a["n_scan"], a["n_maps"], a["n_ref"],
        ptr("q", a["q"]), ptr("qt", a["qt"]), a["n_q"], None if "params" in a["null"] else C.byref(p),
        ptr("out", out), ptr("counts", counts), None)


def test_every_refusal_of_the_search():
    c = AC.search_case(56, 3, 12)
    assert _raw_search(c) == L.CSM_OK                       # info may be null
    bad_travel, inf_travel, bad_map, high_map = c["travel"].copy(), c["travel"].copy(), c["map_index"].copy(), c["map_index"].copy()
    bad_travel[20] = 0.0
    inf_travel[55] = np.inf
    bad_map[20] = 0
    high_map[55] = len(c["runs"])
    causes = [dict(null=(name,)) for name in ("desc", "map", "travel", "q", "qt", "params", "out", "counts")]
    causes += [dict(n_scan=0), dict(n_scan=(1 << 20) + 1), dict(n_maps=0), dict(n_maps=(1 << 16) + 1),
               dict(n_maps=len(c["runs"]) - 1), dict(n_ref=-1), dict(n_ref=57), dict(n_q=0), dict(k=0), dict(k=17),
               dict(one_per_map=2), dict(thr=np.nan), dict(thr=np.inf), dict(travel=bad_travel), dict(travel=inf_travel),
               dict(map=bad_map), dict(map=high_map), dict(q=np.array([50, 50], np.int32)),
               dict(q=np.array([50, 56], np.int32)), dict(q=np.array([-1, 50], np.int32)),
               dict(qt=np.array([20.0, np.nan])), dict(n_rings=0), dict(n_rings=33), dict(n_sectors=0),
               dict(n_sectors=10), dict(n_sectors=132), dict(range_min=np.nan), dict(range_max=np.inf),
               dict(range_min=20.0), dict(range_min=21.0)]
    for change in causes:
        assert _raw_search(c, **change) == L.CSM_EINVAL, change
    # n_scan * n_rings * n_sectors above 2^30: refused before any array is read past what the test owns
    big = dict(n_scan=1 << 20, n_rings=32, n_sectors=64)
    assert (1 << 20) * 32 * 64 > 1 << 30
    assert _raw_search(c, **big) == L.CSM_EINVAL


def test_every_refusal_of_the_descriptor_build():
    angles, ranges, offsets = AC.ragged([5, 6])
    ok = lambda **kw: api.host_scan_descriptors(angles, ranges, kw.pop("offsets", offsets), **kw)
    ok(n_rings=3, n_sectors=12)
    for kw in (dict(n_rings=0), dict(n_rings=33), dict(n_sectors=0), dict(n_sectors=6), dict(n_sectors=132),
               dict(range_min=np.nan), dict(range_max=np.inf), dict(range_min=5.0, range_max=5.0),
               dict(offsets=[1, 5, 11]), dict(offsets=[0, 7, 5]), dict(offsets=[0])):
        with pytest.raises(api.CsmError) as e:
            ok(**kw)
        assert e.value.code == L.CSM_EINVAL, kw
    n = L.DESCRIPTOR_MAX_BEAMS + 1
    with pytest.raises(api.CsmError):
        api.host_scan_descriptors(np.zeros(n), np.ones(n), [0, n], 3, 12)
    p = L.DescriptorParams(3, 12, 0.5, 20.0)
    out, used = np.zeros((2, 36), np.uint8), np.zeros(2, np.int32)
    v = lambda a: a.ctypes.data_as(C.c_void_p)
    fn = L.load().csm_host_scan_descriptors
    assert fn(v(angles), v(ranges), v(offsets), 2, C.byref(p), v(out), v(used)) == L.CSM_OK
    for hole in range(7):
        a = [v(angles), v(ranges), v(offsets), 2, C.byref(p), v(out), v(used)]
        if hole == 3:
            continue
        a[hole] = None
        assert fn(*a) == L.CSM_EINVAL
