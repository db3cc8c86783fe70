"""CPU suite: every case of tests/volume_shape_cases.py has the property it is in the table for, computed
from the reference's window shape, and the references' results on it are such that the GPU comparison of
tests/test_gpu_volume_shapes.py cannot pass vacuously. No GPU."""
import numpy as np
import pytest

import peaks_reference as PR
import prior_reference as P
import volume_reference as VR
import volume_shape_cases as V
from csm_hip import _lib as Lb, api

# The kernels' constants, restated (the case table exists to straddle them):
VOL_STRIDE = 256            # kVolBlock, csm_volume_kernels.hip: candidates between a lane's steps
PRIOR_STRIDE = 1024         # kPriorBlock * kPriorRun, csm_prior_kernels.hip
PRIOR_RUN = 4               # kPriorRun: candidates of one lane and step
CHUNK = 8192                # candidates per workgroup below the cap (J.chunk, csm_peaks_api.hip)
BLOCKS_MAX = 256            # kPeakBlocksMax, csm_peaks.hpp: workgroups per window
KNOWN_TRIP = 256 * 256      # k_peaks_coarse_known: at most 256 workgroups of kPeakBlock = 256 nodes per trip


def _total(name):
    return int(np.prod(V.shape_of(name)))


def _blocks_chunk(total):
    """blocks and chunk of a window as peaks_score_chunk sets them."""
    blocks = min(BLOCKS_MAX, max(1, -(-total // CHUNK)))
    return blocks, -(-total // blocks)


CHECKS = {
    "one": lambda nt, nx, ny, L: nt * nx * ny == 1,
    "nxc1": lambda nt, nx, ny, L: nx // L == 1,
    "nyc1": lambda nt, nx, ny, L: ny // L == 1,
    "nt1": lambda nt, nx, ny, L: nt == 1,
    "row<256": lambda nt, nx, ny, L: nx * ny < VOL_STRIDE,
    "ny<4": lambda nt, nx, ny, L: ny < PRIOR_RUN,
    "<256": lambda nt, nx, ny, L: nt * nx * ny < VOL_STRIDE,
    ">256": lambda nt, nx, ny, L: nt * nx * ny > VOL_STRIDE,
    "<1024": lambda nt, nx, ny, L: nt * nx * ny < PRIOR_STRIDE,
    ">1024": lambda nt, nx, ny, L: nt * nx * ny > PRIOR_STRIDE,
    "<8192": lambda nt, nx, ny, L: nt * nx * ny < CHUNK,
    ">8192": lambda nt, nx, ny, L: nt * nx * ny > CHUNK,
    "mod1": lambda nt, nx, ny, L: nt * nx * ny % PRIOR_RUN == 1,
    "mod2": lambda nt, nx, ny, L: nt * nx * ny % PRIOR_RUN == 2,
    "mod3": lambda nt, nx, ny, L: nt * nx * ny % PRIOR_RUN == 3,
    "capped": lambda nt, nx, ny, L: nt * nx * ny > BLOCKS_MAX * CHUNK,
    "nodes>65536": lambda nt, nx, ny, L: L > 1 and nt * (nx // L) * (ny // L) > KNOWN_TRIP,
}
FROM_RESULTS = {"no_band", "ties", "elig"}


@pytest.mark.parametrize("name", [c["name"] for c in V.CASES + V.BATCH])
def test_every_case_has_the_properties_it_is_there_for(name):
    c = V.BY_NAME[name]
    nt, nx, ny = V.shape_of(name)
    assert nt % 2 == 1 and nx % c["L"] == 0 and ny % c["L"] == 0
    assert c["props"] <= set(CHECKS) | FROM_RESULTS
    for p in c["props"] - FROM_RESULTS:
        assert CHECKS[p](nt, nx, ny, c["L"]), (name, p, (nt, nx, ny))
    if name.startswith("mid_"):
        assert _total(name) == int(name[4:])
    _, vol = V.volume(name)
    if "no_band" in c["props"]:
        assert vol["cf"]["touchesBand"] == 0
    if "ties" in c["props"]:
        assert V.peaks(name)[0]["tie_count"] > 1000 and vol["cf"]["touchesBand"] == 1
        assert all(r["flags"] & Lb.FLAG_KEY_TIE for r in V.peaks(name))


def test_the_table_covers_what_the_issue_lists():
    tiny = [c for c in V.TINY if not c["elig"]]
    assert {c["L"] for c in tiny} == {1, 2, 3, 4, 8} and len(tiny) == 25
    totals = sorted(_total(c["name"]) for c in tiny)
    assert totals[0] == 1 and totals[-1] == 896
    for p in ("one", "nxc1", "nyc1", "nt1", "ny<4"):
        assert any(p in c["props"] for c in tiny), p
    # a degenerate radix at L > 1: the whole axis is one coarse node, every column but one an extended one
    assert any(c["L"] > 1 and "nxc1" in c["props"] for c in tiny) and any(c["L"] > 1 and "nyc1" in c["props"] for c in tiny)
    assert {V.shape_of(c["name"])[2] for c in tiny if "ny<4" in c["props"]} == {1, 2, 3}
    assert all("row<256" in c["props"] for c in tiny)
    assert max(nx * ny for _, nx, ny in (V.shape_of(c["name"]) for c in tiny)) < VOL_STRIDE
    # windows whose only run is a tail, and a tail inside the first run of the first lane
    assert any(_total(c["name"]) < PRIOR_RUN for c in tiny)
    # mid windows: both sides of every stride, every residue of the run length
    mids = [_total(c["name"]) for c in V.MID]
    for edge in (VOL_STRIDE, PRIOR_STRIDE, CHUNK):
        below = max(t for t in mids if t < edge)
        above = min(t for t in mids if t > edge)
        assert edge - below <= edge // 32 and above - edge <= edge // 32 + 16, (edge, below, above)
    assert {t % PRIOR_RUN for t in mids} == {0, 1, 2, 3}
    # above the chunk size the chunk is no multiple of the strides
    assert any(_blocks_chunk(t)[1] % PRIOR_RUN and _blocks_chunk(t)[1] % VOL_STRIDE for t in mids if t > CHUNK)
    big = [c["name"] for c in V.LARGE]
    assert [V.shape_of(n) for n in big] == [(133, 129, 129), (133, 130, 130), (133, 129, 129), (131, 130, 130)]
    for n in big:
        blocks, chunk = _blocks_chunk(_total(n))
        assert blocks == BLOCKS_MAX and chunk > CHUNK and chunk % VOL_STRIDE and chunk % PRIOR_RUN


def test_tiny_windows_run_out_of_peaks_and_the_single_candidate_weighs_one():
    short = [c["name"] for c in V.TINY if len(V.peaks(c["name"])) < V.K_MAX]
    assert "point_L1" in short and len(short) >= 3
    assert all(len(V.peaks(n)) >= 1 for n in short)
    for tau in V.TAUS:
        s = V.summary("point_L1", tau)
        m = s["moments"]
        assert m["m0"] == 1 << 24 and m["m1"] == [0] * 3 and m["m2"] == [0] * 6 and m["support"] == 1
        assert m["border_support"] == 1 and s["covariance"] == [0.0] * 9 and s["sensor_covariance"] == [0.0] * 9


@pytest.mark.parametrize("name", [c["name"] for c in V.TINY if c["elig"]])
def test_the_threshold_of_the_eligibility_cases_bites(name):
    c = V.BY_NAME[name]
    case, vol = V.volume(name)
    n = len(case["angles"])
    thr = V.known_thr(name)
    rate = vol["CK"].astype(np.float64) / float(n)
    assert c["L"] > 1 and _total(name) < PRIOR_STRIDE
    assert 0 < (~(rate > thr)).sum() < rate.size            # a node is out, not all of them
    assert 1 < api.host_min_known(n, thr) <= n
    # the same window at threshold 0: a peak of its list sits under a node that is out now
    rng = V.search_range(c)
    free = PR.peaks(case, *rng, c["L"], V.K_MAX, V.EXCL)[0]
    assert V.peaks(name) != free and len(V.peaks(name)) >= 1
    key = 32268 * vol["K"].astype(np.int64) + 499 * vol["S"].astype(np.int64)
    out = ~np.repeat(np.repeat(rate > thr, c["L"], 1), c["L"], 2)
    assert (key[out] > V.peaks(name)[-1]["key"]).any()          # an ineligible candidate outranks a returned peak
    assert V.summary(name, V.TAUS[1])["moments"] != VR.summary(case, *rng, c["L"], V.TAUS[1])[0]["moments"]
    assert all(V.prior(name, lam)[0]["best"]["found"] for lam in V.LAMBDA_NAMES)


@pytest.mark.parametrize("name", [c["name"] for c in V.LARGE])
def test_large_windows_make_the_comparison_meaningful(name):
    case, vol = V.volume(name)
    win = vol["win"]
    total = _total(name)
    blocks, chunk = _blocks_chunk(total)
    n = len(case["angles"])
    # the prior: none of the matrices is refused at this window's extent, and one of them moves the winner
    for lam in V.LAMBDA_NAMES:
        assert P.quantise(V.LAMBDAS[lam], win["steps"], n, P.d_max_of(win)) is not None
    assert P.d_max_of(win) >= 130
    refs = [V.prior(name, lam)[0] for lam in V.LAMBDA_NAMES]
    assert all(r["best"]["found"] for r in refs) and any(r["best"] != r["unweighted"] for r in refs)
    assert V.prior(name, "indef")[1] > 0                 # the clamp acts
    # the two winners sit in different workgroups' chunks
    rank = lambda r: ((r["best_theta"] + win["win"][2]) * win["shape"][1] + r["best_x"] + win["win"][0]) * win["shape"][2] \
        + r["best_y"] + win["win"][1]
    assert len({rank(r["best"]) // chunk for r in refs} | {rank(refs[0]["unweighted"]) // chunk}) > 1
    # the moments: a support above one chunk, weight in more than one workgroup's chunk and beyond the first 64
    for tau in V.TAUS:
        m = V.summary(name, tau)["moments"]
        assert m["support"] > CHUNK and m["m1"] != [0, 0, 0] and m["border_support"] > 0
        W, shift = api.host_volume_weights(n, tau)
        key = 32268 * vol["K"].astype(np.int64) + 499 * vol["S"].astype(np.int64)
        bins = ((m["best"]["key"] - key) >> shift).reshape(-1)
        heavy = np.flatnonzero((bins >= 0) & (bins < Lb.VOLUME_BINS) & (W[np.clip(bins, 0, Lb.VOLUME_BINS - 1)] > 0))
        chunks = np.unique(heavy // chunk)
        assert len(chunks) > 64 and chunks.max() >= 64
    assert len(V.peaks(name)) == V.K_MAX


def test_the_mixed_batch_shares_one_range_and_mixes_block_counts():
    big = V.BY_NAME["big_L2"]
    assert big["metres"] == V.BATCH_RANGE and big["L"] == V.BATCH_L
    totals = [_total(n) for n in ("batch_short", "batch_long", "big_L2")]
    assert totals[0] < VOL_STRIDE < totals[1] < PRIOR_STRIDE and totals[2] > BLOCKS_MAX * CHUNK
    assert [_blocks_chunk(t)[0] for t in totals] == [1, 1, BLOCKS_MAX]
    # two maps: the two small windows are scans of different maximum range on one map of 1.6 m cells
    a, b = V.scan_case("coarse_short"), V.scan_case("coarse_long")
    assert (a["grid"] == b["grid"]).all() and a["geom"] == b["geom"] and a["ranges"].max() != b["ranges"].max()
    for n in ("batch_short", "batch_long"):
        assert len(V.peaks(n)) == V.K_MAX and V.summary(n, V.TAUS[1])["moments"]["support"] > 1
