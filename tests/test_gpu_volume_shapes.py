"""GPU parity of the three units that read a window's whole score volume -- the K best peaks, the volume
covariance, the motion prior -- at the window shapes of tests/volume_shape_cases.py: windows of 1 to 896
candidates with one coarse node per axis or one slice, totals on both sides of the kernels' strides (256,
1024) and chunk size (8192) with every residue of the prior's run of 4, and windows above the cap of 256
workgroups (chunks that are no multiple of a stride, more coarse nodes than one trip of the known-count
kernel, a tie set over many chunks). Bar: every integer equal, every double bit-equal to the references."""
import numpy as np
import pytest

import peaks_reference as PR
import test_gpu_prior as TP
import test_gpu_volume_cov as TV
import volume_shape_cases as V
from csm_hip import _lib as Lb, api

pytestmark = pytest.mark.gpu

MAP = 1000
K_MAX, EXCL, TAUS = V.K_MAX, V.EXCL, TV.TAUS
LAMBDAS = {k: TP.LAMBDAS[k] for k in V.LAMBDA_NAMES}
assert TAUS == V.TAUS and all((LAMBDAS[k] == V.LAMBDAS[k]).all() for k in LAMBDAS)       # what the references used
NOT_CLOSED_FORM = Lb.FLAG_EDGE_BAND | Lb.FLAG_LITERAL


def _window(ctx, name, map_id=MAP):
    """Uploads the case's map; (case, window dict, csm_window, known-rate threshold, edge-band flag of the
    single-best search on the window)."""
    L = V.BY_NAME[name]["L"]
    case, vol = V.volume(name)
    win = vol["win"]
    wx, wy, wt = win["win"]
    ctx.upload_grid(map_id, case["grid"])
    ctx.build_pyramid(map_id, [1, L])
    n = len(case["angles"])
    thr = V.known_thr(name)
    w = ctx.make_window(2 * wt + 1, n, wx, wy, L, 1 if L > 1 else 0, api.host_min_known(n, thr), 0.0)
    single = ctx.score_window(map_id, w, win["col"], win["row"])
    band = single["flags"] & Lb.FLAG_EDGE_BAND
    if not vol["cf"]["touchesBand"]:
        assert band == 0
    return case, win, w, thr, band, single


def _scan_args(case):
    return case["geom"], case["angles"], case["ranges"], case["rel_pose"], case["init_pose"]


def _marked(records, band):
    return [dict(r, flags=r["flags"] | band) for r in records]


@pytest.mark.parametrize("name", V.NAMES)
def test_peaks(gpu_ctx, name):
    c = V.BY_NAME[name]
    case, win, w, thr, band, single = _window(gpu_ctx, name)
    ref = _marked(V.peaks(name), band)
    assert 1 <= len(ref) <= K_MAX
    got = gpu_ctx.score_window_peaks(MAP, w, win["col"], win["row"], K_MAX, EXCL)
    assert got == ref                   # field by field, score bits included; the list ends where the reference's does
    if not single["flags"] & NOT_CLOSED_FORM:
        assert got[0] == single
    rng = V.search_range(c)
    out = gpu_ctx.correlative_peaks(MAP, *_scan_args(case), *rng, c["L"], K_MAX, EXCL, known_rate_threshold=thr)
    assert [o["raw"] for o in out] == ref
    for o, r in zip(out, ref):
        best, est = PR.poses_of(r, win, case["rel_pose"])
        assert o["best_sensor_pose"] == best and o["estimated_pose"] == est       # bit-exact doubles
        assert (o["win_x"], o["win_y"], o["win_theta"]) == win["win"]
        assert o["candidates"] == int(np.prod(win["shape"]))
    m = gpu_ctx.correlative_match(MAP, *_scan_args(case), *rng, c["L"], 0.0, thr)
    if not m["raw"]["flags"] & NOT_CLOSED_FORM:
        assert out[0]["raw"] == dict(m["raw"], flags=m["raw"]["flags"] & ~Lb.FLAG_PROJ_DELTA)
        assert out[0]["estimated_pose"] == m["estimated_pose"]
    gpu_ctx.release_grid(MAP)


@pytest.mark.parametrize("name", V.NAMES)
def test_covariance(gpu_ctx, name):
    c = V.BY_NAME[name]
    case, win, w, thr, band, _ = _window(gpu_ctx, name)
    for tau in TAUS:
        ref = V.summary(name, tau)
        got = gpu_ctx.score_window_moments(MAP, w, win["col"], win["row"], tau)
        assert got == TV._with_band(ref["moments"], band)
        out = gpu_ctx.correlative_covariance(MAP, *_scan_args(case), *V.search_range(c), c["L"], tau,
                                             known_rate_threshold=thr)
        TV._check_summary(out, ref, win, case, band)
        if "one" in c["props"]:         # the winner alone: full weight, no spread
            assert got["m0"] == 1 << 24 and got["m1"] == [0] * 3 and got["m2"] == [0] * 6 and got["support"] == 1
            assert out["covariance"] == [0.0] * 9 and out["sensor_covariance"] == [0.0] * 9
    gpu_ctx.release_grid(MAP)


@pytest.mark.parametrize("name", V.NAMES)
def test_prior(gpu_ctx, name):
    c = V.BY_NAME[name]
    case, win, w, thr, band, _ = _window(gpu_ctx, name)
    peak0 = gpu_ctx.score_window_peaks(MAP, w, win["col"], win["row"], 1)[0]
    for lam_name, lam in LAMBDAS.items():
        ref, _ = V.prior(name, lam_name)
        got = gpu_ctx.score_window_prior(MAP, w, win["col"], win["row"], lam, win["steps"])
        assert got == TP._with_band(ref, band)
        assert got["unweighted"] == peak0
        out = gpu_ctx.correlative_match_prior(MAP, *_scan_args(case), *V.search_range(c), c["L"], lam,
                                              known_rate_threshold=thr)
        TP._check_summary(out, ref, win, case, band)
    gpu_ctx.release_grid(MAP)


strip = lambda o: {k: v for k, v in o.items() if not k.endswith("_us")}


def test_one_chunk_holds_windows_of_one_and_of_256_workgroups():
    """One call of every batched entry over windows of 108, 2,247,700, 612 and 108 candidates: the search
    range is one per call, so the sizes come from the maps' cell sizes (0.05 m and 1.6 m) and the scans'
    maximum ranges (1 m and 20 m on the coarse map). All of them fit the default scratch limit, so they share
    one chunk, whose launches are (256, 4) workgroups: 255 of them return at once for three of the windows,
    next to a window that uses all 256."""
    names = ["batch_short", "big_L2", "batch_long", "batch_short"]
    base = api.debug_live_bytes()
    ctx = api.Context(0)
    maps = {"coarse_short": MAP + 1, "coarse_long": MAP + 1, "big120": MAP + 2}
    ctx.upload_grid(MAP + 1, V.scan_case("coarse_short")["grid"])
    ctx.upload_grid(MAP + 2, V.scan_case("big120")["grid"])
    cases = [V.volume(n)[0] for n in names]
    wins = [V.volume(n)[1]["win"] for n in names]
    queries = [dict(map_id=maps[V.BY_NAME[n]["maker"]], geom=c["geom"], angles=c["angles"], ranges=c["ranges"],
                    rel_pose=c["rel_pose"], init_pose=c["init_pose"]) for n, c in zip(names, cases)]
    rng, L = V.BATCH_RANGE, V.BATCH_L
    assert [int(np.prod(w["shape"])) for w in wins] == [108, 2247700, 612, 108]
    before = ctx.correlative_match_batch(queries, *rng, L, 0.0, 0.0)
    bands = [b["raw"]["flags"] & Lb.FLAG_EDGE_BAND for b in before]

    def one_chunk(timer, call):
        ctx.enable_kernel_timing(True)
        ctx.reset_kernel_timing()
        got = call()
        chunks = ctx.kernel_time(timer)[1]
        ctx.enable_kernel_timing(False)
        assert chunks == 1
        return got

    got = one_chunk("peaks_select", lambda: ctx.correlative_peaks_batch(queries, *rng, L, K_MAX, EXCL))
    for n, q, c, g, band in zip(names, queries, cases, got, bands):
        assert [o["raw"] for o in g] == _marked(V.peaks(n), band)
        one = ctx.correlative_peaks(q["map_id"], *_scan_args(c), *rng, L, K_MAX, EXCL)
        assert [strip(o) for o in g] == [strip(o) for o in one]

    tau = TAUS[1]
    got = one_chunk("volume_moments", lambda: ctx.correlative_covariance_batch(queries, *rng, L, tau))
    for n, q, c, w, g, band in zip(names, queries, cases, wins, got, bands):
        TV._check_summary(g, V.summary(n, tau), w, c, band)
        one = ctx.correlative_covariance(q["map_id"], *_scan_args(c), *rng, L, tau)
        assert dict(one, summary=strip(one["summary"])) == dict(g, summary=strip(g["summary"]))

    lams = [LAMBDAS[k] for k in ("full", "diag", "indef", "diag")]
    got = one_chunk("prior_select", lambda: ctx.correlative_match_prior_batch(queries, *rng, L, lams))
    for n, q, c, w, g, band, k in zip(names, queries, cases, wins, got, bands, ("full", "diag", "indef", "diag")):
        TP._check_summary(g, V.prior(n, k)[0], w, c, band)
        one = ctx.correlative_match_prior(q["map_id"], *_scan_args(c), *rng, L, LAMBDAS[k])
        assert dict(one, summary=strip(one["summary"])) == dict(g, summary=strip(g["summary"]))

    assert [strip(o) for o in ctx.correlative_match_batch(queries, *rng, L, 0.0, 0.0)] == [strip(o) for o in before]
    ctx.release_grid(MAP + 1)
    ctx.release_grid(MAP + 2)
    ctx.close()
    assert api.debug_live_bytes() == base


def test_large_tiny_large_on_one_context():
    """The workspaces shrink in use, not in size: behind the one workgroup record of a tiny window sit the
    255 stale ones of the large window before it. Every unit: large, tiny, large; the third equals the first."""
    base = api.debug_live_bytes()
    ctx = api.Context(0)
    seq = ["big_L2", "point_L2", "big_L2", "slab_L2", "big_ties_L2", "point_L1", "big_ties_L2"]
    ids = {n: MAP + 10 + i for i, n in enumerate(sorted(set(seq)))}
    sets = {n: _window(ctx, n, ids[n]) for n in ids}
    tau, lam = TAUS[1], "full"
    runs = {"peaks": [], "moments": [], "prior": []}
    for n in seq:
        case, win, w, thr, band, _ = sets[n]
        runs["peaks"].append(ctx.score_window_peaks(ids[n], w, win["col"], win["row"], K_MAX, EXCL))
        assert runs["peaks"][-1] == _marked(V.peaks(n), band)
    for n in seq:
        case, win, w, thr, band, _ = sets[n]
        runs["moments"].append(ctx.score_window_moments(ids[n], w, win["col"], win["row"], tau))
        assert runs["moments"][-1] == TV._with_band(V.summary(n, tau)["moments"], band)
    for n in seq:
        case, win, w, thr, band, _ = sets[n]
        runs["prior"].append(ctx.score_window_prior(ids[n], w, win["col"], win["row"], LAMBDAS[lam], win["steps"]))
        assert runs["prior"][-1] == TP._with_band(V.prior(n, lam)[0], band)
    for r in runs.values():
        assert r[0] == r[2] and r[4] == r[6] and r[0] != r[4]
    for m in ids.values():
        ctx.release_grid(m)
    ctx.close()
    assert api.debug_live_bytes() == base
