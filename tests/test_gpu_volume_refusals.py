"""GPU: which refusal wins when an input is bad in two ways, across the nine entries that read a window's
whole score volume -- (named window, single query, query batch) x (peaks, covariance, prior). The per-unit
refusal tests (test_gpu_peaks, test_gpu_volume_cov, test_gpu_prior) stay; this file pins the precedence
between the refusals, which the entries share through one host driver.

Every cell: the return code and the message's distinctive words, debug_live_bytes() unchanged, no launch of
peaks_coarse / peaks_select / prior_select / volume_moments, and the same entry's next good call equal to its
reference (peaks_reference / volume_reference / prior_reference).

Rows: (a) map not resident; (b) even n_theta / a NaN range; (c) a scratch limit below the volume; (d) a named
level out of range, of another box size, or stale; (e) = (a) + (b); (f) = (a) + (d); (g) = (a) + the unit's own
bad parameter (k_max = 0, temperature = 0, an asymmetric information matrix); (h) = (a) + a negative limit.
Two rows are not what one might guess:
  - (c): the window's volume is 3 x 6 x 6 candidates: 512 + 256 + 256 = 1024 bytes (S, K, coarse K, each padded
    to 256). A limit refuses a volume that does not FIT (csm_peaks_params.scratch_limit_bytes), so 1024 is
    accepted and 1023 is the greatest refusing limit: the row uses 1023 and checks that 1024 is taken.
  - (g): the prior looks at the information matrix only once the window is sized (named window: params -> size
    -> quantise -> level; queries: the pre-pass leaves a query whose map is not resident to the set-up). An
    asymmetric matrix on a map that is not resident is therefore CSM_ENOENT; (h) is the parameter refusal
    that comes first in all nine."""
import math
import types

import numpy as np
import pytest

import peaks_reference as PR
import prior_reference as P
import volume_reference as VR
from csm_hip import _lib as Lb, api, synth
from test_gpu_peaks import _vol_bytes

pytestmark = pytest.mark.gpu

MAP, STALE, GONE = 1300, 1301, 1399
L = 2
K_MAX, EXCL, TAU = 3, (1, 1, 0), 0.02
LAMBDA = np.array([[3.0, 1.0, 4.0], [1.0, 2.0, -3.0], [4.0, -3.0, 60.0]])
ASYM = LAMBDA + np.array([[0.0, 1e-9, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
UNITS = ("peaks", "covariance", "prior")
KINDS = ("named", "single", "batch")
TIMERS = ("peaks_coarse", "peaks_select", "prior_select", "volume_moments")

EINVAL, ENOENT = Lb.CSM_EINVAL, Lb.CSM_ENOENT
OWN = {"peaks": "k_max must be", "covariance": "temperature must be", "prior": "not resident"}


@pytest.fixture(scope="module")
def fx():
    """One 64 x 64 map, one scan of 8 beams, one window: 3 slices, win_x = win_y = 2 at L = 2. The references
    are computed once and never changed."""
    case = synth.csm_case(0, rows=64, cols=64, n_beams=8, max_range=2.0, init_error=(0.04, -0.03, 0.0),
                          rel_pose=(0.05, -0.02, 0.1))
    _, _, st = api.host_search_step(case["geom"][0], case["ranges"])
    rng = (0.19, 0.19, st)
    peaks, cf, win = PR.peaks(case, *rng, L, K_MAX, EXCL)
    cov, _ = VR.summary(case, *rng, L, TAU)
    prior = P.prior(P.volume(case, *rng, L), case, LAMBDA)[0]
    assert win["win"] == (2, 2, 1) and win["shape"] == (3, 6, 6) and len(case["angles"]) == 8
    assert cf["touchesBand"] == 0 and len(peaks) == K_MAX and cov["moments"]["best"]["found"] == 1
    assert _vol_bytes(win["shape"], L) == 1024
    ctx = api.Context(0)
    ctx.enable_kernel_timing(True)
    ctx.upload_grid(MAP, case["grid"])
    ctx.build_pyramid(MAP, [1, L, 3])           # level 1: box-max(2), level 2: box-max(3)
    # a map whose named level went stale: an update after the pyramid
    ctx.upload_grid(STALE, case["grid"])
    ctx.build_pyramid(STALE, [1, L])
    shape = dict(res=case["geom"][0], off_x=case["geom"][1], off_y=case["geom"][2], rows=64, cols=64, log2_block=4)
    node = dict(pose=case["truth"], angles=case["angles"], ranges=np.minimum(case["ranges"], 1.0),
                rel_pose=(0.0, 0.0, 0.0), min_range=0.05, max_range=2.0)
    ctx.update_map_with_scan(STALE, shape, (0.0, 0.0, 0.0), node)
    query = dict(map_id=MAP, geom=case["geom"], angles=case["angles"], ranges=case["ranges"],
                 rel_pose=case["rel_pose"], init_pose=case["init_pose"])
    f = types.SimpleNamespace(ctx=ctx, case=case, rng=rng, win=win, query=query,
                              ref=dict(peaks=peaks, covariance=cov, prior=prior))
    for unit in UNITS:                          # the workspaces at their size
        for kind in KINDS:
            _good(f, unit, kind)
    yield f
    ctx.close()


def _window(f, n_theta=3, level=1):
    n = len(f.case["angles"])
    return f.ctx.make_window(n_theta, n, 2, 2, L, level, api.host_min_known(n, 0.0), 0.0)


def _named(f, unit, map_id=MAP, w=None, limit=0, own_bad=False):
    w, col, row = w or _window(f), f.win["col"], f.win["row"]
    if unit == "peaks":
        return f.ctx.score_window_peaks(map_id, w, col, row, 0 if own_bad else K_MAX, EXCL, limit)
    if unit == "covariance":
        return f.ctx.score_window_moments(map_id, w, col, row, 0.0 if own_bad else TAU, limit)
    return f.ctx.score_window_prior(map_id, w, col, row, ASYM if own_bad else LAMBDA, f.win["steps"], limit)


def _queries(f, unit, kind, bad=None, limit=0, own_bad=False, lams=None):
    """The single-query entry on `bad` (the good query if None), or the batch entry on [good, bad]; one
    output per query."""
    qs = [bad or f.query] if kind == "single" else [f.query, bad or f.query]
    c = f.ctx
    if unit == "peaks":
        k = 0 if own_bad else K_MAX
        if kind == "batch":
            return c.correlative_peaks_batch(qs, *f.rng, L, k, EXCL, scratch_limit_bytes=limit)
    elif unit == "covariance":
        k = 0.0 if own_bad else TAU
        if kind == "batch":
            return c.correlative_covariance_batch(qs, *f.rng, L, k, scratch_limit_bytes=limit)
    else:
        k = ASYM if own_bad else LAMBDA
        if kind == "batch":
            return c.correlative_match_prior_batch(qs, *f.rng, L, lams or [LAMBDA, k], scratch_limit_bytes=limit)
    q = qs[0]
    head = (q["map_id"], q["geom"], q["angles"], q["ranges"], q["rel_pose"], q["init_pose"], *f.rng, L, k)
    if unit == "peaks":
        return [c.correlative_peaks(*head, EXCL, scratch_limit_bytes=limit)]
    if unit == "covariance":
        return [c.correlative_covariance(*head, scratch_limit_bytes=limit)]
    return [c.correlative_match_prior(*head, scratch_limit_bytes=limit)]


def _good(f, unit, kind, limit=0):
    """The entry on good inputs equals its reference."""
    ref = f.ref[unit]
    if kind == "named":
        got = _named(f, unit, limit=limit)
        assert got == (ref["moments"] if unit == "covariance" else ref)
        return
    for out in _queries(f, unit, kind, limit=limit):
        if unit == "peaks":
            assert [o["raw"] for o in out] == ref
        elif unit == "covariance":
            assert out["moments"] == ref["moments"] and out["summary"]["estimated_pose"] == ref["estimated_pose"]
            assert [out[k] for k in ("mean_offset", "sensor_covariance", "covariance")] == \
                   [ref[k] for k in ("mean_offset", "sensor_covariance", "covariance")]
        else:
            assert out["prior"] == ref and out["summary"]["raw"] == ref["best"]


def _cell(f, unit, kind, call, code, words):
    """One cell of the table: the refusal, nothing allocated, nothing launched, the next good call right."""
    live = api.debug_live_bytes()
    launches = [f.ctx.kernel_time(t)[1] for t in TIMERS]
    with pytest.raises(api.CsmError) as e:
        call()
    assert (e.value.code, words in str(e.value)) == (code, True), str(e.value)
    assert api.debug_live_bytes() == live
    assert [f.ctx.kernel_time(t)[1] for t in TIMERS] == launches
    _good(f, unit, kind)
    assert api.debug_live_bytes() == live


def _nan(q):
    r = np.array(q["ranges"], np.float64)
    r[3] = float("nan")
    return dict(q, ranges=r)


def _gone(q):
    return dict(q, map_id=GONE)


@pytest.mark.parametrize("unit", UNITS)
def test_named_window_entries(fx, unit):
    cell = lambda call, code, words: _cell(fx, unit, "named", call, code, words)
    even = _window(fx, n_theta=2)
    cell(lambda: _named(fx, unit, map_id=GONE), ENOENT, "not resident")                                  # (a)
    cell(lambda: _named(fx, unit, w=even), EINVAL, "bad window")                                         # (b)
    cell(lambda: _named(fx, unit, limit=1023), EINVAL, "exceeds the scratch limit")                      # (c)
    _good(fx, unit, "named", limit=1024)                                            # the volume fits exactly
    for w, map_id in ((_window(fx, level=7), MAP), (_window(fx, level=-1), MAP), (_window(fx, level=2), MAP),
                      (_window(fx), STALE)):                                                             # (d)
        cell(lambda: _named(fx, unit, map_id=map_id, w=w), ENOENT, "does not hold box-max(2)")
    cell(lambda: _named(fx, unit, map_id=GONE, w=even), EINVAL, "bad window")                            # (e)
    cell(lambda: _named(fx, unit, map_id=GONE, w=_window(fx, level=7)), ENOENT, "not resident")          # (f)
    cell(lambda: _named(fx, unit, map_id=GONE, own_bad=True), ENOENT if unit == "prior" else EINVAL, OWN[unit])   # (g)
    cell(lambda: _named(fx, unit, map_id=GONE, limit=-1), EINVAL, "scratch limit")                       # (h)
    # what the unit checks once the window is sized comes before the level
    if unit == "prior":
        cell(lambda: _named(fx, unit, w=_window(fx, level=7), own_bad=True), EINVAL, "finite and symmetric")
        cell(lambda: _named(fx, unit, w=even, own_bad=True), EINVAL, "bad window")
    if unit == "covariance":
        huge = lambda **kw: fx.ctx.score_window_moments(kw.get("map_id", MAP), kw.get("w") or _window(fx),
                                                        fx.win["col"], fx.win["row"], 1e30)
        cell(lambda: huge(map_id=GONE), EINVAL, "weight band beyond 2^62")      # temperature -> size
        cell(lambda: huge(w=_window(fx, level=7)), EINVAL, "weight band beyond 2^62")


@pytest.mark.parametrize("kind", ("single", "batch"))
@pytest.mark.parametrize("unit", UNITS)
def test_query_entries(fx, unit, kind):
    cell = lambda call, code, words: _cell(fx, unit, kind, call, code, words)
    q = fx.query
    cell(lambda: _queries(fx, unit, kind, _gone(q)), ENOENT, "not resident")                             # (a)
    cell(lambda: _queries(fx, unit, kind, _nan(q)), EINVAL, "non-finite beam")                           # (b)
    cell(lambda: _queries(fx, unit, kind, limit=1023), EINVAL, "exceeds the scratch limit")              # (c)
    _good(fx, unit, kind, limit=1024)                                               # the volume fits exactly
    cell(lambda: _queries(fx, unit, kind, _gone(_nan(q))), EINVAL, "non-finite beam")                    # (e)
    cell(lambda: _queries(fx, unit, kind, _gone(q), own_bad=True), ENOENT if unit == "prior" else EINVAL,
         OWN[unit])                                                                                      # (g)
    cell(lambda: _queries(fx, unit, kind, _gone(q), limit=-1), EINVAL, "scratch limit")                  # (h)
    if unit == "prior":
        cell(lambda: _queries(fx, unit, kind, own_bad=True), EINVAL, "finite and symmetric")
    if kind != "batch":
        return
    # the units' pre-passes run over all queries before the set-up looks a map up: query 0's map is not
    # resident, query 1 carries the unit's refusal
    if unit == "prior":
        cell(lambda: fx.ctx.correlative_match_prior_batch([_gone(q), q], *fx.rng, L, [LAMBDA, ASYM]), EINVAL,
             "window 1: the prior's information")
    if unit == "covariance":
        cell(lambda: fx.ctx.correlative_covariance_batch([_gone(q), q], *fx.rng, L, 1e30), EINVAL,
             "query 0: temperature")
