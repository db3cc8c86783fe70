"""CPU suite: the host restatements of the likelihood field (csm_host_likelihood_kernel,
csm_host_likelihood_radius, csm_host_likelihood_map) against tests/likelihood_reference.py, equal byte for
byte; the properties the definition promises; every refusal. No GPU."""
import ctypes as C

import numpy as np
import pytest

import likelihood_reference as LR
from csm_hip import _lib as Lb, api


@pytest.mark.parametrize("sigma,res,R", [(0.05, 0.05, 3), (0.05, 0.05, 1), (0.25, 0.05, 16), (0.1, 0.05, 6),
                                         (0.03, 0.1, 2), (0.0123, 0.05, 5), (2.0, 0.05, 16), (0.001, 0.05, 4)])
def test_kernel_table_equals_the_python_table(sigma, res, R):
    got = api.host_likelihood_kernel(sigma, res, R)
    want = LR.kernel(sigma, res, R)
    assert got.dtype == np.uint32 and got.tolist() == want.tolist()
    assert got[0] == 32768
    assert (np.diff(got.astype(np.int64)) <= 0).all()


def test_radius_and_its_clamps():
    for sigma, res in [(0.05, 0.05), (0.25, 0.05), (0.1, 0.05), (0.0001, 0.05), (5.0, 0.05), (0.08, 0.05),
                       (0.26666, 0.05), (0.2667, 0.05), (1e-300, 1.0), (1e300, 1e-300)]:
        assert api.host_likelihood_radius(sigma, res) == LR.radius(sigma, res), (sigma, res)
    assert api.host_likelihood_radius(0.05, 0.05) == 3
    assert api.host_likelihood_radius(0.0001, 0.05) == 1             # clamped from below
    assert api.host_likelihood_radius(5.0, 0.05) == 16               # ... and from above
    assert api.host_likelihood_radius(0.25, 0.05) == 15


@pytest.mark.parametrize("keep_unknown", [False, True])
@pytest.mark.parametrize("name,R", LR.CPU_CASES)
def test_host_map_equals_the_reference(name, R, keep_unknown):
    g, t, want = LR.expected(name, R, keep_unknown)
    occ = LR.occupied_min_of(name)
    got = api.host_likelihood_map(g, radius=R, occupied_min=occ, keep_unknown=keep_unknown, kernel=t)
    assert got.dtype == np.uint16 and got.shape == g.shape
    assert np.array_equal(got, want)
    assert int(got.max(initial=0)) <= 65534
    far = LR.far_from_obstacles(g, R, occ)
    assert np.array_equal(got[far], g[far])                          # no obstacle within R: unchanged
    assert (got >= g).all()
    if keep_unknown:
        assert not got[g == 0].any()
    assert int(got.max(initial=0)) == int(g.max(initial=0))           # T <= 32768: nothing above the largest value


def test_the_cases_cover_what_they_claim():
    g, _, out = LR.expected("csm_case0", 3, False)
    changed = out != g
    assert changed.sum() > 3000 and (changed & (g == 0)).sum() > 1000    # a do-nothing build cannot pass
    _, _, kept = LR.expected("csm_case0", 3, True)
    assert (kept != out).sum() > 1000                                    # ... nor one that ignores keep_unknown
    g, _, out = LR.expected("threshold", 3, False)
    assert out[4, 5] > g[4, 5] and out[4, 31] == g[4, 31] and out[19, 6] > 0
    assert LR.expected("threshold", 3, True)[2][19, 6] == 0
    g, _, out = LR.expected("extremes", 3, False)
    assert out[15, 16] > 1 and out[3, 4] == 1 and out[15, 15] == 65534
    assert not LR.expected("all_unknown", 3, False)[2].any()
    g, _, out = LR.expected("all_obstacle", 3, False)
    assert np.array_equal(out, g)
    g, _, out = LR.expected("corners", 16, False)
    assert out[1, 1] > 0 and out[-2, -2] > 0 and out[1, -2] > 0 and out[-2, 1] > 0
    for name, _ in LR.CPU_CASES + LR.GPU_EXTRA_CASES:
        assert int(LR.grid_of(name).max(initial=0)) <= 65534


def test_default_table_and_radius_come_from_sigma():
    g = LR.grid_of("random37x53")
    got = api.host_likelihood_map(g, 0.05, 0.05)
    want = LR.likelihood_map(g, LR.kernel(0.05, 0.05, 3), 3)
    assert np.array_equal(got, want)


def test_argument_errors_return_their_codes():
    lib = Lb.load()
    g = np.ascontiguousarray(LR.grid_of("random16"))
    out = np.zeros_like(g)
    table = LR.kernel(0.05, 0.05, 3)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def run(radius=3, occupied_min=32768, kernel=table, rows=16, cols=16, grid=g, dst=out):
        p = Lb.LikelihoodParams(radius, occupied_min, 0, 0, None if kernel is None else kernel.ctypes.data)
        return lib.csm_host_likelihood_map(None if grid is None else ptr(grid), rows, cols, C.byref(p),
                                           None if dst is None else ptr(dst))

    assert run() == Lb.CSM_OK
    for bad in (dict(radius=0), dict(radius=17), dict(radius=-1), dict(occupied_min=0), dict(kernel=None),
                dict(rows=0), dict(cols=0), dict(grid=None), dict(dst=None)):
        assert run(**bad) == Lb.CSM_EINVAL, bad
    over = table.copy()
    over[9] = 32769
    assert run(kernel=over) == Lb.CSM_EINVAL
    over[9] = 32768
    assert run(kernel=over) == Lb.CSM_OK
    assert lib.csm_host_likelihood_map(ptr(g), 16, 16, None, ptr(out)) == Lb.CSM_EINVAL

    t = np.zeros(300, np.uint32)
    for sigma, res, R in [(0.0, 0.05, 3), (-1.0, 0.05, 3), (0.05, 0.0, 3), (float("nan"), 0.05, 3),
                          (0.05, float("inf"), 3), (0.05, 0.05, 0), (0.05, 0.05, 17)]:
        assert lib.csm_host_likelihood_kernel(sigma, res, R, ptr(t)) == Lb.CSM_EINVAL
    assert lib.csm_host_likelihood_kernel(0.05, 0.05, 3, None) == Lb.CSM_EINVAL
    for sigma, res in [(0.0, 0.05), (0.05, 0.0), (float("nan"), 0.05), (float("inf"), 0.05), (-0.1, 0.05)]:
        assert lib.csm_host_likelihood_radius(sigma, res) == Lb.CSM_EINVAL
        with pytest.raises(api.CsmError):
            api.host_likelihood_radius(sigma, res)
