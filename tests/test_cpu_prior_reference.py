"""CPU suite: the host restatements of the motion prior (csm_host_motion_prior,
csm_host_prior_from_robot_information) against tests/prior_reference.py bit for bit, every refusal, and the
coverage of the GPU test's fixed inputs (tests/test_gpu_prior.py) on the reference alone. No GPU."""
import math

import numpy as np
import pytest

import prior_reference as P
from csm_hip import _lib as Lb, api
from test_gpu_prior import CASES, LAMBDAS, RANGE, _six

STEPS = (0.05, 0.05, 0.008726640368449268)
N, D_MAX = 360, 24


def sym(xx, yy, tt, xy=0.0, xt=0.0, yt=0.0):
    return np.array([[xx, xy, xt], [xy, yy, yt], [xt, yt, tt]], np.float64)


# 6 max|Q| d_max^2 < 2^62 with Q_xx = (N / c) 0.5 Lambda_xx step_x^2 256: the largest Lambda_xx that passes
BOUND_XX = (1 << 62) / (6.0 * D_MAX * D_MAX) / ((N / P.C_KEY) * 0.5 * STEPS[0] * STEPS[0] * 256.0)

LADDER = [
    sym(2.0, 2.0, 40.0),                                    # diagonal
    sym(3.0, 2.0, 60.0, 1.0, 4.0, -3.0),                    # full
    sym(0.0, 0.0, 0.0),                                     # zero
    sym(1.5, 1.5, 20.0, 2.5),                               # one negative eigenvalue
    sym(1e-7, 3e-9, 1e-5, -2e-8),                           # entries that quantise to a few units, or to 0
    sym(0.999 * BOUND_XX, 1.0, 1.0),                        # just inside the refusal bound
    sym(-0.999 * BOUND_XX, 1.0, 1.0, 0.25 * BOUND_XX),      # ... with a negative entry
]


@pytest.mark.parametrize("lam", LADDER)
def test_quantisation_equals_the_reference_bit_for_bit(lam):
    want = P.quantise(lam, STEPS, N, D_MAX)
    assert want is not None
    assert api.host_motion_prior(lam, STEPS, N, D_MAX) == want
    if not lam.any():
        assert want == [0] * 6
    # another beam count and other steps: the expression, not a table
    steps = (0.04, 0.06, 0.0123)
    if P.quantise(lam, steps, 1080, 7) is not None:
        assert api.host_motion_prior(lam, steps, 1080, 7) == P.quantise(lam, steps, 1080, 7)


def test_one_negative_eigenvalue_is_allowed_and_clamps():
    lam = LADDER[3]
    assert np.linalg.eigvalsh(lam).min() < 0
    Q = api.host_motion_prior(lam, STEPS, N, D_MAX)
    assert P.quad_form(Q, 3, -3, 0) < 0 and P.penalty(Q, 3, -3, 0) == 0 and P.penalty(Q, 3, 3, 0) > 0


def _refused(fn):
    with pytest.raises(api.CsmError) as e:
        fn()
    return e.value.code


def test_every_refusal_is_einval():
    good = LADDER[1]
    bad = []
    for v in (float("nan"), float("inf"), -float("inf")):
        m = good.copy()
        m[1, 1] = v
        bad.append(m)
    asym = good.copy()
    asym[0, 2] = np.nextafter(asym[0, 2], 10.0)             # one ulp apart is asymmetric
    bad.append(asym)
    bad.append(sym(1e30, 1.0, 1.0))                         # q * 256 beyond int64
    bad.append(sym(1.0, 1.0, 1.0, -1e30))
    bad.append(sym(1.001 * BOUND_XX, 1.0, 1.0))             # just past the range bound
    bad.append(sym(1.0, 1.0, 1.0, 0.0, 0.0, -1e9))          # ... by a negative off-diagonal entry
    for m in bad:
        assert P.quantise(m, STEPS, N, D_MAX) is None
        assert _refused(lambda: api.host_motion_prior(m, STEPS, N, D_MAX)) == Lb.CSM_EINVAL
    # the bound moves with d_max: what a window of 25 takes, one of 2001 refuses
    edge = sym(0.5 * BOUND_XX, 1.0, 1.0)
    assert api.host_motion_prior(edge, STEPS, N, D_MAX) == P.quantise(edge, STEPS, N, D_MAX)
    assert P.quantise(edge, STEPS, N, 2000) is None
    assert _refused(lambda: api.host_motion_prior(edge, STEPS, N, 2000)) == Lb.CSM_EINVAL
    assert _refused(lambda: api.host_motion_prior(good, STEPS, 0, D_MAX)) == Lb.CSM_EINVAL
    assert _refused(lambda: api.host_motion_prior(good, STEPS, N, -1)) == Lb.CSM_EINVAL
    assert _refused(lambda: api.host_motion_prior(good, (0.05, float("nan"), 0.01), N, D_MAX)) == Lb.CSM_EINVAL
    assert _refused(lambda: api.host_motion_prior(good[:2], STEPS, N, D_MAX)) == Lb.CSM_EINVAL


@pytest.mark.parametrize("lam", LADDER[:5])
@pytest.mark.parametrize("rel", [(0.0, 0.0, 0.0), (0.21, -0.13, 0.3), (-0.4, 0.05, -1.3)])
def test_robot_information_transform_equals_the_reference_bit_for_bit(lam, rel):
    init = (1.25, -0.5, 0.7853)
    got = api.host_prior_from_robot_information(lam, init, rel)
    assert got == P.sensor_information(lam, init, rel)        # lists of floats: equal means bit-equal
    assert all(got[3 * a + b] == got[3 * b + a] for a in range(3) for b in range(3))
    if not any(rel[:2]):
        assert got == lam.reshape(-1).tolist()
    elif lam[0, 0] != 0.0:
        assert got[8] != lam[2, 2]                            # J moved x / y information into theta
    # what it returns is a prior the quantisation takes
    assert api.host_motion_prior(got, STEPS, N, D_MAX) == P.quantise(got, STEPS, N, D_MAX)


def test_the_gpu_inputs_cover_every_regime():
    """On the reference alone: the six cases under the GPU test's information matrices reach a winner the
    prior moved (to neither the unweighted winner nor the window centre), a winner it left in place at a
    price, and a window where the max(0, .) clamp acts."""
    moved = kept = clamp = 0
    for seed, L in CASES:
        for name in LAMBDAS:
            ref, clamped = _six(seed, L, name)[2:]
            b, u = ref["best"], ref["unweighted"]
            assert b["found"] == 1 and u["found"] == 1
            d = (b["best_x"], b["best_y"], b["best_theta"])
            moved += b != u and d != (0, 0, 0)
            kept += b == u and ref["penalty"] > 0
            clamp += clamped > 0
            if name == "zero":
                assert b == u and ref["penalty"] == 0 and ref["penalised_key"] == b["key"]
    assert moved >= 1 and kept >= 1 and clamp >= 1
