"""CPU suite: the host restatements of the volume covariance (csm_host_volume_weights,
csm_host_volume_covariance) against their definition in include/csm_hip.h, and tests/volume_reference.py on
the oracle's dumps. No GPU."""
import math

import numpy as np
import pytest

import volume_reference as VR
from csm_hip import _lib as Lb, api, synth

C_KEY = 0.998 / (65534 * 499)


@pytest.mark.parametrize("n", [8, 360, 1080])
@pytest.mark.parametrize("tau", [0.005, 0.02, 0.05])
def test_weight_table_follows_the_formula(n, tau):
    W, shift = api.host_volume_weights(n, tau)
    assert W.dtype == np.uint32 and W.shape == (Lb.VOLUME_BINS,)
    assert int(W[0]) == 1 << 24
    assert (np.diff(W.astype(np.int64)) <= 0).all()
    band = int(math.ceil(17.0 * tau * n / C_KEY))
    assert (band >> shift) < Lb.VOLUME_BINS and (shift == 0 or (band >> (shift - 1)) >= Lb.VOLUME_BINS)
    b = np.arange(Lb.VOLUME_BINS, dtype=np.int64)
    want = np.floor(2.0 ** 24 * np.exp(-((b << shift).astype(np.float64) * C_KEY) / (n * tau)) + 0.5)
    assert np.abs(W.astype(np.int64) - want.astype(np.int64)).max() <= 1
    assert int(W[-1]) <= 2         # the band ends where the weight does: 2^24 exp(-17) < 1


def test_weight_table_refuses_bad_temperatures():
    for tau in (0.0, -0.01, float("nan"), float("inf"), 1e60):
        with pytest.raises(api.CsmError) as e:
            api.host_volume_weights(360, tau)
        assert e.value.code == Lb.CSM_EINVAL
    with pytest.raises(api.CsmError):
        api.host_volume_weights(0, 0.02)


STEPS = (0.05, 0.05, 0.004363323129985824)
HAND_MADE = [
    # plain
    (dict(m0=5 << 24, m1=[3 << 24, 1 << 24, 0], m2=[9 << 24, 2 << 24, 1 << 20, 7 << 24, 0, 3 << 24]), (0.0, 0.0, 0.0)),
    # negative first moments (a winner in the far corner), a non-zero relative sensor pose
    (dict(m0=123456789012, m1=[-98765432101, -5555555555, -777777777],
          m2=[987654321098, 55555555555, -4444444444, 66666666666, 3333333333, 2222222222]), (0.31, -0.12, 0.4)),
    # m0 * m2 beyond 2^64: exact only in 128 bits
    (dict(m0=(1 << 40) + 12345, m1=[(1 << 41) + 7, -(1 << 39) - 3, 1 << 30],
          m2=[(1 << 45) + 99991, -(1 << 41) + 17, (1 << 33) + 5, (1 << 44) + 3, -(1 << 35) - 1, (1 << 40) + 11]),
     (-0.2, 0.05, -1.3)),
    # a support of one candidate: the winner alone
    (dict(m0=1 << 24, m1=[0, 0, 0], m2=[0] * 6), (0.1, 0.2, 0.3)),
]


assert HAND_MADE[2][0]["m0"] * HAND_MADE[2][0]["m2"][0] > 1 << 64 and min(HAND_MADE[1][0]["m1"]) < 0


@pytest.mark.parametrize("m,rel", HAND_MADE)
def test_covariance_equals_the_python_integer_form_bit_for_bit(m, rel):
    est = (1.25, -0.5, 0.7853)
    got = api.host_volume_covariance(m, STEPS, est, rel)
    want = VR.covariance(m, STEPS, est, rel)
    assert got == want                 # lists of floats: equal means bit-equal (no NaN here)
    mean, scov, cov = got
    assert all(scov[3 * a + b] == scov[3 * b + a] for a in range(3) for b in range(3))
    if m["m0"] == 1 << 24 and not any(m["m2"]):
        assert mean == [0.0] * 3 and scov == [0.0] * 9 and cov == [0.0] * 9
    else:
        assert scov[0] != 0.0
    if any(rel[:2]) and scov[8] != 0.0:
        assert cov != scov             # J moved the theta variance into x and y


def test_zero_mass_gives_zeros():
    got = api.host_volume_covariance(dict(m0=0, m1=[0, 0, 0], m2=[0] * 6), STEPS, (0.0, 0.0, 0.3), (0.1, 0.0, 0.0))
    assert got == ([0.0] * 3, [0.0] * 9, [0.0] * 9)


@pytest.mark.parametrize("tau", [0.005, 0.02])
def test_reference_moments_on_the_oracle_dump(tau):
    case = synth.csm_case(0)
    ref, win = VR.summary(case, 1.0, 1.0, math.radians(10), 4, tau)
    m = ref["moments"]
    assert m["best"]["found"] == 1 and m["m0"] >= 1 << 24 and m["support"] >= 1
    assert 0 <= m["border_support"] <= m["support"] <= int(np.prod(win["shape"]))
    scov, cov = ref["sensor_covariance"], ref["covariance"]
    # symmetric: the sensor covariance exactly (it is mirrored), J S J^T to rounding
    assert all(scov[3 * a + b] == scov[3 * b + a] for a in range(3) for b in range(3))
    tol = 8 * 2.0 ** -52 * max(map(abs, cov))      # an entry is two sums of three products: a few ulps of the largest
    assert all(abs(cov[3 * a + b] - cov[3 * b + a]) <= tol for a in range(3) for b in range(3))
    assert all(scov[4 * a] >= 0.0 for a in range(3))
    # the host export on the same moments: the covariance the device entries return
    assert api.host_volume_covariance(m, win["steps"], ref["estimated_pose"], case["rel_pose"]) == \
        (ref["mean_offset"], scov, cov)
