"""The scale of the bound pass's key copy (csm_joint_kernels.hip, kKeyScaleLog2), without a GPU, in
numpy float32: a beam count n = 1 .. 15 is used as the fp32 denormal with bit pattern n (n 2^-149)
against key 2^S, and the sum is scaled back by 2^(149 - S) once per candidate. That must give what
key * float(n) gave, bit for bit, and every accumulator value must be a normal, finite float."""
import re
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "my-lidar-graph-slam-v2_amd", "csrc", "csm_joint_kernels.hip")


def _scale_log2():
    with open(SRC) as f:
        m = re.search(r"constexpr int kKeyScaleLog2 = (\d+);", f.read())
    return int(m.group(1))


def _key(v):
    v = np.asarray(v, dtype=np.uint64)
    return (499 * v + 32268 * np.minimum(v, 1)).astype(np.uint32)


def _pow2(e):
    return np.float32(2.0) ** np.float32(e)


def test_scale_is_what_the_design_states():
    assert _scale_log2() == 100


def test_denormal_count_times_scaled_key_is_exact():
    S = _scale_log2()
    rng = np.random.RandomState(3)
    vals = np.concatenate([[0, 1, 2, 255, 256, 32767, 65534, 65535], rng.randint(0, 65536, 1000)])
    keyf = _key(vals).astype(np.float32)                      # the one rounding of the key copy
    scaled = keyf * _pow2(S)
    assert np.all(np.isfinite(scaled))
    assert np.array_equal((scaled * _pow2(-S)).view(np.uint32), keyf.view(np.uint32))   # the scale is exact
    with np.errstate(under="raise", over="raise"):
        for n in range(1, 16):
            den = np.array([n], dtype=np.uint32).view(np.float32)[0]
            assert den == np.float32(n) * _pow2(-100) * _pow2(-49)                  # n 2^-149
            got = (scaled * den) * _pow2(149 - S)
            want = keyf * np.float32(n)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), n
            # fused multiply-add, as the kernel: the product in double is exact (24 + 4 bits); one rounding
            # of acc + product in either scale
            acc = np.float32(12345678.0) * keyf[5]
            fma_want = (acc.astype(np.float64) + keyf.astype(np.float64) * n).astype(np.float32)
            acc_s = acc * _pow2(S - 149)
            fma_got = (acc_s.astype(np.float64) + scaled.astype(np.float64) * np.float64(den)).astype(np.float32)
            assert np.array_equal((fma_got * _pow2(149 - S)).view(np.uint32), fma_want.view(np.uint32)), n


def test_accumulator_range_is_normal_and_finite():
    S = _scale_log2()
    tiny = np.finfo(np.float32).tiny                          # 2^-126
    den1 = np.array([1], dtype=np.uint32).view(np.float32)[0]
    smallest = (np.float32(_key(1)) * _pow2(S)) * den1        # one beam on a cell of value 1
    assert smallest >= tiny and smallest == np.float32(32767.0) * _pow2(S - 149)
    # the greatest sum: kMaxPoints = 10240 beams, each on a cell of value 65535 (< 2^14 2^25 in key units)
    largest = np.float32(10240.0 * float(_key(65535))) * _pow2(S - 149)
    assert np.isfinite(largest) and tiny <= largest < _pow2(39 + S - 149)
    assert np.isfinite(np.float32(_key(65535)) * _pow2(S))    # the scaled key copy itself
    assert float(_key(65535)) < 2.0 ** 25
    assert 9 <= S <= 102
