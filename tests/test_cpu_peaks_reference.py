"""CPU suite: the conditions the GPU peak tests (test_gpu_peaks.py) rest on, on the reference of
tests/peaks_reference.py alone: the six windows touch no edge band, hold four distinct peaks without a
key tie, and peak 0 is the literal sweep's winner."""
import math

import pytest

import peaks_reference as PR
from csm_hip import synth

CASES = [(0, 4), (1, 4), (2, 1), (3, 5), (4, 3), (5, 8)]
RANGE = (1.0, 1.0, math.radians(10))
K_MAX, EXCL = 4, (3, 3, 2)


@pytest.mark.parametrize("seed,L", CASES)
def test_six_cases_have_four_untied_peaks_and_the_literal_winner_first(oracle, seed, L):
    case = synth.csm_case(seed)
    rec, cf, win = PR.peaks(case, *RANGE, L, K_MAX, EXCL)
    assert cf["touchesBand"] == 0
    assert len(rec) == K_MAX
    assert [r["tie_count"] for r in rec] == [1] * K_MAX
    lit = oracle.csm(case, *RANGE, L)
    assert lit["found"] == 1
    assert (rec[0]["best_x"], rec[0]["best_y"], rec[0]["best_theta"]) == (lit["bestX"], lit["bestY"], lit["bestT"])
    assert rec[0]["score"] == lit["scoreMax"]       # bit-exact f64
    best, est = PR.poses_of(rec[0], win, case["rel_pose"])
    assert best == lit["bestSensorPose"] and est == lit["estimatedPose"]
    # distinct: no peak inside an earlier peak's exclusion box; keys never increase
    for j in range(1, K_MAX):
        for p in rec[:j]:
            assert (abs(rec[j]["best_x"] - p["best_x"]) > EXCL[0] or abs(rec[j]["best_y"] - p["best_y"]) > EXCL[1] or
                    abs(rec[j]["best_theta"] - p["best_theta"]) > EXCL[2])
        assert rec[j]["key"] <= rec[j - 1]["key"]


def test_plain_top_k_is_the_sorted_volume(oracle):
    """Exclusion (0, 0, 0): the peaks are the volume's candidates in descending key order."""
    case = synth.csm_case(2)
    rec, cf, win = PR.peaks(case, *RANGE, 1, 16, (0, 0, 0))
    _, S, K, _ = oracle.csm_closed_form(case, *RANGE, 1, dump=True)
    keys = sorted((32268 * K.astype("int64") + 499 * S.astype("int64")).ravel(), reverse=True)
    assert [r["key"] for r in rec] == [int(k) for k in keys[:16]]
