"""Pose covariance read off a correlative window's whole score volume, from the CPU oracle's per-candidate
sums: the complete specification of csm_score_window_moments / csm_correlative_covariance
(include/csm_hip.h). numpy for the volume, Python integers for the moments, plain floats for the covariance.

Winner b = peak 0 of tests/peaks_reference.select. An eligible candidate weighs W[(key_b - key) >> bin_shift]
(0 past the table; W from api.host_volume_weights: glibc's exp, which numpy's need not equal to the last
bit). Moments over d = (x - x_b, y - y_b, t - t_b); covariance = J (m0 m2 - m1 m1^T) / m0^2 J^T in steps."""
import math

import numpy as np

import peaks_reference as PR
from csm_hip import _lib as Lb, api
from oracle import oracle as O

PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))       # xx xy xt yy yt tt


def moments_of(S, K, CK, L, best, wx, wy, wt, n_points, tau, known_thr=0.0):
    """The moments dict of a volume around the winner record `best` (None: nothing found)."""
    W, shift = api.host_volume_weights(n_points, tau)
    out = dict(best=PR_ZERO if best is None else best, m0=0, m1=[0, 0, 0], m2=[0] * 6, support=0, border_support=0,
               bin_shift=shift)
    if best is None:
        return out
    key = 32268 * K.astype(np.int64) + 499 * S.astype(np.int64)
    elig = np.ones(S.shape, bool)
    if L > 1:
        elig = np.repeat(np.repeat(CK.astype(np.float64) / float(n_points) > known_thr, L, 1), L, 2)
    bins = (best["key"] - key) >> shift
    assert (bins[elig] >= 0).all()
    w = np.where(elig & (bins < Lb.VOLUME_BINS), W[np.clip(bins, 0, Lb.VOLUME_BINS - 1)], 0).astype(np.int64)
    t, x, y = np.indices(S.shape)
    d = (x - (best["best_x"] + wx), y - (best["best_y"] + wy), t - (best["best_theta"] + wt))
    out["m0"] = int(w.sum())
    out["m1"] = [int((w * d[a]).sum()) for a in range(3)]
    out["m2"] = [int((w * d[a] * d[b]).sum()) for a, b in PAIRS]       # < 2^63 by the entry's range check
    face = [(i == 0) | (i == n - 1) for i, n in zip((t, x, y), S.shape)]
    out["support"] = int((w > 0).sum())
    out["border_support"] = int(((w > 0) & (face[0] | face[1] | face[2])).sum())
    return out


PR_ZERO = dict(found=0, best_x=0, best_y=0, best_theta=0, key=0, sum_values=0, known=0, tie_count=0, flags=0, score=0.0)


def covariance(m, steps, estimated_pose, rel_pose):
    """(mean_offset[3], sensor_covariance[9], covariance[9]): the header's expression, product by product."""
    mean, S = [0.0] * 3, [[0.0] * 3 for _ in range(3)]
    if m["m0"] > 0:
        m0 = float(m["m0"])
        for k, (a, b) in enumerate(PAIRS):
            num = m["m0"] * m["m2"][k] - m["m1"][a] * m["m1"][b]          # Python integers: exact
            S[a][b] = S[b][a] = ((float(num) / (m0 * m0)) * steps[a]) * steps[b]
        mean = [(float(m["m1"][a]) / m0) * steps[a] for a in range(3)]
    sn, cs = math.sin(estimated_pose[2]), math.cos(estimated_pose[2])
    J = [[1.0, 0.0, sn * rel_pose[0] + cs * rel_pose[1]], [0.0, 1.0, -cs * rel_pose[0] + sn * rel_pose[1]],
         [0.0, 0.0, 1.0]]
    T = [[(J[i][0] * S[0][j] + J[i][1] * S[1][j]) + J[i][2] * S[2][j] for j in range(3)] for i in range(3)]
    C = [[(T[i][0] * J[j][0] + T[i][1] * J[j][1]) + T[i][2] * J[j][2] for j in range(3)] for i in range(3)]
    return mean, [v for r in S for v in r], [v for r in C for v in r]


def moments(case, rx, ry, rt, L, tau, score_thr=0.0, known_thr=0.0):
    """(moments dict, closed-form result dict, window dict) of the case."""
    cf, S, K, CK = O.csm_closed_form(case, rx, ry, rt, L, score_thr, known_thr, dump=True)
    (wx, wy, wt), steps, sensor, col, row = PR.window_of(case, rx, ry, rt)
    rec = PR.select(S, K, CK, L, case["grid"], col, row, wx, wy, wt, 1, (0, 0, 0), score_thr, known_thr)
    win = dict(win=(wx, wy, wt), steps=steps, sensor=sensor, col=col, row=row, shape=S.shape)
    m = moments_of(S, K, CK, L, rec[0] if rec else None, wx, wy, wt, len(case["angles"]), tau, known_thr)
    return m, cf, win


def summary(case, rx, ry, rt, L, tau, score_thr=0.0, known_thr=0.0):
    """What csm_correlative_covariance returns beyond its csm_summary: moments, mean_offset,
    sensor_covariance, covariance, estimated_pose (all zeros / None when nothing is found)."""
    m, cf, win = moments(case, rx, ry, rt, L, tau, score_thr, known_thr)
    if not m["best"]["found"]:
        return dict(moments=m, mean_offset=[0.0] * 3, sensor_covariance=[0.0] * 9, covariance=[0.0] * 9,
                    estimated_pose=None), win
    best, est = PR.poses_of(m["best"], win, case["rel_pose"])
    mean, scov, cov = covariance(m, win["steps"], est, case["rel_pose"])
    return dict(moments=m, mean_offset=mean, sensor_covariance=scov, covariance=cov, estimated_pose=est), win
