"""The winner of a correlative window under a motion prior, from the CPU oracle's per-candidate sums: the
complete specification of csm_score_window_prior / csm_correlative_match_prior (include/csm_hip.h). numpy
int64 for the volume (the entry's range check keeps every sum below 2^62), Python floats for the
quantisation and the Jacobian transform.

Candidates, key and eligibility as in tests/peaks_reference.py. d = (x, y, t) = offsets from the window
centre; pen(d) = max(0, (sum Q_ab d_a d_b) >> 8); pk = key - pen. Winner: the greatest pk, then the greatest
key, then the greatest f64 beam-order score, then the first in the reference's sweep order."""
import math

import numpy as np

import peaks_reference as PR
from csm_hip import _lib as Lb
from oracle import oracle as O

PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))       # xx xy xt yy yt tt
C_KEY = 0.998 / (65534.0 * 499.0)
ZERO = dict(found=0, best_x=0, best_y=0, best_theta=0, key=0, sum_values=0, known=0, tie_count=0, flags=0, score=0.0)


def quantise(information, steps, n_points, d_max):
    """Q[6] as Python ints, or None where csm_host_motion_prior refuses."""
    lam = [[float(v) for v in r] for r in np.asarray(information, np.float64).reshape(3, 3)]
    if not all(math.isfinite(v) for r in lam for v in r):
        return None
    if any(lam[a][b] != lam[b][a] for a in range(3) for b in range(3)):
        return None
    Q = []
    for a, b in PAIRS:
        m = 0.5 if a == b else 1.0
        q = ((((float(n_points) / C_KEY) * m) * lam[a][b]) * steps[a]) * steps[b]
        v = q * 256.0
        if not abs(v) < 2.0 ** 63:
            return None
        Q.append(int(math.floor(v + 0.5)))
    if 6 * max(abs(q) for q in Q) * d_max * d_max >= 1 << 62:
        return None
    return Q


def sensor_information(robot_information, initial_pose, rel_pose):
    """J^T Lambda J as 9 floats: the header's expression, product by product, upper triangle mirrored."""
    R = [float(v) for v in np.asarray(robot_information, np.float64).reshape(-1)]
    sn, cs = math.sin(initial_pose[2]), math.cos(initial_pose[2])
    J = [[1.0, 0.0, sn * rel_pose[0] + cs * rel_pose[1]], [0.0, 1.0, -cs * rel_pose[0] + sn * rel_pose[1]],
         [0.0, 0.0, 1.0]]
    T = [[(J[0][i] * R[j] + J[1][i] * R[3 + j]) + J[2][i] * R[6 + j] for j in range(3)] for i in range(3)]
    out = [0.0] * 9
    for i in range(3):
        for j in range(i, 3):
            out[3 * i + j] = out[3 * j + i] = (T[i][0] * J[0][j] + T[i][1] * J[1][j]) + T[i][2] * J[2][j]
    return out


def quad_form(Q, x, y, t):
    """sum Q_ab d_a d_b before the shift and the clamp (int64 arrays or Python ints)."""
    return Q[0] * x * x + Q[1] * x * y + Q[2] * x * t + Q[3] * y * y + Q[4] * y * t + Q[5] * t * t


def penalty(Q, x, y, t):
    s = quad_form(Q, x, y, t) >> 8
    return np.maximum(s, 0) if isinstance(s, np.ndarray) else max(s, 0)


def select(S, K, CK, L, grid, col, row, wx, wy, wt, Q, score_thr=0.0, known_thr=0.0):
    """(result dict with csm_prior_result's fields, number of eligible candidates the clamp acts on)."""
    n = col.shape[1]
    nt, nx, ny = S.shape
    key = 32268 * K.astype(np.int64) + 499 * S.astype(np.int64)
    alive = np.ones(S.shape, bool)
    if L > 1:
        alive = np.repeat(np.repeat(CK.astype(np.float64) / float(n) > known_thr, L, 1), L, 2)
    t, x, y = (a.astype(np.int64) for a in np.indices(S.shape))
    rank = ((t * (nx // L) + x // L) * (ny // L) + y // L) * L * L + (x % L) * L + (y % L)
    raw = quad_form(Q, x - wx, y - wy, t - wt)
    pen = np.maximum(raw >> 8, 0)
    pk = key - pen
    unweighted = PR.select(S, K, CK, L, grid, col, row, wx, wy, wt, 1, (0, 0, 0), score_thr, known_thr)
    out = dict(best=ZERO, unweighted=unweighted[0] if unweighted else ZERO, penalty=0, penalised_key=0, Q=list(Q))
    clamped = int((alive & (raw < 0)).sum())
    if not alive.any():
        return out, clamped
    tied = alive & (pk == pk[alive].max())
    tied &= key == key[tied].max()
    ties = np.argwhere(tied)
    score = PR.beam_order_scores(np.asarray(grid), O.lut(), col, row, ties, wx, wy)
    top = ties[score == score.max()]
    bt, bx, by = top[np.argmin(rank[top[:, 0], top[:, 1], top[:, 2]])]
    if not score.max() > score_thr:         # the raw score, not the penalised one
        return out, clamped
    flags = 0
    if len(ties) > 1:
        flags = Lb.FLAG_KEY_TIE | (Lb.FLAG_F64_TIE if len(top) > 1 else 0)
    out["best"] = dict(found=1, best_x=int(bx - wx), best_y=int(by - wy), best_theta=int(bt - wt),
                       key=int(key[bt, bx, by]), sum_values=int(S[bt, bx, by]), known=int(K[bt, bx, by]),
                       tie_count=len(ties), flags=flags, score=float(score.max()))
    out["penalty"] = int(pen[bt, bx, by])
    out["penalised_key"] = int(pk[bt, bx, by])
    return out, clamped


def volume(case, rx, ry, rt, L, score_thr=0.0, known_thr=0.0):
    """The oracle's dumps and the window of a case: what every prior on it shares."""
    cf, S, K, CK = O.csm_closed_form(case, rx, ry, rt, L, score_thr, known_thr, dump=True)
    (wx, wy, wt), steps, sensor, col, row = PR.window_of(case, rx, ry, rt)
    win = dict(win=(wx, wy, wt), steps=steps, sensor=sensor, col=col, row=row, shape=S.shape)
    return dict(S=S, K=K, CK=CK, cf=cf, win=win, L=L, score_thr=score_thr, known_thr=known_thr)


def d_max_of(win):
    return max(win["shape"]) - 1


def prior(vol, case, information, steps=None):
    """(result dict, clamped candidates) of a volume() under `information`; steps default to the search's."""
    win = vol["win"]
    wx, wy, wt = win["win"]
    Q = quantise(information, steps or win["steps"], len(case["angles"]), d_max_of(win))
    assert Q is not None
    return select(vol["S"], vol["K"], vol["CK"], vol["L"], case["grid"], win["col"], win["row"], wx, wy, wt, Q,
                  vol["score_thr"], vol["known_thr"])
