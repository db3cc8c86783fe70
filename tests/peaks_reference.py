"""The K best distinct poses of a correlative window, from the CPU oracle's per-candidate sums: the
complete specification of csm_score_window_peaks / csm_correlative_peaks (include/csm_hip.h).

Candidates (t, x, y) over the extended domain; key = 32268 K + 499 S; eligible iff the coarse node's
known rate passes (L = 1: all). Peak j = among the eligible candidates no earlier peak excludes: the
greatest key, then the greatest f64 beam-order score, then the first in the reference's sweep order."""
import numpy as np

from csm_hip import _lib as Lb
from oracle import oracle as O


def window_of(case, rx, ry, rt):
    """(wx, wy, wt), steps, sensor pose, hit indices [n_theta][n] of the case's search window."""
    sx, sy, st = O.search_step(case["geom"][0], case["ranges"])
    wx, wy, wt = (int(np.ceil(0.5 * r / s)) for r, s in ((rx, sx), (ry, sy), (rt, st)))
    sensor = O.compound(case["init_pose"], case["rel_pose"])
    hits = [O.project(case["geom"], (sensor[0], sensor[1], sensor[2] + st * t), case["angles"], case["ranges"])
            for t in range(-wt, wt + 1)]
    return (wx, wy, wt), (sx, sy, st), sensor, np.array([h[0] for h in hits]), np.array([h[1] for h in hits])


def beam_order_scores(grid, lut, col, row, cands, wx, wy):
    """f64 score of every candidate (t, x, y) of cands: lut values of its hit cells added in beam order, / N."""
    t, x, y = cands[:, 0], cands[:, 1], cands[:, 2]
    r = row[t] + (y - wy)[:, None]
    c = col[t] + (x - wx)[:, None]
    inside = (r >= 0) & (r < grid.shape[0]) & (c >= 0) & (c < grid.shape[1])
    v = np.where(inside, grid[np.clip(r, 0, grid.shape[0] - 1), np.clip(c, 0, grid.shape[1] - 1)], 0)
    return np.add.accumulate(lut[v], axis=1)[:, -1] / float(col.shape[1])


def select(S, K, CK, L, grid, col, row, wx, wy, wt, k_max, excl, score_thr=0.0, known_thr=0.0):
    """The peaks' records (dicts with csm_result's fields), best first."""
    n = col.shape[1]
    nt, nx, ny = S.shape
    key = 32268 * K.astype(np.int64) + 499 * S.astype(np.int64)
    alive = np.ones(S.shape, bool)
    if L > 1:
        alive = np.repeat(np.repeat(CK.astype(np.float64) / float(n) > known_thr, L, 1), L, 2)
    t, x, y = np.indices(S.shape)
    rank = ((t * (nx // L) + x // L) * (ny // L) + y // L) * L * L + (x % L) * L + (y % L)
    lut, out = O.lut(), []
    grid = np.asarray(grid)
    while len(out) < k_max and alive.any():
        ties = np.argwhere(alive & (key == key[alive].max()))
        score = beam_order_scores(grid, lut, col, row, ties, wx, wy)
        top = ties[score == score.max()]
        bt, bx, by = top[np.argmin(rank[top[:, 0], top[:, 1], top[:, 2]])]
        if not score.max() > score_thr:
            break
        flags = 0
        if len(ties) > 1:
            flags = Lb.FLAG_KEY_TIE | (Lb.FLAG_F64_TIE if len(top) > 1 else 0)
        out.append(dict(found=1, best_x=int(bx - wx), best_y=int(by - wy), best_theta=int(bt - wt),
                        key=int(key[bt, bx, by]), sum_values=int(S[bt, bx, by]), known=int(K[bt, bx, by]),
                        tie_count=len(ties), flags=flags, score=float(score.max())))
        alive &= ~((abs(t - bt) <= excl[2]) & (abs(x - bx) <= excl[0]) & (abs(y - by) <= excl[1]))
    return out


def peaks(case, rx, ry, rt, L, k_max, excl, score_thr=0.0, known_thr=0.0):
    """(records, closed-form result dict, window dict) of the case."""
    cf, S, K, CK = O.csm_closed_form(case, rx, ry, rt, L, score_thr, known_thr, dump=True)
    (wx, wy, wt), steps, sensor, col, row = window_of(case, rx, ry, rt)
    rec = select(S, K, CK, L, case["grid"], col, row, wx, wy, wt, k_max, excl, score_thr, known_thr)
    return rec, cf, dict(win=(wx, wy, wt), steps=steps, sensor=sensor, col=col, row=row, shape=S.shape)


def poses_of(rec, win, rel_pose):
    """(best sensor pose, estimated pose) rebuilt from a record's indices."""
    sx, sy, st = win["steps"]
    s = win["sensor"]
    best = [s[0] + rec["best_x"] * sx, s[1] + rec["best_y"] * sy, s[2] + rec["best_theta"] * st]
    return best, list(O.move_backward(best, rel_pose))
