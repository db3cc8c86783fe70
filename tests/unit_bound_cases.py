"""numpy restatement of what a coarse-first window batch rests on (csm_joint_kernels.hip:
k_coarse_joint_batch, k_unit_bounds): the integer sums of the box-max(L) level's nodes, and from them
the bound of every unit (slice, candidate block) of the exact pass. Shared by test_cpu_unit_bounds.py
and test_gpu_coarse_first.py; nothing here touches a GPU.

Conventions (include/csm_hip.h): candidate (t, xi, yi) of a window reads, for beam i, the cell
(row[t, i] + y_lo + yi, col[t, i] + x_lo + xi); a read outside the grid is unknown (0). The level has
one node per L x L candidates: node (t, xc, yc) reads the level at the offsets of candidate
(t, xc * L, yc * L). key = 32268 K + 499 S."""
import numpy as np

from csm_hip import api


def window_of(case, rx, ry, rt, L):
    """The window of a case as the library frames it: steps, half widths, candidate domain padded
    to a multiple of L, and the projected hits of every slice."""
    sx, sy, st = api.host_search_step(case["geom"][0], case["ranges"])
    wx, wy, wt = api.host_window(rx, sx), api.host_window(ry, sy), api.host_window(rt, st)
    col, row = api.host_project(case["geom"], case["init_pose"], st, wt, case["angles"], case["ranges"])
    nx, ny = -(-(2 * wx + 1) // L) * L, -(-(2 * wy + 1) // L) * L
    return dict(wx=wx, wy=wy, wt=wt, nx=nx, ny=ny, col=np.asarray(col), row=np.asarray(row), L=L)


def node_sums(level, w):
    """(S, K) of every node of the level: uint64 arrays [n_theta][nx / L][ny / L]."""
    L, nxc, nyc = w["L"], w["nx"] // w["L"], w["ny"] // w["L"]
    rows, cols = level.shape
    n_theta = w["col"].shape[0]
    S = np.zeros((n_theta, nxc, nyc), np.uint64)
    K = np.zeros((n_theta, nxc, nyc), np.uint64)
    xo = -w["wx"] + L * np.arange(nxc)
    yo = -w["wy"] + L * np.arange(nyc)
    for t in range(n_theta):
        c = w["col"][t][:, None, None] + xo[None, :, None]          # [beam][xc][1]
        r = w["row"][t][:, None, None] + yo[None, None, :]          # [beam][1][yc]
        ok = (c >= 0) & (c < cols) & (r >= 0) & (r < rows)
        v = np.where(ok, level[np.clip(r, 0, rows - 1), np.clip(c, 0, cols - 1)], 0).astype(np.uint64)
        S[t] = v.sum(axis=0)
        K[t] = (v != 0).sum(axis=0)
    return S, K


def keys_of(S, K):
    return 32268 * K.astype(np.uint64) + 499 * S.astype(np.uint64)


def blocks_of(n, size):
    """[lo, hi) of the candidate blocks of `size` along an axis of n candidates."""
    return [(lo, min(n, lo + size)) for lo in range(0, n, size)]


def unit_bounds(node_keys, w, cbx, cby):
    """bound[t][by][bx] = the greatest key among the nodes whose L x L candidates intersect block
    (bx, by): columns [bx * cbx, +cbx), rows [by * cby, +cby), cut at the window."""
    L = w["L"]
    xb, yb = blocks_of(w["nx"], cbx), blocks_of(w["ny"], cby)
    out = np.zeros((node_keys.shape[0], len(yb), len(xb)), np.uint64)
    for j, (y0, y1) in enumerate(yb):
        for i, (x0, x1) in enumerate(xb):
            out[:, j, i] = node_keys[:, x0 // L:(x1 - 1) // L + 1, y0 // L:(y1 - 1) // L + 1].max(axis=(1, 2))
    return out


def unit_maxima(fine_keys, w, cbx, cby):
    """The greatest fine key of every unit, same shape as unit_bounds."""
    xb, yb = blocks_of(w["nx"], cbx), blocks_of(w["ny"], cby)
    out = np.zeros((fine_keys.shape[0], len(yb), len(xb)), np.uint64)
    for j, (y0, y1) in enumerate(yb):
        for i, (x0, x1) in enumerate(xb):
            out[:, j, i] = fine_keys[:, x0:x1, y0:y1].max(axis=(1, 2))
    return out


def pair_max(per_slice):
    """Units of the exact pass are PAIRS of slices (2p, 2p + 1; a last single one): the pair's value."""
    n = per_slice.shape[0]
    out = per_slice[0::2].copy()
    out[:n // 2] = np.maximum(out[:n // 2], per_slice[1::2])
    return out


def select_rounds(case, oracle, rx, ry, rt, L, cbx, cby, score_thr=0.0, known_thr=0.0):
    """The two selection rounds of the exact pass restated (k_bound_select on the unit bounds): which
    units round 1 lists (bound near the greatest bound), the best eligible exact key B they hold, which
    units round 2 adds (bound reaches B). Also the oracle's band flag, the number of candidates that
    share the winner's key and the units of the greatest bound and of the winner."""
    w = window_of(case, rx, ry, rt, L)
    S, K = node_sums(oracle.boxmax(case["grid"], L), w)
    d, fS, fK, _ = oracle.csm_closed_form(case, rx, ry, rt, L, score_thr, known_thr, dump=True)
    n = len(case["angles"])
    eligible = np.repeat(np.repeat(K >= api.host_min_known(n, known_thr), L, axis=1), L, axis=2)
    fine = np.where(eligible, keys_of(fS, fK), 0)
    bound = pair_max(unit_bounds(keys_of(S, K), w, cbx, cby))
    best = pair_max(unit_maxima(fine, w, cbx, cby))
    slack = 4.0 * (n + 3) * 2.0 ** -24
    floor = score_thr * n * (65534.0 * 499.0 / 0.998) * (1 - 1e-9) * (1 - slack) if score_thr > 0 else 0.0
    r1 = bound >= max(float(bound.max()) * (1 - slack), floor)
    B = int(best[r1].max()) if r1.any() else 0
    r2 = ~r1 & (bound >= max(B * (1 - slack), floor))
    return dict(window=w, n_theta=fS.shape[0], units=bound.size, round1=int(r1.sum()), round2=int(r2.sum()),
                round1_key=B, best_key=int(fine.max()), ties=int((fine == fine.max()).sum()),
                band=d["touchesBand"], found=d["found"],
                top_unit=np.unravel_index(bound.argmax(), bound.shape),
                winner_unit=np.unravel_index(best.argmax(), best.shape))


def bound_breaks(case, oracle, rx, ry, rt, L):
    """Candidates whose key exceeds their node's: none clear of the negative edge band; where a beam is in
    the band a box of the level may read unknown (outside the grid) under known cells, and the exact
    kernel's check against the level flags the record CSM_FLAG_EDGE_BAND."""
    w = window_of(case, rx, ry, rt, L)
    S, K = node_sums(oracle.boxmax(case["grid"], L), w)
    _, fS, fK, _ = oracle.csm_closed_form(case, rx, ry, rt, L, dump=True)
    parents = np.repeat(np.repeat(keys_of(S, K), L, axis=1), L, axis=2)
    return int((keys_of(fS, fK) > parents).sum())
