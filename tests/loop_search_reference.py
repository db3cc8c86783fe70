"""The loop search rule (include/csm_hip.h, csm_loop_search) as a literal Python statement, and a literal
walk of LoopSearcherNearest::Search (src/mapping/loop_searcher_nearest.cpp:59-170).

hypot and pow come from libm through ctypes: CPython's math.hypot has its own algorithm and need not agree
with glibc in the last bit. The pair loop of the rule is vectorised with numpy; every operation stays a
separate f64 operation (numpy fuses nothing)."""
import ctypes
import ctypes.util

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.hypot.restype = ctypes.c_double
_libm.hypot.argtypes = [ctypes.c_double, ctypes.c_double]
_libm.pow.restype = ctypes.c_double
_libm.pow.argtypes = [ctypes.c_double, ctypes.c_double]

MAX_K = 16

CANDIDATE = np.dtype([("query_scan_index", np.int32), ("ref_scan_index", np.int32), ("ref_map_index", np.int32),
                      ("reserved", np.int32), ("dist_sq", np.float64)])


def hypot(a, b):
    return _libm.hypot(float(a), float(b))


def threshold_sq(node_dist_threshold):
    return _libm.pow(float(node_dist_threshold), 2.0)


def travel_distances(poses):
    """out[0] = 0, out[i] = out[i-1] + hypot(x[i-1] - x[i], y[i-1] - y[i]), in order."""
    p = np.asarray(poses, np.float64).reshape(-1, 3)
    out = np.zeros(len(p))
    for i in range(1, len(p)):
        out[i] = out[i - 1] + hypot(p[i - 1, 0] - p[i, 0], p[i - 1, 1] - p[i, 1])
    return out


def prefix_length(travel, n_ref, query_travel, travel_dist_threshold):
    """Reference nodes before the first r with query_travel - travel[r] < threshold."""
    stop = (np.float64(query_travel) - np.asarray(travel[:n_ref], np.float64)) < np.float64(travel_dist_threshold)
    return int(np.argmax(stop)) if stop.any() else int(n_ref)


def eligible(poses, map_index, travel, n_ref, q, query_travel, travel_dist_threshold, node_dist_threshold):
    """(prefix length, the eligible reference nodes of query q ordered by (d2, r), their d2)."""
    p = np.asarray(poses, np.float64).reshape(-1, 3)
    m = np.asarray(map_index)
    n = prefix_length(travel, n_ref, query_travel, travel_dist_threshold)
    dx = p[:n, 0] - p[q, 0]
    dy = p[:n, 1] - p[q, 1]
    xx = dx * dx
    yy = dy * dy
    d2 = xx + yy
    ok = (m[:n] != m[q]) & (d2 < threshold_sq(node_dist_threshold))
    r = np.nonzero(ok)[0]
    d = d2[r]
    order = np.lexsort((r, d.view(np.uint64)))
    return n, r[order], d[order]


def rule(poses, map_index, travel, n_ref, query_index, query_travel, travel_dist_threshold, node_dist_threshold,
         n_per_query, one_per_map):
    """(records [n_q, K], counts [n_q], info) as the rule states them."""
    m = np.asarray(map_index)
    k = int(n_per_query)
    out = np.zeros((len(query_index), k), CANDIDATE)
    counts = np.zeros(len(query_index), np.int32)
    evaluated = n_eligible = 0
    for i, q in enumerate(query_index):
        n, r, d = eligible(poses, map_index, travel, n_ref, q, query_travel[i], travel_dist_threshold,
                           node_dist_threshold)
        evaluated += n
        n_eligible += len(r)
        out[i]["query_scan_index"] = q
        out[i]["ref_scan_index"] = -1
        out[i]["ref_map_index"] = -1
        taken, used = set(), 0
        for rr, dd in zip(r, d):
            if used == k:
                break
            if one_per_map:
                if m[rr] in taken:
                    continue
                taken.add(m[rr])
            out[i, used] = (q, rr, m[rr], 0, dd)
            used += 1
        counts[i] = used
    return out, counts, dict(pairs_evaluated=int(evaluated), pairs_eligible=int(n_eligible))


def nearest(records, counts, n_total):
    """The first n_total used records by (dist_sq, ref_scan_index, query_scan_index)."""
    used = [records[i, j] for i in range(len(counts)) for j in range(counts[i])]
    used.sort(key=lambda c: (float(c["dist_sq"]), int(c["ref_scan_index"]), int(c["query_scan_index"])))
    return np.array(used[:n_total], CANDIDATE)


def reference_walk(poses, runs, accum_travel_dist, last_finished_map, travel_dist_threshold, node_dist_threshold):
    """LoopSearcherNearest::Search's nested loops with the early exit, then a full sort by (d2, ref, query) in
    place of nth_element. runs: (scan_node_min, scan_node_max) per local map. Returns the sorted list of
    (d2, ref scan node, query scan node, ref local map)."""
    p = np.asarray(poses, np.float64).reshape(-1, 3)
    t2 = threshold_sq(node_dist_threshold)
    q_lo, q_hi = runs[last_finished_map]
    found = []
    node_travel, first, prev = 0.0, True, None
    done = False
    for ref_map in range(last_finished_map):
        lo, hi = runs[ref_map]
        for ref in range(lo, hi + 1):
            rx, ry = float(p[ref, 0]), float(p[ref, 1])
            node_travel += 0.0 if first else hypot(prev[0] - rx, prev[1] - ry)
            prev, first = (rx, ry), False
            if accum_travel_dist - node_travel < travel_dist_threshold:
                done = True
                break
            for query in range(q_lo, q_hi + 1):
                qx, qy = float(p[query, 0]), float(p[query, 1])
                d2 = (rx - qx) * (rx - qx) + (ry - qy) * (ry - qy)
                if d2 < t2:
                    found.append((d2, ref, query, ref_map))
        if done:
            break
    found.sort()
    return found
