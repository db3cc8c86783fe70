"""The appearance rule (include/csm_hip.h, "loop search by appearance") as a literal numpy / integer Python
statement, written from the header's text: the edge tables by its two expressions, the bin as "the greatest k
with edge[k] <= value", the distance as the minimum over every shift of a plain L1 sum, the search as a sort of
the eligible pairs. The edge expressions are evaluated operation by operation in f64, as the header writes
them; everything after the edges is integer arithmetic."""
import math

import numpy as np

from loop_search_reference import prefix_length

CANDIDATE = np.dtype([("query_scan_index", np.int32), ("ref_scan_index", np.int32), ("ref_map_index", np.int32),
                      ("shift", np.int32), ("distance", np.uint32), ("ring_distance", np.uint32)])


def edges(n_rings, n_sectors, range_min, range_max):
    ring = [range_min + ((range_max - range_min) * k) / n_rings for k in range(n_rings + 1)]
    ring[n_rings] = range_max
    sector = [-math.pi + (2.0 * math.pi * k) / n_sectors for k in range(n_sectors + 1)]
    sector[n_sectors] = math.pi
    return np.array(ring, np.float64), np.array(sector, np.float64)


def descriptor(angles, ranges, n_rings, n_sectors, range_min, range_max):
    """(cells [n_rings, n_sectors] uint8, beams used) of one scan."""
    ring_edge, sector_edge = edges(n_rings, n_sectors, float(range_min), float(range_max))
    a, r = np.asarray(angles, np.float64), np.asarray(ranges, np.float64)
    with np.errstate(invalid="ignore"):
        used = (np.isfinite(a) & np.isfinite(r) & (ring_edge[0] <= r) & (r < ring_edge[n_rings]) &
                (sector_edge[0] <= a) & (a < sector_edge[n_sectors]))
    count = np.zeros((n_rings, n_sectors), np.int64)
    for av, rv in zip(a[used], r[used]):
        ring = max(k for k in range(n_rings) if ring_edge[k] <= rv)
        sec = max(k for k in range(n_sectors) if sector_edge[k] <= av)
        count[ring, sec] += 1
    return np.minimum(count, 255).astype(np.uint8), int(used.sum())


def descriptors(angles, ranges, offsets, n_rings, n_sectors, range_min, range_max):
    out = np.zeros((len(offsets) - 1, n_rings, n_sectors), np.uint8)
    used = np.zeros(len(offsets) - 1, np.int32)
    for i in range(len(offsets) - 1):
        out[i], used[i] = descriptor(angles[offsets[i]:offsets[i + 1]], ranges[offsets[i]:offsets[i + 1]], n_rings,
                                     n_sectors, range_min, range_max)
    return out, used


def l1(q, r, s):
    """L1(s) = sum |Q[ring][(sec + s) mod S] - R[ring][sec]|"""
    n_sectors = q.shape[1]
    sec = (np.arange(n_sectors) + s) % n_sectors
    return int(np.abs(q[:, sec].astype(np.int64) - r.astype(np.int64)).sum())


def distance(q, r):
    """(distance, shift, ring_distance) of two descriptors [n_rings, n_sectors]."""
    all_l1 = [l1(q, r, s) for s in range(q.shape[1])]
    d = min(all_l1)
    ring = int(np.abs(q.astype(np.int64).sum(1) - r.astype(np.int64).sum(1)).sum())
    return d, all_l1.index(d), ring


def shift_angle(shift, n_sectors):
    t = math.fmod((-float(shift) * (2.0 * math.pi)) / float(n_sectors), 2.0 * math.pi)
    if t > math.pi:
        t -= 2.0 * math.pi
    elif t < -math.pi:
        t += 2.0 * math.pi
    return t


def search(desc, map_index, travel, n_ref, query_index, query_travel, travel_dist_threshold, max_distance,
           min_cell_sum, n_per_query, one_per_map):
    """(records [n_q, K], counts [n_q], info) as the rule states them."""
    m = np.asarray(map_index)
    k = int(n_per_query)
    total = desc.reshape(len(desc), -1).astype(np.int64).sum(1)
    out = np.zeros((len(query_index), k), CANDIDATE)
    counts = np.zeros(len(query_index), np.int32)
    evaluated = n_eligible = 0
    for i, q in enumerate(query_index):
        p = prefix_length(travel, n_ref, query_travel[i], travel_dist_threshold)
        evaluated += p
        found = []
        for r in range(p):
            if m[r] == m[q] or total[q] < min_cell_sum or total[r] < min_cell_sum:
                continue
            d, s, ring = distance(desc[q], desc[r])
            if d <= max_distance:
                found.append((d, r, s, ring))
        n_eligible += len(found)
        found.sort()
        out[i]["query_scan_index"] = q
        out[i]["ref_scan_index"] = -1
        out[i]["ref_map_index"] = -1
        taken, used = set(), 0
        for d, r, s, ring in found:
            if used == k:
                break
            if one_per_map:
                if m[r] in taken:
                    continue
                taken.add(m[r])
            out[i, used] = (q, r, m[r], s, d, ring)
            used += 1
        counts[i] = used
    return out, counts, dict(pairs_evaluated=int(evaluated), pairs_eligible=int(n_eligible))
