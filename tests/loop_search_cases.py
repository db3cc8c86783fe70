"""Seeded pose graphs for the loop search tests. Each family returns a dict:
poses [n, 3], runs ((scan_node_min, scan_node_max) per local map), map_index [n], travel [n] (the literal
accumulation), travel_dist_threshold, node_dist_threshold.

  laps         three laps of a 10 m x 6 m rectangle on a 0.25 m lattice: 128 nodes per lap, maps of 10 nodes,
               thresholds 10 m and 2 m. Laps revisit identical coordinates, so equal d2 between different
               reference nodes is the rule; lattice coordinates make d2 == T2 and gap == travel threshold
               occur exactly. laps_properties() asserts what the family must contain.
  random_walk  continuous poses, 1 000 nodes, maps of 1 to 30 nodes including single-node maps.
  far_frame    the laps shifted by (1e6, -2e6): every difference, and so every record, is the laps'.
"""
import functools

import numpy as np

import loop_search_reference as R

FAMILIES = ("laps", "random_walk", "far_frame")


def _finish(poses, sizes, travel_thr, node_thr):
    poses = np.ascontiguousarray(poses, np.float64)
    runs, at = [], 0
    for s in sizes:
        runs.append((at, at + s - 1))
        at += s
    assert at == len(poses)
    map_index = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    return dict(poses=poses, runs=runs, map_index=map_index, travel=R.travel_distances(poses),
                travel_dist_threshold=travel_thr, node_dist_threshold=node_thr)


def _lap_poses(shift=(0.0, 0.0)):
    step, pts = 0.25, []
    x = y = 0.0
    for dx, dy, n in ((1, 0, 40), (0, 1, 24), (-1, 0, 40), (0, -1, 24)):
        for _ in range(n):
            pts.append((x, y, np.arctan2(dy, dx)))
            x += dx * step
            y += dy * step
    assert len(pts) == 128 and (x, y) == (0.0, 0.0)
    lap = np.array(pts)
    poses = np.concatenate([lap, lap, lap])
    poses[:, 0] += shift[0]
    poses[:, 1] += shift[1]
    return poses


@functools.lru_cache(maxsize=None)
def family(name):
    if name in ("laps", "far_frame"):
        poses = _lap_poses((1e6, -2e6) if name == "far_frame" else (0.0, 0.0))
        sizes = [10] * 38 + [4]
        return _finish(poses, sizes, 10.0, 2.0)
    if name == "random_walk":
        rng = np.random.default_rng(20240607)
        n = 1000
        poses = np.zeros((n, 3))
        heading = 0.0
        for i in range(1, n):
            heading += rng.normal(0.0, 0.35)
            nxt = poses[i - 1, :2] + rng.uniform(0.15, 0.45) * np.array([np.cos(heading), np.sin(heading)])
            if np.abs(nxt).max() > 9.0:          # stay in an 18 m box: the walk crosses itself often
                heading += np.pi
                nxt = poses[i - 1, :2] + 0.3 * np.array([np.cos(heading), np.sin(heading)])
            poses[i] = (nxt[0], nxt[1], heading)
        sizes = []
        while sum(sizes) < n:
            s = 1 if len(sizes) % 7 == 3 else int(rng.integers(1, 31))
            sizes.append(min(s, n - sum(sizes)))
        assert min(sizes) == 1 and max(sizes) <= 30
        return _finish(poses, sizes, 10.0, 2.0)
    raise KeyError(name)


def all_queries(c):
    """Every node a query, its gate measured from its own travel distance."""
    q = np.arange(len(c["poses"]), dtype=np.int32)
    return q, c["travel"][q].copy()


def eligible_counts(c, n_ref=None):
    n_ref = len(c["poses"]) if n_ref is None else n_ref
    q, qt = all_queries(c)
    return np.array([len(R.eligible(c["poses"], c["map_index"], c["travel"], n_ref, int(i), t,
                                    c["travel_dist_threshold"], c["node_dist_threshold"])[1]) for i, t in zip(q, qt)])


@functools.lru_cache(maxsize=None)
def laps_properties(k=16):
    """What the laps family must contain (all nodes as queries, every node a possible reference), so that
    a generator change cannot quietly lose it. Returns the queries that show each property."""
    c = family("laps")
    t2 = R.threshold_sq(c["node_dist_threshold"])
    q, qt = all_queries(c)
    shows = dict(more=None, fewer=None, none=None, tie_at_cut=None, on_threshold=None, on_gap=None)
    for i, t in zip(q, qt):
        i = int(i)
        n, r, d = R.eligible(c["poses"], c["map_index"], c["travel"], len(q), i, t, c["travel_dist_threshold"],
                             c["node_dist_threshold"])
        if len(r) > k and shows["more"] is None:
            shows["more"] = i
        if 1 <= len(r) <= k - 1 and shows["fewer"] is None:
            shows["fewer"] = i
        if len(r) == 0 and shows["none"] is None:
            shows["none"] = i
        if len(r) > k and d[k - 1] == d[k] and shows["tie_at_cut"] is None:
            shows["tie_at_cut"] = i
        dx = c["poses"][:n, 0] - c["poses"][i, 0]
        dy = c["poses"][:n, 1] - c["poses"][i, 1]
        on = (dx * dx + dy * dy == t2) & (c["map_index"][:n] != c["map_index"][i])
        if on.any() and shows["on_threshold"] is None:
            assert not np.isin(np.nonzero(on)[0], r).any()            # d2 == T2 is excluded
            shows["on_threshold"] = i
        if n > 0 and t - c["travel"][n - 1] == c["travel_dist_threshold"] and shows["on_gap"] is None:
            shows["on_gap"] = i                                        # gap == threshold is inside the prefix
    if k < 2:
        del shows["fewer"]              # no count lies between 1 and K - 1
    missing = [name for name, v in shows.items() if v is None]
    assert not missing, "the laps family lost: %s" % missing
    return shows


def word_edge_graph(n_maps):
    """n_maps local maps of two nodes each on a line. The query is node 0 (map 0); the maps nearest to it
    are, in this order, those at the edges of the 32-bit and 64-bit words of a bitset over the maps, then the
    rest. Every node may be a reference and no travel gate closes (threshold far below zero)."""
    edges = [m for m in (31, 32, 63, 64, n_maps - 1, 1, 33, 65) if 0 < m < n_maps]
    order = [0] + list(dict.fromkeys(edges))
    order += [m for m in range(n_maps) if m not in order]
    rank = {m: i for i, m in enumerate(order)}
    poses = np.zeros((2 * n_maps, 3))
    for m in range(n_maps):
        poses[2 * m, 0] = 0.01 * 2 * rank[m]
        poses[2 * m + 1, 0] = 0.01 * (2 * rank[m] + 1)
    c = _finish(poses, [2] * n_maps, -1e9, 2.0)
    c["travel"] = np.zeros(2 * n_maps)          # the gate reads this, not the geometry
    c["edge_maps"] = order[1:1 + len(set(edges))]
    return c


def dense_cloud_graph(n_ref):
    """n_ref reference nodes scattered over a 1 m box in maps of 7, then one query node in the box's middle
    behind a far stretch: every reference node is eligible (the device keeps up to 1 024 eligible pairs of
    a query in LDS and walks the prefix again per record above that)."""
    rng = np.random.default_rng(n_ref)
    poses = np.zeros((n_ref + 1, 3))
    poses[:n_ref, :2] = rng.uniform(0.0, 1.0, (n_ref, 2))
    poses[n_ref, :2] = (0.5, 0.5)
    sizes = [7] * (n_ref // 7) + ([n_ref % 7] if n_ref % 7 else []) + [1]
    c = _finish(poses, sizes, 10.0, 2.0)
    c["travel"] = np.concatenate([np.linspace(0.0, 50.0, n_ref), [100.0]])
    return c


def one_pose_graph(n_ref=300):
    """n_ref reference nodes at one identical pose in maps of 7, then a far stretch, then one query node
    1 m from them: every d2 ties and the order is by index alone."""
    poses = np.zeros((n_ref + 1, 3))
    poses[:n_ref, :2] = (3.0, -2.0)
    poses[n_ref, :2] = (3.0, -1.0)
    sizes = [7] * (n_ref // 7) + ([n_ref % 7] if n_ref % 7 else []) + [1]
    c = _finish(poses, sizes, 10.0, 2.0)
    c["travel"] = np.concatenate([np.zeros(n_ref), [100.0]])
    return c
