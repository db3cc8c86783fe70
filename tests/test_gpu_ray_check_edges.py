"""GPU parity of csm_ray_check_batch at its edges (cases and references: tests/ray_check_reference.py): far
frames up to the documented 2^20-cell bound, against the windowed reference in Python integers; rays clipped
at every edge of the map; cell values on the thresholds; the bookkeeping of a batch (queries without a beam,
beam counts about the walk's group size, an uncertified list that is exactly full, the switch to host
projection in a later chunk); a seeded sweep. Every case alone, batched per parameter set and with the hit
points from the host. Everything is an integer: records (host_beams aside) and per-beam words are compared for
equality."""
import numpy as np
import pytest

import ray_check_reference as R
from csm_hip import _lib as L, api

pytestmark = pytest.mark.gpu

BASE = 8800                          # 8800 .. 8899: this file's map ids
FAR = R.far_cases()
CLIP = R.clip_cases()
THRESHOLD = R.threshold_cases()
NAMED = FAR + CLIP + THRESHOLD
NAMES = [c["name"] for c in NAMED]


class Maps:
    """The distinct grids of the cases handed in, resident on one context under this file's ids."""

    def __init__(self, ctx, first=BASE):
        self.ctx, self.first, self.ids = ctx, first, {}

    def id_of(self, grid):
        key = (grid.shape, grid.tobytes())
        if key not in self.ids:
            mid = self.first + len(self.ids)
            assert mid < BASE + 100
            self.ctx.upload_grid(mid, grid)
            self.ids[key] = mid
        return self.ids[key]

    def query(self, c):
        return dict(map_id=self.id_of(c["grid"]), geom=c["geom"], angles=c["angles"], ranges=c["ranges"],
                    rel_pose=c["rel_pose"], init_pose=c["pose"])

    def release(self):
        for mid in self.ids.values():
            if self.ctx.has_grid(mid):
                self.ctx.release_grid(mid)
        self.ids = {}


@pytest.fixture(scope="module")
def references():
    refs = {c["name"]: R.check_case_windowed(c) for c in FAR}
    refs.update({c["name"]: R.check_case(c) for c in CLIP + THRESHOLD})
    return refs


@pytest.fixture(scope="module")
def maps(gpu_ctx):
    m = Maps(gpu_ctx)
    yield m
    m.release()


def _by_parameter_set(cases):
    by = {}
    for c in cases:
        by.setdefault(tuple(sorted(c["params"].items())), []).append(c)
    return [(dict(key), cs) for key, cs in by.items()]


def _run(maps, cases, wants, prm, **extra):
    """One call; every record and every word against its reference. Returns the records."""
    got, words = maps.ctx.ray_check_batch([maps.query(c) for c in cases], per_beam=True, **dict(prm, **extra))
    assert len(got) == len(cases)
    for c, g, w, (want, want_words) in zip(cases, got, words, wants):
        assert R.strip(g) == want, c["name"]
        assert np.array_equal(w, want_words), c["name"]
        assert 0 <= g["host_beams"] <= g["usable"]
    return got


@pytest.mark.parametrize("name", NAMES)
def test_case_alone(maps, references, name):
    c = NAMED[NAMES.index(name)]
    _run(maps, [c], [references[name]], c["params"])


@pytest.mark.parametrize("cases", [FAR, CLIP, THRESHOLD], ids=["far", "clip", "thresholds"])
def test_cases_of_one_parameter_set_in_one_call(maps, references, cases):
    groups = _by_parameter_set(cases)
    assert cases is THRESHOLD or max(len(cs) for _, cs in groups) >= 2   # a threshold case is a set of its own
    for prm, cs in groups:
        _run(maps, cs, [references[c["name"]] for c in cs], prm)
        _run(maps, cs, [references[c["name"]] for c in cs], prm, scratch_limit_bytes=1)    # a chunk per query


def test_hit_points_from_the_host(references):
    ctx = api.Context(0, tuning_off=L.TUNE_MAP_HOST_PROJECTION)
    try:
        maps = Maps(ctx)
        for prm, cs in _by_parameter_set(NAMED):
            records = _run(maps, cs, [references[c["name"]] for c in cs], prm)
            assert all(r["host_beams"] == r["usable"] for r in records)
        maps.release()
    finally:
        ctx.close()


# ---- bookkeeping ----

def test_queries_without_a_beam_between_others(maps):
    cases = R.bookkeeping_cases()
    assert [c["angles"].size for c in cases] == [17, 0, 16, 0, 0, 1, 33, 15, 32, 0]
    assert len({maps.id_of(c["grid"]) for c in cases}) == 3
    wants = [R.check_case(c) for c in cases]
    for extra in ({}, dict(scratch_limit_bytes=1)):
        records = _run(maps, cases, wants, cases[0]["params"], **extra)
        for c, r in zip(cases, records):
            if c["angles"].size == 0:
                assert r["beams"] == r["usable"] == r["walked"] == r["host_beams"] == 0
                assert all(r[k] == 0 for k in R.FIELDS)
    got, words = maps.ctx.ray_check_batch([maps.query(c) for c in cases], per_beam=True, **cases[0]["params"])
    assert [w.size for w in words] == [c["angles"].size for c in cases]


def _with_cap(cap, cases, wants, **extra):
    """The cases on a context of their own whose uncertified list holds `cap` beams."""
    ctx = api.Context(0, map_uncertain_cap=cap)
    try:
        maps = Maps(ctx)
        records = _run(maps, cases, wants, cases[0]["params"], **extra)
        maps.release()
    finally:
        ctx.close()
    return records


def test_uncertified_list_exactly_full_and_one_short(maps):
    c = R.edge_fan_case(64)
    want = R.check_case(c)
    n = _run(maps, [c], [want], c["params"])[0]["host_beams"]      # read only to choose the two capacities
    assert 2 <= n < want[0]["usable"]
    assert _with_cap(n, [c], [want])[0]["host_beams"] == n                          # pos < cap for every beam
    assert _with_cap(n - 1, [c], [want])[0]["host_beams"] == want[0]["usable"]      # n_unc > cap: all on the host


def test_switch_to_host_projection_in_a_later_chunk(maps):
    cases = R.late_switch_cases()
    wants = [R.check_case(c) for c in cases]
    usable = [w[0]["usable"] for w in wants]
    listed = [r["host_beams"] for r in _run(maps, cases, wants, cases[0]["params"], scratch_limit_bytes=1)]
    cap = max(listed[:3])
    assert cap >= 1 and listed[3] > cap and all(n < u for n, u in zip(listed[:3], usable))
    records = _with_cap(cap, cases, wants, scratch_limit_bytes=1)
    host = [r["host_beams"] for r in records]
    first = next(i for i, (h, u) in enumerate(zip(host, usable)) if h == u > cap)
    assert first == 3
    assert host[:first] == listed[:first] and all(h <= cap for h in host[:first])   # patched
    assert host[first:] == usable[first:]                                           # this chunk and the rest


# ---- the sweep ----

@pytest.mark.parametrize("seed", R.SWEEP_SEEDS)
def test_sweep(gpu_ctx, seed):
    cases = R.sweep_cases(seed)
    maps = Maps(gpu_ctx, BASE + 80)
    try:
        assert len({maps.id_of(c["grid"]) for c in cases}) >= 4        # two tiny grids may be equal
        _run(maps, cases, [R.check_case(c) for c in cases], cases[0]["params"])
    finally:
        maps.release()
