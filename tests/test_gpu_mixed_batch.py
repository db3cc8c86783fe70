"""Loop-detection batches whose queries differ the way one Detect() call's do: several groups per
call (csm_batch.hip's loop_batch, one run_batch_group per padded leaf-window extent), queries of
other beam counts, maximum ranges, maps and thresholds side by side in one group. Several decisions
of BatchGroup::plan are taken once per group (fine.weighted from the first query, joint from the
largest binning LDS, the bound pass from n_theta_max, two_rounds from any query's min_known) and
every query has its own places in the shared workspaces; the records go back to the input order
through the record scatter and the host patches of flagged queries. Every query is compared with
the literal oracle (tolerance 0); a query's record must not depend on the other queries of its
batch, on the context's launch fall-backs or on the calls before it. The pool is
tests/mixed_batch_cases.py, its premises are checked by tests/test_cpu_mixed_batch_cases.py."""
import math
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from csm_hip import _lib as L, api

import mixed_batch_cases as mb

pytestmark = pytest.mark.gpu

RX = RY = 1.0
RT = math.radians(10)
BNB_RT = 0.2
BNB_THR = (0.3, 0.5)
CSM_THRS = [(0.0, 0.0), (0.2, 0.3), (0.05, 0.6)]
TIMING = ("input_setup_us", "optimization_us")
BEST_SCORED = ("key", "sum_values", "known", "tie_count")

_LIT = {}
_EXEC = ThreadPoolExecutor(16)


def _lits(oracle, pool, kind, queries, args):
    """The oracle's results for these queries, computed once per module (16 threads)."""
    keys = [(kind, q["name"], args) for q in queries]
    fn = oracle.csm if kind == "csm" else oracle.bnb
    futs = {k: _EXEC.submit(fn, mb.oracle_case(pool, q), *args)
            for k, q in zip(keys, queries) if k not in _LIT}
    for k, f in futs.items():
        _LIT[k] = f.result()
    return [_LIT[k] for k in keys]


class Tracked:
    """A context with the pool's maps resident, and the box-max window of every level of every map
    in creation order (level_for_window appends missing levels per map, in query order)."""

    def __init__(self, pool, tuning_off=0):
        self.pool = pool
        self.ctx = api.Context(0, tuning_off=tuning_off)
        self.wins = {}
        for mid, m in pool["maps"].items():
            if m["blocks"] is None:
                self.ctx.upload_grid(mid, m["grid"])
            else:
                blocks, br, bc, k = m["blocks"]
                self.ctx.upload_grid_blocks(mid, blocks, br, bc, k)
            self.wins[mid] = [1]

    def _note(self, queries, strides):
        new = []
        for q in queries:
            w = self.wins[q["map_id"]]
            for s in strides:
                if s not in w:
                    w.append(s)
                    new.append((q["map_id"], len(w) - 1, s))
        return new

    def csm(self, queries, L_, thr, rx=RX, ry=RY, rt=RT, as_records=False):
        new = self._note(queries, [1, L_] if L_ > 1 else [1])
        out = self.ctx.correlative_match_batch(queries, rx, ry, rt, L_, thr[0], thr[1], as_records=as_records)
        return out, new

    def bnb(self, queries, H, thr=BNB_THR, rx=RX, ry=RY, rt=BNB_RT, as_records=False):
        new = self._note(queries, [1 << h for h in range(H + 1)])
        out = self.ctx.bnb_match_batch(queries, rx, ry, rt, H, thr[0], thr[1], as_records=as_records)
        return out, new

    def check_levels(self, oracle, new):
        for mid, level, win in new:
            got = self.ctx.download_level(mid, level)
            assert np.array_equal(got, oracle.boxmax(self.pool["maps"][mid]["grid"], win)), (mid, level, win)

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def pool():
    return mb.make_pool(0)


@pytest.fixture(scope="module")
def csm_ctx(pool):
    t = Tracked(pool)
    yield t
    t.close()


@pytest.fixture(scope="module")
def bnb_ctx(pool):
    t = Tracked(pool)
    yield t
    t.close()


def _same_as_literal(out, lit, where):
    raw = out["raw"]
    assert out["pose_found"] == lit["found"], (where, raw, lit)
    assert (raw["best_x"], raw["best_y"], raw["best_theta"]) == (lit["bestX"], lit["bestY"], lit["bestT"]), \
        (where, raw, lit)
    assert raw["score"] == lit["scoreMax"], (where, raw, lit)
    assert out["estimated_pose"] == lit["estimatedPose"], (where, out, lit)
    assert (out["win_x"], out["win_y"], out["win_theta"]) == (lit["winX"], lit["winY"], lit["winT"]), where
    assert (out["step_x"], out["step_y"], out["step_theta"]) == (lit["stepX"], lit["stepY"], lit["stepT"]), where


def _record(out):
    """A summary without its timing: what must not depend on the rest of the batch. A query that
    finds nothing reports the threshold as its score and the first candidate as its best; what its
    record says of the best candidate scored (key, sums, known count, ties) depends on which blocks
    were scored at all (the bound pass never scores blocks below the threshold's key, key_floor),
    so those four fields are compared for found queries only."""
    r = {k: v for k, v in out.items() if k not in TIMING}
    if not out["pose_found"]:
        r["raw"] = {k: v for k, v in r["raw"].items() if k not in BEST_SCORED}
    return r


def _diff(a, b):
    """The fields (raw ones by name) in which two _record()s differ."""
    d = {k: (a[k], b[k]) for k in a if k != "raw" and a[k] != b[k]}
    d.update({k: (a["raw"][k], b["raw"].get(k)) for k in a["raw"] if a["raw"][k] != b["raw"].get(k)})
    return d


def _groups(queries, unit):
    key = lambda q: mb.group_key(q, api.host_search_step, api.host_window, RX, RY, unit)   # noqa: E731
    return [key(q) for q in queries]


@pytest.mark.parametrize("Lr", [1, 3, 4, 5])
@pytest.mark.parametrize("thr", CSM_THRS)
def test_correlative_mixed_batch_equals_literal_sweep(csm_ctx, oracle, pool, Lr, thr):
    qs = pool["queries"]
    assert len(set(_groups(qs, Lr))) >= 3
    outs, new = csm_ctx.csm(qs, Lr, thr)
    lits = _lits(oracle, pool, "csm", qs, (RX, RY, RT, Lr, thr[0], thr[1]))
    for q, o, lit in zip(qs, outs, lits):
        _same_as_literal(o, lit, (q["name"], Lr, thr))
    csm_ctx.check_levels(oracle, new)


def test_correlative_full_turn_mixes_long_and_short_ranges(csm_ctx, oracle, pool):
    """range_theta = 2 pi: the 20 m scan's group needs > 2048 slices (no bound pass there, and the
    short scans of that group run in its longer launch), the other groups about 700."""
    qs = mb.long_range_subset(pool)
    rt = 2 * math.pi
    for thr in ((0.0, 0.0), (0.05, 0.6)):
        outs, new = csm_ctx.csm(qs, 4, thr, rt=rt)
        assert max(2 * o["win_theta"] + 1 for o in outs) > 2048
        lits = _lits(oracle, pool, "csm", qs, (RX, RY, rt, 4, thr[0], thr[1]))
        for q, o, lit in zip(qs, outs, lits):
            _same_as_literal(o, lit, (q["name"], thr))
        csm_ctx.check_levels(oracle, new)


@pytest.mark.parametrize("H", [0, 2, 4])
def test_bnb_mixed_batch_equals_literal_and_builds_every_level(bnb_ctx, oracle, pool, H):
    """Every level the call builds (all missing box-max levels of all maps in one launch) equals the
    oracle's box maximum byte for byte."""
    qs = pool["queries"]
    assert len(set(_groups(qs, 1 << H))) >= 3
    outs, new = bnb_ctx.bnb(qs, H)
    lits = _lits(oracle, pool, "bnb", qs, (RX, RY, BNB_RT, H, BNB_THR[0], BNB_THR[1]))
    for q, o, lit in zip(qs, outs, lits):
        _same_as_literal(o, lit, (q["name"], H))
    if H > 0:
        assert new
    bnb_ctx.check_levels(oracle, new)


def _device_records(ctx, n):
    dev = torch.zeros(n * 48, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()            # the fill runs on torch's stream, the copy on the context's
    ctx.copy_last_batch_records(dev.data_ptr())
    ctx.synchronize()
    return dev.cpu().numpy()


def _orders(n):
    shuffled = list(range(n))
    random.Random(7).shuffle(shuffled)
    return {"forward": list(range(n)), "reversed": list(range(n))[::-1], "shuffled": shuffled}


@pytest.mark.parametrize("kind,param,thr", [("csm", 4, (0.05, 0.6)), ("csm", 5, (0.2, 0.3)), ("bnb", 2, BNB_THR)])
def test_record_does_not_depend_on_the_rest_of_the_batch(csm_ctx, bnb_ctx, oracle, pool, kind, param, thr):
    """A query's record in the mixed batch equals its record alone, in the reversed batch (the first
    query of the dense / sparse groups changes: both merging_pays outcomes decide fine.weighted) and
    in a shuffled one. After every mixed call the device copy of the records (record scatter through
    the group's index list, host patches of flagged queries) equals the host records in input order."""
    qs = pool["queries"]
    t = csm_ctx if kind == "csm" else bnb_ctx
    call = (lambda b, **kw: t.csm(b, param, thr, **kw)) if kind == "csm" else (lambda b, **kw: t.bnb(b, param, thr, **kw))
    unit = param if kind == "csm" else 1 << param
    keys = _groups(qs, unit)
    pays = [mb.merging_pays(q["angles"], q["ranges"], q["geom"][0]) for q in qs]
    ref = None
    for name, order in _orders(len(qs)).items():
        batch = [qs[i] for i in order]
        out, new = call(batch, as_records=True)
        t.check_levels(oracle, new)
        dev = _device_records(t.ctx, len(batch))
        assert np.array_equal(dev, out.record_bytes()), name
        got = [None] * len(qs)
        for j, i in enumerate(order):
            got[i] = _record(out[j])
        if ref is None:
            ref = got
            flagged = {keys[i] for i in range(len(qs)) if got[i]["raw"]["flags"] & mb.FLAGGED}
            assert len(flagged) >= 2, flagged          # patched queries in at least two groups
        else:
            for i in range(len(qs)):
                assert got[i] == ref[i], (name, qs[i]["name"], _diff(got[i], ref[i]))
        # what the first query of each dense / sparse group decides: weighted lists forward, not reversed
        firsts = {}
        for i in order:
            firsts.setdefault(keys[i], i)
        lead = {pays[i] for key, i in firsts.items() if len({pays[j] for j in range(len(qs)) if keys[j] == key}) == 2}
        if name == "forward":
            assert True in lead
        if name == "reversed":
            assert False in lead
    for i, q in enumerate(qs):
        one, _ = call([q])
        assert _record(one[0]) == ref[i], (q["name"], _diff(_record(one[0]), ref[i]))
    args = (RX, RY, RT, param, thr[0], thr[1]) if kind == "csm" else (RX, RY, BNB_RT, param, thr[0], thr[1])
    for q, r, lit in zip(qs, ref, _lits(oracle, pool, kind, qs, args)):
        _same_as_literal(r, lit, q["name"])


@pytest.mark.parametrize("bit", ["TUNE_NO_JOINT", "TUNE_NO_BOUND_PASS", "TUNE_NO_TWO_SLICES", "TUNE_NO_XCD_MAP"])
def test_fallback_paths_give_the_same_records(pool, oracle, bit):
    """The same mixed batches on a context with one launch optimisation switched off: identical
    records. The bound pass runs in some groups of the default context and in none without it."""
    base, alt = Tracked(pool), Tracked(pool, tuning_off=getattr(L, bit))
    try:
        qs = pool["queries"]
        for kind, param, thr in (("csm", 4, (0.05, 0.6)), ("csm", 5, (0.0, 0.0)), ("csm", 1, (0.2, 0.3)),
                                 ("bnb", 2, BNB_THR)):
            stats = []
            recs = []
            for t in (base, alt):
                t.ctx.bound_pass_stats()                      # reset
                out, _ = t.csm(qs, param, thr) if kind == "csm" else t.bnb(qs, param, thr)
                stats.append(t.ctx.bound_pass_stats())
                recs.append([_record(o) for o in out])
            for q, a, b in zip(qs, recs[0], recs[1]):
                assert a == b, (bit, kind, param, q["name"], _diff(a, b))
            if kind == "csm" and param > 1:
                assert sum(stats[0]) > 0, (kind, param, stats)
            if bit == "TUNE_NO_BOUND_PASS":
                assert stats[1] == (0, 0), stats
            if kind == "csm":
                lits = _lits(oracle, pool, "csm", qs, (RX, RY, RT, param, thr[0], thr[1]))
                for q, o, lit in zip(qs, recs[1], lits):
                    _same_as_literal(o, lit, (bit, q["name"]))
    finally:
        base.close()
        alt.close()


# (query, range x = range y, L, merge mode, score threshold, known-rate threshold)
RESIDENT = [("a_dense", 1.0, 4, 0, 0.0, 0.0), ("a_sparse", 1.0, 4, 0, 0.2, 0.0), ("a_one", 0.6, 1, 0, 0.0, 0.5),
            ("a_rel", 1.0, 5, 1, 0.0, 0.3),
            ("b_360", 1.0, 4, 0, 0.2, 0.3), ("b_long", 1.0, 4, 0, 0.0, 0.6), ("t_tie", 1.0, 4, 0, 0.0, 0.0),
            ("e_edge", 1.0, 5, 0, 0.0, 0.0), ("n_thin", 1.0, 5, 1, 0.1, 0.0), ("k_blocks", 0.6, 1, 0, 0.0, 0.0),
            ("u_unknown", 0.6, 1, 0, 0.3, 0.0), ("b_360", 0.6, 1, 0, 0.0, "beat"), ("b_long", 0.6, 1, 0, 0.0, "beat"),
            ("t_shared", 0.6, 1, 0, 0.0, "beat"),
            ("c_dense", 1.0, 4, 0, 0.0, 0.0), ("c_sparse", 1.0, 4, 0, 0.05, 0.6), ("c_tie", 1.0, 5, 1, 0.0, 0.0)]


def _beating_min_known(oracle, case, r):
    """A min_known that the window's greatest key fails and some candidate passes (L = 1: every
    candidate's own known count is tested): the winner lies below the bound pass's first round, only
    a second round finds it. The first window of the group needs no second round (min_known 1)."""
    _, S, K, _ = oracle.csm_closed_form(case, r, r, RT, 1, dump=True)
    mk = int(K[S == S.max()].max()) + 1
    assert mk > 1 and int(K.max()) >= mk
    return mk


def test_resident_windows_of_several_groups(pool, oracle):
    """csm_score_windows_dev with windows of other padded extents, L, merge modes, thresholds,
    beam counts and slice counts in one call: every record equals csm_score_window_dev's alone,
    unflagged ones the literal sweep; one window per group dumps its every candidate's S and K,
    which must equal the closed form."""
    dev = torch.device("cuda", 0)
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    by_name = {q["name"]: q for q in pool["queries"]}
    try:
        for mid, m in pool["maps"].items():
            ctx.upload_grid(mid, m["grid"])
            ctx.build_pyramid(mid, [1, 4, 5])
        coarse = {1: 0, 4: 1, 5: 2}
        ids, windows, cols, rows, keep, cases, params, keys = [], [], [], [], [], [], [], []
        for name, r, Lr, merge, sthr, kthr in RESIDENT:
            q = by_name[name]
            case = dict(mb.oracle_case(pool, q), rel_pose=(0.0, 0.0, 0.0))
            sx, sy, st = api.host_search_step(q["geom"][0], q["ranges"])
            wx, wy, wt = api.host_window(r, sx), api.host_window(r, sy), api.host_window(RT, st)
            col, row = api.host_project(q["geom"], q["init_pose"], st, wt, q["angles"], q["ranges"])
            n = len(q["angles"])
            if kthr == "beat":
                mk = _beating_min_known(oracle, case, r)
                kthr = (mk - 0.5) / n
                assert api.host_min_known(n, kthr) == mk
            windows.append(ctx.make_window(2 * wt + 1, n, wx, wy, Lr, coarse[Lr], api.host_min_known(n, kthr), sthr,
                                           merge_mode=merge))
            c_d, r_d = torch.from_numpy(col).to(dev), torch.from_numpy(row).to(dev)
            keep += [c_d, r_d]
            ids.append(q["map_id"])
            cols.append(c_d.data_ptr())
            rows.append(r_d.data_ptr())
            cases.append(case)
            params.append((r, r, RT, Lr, sthr, kthr))
            keys.append((mb.padded_extent(wx, Lr), mb.padded_extent(wy, Lr), Lr, merge))
        n = len(windows)
        assert len(set(keys)) >= 3 and len({k[:2] for k in keys}) >= 3
        dumped = {}
        for k, key in enumerate(keys):
            dumped.setdefault(key, k)
        want = {}
        ds, dk, bufs = [0] * n, [0] * n, {}
        for k in dumped.values():
            want[k] = _EXEC.submit(oracle.csm_closed_form, cases[k], *params[k], dump=True)
        for k in dumped.values():
            want[k] = want[k].result()
            S = torch.zeros(want[k][1].size, dtype=torch.int32, device=dev)
            K = torch.zeros(want[k][2].size, dtype=torch.int16, device=dev)
            bufs[k] = (S, K)
            ds[k], dk[k] = S.data_ptr(), K.data_ptr()
        single = torch.zeros(n * 48, dtype=torch.uint8, device=dev)
        for k in range(n):
            ctx.score_window_dev(ids[k], windows[k], cols[k], rows[k], single.data_ptr() + 48 * k)
        batch = torch.zeros(n * 48, dtype=torch.uint8, device=dev)
        dumps = torch.zeros(n * 48, dtype=torch.uint8, device=dev)
        prepared = ctx.prepare_windows(ids, windows, cols, rows)
        ctx.score_windows_dev(prepared, batch.data_ptr())
        ctx.score_windows_dump_dev(prepared, dumps.data_ptr(), ds, dk, [0] * n)
        torch.cuda.synchronize(dev)
        a = single.cpu().numpy().reshape(n, 48)
        b = batch.cpu().numpy().reshape(n, 48)
        c = dumps.cpu().numpy().reshape(n, 48)
        lits = [_EXEC.submit(oracle.csm, cases[k], *params[k]) for k in range(n)]
        for k in range(n):
            assert np.array_equal(a[k], b[k]), (RESIDENT[k], L.Result.from_buffer_copy(a[k].tobytes()).flags,
                                                L.Result.from_buffer_copy(b[k].tobytes()).flags)
            assert np.array_equal(b[k], c[k]), RESIDENT[k]
            rb = L.Result.from_buffer_copy(b[k].tobytes())
            if rb.flags & (L.FLAG_EDGE_BAND | L.FLAG_KEY_TIE):
                continue                                  # finished by the exact single-window paths
            lit = lits[k].result()
            assert rb.found == lit["found"], RESIDENT[k]
            if lit["found"]:
                assert (rb.best_x, rb.best_y, rb.best_theta) == (lit["bestX"], lit["bestY"], lit["bestT"]), RESIDENT[k]
                assert rb.score == lit["scoreMax"], RESIDENT[k]
        for k, (S, K) in bufs.items():
            _, oS, oK, _ = want[k]
            assert np.array_equal(S.cpu().numpy().view(np.uint32).reshape(oS.shape), oS), RESIDENT[k]
            assert np.array_equal(K.cpu().numpy().view(np.uint16).reshape(oK.shape), oK), RESIDENT[k]
    finally:
        ctx.close()


def test_back_to_back_calls_on_one_context(pool, oracle):
    """A large mixed call, a small call of another shape, the large call again: the third equals the
    first. Then calls on the same resident maps with range_x growing and shrinking (the pair-row
    copy's padding only grows) and with L changing (more cached levels per map), each checked
    against the literal sweep and its new levels against the box maximum."""
    t = Tracked(pool)
    try:
        qs = pool["queries"]
        first, new = t.csm(qs, 4, (0.2, 0.3))
        t.check_levels(oracle, new)
        small = [q for q in qs if q["name"] in ("b_360", "c_sparse")]
        _, new = t.csm(small, 3, (0.0, 0.0), rx=0.5, ry=1.6, rt=math.radians(4))
        t.check_levels(oracle, new)
        third, _ = t.csm(qs, 4, (0.2, 0.3))
        for q, a, b in zip(qs, first, third):
            assert _record(a) == _record(b), (q["name"], _diff(_record(a), _record(b)))
        sub = [q for q in qs if len(q["angles"]) <= 1080]
        for rx, Lr, thr in ((0.5, 4, (0.0, 0.0)), (1.6, 4, (0.2, 0.3)), (0.8, 4, (0.0, 0.0)), (1.0, 2, (0.05, 0.6)),
                            (1.0, 6, (0.0, 0.0)), (1.0, 3, (0.2, 0.3)), (0.7, 2, (0.0, 0.0))):
            outs, new = t.csm(sub, Lr, thr, rx=rx)
            lits = _lits(oracle, pool, "csm", sub, (rx, RY, RT, Lr, thr[0], thr[1]))
            for q, o, lit in zip(sub, outs, lits):
                _same_as_literal(o, lit, (q["name"], rx, Lr, thr))
            t.check_levels(oracle, new)
    finally:
        t.close()
