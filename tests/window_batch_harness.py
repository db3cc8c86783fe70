"""What the GPU tests of the coarse-first window batches share (test_gpu_coarse_first.py,
test_gpu_beam_ladder.py): a batch of resident windows prepared once for score_windows_dev, the same batch on a
default context and on one without the bound pass, and csm_correlative_match_batch with the loop detector's
thresholds on both. Records flagged EDGE_BAND or KEY_TIE are finished by the single-window path, as in
test_gpu_headline.py. The reference is always the oracle's literal sweep."""
import torch

from csm_hip import _lib as L, api

import unit_bound_cases as U


def _want(oracle, case, rx, ry, rt, Lr, sthr=0.0, kthr=0.0):
    lit = oracle.csm(case, rx, ry, rt, Lr, sthr, kthr)
    return (lit["found"], lit["bestX"], lit["bestY"], lit["bestT"], lit["scoreMax"])


class Batch:
    """Windows of several (map id, case) prepared once for score_windows_dev."""

    def __init__(self, ctx, items, rx, ry, rt, Lr):
        self.ctx, self.items, self.dev = ctx, items, torch.device("cuda", 0)
        self.keep, self.windows, self.hits = [], [], []
        cols, rows = [], []
        for map_id, case in items:
            w = U.window_of(case, rx, ry, rt, Lr)
            n = len(case["angles"])
            self.windows.append(ctx.make_window(2 * w["wt"] + 1, n, w["wx"], w["wy"], Lr, 1, api.host_min_known(n, 0.0), 0.0))
            self.hits.append((w["col"], w["row"]))
            self.keep += [torch.from_numpy(w["col"]).to(self.dev), torch.from_numpy(w["row"]).to(self.dev)]
            cols.append(self.keep[-2].data_ptr())
            rows.append(self.keep[-1].data_ptr())
        self.out = torch.zeros(len(items) * 48, dtype=torch.uint8, device=self.dev)
        self.prepared = ctx.prepare_windows([m for m, _ in items], self.windows, cols, rows)

    def score(self):
        """(records finished as the header says, flagged records, (units scored, units skipped))"""
        self.out.zero_()
        self.ctx.bound_pass_stats()
        self.ctx.score_windows_dev(self.prepared, self.out.data_ptr())
        torch.cuda.synchronize(self.dev)
        stats = self.ctx.bound_pass_stats()
        raw = self.out.cpu().numpy().tobytes()
        final, flagged = [], 0
        for k, (map_id, _) in enumerate(self.items):
            r = L.Result.from_buffer_copy(raw[48 * k:48 * (k + 1)])
            if r.flags & (L.FLAG_EDGE_BAND | L.FLAG_KEY_TIE):
                flagged += 1
                d = self.ctx.score_window(map_id, self.windows[k], *self.hits[k])
                final.append((d["found"], d["best_x"], d["best_y"], d["best_theta"], d["score"]))
            else:
                final.append((r.found, r.best_x, r.best_y, r.best_theta, r.score))
        return final, flagged, stats


def _context(tuning_off=0):
    c = api.Context(0, tuning_off=tuning_off)
    c.set_stream(torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream)
    return c


def _both_contexts(items, rx, ry, rt, Lr, grids):
    """The batch on a default context and on one without the bound pass: records, flagged, stats of each."""
    outs = []
    for off in (0, L.TUNE_NO_BOUND_PASS):
        ctx = _context(off)
        for map_id, grid in grids.items():
            ctx.upload_grid(map_id, grid)
            ctx.build_pyramid(map_id, [1, Lr])
        outs.append(Batch(ctx, items, rx, ry, rt, Lr).score())
        ctx.close()
    return outs


THR = (0.55, 0.6)           # LoopDetectorCorrelative's score and known-rate thresholds


def _match_batches(oracle, cases, rx, ry, rt, Lr, first_id):
    """csm_correlative_match_batch with THR on a default context and on one without the bound pass: every
    summary equals the oracle's literal sweep, found or not found, and the two contexts agree. Returns the
    default context's (units scored, units skipped) and the oracle's found flags."""
    wants = [oracle.csm(c, rx, ry, rt, Lr, *THR) for c in cases]
    qs = [dict(map_id=first_id + i, geom=c["geom"], angles=c["angles"], ranges=c["ranges"], rel_pose=c["rel_pose"],
               init_pose=c["init_pose"]) for i, c in enumerate(cases)]
    stats, plain = None, []
    for off in (0, L.TUNE_NO_BOUND_PASS):
        ctx = _context(off)
        for q, c in zip(qs, cases):
            ctx.upload_grid(q["map_id"], c["grid"])
        ctx.bound_pass_stats()
        outs = ctx.correlative_match_batch(qs, rx, ry, rt, Lr, *THR)
        if off == 0:
            stats = ctx.bound_pass_stats()
        else:
            assert ctx.bound_pass_stats() == (0, 0)
        ctx.close()
        for o, want in zip(outs, wants):
            assert o["pose_found"] == want["found"]
            if want["found"]:
                assert (o["raw"]["best_x"], o["raw"]["best_y"], o["raw"]["best_theta"]) == \
                    (want["bestX"], want["bestY"], want["bestT"])
                assert o["raw"]["score"] == want["scoreMax"]
            assert o["estimated_pose"] == want["estimatedPose"]
        plain.append([(o["pose_found"], o["raw"]["best_x"], o["raw"]["best_y"], o["raw"]["best_theta"], o["raw"]["score"])
                      for o in outs])
    assert plain[0] == plain[1]
    return stats, [w["found"] for w in wants]
