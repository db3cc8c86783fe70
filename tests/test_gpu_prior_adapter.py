"""GPU parity of the Python adapter's motion-prior option: ScanMatcherCorrelativeHIP(prior_information=...)
equals the direct csm_correlative_match_prior call and reports the unweighted winner beside the summary;
without the option the adapter is unchanged."""
import math

import pytest

import prior_reference as P
from csm_hip import api, synth
from test_gpu_prior import LAMBDAS, RANGE, _six

pytestmark = pytest.mark.gpu


def test_python_adapter_with_a_prior_equals_the_direct_call(gpu_ctx):
    L = 4
    case, vol, ref, _ = _six(0, L, "full")
    assert ref["best"] != ref["unweighted"]
    strip = lambda o: {k: v for k, v in o.items() if not k.endswith("_us")}
    plain = api.ScanMatcherCorrelativeHIP("plain", L, *RANGE, ctx=gpu_ctx)
    prior = api.ScanMatcherCorrelativeHIP("prior", L, *RANGE, ctx=gpu_ctx, prior_information=LAMBDAS["full"])
    args = (case["grid"], case["geom"], case["angles"], case["ranges"], case["rel_pose"], case["init_pose"])
    before = plain.optimize_pose(*args)
    out = prior.optimize_pose(*args, map_id=77)
    direct = gpu_ctx.correlative_match_prior(77, case["geom"], case["angles"], case["ranges"], case["rel_pose"],
                                             case["init_pose"], *RANGE, L, LAMBDAS["full"])
    assert direct["prior"] == ref
    assert out["raw"] == ref["best"] and out["unweighted"] == ref["unweighted"] and out["prior"] == ref
    assert strip({k: v for k, v in out.items() if k not in ("unweighted", "prior")}) == strip(direct["summary"])
    assert out["estimated_pose"] != before["estimated_pose"] and before["raw"] == ref["unweighted"]
    assert strip(plain.optimize_pose(*args)) == strip(before)
    gpu_ctx.release_grid(77)
