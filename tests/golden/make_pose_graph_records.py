#!/usr/bin/env python3
"""Generates tests/golden/pose_graph_records.json ON A GPU BOX: what csm_pose_graph_lm (both solvers) and
csm_pose_graph_marginals of the library of THIS commit compute on the seeded cases of
tests/pose_graph_record_cases.py, every double as its float.hex() string. A refactor of the pose-graph unit is
run against the records of its parent. Usage (GPU box): python tests/golden/make_pose_graph_records.py OUT.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "my-lidar-graph-slam-v2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(out_path):
    import __graft_entry__ as ge
    ge.build()
    from csm_hip import api
    import pose_graph_record_cases as cases
    ctx = api.Context(0)
    doc = {"generator": "tests/golden/make_pose_graph_records.py", "library": ctx.lib.csm_version().decode()}
    doc.update(cases.record(ctx))
    ctx.close()
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out_path)
    for family in sorted(doc):
        if isinstance(doc[family], dict):
            for name in sorted(doc[family]):
                print(family, name, json.dumps(doc[family][name], sort_keys=True)[:200])


if __name__ == "__main__":
    main(sys.argv[1])
