"""Writes tests/golden/launch_plans.json, the fixture of tests/test_launch_plans_cpu.py: per model the frame plans of the depth-first walks
(three algorithms, seven budgets, knapsack and leaves-upwards), the run-time tree split with its three record sets and launch shapes, and
the launch choice and geometry of the depth-first kernels over CU counts, batches and the placement switches -- SHA-256 of the big tables,
the scalars verbatim.

It was written from a library whose planners (mecano_amd/csrc/mh_launch_plans.h) were the text of dfs_plan, split_rt_plan,
split_rt_upload_meta, dfs_choose, dfs_setup and launch_split_rt moved unchanged: it pins the plans to what the library made before the
restructuring.  The planners are deterministic, so a run on an unchanged library reproduces the file byte for byte; a run that changes it
is a finding in the planners, never a reason to commit the new file.  Data only.
python tests/golden/make_launch_plan_fixtures.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))


def main():
    import test_launch_plans_cpu as t
    from mecano_amd import _lib
    lib = _lib.load()
    planners = {name: t.Planner(lib, name) for name in t.SPLIT_MODELS}
    doc = {"comment": "Launch plans (mecano_amd/csrc/mh_launch_plans.h) per model, from the statements of mh_api.hip as they stood before they moved; "
                      "tests/golden/make_launch_plan_fixtures.py.",
           "frames": {name: t.frames_digest(planners[name]) for name in t.MODELS},
           "split": {name: t.split_digest(planners[name]) for name in t.SPLIT_MODELS},
           "choice": {name: t.choice_digest(planners[name]) for name in t.CHOICE_MODELS}}
    path = os.path.join(HERE, "launch_plans.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
