#!/usr/bin/env python3
"""Records what every case of tests/plan_cases.py chooses and computes on the
GPU: the candidate kernel's name and path, the launch geometry, the rescan
count and a hash of labels and flags.  Run at a commit whose behaviour is the
reference for a later refactor; tests/test_gpu_plan.py holds the next commits
to the table.

  python tools/record_plans.py --commit $(git rev-parse HEAD) --out tests/plan_parent.json

Every case runs twice, each on a fresh classifier: a case whose two runs
differ is listed under "unstable" (and not under "cases")."""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

try:  # import torch before the HIP library is loaded (see knn_amd.lib())
    import torch  # noqa: F401
except Exception:
    pass


def load_knn():
    spec = importlib.util.spec_from_file_location(
        "knn_amd", os.path.join(ROOT, "-mpi-knn-_amd", "knn_amd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--commit", required=True, help="hash of the commit being recorded")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import plan_cases
    knn = load_knn()
    table = {"commit": args.commit, "cases": {}, "unstable": {}}
    for case in plan_cases.CASES:
        a = plan_cases.run_case(knn, case)
        b = plan_cases.run_case(knn, case)
        if a == b:
            table["cases"][case["id"]] = a
        else:
            table["unstable"][case["id"]] = [a, b]
        print(case["id"], a if a == b else ("UNSTABLE", a, b), flush=True)
    with open(args.out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
