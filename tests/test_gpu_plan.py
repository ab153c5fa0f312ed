"""The search plan moved into csrc/knn_plan.cpp without moving a decision:
every case of plan_cases.py launches the kernel, takes the path and geometry,
rescans as many queries and computes the labels and flags that the commit
before the move did (plan_parent.json, recorded there on an MI355X by
tools/record_plans.py)."""
import importlib.util
import json
import os

import pytest

import plan_cases

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "plan_parent.json")) as f:
    PARENT = json.load(f)


@pytest.fixture(scope="module")
def knn():
    spec = importlib.util.spec_from_file_location(
        "knn_amd", os.path.join(os.path.dirname(HERE), "-mpi-knn-_amd", "knn_amd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if mod.lib().knn_device_count() < 1:
        pytest.fail("no HIP device visible: the KNN path has no CPU fallback")
    return mod


def test_table_covers_every_case():
    assert len(PARENT["commit"]) == 40
    assert not PARENT["unstable"]
    assert sorted(PARENT["cases"]) == sorted(c["id"] for c in plan_cases.CASES)


@pytest.mark.parametrize("case", plan_cases.CASES, ids=lambda c: c["id"])
def test_plan_matches_parent(knn, case):
    want = PARENT["cases"][case["id"]]
    got = plan_cases.run_case(knn, case)
    for field in plan_cases.FIELDS:
        assert got[field] == want[field], (field, got, want)
