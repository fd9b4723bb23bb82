"""The launch plan of an iteration stays what it was: for every case of tests/launch_plan_cases.py — every branch of the device
shim's launch layer (the search's three forms and their stages, fused and unfused derivatives, the rows twins, the stage-by-
stage calls, multipliers; in the wave mapping the quad, speculative, row and per-element sweeps, the pieces and chunks of the
work buffer, roll-outs in parts or not, records through LDS or not, derivative records in parts) — kernel_times() reports the
launch counts the commit before the launch layer was restated gave (tests/golden/launch_counts_parent.json, recorded on an
MI355X; profiles/r19_launch_layer.txt has the byte-for-byte comparison of the results made then)."""
import gc
import json
import os

import pytest

from conftest import GOLDEN, load_package
from launch_plan_cases import CASES, ENV, run
from test_gpu_parity import ilqg  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "launch_counts_parent.json")) as f:
    PARENT = json.load(f)


def test_every_case_has_a_record():
    assert sorted(PARENT) == sorted(c["name"] for c in CASES)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_launch_counts_are_the_parents(ilqg, monkeypatch, c):  # noqa: F811
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in c["env"].items():
        monkeypatch.setenv(name, value)
    gc.collect()  # the device's work buffer goes with its last user and is sized by the next first one (ILQG_WORK_GB)
    assert run(load_package(), c)[1] == PARENT[c["name"]]
