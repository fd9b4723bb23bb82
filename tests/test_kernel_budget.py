"""Register budget of the lane-mapped hot kernels and scratch of every kernel, read from the code objects' metadata as
tools/kernel_resources.py reads it (register counts only; no instruction text is looked at).  No GPU.

The shared k_search<0, true> / k_search<1, true> and k_backward<2> hold the problem's fixed-size parameters per lane
(ilqg_kernels.hip load_params): the searches then spill no scalar register, the fused sweep no more than its per-trajectory
twin, and none of them uses scratch memory.  tests/golden/kernel_scratch_parent.json lists, per library, the kernels that used
scratch memory before that change, with the bytes per lane (names as `kernel_resources.py --digest` prints them: in full);
no kernel of any library that is built may use more."""
import glob
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, ROOT

TWIN = ", double const*, PolicyParamMap>"


@pytest.fixture(scope="module")
def resources():
    import __graft_entry__ as g
    g.load_package()
    from ddp_generator_amd import ilqg
    if not os.path.exists(ilqg.library_path("carparking", 0)):
        g.build()
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    return ilqg, kr


@pytest.fixture(scope="module")
def car(resources):
    ilqg, kr = resources
    return {k["name"]: k for k in kr.kernels(ilqg.library_path("carparking", 0))}


@pytest.mark.parametrize("name", ["k_search<0, true>", "k_search<1, true>"])
def test_the_shared_searches_spill_no_scalar_register(car, name):
    k = car[name]
    print(name, k)
    assert k.get("sgpr_spill", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("scratch", 0) == 0


def test_the_shared_fused_sweep_spills_no_more_than_its_twin(car):
    k, twin = car["k_backward<2>"], car["k_backward<2" + TWIN]
    print(k, twin)
    assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0
    assert k.get("sgpr_spill", 0) <= twin.get("sgpr_spill", 0)


def test_no_kernel_of_any_library_gained_scratch(resources):
    ilqg, kr = resources
    before = json.load(open(os.path.join(GOLDEN, "kernel_scratch_parent.json")))
    libs = sorted(glob.glob(os.path.join(os.path.dirname(ilqg.library_path("carparking", 0)), "libilqg_*.so")))
    assert libs
    more = []
    for path in libs:
        was = before.get(os.path.basename(path), {})
        for k in kr.kernels(path):
            if k.get("scratch", 0) > was.get(k["name"], 0):
                more.append((os.path.basename(path), k["name"], was.get(k["name"], 0), k["scratch"]))
    assert not more, "scratch bytes per lane (library, kernel, before, now): %r" % more
