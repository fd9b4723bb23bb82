"""Resources of the kernels of the drawn process noise, read from the code objects' metadata as tools/kernel_resources.py
reads it (no instruction text is looked at).  No GPU.

Where a problem's policy roll-out needs no scratch memory (N_X <= 8) the drawn form is a kernel of its own, k_policy_drawn,
k_policy's text with the noise drawn in registers (k_policy_body.inc): each instantiation exists beside its k_policy twin,
uses no scratch memory and the twin's LDS.  Where the roll-outs keep their trajEl_t in scratch memory (N_X > 8) there is NO
second kernel — k_policy itself takes the drawn form as a run-time argument — so that no new kernel name uses scratch memory
(tests/test_kernel_budget.py holds every kernel to tests/golden/kernel_scratch_parent.json, which is the parent's).
k_noise_fill, which writes the same draws as a table, uses no scratch memory, spills nothing and has no LDS in any library."""
import glob
import importlib.util
import os

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def libraries():
    import __graft_entry__ as g
    g.load_package()
    from ddp_generator_amd import ilqg
    if not os.path.exists(ilqg.library_path("carparking", 0)):
        g.build()
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    libs = sorted(glob.glob(os.path.join(os.path.dirname(ilqg.library_path("carparking", 0)), "libilqg_*.so")))
    assert libs
    return {os.path.basename(p): {k["name"]: k for k in kr.kernels(p)} for p in libs}


def test_a_drawn_kernel_exists_exactly_where_the_rollout_needs_no_scratch(libraries):
    wrong = []
    for lib, kernels in libraries.items():
        plain = [n for n in kernels if n.startswith("k_policy<")]
        drawn = [n for n in kernels if n.startswith("k_policy_drawn<")]
        assert plain, lib
        if any(kernels[n].get("scratch", 0) for n in plain):
            if drawn:
                wrong.append((lib, "k_policy uses scratch memory and there is a second kernel", drawn))
            continue
        if sorted(drawn) != sorted("k_policy_drawn" + n[len("k_policy"):] for n in plain):
            wrong.append((lib, "not one drawn kernel per k_policy instantiation", drawn))
        for n in drawn:
            twin = kernels["k_policy" + n[len("k_policy_drawn"):]]
            if kernels[n].get("scratch", 0) != 0 or kernels[n].get("lds", 0) != twin.get("lds", 0):
                wrong.append((lib, n, kernels[n].get("scratch", 0), kernels[n].get("lds", 0), twin.get("lds", 0)))
    assert not wrong, repr(wrong)
    assert any(n.startswith("k_policy_drawn<") for n in libraries["libilqg_carparking_fd0_hip.so"])


def test_the_table_kernel_needs_no_scratch_and_no_lds(libraries):
    for lib, kernels in libraries.items():
        k = kernels["k_noise_fill"]
        assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0 and k.get("lds", 0) == 0, (lib, k)
