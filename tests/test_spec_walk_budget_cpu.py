"""Register, scratch and LDS budgets of the closest-hit link walk's form with leaf holders that keep walking (k_trace_spec<1>; a further form, were one built,
is held to the same), read from the built library: they run under the seven-wave bound of the kernel they stand in for, k_trace<false, false, 256, 16, 0, 0> - 72 VGPRs, nothing spilled, no scratch, and LDS
that lets seven workgroups share a CU - and that kernel keeps its own allocation."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = "rtx::k_trace<false, false, 256, 16, 0, 0>"


@pytest.fixture(scope="module")
def resources(host):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_budget
    finally:
        sys.path.pop(0)
    return kernel_budget.kernel_resources(host.HIP_LIB)


def _seven_waves(r):
    assert r["vgpr"] + r["agpr"] <= 72, r          # 8-register granules: 73 would be 80, six waves per SIMD
    assert r["scratch"] == 0 and r["vgpr_spills"] == 0, r
    assert 7 * r["lds"] <= 160 * 1024, r           # seven 256-lane workgroups per CU


def test_the_forms_that_are_built_fit_seven_waves(resources):
    forms = sorted(k for k in resources if k.startswith("rtx::k_trace_spec<"))
    assert "rtx::k_trace_spec<1>" in forms, forms      # the form S1's frames run by default (MEASUREMENTS R9)
    for name in forms:
        print(name, resources[name])
        _seven_waves(resources[name])
        assert resources[name]["lds"] == resources[PLAIN]["lds"]   # the same staged scene: nothing added to LDS


def test_the_as_built_walk_keeps_its_name_and_allocation(resources):
    _seven_waves(resources[PLAIN])
