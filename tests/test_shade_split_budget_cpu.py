"""Register, scratch and LDS budgets of the split shade kernels (k_shade_split<1>: camera vertices, k_shade_split<2>: later bounces), read from the built
library. They run under the four-wave bound of k_shade<1, .., 1> and may spill no more than that kernel did before they existed: 4 dwords.

As built: k_shade_split<1> 16 B of scratch, 3 spilled dwords, 30988 B of LDS; k_shade_split<2> 20 B, 4 dwords, 33036 B (MEASUREMENTS.md R8)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_SPILLED_DWORDS = 4  # k_shade<1, false, false, false, false, 1> in the build before the split (128 VGPRs, 20 B of scratch)


@pytest.fixture(scope="module")
def resources(host):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_budget
    finally:
        sys.path.pop(0)
    return kernel_budget.kernel_resources(host.HIP_LIB)


@pytest.mark.parametrize("name", ["rtx::k_shade_split<1>", "rtx::k_shade_split<2>"])
def test_split_kernel_budgets(resources, name):
    r = resources[name]
    print(name, r)
    assert r["vgpr"] <= 128, r
    assert r["scratch"] <= 32, r
    assert r["lds"] <= 36864, r
    assert r["vgpr_spills"] <= PARENT_SPILLED_DWORDS, r


def test_the_old_kernel_keeps_its_name_and_allocation(resources):
    r = resources["rtx::k_shade<1, false, false, false, false, 1>"]
    assert r["vgpr"] <= 128 and r["scratch"] <= 20 and r["vgpr_spills"] <= PARENT_SPILLED_DWORDS, r
