"""The shade kernels' vertex bodies re-read their arguments from the kernarg segment (RT_SHADE_KARGS, rtx_shade_body.inl) at offsets computed from a
struct of the same members. Held here, on the built library: (a) the offsets rt_shade_karg_offsets reports are the `.offset` entries of the kernels' argument
metadata in the code object, for one kernel of each signature; (b) what the re-read buys - the three kernels of a Cornell-box frame and k_shade<3> plain spill
no vector register and have no scratch frame, and no other shade kernel spills more dwords or has a larger scratch frame than in the build before (PARENT: the
figures of that build's notes, MEASUREMENTS.md R10); (c) the control kernels (RTX_SHADE_KARGS=0) exist under their own names with the allocation of that build."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (spilled dwords, bytes of scratch) of every shade kernel in the build before the re-read
PARENT = {
    "rtx::k_shade<0, false, false, false, false, 0>": (18, 1696),
    "rtx::k_shade<0, true, false, false, false, 0>": (19, 1712),
    "rtx::k_shade<1, false, false, false, false, 0>": (4, 20),
    "rtx::k_shade<1, false, false, false, false, 1>": (4, 20),
    "rtx::k_shade<1, false, false, false, false, 3>": (5, 24),
    "rtx::k_shade<3, false, false, false, false, 0>": (25, 64),
    "rtx::k_shade<3, false, false, false, false, 3>": (25, 64),
    "rtx::k_shade<3, false, false, true, false, 0>": (0, 0),
    "rtx::k_shade<3, false, false, true, false, 3>": (0, 0),
    "rtx::k_shade<3, false, true, false, false, 0>": (0, 0),
    "rtx::k_shade<3, false, true, false, false, 2>": (0, 0),
    "rtx::k_shade<3, false, true, false, true, 0>": (0, 0),
    "rtx::k_shade<3, false, true, false, true, 1>": (0, 0),
    "rtx::k_shade<3, false, true, false, true, 2>": (0, 0),
    "rtx::k_shade<3, true, false, false, false, 0>": (0, 368),
    "rtx::k_shade<5, false, false, false, false, 0>": (52, 128),
    "rtx::k_shade<5, false, false, false, false, 3>": (55, 144),
    "rtx::k_shade<5, false, true, false, false, 0>": (0, 0),
    "rtx::k_shade<5, false, true, false, false, 2>": (0, 0),
    "rtx::k_shade<5, false, true, false, true, 0>": (0, 0),
    "rtx::k_shade<5, false, true, false, true, 1>": (0, 0),
    "rtx::k_shade<5, false, true, false, true, 2>": (0, 0),
    "rtx::k_shade<5, true, false, false, false, 0>": (29, 432),
    "rtx::k_shade<6, false, false, false, false, 0>": (65, 144),
    "rtx::k_shade<6, false, false, false, false, 3>": (65, 160),
    "rtx::k_shade<6, false, true, false, false, 0>": (0, 0),
    "rtx::k_shade<6, false, true, false, false, 2>": (0, 0),
    "rtx::k_shade<6, false, true, false, true, 0>": (0, 0),
    "rtx::k_shade<6, false, true, false, true, 1>": (0, 0),
    "rtx::k_shade<6, false, true, false, true, 2>": (0, 0),
    "rtx::k_shade<6, true, false, false, false, 0>": (34, 448),
    "rtx::k_shade_rays<0, false>": (0, 1680),
    "rtx::k_shade_rays<0, true>": (0, 1680),
    "rtx::k_shade_rays<3, false>": (16, 32),
    "rtx::k_shade_rays<3, true>": (0, 368),
    "rtx::k_shade_rays<5, false>": (38, 80),
    "rtx::k_shade_rays<5, true>": (4, 384),
    "rtx::k_shade_rays<6, false>": (45, 96),
    "rtx::k_shade_rays<6, true>": (24, 416),
    "rtx::k_shade_split<1>": (3, 16),
    "rtx::k_shade_split<2>": (4, 20),
}
# nothing spilled, no scratch: a Cornell-box frame's three kernels and the plain Lambert front-end under any light
CLEAN = ["rtx::k_shade_split<1>", "rtx::k_shade_split<2>", "rtx::k_shade<1, false, false, false, false, 1>",
         "rtx::k_shade<3, false, false, false, false, 0>", "rtx::k_shade<3, false, false, false, false, 3>"]
# the control kernels and the kernel each stands in for
CONTROL = {"rtx::k_shade_split_live<1>": "rtx::k_shade_split<1>", "rtx::k_shade_split_live<2>": "rtx::k_shade_split<2>",
           "rtx::k_shade_const_live<1>": "rtx::k_shade<1, false, false, false, false, 1>"}


@pytest.fixture(scope="module")
def resources(host):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_budget
    finally:
        sys.path.pop(0)
    return kernel_budget.kernel_resources(host.HIP_LIB)


@pytest.fixture(scope="module")
def offsets(host):
    out = (ctypes.c_uint32 * 5)()
    host.hip_lib().rt_shade_karg_offsets(out)
    return list(out)


def test_offsets_are_aligned_and_ordered(offsets):
    sc, fp, ps, hit_mask, rdiff = offsets
    assert sc == 0 and sc < fp < ps < hit_mask and ps < rdiff
    assert all(o % 8 == 0 for o in offsets)  # (every argument holds a pointer or a 64-bit count)


@pytest.mark.parametrize("name,last", [("rtx::k_shade<1, false, false, false, false, 1>", None), ("rtx::k_shade<3, false, false, false, false, 0>", None),
                                       ("rtx::k_shade<0, true, false, false, false, 0>", None), ("rtx::k_shade_split<1>", 3), ("rtx::k_shade_split<2>", 3),
                                       ("rtx::k_shade_rays<3, false>", 4), ("rtx::k_shade_rays<0, true>", 4)])
def test_offsets_are_the_code_objects(resources, offsets, name, last):
    """the explicit arguments' offsets in the kernel's metadata: (sc, fp, ps) and, for the two longer signatures, the fourth argument"""
    want = offsets[:3] + ([offsets[last]] if last is not None else [])
    assert resources[name]["arg_offsets"] == want, (name, resources[name]["arg_offsets"], want)


def test_every_shade_kernel_of_the_parent_is_still_built(resources):
    assert set(PARENT) <= set(resources), sorted(set(PARENT) - set(resources))
    shade = {k for k in resources if k.startswith(("rtx::k_shade<", "rtx::k_shade_split<", "rtx::k_shade_rays<"))}
    assert shade == set(PARENT), sorted(shade ^ set(PARENT))  # (a new form needs its own line above)


@pytest.mark.parametrize("name", CLEAN)
def test_nothing_spilled_where_the_frames_are(resources, name):
    r = resources[name]
    print(name, r)
    assert r["vgpr_spills"] == 0 and r["scratch"] == 0, r


@pytest.mark.parametrize("name", sorted(PARENT))
def test_no_kernel_spills_more_than_before(resources, name):
    r = resources[name]
    print(name, r, PARENT[name])
    assert r["vgpr_spills"] <= PARENT[name][0] and r["scratch"] <= PARENT[name][1], (r, PARENT[name])


@pytest.mark.parametrize("name", sorted(CONTROL))
def test_control_kernels_have_the_parents_allocation(resources, name):
    r = resources[name]
    print(name, r)
    assert r["vgpr"] <= 128 and (r["vgpr_spills"], r["scratch"]) == PARENT[CONTROL[name]], r
    assert r["sgpr_spills"] > resources[CONTROL[name]]["sgpr_spills"]  # (what the re-read frees: the scalars parked in vector lanes)
