"""The closest-hit link walk of an LDS-resident scene of plain triangles with leaf holders that keep walking (k_trace_spec<1>, RTX_LDS_SPEC read per scene)
against the walk as built (RTX_LDS_SPEC=0, k_trace<false, false, 256, 16>): hit records bit for bit through the batch entry point, a frame's film bit for bit with every
integer of its stats, and the counting frame (the stack walk: no form touches it) unchanged. Rays of the fuzz's classes (scripts/fuzz_lds_walks.py): random, zero and
denormal direction components, axis-parallel, origins on vertices; whole waves of zero-component rays, which walk link8_full in the as-built form whatever the knob says;
ray counts of 1, 63, 65 and 40 000."""
import ctypes
import os

import numpy as np
import pytest

from rustracer_amd.scenes import cornell_box, random_soup

pytestmark = pytest.mark.gpu
KNOB = "RTX_LDS_SPEC"
N_RAYS = 40000

SCENES = {
    "cornell": (lambda: cornell_box(32, 32, 1), [-50, -50, -850], [600, 600, 600]),                       # 32 triangles
    "soup-126": (lambda: random_soup(126, seed=5, max_prims=4), [-20] * 3, [120] * 3),                    # leaves of 4
    "soup-40-degenerate": (lambda: random_soup(40, seed=9, max_prims=1, degenerate=True), [-20] * 3, [120] * 3),
}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rays(desc, lo, hi, n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = np.float32(lo), np.float32(hi)
    verts = desc.arrays()[0]
    org = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    k = np.arange(n)
    d[k % 11 == 0, rng.integers(0, 3)] = 0.0
    d[k % 13 == 0, rng.integers(0, 3)] = -0.0
    d[k % 17 == 0] = np.float32([0, 0, 1])                      # axis-parallel
    d[k % 19 == 0, rng.integers(0, 3)] = 1e-39                  # a denormal component: its reciprocal overflows
    wave = k // 64
    whole = (wave % 5 == 3)                                     # every fifth wave: a zero component in every lane ...
    d[whole, 1] = 0.0
    clean = (wave % 5 == 1)                                     # ... and one without any: the min / max node test, the forms under test
    fresh = rng.normal(size=(n, 3)).astype(np.float32)
    fresh /= np.linalg.norm(fresh, axis=1, keepdims=True)
    d[clean] = fresh[clean]
    sel = k % 7 == 0
    org[sel] = verts[rng.integers(0, len(verts), int(sel.sum()))]   # origins on box bounds (a vertex lies on the bounds of every node above it)
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3] = org
    rays[:, 3] = np.where(k % 5 == 0, rng.uniform(1, 700, n), np.inf).astype(np.float32)
    rays[:, 4:7] = d
    return rays


def _with_knob(value, fn):
    saved = os.environ.pop(KNOB, None)
    try:
        if value is not None:
            os.environ[KNOB] = str(value)
        return fn()
    finally:
        os.environ.pop(KNOB, None)
        if saved is not None:
            os.environ[KNOB] = saved


def _scene(gpu_host, desc, form):
    """The scene uploaded with the knob at `form` (None: unset), or None if the library holds no such form (rt_scene_create refuses it by name)."""
    def make():
        h = gpu_host.HostScene(desc)
        try:
            h.upload(0)
        except gpu_host.BackendError as e:
            assert "not built" in str(e) and form not in (None, 0), e
            return None
        return h
    return _with_knob(form, make)


@pytest.fixture(scope="module")
def built_forms(gpu_host):
    d = cornell_box(8, 8, 1)
    forms = [f for f in (1, 2) if _scene(gpu_host, d, f) is not None]      # (form 2 was measured and not kept: a library that holds it again is tested on it)
    default = _scene(gpu_host, d, None).scene_query(gpu_host.RT_QUERY_LDS_SPEC)
    assert 1 in forms and (default == 0 or default in forms)
    assert _scene(gpu_host, d, 7) is None                                   # a form that is not built is refused by name, never replaced
    return forms, default


@pytest.mark.parametrize("name", list(SCENES))
def test_hit_records_are_the_as_built_walks_bit_for_bit(gpu_host, built_forms, name):
    make, lo, hi = SCENES[name]
    desc = make()
    rays = _rays(desc, lo, hi, N_RAYS, seed=23)
    h0 = _scene(gpu_host, desc, 0)
    assert h0.lds_resident() and h0.scene_query(gpu_host.RT_QUERY_LDS_SPEC) == 0
    counts = (1, 63, 65, N_RAYS)
    # (ray 0 has a zero component, k % 11: the single ray starts one past it, the short batches at a wave without special rays)
    batches = {n: rays[1:2] if n == 1 else rays[64:64 + n] if n < N_RAYS else rays for n in counts}
    want = {n: h0.trace(batches[n], count=False) for n in counts}
    assert (want[N_RAYS]["prim"] >= 0).mean() > 0.02
    for form in built_forms[0]:
        h = _scene(gpu_host, desc, form)
        assert h.scene_query(gpu_host.RT_QUERY_LDS_SPEC) == form
        for n in counts:
            got = h.trace(batches[n], count=False)
            assert np.array_equal(want[n]["prim"], got["prim"]), (form, n)
            for f in ("t", "b0", "b1"):
                assert np.array_equal(bits(want[n][f]), bits(got[f])), (form, n, f)


def test_frame_and_counting_frame_do_not_notice_the_form(gpu_host, built_forms):
    desc = cornell_box(64, 64, 16)
    ints = [n for n, t in gpu_host.Stats._fields_ if t is ctypes.c_uint64]
    film0, st0 = _scene(gpu_host, desc, 0).render()
    _, cnt0 = _scene(gpu_host, desc, 0).render(count_traversal=True)
    assert cnt0["nodes_closest"] > 0 and cnt0["tris_closest"] > 0
    for form in [None] + built_forms[0]:            # the default (knob unset) and every built form
        h = _scene(gpu_host, desc, form)
        assert h.scene_query(gpu_host.RT_QUERY_LDS_SPEC) == (built_forms[1] if form is None else form)
        film, st = h.render()
        assert np.array_equal(bits(film0), bits(film)), form
        for k in ints:
            assert st0[k] == st[k], (form, k, st0[k], st[k])
        _, cnt = h.render(count_traversal=True)
        for k in ("nodes_closest", "tris_closest", "nodes_shadow", "tris_shadow"):
            if k in cnt0:
                assert cnt0[k] == cnt[k], (form, k)


def test_a_general_scene_keeps_the_as_built_walk(gpu_host, built_forms):
    """Quadrics and masks (the GENERAL kernels) are not given the form: the knob does not reach them."""
    from test_gpu_sphere import _sphere_zoo
    for form in built_forms[0]:
        h = _scene(gpu_host, _sphere_zoo(8, 1), form)
        assert h.lds_resident() and h.scene_query(gpu_host.RT_QUERY_LDS_SPEC) == 0
