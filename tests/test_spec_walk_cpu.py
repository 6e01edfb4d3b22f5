"""The forms of the closest-hit link walk of an LDS-resident scene (closest_small_links<.., SPEC>, DESIGN 5.3 "leaf holders keep walking"), restated on the CPU over
HostScene.link_tables() - scripts/sim_lds_walk.py holds the state machines (one statement of them, shared with the model's table), the float64 slab test of
test_link_tables_cpu.py and a float64 triangle test. No device.

SPEC 1 (built: k_trace_spec<1>) and SPEC 2 / 3 (measured and not kept, MEASUREMENTS R9; the model keeps them) let a lane that holds a leaf go on testing nodes with the
t_max it has. What they must keep is the walk's RESULT: per ray the same primitive tests in the same
order, each under the same t_max, as SPEC 0 - and so the same hit."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ["cornell", "soup-126", "soup-40-degenerate"]
LEAF_MINS = (16, 24)      # the thresholds the kernel is measured at


@pytest.fixture(scope="module")
def sim(host):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import sim_lds_walk
    finally:
        sys.path.pop(0)
    return sim_lds_walk


@pytest.fixture(scope="module")
def cases(sim):
    """Per scene: the model and the waves - 1500 random rays in waves of 64 (the last one partial: 28 rays), then waves of 1 and of 63 rays - with SPEC 0's walk of
    each wave at each threshold, computed once."""
    out = {}
    for name in SCENES:
        m = sim.Model(sim.scene_desc(name))
        rng = np.random.default_rng(7)
        ext = m.hi[0] - m.lo[0]
        n = 1500 + 1 + 63
        org = rng.uniform(m.lo[0] - 0.3 * ext, m.hi[0] + 0.3 * ext, (n, 3))
        org[::3] = rng.uniform(m.lo[0], m.hi[0], (len(org[::3]), 3))          # a third of them start inside the scene, as path rays do
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        caps = rng.choice([np.inf, 0.5 * float(np.linalg.norm(ext)), 0.1 * float(np.linalg.norm(ext))], n).tolist()
        prep = m.prepare(org, d)
        cuts = list(range(0, 1500, 64)) + [1500, 1501, n]
        waves = [(prep[a:b], caps[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        assert [len(w[0]) for w in waves[-3:]] == [28, 1, 63]
        base = {lm: [sim.walk_wave(m, w, c, 0, lm) for w, c in waves] for lm in LEAF_MINS}
        out[name] = (m, waves, base)
    return out


@pytest.mark.parametrize("spec", [1, 2, 3])
@pytest.mark.parametrize("name", SCENES)
def test_speculative_walks_test_the_same_primitives_under_the_same_t_max(sim, cases, name, spec):
    m, waves, base = cases[name]
    tested = 0
    for lm in LEAF_MINS:
        for (w, caps), (res0, _) in zip(waves, base[lm]):
            res, st = sim.walk_wave(m, w, caps, spec, lm)
            for r, r0 in zip(res, res0):
                assert r[2] == r0[2]                       # (leaf slot, t_max at its test), in order
                assert r[:2] == r0[:2]                     # the hit
                tested += len(r[2])
            # every node round advances or stalls a lane, every leaf phase tests a primitive: the walk ends, and well inside this bound
            assert st["node_rounds"] + st["leaf_phases"] <= m.n_nodes * 64 + m.n_prims
    assert tested > 1000       # (primitive tests compared: the comparison is not vacuous)


@pytest.mark.parametrize("name", SCENES)
def test_every_form_finds_the_brute_force_closest_primitive(sim, cases, name):
    m, waves, base = cases[name]
    hits = 0
    for spec in (0, 1, 2, 3):
        for (w, caps), (res0, _) in zip(waves, base[16]):
            res = res0 if spec == 0 else sim.walk_wave(m, w, caps, spec, 16)[0]
            for prep, cap, r in zip(w, caps, res):
                p, t = sim.brute_force(prep, cap)
                assert r[1] == t                           # the distance: exactly the smallest of all primitives' under the cap
                if p >= 0 and sorted(prep[2])[1] > t:      # ... and its primitive, where no second one lies at the same distance
                    assert r[0] == p
                assert (r[0] < 0) == (p < 0)
                hits += p >= 0
    assert hits > 300


def test_the_model_sees_what_the_forms_are_for(sim, cases):
    """On S1's tree the holders' own walk fills node rounds: fewer rounds per wave, more lanes in each, the same leaf phases' primitive tests."""
    m, waves, base = cases["cornell"]
    tot = {}
    for spec in (0, 1, 2, 3):
        sts = [st for _, st in base[16]] if spec == 0 else [sim.walk_wave(m, w, c, spec, 16)[1] for w, c in waves]
        tot[spec] = {k: sum(s[k] for s in sts) for k in sts[0]}
    assert tot[0]["tri_tests"] == tot[1]["tri_tests"] == tot[2]["tri_tests"]
    assert tot[2]["node_rounds"] < tot[1]["node_rounds"] < tot[0]["node_rounds"]
    lanes = {s: tot[s]["node_lanes"] / tot[s]["node_rounds"] for s in tot}
    assert lanes[2] > lanes[1] > lanes[0]
