"""Image maps on the CPU: the oracle's and the host's MIP pyramids and the oracle's image-texture probe against tests/mipmap_model.py, a float64 model written
from the reference's source (not from the oracle), at the shapes of mipmap_model.SHAPES under every wrap and filter; and the properties that keep the model
from being a third copy. The envelopes measured here (mipmap_model.ENVELOPE_K, PYRAMID_ENVELOPE; MEASUREMENTS.md) are what tests/test_gpu_mipmap.py holds the
device to."""
import numpy as np
import pytest

import mipmap_model as M


def _base():
    from rustracer_amd.scenes import cornell_box
    return cornell_box(16, 16, 1)


def _probe(o, tex, q):
    return np.stack([o.tex_probe(tex, q["uv"][i], (0.0, 0.0, 0.0), q["duv"][i]) for i in range(q["uv"].shape[0])])


@pytest.fixture(scope="module")
def world(orc, host):
    d = _base()
    cases = M.add_cases(d)
    return dict(cases=cases, o=orc.OracleScene(d), h=host.HostScene(d))


def test_pyramids_of_oracle_and_host_match_the_model(world):
    assert 4.0 * M.PYRAMID_ENVELOPE < M.PYRAMID_CEILING  # beyond 8 single-precision taps with sinf weights something other than rounding is wrong
    worst = 0.0
    for c in world["cases"]:
        if c["filter"] != "trilinear":  # the pyramid does not depend on the filter
            continue
        m = M.model_of(c)
        top = max(float(L.max()) for L in m.levels)
        for who in ("o", "h"):
            lv = world[who].mip_levels(c["mip"])
            assert [a.shape for a in lv] == [a.shape for a in m.levels], (c["name"], who)
            err = max(float(np.abs(a - b).max()) for a, b in zip(lv, m.levels)) / top
            worst = max(worst, err)
            assert err <= 4.0 * M.PYRAMID_ENVELOPE, (c["name"], who, err)
    print(f"pyramids: largest |texel - model| / max texel {worst:.3e} (PYRAMID_ENVELOPE {M.PYRAMID_ENVELOPE:.1e})")


@pytest.mark.parametrize("wrap_name", [w for w, _ in M.WRAPS])
def test_lookups_oracle_against_the_model(world, wrap_name):
    worst = 0.0
    for c in world["cases"]:
        if c["wrap_name"] != wrap_name:
            continue
        q, kind = M.queries(*c["shape"], c["seed"])
        j = M.judge(M.model_of(c), c, q, _probe(world["o"], c["tex"], q))
        k = float(j["ratio"].max())
        worst = max(worst, k)
        print(f"{c['name']:24s} n={len(kind):3d} envelope {k:6.3f} unit  widened {100 * j['share']:5.1f} %  largest footprint {max(i.get('taps', 0) for i in j['infos'])} taps")
        assert k <= 4.0 * M.ENVELOPE_K, (c["name"], k, kind[int(j["ratio"].argmax())])
        assert j["share"] <= 0.10, (c["name"], j["share"])      # the caps on widened allowances: a tenth of the queries at the most ...
        assert not j["over"], (c["name"], j["over"])            # ... and none beyond one table step of its level's range
    print(f"{wrap_name}: largest (|oracle - model| - widened) / unit {worst:.3f} (ENVELOPE_K {M.ENVELOPE_K})")


def test_far_coordinates_oracle_against_the_model(world):
    """st * size from 2^31 to 2^40: float32 coordinates are far coarser than a texel there, so what the model can judge is that the result is finite and a
    convex combination of the texels a lookup can read - which a 32-bit saturated texel index is not (triangle returns texels scaled by 1e9, EWA finds no tap)."""
    for c in world["cases"]:
        if c["shape"] not in ((1, 1), (5, 3), (64, 4), (16, 16)):
            continue
        q = M.far_queries(*c["shape"], c["seed"])
        m = M.model_of(c)
        got = _probe(world["o"], c["tex"], q)
        j = M.judge(m, c, q, got)
        tol = np.minimum(4.0 * M.ENVELOPE_K * j["unit"] + j["wid"], m.rng[0] + 8.0 * M.E * m.mx[0])
        err = np.abs(got.astype(np.float64) - j["val"])
        assert np.isfinite(got).all(), (c["name"], q["uv"][~np.isfinite(got).all(axis=1)][:3])
        assert (err <= tol).all(), (c["name"], float((err - tol).max()))


# ---------------------------------------------------------------- the model's own properties
def test_model_constant_image_gives_the_constant():
    col = np.float32([0.25, 0.5, 0.75])
    for w, h in ((1, 1), (4, 2), (5, 3), (2, 8)):
        for _, wrap in (M.WRAPS[0], M.WRAPS[2]):
            for _, tri, an in M.FILTERS:
                m = M.MipModel(np.broadcast_to(col, (h, w, 3)), tri, an, wrap)
                q, _ = M.queries(w, h, 5, n_a=24, n_b=2)
                val = M.evaluate(m, M.MAPPINGS[1], q)[0]
                assert np.abs(val - col).max() <= 1e-12, (w, h, wrap, tri, an)


def test_model_black_outside_the_border_is_zero():
    rng = np.random.default_rng(2)
    for w, h in ((1, 1), (2, 8), (5, 3), (16, 16)):
        for _, tri, an in M.FILTERS:
            m = M.MipModel(M.image(w, h), tri, an, M.WRAP_BLACK)
            q = M.outside_queries(rng, 40)
            assert np.array_equal(M.evaluate(m, M.MAPPINGS[0], q)[0], np.zeros((40, 3))), (w, h, tri, an)


def test_model_repeat_is_periodic_under_integer_shifts():
    rng = np.random.default_rng(3)
    for w, h in ((1, 2), (8, 2), (5, 3), (4, 64)):
        for _, tri, an in M.FILTERS:
            m = M.MipModel(M.image(w, h), tri, an, M.WRAP_REPEAT)
            q, shifted = M.periodic_queries(rng, 40)
            assert np.abs(M.evaluate(m, M.MAPPINGS[0], q)[0] - M.evaluate(m, M.MAPPINGS[0], shifted)[0]).max() <= 1e-13, (w, h, tri, an)


def test_model_in_single_precision_stays_inside_its_own_allowance():
    """the diagnostic mode, exercised so that it keeps working; nothing about the code under test rests on it"""
    c = dict(img=M.image(8, 2), trilinear=False, aniso=8.0, wrap=M.WRAP_REPEAT, mapping=M.MAPPINGS[0])
    q, _ = M.queries(8, 2, 9, n_a=24, n_b=2)
    single = M.evaluate(M.model_of(c, np.float32), c["mapping"], q)[0]
    assert M.judge(M.model_of(c), c, q, single)["ratio"].max() <= 4.0
