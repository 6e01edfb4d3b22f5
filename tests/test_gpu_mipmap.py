"""Image maps on the GPU (rt_texture_eval, the evaluator the shade kernels call) at the shapes where the texel layout can go wrong - levels narrower than a
tile, non-square and resampled images, images behind oddly padded ones in the texel array - against the oracle's probe and against the float64 model of
tests/mipmap_model.py, plus checks that need neither (transposition, periodicity, constants, black borders) and the pyramids built on the device."""
import numpy as np
import pytest

import mipmap_model as M

pytestmark = pytest.mark.gpu


def _base():
    from rustracer_amd.scenes import cornell_box
    return cornell_box(16, 16, 1)


def _probe(o, tex, q):
    return np.stack([o.tex_probe(tex, q["uv"][i], (0.0, 0.0, 0.0), q["duv"][i]) for i in range(q["uv"].shape[0])])


def _image_gate(got, want):
    """the image gate of test_gpu_texture_graphs.py: <= 0 where it holds"""
    return np.abs(got.astype(np.float64) - want) - 1e-5 * np.abs(np.asarray(want, np.float64)) - 1e-7


TRANSPOSED = [(8, 2), (64, 4), (2, 1)]  # powers of two: a resampled image and its transpose differ by the zoom's own rounding
CONSTANT = np.float32([0.25, 0.5, 0.75])


@pytest.fixture(scope="module")
def world(gpu_host, orc):
    """one scene with every (shape, wrap, filter) of the model's cases - the 1 x 1, the 2 x 8 and the resampled 5 x 3 first - and the images of the metamorphic
    checks behind them"""
    d = _base()
    cases = M.add_cases(d)
    plain, pairs, consts = {}, [], []
    for c in cases:  # identity-mapped twins for the checks that need exact coordinates
        plain[c["name"]] = d.image_tex(c["mip"])
    for w, h in TRANSPOSED:
        img = M.image(w, h)
        for k, (_, wrap) in enumerate(M.WRAPS):
            _, tri, an = M.FILTERS[(k + w) % 4]
            a = d.image_tex(d.add_mip(img, trilinear=tri, max_aniso=an, wrap=wrap))
            b = d.image_tex(d.add_mip(np.ascontiguousarray(img.transpose(1, 0, 2)), trilinear=tri, max_aniso=an, wrap=wrap))
            pairs.append((f"{w}x{h} wrap {wrap} filter {(k + w) % 4}", (w, h), a, b))
    for w, h in ((8, 2), (5, 3), (1, 1)):
        for wrap in (M.WRAP_REPEAT, M.WRAP_CLAMP):
            for _, tri, an in M.FILTERS:
                consts.append((f"{w}x{h} wrap {wrap} aniso {an} trilinear {tri}", (w, h),
                               d.image_tex(d.add_mip(np.broadcast_to(CONSTANT, (h, w, 3)), trilinear=tri, max_aniso=an, wrap=wrap), 2.0, 0.5, 0.25, -0.5)))
    return dict(cases=cases, plain=plain, pairs=pairs, consts=consts, h=gpu_host.HostScene(d), o=orc.OracleScene(d))


def _eval(world, tex, q):
    return world["h"].texture_eval(tex, uv=q["uv"], duv=q["duv"])


@pytest.mark.parametrize("wrap_name", [w for w, _ in M.WRAPS])
def test_every_shape_and_filter_matches_the_oracle_probe_and_the_model(world, wrap_name):
    """Against the oracle: the existing image gate, not loosened. Against the model: what the CPU test asserts of the oracle (4 ENVELOPE_K units and the per-query
    allowance) plus that gate - a triangle inequality; nothing here is measured on the device."""
    equal = total = 0
    for c in world["cases"]:
        if c["wrap_name"] != wrap_name:
            continue
        q, kind = M.queries(*c["shape"], c["seed"])
        got, want = _eval(world, c["tex"], q), _probe(world["o"], c["tex"], q)
        j = M.judge(M.model_of(c), c, q, got)
        same = (got.view(np.uint32) == want.view(np.uint32)).all(axis=1)
        equal += int(same.sum()); total += len(same)
        err = _image_gate(got, want)
        print(f"{c['name']:24s} n={len(kind):3d} bit-unequal {100.0 * (1.0 - same.mean()):6.2f} %  gate {err.max():+.2e}  against the model {j['ratio'].max():6.3f} unit")
        assert np.isfinite(got).all(), c["name"]
        assert err.max() <= 0.0, (c["name"], float(err.max()), kind[int(err.max(axis=1).argmax())])
        excess = np.abs(got.astype(np.float64) - j["val"]) - j["wid"] - 4.0 * M.ENVELOPE_K * j["unit"] - 1e-5 * np.abs(j["val"]) - 1e-7
        assert excess.max() <= 0.0, (c["name"], float(excess.max()), kind[int(excess.max(axis=1).argmax())])
    print(f"{wrap_name}: bit-equal to the oracle {100.0 * equal / total:.2f} % of {total}")


def test_scaled_coordinates_match_the_oracle_probe(world):
    """the scaling of test_gpu_texture_graphs._records (coordinates x 1e3, a third of the records without differentials), against the oracle only: float32
    coordinates are coarse against a texel there, so the float64 model is no judge"""
    rng = np.random.default_rng(11)
    n = 300
    for k, c in enumerate(world["cases"]):
        if k % 12 != (k // 12) % 12:  # one (wrap, filter) per shape, a different one from shape to shape
            continue
        uv = rng.normal(0.0, 3.0, (n, 2))
        uv[::7] *= 1e3
        uv[::5] = -np.abs(uv[::5])
        duv = rng.normal(0.0, 1.0, (n, 4)) * 10.0 ** rng.uniform(-4, 0.5, (n, 1))
        duv[np.arange(n) % 3 == 0] = 0.0
        q = dict(uv=uv.astype(np.float32), duv=duv.astype(np.float32))
        got, want = _eval(world, c["tex"], q), _probe(world["o"], c["tex"], q)
        same = (got.view(np.uint32) == want.view(np.uint32)).all(axis=1)
        print(f"{c['name']:24s} bit-unequal {100.0 * (1.0 - same.mean()):6.2f} % of {n}")
        assert _image_gate(got, want).max() <= 0.0, c["name"]


def test_far_coordinates_match_the_oracle_and_stay_inside_the_texels(world):
    """st * size from 2^31 to 2^40 (mipmap_model.far_queries): the texel indices are 64-bit in the reference"""
    for c in world["cases"]:
        if c["shape"] not in ((1, 1), (5, 3), (64, 4), (16, 16)):
            continue
        q = M.far_queries(*c["shape"], c["seed"])
        m = M.model_of(c)
        got, want = _eval(world, c["tex"], q), _probe(world["o"], c["tex"], q)
        assert np.isfinite(got).all(), c["name"]
        assert _image_gate(got, want).max() <= 0.0, (c["name"], float(_image_gate(got, want).max()))
        j = M.judge(m, c, q, got)
        tol = np.minimum(4.0 * M.ENVELOPE_K * j["unit"] + j["wid"], m.rng[0] + 8.0 * M.E * m.mx[0]) + 1e-5 * np.abs(j["val"]) + 1e-7
        assert (np.abs(got.astype(np.float64) - j["val"]) <= tol).all(), c["name"]


# ---------------------------------------------------------------- checks that need neither oracle nor model
def test_a_transposed_image_gives_the_same_values_at_transposed_queries(world):
    for name, (w, h), a, b in world["pairs"]:
        q, _ = M.queries(w, h, 7 * w + h)
        t = dict(uv=np.ascontiguousarray(q["uv"][:, ::-1]), duv=np.ascontiguousarray(q["duv"][:, [1, 0, 3, 2]]))
        va, vb = _eval(world, a, q), _eval(world, b, t)
        err = _image_gate(vb, va)  # the taps are summed in another order: the image gate, not bit equality
        assert err.max() <= 0.0, (name, float(err.max()))
        assert va.max() > 0.0


def test_repeat_is_periodic_bit_for_bit_where_the_coordinates_are_exact(world):
    rng = np.random.default_rng(5)
    for c in world["cases"]:
        if c["wrap"] != M.WRAP_REPEAT:
            continue
        q, shifted = M.periodic_queries(rng, 64)
        a, b = _eval(world, world["plain"][c["name"]], q), _eval(world, world["plain"][c["name"]], shifted)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (c["name"], np.argwhere(a != b)[:4].ravel())


def test_a_constant_image_gives_the_constant(world):
    for name, (w, h), tex in world["consts"]:
        q, _ = M.queries(w, h, 3 * w + h, n_a=64, n_b=4)
        got = _eval(world, tex, q)
        assert _image_gate(got, np.broadcast_to(CONSTANT, got.shape)).max() <= 0.0, name


def test_black_outside_the_border_is_zero(world):
    rng = np.random.default_rng(6)
    for c in world["cases"]:
        if c["wrap"] != M.WRAP_BLACK:
            continue
        got = _eval(world, world["plain"][c["name"]], M.outside_queries(rng, 64))
        assert np.array_equal(got, np.zeros_like(got)), c["name"]


def test_pyramids_built_on_the_device_match_the_model(gpu_host):
    """test_gpu_ingest_build.py ties them to the host bit for bit; this ties them to something that is not the host"""
    d = _base()
    mips = []
    for w, h in M.SHAPES:
        if not ((w & (w - 1)) or (h & (h - 1))):
            continue
        for _, wrap in M.WRAPS:
            mips.append((w, h, wrap, d.add_mip(M.image(w, h), wrap=wrap)))
    s = gpu_host.HostScene(d, device_ingest=True)
    worst = 0.0
    for w, h, wrap, mip in mips:
        m = M.MipModel(M.image(w, h), wrap=wrap)
        lv = s.mip_levels(mip)
        assert [a.shape for a in lv] == [a.shape for a in m.levels], (w, h, wrap)
        err = max(float(np.abs(a - b).max()) for a, b in zip(lv, m.levels)) / max(float(L.max()) for L in m.levels)
        worst = max(worst, err)
        assert err <= 4.0 * M.PYRAMID_ENVELOPE, (w, h, wrap, err)
    print(f"device pyramids: largest |texel - model| / max texel {worst:.3e}")
