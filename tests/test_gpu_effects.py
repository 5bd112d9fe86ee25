"""The seven effects after Fog and Toon on the GPU (csrc/effects.hip through nerfmi.PostProcessor):
Vignette, Cross Processing, Film Grain, Hologram, Posterize, Bloom, Pencil Sketch.

Against fixture F10 (the reference's own methods, tests/golden/make_effects_golden.py) and against
the numpy restatement (tests/effects_restated.py) at sizes that leave the tiles ragged (37x53),
that are smaller than the 21- and 51-tap radii (5x7: repeated reflection) and at
test_post_effects.py's 96x120 scene.  Tolerance: none.  Every step is an IEEE operation in the
reference's order and dtype on both sides (float64 where numpy 2 promotes to it), the blur's
coefficients come from the same double formula, and the percentile is an exact selection.
"""
import functools

import numpy as np
import pytest
import torch

import effects_restated as R
from oracle import post_oracle as P
from test_effects_cpu import NEW_EFFECTS, f10_case, f10_cases, percentile_planes
from test_post_effects import scene

pytestmark = pytest.mark.gpu

SHAPES = [(37, 53), (5, 7), (96, 120)]
DEPTH_AWARE = ("Hologram", "Pencil Sketch")


def processor(effect, params=None, rng=None):
    import nerfmi
    pp = nerfmi.PostProcessor()
    pp.current_effect = effect
    pp.params.update(params or {})
    pp.rng = rng
    return pp


@functools.lru_cache(maxsize=None)
def frame(shape):
    return scene(H=shape[0], W=shape[1], seed=shape[0])          # shared: the tests leave it unchanged


def depth_of(shape, kind):
    _, depth = frame(shape)
    return {"none": None, "norm": P.depth_normalize(depth), "raw": depth,
            "chan": np.stack([depth, depth * 3, depth * 0.5], -1).astype(np.float32)}[kind]


@functools.lru_cache(maxsize=None)
def restated(effect, shape, kind, params=()):
    np.random.seed(shape[0] + 1)
    return R.apply(effect, frame(shape)[0], depth_of(shape, kind), dict(params))


@pytest.mark.parametrize("case", f10_cases(), ids=lambda c: c["name"])
def test_effect_matches_reference_f10(case):
    img, depth, ref = f10_case(case)
    np.random.seed(case["seed"])
    got = processor(case["effect"], case["params"]).apply_effect(img, depth)
    assert got.dtype == np.uint8 and np.array_equal(got, ref), int((got != ref).sum())


CASES = [(e, k, ()) for e in NEW_EFFECTS for k in (("none", "norm", "raw") if e in DEPTH_AWARE else ("none",))] + [
    ("Hologram", "chan", ()),
    ("Hologram", "norm", (("hologram_lines", 7),)),
    ("Bloom", "none", (("bloom_size", 51),)),
    ("Bloom", "none", (("bloom_size", 8), ("bloom_strength", 0.85))),
    ("Pencil Sketch", "norm", (("sketch_strength", 0.4),)),
    ("Posterize", "none", (("posterize_levels", 7.5),)),
    ("Vignette", "none", (("vignette_strength", 1.0),)),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("effect,kind,params", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_effect_matches_restatement(effect, kind, params, shape):
    exp = restated(effect, shape, kind, params)
    np.random.seed(shape[0] + 1)
    got = processor(effect, dict(params)).apply_effect(frame(shape)[0], depth_of(shape, kind))
    assert np.array_equal(got, exp), (int((got != exp).sum()), int(np.abs(got.astype(int) - exp).max()))


@pytest.mark.parametrize("shape", [(37, 53), (5, 7), (40, 300)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("channels", [1, 3])
def test_blur_matches_restatement(shape, channels):
    """Every coefficient path (the fixed tables, the formula, the largest size), more than one tile
    in both passes (40x300: two row tiles of 256 pixels, two column tiles of 32 rows)."""
    from nerfmi.post_processor import gaussian_blur
    g = np.random.default_rng(shape[1])
    img = g.integers(0, 256, shape + (3,), dtype=np.uint8)
    img[: shape[0] // 2, : shape[1] // 2] = 255                      # saturated block: .5 ties at its edge
    if channels == 1:
        img = np.ascontiguousarray(img[:, :, 0])
    for k in (1, 3, 5, 7, 9, 21, 51, 63):
        got = gaussian_blur(img, k)
        exp = R.gaussian_blur_u8(img, k)
        assert got.shape == img.shape and np.array_equal(got, exp), (k, int((got != exp).sum()))
    with pytest.raises(ValueError):
        gaussian_blur(img, 65)
    with pytest.raises(ValueError):
        gaussian_blur(img, 4)


@pytest.mark.parametrize("name", ["1x11", "constant", "ties", "f9", "large"])
def test_depth_percentile_is_numpys(name):
    from nerfmi.post_processor import depth_percentile
    if name == "large":      # more values than one pass of the grid covers, negative ones included
        x = np.random.default_rng(5).normal(0, 3, (600, 500)).astype(np.float32)
    else:
        x = percentile_planes()[name]
    for q in (70, 50, 0, 100):
        got = depth_percentile(x, q)
        assert type(got) is np.float32 and got == np.percentile(x, q), (q, got, np.percentile(x, q))
    t = depth_percentile(torch.from_numpy(x).cuda(), 70)
    assert t.is_cuda and t.dim() == 0 and t.item() == np.percentile(x, 70)
    with pytest.raises(ValueError):
        depth_percentile(x, 101)


@pytest.mark.parametrize("effect", NEW_EFFECTS)
def test_device_tensor_in_device_tensor_out(effect):
    img, depth = frame((37, 53))
    d = P.depth_normalize(depth)
    np.random.seed(11)
    host = processor(effect).apply_effect(img, d)
    np.random.seed(11)
    dev = processor(effect).apply_effect(torch.from_numpy(img.copy()).cuda(), torch.from_numpy(d).cuda())
    assert isinstance(host, np.ndarray) and dev.is_cuda and dev.dtype == torch.uint8
    assert np.array_equal(dev.cpu().numpy(), host)


@pytest.mark.parametrize("effect", ["Film Grain", "Hologram"])
def test_rng_object_equals_the_global_seed_path(effect):
    img, depth = frame((37, 53))
    np.random.seed(7)
    a = processor(effect).apply_effect(img, depth)
    np.random.seed(99)                                   # the global stream is not what is drawn from
    b = processor(effect, rng=np.random.RandomState(7)).apply_effect(img, depth)
    assert np.array_equal(a, b)
    c = processor(effect, rng=np.random.RandomState(8)).apply_effect(img, depth)
    assert not np.array_equal(a, c)


@pytest.mark.parametrize("effect", ["Film Grain", "Hologram"])
def test_device_generator_is_reproducible_and_different(effect):
    img, depth = frame((37, 53))
    dimg, ddepth = torch.from_numpy(img.copy()).cuda(), torch.from_numpy(depth.copy()).cuda()

    def run(seed):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        out = processor(effect, rng=g).apply_effect(dimg, ddepth)
        assert out.is_cuda
        return out.cpu().numpy()

    a, b, c = run(3), run(3), run(4)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    np.random.seed(3)
    assert not np.array_equal(a, processor(effect).apply_effect(img, depth))       # not numpy's stream


def test_explicit_noise_and_spans():
    """Noise and spans handed in take the place of the draws (and leave the generator alone)."""
    img, depth = frame((37, 53))
    st = np.random.RandomState(5)
    noise = st.normal(0, 0.03, img.shape).astype(np.float32)
    spans = [(int(st.randint(0, 53)), int(st.randint(2, 6))) for _ in range(3)]
    pp = processor("Hologram")
    got = pp._effect_hologram(img, depth, noise=noise, spans=spans)
    assert np.array_equal(got, R.hologram(img, depth, 50, rng=np.random.RandomState(5)))
    grain = np.random.RandomState(6).normal(0, 50, img.shape).astype(np.float32)
    got = processor("Film Grain")._effect_film_grain(img, noise=torch.from_numpy(grain).cuda())
    assert np.array_equal(got, R.film_grain(img, None, 0.2, rng=np.random.RandomState(6)))


def test_new_effect_errors():
    img, depth = frame((37, 53))
    for effect in NEW_EFFECTS:
        with pytest.raises(ValueError):
            processor(effect).apply_effect(img[:, :, :2].copy(), None)
        with pytest.raises(ValueError):
            processor(effect).apply_effect(img.astype(np.float32), None)
    for effect in DEPTH_AWARE:
        with pytest.raises(ValueError):
            processor(effect).apply_effect(img, depth[:-1])
        with pytest.raises(ValueError):
            processor(effect).apply_effect(img, depth[0])
    with pytest.raises(ValueError):                      # the reference's Pencil Sketch takes (H,W) only
        processor("Pencil Sketch").apply_effect(img, depth_of((37, 53), "chan"))
    with pytest.raises(ValueError):
        processor("Bloom", {"bloom_size": 65}).apply_effect(img, None)
    processor("Bloom", {"bloom_size": 62}).apply_effect(img, None)             # 62 -> 63 taps, the largest
    with pytest.raises(ValueError):
        processor("Film Grain")._effect_film_grain(img, noise=np.zeros((37, 53), np.float32))
    with pytest.raises(ValueError):
        processor("Hologram")._effect_hologram(img, noise=np.zeros((36, 53, 3), np.float32))
    with pytest.raises(TypeError):
        processor("Hologram", {"hologram_lines": 50.0}).apply_effect(img, depth)


def test_ten_effects_and_the_four_left_out():
    import nerfmi
    from nerfmi.post_processor import REFERENCE_ONLY_EFFECTS
    pp = nerfmi.PostProcessor()
    assert sorted(pp.effects) == sorted(["Original", "Toon Shader", "Fog"] + NEW_EFFECTS)
    assert sorted(REFERENCE_ONLY_EFFECTS) == ["Color Boost", "Neon Glow", "Night Vision", "Sepia"]
    img, depth = frame((5, 7))
    for name in REFERENCE_ONLY_EFFECTS:
        pp.current_effect = name
        with pytest.raises(NotImplementedError):
            pp.apply_effect(img, depth)
