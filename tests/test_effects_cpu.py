"""The seven effects after Fog and Toon, host side: the numpy restatement (tests/effects_restated.py)
against fixture F10 (tests/golden/f10_effects.npz, tests/golden/make_effects_golden.py: the
reference's own methods run on synthetic frames), the restated percentile against numpy, and the
library's new entry points without a GPU.

Where F10 records no cv2 stand-in for a case (Vignette, Cross Processing, Film Grain, Hologram
without depth) the fixture is the reference's own arithmetic and the restatement equals it; for
the other cases the equality pins the numpy glue around the restated cv2 calls.  Bit for bit.
"""
import json
import os

import numpy as np
import pytest

import effects_restated as R
from nerfmi import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F10 = os.path.join(GOLDEN, "f10_effects.npz")
NEW_EFFECTS = ["Vignette", "Cross Processing", "Film Grain", "Hologram", "Posterize", "Bloom", "Pencil Sketch"]
NEW_SYMBOLS = ["nerf_effect_vignette", "nerf_effect_cross_processing", "nerf_effect_film_grain",
               "nerf_effect_posterize", "nerf_effect_bloom", "nerf_effect_pencil_sketch", "nerf_effect_hologram",
               "nerf_gaussian_blur", "nerf_depth_percentile"]


def f10_cases():
    z = np.load(F10)
    return json.loads(str(z["cases"]))


def f10_case(case):
    """(image, depth or None, expected output) of one F10 case."""
    z = np.load(F10)
    depth = None
    if case["depth"] == "depth_chan":            # derived, not stored (make_effects_golden.py depth_chan)
        raw = z["depth_raw"]
        depth = np.stack([raw, raw * 2, raw * 0.5], -1).astype(np.float32)
    elif case["depth"] is not None:
        depth = z[case["depth"]]
    return z["img"], depth, z[case["name"] + "_out"]


def percentile_planes():
    """The planes the percentile is checked on: 1x11 (an integer index at q = 70 and 50), a
    constant, heavy ties, and the F9 depth."""
    g = np.random.default_rng(3)
    return {"1x11": g.random((1, 11), dtype=np.float32),
            "constant": np.full((9, 13), 0.3, np.float32),
            "ties": (g.integers(0, 4, (40, 50)) / 4).astype(np.float32),
            "f9": np.load(os.path.join(GOLDEN, "f9_fog.npz"))["norm_depth"]}


def test_f10_covers_the_cases():
    cases = f10_cases()
    assert os.path.getsize(F10) < 200_000
    by_effect = {e: [c for c in cases if c["effect"] == e] for e in NEW_EFFECTS}
    for e, cs in by_effect.items():
        assert {c["depth"] for c in cs} >= {None, "depth_norm"}, e
    assert any(c["depth"] == "depth_raw" for c in by_effect["Hologram"])
    assert {c["params"].get("bloom_size", 15) for c in by_effect["Bloom"]} >= {15, 14, 3, 51}
    assert {c["params"].get("sketch_strength", 1.0) for c in by_effect["Pencil Sketch"]} >= {1.0, 0.4}
    assert {c["params"].get("posterize_levels", 4) for c in by_effect["Posterize"]} >= {4, 7}
    assert {c["params"].get("vignette_strength", 0.5) for c in by_effect["Vignette"]} >= {0.5, 1.0}
    # the numpy-only effects ran none of the cv2 stand-ins: those outputs are the reference's own
    for c in cases:
        if c["effect"] in ("Vignette", "Cross Processing", "Film Grain") or (c["effect"] == "Hologram"
                                                                             and c["depth"] is None):
            assert c["called"] == [], c


@pytest.mark.parametrize("case", f10_cases(), ids=lambda c: c["name"])
def test_restatement_matches_f10(case):
    img, depth, ref = f10_case(case)
    np.random.seed(case["seed"])
    got = R.apply(case["effect"], img, depth, case["params"])
    assert got.dtype == np.uint8 and np.array_equal(got, ref)


@pytest.mark.parametrize("name", ["1x11", "constant", "ties", "f9"])
@pytest.mark.parametrize("q", [70, 50, 0, 100, 33.3])
def test_restated_percentile_is_numpys(name, q):
    x = percentile_planes()[name]
    got, ref = R.percentile(x, q), np.percentile(x, q)
    assert type(ref) is np.float32 and got == ref


def test_restated_blur_properties():
    """Repeated reflection, the fixed tables, and a constant image staying constant."""
    assert list(R.reflect101(np.arange(-7, 9), 3)) == [1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0]
    assert list(R.reflect101(np.arange(-2, 3), 1)) == [0] * 5
    assert np.array_equal(R.gaussian_kernel(5), np.array([.0625, .25, .375, .25, .0625], np.float32))
    for k in (9, 21, 51, 63):
        w = R.gaussian_kernel(k)
        assert w.dtype == np.float32 and len(w) == k and abs(float(w.astype(np.float64).sum()) - 1) < 1e-6
        assert np.array_equal(w, w[::-1])
    img = np.full((5, 7, 3), 200, np.uint8)
    assert np.array_equal(R.gaussian_blur_u8(img, 51), img)          # narrower than the radius
    one = np.zeros((9, 9), np.uint8)
    one[4, 4] = 255
    assert np.array_equal(R.gaussian_blur_u8(one, 1), one)
    assert R.gaussian_blur_u8(one, 3)[4, 4] == 64                    # 255 / 4 = 63.75 -> 64


@pytest.mark.parametrize("H,lines", [(100, 50), (5, 50), (37, 50), (48, 7), (3, 1)])
def test_hologram_rows_count_the_covering_lines(H, lines):
    """Row y is darkened once per line whose [int(i lh), int(min((i + 0.7) lh, H))) span holds it
    (a per-row count here, slices in the restatement)."""
    f = R.hologram_rows(H, lines)
    assert f.dtype == np.float32 and f.shape == (H,)
    lh = H / lines
    for y in range(H):
        exp = np.float32(1)
        for i in range(lines):
            if int(i * lh) <= y < int(min((i + 0.7) * lh, H)):
                exp = exp * np.float32(0.85)
        assert f[y] == exp
    if (H, lines) == (100, 50):
        assert set(np.unique(f)) == {np.float32(0.85), np.float32(1.0)}


def test_library_exports_the_new_symbols():
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert s in _lib.EXPORTED and hasattr(lib, s), s


def test_new_entry_points_reject_null_pointers():
    """Status 1 with the entry point's name in nerf_last_error(), before any launch (no GPU)."""
    lib = _lib.load()
    calls = {
        "nerf_effect_vignette": lambda: lib.nerf_effect_vignette(None, 8, 8, 0.5, None, None),
        "nerf_effect_cross_processing": lambda: lib.nerf_effect_cross_processing(None, 8, 8, None, None),
        "nerf_effect_film_grain": lambda: lib.nerf_effect_film_grain(None, None, 8, 8, 0.2, None, None),
        "nerf_effect_posterize": lambda: lib.nerf_effect_posterize(None, 8, 8, 4.0, None, None),
        "nerf_effect_bloom": lambda: lib.nerf_effect_bloom(None, 8, 8, 15, 0.3, None, None, 0, None),
        "nerf_effect_pencil_sketch": lambda: lib.nerf_effect_pencil_sketch(None, None, 8, 8, 1.0, None, None, 0, None),
        "nerf_effect_hologram": lambda: lib.nerf_effect_hologram(None, None, 1, 8, 8, 50, None, 0, 2, 0, 2, 0, 2, None,
                                                                 None, None, 0, None),
        "nerf_gaussian_blur": lambda: lib.nerf_gaussian_blur(None, 8, 8, 3, 5, None, None, 0, None),
        "nerf_depth_percentile": lambda: lib.nerf_depth_percentile(None, 64, 1, 70.0, None, None, 0, None),
    }
    assert sorted(calls) == sorted(NEW_SYMBOLS)
    for name, call in calls.items():
        assert call() == 1, name
        assert name.encode() in lib.nerf_last_error(), (name, lib.nerf_last_error())


def test_new_entry_points_reject_bad_sizes():
    lib = _lib.load()
    assert lib.nerf_gaussian_blur(None, 8, 8, 3, 65, None, None, 0, None) == 1 and b"k=65" in lib.nerf_last_error()
    assert lib.nerf_gaussian_blur(None, 8, 8, 3, 4, None, None, 0, None) == 1
    assert lib.nerf_gaussian_blur(None, 8, 8, 2, 5, None, None, 0, None) == 1
    assert lib.nerf_effect_bloom(None, 8, 8, 64, 0.3, None, None, 0, None) == 1 and b"64" in lib.nerf_last_error()
    assert lib.nerf_effect_hologram(None, None, 1, 8, 8, 0, None, 0, 2, 0, 2, 0, 2, None, None, None, 0, None) == 1
    assert b"lines=0" in lib.nerf_last_error()
    assert lib.nerf_depth_percentile(None, 64, 1, 101.0, None, None, 0, None) == 1
    assert lib.nerf_effect_posterize(None, 8, 8, 0.0, None, None) == 1 and b"levels" in lib.nerf_last_error()
    assert lib.nerf_effect_workspace_bytes(800, 800) >= 256 + 3 * 800 * 800 * 4 + 4096 + 800 * 4
