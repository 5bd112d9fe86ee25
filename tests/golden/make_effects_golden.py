"""Generate tests/golden/f10_effects.npz: the reference's own Vignette, Cross Processing, Film Grain,
Hologram, Posterize, Bloom and Pencil Sketch on synthetic frames.

Runs ONLY in the build container, where the reference is mounted read-only at /root/reference.
src/post_processor.py imports cv2 and tkinter at module level (post_processor.py:2-4), neither of
which is installed, so the module cannot be imported.  Like make_post_golden.py for Fog, this
script parses the module with `ast`, compiles each of the seven methods by itself and calls it on
a stand-in `self` that carries the reference's default parameter table (post_processor.py:33-55,
read from the same parse).  The namespace holds numpy and, under the name cv2, the stand-in of
tests/effects_restated.py (Cv2StandIn: cvtColor, Laplacian, Sobel, GaussianBlur, addWeighted,
divide restated in numpy).  Each case records which stand-ins its run called: none for Vignette,
Cross Processing, Film Grain and Hologram without depth, whose outputs are therefore the
reference's own arithmetic; for the others the fixture pins the reference's numpy glue around the
restated cv2 calls.  What gets committed is data: the inputs and the outputs, never reference code.

    python tests/golden/make_effects_golden.py      # rewrites tests/golden/f10_effects.npz

Layout: `img` (48,64,3) uint8; `depth_norm` (run.py:248's normalisation), `depth_raw` (max > 1;
the 3-channel `depth_chan` is derived from it by depth_chan() below and not stored, to keep the
file under 200 KB); `cases`: JSON list of {name, effect, depth (null or a key), params (overrides
of the defaults), seed, called}; `<name>_out` per case.  Random effects store the seed given to
np.random.seed before the call, not the draws (legacy streams are stable).
"""
import ast
import contextlib
import io
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
REF_FILE = "/root/reference/src/post_processor.py"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from oracle import post_oracle as P     # noqa: E402
import effects_restated as R            # noqa: E402

METHODS = {"Vignette": "_effect_vignette", "Cross Processing": "_effect_cross_processing",
           "Film Grain": "_effect_film_grain", "Hologram": "_effect_hologram", "Posterize": "_effect_posterize",
           "Bloom": "_effect_bloom", "Pencil Sketch": "_effect_sketch"}


def reference_methods_and_params(cv2):
    tree = ast.parse(open(REF_FILE).read(), REF_FILE)
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "PostProcessor")
    defs = {n.name: n for n in cls.body if isinstance(n, ast.FunctionDef)}
    params = None
    for node in ast.walk(defs["__init__"]):
        if (isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Attribute)
                and node.targets[0].attr == "params"):
            params = ast.literal_eval(node.value)
    fns = {}
    for effect, name in METHODS.items():
        ns = {"np": np, "cv2": cv2}
        exec(compile(ast.Module(body=[defs[name]], type_ignores=[]), REF_FILE, "exec"), ns)
        fns[effect] = ns[name]
    return fns, params


class _Self:
    def __init__(self, params):
        self.params = params


def frame(H, W, seed):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.stack([(xx / W) * 255, (yy / H) * 255, 128 + 100 * np.sin(xx / 7 + yy / 11)], -1)
    img = np.clip(img + g.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
    img.reshape(-1, 3)[:256, 0] = np.arange(256, dtype=np.uint8)          # every byte value
    depth = (2.5 + 1.5 * g.random((H, W))).astype(np.float32)
    depth[H // 4: 3 * H // 4, W // 3: 2 * W // 3] = 2.2
    return img, depth


def depth_chan(depth_raw):
    """The 3-channel depth of the `depth_chan` cases (not stored: the test derives it the same way)."""
    return np.stack([depth_raw, depth_raw * 2, depth_raw * 0.5], -1).astype(np.float32)


CASES = [(f"{e.lower().replace(' ', '_')}_{d}", e, None if d == "none" else "depth_norm", {})
         for e in METHODS for d in ("none", "norm")] + [
    ("hologram_raw", "Hologram", "depth_raw", {}),
    ("hologram_chan", "Hologram", "depth_chan", {}),
    ("bloom_14", "Bloom", None, {"bloom_size": 14}),
    ("bloom_3", "Bloom", None, {"bloom_size": 3}),
    ("bloom_51", "Bloom", None, {"bloom_size": 51}),
    ("pencil_sketch_04", "Pencil Sketch", "depth_norm", {"sketch_strength": 0.4}),
    ("pencil_sketch_raw", "Pencil Sketch", "depth_raw", {}),
    ("posterize_7", "Posterize", None, {"posterize_levels": 7}),
    ("vignette_10", "Vignette", None, {"vignette_strength": 1.0}),
]


def main():
    cv2 = R.Cv2StandIn()
    fns, defaults = reference_methods_and_params(cv2)
    img, depth = frame(48, 64, 10)
    out = {"img": img, "depth_norm": P.depth_normalize(depth), "depth_raw": depth}
    derived = {"depth_chan": depth_chan(depth)}
    meta = []
    for seed, (name, effect, dkey, over) in enumerate(CASES, start=100):
        cv2.called = []
        np.random.seed(seed)
        with contextlib.redirect_stdout(io.StringIO()) as said:
            ref = fns[effect](_Self(dict(defaults, **over)), img.copy(), None if dkey is None else {**out, **derived}[dkey].copy())
        assert not said.getvalue(), said.getvalue()          # Hologram prints when its depth branch raised
        assert ref.dtype == np.uint8 and ref.shape == img.shape
        out[f"{name}_out"] = ref
        meta.append({"name": name, "effect": effect, "depth": dkey, "params": over, "seed": seed,
                     "called": sorted(set(cv2.called))})
    out["cases"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "f10_effects.npz")
    np.savez_compressed(path, **out)
    print(f"wrote f10_effects.npz: {len(meta)} cases, {os.path.getsize(path)} bytes")
    for m in meta:
        print(f"  {m['name']:22s} stand-ins: {', '.join(m['called']) or 'none'}")


if __name__ == "__main__":
    main()
