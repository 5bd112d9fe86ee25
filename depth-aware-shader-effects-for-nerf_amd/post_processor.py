"""Post effects on the GPU — the reference's PostProcessor (src/post_processor.py:8-57, :495-499),
SURVEY.md §8f row 4.

Same surface: ``PostProcessor()`` with ``effects`` (name -> callable), ``params`` (the reference's
defaults, post_processor.py:33-55), ``current_effect`` and ``apply_effect(image, depth=None)``.
The arithmetic runs in csrc/effects.hip through the C ABI (one nerf_effect_* entry point per
effect); there is no CPU path.

Effects here, ten of the reference's fourteen: "Original", "Toon Shader" (:64-117), "Fog"
(:451-493), "Vignette" (:161-186), "Cross Processing" (:271-298), "Film Grain" (:214-224),
"Hologram" (:373-449), "Posterize" (:300-318), "Bloom" (:146-159) and "Pencil Sketch" (:226-269).
Toon, Fog, Hologram and Pencil Sketch read the depth map.  The other four (REFERENCE_ONLY_EFFECTS)
need cv2 internals that are not restated here (8-bit HSV tables, equalizeHist, Canny, transform);
selecting one raises NotImplementedError naming it.

Randomness (Film Grain, Hologram) is drop-in by default: with ``rng = None`` the draws are the
reference's, from numpy's global generator in the reference's order (``np.random.normal``, then for
Hologram three times ``randint(0, W)`` and ``randint(2, 6)``), made on the host, cast to float32 and
uploaded, so under ``np.random.seed(s)`` the frame equals the reference's.  ``rng`` may be any
object with ``normal`` and ``randint`` (``np.random.RandomState(7)``), or a ``torch.Generator``: a
device generator draws with torch.randn / torch.randint on the GPU and nothing visits the host.

``image``: uint8 (H,W,3) RGB, a numpy array (as the reference takes) or a torch tensor on the GPU;
``depth``: float (H,W) (Fog and Hologram also take (H,W,C) and use channel 0, as :474-475 and
:412-413 do) or None.  The result has the image's kind: numpy in, numpy out; a device tensor in, a
device tensor out.
"""
import numpy as np
import torch

from . import _lib

REFERENCE_ONLY_EFFECTS = ("Color Boost", "Sepia", "Night Vision", "Neon Glow")
MAX_BLUR = 63      # largest Gaussian kernel size of the blur kernels (csrc/effects.hip kBlurMaxK)


def normalize_depth(depth):
    """run.py:248: (d - min) / (max - min + 1e-6), on the GPU; depth (H,W) float32 (numpy or torch)."""
    lib, dev = _lib.load(), _lib.device()
    as_numpy = isinstance(depth, np.ndarray)
    d = torch.as_tensor(np.ascontiguousarray(depth, np.float32) if as_numpy else depth).to(dev, torch.float32)
    d = d.contiguous()
    out = torch.empty_like(d)
    ws = torch.empty(256, dtype=torch.uint8, device=dev)
    _lib.check(lib.nerf_depth_normalize(_lib.ptr(d), d.numel(), _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                        _lib.stream()), "nerf_depth_normalize")
    return out.cpu().numpy() if as_numpy else out


def depth_percentile(depth, q):
    """np.percentile(depth, q) (method "linear") of a float32 array of any shape on the GPU, exact:
    nerf_depth_percentile's radix select and numpy's float32 interpolation.  A numpy array gives an
    np.float32, a tensor a 0-d device tensor (no device-to-host copy)."""
    lib, dev = _lib.load(), _lib.device()
    as_numpy = isinstance(depth, np.ndarray)
    d = torch.as_tensor(np.ascontiguousarray(depth, np.float32) if as_numpy else depth).to(dev, torch.float32)
    d = d.contiguous()
    if d.numel() == 0 or not 0 <= q <= 100:
        raise ValueError(f"depth_percentile: {d.numel()} values, q={q} (needs values and 0 <= q <= 100)")
    out = torch.empty((), dtype=torch.float32, device=dev)
    ws = torch.empty(4096, dtype=torch.uint8, device=dev)
    _lib.check(lib.nerf_depth_percentile(_lib.ptr(d), d.numel(), 1, float(q), _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                         _lib.stream()), "nerf_depth_percentile")
    return out.cpu().numpy()[()] if as_numpy else out


def gaussian_blur(image, k):
    """The effects' Gaussian blur by itself (nerf_gaussian_blur: cv2.GaussianBlur(image, (k, k), 0)
    restated in float32): uint8 (H,W) or (H,W,3), odd k in 1..63."""
    lib, dev = _lib.load(), _lib.device()
    as_numpy = isinstance(image, np.ndarray)
    img = torch.as_tensor(np.ascontiguousarray(image) if as_numpy else image)
    if img.dtype != torch.uint8 or img.dim() not in (2, 3) or (img.dim() == 3 and img.shape[2] not in (1, 3)):
        raise ValueError(f"gaussian_blur: image must be uint8 (H,W) or (H,W,3), got {tuple(img.shape)} {img.dtype}")
    if not isinstance(k, (int, np.integer)) or k % 2 == 0 or not 1 <= k <= MAX_BLUR:
        raise ValueError(f"gaussian_blur: k={k!r} must be an odd integer in 1..{MAX_BLUR}")
    img = img.to(dev).contiguous()
    H, W = img.shape[:2]
    out = torch.empty_like(img)
    ws = torch.empty(lib.nerf_effect_workspace_bytes(H, W), dtype=torch.uint8, device=dev)
    _lib.check(lib.nerf_gaussian_blur(_lib.ptr(img), H, W, 1 if img.dim() == 2 else img.shape[2], int(k),
                                      _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream()), "nerf_gaussian_blur")
    return out.cpu().numpy() if as_numpy else out


def frame_fog(rgb, depth, fog_start=0.1):
    """The CLI's Fog frame straight from the render outputs (nerf_frame_fog): rgb float (H,W,3) in
    [0, 1] -> uint8 by truncation (run.py:233), depth float (H,W) normalised (run.py:248), then Fog
    (post_processor.py:451-493) — one reduction and one per-pixel pass on the GPU instead of a host
    round trip, a normalisation pass and the effect's own reduction.  Bit-identical to
    ``PostProcessor`` Fog on ``normalize_depth(depth)`` and ``(rgb * 255).astype(uint8)``.
    Device tensors in, a uint8 (H,W,3) device tensor out."""
    lib, dev = _lib.load(), _lib.device()
    r = torch.as_tensor(rgb).to(dev, torch.float32).contiguous()
    d = torch.as_tensor(depth).to(dev, torch.float32).contiguous()
    if r.dim() != 3 or r.shape[2] != 3 or tuple(d.shape) != tuple(r.shape[:2]):
        raise ValueError(f"frame_fog: rgb {tuple(r.shape)} must be (H,W,3) and depth {tuple(d.shape)} (H,W)")
    H, W = d.shape
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    ws = torch.empty(256, dtype=torch.uint8, device=dev)
    _lib.check(lib.nerf_frame_fog(_lib.ptr(r), _lib.ptr(d), H, W, float(fog_start), _lib.ptr(out), _lib.ptr(ws),
                                  ws.numel(), _lib.stream()), "nerf_frame_fog")
    return out


class PostProcessor:
    """GPU post-processor with the reference's effect names and parameters."""

    def __init__(self):
        self.effects = {
            "Original": self._effect_original,
            "Toon Shader": self._effect_toon,
            "Fog": self._effect_fog,
            "Bloom": self._effect_bloom,
            "Vignette": self._effect_vignette,
            "Film Grain": self._effect_film_grain,
            "Pencil Sketch": self._effect_sketch,
            "Cross Processing": self._effect_cross_processing,
            "Posterize": self._effect_posterize,
            "Hologram": self._effect_hologram,
        }
        self.rng = None        # None: numpy's global generator, as the reference (module docstring)
        self.params = {                                  # post_processor.py:33-55
            "toon_levels": 5,
            "toon_edge_strength": 1.0,
            "edge_threshold": 20,
            "color_saturation": 1.5,
            "bloom_strength": 0.3,
            "bloom_size": 15,
            "vignette_strength": 0.5,
            "fog_density": 5.0,
            "fog_color_r": 200,
            "fog_color_g": 220,
            "fog_color_b": 255,
            "fog_start": 0.1,
            "fog_ray_intensity": 0.5,
            "fog_opacity": 0.8,
            "film_grain_amount": 0.2,
            "sketch_strength": 1.0,
            "posterize_levels": 4,
            "neon_glow_intensity": 0.7,
            "neon_glow_radius": 10,
            "hologram_lines": 50,
            "hologram_intensity": 0.8,
        }
        self.current_effect = "Original"

    # ------------------------------------------------------------------ plumbing
    @staticmethod
    def _inputs(image, depth, allow_channels):
        dev = _lib.device()
        as_numpy = isinstance(image, np.ndarray)
        img = torch.as_tensor(np.ascontiguousarray(image) if as_numpy else image)
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
            raise ValueError(f"PostProcessor: image must be uint8 (H,W,3), got {tuple(img.shape)} {img.dtype}")
        img = img.to(dev).contiguous()
        H, W = img.shape[:2]
        d, stride = None, 1
        if depth is not None:
            d = torch.as_tensor(np.ascontiguousarray(depth, np.float32) if isinstance(depth, np.ndarray) else depth)
            d = d.to(dev, torch.float32).contiguous()
            if d.dim() == 3 and allow_channels:
                stride = d.shape[2]
            elif d.dim() != 2:
                raise ValueError(f"PostProcessor: depth must be (H,W){' or (H,W,C)' if allow_channels else ''}, "
                                 f"got {tuple(d.shape)}")
            if tuple(d.shape[:2]) != (H, W):
                raise ValueError(f"PostProcessor: depth {tuple(d.shape)} does not match image {H}x{W}")
        return img, d, stride, as_numpy

    @staticmethod
    def _workspace(H, W):
        return torch.empty(_lib.load().nerf_effect_workspace_bytes(H, W), dtype=torch.uint8, device=_lib.device())

    # ------------------------------------------------------------------- effects
    def _effect_original(self, image, depth=None):
        """post_processor.py:60-62."""
        return image

    def _effect_fog(self, image, depth=None):
        """post_processor.py:451-493 on the GPU (nerf_effect_fog)."""
        img, d, stride, as_numpy = self._inputs(image, depth, allow_channels=True)
        H, W = img.shape[:2]
        if d is None:
            print("Warning: No depth information for fog effect")      # post_processor.py:467
        out = torch.empty_like(img)
        ws = self._workspace(H, W)
        _lib.check(_lib.load().nerf_effect_fog(_lib.ptr(img), _lib.ptr(d), stride, H, W,
                                               float(self.params.get("fog_start", 0.0)), _lib.ptr(out),
                                               _lib.ptr(ws), ws.numel(), _lib.stream()), "nerf_effect_fog")
        return out.cpu().numpy() if as_numpy else out

    def _effect_toon(self, image, depth=None):
        """post_processor.py:64-117 on the GPU (nerf_effect_toon)."""
        img, d, _, as_numpy = self._inputs(image, depth, allow_channels=False)
        H, W = img.shape[:2]
        out = torch.empty_like(img)
        ws = self._workspace(H, W)
        _lib.check(_lib.load().nerf_effect_toon(_lib.ptr(img), _lib.ptr(d), 1, H, W,
                                                float(self.params.get("toon_levels", 5)),
                                                float(self.params.get("toon_edge_strength", 1.0)), _lib.ptr(out),
                                                _lib.ptr(ws), ws.numel(), _lib.stream()), "nerf_effect_toon")
        return out.cpu().numpy() if as_numpy else out

    def _normal(self, scale, shape):
        """float32 draws of N(0, scale) on the device: the reference's np.random.normal(0, scale,
        shape).astype(float32) from `rng` (None: numpy's global generator), or torch.randn * scale
        on a torch.Generator's own device."""
        dev = _lib.device()
        if isinstance(self.rng, torch.Generator):
            return (torch.randn(shape, generator=self.rng, device=self.rng.device, dtype=torch.float32) * scale).to(dev)
        src = np.random if self.rng is None else self.rng
        return torch.from_numpy(src.normal(0, scale, shape).astype(np.float32)).to(dev)

    @staticmethod
    def _noise(noise, shape):
        n = torch.as_tensor(noise).to(_lib.device(), torch.float32).contiguous()
        if tuple(n.shape) != tuple(shape):
            raise ValueError(f"PostProcessor: noise {tuple(n.shape)} does not match the image {tuple(shape)}")
        return n

    def _pixelwise(self, name, image, *args):
        """An effect that reads the image alone (the reference ignores its depth argument)."""
        img, _, _, as_numpy = self._inputs(image, None, allow_channels=False)
        H, W = img.shape[:2]
        out = torch.empty_like(img)
        _lib.check(getattr(_lib.load(), name)(_lib.ptr(img), H, W, *args, _lib.ptr(out), _lib.stream()), name)
        return out.cpu().numpy() if as_numpy else out

    def _effect_vignette(self, image, depth=None):
        """post_processor.py:161-186 on the GPU (nerf_effect_vignette)."""
        return self._pixelwise("nerf_effect_vignette", image, float(self.params["vignette_strength"]))

    def _effect_cross_processing(self, image, depth=None):
        """post_processor.py:271-298 on the GPU (nerf_effect_cross_processing)."""
        return self._pixelwise("nerf_effect_cross_processing", image)

    def _effect_posterize(self, image, depth=None):
        """post_processor.py:300-318 on the GPU (nerf_effect_posterize)."""
        return self._pixelwise("nerf_effect_posterize", image, float(self.params["posterize_levels"]))

    def _effect_film_grain(self, image, depth=None, noise=None):
        """post_processor.py:214-224 on the GPU (nerf_effect_film_grain).  `noise`: the float32
        grain (H,W,3) instead of a draw of N(0, 50) from `rng`."""
        img, _, _, as_numpy = self._inputs(image, None, allow_channels=False)
        H, W = img.shape[:2]
        grain = self._normal(50, tuple(img.shape)) if noise is None else self._noise(noise, img.shape)
        out = torch.empty_like(img)
        _lib.check(_lib.load().nerf_effect_film_grain(_lib.ptr(img), _lib.ptr(grain), H, W,
                                                      float(self.params["film_grain_amount"]), _lib.ptr(out),
                                                      _lib.stream()), "nerf_effect_film_grain")
        return out.cpu().numpy() if as_numpy else out

    def _effect_bloom(self, image, depth=None):
        """post_processor.py:146-159 on the GPU (nerf_effect_bloom): Gaussian blur of bloom_size
        (an even size uses the next odd one), then image + blur * bloom_strength."""
        img, _, _, as_numpy = self._inputs(image, None, allow_channels=False)
        H, W = img.shape[:2]
        size = int(self.params["bloom_size"])
        if size % 2 == 0:
            size += 1
        if not 1 <= size <= MAX_BLUR:
            raise ValueError(f"PostProcessor: bloom_size {self.params['bloom_size']!r} gives a {size}-tap blur; the "
                             f"GPU blur takes 1..{MAX_BLUR}")
        out = torch.empty_like(img)
        ws = self._workspace(H, W)
        _lib.check(_lib.load().nerf_effect_bloom(_lib.ptr(img), H, W, size, float(self.params["bloom_strength"]),
                                                 _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream()),
                   "nerf_effect_bloom")
        return out.cpu().numpy() if as_numpy else out

    def _effect_sketch(self, image, depth=None):
        """post_processor.py:226-269 on the GPU (nerf_effect_pencil_sketch); sketch_strength is
        taken as a float, as the reference's editor stores it."""
        img, d, _, as_numpy = self._inputs(image, depth, allow_channels=False)
        H, W = img.shape[:2]
        out = torch.empty_like(img)
        ws = self._workspace(H, W)
        _lib.check(_lib.load().nerf_effect_pencil_sketch(_lib.ptr(img), _lib.ptr(d), H, W,
                                                         float(self.params.get("sketch_strength", 1.0)),
                                                         _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream()),
                   "nerf_effect_pencil_sketch")
        return out.cpu().numpy() if as_numpy else out

    def _effect_hologram(self, image, depth=None, noise=None, spans=None):
        """post_processor.py:373-449 on the GPU (nerf_effect_hologram).  `noise`: the float32
        flicker (H,W,3) instead of a draw of N(0, 0.03); `spans`: three (x, width) column spans
        instead of three draws of randint(0, W), randint(2, 6).  hologram_intensity is read by the
        reference and never used; so here."""
        lines = self.params.get("hologram_lines", 50)
        if isinstance(lines, bool) or not isinstance(lines, (int, np.integer)):
            raise TypeError(f"PostProcessor: hologram_lines must be an int (the reference passes it to range()), "
                            f"got {lines!r}")
        img, d, stride, as_numpy = self._inputs(image, depth, allow_channels=True)
        H, W = img.shape[:2]
        flicker = self._normal(0.03, tuple(img.shape)) if noise is None else self._noise(noise, img.shape)
        by_value, on_device = [0] * 6, None
        if spans is not None:
            by_value = [int(v) for pair in spans for v in pair]
            if len(by_value) != 6:
                raise ValueError(f"PostProcessor: spans must be three (x, width) pairs, got {spans!r}")
        elif isinstance(self.rng, torch.Generator):
            g = self.rng
            pairs = torch.stack([torch.stack([torch.randint(0, W, (), generator=g, device=g.device),
                                              torch.randint(2, 6, (), generator=g, device=g.device)])
                                 for _ in range(3)])
            on_device = pairs.reshape(6).to(_lib.device(), torch.int64).contiguous()
        else:
            src = np.random if self.rng is None else self.rng
            for j in range(3):                                            # post_processor.py:443-446
                by_value[2 * j] = int(src.randint(0, W))
                by_value[2 * j + 1] = int(src.randint(2, 6))
        out = torch.empty_like(img)
        ws = self._workspace(H, W)
        _lib.check(_lib.load().nerf_effect_hologram(_lib.ptr(img), _lib.ptr(d), stride, H, W, int(lines),
                                                    _lib.ptr(flicker), *by_value, _lib.ptr(on_device), _lib.ptr(out),
                                                    _lib.ptr(ws), ws.numel(), _lib.stream()), "nerf_effect_hologram")
        return out.cpu().numpy() if as_numpy else out

    def apply_effect(self, image, depth=None):
        """post_processor.py:495-499: the current effect (unknown names return the image)."""
        if self.current_effect in self.effects:
            return self.effects[self.current_effect](image, depth)
        if self.current_effect in REFERENCE_ONLY_EFFECTS:
            raise NotImplementedError(f"PostProcessor: '{self.current_effect}' is an effect of the reference that "
                                      f"nerfmi does not run on the GPU (available: {sorted(self.effects)})")
        return image
