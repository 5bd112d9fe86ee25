"""numpy restatement of the seven PostProcessor effects added after Fog and Toon — TEST
INFRASTRUCTURE ONLY (the checker of csrc/effects.hip's second half).

Vignette (src/post_processor.py:161-186), Cross Processing (:271-298), Film Grain (:214-224),
Hologram (:373-449), Posterize (:300-318), Bloom (:146-159) and Pencil Sketch (:226-269), each
restated operation for operation with numpy 2's promotion rules (a Python float with a uint8 array
gives float64, with a float32 array float32; uint8 with a float32 array gives float32;
np.percentile of a float32 array works in float32 throughout, index included).

Pinning (tests/golden/make_effects_golden.py, fixture F10).  Vignette, Cross Processing, Film Grain
and Hologram without depth are numpy alone in the reference: F10 holds the reference's own outputs
and these functions equal them bit for bit.  The other effects call cv2, which is not installed:
the generator runs the reference's methods with `Cv2StandIn` below in cv2's place, so F10 pins the
numpy glue around six cv2 calls, and the calls themselves are **parity unpinned**:
  cvtColor(RGB2GRAY), Laplacian, Sobel   as oracle/post_oracle.py restates them (exact in integers
                                         for the first two);
  divide(a, b, scale)                    0 where b is 0, else rint(scale a / b) saturated;
  GaussianBlur(src, (k, k), 0)           float32 separable filter defined in `gaussian_blur_u8`
                                         (cv2's 8-bit path uses fixed-point coefficients and may
                                         differ by a count);
  addWeighted(a, 1, b, beta, 0)          a + b float32(beta) in float32, rounded half to even.
Reflect-101 borders reflect repeatedly, so images narrower than a filter radius work.
"""
import math

import numpy as np

from oracle import post_oracle as P

F32 = np.float32

DEFAULTS = {"bloom_strength": 0.3, "bloom_size": 15, "vignette_strength": 0.5, "film_grain_amount": 0.2,
            "sketch_strength": 1.0, "posterize_levels": 4, "hologram_lines": 50, "hologram_intensity": 0.8}


def reflect101(i, n):
    """cv2 BORDER_REFLECT_101 applied until the index is inside [0, n)."""
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    period = 2 * n - 2
    i = np.mod(i, period)
    return np.where(i >= n, period - i, i)


def shift(a, dy, dx):
    """a[reflect101(y+dy), reflect101(x+dx)] for every (y, x)."""
    H, W = a.shape
    return a[reflect101(np.arange(H) + dy, H)][:, reflect101(np.arange(W) + dx, W)]


# ------------------------------------------------------------------------------ cv2 stand-ins
def gaussian_kernel(k):
    """cv2.getGaussianKernel(k, 0) as float32: OpenCV's fixed tables for k <= 7, else
    exp(-(i - (k-1)/2)^2 / (2 sigma^2)) with sigma = 0.3 ((k-1) 0.5 - 1) + 0.8, normalised in double."""
    small = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
             7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}
    if k in small:
        return np.array(small[k], F32)
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    w = []
    for i in range(k):
        x = i - (k - 1) * 0.5
        w.append(math.exp(-(x * x) / (2.0 * sigma * sigma)))
    s = 0.0
    for v in w:
        s += v
    return np.array([v / s for v in w], np.float64).astype(F32)


def gaussian_blur_u8(src, k):
    """GaussianBlur on uint8 (H,W) or (H,W,C), odd k: horizontal then vertical pass, float32
    intermediate, taps accumulated in order (one multiply and one add rounding each), reflect-101,
    then round half to even and saturate."""
    assert k % 2 == 1 and 1 <= k <= 63
    w = gaussian_kernel(k)
    a = src.astype(F32)
    if a.ndim == 2:
        a = a[:, :, None]
    H, W = a.shape[:2]
    r = k // 2
    pad = a[:, reflect101(np.arange(-r, W + r), W)]
    acc = np.zeros_like(a)
    for i in range(k):
        acc = acc + w[i] * pad[:, i:i + W]
    pad = acc[reflect101(np.arange(-r, H + r), H)]
    out = np.zeros_like(a)
    for i in range(k):
        out = out + w[i] * pad[i:i + H]
    out = np.clip(np.rint(out), 0, 255).astype(np.uint8)
    return out.reshape(src.shape)


def gray_u8(image):
    return P.gray_u8(image).astype(np.uint8)


def laplacian_i(gray):
    """cv2.Laplacian (ksize 1) of a uint8 image, exact in integers."""
    g = gray.astype(np.int64)
    return shift(g, -1, 0) + shift(g, 0, -1) + shift(g, 0, 1) + shift(g, 1, 0) - 4 * g


def sobel_xy(f):
    """cv2.Sobel(f, CV_32F, 1, 0, 3) and (0, 1): the two halves of oracle/post_oracle.py sobel_mag."""
    f = np.asarray(f, F32)
    r = {k: shift(f, k, 1) - shift(f, k, -1) for k in (-1, 0, 1)}
    gx = r[0] * F32(2.0) + (r[-1] + r[1])
    h = {k: shift(f, k, 0) * F32(2.0) + (shift(f, k, -1) + shift(f, k, 1)) for k in (-1, 1)}
    return gx, h[1] - h[-1]


def divide_u8(a, b, scale):
    q = np.rint(scale * a.astype(np.float64) / np.where(b == 0, 1, b).astype(np.float64))
    return np.where(b == 0, 0, np.clip(q, 0, 255)).astype(np.uint8)


def add_weighted_u8(a, b, beta):
    return np.clip(np.rint(a.astype(F32) + b.astype(F32) * F32(beta)), 0, 255).astype(np.uint8)


class Cv2StandIn:
    """The six cv2 calls of the seven effects, for running the reference's methods without cv2;
    `called` lists the names used."""
    COLOR_RGB2GRAY, CV_32F, CV_64F = 7, 5, 6

    def __init__(self):
        self.called = []

    def cvtColor(self, image, code):
        assert code == self.COLOR_RGB2GRAY and image.dtype == np.uint8
        self.called.append("cvtColor")
        return gray_u8(image)

    def Laplacian(self, src, ddepth):
        assert ddepth == self.CV_64F and src.dtype == np.uint8
        self.called.append("Laplacian")
        return laplacian_i(src).astype(np.float64)

    def Sobel(self, src, ddepth, dx, dy, ksize=3):
        assert ddepth == self.CV_32F and ksize == 3 and src.dtype == np.float32 and (dx, dy) in ((1, 0), (0, 1))
        self.called.append("Sobel")
        return sobel_xy(src)[0 if dx else 1]

    def GaussianBlur(self, src, ksize, sigma):
        assert sigma == 0 and ksize[0] == ksize[1] and src.dtype == np.uint8
        self.called.append("GaussianBlur")
        return gaussian_blur_u8(src, ksize[0])

    def addWeighted(self, a, alpha, b, beta, gamma):
        assert alpha == 1.0 and gamma == 0 and a.dtype == b.dtype == np.uint8
        self.called.append("addWeighted")
        return add_weighted_u8(a, b, beta)

    def divide(self, a, b, scale=1.0):
        assert a.dtype == b.dtype == np.uint8
        self.called.append("divide")
        return divide_u8(a, b, scale)


# ----------------------------------------------------------------------------------- helpers
def percentile(x, q):
    """np.percentile(x, q) of a float32 array (method "linear"), as numpy 2 computes it: the
    quantile q / 100, the virtual index (n - 1) quantile and the interpolation all in float32,
    a + (b - a) t replaced by b - (b - a)(1 - t) where t >= 0.5."""
    a = np.sort(np.asarray(x, F32).ravel())
    n = a.size
    v = F32(n - 1) * (F32(q) / F32(100))
    if v >= F32(n - 1):
        return a[-1]
    lo = int(np.floor(v))
    hi = min(lo + 1, n - 1)
    t = F32(v - F32(lo))
    d = a[hi] - a[lo]
    return a[hi] - d * (F32(1) - t) if t >= F32(0.5) else a[lo] + d * t


def depth_norm(depth):
    d = np.array(depth, dtype=F32, copy=True)
    if d.max() > 1.0:
        d = d / d.max()
    return d


def _radial(H, W):
    y, x = np.ogrid[0:H, 0:W]
    return (x - W // 2) ** 2 + (y - H // 2) ** 2


# ----------------------------------------------------------------------------------- effects
def vignette(image, depth=None, strength=0.5):
    H, W = image.shape[:2]
    dist = np.sqrt(_radial(H, W)) / np.sqrt(np.float64((W // 2) ** 2 + (H // 2) ** 2))
    v = np.clip(1 - dist * float(strength), 0, 1)                        # float64
    result = (image.astype(F32) * v[:, :, None]).astype(F32)             # float64 product, stored as float32
    return np.clip(result, 0, 255).astype(np.uint8)


def cross_processing(image, depth=None):
    f = image.astype(F32) / F32(255.0)
    for c, k in enumerate((1.1, 1.3, 0.8)):
        f[:, :, c] = np.clip(f[:, :, c] * F32(k), 0, 1)
    f = (f - F32(0.5)) * F32(1.4) + F32(0.5)
    result = np.clip(f * F32(255), 0, 255).astype(np.uint8)
    H, W = image.shape[:2]
    mask = np.clip(1.2 - (_radial(H, W) / (W / 2) ** 2) * 0.4, 0, 1)     # float64
    return (result.astype(F32) * mask[:, :, None]).astype(np.uint8)


def film_grain(image, depth=None, amount=0.2, rng=None):
    rng = np.random if rng is None else rng
    grain = rng.normal(0, 50, image.shape).astype(F32)
    return np.clip(image.astype(F32) + grain * F32(amount), 0, 255).astype(np.uint8)


def hologram_rows(H, lines):
    """The scanline factor of each row: 0.85 multiplied in once per line i whose span covers it."""
    lh = H / lines
    f = np.ones(H, F32)
    for i in range(lines):
        f[int(i * lh):int(min((i + 0.7) * lh, H))] *= F32(0.85)
    return f


def hologram(image, depth=None, lines=50, rng=None):
    rng = np.random if rng is None else rng
    f = image.astype(F32) / F32(255.0)
    base = f * np.array([0.8, 1.0, 0.2], F32) * hologram_rows(image.shape[0], lines)[:, None, None]
    noise = rng.normal(0, 0.03, f.shape).astype(F32)
    glow = np.zeros_like(f)
    if depth is not None:
        dn = depth_norm(depth)                       # the max is over every channel (:407-409) ...
        if dn.ndim > 2:
            dn = dn[:, :, 0]                         # ... then channel 0 (:412-413)
        gx, gy = sobel_xy(dn)
        edges = np.sqrt(gx * gx + gy * gy)
        if edges.max() > 0:
            edges = edges / edges.max()
        glow = np.stack([edges * F32(0.1), edges * F32(0.6), edges * F32(0.3)], axis=2)
    h = base + glow + noise
    W = image.shape[1]
    for _ in range(3):
        x0 = rng.randint(0, W)
        x1 = min(x0 + rng.randint(2, 6), W)
        h[:, x0:x1, :] *= F32(1.5)
    return np.clip(h * F32(255), 0, 255).astype(np.uint8)


def posterize(image, depth=None, levels=4):
    q = np.floor(image.astype(F32) / F32(255.0) * F32(levels)) / F32(levels) * F32(255.0)
    edges = np.abs(laplacian_i(gray_u8(image))) > 20
    mixed = np.float64(255) * 0.3 + (q * F32(0.7)).astype(np.float64)
    result = np.where(edges[:, :, None], mixed, q.astype(np.float64))
    return np.clip(result, 0, 255).astype(np.uint8)


def bloom(image, depth=None, strength=0.3, size=15):
    size = int(size)
    if size % 2 == 0:
        size += 1
    return add_weighted_u8(image, gaussian_blur_u8(image, size), strength)


def pencil_sketch(image, depth=None, strength=1.0):
    strength = float(strength)
    gray = gray_u8(image)
    inv_blur = 255 - gaussian_blur_u8(255 - gray, 21)
    sketch = divide_u8(gray, inv_blur, 256.0)
    mask = np.ones(gray.shape, F32)
    if depth is not None:
        dn = depth_norm(depth)
        mask = F32(1.0) - np.clip((dn - percentile(dn, 70)) * F32(5), 0, 1)
    img64 = image.astype(np.float64)
    blend = (1 - strength) * img64 + strength * sketch.astype(np.float64)[:, :, None]
    result = (blend * mask.astype(np.float64)[:, :, None]).astype(F32)
    result = result + image.astype(F32) * (F32(1) - mask)[:, :, None]
    return np.clip(result, 0, 255).astype(np.uint8)


def apply(name, image, depth=None, params=None, rng=None):
    """Effect `name` with the reference's parameter table (defaults where `params` has no entry)."""
    p = dict(DEFAULTS, **(params or {}))
    if name == "Vignette":
        return vignette(image, depth, p["vignette_strength"])
    if name == "Cross Processing":
        return cross_processing(image, depth)
    if name == "Film Grain":
        return film_grain(image, depth, p["film_grain_amount"], rng)
    if name == "Hologram":
        return hologram(image, depth, p["hologram_lines"], rng)
    if name == "Posterize":
        return posterize(image, depth, p["posterize_levels"])
    if name == "Bloom":
        return bloom(image, depth, p["bloom_strength"], p["bloom_size"])
    if name == "Pencil Sketch":
        return pencil_sketch(image, depth, p["sketch_strength"])
    raise KeyError(name)
