"""Occupancy grid for sample skipping (include/nerfmi.h "occupancy grid").  Not a
reference feature: the reference evaluates its MLP on every sample of every ray.

``OccupancyGrid(aabb_min, aabb_max, resolution)`` is an axis-aligned box, G = resolution cells per
axis and G^3 bits on the device (all clear until one of the builders fills them):

    grid = OccupancyGrid.from_model(model, (-1.5,) * 3, (1.5,) * 3, resolution=128)
    rgb, depth, extras = volume_render(model, o, d, near, far, N, Nf, occupancy=grid)

Cell (ix, iy, iz) is bit ``index & 31`` of word ``index >> 5``, index = (iz*G + iy)*G + ix.  A sample
at p = o + d*z is live iff for every axis t = (p - lo) * inv (float32, two roundings) has
0 <= t < G and the bit of cell (int(t_x), int(t_y), int(t_z)) is set; rendering with a grid is the
plain render with the sigma of every dead sample replaced by 0 (the MLP is not run on them).
Training takes the same grid and the same rule (train.py: ``Trainer(config, occupancy=grid,
occupancy_refresh={...})``, ``train_nerf(..., occupancy=grid)``): a step runs the MLP
forward, backward and weight gradients on the live samples only, and with ``occupancy_refresh`` the
trainer rebuilds the bits from its own model (from_model) as the weights change.

Builders (each returns the grid):
  grid.from_mask(mask)           bool (G,G,G) indexed [iz, iy, ix]
  grid.from_density(sigma, threshold=0.0, supersample=1, dilate=1)
                                 float (sG,sG,sG) lattice of densities indexed [z, y, x], s probes per
                                 cell and axis: bit = max over the cell's s^3 probes > threshold, then
                                 `dilate` 3x3x3 dilations (libnerfmi.so's pack and dilate kernels)
  OccupancyGrid.from_model(model, aabb_min, aabb_max, resolution=128, threshold=0.0, supersample=1,
                           dilate=1)
                                 from_density of the model's sigma at probe_points(supersample),
                                 evaluated by the render MLP in slabs of lattice rows
"""
import ctypes

import numpy as np
import torch

from . import _lib

MAX_RESOLUTION = 1024


def _f3(v, name):
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.shape != (3,) or not np.all(np.isfinite(a)):
        raise ValueError(f"OccupancyGrid: {name} must be 3 finite numbers, got {v!r}")
    return a.astype(np.float32)


class OccupancyGrid:
    def __init__(self, aabb_min, aabb_max, resolution, device=None):
        lo, hi = _f3(aabb_min, "aabb_min"), _f3(aabb_max, "aabb_max")
        if isinstance(resolution, bool) or int(resolution) != resolution:
            raise ValueError(f"OccupancyGrid: resolution must be an integer, got {resolution!r}")
        G = int(resolution)
        if not 1 <= G <= MAX_RESOLUTION:
            raise ValueError(f"OccupancyGrid: resolution {G} outside 1..{MAX_RESOLUTION}")
        if not np.all(hi > lo):
            raise ValueError(f"OccupancyGrid: aabb_max {tuple(hi)} must exceed aabb_min {tuple(lo)} on every axis")
        inv = (G / (hi.astype(np.float64) - lo.astype(np.float64))).astype(np.float32)
        if not np.all(np.isfinite(inv)):
            raise ValueError("OccupancyGrid: the box is too thin for this resolution")
        self.resolution = G
        self.lo, self.hi, self.inv = lo, hi, inv
        self.device = torch.device(device) if device is not None else _lib.device()
        self.bits = torch.zeros(self.words, dtype=torch.int32, device=self.device)

    # ------------------------------------------------------------------ layout
    @property
    def words(self):
        return (self.resolution ** 3 + 31) // 32

    def c_lo(self):
        return (ctypes.c_float * 3)(*[float(v) for v in self.lo])

    def c_inv(self):
        return (ctypes.c_float * 3)(*[float(v) for v in self.inv])

    # ---------------------------------------------------------------- builders
    def from_mask(self, mask):
        G = self.resolution
        m = torch.as_tensor(mask)
        if m.dtype != torch.bool or tuple(m.shape) != (G, G, G):
            raise ValueError(f"OccupancyGrid.from_mask: expected a bool ({G},{G},{G}) mask indexed [iz, iy, ix], "
                             f"got {m.dtype} {tuple(m.shape)}")
        flat = torch.zeros(self.words * 32, dtype=torch.int64, device=self.device)
        flat[:G ** 3] = m.reshape(-1).to(self.device, torch.int64)
        w = (flat.reshape(-1, 32) << torch.arange(32, device=self.device)).sum(1)
        self.bits = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
        return self

    def from_density(self, sigma, threshold=0.0, supersample=1, dilate=1):
        G, s = self.resolution, int(supersample)
        if s < 1 or int(dilate) < 0:
            raise ValueError(f"OccupancyGrid.from_density: supersample={supersample} dilate={dilate}")
        L = s * G
        lat = torch.as_tensor(sigma)
        if lat.numel() != L ** 3:
            raise ValueError(f"OccupancyGrid.from_density: expected {L}^3 densities, got {tuple(lat.shape)}")
        lat = lat.reshape(-1).to(self.device, torch.float32).contiguous()
        lib = _lib.load()
        bits = torch.empty(self.words, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.nerf_occupancy_pack(_lib.ptr(lat), G, s, float(threshold), _lib.ptr(bits), _lib.stream()),
                       "nerf_occupancy_pack")
            for _ in range(int(dilate)):
                out = torch.empty_like(bits)
                _lib.check(lib.nerf_occupancy_dilate(_lib.ptr(bits), G, _lib.ptr(out), _lib.stream()),
                           "nerf_occupancy_dilate")
                bits = out
        self.bits = bits
        return self

    def _axis_probes(self, c, s):
        """Probe coordinates of axis c (float32, on the grid's device): lo + (k + 0.5) h for the y and z
        axes; for x the value the MLP kernel forms for sample k of a lattice-row ray, o + 1*z with
        o = lo + 0.5 h and z = k h (from_model passes each lattice row as one ray along x)."""
        L = s * self.resolution
        lo = torch.tensor(float(self.lo[c]), dtype=torch.float32, device=self.device)
        h = torch.tensor(float(np.float32((np.float64(self.hi[c]) - np.float64(self.lo[c])) / L)),
                         dtype=torch.float32, device=self.device)
        k = torch.arange(L, dtype=torch.float32, device=self.device)
        if c == 0:
            return (lo + 0.5 * h) + k * h, lo + 0.5 * h, k * h
        return lo + (k + 0.5) * h, None, None

    def probe_points(self, supersample=1):
        """The (sG, sG, sG, 3) probe lattice indexed [z, y, x], float32: exactly the points from_model
        evaluates."""
        s = int(supersample)
        L = s * self.resolution
        px = self._axis_probes(0, s)[0]
        py = self._axis_probes(1, s)[0]
        pz = self._axis_probes(2, s)[0]
        pts = torch.empty(L, L, L, 3, dtype=torch.float32, device=self.device)
        pts[..., 0] = px.view(1, 1, L)
        pts[..., 1] = py.view(1, L, 1)
        pts[..., 2] = pz.view(L, 1, 1)
        return pts

    @classmethod
    def from_model(cls, model, aabb_min, aabb_max, resolution=128, threshold=0.0, supersample=1, dilate=1,
                   slab_samples=1 << 21):
        """Sigma of `model` on the probe lattice through nerf_mlp_forward (sigma ignores direction and
        appearance): each lattice row along x is one ray, so the ray features are one row per lattice
        row; slabs of about slab_samples samples keep the memory bounded."""
        from .render import packed_for
        grid = cls(aabb_min, aabb_max, resolution)
        s = int(supersample)
        if s < 1:
            raise ValueError(f"OccupancyGrid.from_model: supersample={supersample}")
        dev, L = grid.device, s * grid.resolution
        lib = _lib.load()
        packed = packed_for(model)
        _, ox, zrow = grid._axis_probes(0, s)
        py, pz = grid._axis_probes(1, s)[0], grid._axis_probes(2, s)[0]
        rows = L * L
        per = max(1, min(rows, int(slab_samples) // L))
        lattice = torch.empty(rows * L, device=dev)
        dirs = torch.zeros(per, 3, device=dev)
        dirs[:, 0] = 1.0
        feat = torch.empty(per, 256, device=dev)
        rgb = torch.empty(per * L, 3, device=dev)
        zv = zrow.repeat(per).contiguous()
        st = _lib.stream()
        _lib.check(lib.nerf_ray_features(_lib.ptr(packed), _lib.ptr(dirs), per, None, 0, _lib.ptr(feat), st),
                   "nerf_ray_features")
        for r0 in range(0, rows, per):
            n = min(per, rows - r0)
            j = torch.arange(r0, r0 + n, device=dev)
            o = torch.stack([ox.expand(n), py[j % L], pz[j // L]], dim=1).contiguous()
            sig = lattice[r0 * L:(r0 + n) * L]
            _lib.check(lib.nerf_mlp_forward(_lib.ptr(packed), _lib.ptr(o), _lib.ptr(dirs), _lib.ptr(zv), n, L,
                                            _lib.ptr(feat), _lib.ptr(rgb), _lib.ptr(sig), None, 0, st),
                       "nerf_mlp_forward")
        return grid.from_density(lattice, threshold, s, dilate)

    # ---------------------------------------------------------------- queries
    def to_mask(self):
        """bool (G,G,G) indexed [iz, iy, ix], on the grid's device."""
        G = self.resolution
        sh = torch.arange(32, device=self.bits.device)
        cells = ((self.bits.view(-1, 1) >> sh) & 1).reshape(-1)[:G ** 3]
        return cells.bool().reshape(G, G, G)

    def fraction(self):
        """Share of set cells (reduced on the device)."""
        n = sum(((self.bits >> k) & 1).sum(dtype=torch.int64) for k in range(32))
        return float(n) / self.resolution ** 3

    def state_dict(self):
        return {"bits": self.bits.cpu(), "aabb_min": torch.from_numpy(self.lo.copy()),
                "aabb_max": torch.from_numpy(self.hi.copy()), "resolution": self.resolution}

    def load_state_dict(self, sd):
        other = OccupancyGrid.__new__(OccupancyGrid)
        OccupancyGrid.__init__(other, sd["aabb_min"].tolist(), sd["aabb_max"].tolist(), int(sd["resolution"]),
                               device=self.device)
        bits = torch.as_tensor(sd["bits"])
        if bits.dtype != torch.int32 or bits.numel() != other.words:
            raise ValueError(f"OccupancyGrid.load_state_dict: bits {bits.dtype} x {bits.numel()}, expected int32 x "
                             f"{other.words}")
        self.resolution, self.lo, self.hi, self.inv = other.resolution, other.lo, other.hi, other.inv
        self.bits = bits.reshape(-1).to(self.device).contiguous()
        return self
