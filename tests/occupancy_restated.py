"""The occupancy-grid contract restated in torch CPU float32 / numpy, operation for operation
(include/nerfmi.h "occupancy grid"): the yardstick of tests/test_occupancy_host.py and
tests/test_gpu_occupancy.py.  Nothing here is derived from the code under test.

Grid: box lo, hi (float32), G cells per axis, mask bool (G,G,G) indexed [iz, iy, ix]; cell
(ix, iy, iz) has index (iz G + iy) G + ix = bit (index & 31) of uint32 word (index >> 5).
"""
import numpy as np
import torch


def inv_of(lo, hi, G):
    """inv_c = float32(G / (double(hi_c) - double(lo_c)))."""
    lo32, hi32 = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    return (G / (hi32.astype(np.float64) - lo32.astype(np.float64))).astype(np.float32)


def cell_coords(o, dn, z, lo, hi, G):
    """t (B,n,3) float32 of every sample: p = o + d*z with two roundings, t = (p - lo) * inv with two
    more (separate torch ops: no fused multiply-add)."""
    lo_t = torch.from_numpy(np.asarray(lo, np.float32))
    inv_t = torch.from_numpy(inv_of(lo, hi, G))
    prod = dn.float().unsqueeze(1) * z.float().unsqueeze(-1)
    p = o.float().unsqueeze(1) + prod
    diff = p - lo_t
    return diff * inv_t


def classify(o, dn, z, lo, hi, G, mask):
    """live (B,n) bool: 0 <= t_c < G on every axis (float compares: NaN is dead) and the cell's bit."""
    t = cell_coords(o, dn, z, lo, hi, G)
    Gf = torch.tensor(float(G), dtype=torch.float32)
    inside = ((t >= 0) & (t < Gf)).all(-1)
    c = torch.where(inside.unsqueeze(-1), t, torch.zeros_like(t)).to(torch.int64)   # (int)t, truncation
    m = torch.as_tensor(mask).bool()
    return inside & m[c[..., 2], c[..., 1], c[..., 0]]


def live_list(live):
    """Ascending indices r*n + s of the live samples (int32) and their count."""
    idx = torch.nonzero(live.reshape(-1)).reshape(-1).to(torch.int32)
    return idx, int(idx.numel())


def pack_bits(mask):
    """uint32 words (numpy) of a bool (G,G,G) [iz, iy, ix] mask."""
    flat = np.asarray(mask, bool).reshape(-1)
    words = (flat.size + 31) // 32
    padded = np.zeros(words * 32, np.uint64)
    padded[:flat.size] = flat
    return (padded.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)


def unpack_bits(words, G):
    w = np.asarray(words).view(np.uint32).reshape(-1, 1)
    return ((w >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1)[:G ** 3].astype(bool).reshape(G, G, G)


def threshold_mask(lattice, G, s, thr):
    """bit = (max over the cell's s^3 probes) > thr, lattice (sG,sG,sG) indexed [z, y, x]."""
    lat = np.asarray(lattice, np.float32).reshape(G, s, G, s, G, s)
    return lat.max(axis=(1, 3, 5)) > np.float32(thr)


def dilate(mask, times=1):
    """3 x 3 x 3 binary dilation clamped at the box faces (cells outside the box are unset)."""
    m = np.asarray(mask, bool)
    G = m.shape[0]
    for _ in range(times):
        pad = np.zeros((G + 2,) * 3, bool)
        pad[1:-1, 1:-1, 1:-1] = m
        out = np.zeros_like(m)
        for dz in range(3):
            for dy in range(3):
                for dx in range(3):
                    out |= pad[dz:dz + G, dy:dy + G, dx:dx + G]
        m = out
    return m


# ------------------------------------------------------------------ masks used by the tests
def sphere_mask(G, radius=0.3):
    c = (np.arange(G) + 0.5) / G - 0.5
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    return x * x + y * y + z * z < radius * radius


def checker_mask(G):
    i = np.arange(G)
    z, y, x = np.meshgrid(i, i, i, indexing="ij")
    return (x + y + z) % 2 == 0


def single_cell_mask(G, cell):
    m = np.zeros((G, G, G), bool)
    m[cell[2], cell[1], cell[0]] = True
    return m
