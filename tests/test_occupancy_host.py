"""CPU-side checks of the occupancy-grid feature: the new C-ABI symbols and their argument checks
(none of which launches anything), OccupancyGrid's argument validation, and the invariants of the
restated contract (tests/occupancy_restated.py) that the GPU tests measure the kernels against."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from nerfmi import _lib

sys.path.insert(0, os.path.join(REPO, "tests"))
import occupancy_restated as R   # noqa: E402

NEW = ("nerf_occupancy_words", "nerf_occupancy_pack", "nerf_occupancy_dilate", "nerf_occupancy_classify",
       "nerf_occupancy_classify_workspace_bytes", "nerf_mlp_forward_live", "nerf_render_occ_workspace_bytes",
       "nerf_render_rays_occ")
FAKE = ctypes.c_void_p(0x1000)
F3 = ctypes.c_float * 3


def test_new_symbols_are_exported_with_signatures():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTED, name
        res, args = _lib._SIGNATURES[name]
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert lib.nerf_abi_version() == 11          # additions only


def test_occupancy_words():
    lib = _lib.load()
    for G in (1, 2, 3, 4, 5, 32, 33, 128, 1024):
        assert lib.nerf_occupancy_words(G) == (G ** 3 + 31) // 32, G
    assert lib.nerf_occupancy_words(0) == 0 and lib.nerf_occupancy_words(1025) == 0 and lib.nerf_occupancy_words(-3) == 0


def _render_occ(lib, B=4, N=8, Nf=0, G=8, bits=FAKE, ws=FAKE, ws_bytes=1 << 30, packed=FAKE):
    lo, inv = F3(-1, -1, -1), F3(4, 4, 4)
    return lib.nerf_render_rays_occ(packed, FAKE, FAKE, B, 2.0, 6.0, N, Nf, FAKE, FAKE, 0, None, None, 0, 0, None, 0,
                                    bits, G, lo, inv, FAKE, FAKE, None, None, None, None, ws, ws_bytes, None)


def test_bad_arguments_return_the_right_code_without_a_launch():
    lib = _lib.load()
    lo, inv = F3(-1, -1, -1), F3(4, 4, 4)
    # null pointers -> NERF_ERR_BAD_ARG
    assert lib.nerf_occupancy_pack(None, 8, 1, 0.0, FAKE, None) == 1
    assert b"nerf_occupancy_pack" in lib.nerf_last_error()
    assert lib.nerf_occupancy_pack(FAKE, 8, 0, 0.0, FAKE, None) == 1            # s >= 1
    assert lib.nerf_occupancy_dilate(FAKE, 8, None, None) == 1
    assert lib.nerf_occupancy_dilate(FAKE, 8, FAKE, None) == 1                  # not in place
    assert lib.nerf_occupancy_classify(None, None, None, 4, 8, FAKE, 8, lo, inv, FAKE, FAKE, None, FAKE, 1 << 20,
                                       None) == 1
    assert lib.nerf_occupancy_classify(FAKE, FAKE, FAKE, 4, 8, None, 8, lo, inv, FAKE, FAKE, None, FAKE, 1 << 20,
                                       None) == 1
    assert lib.nerf_occupancy_classify(FAKE, FAKE, FAKE, 4, 8, FAKE, 8, None, inv, FAKE, FAKE, None, FAKE, 1 << 20,
                                       None) == 1
    assert lib.nerf_mlp_forward_live(None, None, None, None, 4, 8, None, None, FAKE, None, None, None) == 1
    assert lib.nerf_mlp_forward_live(FAKE, FAKE, FAKE, FAKE, 4, 8, FAKE, FAKE, None, FAKE, FAKE, None) == 1
    assert _render_occ(lib, bits=None) == 1
    assert _render_occ(lib, packed=None) == 1 and b"nerf_render_rays_occ" in lib.nerf_last_error()
    assert _render_occ(lib, B=-1) == 1
    # G = 0 or G > 1024 -> NERF_ERR_UNSUPPORTED
    for G in (0, 1025):
        assert lib.nerf_occupancy_pack(FAKE, G, 1, 0.0, FAKE, None) == 3, G
        assert lib.nerf_occupancy_dilate(FAKE, G, ctypes.c_void_p(0x2000), None) == 3, G
        assert lib.nerf_occupancy_classify(FAKE, FAKE, FAKE, 4, 8, FAKE, G, lo, inv, FAKE, FAKE, None, FAKE, 1 << 20,
                                           None) == 3, G
        assert _render_occ(lib, G=G) == 3, G
        assert b"1..1024" in lib.nerf_last_error()
    assert _render_occ(lib, N=5000) == 3 and _render_occ(lib, N=300, Nf=8) == 3   # nerf_render_rays' ranges
    # a short workspace -> NERF_ERR_WORKSPACE
    need = lib.nerf_occupancy_classify_workspace_bytes(1000, 7)
    assert need >= 4 * ((7000 + 255) // 256)
    assert lib.nerf_occupancy_classify(FAKE, FAKE, FAKE, 1000, 7, FAKE, 8, lo, inv, FAKE, FAKE, None, FAKE, need - 1,
                                       None) == 4
    for N, Nf in ((8, 0), (8, 4)):
        need = lib.nerf_render_occ_workspace_bytes(4, N, Nf)
        assert _render_occ(lib, N=N, Nf=Nf, ws_bytes=need - 1) == 4, (N, Nf)
        assert b"workspace" in lib.nerf_last_error()
    # empty batches are a no-op
    assert _render_occ(lib, B=0) == 0


def test_render_occ_workspace_bytes():
    lib = _lib.load()
    assert lib.nerf_render_occ_workspace_bytes(-1, 64, 0) == 0
    assert lib.nerf_render_occ_workspace_bytes(4, 0, 0) == 0
    for B, N, Nf in ((37, 7, 0), (1024, 64, 128), (37, 5, 3)):
        plain = lib.nerf_render_workspace_bytes(B, N, Nf)
        occ = lib.nerf_render_occ_workspace_bytes(B, N, Nf)
        per = B * max(N, Nf)
        # the plain carve plus the live list, the count and the classify block counts
        assert occ >= plain + 4 * per + 4 + 4 * ((per + 255) // 256)
        assert occ <= plain + 4 * per + 4 * ((per + 255) // 256) + 3 * 256
    assert lib.nerf_occupancy_classify_workspace_bytes(-1, 4) == 0
    assert lib.nerf_occupancy_classify_workspace_bytes(4, 0) == 0


def test_grid_argument_validation():
    from nerfmi import OccupancyGrid
    bad = [dict(aabb_min=(0, 0), aabb_max=(1, 1, 1), resolution=8),
           dict(aabb_min=(0, 0, 0), aabb_max=(1, 1, float("nan")), resolution=8),
           dict(aabb_min=(0, 0, 0), aabb_max=(1, 0, 1), resolution=8),          # empty on y
           dict(aabb_min=(0, 0, 0), aabb_max=(1, 1, 1), resolution=0),
           dict(aabb_min=(0, 0, 0), aabb_max=(1, 1, 1), resolution=1025),
           dict(aabb_min=(0, 0, 0), aabb_max=(1, 1, 1), resolution=7.5)]
    for kw in bad:
        with pytest.raises(ValueError, match="OccupancyGrid"):
            OccupancyGrid(**kw)
    g = OccupancyGrid((-1.5, -1.3, -1.7), (1.6, 1.9, 1.4), 5, device="cpu")     # (no kernel runs on a CPU grid)
    assert g.bits.dtype == torch.int32 and g.bits.numel() == 4 and g.words == 4
    assert np.array_equal(g.inv, R.inv_of((-1.5, -1.3, -1.7), (1.6, 1.9, 1.4), 5)) and g.inv.dtype == np.float32
    with pytest.raises(ValueError, match="from_mask"):
        g.from_mask(torch.zeros(5, 5, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="from_mask"):
        g.from_mask(torch.zeros(5, 5, 5))
    m = R.checker_mask(5)
    g.from_mask(torch.from_numpy(m))
    assert np.array_equal(g.bits.numpy().view(np.uint32), R.pack_bits(m))
    assert np.array_equal(g.to_mask().numpy(), m) and g.fraction() == m.sum() / 125
    g2 = OccupancyGrid((0, 0, 0), (1, 1, 1), 3, device="cpu").load_state_dict(g.state_dict())
    assert g2.resolution == 5 and np.array_equal(g2.lo, g.lo) and torch.equal(g2.bits, g.bits)
    with pytest.raises(ValueError, match="from_density"):
        g.from_density(torch.zeros(5, 5, 5), supersample=2)


def test_volume_render_refuses_what_a_grid_cannot_do():
    import nerfmi
    g = nerfmi.OccupancyGrid((-1, -1, -1), (1, 1, 1), 4, device="cpu")
    model = nerfmi.NeRF(nerfmi.Config()).requires_grad_(False)
    o, d = torch.zeros(2, 3), torch.ones(2, 3)
    with torch.no_grad():
        for kw, what in ((dict(staged=True), "staged=True"), (dict(timing=[]), "timing=")):
            with pytest.raises(ValueError, match=what):
                nerfmi.volume_render(model, o, d, 2.0, 6.0, 8, 0, occupancy=g, **kw)
        with pytest.raises(ValueError, match="OccupancyGrid"):
            nerfmi.volume_render(model, o, d, 2.0, 6.0, 8, 0, occupancy=torch.zeros(4))
    model.requires_grad_(True)
    with pytest.raises(ValueError, match="gradients"):
        nerfmi.volume_render(model, o, d, 2.0, 6.0, 8, 0, occupancy=g)


def test_restated_rule_invariants():
    """A point on lo is live in cell 0, a point on hi is dead, NaN is dead.  The box has power-of-two
    extents (inv = 1, 2, 1), so t is exact; on a box whose inv is rounded, t of a point on hi is
    fl(fl(hi - lo) * inv), which the float rule may place just below G (the last cell): there the
    rule as written decides, and the GPU tests compare against it sample by sample."""
    lo, hi, G = (-1.5, -1.0, -2.0), (2.5, 1.0, 2.0), 4
    assert R.inv_of(lo, hi, G).tolist() == [1.0, 2.0, 1.0]
    ones = np.ones((G, G, G), bool)
    d = torch.tensor([[1.0, 0.0, 0.0]])
    zero = torch.zeros(1, 1)

    def live(p, mask=ones):
        return bool(R.classify(torch.tensor([p], dtype=torch.float32), d, zero, lo, hi, G, mask)[0, 0])

    assert live(lo) and live(lo, R.single_cell_mask(G, (0, 0, 0)))          # a point on lo: cell 0
    assert not live(lo, ~R.single_cell_mask(G, (0, 0, 0)))
    for c in range(3):                                                       # a point on hi is dead, per axis
        p = list(lo)
        p[c] = hi[c]
        assert not live(p), c
        p[c] = hi[c] - 0.25 * (hi[c] - lo[c]) / G                            # inside the last cell
        last = [0, 0, 0]
        last[c] = G - 1
        assert live(p, R.single_cell_mask(G, last)), c
        p[c] = float(np.nextafter(np.float32(lo[c]), np.float32(-10)))       # just below lo: t < 0
        assert not live(p), c
        p[c] = float("nan")
        assert not live(p), c
    assert not live(hi) and live((0.0, 0.0, 0.0))
    t = R.cell_coords(torch.tensor([lo], dtype=torch.float32), d, zero, lo, hi, G)
    assert t.dtype == torch.float32 and torch.equal(t, torch.zeros(1, 1, 3))
    # the asymmetric box of the GPU tests: lo still maps to cell 0 exactly, NaN is dead
    lo2, hi2 = (-1.5, -1.3, -1.7), (1.6, 1.9, 1.4)
    z1 = R.classify(torch.tensor([lo2], dtype=torch.float32), d, zero, lo2, hi2, 5, R.single_cell_mask(5, (0, 0, 0)))
    assert bool(z1[0, 0])
    zn = R.classify(torch.tensor([[0.0, float("nan"), 0.0]]), d, zero, lo2, hi2, 5, np.ones((5, 5, 5), bool))
    assert not bool(zn[0, 0])
    # bit layout and dilation
    m = R.single_cell_mask(5, (3, 1, 2))
    idx = (2 * 5 + 1) * 5 + 3
    w = R.pack_bits(m)
    assert w.dtype == np.uint32 and w.size == 4 and w[idx >> 5] == 1 << (idx & 31) and w.sum() == w[idx >> 5]
    assert np.array_equal(R.unpack_bits(w, 5), m)
    assert R.dilate(m).sum() == 27 and R.dilate(m, 2).sum() == 4 * 4 * 5      # clamped: x 1..4, y 0..3 after two steps
    assert R.dilate(R.single_cell_mask(5, (0, 0, 0))).sum() == 8              # clamped at the faces
    lat = np.zeros((4, 4, 4), np.float32)
    lat[3, 0, 1] = 2.0
    assert np.array_equal(R.threshold_mask(lat, 2, 2, 1.0), R.single_cell_mask(2, (0, 0, 1)))
    assert not R.threshold_mask(lat, 2, 2, 2.0).any()                         # strictly greater
    idx_l, n = R.live_list(torch.tensor([[False, True, True], [True, False, False]]))
    assert n == 3 and idx_l.tolist() == [1, 2, 3] and idx_l.dtype == torch.int32
