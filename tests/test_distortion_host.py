"""CPU-side checks of the distortion loss (include/nerfmi_train.h "distortion"): the float64
definition of tests/distortion_cases.py against torch's own autograd and against the O(T) closed form the
kernel uses, the new C-ABI symbols and their refusals (none of which launches anything), and the Python
and CLI argument validation."""
import ctypes
import os
import re
import sys

import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests"))
import distortion_cases as DC   # noqa: E402

from nerfmi import _lib   # noqa: E402

NEW = ("nerf_distortion", "nerf_composite_backward_grad_w", "nerf_composite_merged_backward_w",
       "nerf_train_backward_dist", "nerf_train_occ_backward_dist", "nerf_train_hier_backward_dist")
FAKE = ctypes.c_void_p(0x1000)
BAD_ARG, UNSUPPORTED = 1, 3
NAN, INF = float("nan"), float("inf")
NEAR, FAR = 2.0, 6.0
_V, _I64, _I, _D, _F = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_float


# ----------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("T", [2, 5, 64, 65, 100])
def test_definition_gradient_is_autograd_of_its_loss(T):
    w, z, keep = DC.profile_weights(67, T)                 # every profile, the descending pair included
    g = torch.Generator().manual_seed(T)
    w = (w.double() + 0.01 * torch.rand(67, T, generator=g, dtype=torch.float64)).requires_grad_(True)
    loss = DC.loss_autograd(w, z, NEAR, FAR)
    loss.sum().backward()
    l_def, g_def = DC.definition(w.detach(), z, NEAR, FAR)
    assert torch.allclose(l_def, loss.detach(), rtol=1e-12, atol=1e-15)
    assert torch.allclose(g_def, w.grad, rtol=1e-12, atol=1e-15)
    assert bool((l_def[keep] > 0).all())                   # (a negative interval can make the descending ray's negative)


def test_definition_edge_cases():
    z = torch.sort(torch.rand(3, 9) * 4 + 2, dim=-1).values
    l0, g0 = DC.definition(torch.zeros(3, 9), z, NEAR, FAR)
    assert not bool(l0.any()) and not bool(g0.any())                      # zero weights: exact zeros
    l1, g1 = DC.definition(torch.rand(3, 1), z[:, :1], NEAR, FAR)
    assert not bool(l1.any()) and not bool(g1.any()) and g1.shape == (3, 1)   # T = 1
    # one weight of 1 on sample k: only the sample's own width is left, delta_k / (3 (far - near))
    w = torch.zeros(3, 9)
    w[:, 4] = 1.0
    l2, _ = DC.definition(w, z, NEAR, FAR)
    assert torch.allclose(l2, (z[:, 5] - z[:, 4]).double() / 3.0 / (FAR - NEAR), rtol=1e-12)
    # two lumps cost more than one: the loss is what tells a floater from a surface
    w2 = torch.zeros(3, 9)
    w2[:, 1], w2[:, 7] = 0.5, 0.5
    assert bool((DC.definition(w2, z, NEAR, FAR)[0] > l2).all())


@pytest.mark.parametrize("T", [2, 5, 64, 65, 100, 259, 1280, 4096])
def test_closed_form_equals_the_definition(T):
    """The O(T) closed form in float64, rounded to float as the kernel rounds its outputs, against the
    O(T^2) definition on the sorted rays of ray_profiles(67, T): within 2^-23 |ref| + T 2^-48 S."""
    w, z, keep = DC.profile_weights(67, T)
    w, z = w[keep], z[keep]
    l_ref, g_ref = DC.definition(w, z, NEAR, FAR)
    l_cf, g_cf = DC.closed_form(w, z, NEAR, FAR)
    S = DC.ray_scale(w, z, NEAR, FAR)
    worst = {}
    for name, cf, ref in (("l", l_cf, l_ref), ("g", g_cf, g_ref)):
        b = DC.bound(ref, T, S)
        err32, err64 = (cf.float().double() - ref).abs(), (cf - ref).abs()
        tiny = torch.finfo(torch.float64).tiny
        worst[name] = (float((err32 / b.clamp_min(tiny)).max()), float((err64 / (T * 2.0 ** -48 * (S if ref.dim() == 1 else S[:, None])).clamp_min(tiny)).max()))
        assert bool((err32 <= b).all()), (name, T, worst[name])
    print(f"T={T}: worst ratio to the bound, rounded to float (double part alone): "
          f"l {worst['l'][0]:.3f} ({worst['l'][1]:.3f})  g {worst['g'][0]:.3f} ({worst['g'][1]:.3f})")


# ------------------------------------------------------------------------------- the C ABI
def test_new_symbols_are_declared_and_exported():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "nerfmi_train.h")).read()
    loss = [_V, _V, _I64, _D, _V]                          # alpha, bg, bg_rows, acc_weight, rgb_final
    dist = [_D, _D, _D]                                    # dist_weight, near, far
    want = {
        "nerf_distortion": [_V, _V, _I64, _I, _D, _D, _D, _V, _V, _V],
        "nerf_composite_backward_grad_w": [_V, _V, _V, _V, _V, _I64, _I, _V, _V, _V, _F, _V, _V],
        "nerf_composite_merged_backward_w": [_V, _V, _V, _V, _V, _V, _V, _V, _I64, _I, _I, _I, _V, _V, _V, _V, _V, _F,
                                             _V, _V],
        "nerf_train_backward_dist": [_V, _V, _V, _V, _I64, _I, _V, _I64, ctypes.POINTER(_V), _V, _V, _V,
                                     ctypes.c_size_t] + loss + dist + [_V],
        "nerf_train_occ_backward_dist": [_V, _V, _V, _V, _I64, _I, _I64, _V, _I64, ctypes.POINTER(_V), _V, _V, _V,
                                         ctypes.c_size_t] + loss + dist + [_V],
        "nerf_train_hier_backward_dist": [_V, _V, _V, _V, _V, _I64, _I, _I, _D, _V, _I64, ctypes.POINTER(_V), _V, _V,
                                          _V, ctypes.c_size_t] + loss + [_V] + dist + [_V],
    }
    assert set(want) == set(NEW)
    for name, args in want.items():
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.EXPORTED, name
        fn = getattr(lib, name)
        assert fn.restype is _I and list(fn.argtypes) == args, name
    # each entry is its original's argument list (up to the stream) with the additions behind it
    for new, old in (("nerf_train_backward_dist", "nerf_train_backward_bg"),
                     ("nerf_train_occ_backward_dist", "nerf_train_occ_backward_bg"),
                     ("nerf_train_hier_backward_dist", "nerf_train_hier_backward_bg"),
                     ("nerf_composite_backward_grad_w", "nerf_composite_backward_grad_acc"),
                     ("nerf_composite_merged_backward_w", "nerf_composite_merged_backward_acc")):
        o = list(getattr(lib, old).argtypes)
        assert list(getattr(lib, new).argtypes)[:len(o) - 1] == o[:-1], new
    assert lib.nerf_abi_version() == _lib.ABI_VERSION == 11          # additions only
    assert not [s for s in _lib.EXPORTED if s.endswith("_dist_workspace_bytes")]


def test_scratch_fits_the_gradient_rows():
    """The head's scratch with a distortion term: 7 x roundup64(B) + 2 x roundup64(B T) floats in the
    sample set's gradient rows (the fine part: T = N + Nf over the B Nf fine rows)."""
    up = lambda n: (n + 63) // 64 * 64   # noqa: E731
    for B, rows_per_ray, T in ((1, 1, 1), (3, 1, 1), (4096, 64, 64), (1, 1, 257), (5, 1, 257), (4096, 128, 192),
                               (100000, 2, 2), (1, 4096, 4096)):
        assert 7 * up(B) + 2 * up(B * T) <= _lib.tile_rows(B * rows_per_ray) * _lib.GRAD_ROW, (B, rows_per_ray, T)


def _train_dist(lib, kind, B=4, dw=0.0, near=NEAR, far=FAR, packedT=None, aw=0.0):
    g = (ctypes.c_void_p * 24)(*[0x1000] * 24)
    tail = [FAKE, FAKE, 1 << 30, None, None, 0, aw, None]
    if kind == "dense":
        return lib.nerf_train_backward_dist(FAKE, packedT, FAKE, FAKE, B, 8, None, 0, g, None, *tail, dw, near, far, None)
    if kind == "occ":
        return lib.nerf_train_occ_backward_dist(FAKE, packedT, FAKE, FAKE, B, 8, 0, None, 0, g, None, *tail, dw, near, far,
                                                None)
    return lib.nerf_train_hier_backward_dist(FAKE, packedT, FAKE, FAKE, FAKE, B, 8, 16, 1.0, None, 0, g, None, *tail,
                                             None, dw, near, far, None)


def test_argument_refusals():
    lib = _lib.load()
    for kind, name in (("dense", b"nerf_train_backward_dist"), ("occ", b"nerf_train_occ_backward_dist"),
                       ("hier", b"nerf_train_hier_backward_dist")):
        if kind == "occ" and _lib.get_mlp_arith() != "f16x3":
            continue
        for dw in (-0.5, NAN, INF):
            assert _train_dist(lib, kind, dw=dw) == BAD_ARG and b"dist_weight" in lib.nerf_last_error(), (kind, dw)
            assert name in lib.nerf_last_error()
        for near, far in ((6.0, 2.0), (2.0, 2.0), (NAN, 6.0), (2.0, INF), (-INF, 6.0)):
            assert _train_dist(lib, kind, dw=0.1, near=near, far=far) == BAD_ARG, (kind, near, far)
            assert b"far" in lib.nerf_last_error(), (kind, near, far)
            # with the weight at 0 the bounds are not looked at: the original's checks come next (a null packedT)
            assert _train_dist(lib, kind, dw=0.0, near=near, far=far) == BAD_ARG
            assert b"null pointer" in lib.nerf_last_error(), (kind, near, far)
        # the original's refusals hold: acc_weight, then the pointers, then the workspace kind
        assert _train_dist(lib, kind, dw=0.1, aw=-1.0) == BAD_ARG and b"acc_weight" in lib.nerf_last_error()
        assert _train_dist(lib, kind, dw=0.1) == BAD_ARG and b"null pointer" in lib.nerf_last_error(), kind
        assert _train_dist(lib, kind, dw=0.1, packedT=FAKE) == BAD_ARG
        assert b"wrote this workspace" in lib.nerf_last_error(), kind
        assert _train_dist(lib, kind, B=0, dw=0.1, packedT=FAKE) == 0
    d = lib.nerf_distortion
    assert d(FAKE, FAKE, -1, 8, NEAR, FAR, 1.0, FAKE, FAKE, None) == BAD_ARG
    for T in (0, 4097):
        assert d(FAKE, FAKE, 4, T, NEAR, FAR, 1.0, FAKE, FAKE, None) == UNSUPPORTED
        assert b"nerf_distortion" in lib.nerf_last_error()
    for near, far in ((6.0, 2.0), (2.0, 2.0), (NAN, 6.0), (2.0, INF)):
        assert d(FAKE, FAKE, 4, 8, near, far, 1.0, FAKE, FAKE, None) == BAD_ARG and b"far" in lib.nerf_last_error()
    for scale in (NAN, INF):
        assert d(FAKE, FAKE, 4, 8, NEAR, FAR, scale, FAKE, FAKE, None) == BAD_ARG and b"scale" in lib.nerf_last_error()
    assert d(None, FAKE, 4, 8, NEAR, FAR, 1.0, FAKE, FAKE, None) == BAD_ARG and b"null pointer" in lib.nerf_last_error()
    assert d(None, None, 0, 8, NEAR, FAR, 1.0, None, None, None) == 0
    assert d(FAKE, FAKE, 4, 8, NEAR, FAR, 1.0, None, None, None) == 0          # nothing asked for: no launch
    w = lib.nerf_composite_backward_grad_w
    assert w(None, None, None, None, None, 4, 64, None, None, None, NAN, None, None) == BAD_ARG
    assert b"nerf_composite_backward_grad_w" in lib.nerf_last_error()
    assert w(None, None, None, None, None, 4, 0, None, None, None, NAN, None, None) == UNSUPPORTED
    assert w(None, None, None, None, None, 0, 64, None, None, None, NAN, None, None) == 0
    m = lib.nerf_composite_merged_backward_w
    args = [FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, None]
    outs = [0, FAKE, FAKE, FAKE, FAKE, None, NAN, None, None]
    assert m(FAKE, FAKE, FAKE, FAKE, None, FAKE, None, None, 4, 8, 16, *outs) == BAD_ARG
    assert m(*args, 4, 257, 16, *outs) == UNSUPPORTED and m(*args, 0, 8, 16, *outs) == 0


# ------------------------------------------------------------------------- Python and the CLI
def test_python_argument_errors():
    import nerfmi
    from nerfmi.distortion import _check_distortion_inputs
    from nerfmi.train import Trainer, train_nerf
    cfg = nerfmi.Config()
    for make in (lambda **kw: Trainer(cfg, **kw), lambda **kw: train_nerf(cfg, None, **kw)):
        for bad in (-0.1, NAN, INF):
            with pytest.raises(ValueError, match="distortion_weight"):
                make(distortion_weight=bad)
    assert "distortion_loss" in nerfmi.__all__
    w, z = torch.rand(5, 8), torch.rand(5, 8)
    got, B, T, near, far = _check_distortion_inputs(w[..., None], z, 2, 6)     # extras['weights'] is (B,T,1)
    assert got.shape == (5, 8) and (B, T, near, far) == (5, 8, 2.0, 6.0)
    for bad_w, bad_z in ((w, z[:, :7]), (w[0], z[0]), (torch.rand(5, 8, 2), z), (torch.rand(5, 0), torch.rand(5, 0)),
                         (torch.rand(1, 4097), torch.rand(1, 4097))):
        with pytest.raises(ValueError, match="distortion_loss"):
            nerfmi.distortion_loss(bad_w, bad_z, 2.0, 6.0)
    for near, far in ((6.0, 2.0), (2.0, 2.0), (NAN, 6.0), (2.0, INF)):
        with pytest.raises(ValueError, match="far"):
            nerfmi.distortion_loss(w, z, near, far)


def test_cli_option(capsys):
    import run as cli
    a = cli.parse_args(["--mode", "train", "--distortion_weight", "0.01", "--hierarchical"])
    assert a.distortion_weight == 0.01
    assert cli.parse_args(["--mode", "train"]).distortion_weight == 0.0
    assert cli.parse_args(["--mode", "render", "--distortion_weight", "0"]).distortion_weight == 0.0
    for argv, word in ((["--mode", "train", "--distortion_weight", "-1"], "--distortion_weight"),
                       (["--mode", "train", "--distortion_weight", "nan"], "--distortion_weight"),
                       (["--mode", "render", "--distortion_weight", "0.1"], "--mode train")):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(argv)
        assert e.value.code == 2, argv
        assert word in capsys.readouterr().err, argv
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "--distortion_weight" in readme
