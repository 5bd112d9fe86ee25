"""CPU-side checks of training with an occupancy grid (include/nerfmi_train.h "training with an
occupancy grid"): the new C-ABI symbols, their workspace size and argument checks (none of which
launches anything), and the Python surface's argument validation."""
import ctypes

import pytest
import torch

from nerfmi import _lib

NEW = ("nerf_train_occ_workspace_bytes", "nerf_train_occ_sample", "nerf_train_occ_forward",
       "nerf_train_occ_backward", "nerf_mlp_forward_train_live")
FAKE = ctypes.c_void_p(0x1000)
F3 = ctypes.c_float * 3
BAD_ARG, UNSUPPORTED, WORKSPACE = 1, 3, 4
_V, _I64, _I, _D = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
_F3P = ctypes.POINTER(ctypes.c_float)


def test_new_symbols_are_exported_with_the_documented_signatures():
    lib = _lib.load()
    want = {
        "nerf_train_occ_workspace_bytes": (ctypes.c_size_t, [_I64, _I]),
        "nerf_train_occ_sample": (_I, [_V, _V, _I64, _D, _D, _I, _V, _I, _V, ctypes.c_uint64, _V, _I, _F3P, _F3P, _V,
                                       _V, ctypes.c_size_t, _V]),
        "nerf_train_occ_forward": (_I, [_V, _V, _I64, _I, _I64, _V, _I64, _V, _V, _V, _V, _V, ctypes.c_size_t, _V]),
        "nerf_train_occ_backward": (_I, [_V, _V, _V, _V, _I64, _I, _I64, _V, _I64, ctypes.POINTER(_V), _V, _V, _V,
                                         ctypes.c_size_t, _V]),
        "nerf_mlp_forward_train_live": (_I, [_V, _V, _V, _V, _I64, _I, _V, _V, _V, _I64, _V, _V, _V, _V, _V, _V, _V]),
    }
    assert set(want) == set(NEW)
    for name, (res, args) in want.items():
        assert name in _lib.EXPORTED, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert lib.nerf_abi_version() == 11          # additions only


def test_workspace_bytes():
    lib = _lib.load()
    for B, N in ((-1, 64), (4, 0), (4, 4097), (1 << 28, 64)):
        assert lib.nerf_train_occ_workspace_bytes(B, N) == 0, (B, N)
    for B, N in ((37, 7), (256, 64), (4096, 64)):
        M = B * N
        plain = lib.nerf_train_workspace_bytes(B, N)
        occ = lib.nerf_train_occ_workspace_bytes(B, N)
        # the plain carve, the live list, the classify block counts, the compact sigma, rgb, dsigma, drgb
        extra = 4 * M + 4 * ((M + 255) // 256) + 4 * M * (1 + 3 + 1 + 3)
        assert plain + extra <= occ <= plain + extra + 6 * 256, (B, N)


def _sample(lib, B=4, N=8, G=8, bits=FAKE, count=FAKE, o=FAKE, ws=FAKE, ws_bytes=1 << 30, lo=None):
    lo_, inv = F3(-1, -1, -1), F3(4, 4, 4)
    return lib.nerf_train_occ_sample(o, FAKE, B, 2.0, 6.0, N, FAKE, 1, None, 0, bits, G, lo_ if lo is None else lo[0],
                                     inv, count, ws, ws_bytes, None)


def _forward(lib, B=4, N=8, M_live=5, packed=FAKE, app=None, rows=0, ws=FAKE, ws_bytes=1 << 30):
    return lib.nerf_train_occ_forward(packed, FAKE, B, N, M_live, app, rows, FAKE, FAKE, None, None, ws, ws_bytes,
                                      None)


def _backward(lib, B=4, N=8, M_live=5, packedT=FAKE, rows=0, app=None, grads=None, loss=FAKE, ws_bytes=1 << 30):
    g = (ctypes.c_void_p * 24)(*[0x1000] * 24) if grads is None else grads
    return lib.nerf_train_occ_backward(FAKE, packedT, FAKE, FAKE, B, N, M_live, app, rows, g, None, loss, FAKE,
                                       ws_bytes, None)


def _live(lib, R=4, N=8, M_live=5, live=FAKE, masks=FAKE):
    return lib.nerf_mlp_forward_train_live(FAKE, FAKE, FAKE, FAKE, R, N, FAKE, FAKE, live, M_live, FAKE, FAKE, FAKE,
                                           FAKE, FAKE, masks, None)


def test_bad_arguments_return_the_documented_code_without_a_launch():
    lib = _lib.load()
    assert lib.nerf_get_mlp_arith() == 1                                       # f16x3, the default
    # null pointers -> NERF_ERR_BAD_ARG
    assert _sample(lib, bits=None) == BAD_ARG and b"nerf_train_occ_sample" in lib.nerf_last_error()
    assert _sample(lib, count=None) == BAD_ARG and _sample(lib, o=None) == BAD_ARG and _sample(lib, ws=None) == BAD_ARG
    assert _forward(lib, packed=None) == BAD_ARG and b"nerf_train_occ_forward" in lib.nerf_last_error()
    assert _forward(lib, ws=None) == BAD_ARG and _forward(lib, rows=1, app=None) == BAD_ARG
    assert _backward(lib, packedT=None) == BAD_ARG and b"nerf_train_occ_backward" in lib.nerf_last_error()
    assert _backward(lib, loss=None) == BAD_ARG
    assert _backward(lib, grads=(ctypes.c_void_p * 24)(*([0x1000] * 23 + [0]))) == BAD_ARG
    assert _live(lib, live=None) == BAD_ARG and b"nerf_mlp_forward_train_live" in lib.nerf_last_error()
    assert _live(lib, masks=None) == BAD_ARG
    # negative counts and M_live > B N -> NERF_ERR_BAD_ARG
    for fn in (_sample, _forward, _backward):
        assert fn(lib, B=-1) == BAD_ARG, fn.__name__
    assert _live(lib, R=-1) == BAD_ARG
    for fn in (_forward, _backward, _live):
        assert fn(lib, M_live=-1) == BAD_ARG, fn.__name__
        assert fn(lib, M_live=33) == BAD_ARG and b"M_live=33" in lib.nerf_last_error(), fn.__name__
    assert _forward(lib, rows=-1) == BAD_ARG and _backward(lib, rows=-1) == BAD_ARG
    # G outside 1..1024, N outside 1..4096, per-ray appearance rows -> NERF_ERR_UNSUPPORTED
    for G in (0, 1025):
        assert _sample(lib, G=G) == UNSUPPORTED and b"1..1024" in lib.nerf_last_error(), G
    for fn in (_sample, _forward, _backward, _live):
        assert fn(lib, N=0) == UNSUPPORTED and fn(lib, N=4097) == UNSUPPORTED, fn.__name__
    assert _forward(lib, rows=4, app=FAKE) == UNSUPPORTED and b"app_rows" in lib.nerf_last_error()
    assert _backward(lib, rows=4, app=FAKE) == UNSUPPORTED
    # a short workspace -> NERF_ERR_WORKSPACE
    need = lib.nerf_train_occ_workspace_bytes(4, 8)
    for fn in (_sample, _forward, _backward):
        assert fn(lib, ws_bytes=need - 1) == WORKSPACE and b"workspace" in lib.nerf_last_error(), fn.__name__
    # a backward on a workspace no occupancy forward wrote -> NERF_ERR_BAD_ARG
    assert _backward(lib) == BAD_ARG and b"nerf_train_occ_forward" in lib.nerf_last_error()
    # empty launches are a no-op
    assert _forward(lib, B=0, M_live=0) == 0 and _backward(lib, B=0, M_live=0) == 0 and _live(lib, M_live=0) == 0


def test_f32_arithmetic_is_unsupported():
    lib = _lib.load()
    prev = _lib.set_mlp_arith("f32")
    try:
        for rc in (_forward(lib), _backward(lib), _live(lib)):
            assert rc == UNSUPPORTED and b"f16x3" in lib.nerf_last_error()
    finally:
        _lib.set_mlp_arith(prev)


def test_trainer_and_train_nerf_reject_a_non_grid():
    import nerfmi
    from nerfmi.train import Trainer, train_nerf
    cfg = nerfmi.Config()
    for bad in (torch.zeros(4), 16, "grid"):
        with pytest.raises(ValueError, match="OccupancyGrid"):
            Trainer(cfg, occupancy=bad)
        with pytest.raises(ValueError, match="OccupancyGrid"):
            train_nerf(cfg, None, occupancy=bad)
    g = nerfmi.OccupancyGrid((-1, -1, -1), (1, 1, 1), 4, device="cpu")
    for bad in (dict(evry=3), 5, dict(every=0), dict(supersample=0)):
        with pytest.raises(ValueError, match="occupancy_refresh"):
            Trainer(cfg, occupancy=g, occupancy_refresh=bad)
    with pytest.raises(ValueError, match="occupancy_refresh"):
        train_nerf(cfg, None, occupancy_refresh={})            # a refresh without a grid
