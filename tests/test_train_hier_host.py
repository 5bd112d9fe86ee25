"""CPU-side checks of training with the hierarchical fine pass (include/nerfmi_train.h "training with
the hierarchical fine pass"): the new C-ABI symbols, the workspace size, the argument
checks (none of which launches anything) and the Python / CLI surface's argument validation."""
import ctypes

import pytest

from nerfmi import _lib

NEW = ("nerf_train_hier_workspace_bytes", "nerf_train_hier_forward", "nerf_train_hier_backward",
       "nerf_sample_importance_src", "nerf_composite_merged_backward")
FAKE = ctypes.c_void_p(0x1000)
BAD_ARG, UNSUPPORTED, WORKSPACE = 1, 3, 4
_V, _I64, _I, _D = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double


def test_new_symbols_are_exported_with_the_documented_signatures():
    lib = _lib.load()
    want = {
        "nerf_train_hier_workspace_bytes": (ctypes.c_size_t, [_I64, _I, _I]),
        "nerf_train_hier_forward": (_I, [_V, _V, _V, _I64, _D, _D, _I, _I, _V, _V, _I, _V, _V, ctypes.c_uint64, _V,
                                         _I64, _V, _V, _V, _V, _V, _V, _V, _V, ctypes.c_size_t, _V]),
        "nerf_train_hier_backward": (_I, [_V, _V, _V, _V, _V, _I64, _I, _I, _D, _V, _I64, ctypes.POINTER(_V), _V, _V,
                                          _V, ctypes.c_size_t, _V]),
        "nerf_sample_importance_src": (_I, [_V, _V, _I64, _I, _I, _V, _V, ctypes.c_uint64, _V, _V, _V, _V]),
        "nerf_composite_merged_backward": (_I, [_V, _V, _V, _V, _V, _V, _V, _V, _I64, _I, _I, _I, _V, _V, _V, _V, _V]),
    }
    assert set(want) == set(NEW)
    for name, (res, args) in want.items():
        assert name in _lib.EXPORTED, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert lib.nerf_abi_version() == 11          # additions only


def test_workspace_bytes():
    lib = _lib.load()
    for B, N, Nf in ((-1, 64, 128), (4, 1, 128), (4, 0, 128), (4, 257, 128), (4, 64, 0), (4, 64, 1025),
                     (1 << 25, 64, 128)):                                   # (B N >= 2^31)
        assert lib.nerf_train_hier_workspace_bytes(B, N, Nf) == 0, (B, N, Nf)
    for N, Nf in ((8, 16), (32, 40), (64, 128), (256, 1024), (2, 1)):
        prev = 0
        for B in (0, 1, 5, 37, 256, 4096):
            got = lib.nerf_train_hier_workspace_bytes(B, N, Nf)
            wc, wf = (lib.nerf_param_grads_workspace_bytes(B * n) for n in (N, Nf))
            # both parts' carves minus one weight-gradient region (the parts share the larger one)
            floor = lib.nerf_train_workspace_bytes(B, N) + lib.nerf_train_workspace_bytes(B, Nf) - min(wc, wf) - 256
            assert got >= floor, (B, N, Nf, got, floor)
            assert got >= prev, (B, N, Nf)
            prev = got
    # beside the two parts: the coarse weights, z_all, merged_src, a second gradient set, a second dapp
    B, N, Nf = 4096, 64, 128
    got = lib.nerf_train_hier_workspace_bytes(B, N, Nf)
    parts = lib.nerf_train_workspace_bytes(B, N) + lib.nerf_train_workspace_bytes(B, Nf) - \
        lib.nerf_param_grads_workspace_bytes(B * N)
    extra = 4 * B * N + 4 * B * (N + Nf) + 2 * B * (N + Nf) + 4 * 534276 + 4 * 32 * B
    assert parts + extra <= got <= parts + extra + 4 * 24 * 64 + 8 * 256, (got, parts, extra)


def _forward(lib, B=4, N=8, Nf=16, packed=FAKE, u_lin=FAKE, coarse_rgb=FAKE, app=None, rows=0, ws=FAKE,
             ws_bytes=1 << 30):
    return lib.nerf_train_hier_forward(packed, FAKE, FAKE, B, 2.0, 6.0, N, Nf, FAKE, u_lin, 1, None, None, 0, app,
                                       rows, FAKE, FAKE, None, None, coarse_rgb, FAKE, None, ws, ws_bytes, None)


def _backward(lib, B=4, N=8, Nf=16, packedT=FAKE, coarse_rgb=FAKE, cw=1.0, app=None, rows=0, grads=None, loss=FAKE,
              ws=ctypes.c_void_p(0x3000), ws_bytes=1 << 30):
    g = (ctypes.c_void_p * 24)(*[0x1000] * 24) if grads is None else grads
    return lib.nerf_train_hier_backward(FAKE, packedT, FAKE, coarse_rgb, FAKE, B, N, Nf, cw, app, rows, g, None, loss,
                                        ws, ws_bytes, None)


def _merged(lib, B=4, N=8, Nf=16, src=FAKE, drgb_f=FAKE):
    return lib.nerf_composite_merged_backward(FAKE, FAKE, FAKE, FAKE, src, FAKE, None, None, B, N, Nf, 0, FAKE, FAKE,
                                              FAKE, drgb_f, None)


def _resample(lib, B=4, N=8, Nf=16, src=FAKE, z_fine=FAKE):
    return lib.nerf_sample_importance_src(FAKE, FAKE, B, N, Nf, FAKE, None, 0, FAKE, z_fine, src, None)


def test_bad_arguments_return_the_documented_code_without_a_launch():
    lib = _lib.load()
    # null pointers -> NERF_ERR_BAD_ARG
    assert _forward(lib, packed=None) == BAD_ARG and b"nerf_train_hier_forward" in lib.nerf_last_error()
    assert _forward(lib, u_lin=None) == BAD_ARG and _forward(lib, coarse_rgb=None) == BAD_ARG
    assert _forward(lib, ws=None) == BAD_ARG and _forward(lib, rows=1, app=None) == BAD_ARG
    assert _backward(lib, packedT=None) == BAD_ARG and b"nerf_train_hier_backward" in lib.nerf_last_error()
    assert _backward(lib, loss=None) == BAD_ARG and _backward(lib, coarse_rgb=None) == BAD_ARG
    assert _backward(lib, ws=None) == BAD_ARG
    assert _backward(lib, grads=(ctypes.c_void_p * 24)(*([0x1000] * 23 + [0]))) == BAD_ARG
    assert _merged(lib, src=None) == BAD_ARG and b"nerf_composite_merged_backward" in lib.nerf_last_error()
    assert _merged(lib, drgb_f=None) == BAD_ARG
    assert _resample(lib, src=None) == BAD_ARG and b"nerf_sample_importance_src" in lib.nerf_last_error()
    assert _resample(lib, z_fine=None) == BAD_ARG
    # negative counts, app_rows other than 0 / 1 / B, a negative loss weight -> NERF_ERR_BAD_ARG
    for fn in (_forward, _backward, _merged, _resample):
        assert fn(lib, B=-1) == BAD_ARG, fn.__name__
    assert _forward(lib, rows=2, app=FAKE) == BAD_ARG and _backward(lib, rows=2, app=FAKE) == BAD_ARG
    assert _backward(lib, cw=-0.5) == BAD_ARG and b"coarse_weight" in lib.nerf_last_error()
    assert _backward(lib, cw=float("nan")) == BAD_ARG
    # N = 1, N > 256, Nf = 0, Nf = 2000 -> NERF_ERR_UNSUPPORTED
    for fn in (_forward, _backward):
        assert fn(lib, N=1) == UNSUPPORTED and b"2..256" in lib.nerf_last_error(), fn.__name__
        assert fn(lib, N=257) == UNSUPPORTED and fn(lib, Nf=0) == UNSUPPORTED, fn.__name__
        assert fn(lib, Nf=2000) == UNSUPPORTED and b"1..1024" in lib.nerf_last_error(), fn.__name__
    for fn in (_merged, _resample):
        assert fn(lib, N=0) == UNSUPPORTED and fn(lib, N=257) == UNSUPPORTED, fn.__name__
        assert fn(lib, Nf=0) == UNSUPPORTED and fn(lib, Nf=2000) == UNSUPPORTED, fn.__name__
    # a short workspace -> NERF_ERR_WORKSPACE
    need = lib.nerf_train_hier_workspace_bytes(4, 8, 16)
    for fn in (_forward, _backward):
        assert fn(lib, ws_bytes=need - 1) == WORKSPACE and b"workspace" in lib.nerf_last_error(), fn.__name__
    # a backward on a workspace no hierarchical forward wrote -> NERF_ERR_BAD_ARG
    assert _backward(lib) == BAD_ARG and b"no nerf_train_hier_forward" in lib.nerf_last_error()
    # empty launches are a no-op
    assert _forward(lib, B=0) == 0 and _backward(lib, B=0) == 0 and _merged(lib, B=0) == 0 and _resample(lib, B=0) == 0


def test_trainer_and_train_nerf_argument_errors():
    import nerfmi
    from nerfmi.train import Trainer, train_nerf
    cfg = nerfmi.Config()
    grid = nerfmi.OccupancyGrid((-1, -1, -1), (1, 1, 1), 4, device="cpu")
    for make in (lambda **kw: Trainer(cfg, **kw), lambda **kw: train_nerf(cfg, None, **kw)):
        with pytest.raises(ValueError, match="hierarchical=True.*occupancy"):
            make(hierarchical=True, occupancy=grid)
        for bad in (0, 1025, -3, 2.5, "128", True):
            with pytest.raises(ValueError, match="n_importance"):
                make(hierarchical=True, n_importance=bad)
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="coarse_loss_weight"):
                make(hierarchical=True, coarse_loss_weight=bad)
        # the fine pass's options without the fine pass
        with pytest.raises(ValueError, match="n_importance needs hierarchical=True"):
            make(n_importance=64)
        with pytest.raises(ValueError, match="coarse_loss_weight needs hierarchical=True"):
            make(coarse_loss_weight=0.5)
    one = nerfmi.Config()
    one.num_samples = 1
    with pytest.raises(ValueError, match="num_samples"):
        Trainer(one, hierarchical=True)


def test_cli_refuses_hierarchical_with_occupancy(capsys):
    import run as cli
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--mode", "train", "--hierarchical", "--occupancy", "32"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--hierarchical" in err and "--occupancy" in err
    # each alone, and the pair in render mode, still parse
    a = cli.parse_args(["--mode", "train", "--hierarchical", "--n_importance", "32"])
    assert a.hierarchical and a.n_importance == 32 and not a.occupancy
    assert cli.parse_args(["--mode", "train", "--occupancy", "32"]).occupancy == 32
    assert cli.parse_args(["--mode", "render", "--hierarchical", "--occupancy", "32"]).hierarchical
