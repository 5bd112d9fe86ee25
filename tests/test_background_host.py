"""CPU-side checks of the opacity map and background feature (include/nerfmi.h "opacity map and
background", include/nerfmi_train.h "training with a background"): the new C-ABI symbols
and their signatures, the argument refusals (none of which launches anything), the unchanged workspace
sizes, the Python and CLI argument validation, and train_nerf handing the dataset's alpha channel to the
trainer."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from nerfmi import _lib

NEW = ("nerf_composite_bg", "nerf_render_rays_bg", "nerf_render_rays_occ_bg", "nerf_train_backward_bg",
       "nerf_train_occ_backward_bg", "nerf_train_hier_backward_bg", "nerf_composite_backward_grad_acc",
       "nerf_composite_merged_backward_acc")
FAKE = ctypes.c_void_p(0x1000)
BAD_ARG, UNSUPPORTED = 1, 3
NAN = float("nan")
_V, _I64, _I, _D, _F = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_float
_FP = ctypes.POINTER(ctypes.c_float)


def test_new_symbols_are_exported_with_the_documented_signatures():
    lib = _lib.load()
    render = [_V, _V, _V, _I64, _D, _D, _I, _I, _V, _V, _I, _V, _V, ctypes.c_uint64, _I64, _V, _I64]
    outs = [_V, _V, _V, _V, _V, _V, _V, ctypes.c_size_t]
    bg = [_V, _I64, _F, _V, _V, _V]                       # bg, bg_rows, bd, acc_map, coarse_acc, stream
    loss = [_V, _V, _I64, _D, _V]                         # alpha, bg, bg_rows, acc_weight, rgb_final
    want = {
        "nerf_composite_bg": [_V, _V, _V, _I64, _I, _V, _V, _V, _V, _I64, _F, _V, _V],
        "nerf_render_rays_bg": render + outs + bg,
        "nerf_render_rays_occ_bg": render + [_V, _I, _FP, _FP] + outs + bg,
        "nerf_train_backward_bg": [_V, _V, _V, _V, _I64, _I, _V, _I64, ctypes.POINTER(_V), _V, _V, _V,
                                   ctypes.c_size_t] + loss + [_V],
        "nerf_train_occ_backward_bg": [_V, _V, _V, _V, _I64, _I, _I64, _V, _I64, ctypes.POINTER(_V), _V, _V, _V,
                                       ctypes.c_size_t] + loss + [_V],
        "nerf_train_hier_backward_bg": [_V, _V, _V, _V, _V, _I64, _I, _I, _D, _V, _I64, ctypes.POINTER(_V), _V, _V, _V,
                                        ctypes.c_size_t] + loss + [_V, _V],
        "nerf_composite_backward_grad_acc": [_V, _V, _V, _V, _V, _I64, _I, _V, _V, _V, _F, _V],
        "nerf_composite_merged_backward_acc": [_V, _V, _V, _V, _V, _V, _V, _V, _I64, _I, _I, _I, _V, _V, _V, _V, _V, _F,
                                               _V],
    }
    assert set(want) == set(NEW)
    for name, args in want.items():
        assert name in _lib.EXPORTED, name
        fn = getattr(lib, name)
        assert fn.restype is _I and list(fn.argtypes) == args, name
    # the originals' argument lists are prefixes (up to the stream) of the new entries'
    for new, old in (("nerf_composite_bg", "nerf_composite"), ("nerf_render_rays_bg", "nerf_render_rays"),
                     ("nerf_render_rays_occ_bg", "nerf_render_rays_occ"), ("nerf_train_backward_bg", "nerf_train_backward"),
                     ("nerf_train_occ_backward_bg", "nerf_train_occ_backward"),
                     ("nerf_train_hier_backward_bg", "nerf_train_hier_backward"),
                     ("nerf_composite_backward_grad_acc", "nerf_composite_backward_grad"),
                     ("nerf_composite_merged_backward_acc", "nerf_composite_merged_backward")):
        o = list(getattr(lib, old).argtypes)
        assert list(getattr(lib, new).argtypes)[:len(o) - 1] == o[:-1], new
    assert lib.nerf_abi_version() == _lib.ABI_VERSION == 11          # additions only


def test_workspace_sizes_are_unchanged():
    """The _bg backwards keep their scratch in the gradient rows: no sizer was added and the committed
    sizes hold (tests/golden/host_workspace_bytes.json is checked by its own test)."""
    assert not [s for s in _lib.EXPORTED if s.endswith("_bg_workspace_bytes")]
    lib = _lib.load()
    # the scratch is 6 x B floats rounded up to 64; the smallest gradient-row region is 32 rows
    for B, N in ((1, 1), (3, 1), (4096, 1), (100000, 2)):
        rows = _lib.tile_rows(B * N) * _lib.GRAD_ROW
        assert 6 * ((B + 63) // 64 * 64) <= rows, (B, N)
        assert lib.nerf_train_workspace_bytes(B, N) > 4 * rows


def _composite_bg(lib, B=4, N=8, bg=FAKE, rows=1, bd=NAN, rgb=FAKE):
    return lib.nerf_composite_bg(rgb, FAKE, FAKE, B, N, FAKE, FAKE, None, bg, rows, bd, None, None)


def _render_bg(lib, occ=False, B=4, bg=FAKE, rows=1, packed=None):
    head = [packed, FAKE, FAKE, B, 2.0, 6.0, 8, 0, FAKE, None, 1, None, None, 0, 0, None, 0]
    tail = [FAKE, FAKE, None, None, None, None, FAKE, 1 << 30, bg, rows, NAN, None, None, None]
    if occ:
        lo = (ctypes.c_float * 3)(-1, -1, -1)
        return lib.nerf_render_rays_occ_bg(*head, FAKE, 4, lo, lo, *tail)
    return lib.nerf_render_rays_bg(*head, *tail)


def _train_bg(lib, kind, B=4, alpha=None, bg=None, rows=0, aw=0.0, packedT=None):
    g = (ctypes.c_void_p * 24)(*[0x1000] * 24)
    tail = [FAKE, FAKE, 1 << 30, alpha, bg, rows, aw, None]
    if kind == "dense":
        return lib.nerf_train_backward_bg(FAKE, packedT, FAKE, FAKE, B, 8, None, 0, g, None, *tail, None)
    if kind == "occ":
        return lib.nerf_train_occ_backward_bg(FAKE, packedT, FAKE, FAKE, B, 8, 0, None, 0, g, None, *tail, None)
    return lib.nerf_train_hier_backward_bg(FAKE, packedT, FAKE, FAKE, FAKE, B, 8, 16, 1.0, None, 0, g, None, *tail, None,
                                           None)


def test_argument_refusals():
    lib = _lib.load()
    # bg_rows outside {0, 1, B}; a null bg with bg_rows > 0
    for rows in (2, 3, -1):
        assert _composite_bg(lib, rows=rows) == BAD_ARG and b"bg_rows" in lib.nerf_last_error()
        for occ in (False, True):
            assert _render_bg(lib, occ, rows=rows) == BAD_ARG and b"bg_rows" in lib.nerf_last_error()
    assert _composite_bg(lib, bg=None) == BAD_ARG and b"null bg" in lib.nerf_last_error()
    assert b"nerf_composite_bg" in lib.nerf_last_error()
    for occ, name in ((False, b"nerf_render_rays_bg"), (True, b"nerf_render_rays_occ_bg")):
        assert _render_bg(lib, occ, bg=None) == BAD_ARG and b"null bg" in lib.nerf_last_error()
        assert name in lib.nerf_last_error()
        # accepted backgrounds reach the original checks (a null packed pointer here)
        for rows in (0, 1, 4):
            assert _render_bg(lib, occ, rows=rows) == BAD_ARG and b"null pointer" in lib.nerf_last_error()
        assert _render_bg(lib, occ, B=0) == 0
    # the originals' refusals still come first where they did
    assert _composite_bg(lib, N=5000) == UNSUPPORTED and _composite_bg(lib, B=-1) == BAD_ARG
    assert _composite_bg(lib, rgb=None) == BAD_ARG and b"null pointer" in lib.nerf_last_error()
    assert _composite_bg(lib, B=0) == 0
    for kind, name in (("dense", b"nerf_train_backward_bg"), ("occ", b"nerf_train_occ_backward_bg"),
                       ("hier", b"nerf_train_hier_backward_bg")):
        for rows in (2, -1):
            assert _train_bg(lib, kind, bg=FAKE, rows=rows) == BAD_ARG and b"bg_rows" in lib.nerf_last_error(), kind
        assert _train_bg(lib, kind, rows=1) == BAD_ARG and b"null bg" in lib.nerf_last_error(), kind
        for aw in (-0.5, NAN, float("inf")):
            assert _train_bg(lib, kind, aw=aw) == BAD_ARG and b"acc_weight" in lib.nerf_last_error(), (kind, aw)
        assert name in lib.nerf_last_error()
        # accepted options reach the original checks (a null packedT here), then the workspace-kind refusal
        assert _train_bg(lib, kind, alpha=FAKE, bg=FAKE, rows=4, aw=0.1) == BAD_ARG
        assert b"null pointer" in lib.nerf_last_error(), kind
        if kind != "occ" or _lib.get_mlp_arith() == "f16x3":
            assert _train_bg(lib, kind, alpha=FAKE, bg=FAKE, rows=1, aw=0.1, packedT=FAKE) == BAD_ARG
            assert b"wrote this workspace" in lib.nerf_last_error(), kind
        assert _train_bg(lib, kind, B=0, packedT=FAKE) == 0
    # the stage entries
    assert lib.nerf_composite_backward_grad_acc(None, None, None, None, None, 4, 64, None, None, None, NAN, None) == 1
    assert b"nerf_composite_backward_grad_acc" in lib.nerf_last_error()
    assert lib.nerf_composite_backward_grad_acc(None, None, None, None, None, 4, 0, None, None, None, NAN, None) == 3
    assert lib.nerf_composite_backward_grad_acc(None, None, None, None, None, 0, 64, None, None, None, NAN, None) == 0
    m = lib.nerf_composite_merged_backward_acc
    assert m(FAKE, FAKE, FAKE, FAKE, None, FAKE, None, None, 4, 8, 16, 0, FAKE, FAKE, FAKE, FAKE, None, NAN, None) == 1
    assert m(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, None, 4, 257, 16, 0, FAKE, FAKE, FAKE, FAKE, None, NAN, None) == 3
    assert m(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, None, 0, 8, 16, 0, FAKE, FAKE, FAKE, FAKE, None, NAN, None) == 0


def test_python_argument_errors():
    import nerfmi
    from nerfmi.render import background_rows
    from nerfmi.train import Trainer, train_nerf
    cfg = nerfmi.Config()
    for make in (lambda **kw: Trainer(cfg, **kw), lambda **kw: train_nerf(cfg, None, **kw)):
        for bad in ("white", (1.0, 0.0), (1.0, 0.0, NAN), 1.0, ("a", "b", "c"), (0, 0, 0, 0)):
            with pytest.raises(ValueError, match="background"):
                make(background=bad)
        for bad in (-0.1, NAN, float("inf")):
            with pytest.raises(ValueError, match="acc_weight"):
                make(acc_weight=bad)
    bg, rows = background_rows((0.25, 0.5, 1.0), 7, "cpu")
    assert rows == 1 and bg.shape == (1, 3) and bg.dtype == torch.float32
    bg, rows = background_rows(torch.rand(7, 3, dtype=torch.float64), 7, "cpu")
    assert rows == 7 and bg.shape == (7, 3) and bg.dtype == torch.float32 and bg.is_contiguous()
    assert background_rows(None, 7, "cpu") == (None, 0)
    with pytest.raises(ValueError, match="background"):
        background_rows(torch.rand(5, 3), 7, "cpu")
    model = nerfmi.NeRF(cfg)
    o = torch.zeros(4, 3)
    for kw in (dict(staged=True), dict(timing=[])):
        with pytest.raises(ValueError, match="single-call"):
            nerfmi.volume_render(model, o, o, 2.0, 6.0, 8, 0, return_acc=True, **kw)


def test_cli_options(capsys):
    import run as cli
    a = cli.parse_args(["--mode", "render", "--background", "1", "0.5", "0", "--background_depth", "far", "--save_acc"])
    assert a.background == (1.0, 0.5, 0.0) and a.background_depth == "far" and a.save_acc and a.acc_weight == 0.0
    a = cli.parse_args(["--mode", "render", "--background_depth", "7.5"])
    assert a.background is None and a.background_depth == 7.5 and not a.save_acc
    assert cli.parse_args(["--mode", "render", "--background_depth", "0"]).background_depth == 0.0
    a = cli.parse_args(["--mode", "train", "--background", "random", "--acc_weight", "0.01", "--hierarchical"])
    assert a.background == "random" and a.acc_weight == 0.01
    a = cli.parse_args(["--mode", "train", "--background", "1", "1", "1", "--occupancy", "32"])
    assert a.background == (1.0, 1.0, 1.0)
    d = cli.parse_args(["--mode", "render"])
    assert d.background is None and d.background_depth is None and d.acc_weight == 0.0 and not d.save_acc
    for argv, word in ((["--mode", "render", "--background", "random"], "random"),
                       (["--mode", "render", "--background", "1", "0"], "three floats"),
                       (["--mode", "train", "--background", "red", "0", "0"], "three floats"),
                       (["--mode", "train", "--background", "nan", "0", "0"], "three floats"),
                       (["--mode", "render", "--background_depth", "near"], "--background_depth"),
                       (["--mode", "render", "--background_depth", "inf"], "--background_depth"),
                       (["--mode", "train", "--acc_weight", "-1"], "--acc_weight"),
                       (["--mode", "train", "--background_depth", "far"], "render modes"),
                       (["--mode", "train", "--save_acc"], "render modes"),
                       (["--mode", "render", "--acc_weight", "0.1"], "--mode train")):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(argv)
        assert e.value.code == 2, argv
        assert word in capsys.readouterr().err, argv


def test_frames_carry_the_opacity_map():
    """render_frames_sharded(with_acc=True) gathers a fifth column like the depth (virtual shards, CPU)."""
    from nerfmi import frames
    H, W, n = 5, 7, 2

    def ray_fn(f, row0, nrows):
        idx = (f * H * W + row0 * W + torch.arange(nrows * W)).float()
        return idx[:, None].expand(-1, 3).clone(), idx[:, None].expand(-1, 3).clone()

    def render_fn(o, d, offset):
        assert float(o[0, 0]) == offset
        return o / 100.0, o[:, :1] + 0.5, o[:, :1] * 2.0

    rgb, depth, acc = frames.render_frames_sharded(ray_fn, render_fn, H, W, n, virtual_shards=3, with_acc=True)
    idx = torch.arange(n * H * W).float().reshape(n, H, W)
    assert torch.equal(depth, idx + 0.5) and torch.equal(acc, idx * 2.0) and torch.equal(rgb[..., 0], idx / 100.0)
    rgb2, depth2 = frames.render_frames_sharded(ray_fn, lambda o, d, s: render_fn(o, d, s)[:2], H, W, n, virtual_shards=3)
    assert torch.equal(rgb2, rgb) and torch.equal(depth2, depth)


class _StubTrainer:
    """Records what train_nerf hands to a trainer (no device)."""
    made = []

    def __init__(self, config, **kw):
        self.kw, self.steps_seen = kw, []
        self.rank, self.lr, self.hierarchical, self.n_importance = 0, 1e-3, False, None
        self.loss_parts = torch.tensor([0.25, 0.5])
        self.loss_form = "_bg" if "background" in kw else ""      # as Trainer decides it from its arguments
        self.model = object()
        _StubTrainer.made.append(self)

    def step(self, rays_o, rays_d, target, app_idx=None, **kw):
        self.steps_seen.append((target.clone(), kw))
        return torch.tensor(0.3)

    def checkpoint(self, loss, psnr, iteration):
        return {"loss": loss, "iteration": iteration}


def _write_scene(root, n=2, hw=6):
    from PIL import Image
    scene = os.path.join(root, "toy")
    os.makedirs(os.path.join(scene, "train"))
    rng = np.random.RandomState(0)
    frames, images = [], []
    for i in range(n):
        img = rng.randint(0, 256, size=(hw, hw, 4), dtype=np.uint8)
        img[0, 0, 3], img[0, 1, 3] = 0, 255
        Image.fromarray(img, mode="RGBA").save(os.path.join(scene, "train", f"r_{i}.png"))
        images.append(img)
        frames.append({"file_path": f"./train/r_{i}", "transform_matrix": np.eye(4).tolist()})
    with open(os.path.join(scene, "transforms_train.json"), "w") as f:
        json.dump({"camera_angle_x": 0.69, "frames": frames}, f)
    return images


def test_train_nerf_passes_the_alpha_channel(tmp_path, monkeypatch):
    import nerfmi
    from nerfmi.dataset import NeRFDataset
    from nerfmi.train import train_nerf
    images = _write_scene(str(tmp_path))
    cfg = nerfmi.Config()
    cfg.dataset_path, cfg.scene, cfg.batch_size = str(tmp_path), "toy", 9
    ds = NeRFDataset(cfg)
    # the rays themselves do not matter here (ray generation runs on the GPU): zeros on the CPU
    monkeypatch.setattr(NeRFDataset, "_rays", lambda self, idx: (torch.zeros(self.H * self.W, 3),) * 2)
    alphas = {i: torch.from_numpy(im[..., 3].reshape(-1).astype(np.float32) / 255) for i, im in enumerate(images)}
    _StubTrainer.made.clear()
    np.random.seed(0)
    train_nerf(cfg, ds, save_dir=str(tmp_path / "ck"), num_iterations=7, log_every=0, checkpoint_every=0, plots=False,
               background="random", acc_weight=0.05, trainer_cls=_StubTrainer)
    tr = _StubTrainer.made[-1]
    assert tr.kw["background"] == "random" and tr.kw["acc_weight"] == 0.05
    assert len(tr.steps_seen) == 7
    for target, kw in tr.steps_seen:
        a = kw["alpha"]
        assert a is not None and a.shape == (target.shape[0], 1)
        assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0
    # every alpha the trainer saw is a value of the PNGs' fourth channel, with an exact 0 or 1 among them
    seen = torch.cat([kw["alpha"].reshape(-1) for _, kw in tr.steps_seen])
    pool = torch.cat(list(alphas.values()))
    assert bool(torch.isin(seen, pool).all())
    assert train_nerf.losses == [0.25] * 7                              # the colour term is what is logged
    # without a background the trainer is constructed and stepped as before: no new keywords
    _StubTrainer.made.clear()
    train_nerf(cfg, ds, save_dir=str(tmp_path / "ck2"), num_iterations=2, log_every=0, checkpoint_every=0, plots=False,
               trainer_cls=_StubTrainer)
    tr = _StubTrainer.made[-1]
    assert "background" not in tr.kw and "acc_weight" not in tr.kw
    assert all("alpha" not in kw for _, kw in tr.steps_seen)
    assert train_nerf.losses == [pytest.approx(0.3)] * 2
    # an opacity weight alone gets the alpha channel too (without it every ray would be pulled to acc = 1)
    _StubTrainer.made.clear()
    train_nerf(cfg, ds, save_dir=str(tmp_path / "ck4"), num_iterations=2, log_every=0, checkpoint_every=0, plots=False,
               acc_weight=0.05, trainer_cls=_StubTrainer)
    tr = _StubTrainer.made[-1]
    assert tr.kw["background"] is None and tr.kw["acc_weight"] == 0.05
    assert all(kw["alpha"] is not None for _, kw in tr.steps_seen)
    # the custom format has no alpha channel: None reaches the trainer (it means ones)
    monkeypatch.setattr(ds, "get_rays", lambda **kw: {"rays_o": torch.zeros(4, 3), "rays_d": torch.zeros(4, 3),
                                                      "rgb": torch.zeros(4, 3), "alpha": None, "appearance_idx": 0})
    _StubTrainer.made.clear()
    train_nerf(cfg, ds, save_dir=str(tmp_path / "ck3"), num_iterations=1, log_every=0, checkpoint_every=0, plots=False,
               background=(1.0, 1.0, 1.0), trainer_cls=_StubTrainer)
    assert _StubTrainer.made[-1].steps_seen[0][1] == {"seed": None, "alpha": None}
