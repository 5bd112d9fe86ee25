"""CPU-side checks of the density-gradient normals (include/nerfmi_train.h "position gradient and
normals"): the new symbols are exported, bad arguments are refused before any launch,
the host packer produces the layout the position-gradient kernel assumes (its register dataflow is
replayed in numpy on the host-packed buffer, as tests/test_capi_host.py does for the forward), and the
Python and CLI argument checks fire without a device."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from nerfmi import _lib

NEW = ("nerf_packed_input_floats", "nerf_pack_weights_input", "nerf_pack_weights_input_host",
       "nerf_mlp_position_grad", "nerf_composite_normals", "nerf_render_normals_workspace_bytes",
       "nerf_render_normals")


def test_new_symbols_are_exported():
    lib = _lib.load()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTED, s
    assert lib.nerf_abi_version() == _lib.ABI_VERSION == 11
    assert lib.nerf_packed_input_floats() == 64 * 512


def test_bad_arguments_are_reported_not_launched():
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    arr = (ctypes.c_void_p * 24)(*([0x1000] * 24))
    # packers
    assert lib.nerf_pack_weights_input(None, fake, None) == 1
    assert lib.nerf_pack_weights_input(arr, None, None) == 1 and b"nerf_pack_weights_input" in lib.nerf_last_error()
    assert lib.nerf_pack_weights_input_host(arr, None) == 1
    holes = (ctypes.c_void_p * 24)(*([0x1000] * 8 + [0] + [0x1000] * 15))
    assert lib.nerf_pack_weights_input_host(holes, fake) == 1 and b"parameter 8" in lib.nerf_last_error()
    # position gradient
    assert lib.nerf_mlp_position_grad(None, fake, fake, 5, fake, None) == 1
    assert b"null pointer" in lib.nerf_last_error()
    assert lib.nerf_mlp_position_grad(fake, fake, fake, 5, None, None) == 1
    assert lib.nerf_mlp_position_grad(fake, fake, fake, -1, fake, None) == 1
    assert lib.nerf_mlp_position_grad(None, None, None, 0, None, None) == 0
    # composite
    assert lib.nerf_composite_normals(None, fake, 4, 16, fake, None) == 1
    assert lib.nerf_composite_normals(fake, fake, 4, 16, None, None) == 1
    assert lib.nerf_composite_normals(fake, fake, 4, 0, fake, None) == 3
    assert lib.nerf_composite_normals(fake, fake, 4, 5000, fake, None) == 3 and b"1..4096" in lib.nerf_last_error()
    assert lib.nerf_composite_normals(fake, fake, -1, 16, fake, None) == 1
    assert lib.nerf_composite_normals(None, None, 0, 16, None, None) == 0
    # the render-side pass
    assert lib.nerf_render_normals_workspace_bytes(4, 0) == 0
    assert lib.nerf_render_normals_workspace_bytes(4, 5000) == 0
    assert lib.nerf_render_normals_workspace_bytes(-1, 16) == 0
    need = lib.nerf_render_normals_workspace_bytes(37, 24)
    assert need > 37 * 24 * (2400 + 2320) * 4          # one chunk's save and gradient rows, and the rest
    # the workspace holds one chunk: 2^18 samples at the most, whatever B
    assert lib.nerf_render_normals_workspace_bytes(1 << 20, 64) == lib.nerf_render_normals_workspace_bytes(4096, 64)
    args = [fake] * 7 + [37, 24, fake, fake]
    assert lib.nerf_render_normals(*args, need - 1, None) == 1 and b"workspace" in lib.nerf_last_error()
    for hole in (0, 1, 2, 3, 4, 5, 6, 9, 10):
        a = list(args)
        a[hole] = None
        assert lib.nerf_render_normals(*a, need, None) == 1, hole
        assert b"null pointer" in lib.nerf_last_error()
    assert lib.nerf_render_normals(*([fake] * 7 + [37, 0, fake, fake]), need, None) == 3
    assert lib.nerf_render_normals(*([fake] * 7 + [37, 5000, fake, fake]), need, None) == 3
    assert lib.nerf_render_normals(*([fake] * 7 + [-1, 24, fake, fake]), need, None) == 1
    assert lib.nerf_render_normals(*([None] * 7 + [0, 24, None, None]), 0, None) == 0


# ---- restatement of csrc/layout.h "input-gradient weights" for the emulator
GRAD_ROW, SAVE_ROW, SAVE_ENC_X = 2320, 2400, 1024
IN_GROUPS = 64


def in_out_feature(i, h):
    if i < 30:
        j = i >> 1
        level, c = 2 * (j // 3) + h, j % 3
        return 3 + 6 * level + c + 3 * (i & 1)
    if i == 30:
        return h
    return -1 if h else 2


def in_row_feature(t, r):
    return in_out_feature(16 * t + (r & 3) + 4 * (r >> 3), (r >> 2) & 1)


def in_grad_feature(k):
    return k if k < 256 else 4 * 256 + (k - 256)


def tile_off(m, f, R):
    return (m // 32) * 32 * R + (f // 8) * 256 + (m % 32) * 8 + f % 8


def host_pack_input(state):
    lib = _lib.load()
    ts = [state[k].contiguous().float() for k in O.STATE_KEYS]
    arr = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    out = np.full(lib.nerf_packed_input_floats(), np.nan, dtype=np.float32)
    assert lib.nerf_pack_weights_input_host(arr, out.ctypes.data) == 0
    return out


def test_packed_input_fragments_are_permuted_weight_transposes(ref_state):
    """Element j of lane l of fragment block (tile t, group G) is W_in[row feature][input 8 G + 4 (l >> 5) + j]:
    W0^T for the first 256 inputs, W4[:, 256:319]^T for the rest, the zero row where the feature is -1."""
    pk = host_pack_input(ref_state).reshape(2, IN_GROUPS, 64, 4)
    w0 = ref_state["pts_linears.0.weight"].numpy()              # (256, 63)
    w4 = ref_state["pts_linears.4.weight"].numpy()[:, 256:]     # (256, 63)
    w_in = np.concatenate([w0.T, w4.T], axis=1)                 # (63, 512): feature x input
    rows = sorted(in_row_feature(t, r) for t in range(2) for r in range(32))
    assert rows == [-1] + list(range(63)), "every feature is one output row, and one row is zero"
    for t in range(2):
        for r in range(32):
            f = in_row_feature(t, r)
            for hh in range(2):
                got = pk[t, :, 32 * hh + r, :]                  # (G, j)
                k = 8 * np.arange(IN_GROUPS)[:, None] + 4 * hh + np.arange(4)[None, :]
                want = np.zeros_like(got) if f < 0 else w_in[f][k]
                assert np.array_equal(got, want), (t, r, hh)


def test_emulated_position_gradient_matches_autograd(ref_state):
    """The kernel's dataflow on the host-packed buffer, in numpy: the B operands read from tile-major
    gradient rows as they lie, the A operands from the packed fragments, the accumulator's (lane half,
    value) -> feature map, the sin/cos partners from the tile-major save rows, one exchange between the
    lane halves.  Against float64 autograd of positional_encoding -> the two linear maps.

    Slot 63 of enc_x holds garbage (a block-exponent record under f16x3): a replay or a layout that read
    it as a feature would be off by orders of magnitude.

    Bound: the replay runs in float64 on float32 inputs; the only rounding autograd does not share is that
    of the stored float32 sines and cosines (2^-24 relative each, scaled by the same 2^k as the value they
    stand in for), so the rel-L2 distance is a few 1e-8: 1e-6 is asserted."""
    M = 64
    g = torch.Generator().manual_seed(21)
    x = (torch.rand(M, 3, generator=g) * 3 - 1.5).double()
    dpre0 = torch.randn(M, 256, generator=g)
    dpre4 = torch.randn(M, 256, generator=g)
    enc = O.positional_encoding(x, 10).float()                  # what the forward saves (63 values)
    grad_rows = torch.randn(M, GRAD_ROW, generator=g)           # every other slice: values that must not matter
    grad_rows[:, 0:256] = dpre0
    grad_rows[:, 1024:1280] = dpre4
    save_rows = torch.randn(M, SAVE_ROW, generator=g)
    save_rows[:, SAVE_ENC_X:SAVE_ENC_X + 63] = enc
    save_rows[:, SAVE_ENC_X + 63] = -1000.0 - torch.arange(M)   # the pad slot: block-exponent records
    grad_t = _lib.tile(grad_rows).numpy().reshape(-1).astype(np.float64)
    save_t = _lib.tile(save_rows).numpy().reshape(-1).astype(np.float64)
    pk = host_pack_input(ref_state).reshape(2, IN_GROUPS, 64, 4).astype(np.float64)

    dx = np.zeros((M, 3))
    for b in range(M // 32):
        # MFMA: acc[t][row r][sample s] = sum over k-steps (G, j) and k halves hh of A[r, hh] B[hh, s]
        acc = np.zeros((2, 32, 32))
        for G in range(IN_GROUPS):
            for j in range(4):
                B = np.empty((2, 32))
                for hh in range(2):
                    f = in_grad_feature(8 * G + 4 * hh + j)
                    assert f % 8 == 4 * hh + j              # the lane's 16 bytes of the group, as they lie
                    B[hh] = [grad_t[tile_off(32 * b + s, f, GRAD_ROW)] for s in range(32)]
                for t in range(2):
                    A = np.stack([pk[t, G, 32 * hh:32 * hh + 32, j] for hh in range(2)], axis=1)   # (row, hh)
                    acc[t] += A @ B
        # the accumulator as lanes hold it: value i = 16 t + g of lane half h = tile row (g & 3) + 8 (g >> 2) + 4 h
        for s in range(32):
            part = np.zeros((2, 3))
            for h in range(2):
                v = [acc[i // 16, (i % 16 & 3) + 8 * (i % 16 >> 2) + 4 * h, s] for i in range(32)]
                e = lambda f: save_t[tile_off(32 * b + s, SAVE_ENC_X + f, SAVE_ROW)]
                for i in (30, 31):
                    f = in_out_feature(i, h)
                    if f >= 0:
                        part[h, f] += v[i]
                    else:
                        assert v[i] == 0.0                    # the zero row
                for jj in range(15):
                    fs, fc = in_out_feature(2 * jj, h), in_out_feature(2 * jj + 1, h)
                    level, c = 2 * (jj // 3) + h, jj % 3
                    assert fs == 3 + 6 * level + c and fc == fs + 3
                    part[h, c] += 2.0 ** level * (e(fc) * v[2 * jj] - e(fs) * v[2 * jj + 1])
            dx[32 * b + s] = part[0] + part[1]

    xg = x.clone().requires_grad_(True)
    w0 = ref_state["pts_linears.0.weight"].double()
    w4 = ref_state["pts_linears.4.weight"].double()[:, 256:]
    e64 = O.positional_encoding(xg, 10)
    ((e64 @ w0.T * dpre0.double()).sum() + (e64 @ w4.T * dpre4.double()).sum()).backward()
    ref = xg.grad.numpy()
    rel = np.linalg.norm(dx - ref) / np.linalg.norm(ref)
    print(f"emulated position gradient vs float64 autograd: rel-L2 {rel:.3g}")
    assert rel <= 1e-6, rel


@pytest.mark.parametrize("with_acc", [False, True])
def test_sharded_frames_gather_the_normal_map(with_acc):
    """render_frames_sharded(with_normals=True) with an injected renderer: the normal map travels as three
    more columns behind the depth (and the opacity) and comes back as (n_frames,H,W,3) at the end of the
    result, in ray order, for shards that cut frames and rows."""
    from nerfmi import frames
    H, W, n_frames = 5, 7, 2

    def ray_fn(frame, row0, nrows):
        idx = frame * H * W + row0 * W + torch.arange(nrows * W, dtype=torch.float32)
        return idx[:, None].repeat(1, 3), idx[:, None].repeat(1, 3) + 0.5

    def render_fn(o, d, offset):
        i = o[:, 0]
        assert int(i[0]) == offset
        out = (torch.stack([i, 2 * i, 3 * i], 1), (4 * i)[:, None]) + (((5 * i)[:, None],) if with_acc else ())
        return out + (torch.stack([-i, i + 0.25, 7 * i], 1),)

    res = frames.render_frames_sharded(ray_fn, render_fn, H, W, n_frames, device="cpu", virtual_shards=3,
                                       with_acc=with_acc, with_normals=True)
    assert len(res) == (4 if with_acc else 3)
    i = torch.arange(n_frames * H * W, dtype=torch.float32).reshape(n_frames, H, W)
    assert torch.equal(res[0], torch.stack([i, 2 * i, 3 * i], -1)) and torch.equal(res[1], 4 * i)
    if with_acc:
        assert torch.equal(res[2], 5 * i)
    assert res[-1].shape == (n_frames, H, W, 3)
    assert torch.equal(res[-1], torch.stack([-i, i + 0.25, 7 * i], -1))


def test_python_and_cli_argument_checks():
    """return_normals is refused with staged=True and with timing= before any device use, naming the
    argument; run.py takes --save_normals in the render modes only."""
    import nerfmi
    import run
    model = nerfmi.NeRF(nerfmi.Config())
    o, d = torch.zeros(4, 3), torch.ones(4, 3)
    with pytest.raises(ValueError, match="return_normals"):
        nerfmi.volume_render(model, o, d, 2.0, 6.0, 8, 0, return_normals=True, staged=True)
    with pytest.raises(ValueError, match="return_normals"):
        nerfmi.volume_render(model, o, d, 2.0, 6.0, 8, 0, return_normals=True, timing=[])
    with pytest.raises(ValueError, match="return_normals"):       # a trainable model with gradients enabled
        nerfmi.volume_render(model, o, d, 2.0, 6.0, 8, 0, return_normals=True)
    assert run.parse_args(["--mode", "render", "--save_normals"]).save_normals
    assert not run.parse_args(["--mode", "render"]).save_normals
    with pytest.raises(SystemExit):
        run.parse_args(["--mode", "train", "--save_normals"])
