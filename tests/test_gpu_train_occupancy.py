"""Training with an occupancy grid on the GPU (include/nerfmi_train.h "training with an occupancy
grid"): the gathered training forward (csrc/mlp16.hip, mlp16_live_kernel), the
whole-step entry points (csrc/train_api.hip) and the Trainer plumbing.

The main criterion is bit-identity with compositions of the existing stage entry points: the gathered
forward equals nerf_mlp_forward_train at N = 1 on the gathered inputs, and the whole step equals
that forward scattered into zero-filled dense rows, nerf_composite, nerf_composite_backward, a
gather, nerf_mlp_backward and nerf_param_grads over the live rows.  The semantics (a dead sample has
sigma = 0 as a constant) are held to the oracle's sigma-masked step with the helpers and factors of
tests/test_gpu_train.py.  f16x3 throughout (the gathered kernel's arithmetic).
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO
from oracle import nerf_oracle as O

sys.path.insert(0, os.path.join(REPO, "tests"))
import occupancy_restated as R   # noqa: E402
from test_gpu_train import (assert_branch_flips_bounded, gpu_step_masks, no_worse_on_own_branches,   # noqa: E402
                            step_refs)

pytestmark = pytest.mark.gpu

F3 = ctypes.c_float * 3
SENT = 12345.0
G = 16
# (B, N) -> box and sphere radius of the G = 16 grid (live shares 0.12 and 0.17, some rays all dead:
# asserted in `batch`)
GRIDS = {(256, 64): ((-0.85, -1.5, -1.5), (2.25, 1.6, 1.6), 0.3), (37, 7): ((-1.5, -1.3, -1.7), (1.6, 1.9, 1.4), 0.15)}
NAMES = list(O.STATE_KEYS) + ["appearance_embeddings"]


@pytest.fixture(scope="module", autouse=True)
def f16x3():
    from nerfmi import _lib as L
    prev = L.set_mlp_arith("f16x3")
    yield
    L.set_mlp_arith(prev)


@pytest.fixture(scope="module")
def L():
    from nerfmi import _lib
    return _lib


@pytest.fixture(scope="module")
def lib(L):
    return L.load()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc, lib):
    assert rc == 0, lib.nerf_last_error()


def make_trainer(ref_state, N=64, n_images=3, **kw):
    import nerfmi
    from nerfmi.train import Trainer
    cfg = nerfmi.Config()
    cfg.num_samples = N
    torch.manual_seed(0)
    model = nerfmi.NeRF(cfg)
    model.load_state_dict(ref_state)
    torch.manual_seed(1)
    table = torch.randn(n_images, 32)
    return Trainer(cfg, model=model, appearance_embeddings=table, **kw), table


def grid_for(B, N, mask=None, box=None):
    import nerfmi
    lo, hi, rad = GRIDS[(B, N)]
    if box is not None:
        lo, hi = box
    m = R.sphere_mask(G, rad) if mask is None else mask
    return nerfmi.OccupancyGrid(lo, hi, G).from_mask(torch.from_numpy(m)), m


@pytest.fixture(scope="module")
def batch(lib, L, ref_state, golden, app_vec):
    """The two batches, staged once through the existing entry points (f16x3): F7's 256 rays x 64 and
    37 chair rays x 7 with jitter; dn, z, ray features, enc_d, the packed weights, the restated
    rule's live mask of the case's sphere grid, and the N = 1 training forward of the live samples."""
    from nerfmi.ray_utils import linspace_table
    f7, f1 = golden("f7_train_step.npz"), golden("f1_get_rays.npz")
    tr, _ = make_trainer(ref_state)
    ok(lib.nerf_pack_weights(tr.param_ptrs, P(tr.packed), S()), lib)
    ok(lib.nerf_pack_weights_transposed(tr.param_ptrs, P(tr.packedT), S()), lib)
    app = app_vec.reshape(1, 32).cuda()
    out = {}
    for (B, N), o, d, tgt in (((256, 64), f7["o"], f7["d"], f7["target"]),
                              ((37, 7), f1["chair_o"][::110][:37], f1["chair_d"][::110][:37], None)):
        g = torch.Generator().manual_seed(5)
        o, d = torch.from_numpy(o.copy()).cuda().contiguous(), torch.from_numpy(d.copy()).cuda().contiguous()
        t_rand = torch.rand(B, N, generator=g)
        tgt = torch.rand(B, 3, generator=g) if tgt is None else torch.from_numpy(tgt.copy())
        dn, z = torch.empty(B, 3, device="cuda"), torch.empty(B, N, device="cuda")
        feat, encd = torch.empty(B, 256, device="cuda"), torch.empty(B, 32, device="cuda")
        ok(lib.nerf_normalize_dirs(P(d), B, P(dn), S()), lib)
        ok(lib.nerf_sample_stratified(P(o), P(dn), B, 2.0, 6.0, N, P(linspace_table(N, o.device)), 1,
                                      P(t_rand.cuda()), 0, P(z), None, S()), lib)
        ok(lib.nerf_ray_features_train(P(tr.packed), P(dn), B, P(app), 1, P(feat), P(encd), S()), lib)
        lo, hi, rad = GRIDS[(B, N)]
        mask = R.sphere_mask(G, rad)
        live = R.classify(o.cpu(), dn.cpu(), z.cpu(), lo, hi, G, mask)
        share, per_ray = float(live.float().mean()), live.sum(1)
        assert 0.1 <= share <= 0.9, share
        assert bool((per_ray == 0).any()) and bool((per_ray > 0).any())       # neither an empty nor a full list
        idx, cnt = R.live_list(live)
        c = dict(B=B, N=N, o=o, d=d, dn=dn, z=z, feat=feat, encd=encd, t_rand=t_rand, target=tgt.cuda(), app=app,
                 packed=tr.packed, packedT=tr.packedT, live=live, idx=idx, cnt=cnt, mask=mask, trainer=tr)
        c["n1"] = forward_n1(lib, L, c, idx.long())
        out[(B, N)] = c
    torch.cuda.synchronize()
    return out


def forward_n1(lib, L, c, idx):
    """nerf_mlp_forward_train at N = 1 on the gathered inputs of the samples idx (ascending, int64, CPU):
    save, masks, rgb, sigma, every buffer pre-filled with the sentinel."""
    k = idx.numel()
    r = (idx // c["N"]).cuda()
    o1, d1 = c["o"][r].contiguous(), c["dn"][r].contiguous()
    z1 = c["z"].reshape(-1)[idx.cuda()].contiguous()
    f1, e1 = c["feat"][r].contiguous(), c["encd"][r].contiguous()
    save = torch.full((L.tile_rows(k), L.SAVE_ROW), SENT, device="cuda")
    masks = torch.full((max(k, 1), L.MASK_ROW), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    rgb, sigma = torch.full((max(k, 1), 3), SENT, device="cuda"), torch.full((max(k, 1),), SENT, device="cuda")
    if k:
        ok(lib.nerf_mlp_forward_train(P(c["packed"]), P(o1), P(d1), P(z1), k, 1, P(f1), P(e1), P(rgb), P(sigma),
                                      P(save), P(masks), S()), lib)
    return save, masks, rgb, sigma


# ------------------------------------------------------------------------ 1. the gathered forward
@pytest.mark.parametrize("B,N,k", [(100, 64, k) for k in (0, 1, 31, 32, 33, 129, 3001, 6400)] +
                         [(37, 7, k) for k in (1, 31, 32, 33, 129, 259)])
def test_gathered_forward_equals_the_dense_forward_on_the_gathered_inputs(lib, L, batch, B, N, k):
    c = dict(batch[(256, 64) if N == 64 else (37, 7)])
    c["o"], c["dn"], c["z"], c["feat"], c["encd"] = (c[n][:B].contiguous() for n in ("o", "dn", "z", "feat", "encd"))
    M = B * N
    g = torch.Generator().manual_seed(100 + k)
    if k == M:
        idx = torch.arange(M)
    else:                                        # sample 0 stays outside the list: the list's tail names it
        idx = (torch.randperm(M - 1, generator=g)[:k] + 1).sort().values
    live = torch.zeros(M, dtype=torch.int32, device="cuda")
    live[:k] = idx.to(torch.int32).cuda()
    save = torch.full((L.tile_rows(k), L.SAVE_ROW), SENT, device="cuda")
    masks = torch.full((max(k, 1), L.MASK_ROW), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    rgb_l, sig_l = torch.full((max(k, 1), 3), SENT, device="cuda"), torch.full((max(k, 1),), SENT, device="cuda")
    rgb, sig = torch.full((M, 3), SENT, device="cuda"), torch.full((M,), SENT, device="cuda")
    ok(lib.nerf_mlp_forward_train_live(P(c["packed"]), P(c["o"]), P(c["dn"]), P(c["z"]), B, N, P(c["feat"]),
                                       P(c["encd"]), P(live), k, P(rgb), P(sig), P(rgb_l), P(sig_l), P(save), P(masks),
                                       S()), lib)
    e_save, e_masks, e_rgb, e_sig = forward_n1(lib, L, c, idx)
    assert torch.equal(save, e_save)             # padding rows and block-exponent records included
    assert torch.equal(masks, e_masks)
    assert torch.equal(rgb_l, e_rgb) and torch.equal(sig_l, e_sig)
    sel = torch.zeros(M, dtype=torch.bool)
    sel[idx] = True
    sel = sel.cuda()
    if k:
        assert torch.equal(rgb[sel], e_rgb) and torch.equal(sig[sel], e_sig)
        assert not bool((save == SENT).all()) and bool((e_sig != SENT).all())
    assert bool((rgb[~sel] == SENT).all()) and bool((sig[~sel] == SENT).all())


# ------------------------------------------------------------------------------ 2. the whole step
def occ_step(lib, c, grid, bufs=None):
    """The three whole-step calls on case c: (M_live, loss, rgb_map, depth, weights, z_out, grads, dapp)."""
    from nerfmi.ray_utils import linspace_table
    B, N = c["B"], c["N"]
    ws = torch.empty(lib.nerf_train_occ_workspace_bytes(B, N), dtype=torch.uint8, device="cuda")
    count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    ok(lib.nerf_train_occ_sample(P(c["o"]), P(c["d"]), B, 2.0, 6.0, N, P(linspace_table(N, c["o"].device)), 1,
                                 P(c["t_rand"].cuda()), 0, P(grid.bits), grid.resolution, grid.c_lo(), grid.c_inv(),
                                 P(count), P(ws), ws.numel(), S()), lib)
    m_live = int(count.item())
    rgb_map, depth = torch.full((B, 3), SENT, device="cuda"), torch.full((B,), SENT, device="cuda")
    w, z_out = torch.full((B, N), SENT, device="cuda"), torch.full((B, N), SENT, device="cuda")
    ok(lib.nerf_train_occ_forward(P(c["packed"]), P(c["o"]), B, N, m_live, P(c["app"]), 1, P(rgb_map), P(depth), P(w),
                                  P(z_out), P(ws), ws.numel(), S()), lib)
    tr = c["trainer"]
    grads = [torch.full_like(tr.view(tr.grad, i), SENT) for i in range(24)]
    gptr = (ctypes.c_void_p * 24)(*[t.data_ptr() for t in grads])
    dapp, loss = torch.full((32,), SENT, device="cuda"), torch.full((1,), SENT, device="cuda")
    ok(lib.nerf_train_occ_backward(P(c["packed"]), P(c["packedT"]), P(rgb_map), P(c["target"]), B, N, m_live,
                                   P(c["app"]), 1, gptr, P(dapp), P(loss), P(ws), ws.numel(), S()), lib)
    torch.cuda.synchronize()
    return m_live, loss, rgb_map, depth, w, z_out, grads, dapp


@pytest.mark.parametrize("B,N", [(256, 64), (37, 7)])
def test_whole_step_equals_the_composition_of_the_stages(lib, L, batch, B, N):
    c = batch[(B, N)]
    grid, _ = grid_for(B, N)
    m_live, loss, rgb_map, depth, w, z_out, grads, dapp = occ_step(lib, c, grid)
    assert m_live == c["cnt"] and 0 < m_live < B * N
    # the expected side: the N = 1 forward scattered into zero-filled dense rows, the dense composite and
    # its backward, a gather, the backward and the weight gradients over the live rows
    M, idx = B * N, c["idx"].long().cuda()
    save, masks, rgb1, sig1 = c["n1"]
    rgb_d, sig_d = torch.zeros(M, 3, device="cuda"), torch.zeros(M, device="cuda")
    rgb_d[idx], sig_d[idx] = rgb1, sig1
    e_map, e_depth, e_w = (torch.empty(B, 3, device="cuda"), torch.empty(B, device="cuda"),
                           torch.empty(B, N, device="cuda"))
    ok(lib.nerf_composite(P(rgb_d), P(sig_d), P(c["z"]), B, N, P(e_map), P(e_depth), P(e_w), S()), lib)
    dsig, drgb, sq = torch.empty(M, device="cuda"), torch.empty(M, 3, device="cuda"), torch.empty(B, device="cuda")
    ok(lib.nerf_composite_backward(P(rgb_d), P(sig_d), P(c["z"]), P(e_map), P(c["target"]), B, N, 2.0 / (3 * B),
                                   P(dsig), P(drgb), P(sq), S()), lib)
    dsig1, drgb1 = dsig[idx].contiguous(), drgb[idx].contiguous()
    grad = torch.empty(L.tile_rows(m_live), L.GRAD_ROW, device="cuda")
    ok(lib.nerf_mlp_backward(P(c["packed"]), P(c["packedT"]), P(save), P(masks), P(sig1), P(rgb1), P(dsig1),
                             P(drgb1), m_live, P(grad), S()), lib)
    tr = c["trainer"]
    e_grads = [torch.full_like(tr.view(tr.grad, i), SENT) for i in range(24)]
    gptr = (ctypes.c_void_p * 24)(*[t.data_ptr() for t in e_grads])
    e_dapp = torch.full((32,), SENT, device="cuda")
    wsz = lib.nerf_param_grads_workspace_bytes(m_live)
    pws = torch.empty(wsz, dtype=torch.uint8, device="cuda")
    ok(lib.nerf_param_grads(P(save), P(grad), m_live, 1, P(c["app"]), 1, P(c["packed"]), gptr, P(e_dapp), P(pws), wsz,
                            S()), lib)
    torch.cuda.synchronize()
    assert torch.equal(rgb_map, e_map) and torch.equal(depth, e_depth) and torch.equal(w, e_w)
    assert torch.equal(z_out, c["z"])
    assert torch.equal(loss[0], (sq.double().sum() / (3.0 * B)).float())
    for i, (a, b) in enumerate(zip(grads, e_grads)):
        assert torch.equal(a, b), NAMES[i]
        assert not bool((a == SENT).any()), NAMES[i]
    assert torch.equal(dapp, e_dapp)
    dead = ~c["live"].cuda()
    assert bool((w[dead] == 0).all()) and bool((w[~dead] >= 0).all()) and float(w.sum()) > 0


# -------------------------------------------------------------------- 3. semantics vs the oracle
def masked_step_refs(c, state, table, app_idx, m_gpu, name):
    """step_refs of tests/test_gpu_train.py for the sigma-masked step: the oracle's NeRF.forward on every
    sample, sigma (and rgb) of the dead ones replaced by 0 (the restated rule's mask, a constant),
    O.composite and F.mse_loss: fp32 autograd on its own ReLU branches, float64 on those, float64 on
    the GPU's branches.  Returns (loss fp32, g32, g64 on the CPU's branches, g64 on the GPU's)."""
    live = c["live"].reshape(-1, 1)

    def hook(masks=None, record=None, pres=None):
        def relu(pre, i):
            if record is not None:
                record.append(pre.detach() > 0)
            if pres is not None:
                pres.append(pre.detach())
            return torch.relu(pre) if masks is None else pre * masks[i].to(pre.dtype)
        return relu

    def run(dtype, relu):
        st = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in state.items()}
        tab = table.detach().to(dtype).clone().requires_grad_(True)
        o, d = c["o"].cpu().to(dtype), O.normalize(c["d"].cpu().to(dtype))
        z, pts = O.sample_stratified(o, d, 2.0, 6.0, c["N"], c["t_rand"].to(dtype))
        B, N = z.shape
        with torch.enable_grad():
            dexp = d.unsqueeze(1).expand(-1, N, -1).reshape(-1, 3)
            rgb, sigma = O.nerf_forward(st, pts.reshape(-1, 3), dexp, tab[app_idx].unsqueeze(0).expand(B * N, -1),
                                        relu=relu)
            keep = live.to(dtype)
            rgb_map, _, _ = O.composite((rgb * keep).reshape(B, N, 3), (sigma * keep).reshape(B, N, 1), z)
            loss = F.mse_loss(rgb_map, c["target"].cpu().to(dtype))
            loss.backward()
        g = {k: v.grad.detach().double().numpy() for k, v in st.items()}
        g["appearance_embeddings"] = tab.grad.detach().double().numpy()
        return float(loss.detach()), g
    m_cpu, pre64 = [], []
    loss32, g32 = run(torch.float32, hook(record=m_cpu))
    _, g64c = run(torch.float64, hook(masks=m_cpu, pres=pre64))
    assert_branch_flips_bounded(m_cpu, m_gpu, pre64, name)
    return loss32, g32, g64c, run(torch.float64, hook(masks=m_gpu))[1]


@pytest.mark.parametrize("B,N", [(256, 64), (37, 7)])
def test_masked_step_matches_the_oracle(ref_state, batch, B, N):
    c = batch[(B, N)]
    grid, _ = grid_for(B, N)
    tr, table = make_trainer(ref_state, N=N, occupancy=grid)
    loss, _ = tr.forward_backward(c["o"], c["d"], c["target"], 2, t_rand=c["t_rand"])
    torch.cuda.synchronize()
    assert tr.live_fraction == c["cnt"] / (B * N)
    m_gpu = gpu_step_masks(tr, c["o"], c["d"], c["t_rand"], 2)
    loss_o, g32, g64c, g64g = masked_step_refs(c, ref_state, table, 2, m_gpu, f"masked step {B}x{N}")
    print(f"loss gpu {float(loss):.9g} oracle {loss_o:.9g}")
    assert abs(float(loss) - loss_o) <= 2e-5 * loss_o
    for i, n in enumerate(NAMES):
        got = tr.view(tr.grad, i).detach().cpu().numpy()
        no_worse_on_own_branches(got, g64g[n], g32[n], g64c[n], n)


# ------------------------------------------------------------------- 4. all ones and all zeros
def test_all_ones_grid_is_the_dense_step(ref_state, batch):
    """The forward is placement-independent (test 1), so with every sample live rgb_map and the loss
    are nerf_train_forward's bit for bit; the gradients take the per-row route (different summation
    grouping in the weight gradients) and are held to the dense step's float64 like test 3."""
    c = batch[(256, 64)]
    grid, _ = grid_for(256, 64, mask=np.ones((G, G, G), bool), box=((-10.0,) * 3, (10.0,) * 3))
    tr, table = make_trainer(ref_state, occupancy=grid)
    dense, _ = make_trainer(ref_state)
    loss, rgb = tr.forward_backward(c["o"], c["d"], c["target"], 2, t_rand=c["t_rand"])
    loss_d, rgb_d = dense.forward_backward(c["o"], c["d"], c["target"], 2, t_rand=c["t_rand"])
    torch.cuda.synchronize()
    assert tr.live_fraction == 1.0
    assert torch.equal(rgb, rgb_d) and torch.equal(loss, loss_d)
    m_gpu = gpu_step_masks(tr, c["o"], c["d"], c["t_rand"], 2)
    g32, g64c, g64g = step_refs(ref_state, table, 2, c["o"], c["d"], c["target"], c["t_rand"], m_gpu,
                                name="all-ones grid")
    for i, n in enumerate(NAMES):
        no_worse_on_own_branches(tr.view(tr.grad, i).detach().cpu().numpy(), g64g[n], g32[n], g64c[n], n)


def test_all_zeros_grid(ref_state, batch):
    c = batch[(37, 7)]
    grid, _ = grid_for(37, 7, mask=np.zeros((G, G, G), bool))
    tr, _ = make_trainer(ref_state, N=7, occupancy=grid)
    tr.grad.fill_(SENT)
    loss, rgb = tr.forward_backward(c["o"], c["d"], c["target"], 2, t_rand=c["t_rand"])
    torch.cuda.synchronize()
    assert tr.live_fraction == 0.0
    assert bool((rgb == 0).all())
    # mean(target^2): the kernels round each ray's three squared errors and their sum to float (four
    # roundings of 2^-24 each) before the double-precision mean
    want = float((c["target"].double() ** 2).mean())
    assert abs(float(loss) - want) <= 4 * 2.0 ** -24 * want
    for i in range(24):
        assert bool((tr.view(tr.grad, i) == 0).all()), NAMES[i]
    assert bool((tr.app_grad == 0).all())
    tr.optimizer_step()
    before = tr.flat.detach().clone()
    grid.from_mask(torch.from_numpy(c["mask"]))           # two further steps run normally
    for _ in range(2):
        loss = tr.step(c["o"], c["d"], c["target"], 2, t_rand=c["t_rand"])
        assert 0 < tr.live_fraction < 1 and np.isfinite(float(loss.detach()))
    assert bool(torch.isfinite(tr.flat).all()) and not torch.equal(tr.flat, before)


# --------------------------------------------------------------------------------- 5. Trainer
def test_trainer_is_deterministic_refreshes_and_checkpoints(ref_state, batch):
    import nerfmi
    c = batch[(37, 7)]
    lo, hi, _ = GRIDS[(37, 7)]
    refresh = dict(every=3, warmup=2, threshold=0.5, dilate=1, supersample=1)
    runs = []
    for _ in range(2):
        grid = nerfmi.OccupancyGrid(lo, hi, G)                       # all clear: the trainer fills it
        tr, _ = make_trainer(ref_state, N=7, occupancy=grid, occupancy_refresh=refresh)
        ones = nerfmi.OccupancyGrid(lo, hi, G).from_mask(torch.ones(G, G, G, dtype=torch.bool))
        losses = []
        for i in range(5):
            if i < 2:
                assert torch.equal(grid.bits, ones.bits)             # all ones during warm-up
            losses.append(float(tr.step(c["o"], c["d"], c["target"], 2, seed=i + 1)))
            if i + 1 in (2, 3):                                      # rebuilt after steps warmup and every
                want = nerfmi.OccupancyGrid.from_model(tr.model, lo, hi, resolution=G, threshold=0.5, dilate=1)
                assert torch.equal(grid.bits, want.bits), i
        torch.cuda.synchronize()
        runs.append((tr.flat.detach().cpu().clone(), losses, grid.bits.cpu().clone()))
        ck = tr.checkpoint(losses[-1], 0.0, 5)
    assert runs[0][1] == runs[1][1] and torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][2], runs[1][2])
    g2 = nerfmi.OccupancyGrid((0, 0, 0), (1, 1, 1), 3).load_state_dict(ck["occupancy"])
    assert g2.resolution == G and torch.equal(g2.bits.cpu(), runs[1][2]) and np.array_equal(g2.lo, grid.lo)
    assert np.array_equal(g2.hi, grid.hi)
    plain, _ = make_trainer(ref_state, N=7)
    assert "occupancy" not in plain.checkpoint(0.0, 0.0, 0)


def test_trainer_refuses_f32_arithmetic(ref_state, batch, L):
    c = batch[(37, 7)]
    grid, _ = grid_for(37, 7)
    tr, _ = make_trainer(ref_state, N=7, occupancy=grid)
    prev = L.set_mlp_arith("f32")
    try:
        with pytest.raises(ValueError, match="f16x3"):
            tr.forward_backward(c["o"], c["d"], c["target"], 2, t_rand=c["t_rand"])
    finally:
        L.set_mlp_arith(prev)


# ------------------------------------------------------------------------------------- 6. CLI
def test_cli_trains_with_a_grid(tmp_path, monkeypatch):
    import run as cli
    monkeypatch.chdir(tmp_path)
    assert cli.main(["--mode", "train", "--random_init", "0", "--occupancy", "16", "--iterations", "3"]) == 0
    ck = torch.load(tmp_path / "checkpoints" / "checkpoint_final.pt", weights_only=False)
    assert ck["occupancy"]["resolution"] == 16 and ck["occupancy"]["bits"].numel() == 16 ** 3 // 32
