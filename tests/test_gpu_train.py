"""Training path parity on the GPU (include/nerfmi_train.h through the C ABI) against torch autograd
on the oracle (oracle/nerf_oracle.py, pinned to the reference by F7) — SURVEY.md §8f row 2.

Every test runs under both MLP arithmetics: "f32" (fp32 MFMA throughout) and the default "f16x3"
(split-f16 forward, data gradients and weight gradients, with per-chunk block scales in the weight
gradients: fp32-level results from multi-part products).  Against a float64 autograd of the same inputs, gradients
agree to ~1e-5 relative in L2; a ReLU whose
pre-activation sits within fp32 rounding of 0 can flip its mask between fp32 and fp64 and
perturb single entries, so per-layer checks bound the relative L2 error (2e-4) and require
>= 99.9% of entries within rtol 1e-3 rather than demanding every entry.

Against the reference's own steps (fixture F7) and the oracle's multi-step training, gradients and
parameters are held to a float64 run of the same step(s): the GPU's deviation from float64 is no
larger than the reference's fp32 CPU deviation (grads_no_worse_than_reference,
params_no_worse_than_reference).  A fraction-of-entries tolerance would let a real error hide in the
allowed fraction; this lets only the entries the reference itself cannot pin down (a ReLU kink in
the float64 run, a gradient cancelling to ~0 whose sign decides Adam's first move) differ.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import seeded_uniform
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True, params=["f16x3", "f32"])
def arith(request):
    """The training forward runs on the MLP arithmetic in force (include/nerfmi.h, nerf_arith):
    every test here runs under both."""
    from nerfmi import _lib as L
    prev = L.set_mlp_arith(request.param)
    yield request.param
    L.set_mlp_arith(prev)


def _lib():
    from nerfmi import _lib as L
    return L


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def f7_float64(ref_state, f7, meta):
    """Fixture F7's training step (one reference step, src/train.py:77-92) run by the oracle in
    float64 from the same weights, table, rays and jitter: (gradients, updated parameters), keyed by
    F7's names.  F7 is the reference's own fp32 CPU step, so it and the GPU can both be measured
    against this float64 truth."""
    st = {k: v.double().clone() for k, v in ref_state.items()}
    torch.manual_seed(1)
    table = torch.randn(100, 32).double()
    t_rand = seeded_uniform(meta["seed_t_rand"], (256, 64), meta["t_rand_sha256"])
    o, d, tgt = (torch.from_numpy(f7[k]).double() for k in ("o", "d", "target"))
    _, _, g64, _ = O.train_step(st, table, 0, o, d, tgt, 2.0, 6.0, 64, t_rand.double(), lr=meta["lr"])
    params = dict(st, appearance_embeddings=table)
    return ({k: v.detach().numpy() for k, v in g64.items()},
            {k: v.detach().numpy() for k, v in params.items()})


def grads_no_worse_than_reference(got, ref, f64, name, factor=1.5):
    """Gradient entries (F7's sampled ones): the GPU's deviation from float64 is no larger than the
    reference's own fp32 step's, in max, p99.9 and median, each relative to the tensor's largest
    float64 entry (per-entry relative errors are meaningless at entries that cancel to ~0)."""
    got, ref, f64 = (np.asarray(t, np.float64).ravel() for t in (got, ref, f64))
    sc = np.abs(f64).max() + 1e-300
    eg, er = np.abs(got - f64) / sc, np.abs(ref - f64) / sc
    for stat, f in (("max", np.max), ("p99.9", lambda v: np.quantile(v, 0.999)), ("median", np.median)):
        assert f(eg) <= factor * f(er) + 1e-9, (name, stat, float(f(eg)), float(f(er)))


def params_no_worse_than_reference(got, ref, f64, name, tol=2e-6):
    """Parameters after Adam steps: Adam's first moves are +-lr by the sign of the gradient, so an entry
    whose gradient cancels to ~0 lands +-lr apart between any two fp32 evaluations, and a flip feeds
    the later steps.  Held to the float64 trajectory like the reference's fp32 CPU steps: no more entries
    off it by > tol than the reference (x1.25 + 4), and the largest deviation within twice the
    reference's (+ tol)."""
    got, ref, f64 = (np.asarray(t, np.float64).ravel() for t in (got, ref, f64))
    og, orf = int((np.abs(got - f64) > tol).sum()), int((np.abs(ref - f64) > tol).sum())
    assert og <= 1.25 * orf + 4, (name, "entries off the float64 trajectory", og, orf)
    mg, mr = float(np.abs(got - f64).max()), float(np.abs(ref - f64).max())
    assert mg <= 2 * mr + tol, (name, "largest deviation from the float64 trajectory", mg, mr)


def assert_branch_flips_bounded(m_cpu, m_gpu, pre64, name):
    """Kink-proof must not mean mask-blind (test_gpu_accuracy.py::test_gradients_vs_float64's rule):
    a GPU forward that took wrong ReLU branches would drag its float64 reference (on those branches)
    along.  Two fp32 evaluations may only disagree where the true pre-activation sits within their
    rounding of 0, so the branches of the ten ReLUs (models.py:128-150) that differ between the GPU
    and the fp32 CPU evaluation are bounded by the float64 pre-activations (on the CPU's branches)
    within 1e-4 of their layer's rms of zero, x4 + 8."""
    assert len(m_cpu) == len(m_gpu) == len(pre64) == 10, (name, len(m_cpu), len(m_gpu), len(pre64))
    flips = sum(int((torch.as_tensor(a).reshape(-1) != torch.as_tensor(b).reshape(-1)).sum())
                for a, b in zip(m_cpu, m_gpu))
    near = sum(int((p.abs() <= 1e-4 * p.pow(2).mean().sqrt()).sum()) for p in pre64)
    print(f"{name}: {flips} ReLU branches differ between the GPU and the CPU ({near} float64 pre-activations "
          f"within 1e-4 rms of a kink)")
    assert flips <= 4 * near + 8, (name, "ReLU branches differ between the GPU and the CPU", flips, near)


def block_records(rows, slices):
    """The block exponent records (layout.h) rows should carry: entry j of 32-sample block b, in row
    32 b + j, is -(1000 + e) for e = frexp's exponent of the block's largest |value| in slices[j]
    (an all-zero block: e = -126); every other row 0."""
    M = rows.shape[0]
    out = np.zeros(M, np.float32)
    for b in range(0, M, 32):
        for j, sl in enumerate(slices):
            if b + j >= M:
                break
            m = float(np.abs(rows[b:b + 32, sl]).max())
            e = int(np.frexp(np.float32(m))[1]) if m > 0 else -126
            out[b + j] = -(1000 + e)
    return out


def packed_of(state, dev):
    L = _lib()
    lib = L.load()
    ts = [state[k].to(dev).float().contiguous() for k in O.STATE_KEYS]
    arr = (ctypes.c_void_p * 24)(*[t.data_ptr() for t in ts])
    packed = torch.empty(lib.nerf_packed_weights_floats(), device=dev)
    packedT = torch.empty(lib.nerf_packed_transposed_floats(), device=dev)
    L.check(lib.nerf_pack_weights(arr, L.ptr(packed), L.stream()), "pack")
    L.check(lib.nerf_pack_weights_transposed(arr, L.ptr(packedT), L.stream()), "packT")
    return packed, packedT, ts


@pytest.mark.parametrize("scale", [1.0, 37.5])
def test_device_pack_equals_host_pack(ref_state, scale):
    """nerf_pack_weights / _transposed on the device (parallel statistics with atomicMax, then the
    fragment packs) equal the host packers word for word, except the row-L1 bound constants R_L,
    which the device sums lane-strided and the host sequentially (a few ulp apart; they only bound
    the activation split scale, a power of two, so the packed fragments are identical)."""
    L = _lib()
    lib, dev = L.load(), L.device()
    st = {k: v * (scale if i % 3 == 0 else 1.0) for i, (k, v) in enumerate(ref_state.items())}
    ts = [st[k].to(dev).float().contiguous() for k in O.STATE_KEYS]
    darr = (ctypes.c_void_p * 24)(*[t.data_ptr() for t in ts])
    packed = torch.zeros(lib.nerf_packed_weights_floats(), device=dev)
    packedT = torch.zeros(lib.nerf_packed_transposed_floats(), device=dev)
    L.check(lib.nerf_pack_weights(darr, L.ptr(packed), L.stream()), "pack")
    L.check(lib.nerf_pack_weights_transposed(darr, L.ptr(packedT), L.stream()), "packT")
    hs = [st[k].float().contiguous() for k in O.STATE_KEYS]
    arr = (ctypes.c_void_p * 24)(*[t.data_ptr() for t in hs])
    hp = np.zeros(lib.nerf_packed_weights_floats(), np.float32)
    hT = np.zeros(lib.nerf_packed_transposed_floats(), np.float32)
    assert lib.nerf_pack_weights_host(arr, hp.ctypes.data) == 0
    assert lib.nerf_pack_weights_transposed_host(arr, hT.ctypes.data) == 0
    torch.cuda.synchronize()
    dp = packed.cpu().numpy()
    diff = np.nonzero(dp.view(np.uint32) != hp.view(np.uint32))[0]
    assert len(diff) <= 8, diff[:20]                       # at most the 8 trunk layers' R_L
    assert np.all(np.abs(dp[diff] - hp[diff]) <= 1e-6 * np.abs(hp[diff])), (dp[diff], hp[diff])
    assert np.array_equal(packedT.cpu().numpy().view(np.uint32), hT.view(np.uint32))


# ----------------------------------------------------------------------------- composite backward
@pytest.mark.parametrize("N", [1, 2, 7, 64, 100, 200])
def test_composite_backward_matches_autograd(N):
    L = _lib()
    lib, dev = L.load(), L.device()
    B = 37
    g = torch.Generator().manual_seed(N)
    rgb = torch.rand(B, N, 3, generator=g)
    sigma = F.relu(torch.randn(B, N, 1, generator=g) * 3)
    z = torch.sort(2 + 4 * torch.rand(B, N, generator=g), dim=-1).values
    target = torch.rand(B, 3, generator=g)
    # oracle: autograd in float64 through the reference composite (render.py:56-80) + mse (train.py:87)
    r64, s64 = rgb.double().requires_grad_(True), sigma.double().requires_grad_(True)
    if N == 1:   # the reference's per-sample tensors are empty there: zero output, zero gradient
        exp_dr, exp_ds = np.zeros((B, N, 3)), np.zeros((B, N))
        rgb_map_ref = torch.zeros(B, 3, dtype=torch.float64)
    else:
        rgb_map_ref, _, _ = O.composite(r64, s64, z.double())
        F.mse_loss(rgb_map_ref, target.double()).backward()
        exp_dr, exp_ds = r64.grad.numpy(), s64.grad[..., 0].numpy()
    rg, sg, zg = rgb.to(dev).contiguous(), sigma[..., 0].to(dev).contiguous(), z.to(dev).contiguous()
    rgb_map, depth = torch.empty(B, 3, device=dev), torch.empty(B, device=dev)
    L.check(lib.nerf_composite(L.ptr(rg), L.ptr(sg), L.ptr(zg), B, N, L.ptr(rgb_map), L.ptr(depth), None,
                               L.stream()), "composite")
    tg = target.to(dev)
    ds, dr, sq = torch.empty(B, N, device=dev), torch.empty(B, N, 3, device=dev), torch.empty(B, device=dev)
    L.check(lib.nerf_composite_backward(L.ptr(rg), L.ptr(sg), L.ptr(zg), L.ptr(rgb_map), L.ptr(tg), B, N,
                                        2.0 / (3 * B), L.ptr(ds), L.ptr(dr), L.ptr(sq), L.stream()), "bwd")
    torch.cuda.synchronize()
    np.testing.assert_allclose(sq.cpu().numpy(), ((rgb_map_ref.detach() - target.double()) ** 2).sum(-1).numpy(),
                               rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(dr.cpu().numpy(), exp_dr, rtol=1e-4, atol=1e-8)
    np.testing.assert_allclose(ds.cpu().numpy(), exp_ds, rtol=1e-3, atol=1e-8 + 1e-4 * np.abs(exp_ds).max())


# --------------------------------------------------------------------------------- MLP backward
def check_mask_words(sv, mk):
    """The f16x3 forward's mask rows: bit (layer l, half h, tile T, quarter q, element e) ==
    [h_l[32T + 8q + 4h + e] > 0]; r_dir likewise (include/nerfmi_train.h NERF_MASK_ROW)."""
    words = mk.contiguous().numpy().view(np.uint32)
    offs = [0, 256, 512, 768, 1088, 1344, 1600, 1856]
    groups = [(8 * l, sv[:, off:off + 256].numpy() > 0, 8) for l, off in enumerate(offs)]
    groups.append((64, sv[:, 2144:2272].numpy() > 0, 4))          # r_dir: 8 bytes per half
    for w0, act, ntiles in groups:
        for hh in range(2):
            w = words[:, w0 + (ntiles // 2) * hh: w0 + (ntiles // 2) * (hh + 1)]
            for T in range(ntiles):
                bits16 = (w[:, T // 2] >> (16 * (T % 2))) & 0xFFFF
                for q in range(4):
                    for e in range(4):
                        got = ((bits16 >> (4 * q + e)) & 1).astype(bool)
                        assert np.array_equal(got, act[:, 32 * T + 8 * q + 4 * hh + e]), (w0, hh, T, q, e)


def _draw(R, N, seed, place=None):
    """Random rays (o, d, sorted z in [2, 6]) and upstream gradients of their R*N samples.  place:
    (o, d, z) -> (o, d, z), moves rays after the draw (test_gpu_pe_range.py: per-ray origin offsets
    that put samples beyond the fast sin/cos range); the random stream is the same with and without."""
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(R, 3, generator=g) * 0.3
    d = F.normalize(torch.randn(R, 3, generator=g), dim=-1)
    z = torch.sort(2 + 4 * torch.rand(R, N, generator=g), dim=-1).values
    if place is not None:
        o, d, z = place(o, d, z)
    return o, d, z, torch.randn(R * N, 3, generator=g), torch.randn(R * N, generator=g)


def _safe_draw(state, app, R, N, seed, rel=1e-5, place=None):
    """_draw, keeping only rays none of whose float64 ReLU pre-activations lies within rel x (that
    layer's rms) of the kink: there an fp32 evaluation may land on either side (the CPU's and the
    GPU's roundings differ by host), which moves that sample's whole gradient chain and makes a
    tensor's error a lottery instead of a measurement.  place (see _draw) moves the candidates before
    the filter, so the rays kept are clear of the kinks where they end up."""
    K = 8 * R                       # candidates (a 64-sample ray clears every kink ~1 time in 4)
    o, d, z, gr, gs = _draw(K, N, seed, place)
    pts = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3)
    dexp = d[:, None, :].expand(K, N, 3).reshape(-1, 3)
    a = None if app is None else (app.double() if app.dim() == 1 else None)
    pres = []
    with torch.no_grad():
        O.nerf_forward({k: v.double() for k, v in state.items()}, pts.double(), dexp.double(), a, keep=pres)
    ok = torch.ones(K, dtype=torch.bool)
    for p_ in pres:
        ok &= ((p_.abs() / p_.pow(2).mean().sqrt()) > rel).reshape(K, -1).all(dim=1)
    keep = torch.nonzero(ok)[:, 0][:R]
    assert keep.numel() == R, f"only {keep.numel()} of {K} rays clear the ReLU kinks"
    samp = (keep[:, None] * N + torch.arange(N)).reshape(-1)
    return o[keep], d[keep], z[keep], gr[samp], gs[samp]


def _mlp_forward_backward(state, app, R=96, N=11, seed=3, draw=None):
    """GPU forward-with-saves + data-gradient chain on random points, and the float64 autograd of
    the oracle's NeRF.forward on the same points (draw: the rays and upstream gradients, else _draw)."""
    L = _lib()
    lib, dev = L.load(), L.device()
    o, d, z, g_rgb, g_sigma = _draw(R, N, seed) if draw is None else draw
    M = R * N
    packed, packedT, _ = packed_of(state, dev)
    og, dg, zg = o.to(dev), d.to(dev), z.to(dev).contiguous()
    per_ray = app is not None and app.dim() == 2 and app.shape[0] == R   # one appearance row per ray
    a, rows = (None, 0) if app is None else (app.reshape(-1, 32).to(dev).contiguous(), R if per_ray else 1)
    feat, encd = torch.empty(R, 256, device=dev), torch.empty(R, 32, device=dev)
    rgb, sigma = torch.empty(M, 3, device=dev), torch.empty(M, device=dev)
    save = torch.empty(L.tile_rows(M), L.SAVE_ROW, device=dev)
    masks = torch.empty(M, L.MASK_ROW, dtype=torch.int32, device=dev)
    grad = torch.zeros(L.tile_rows(M), L.GRAD_ROW, device=dev)
    s = L.stream()
    L.check(lib.nerf_ray_features_train(L.ptr(packed), L.ptr(dg), R, L.ptr(a), rows, L.ptr(feat), L.ptr(encd), s),
            "feat")
    L.check(lib.nerf_mlp_forward_train(L.ptr(packed), L.ptr(og), L.ptr(dg), L.ptr(zg), R, N, L.ptr(feat),
                                       L.ptr(encd), L.ptr(rgb), L.ptr(sigma), L.ptr(save), L.ptr(masks), s), "fwd")
    ggr, ggs = g_rgb.to(dev), g_sigma.to(dev)
    f16 = L.get_mlp_arith() == "f16x3"
    L.check(lib.nerf_mlp_backward(L.ptr(packed), L.ptr(packedT), L.ptr(save), L.ptr(masks) if f16 else None,
                                  L.ptr(sigma), L.ptr(rgb), L.ptr(ggs), L.ptr(ggr), M, L.ptr(grad), s), "bwd")
    if f16:   # the activation-mask path of the same kernel gives the same gradient rows
        grad2 = torch.zeros_like(grad)
        L.check(lib.nerf_mlp_backward(L.ptr(packed), L.ptr(packedT), L.ptr(save), None, L.ptr(sigma), L.ptr(rgb),
                                      L.ptr(ggs), L.ptr(ggr), M, L.ptr(grad2), s), "bwd")
    torch.cuda.synchronize()
    if f16:
        # the mask-row kernel splits each layer's gradient at a scale from a bound, the activation-mask
        # kernel at the exact row maximum: the same gradient up to the split's rounding
        g1, g2 = L.untile(grad.cpu(), M).numpy(), L.untile(grad2.cpu(), M).numpy()
        for l in range(9):
            sl = slice(256 * l, 256 * l + (256 if l < 8 else 128))
            assert rel_l2(g1[:, sl], g2[:, sl]) < 1e-5, (l, rel_l2(g1[:, sl], g2[:, sl]))
        assert np.all(g2[:, 2177] == 0)   # the activation-mask kernel records no block exponents
        check_mask_words(L.untile(save.cpu(), M), masks.cpu())
    # oracle in float64 on the points the kernel evaluated (o + d z in fp32, render.py:22 / ray_utils.py:86)
    pts = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3)
    dexp = d[:, None, :].expand(R, N, 3).reshape(-1, 3)
    st64 = {k: v.double().requires_grad_(True) for k, v in state.items()}
    pres = []
    app_o = None if app is None else (app[:, None, :].expand(R, N, 32).reshape(-1, 32) if per_ray else app)
    rgb_o, sigma_o = O.nerf_forward(st64, pts.double(), dexp.double(), None if app is None else app_o.double(),
                                    keep=pres)
    for t in pres:
        t.retain_grad()
    ((rgb_o * g_rgb.double()).sum() + (sigma_o[:, 0] * g_sigma.double()).sum()).backward()
    return dict(rgb=rgb.cpu(), sigma=sigma.cpu(), save=L.untile(save.cpu(), M), grad=L.untile(grad.cpu(), M),
                save_tiled=save.cpu(), grad_tiled=grad.cpu(), encd=encd.cpu(), pts=pts,
                dexp=dexp, rgb_o=rgb_o.detach(), sigma_o=sigma_o.detach(), pres=pres, st64=st64)


@pytest.mark.parametrize("with_app,N", [(False, 11), (True, 11), (True, 64)])
def test_forward_saves_are_the_activations(ref_state, app_vec, with_app, N):
    """N = 64: a wave's 32 samples share one ray (the f16x3 kernel's LDS feature path)."""
    r = _mlp_forward_backward(ref_state, app_vec if with_app else None, R=40 if N == 64 else 96, N=N)
    saves_are_the_activations(r, N)


def saves_are_the_activations(r, N):
    """The checks of test_forward_saves_are_the_activations on a result of _mlp_forward_backward."""
    np.testing.assert_allclose(r["rgb"].numpy(), r["rgb_o"].numpy(), rtol=1e-4, atol=1e-6)
    save = r["save"].numpy()
    offs = [0, 256, 512, 768, 1088, 1344, 1600, 1856]
    for l, off in enumerate(offs):
        h = F.relu(r["pres"][l]).detach().numpy()
        assert rel_l2(save[:, off:off + 256], h) < 1e-5, l
    enc_x = O.positional_encoding(r["pts"], 10).numpy()
    np.testing.assert_allclose(save[:, 1024:1087], enc_x, rtol=1e-5, atol=2e-6)
    # enc_x's pad slot: the block exponent records of h_0..h_7 and enc_x under f16x3 (layout.h), else
    # the zero pad
    if _lib().get_mlp_arith() == "f16x3":
        exp = block_records(save, [slice(o, o + 256) for o in offs] + [slice(1024, 1087)])
        np.testing.assert_array_equal(save[:, 1087], exp)
    else:
        assert np.all(save[:, 1087] == 0)
    # enc_d: every row when N < 32, else each ray's first row only (layout.h kEncDPerRayMinN)
    first = slice(None) if N < 32 else slice(0, None, N)
    enc_d = O.positional_encoding(r["dexp"], 4).numpy()
    np.testing.assert_allclose(save[first, 2112:2139], enc_d[first], rtol=1e-5, atol=2e-6)
    assert np.all(save[first, 2139:2144] == 0)


def test_gradient_block_records(ref_state, app_vec):
    """The f16x3 data-gradient kernel records each block's exponent of d pre_1..7, [d pre_dir |
    d sigma] and d pre_0 in the gradient rows' padding (layout.h); the activation-mask kernel and the
    f32 path leave the slots 0 (absent), so the weight gradients find the maxima themselves."""
    r = _mlp_forward_backward(ref_state, app_vec, R=40, N=64)
    grad = r["grad"].numpy()
    slot = 2177
    if _lib().get_mlp_arith() == "f16x3":
        slices = [slice(256 * (j + 1), 256 * (j + 2)) for j in range(7)] + [slice(2048, 2177), slice(0, 256)]
        np.testing.assert_array_equal(grad[:, slot], block_records(grad, slices))
    else:
        assert np.all(grad[:, slot] == 0)


def no_worse_on_own_branches(got, f64_got, ref, f64_ref, name, factor=2.0, floor=1e-6):
    """got (the GPU) against float64 on the GPU's own ReLU branches is no further than ref (the fp32 CPU
    autograd) against float64 on the CPU's branches: within factor x the CPU's + floor in rel-L2 and in
    the max, p99.9 and median of the per-entry error (relative to the tensor's largest float64 entry):
    test_gpu_accuracy.py's criterion (2x CPU + 1e-6) applied to every statistic.
    Kink-proof as test_gpu_accuracy's gradient test: a pre-activation within rounding of 0 costs each
    evaluation its rounding, not a jump between the linear pieces of two branches.
    Why a floor (profiles/r05/pytest_train_tight*.log, diag_dir_grads*.log, composite_bias_hosts.log):
    the data-gradient rows of both GPU arithmetics sit at 1.2-1.5x the CPU's error (the MFMA's f32
    accumulation is not correctly rounded; the exact-f32 path shows it too), and the head gradients
    (dir_linear, rgb_linear and appearance_projection biases, the appearance row: sums over every
    sample of rows) carry the composite's mean error, a draw of the host: on one batch's inputs
    torch's CPU float exp gave rgb_map a mean error of +6e-8 on the GPU box and +2.6e-6 in the build
    container, the GPU's correctly rounded exp +2.8e-7 on both.  Such tensors land at 2-4x the CPU's
    draw, at 1-4e-7 absolute; a real fault (a wrong mask, scale or dropped product) costs >= 1e-5."""
    got, f64_got, ref, f64_ref = (np.asarray(t, np.float64).ravel() for t in (got, f64_got, ref, f64_ref))
    sc = max(np.abs(f64_got).max(), np.abs(f64_ref).max()) + 1e-300
    eg, er = np.abs(got - f64_got) / sc, np.abs(ref - f64_ref) / sc
    stats = [("max", np.max), ("p99.9", lambda v: np.quantile(v, 0.999)), ("median", np.median)]
    line = [f"{n}: {float(f(eg)):.3g}/{float(f(er)):.3g}" for n, f in stats]
    line.append(f"rel-L2: {rel_l2(got, f64_got):.3g}/{rel_l2(ref, f64_ref):.3g}")
    print(f"{name} (gpu/cpu vs float64) " + "  ".join(line))
    for stat, f in stats:
        assert f(eg) <= factor * f(er) + floor, (name, stat, float(f(eg)), float(f(er)))
    assert rel_l2(got, f64_got) <= factor * rel_l2(ref, f64_ref) + floor, (name, rel_l2(got, f64_got), rel_l2(ref, f64_ref))


def gpu_step_masks(tr, o, d, t_rand, app_idx):
    """The ten ReLU branches (trunk layers 0-7, density, dir_linear; models.py:128-150) the trainer's
    forward takes on this batch at its current packing: the same kernels on the same inputs
    (normalise, stratified samples on t_rand, ray features, forward with saves; nerf_train_forward's
    sequence), read from the saved activations (ReLU output > 0, the mask its backward applies)."""
    from nerfmi.ray_utils import linspace_table
    L = _lib()
    lib, P, s, dev = L.load(), L.ptr, L.stream(), tr.dev
    N = tr.config.num_samples
    o = o.reshape(-1, 3).to(dev, torch.float32).contiguous()
    d = d.reshape(-1, 3).to(dev, torch.float32).contiguous()
    B = o.shape[0]
    M = B * N
    dn, z = torch.empty(B, 3, device=dev), torch.empty(B, N, device=dev)
    feat, encd = torch.empty(B, 256, device=dev), torch.empty(B, 32, device=dev)
    rgb, sigma = torch.empty(M, 3, device=dev), torch.empty(M, device=dev)
    save = torch.empty(L.tile_rows(M), L.SAVE_ROW, device=dev)
    masks = torch.empty(M, L.MASK_ROW, dtype=torch.int32, device=dev)
    app, rows = (tr.appearance_embeddings[int(app_idx)].reshape(1, 32), 1) if (tr.n_images and app_idx is not None) \
        else (None, 0)
    tr_ = t_rand.to(dev, torch.float32).contiguous()
    L.check(lib.nerf_normalize_dirs(P(d), B, P(dn), s), "normalize")
    L.check(lib.nerf_sample_stratified(P(o), P(dn), B, tr.near, tr.far, N, P(linspace_table(N, dev)), 1, P(tr_), 0,
                                       P(z), None, s), "stratified")
    L.check(lib.nerf_ray_features_train(P(tr.packed), P(dn), B, P(app), rows, P(feat), P(encd), s), "features")
    L.check(lib.nerf_mlp_forward_train(P(tr.packed), P(o), P(dn), P(z), B, N, P(feat), P(encd), P(rgb), P(sigma),
                                       P(save), P(masks), s), "mlp_forward_train")
    torch.cuda.synchronize()
    r = L.untile(save.cpu(), M)
    offs = [0, 256, 512, 768, 1088, 1344, 1600, 1856]
    return [r[:, a:a + 256] > 0 for a in offs] + [(sigma.cpu() > 0).reshape(M, 1), r[:, 2144:2272] > 0]


def step_refs(state, table, app_idx, o, d, target, t_rand, m_gpu, name="step"):
    """One training step's gradients at `state` (+ appearance table): the oracle's fp32 autograd (its
    own branches, recorded), float64 on those branches, and float64 on the GPU's branches m_gpu.  The
    GPU's branches are first held to the CPU's (assert_branch_flips_bounded)."""
    def hook(masks=None, record=None, pres=None):
        def relu(pre, i):
            if record is not None:
                record.append(pre.detach() > 0)
            if pres is not None:
                pres.append(pre.detach())
            return torch.relu(pre) if masks is None else pre * masks[i].to(pre.dtype)
        return relu

    def run(dtype, relu):
        st = {k: v.detach().to(dtype).clone() for k, v in state.items()}
        tab = None if table is None else table.detach().to(dtype).clone()
        _, _, g, _ = O.train_step(st, tab, app_idx, o.cpu().to(dtype), d.cpu().to(dtype), target.cpu().to(dtype), 2.0,
                                  6.0, 64, t_rand.cpu().to(dtype), relu=relu)
        return {k: v.detach().double().numpy() for k, v in g.items()}
    m_cpu, pre64 = [], []
    g32 = run(torch.float32, hook(record=m_cpu))
    g64c = run(torch.float64, hook(masks=m_cpu, pres=pre64))
    assert_branch_flips_bounded(m_cpu, m_gpu, pre64, name)
    return g32, g64c, run(torch.float64, hook(masks=m_gpu))


def _data_grads(st, r, app, g_rgb, g_sigma, dtype, masks=None, record=None, pre_out=None):
    """d (sum rgb g_rgb + sigma g_sigma) / d pre_l, l = 0..7, of the oracle's NeRF.forward in `dtype` on
    the points of `r`, on the ReLU branches `masks` (None: its own; `record` collects them, `pre_out` the
    ten pre-activations)."""
    sd = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in st.items()}
    pres = []

    def relu(pre, i):
        if record is not None:
            record.append(pre.detach() > 0)
        if pre_out is not None:
            pre_out.append(pre.detach())
        return torch.relu(pre) if masks is None else pre * masks[i].to(dtype)
    with torch.enable_grad():
        rgb, sigma = O.nerf_forward(sd, r["pts"].to(dtype), r["dexp"].to(dtype), None if app is None else app.to(dtype),
                                    keep=pres, relu=relu)
        for t in pres:
            t.retain_grad()
        ((rgb * g_rgb.to(dtype)).sum() + (sigma[:, 0] * g_sigma.to(dtype)).sum()).backward()
    return [t.grad.double().numpy() for t in pres]


@pytest.mark.parametrize("with_app", [False, True])
def test_mlp_backward_matches_autograd(ref_state, app_vec, with_app):
    """The data-gradient rows d pre_0..7 against float64, each fp32 evaluation on its own ReLU branches
    (the GPU's read from its saved activations): no worse than the fp32 CPU autograd."""
    app = app_vec if with_app else None
    R, N = 96, 11
    draw = _draw(R, N, 3)
    r = _mlp_forward_backward(ref_state, app, R=R, N=N, draw=draw)
    data_grads_match_autograd(ref_state, app, r, draw, f"data gradients, app={with_app}")


def data_grads_match_autograd(ref_state, app, r, draw, name):
    """The check of test_mlp_backward_matches_autograd on a result r of _mlp_forward_backward(draw=draw)."""
    g_rgb, g_sigma = draw[3], draw[4]
    save, M = r["save"].numpy(), draw[2].numel()
    offs = [0, 256, 512, 768, 1088, 1344, 1600, 1856]
    m_gpu = [torch.from_numpy(save[:, o:o + 256] > 0) for o in offs]
    m_gpu += [(r["sigma"] > 0).reshape(M, 1), torch.from_numpy(save[:, 2144:2272] > 0)]
    m_cpu, pre64 = [], []
    d32 = _data_grads(ref_state, r, app, g_rgb, g_sigma, torch.float32, record=m_cpu)
    d64_cpu = _data_grads(ref_state, r, app, g_rgb, g_sigma, torch.float64, masks=m_cpu, pre_out=pre64)
    assert_branch_flips_bounded(m_cpu, m_gpu, pre64, name)
    d64_gpu = _data_grads(ref_state, r, app, g_rgb, g_sigma, torch.float64, masks=m_gpu)
    grad = r["grad"].numpy()
    for l in range(8):
        no_worse_on_own_branches(grad[:, 256 * l: 256 * (l + 1)], d64_gpu[l], d32[l], d64_cpu[l], f"d pre_{l}")


@pytest.mark.parametrize("R,N", [(40, 64), (2048, 64)])
def test_param_grads_records_match_fallback(ref_state, app_vec, R, N):
    """The split-f16 weight gradient scales each chunk by its operands' largest exponents, taken from
    the producers' block records or, with the records absent, found by reading the chunk first.  Both
    give the same exponents, so every gradient is bit-identical (R = 2048: 1,024-sample chunks)."""
    L = _lib()
    lib, dev = L.load(), L.device()
    r = _mlp_forward_backward(ref_state, app_vec, R=R, N=N)
    M = R * N
    packed, _, ts = packed_of(ref_state, dev)
    a = app_vec.reshape(1, 32).to(dev).contiguous()
    dapp = torch.empty(1, 32, device=dev)
    ws = torch.empty(lib.nerf_param_grads_workspace_bytes(M), dtype=torch.uint8, device=dev)
    outs = []
    for absent in (False, True):
        save, grad = r["save_tiled"].to(dev), r["grad_tiled"].to(dev)
        if absent:   # the record slots (layout.h kMetaSaveF / kMetaGradF) zeroed: "absent"
            save.view(-1, L.SAVE_ROW // 8, 32, 8)[:, 1087 // 8, :, 1087 % 8] = 0.0
            grad.view(-1, L.GRAD_ROW // 8, 32, 8)[:, 2177 // 8, :, 2177 % 8] = 0.0
        grads = [torch.empty_like(t) for t in ts]
        arr = (ctypes.c_void_p * 24)(*[t.data_ptr() for t in grads])
        L.check(lib.nerf_param_grads(L.ptr(save), L.ptr(grad), M, N, L.ptr(a), 1, L.ptr(packed), arr, L.ptr(dapp),
                                     L.ptr(ws), ws.numel(), L.stream()), "param_grads")
        torch.cuda.synchronize()
        outs.append([g.cpu() for g in grads])
    for k, g1, g2 in zip(O.STATE_KEYS, *outs):
        assert torch.equal(g1, g2), k
        assert torch.isfinite(g1).all(), k


def test_pe_columns_follow_the_arithmetic(ref_state, app_vec):
    """Layer 0's weight gradient and the skip layer's PE columns (both d pre over enc_x, K = 63).  Under
    f32 nerf_param_grads runs them as two jobs of the f32 weight-gradient GEMM, so they equal
    nerf_wgrad on the same rows bit for bit; under f16x3 they run as one launch of the split
    arithmetic's pair kernel, held to float64 like every other tensor (test_param_grads_match_autograd)."""
    L = _lib()
    lib, dev = L.load(), L.device()
    R, N = 40, 64
    r = _mlp_forward_backward(ref_state, app_vec, R=R, N=N)
    M = R * N
    save, grad = r["save_tiled"].to(dev), r["grad_tiled"].to(dev)
    packed, _, ts = packed_of(ref_state, dev)
    grads = [torch.full_like(t, float("nan")) for t in ts]
    arr = (ctypes.c_void_p * 24)(*[t.data_ptr() for t in grads])
    a = app_vec.reshape(1, 32).to(dev).contiguous()
    ws = torch.empty(lib.nerf_param_grads_workspace_bytes(M), dtype=torch.uint8, device=dev)
    L.check(lib.nerf_param_grads(L.ptr(save), L.ptr(grad), M, N, L.ptr(a), 1, L.ptr(packed), arr, None,
                                 L.ptr(ws), ws.numel(), L.stream()), "param_grads")
    enc_x = r["save"][:, 1024:1088].contiguous().to(dev)   # (row length 64: the aligned GEMM, as the tile-major rows)
    outs = {}
    for name, a_cols in (("layer0", slice(0, 256)), ("skip_pe", slice(1024, 1280))):
        a_rows = r["grad"][:, a_cols].contiguous().to(dev)
        ow, ob = torch.empty(256, 63, device=dev), torch.empty(256, device=dev)
        wsw = torch.empty(lib.nerf_wgrad_workspace_bytes(M, 256, 63), dtype=torch.uint8, device=dev)
        L.check(lib.nerf_wgrad(L.ptr(a_rows), 256, 256, L.ptr(enc_x), 64, 63, 1, M, L.ptr(ow), L.ptr(ob), 0,
                               L.ptr(wsw), wsw.numel(), L.stream()), "wgrad")
        outs[name] = (ow, ob)
    torch.cuda.synchronize()
    got = {"layer0": (grads[0].cpu(), grads[1].cpu()), "skip_pe": (grads[8][:, 256:].cpu(), None)}
    for name in outs:
        w_ref, b_ref = outs[name][0].cpu(), outs[name][1].cpu()
        w_got, b_got = got[name]
        assert torch.isfinite(w_got).all(), name
        if L.get_mlp_arith() == "f32":
            assert torch.equal(w_got, w_ref), name
            assert b_got is None or torch.equal(b_got, b_ref), name
        else:
            exp = r["st64"]["pts_linears.0.weight" if name == "layer0" else "pts_linears.4.weight"].grad.numpy()
            exp = exp if name == "layer0" else exp[:, 256:]
            assert rel_l2(w_got.numpy(), exp) < 2e-4, (name, rel_l2(w_got.numpy(), exp))


def test_weight_gradient_small_rows_keep_relative_precision(ref_state):
    """Per-entry precision of the 256 x 256 weight gradients where one neuron's gradients and one
    activation column sit ~1e-6 (2^-20) below the rest.  Under f16x3 each operand carries one power-of-
    two scale per 2,048-sample chunk (wgrad.hip, h16_chunk_exps), so such a column's values keep their
    hi part but a subnormal lo part: its products carry a relative error up to ~2^(k-39) at 2^-k of the
    chunk's maximum (2^-19 here) instead of fp32's 2^-24.  Held, per entry and relative to the entry's
    sum of |a x| (an fp32 sum's own error scale), to 1e-5 in the small row, the small column and their
    crossing, and everywhere else to twice the fp32 CPU GEMM's error.  Production path: tile-major rows
    through nerf_param_grads (layer 1: d pre_1 over h_0), the records absent (the kernel's own chunk
    maxima, which equal the records')."""
    L = _lib()
    lib, dev = L.load(), L.device()
    R, N = 128, 64
    M = R * N
    g = torch.Generator().manual_seed(17)
    a = torch.randn(M, 256, generator=g)                        # d pre_1
    x = torch.relu(torch.randn(M, 256, generator=g))            # h_0
    n0, k0 = 77, 130
    a[:, n0] *= 2.0 ** -20
    x[:, k0] *= 2.0 ** -20
    save, grad = torch.zeros(M, L.SAVE_ROW), torch.zeros(M, L.GRAD_ROW)
    save[:, 0:256], grad[:, 256:512] = x, a
    save_t, grad_t = L.tile(save).to(dev), L.tile(grad).to(dev)
    packed, _, ts = packed_of(ref_state, dev)
    grads = [torch.full_like(t, float("nan")) for t in ts]
    arr = (ctypes.c_void_p * 24)(*[t.data_ptr() for t in grads])
    ws = torch.empty(lib.nerf_param_grads_workspace_bytes(M), dtype=torch.uint8, device=dev)
    L.check(lib.nerf_param_grads(L.ptr(save_t), L.ptr(grad_t), M, N, None, 0, L.ptr(packed), arr, None,
                                 L.ptr(ws), ws.numel(), L.stream()), "param_grads")
    torch.cuda.synchronize()
    got = grads[2].cpu().double().numpy()
    exp = (a.double().T @ x.double()).numpy()
    mag = (a.double().abs().T @ x.double().abs()).numpy() + 1e-300
    cpu = (a.T @ x).double().numpy()
    e_gpu, e_cpu = np.abs(got - exp) / mag, np.abs(cpu - exp) / mag
    small = np.zeros_like(e_gpu, dtype=bool)
    small[n0, :] = True
    small[:, k0] = True
    print(f"[{_lib().get_mlp_arith()}] small row/column: max {e_gpu[small].max():.3g} (cpu {e_cpu[small].max():.3g}); "
          f"rest: max {e_gpu[~small].max():.3g} (cpu {e_cpu[~small].max():.3g}); crossing {e_gpu[n0, k0]:.3g}")
    assert e_gpu[small].max() <= 1e-5, float(e_gpu[small].max())
    # (the rest: within twice the CPU's error + 1e-7 of the sum of |terms|, the floor for the exact-f32
    # path's f32 accumulation over 2,048-sample chunks: 8.7e-8 against the CPU's 3.7e-8, where f16x3's
    # double-reduced split products measure 1.4e-8, profiles/r06/a/pytest_train.log)
    for stat, f in (("max", np.max), ("p99.9", lambda v: np.quantile(v, 0.999))):
        assert f(e_gpu[~small]) <= 2 * f(e_cpu[~small]) + 1e-7, (stat, float(f(e_gpu[~small])), float(f(e_cpu[~small])))
    # the bias column (a's column sums, in double) and the untouched parameters stay finite
    np.testing.assert_allclose(grads[3].cpu().double().numpy(), a.double().sum(0).numpy(), rtol=1e-6,
                               atol=1e-6 * float(a.abs().sum(0).max()))


@pytest.mark.parametrize("with_app,R", [(False, 96), (True, 96), (True, 37)])
def test_param_grads_match_autograd(ref_state, app_vec, with_app, R):
    """nerf_param_grads (every weight gradient as an MFMA reduction) on the chain above.  R = 37: 407
    samples, so the whole-tile GEMMs run 26 chunks of 16 with a 7-sample last chunk, and the grid of
    the two-workgroups-per-CU kernel (rounded up to 8 chunks) has idle workgroups."""
    L = _lib()
    lib, dev = L.load(), L.device()
    app = app_vec if with_app else None
    N = 11
    r = _mlp_forward_backward(ref_state, app, R=R, N=N)
    save, grad = r["save_tiled"].to(dev), r["grad_tiled"].to(dev)
    packed, _, ts = packed_of(ref_state, dev)
    grads = [torch.empty_like(t) for t in ts]
    arr = (ctypes.c_void_p * 24)(*[t.data_ptr() for t in grads])
    a = None if app is None else app.reshape(1, 32).to(dev).contiguous()
    dapp = torch.empty(1, 32, device=dev)
    M = R * N
    ws = torch.empty(lib.nerf_param_grads_workspace_bytes(M), dtype=torch.uint8, device=dev)
    L.check(lib.nerf_param_grads(L.ptr(save), L.ptr(grad), M, N, L.ptr(a), 0 if a is None else 1, L.ptr(packed),
                                 arr, L.ptr(dapp), L.ptr(ws), ws.numel(), L.stream()), "param_grads")
    torch.cuda.synchronize()
    for k, gt in zip(O.STATE_KEYS, grads):
        if app is None and k.startswith("appearance_projection"):
            continue
        exp = r["st64"][k].grad.numpy()
        assert rel_l2(gt.cpu().numpy(), exp) < 2e-4, (k, rel_l2(gt.cpu().numpy(), exp))


def _oracle_grads_f32(state, app, R, N, draw):
    """The oracle's fp32 autograd on _mlp_forward_backward's points and upstream gradients."""
    o, d, z, g_rgb, g_sigma = draw
    pts = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3)
    dexp = d[:, None, :].expand(R, N, 3).reshape(-1, 3)
    per_ray = app is not None and app.dim() == 2 and app.shape[0] == R
    app_o = None if app is None else (app[:, None, :].expand(R, N, 32).reshape(-1, 32) if per_ray else app)
    sd = {k: v.detach().clone().float().requires_grad_(True) for k, v in state.items()}
    with torch.enable_grad():
        rgb_o, sigma_o = O.nerf_forward(sd, pts, dexp, app_o)
        ((rgb_o * g_rgb).sum() + (sigma_o[:, 0] * g_sigma).sum()).backward()
    return {k: v.grad.numpy() for k, v in sd.items() if v.grad is not None}


@pytest.mark.parametrize("N", [32, 40, 64])
@pytest.mark.parametrize("app_kind", ["broadcast", "per_ray", "none"])
def test_param_grads_ray_path(ref_state, app_vec, app_kind, N):
    """nerf_param_grads with N >= 32 samples per ray: the per-ray gradient sums (dir_linear's PE_4(d)
    columns, the appearance projection and the appearance rows as GEMMs over rays), dir/sigma on the
    whole-tile GEMM, the two-stream schedule.  N = 40: tile-major blocks straddle rays (ray_sums_kernel);
    N = 32 and 64 under f16x3: the fused sums (the dir/density launch's 8-sample sums of d pre_dir, the
    rgb head launch's d hd block sums, wgrad_head3_kernel<true>; N = 32: one ray per 32-sample block).
    Against the oracle's float64 autograd, and two calls bit-identical (fixed-order reductions on both
    streams)."""
    R = 48
    app = {"broadcast": app_vec, "per_ray": torch.randn(R, 32, generator=torch.Generator().manual_seed(5)),
           "none": None}[app_kind]
    draw = _safe_draw(ref_state, app, R, N, seed=3)
    r = _mlp_forward_backward(ref_state, app, R=R, N=N, draw=draw)
    param_grads_ray_path(ref_state, app, app_kind, R, N, draw, r)


def param_grads_ray_path(ref_state, app, app_kind, R, N, draw, r):
    """The checks of test_param_grads_ray_path on a result r of _mlp_forward_backward(draw=draw)."""
    L = _lib()
    lib, dev = L.load(), L.device()
    save, grad = r["save_tiled"].to(dev), r["grad_tiled"].to(dev)
    packed, _, ts = packed_of(ref_state, dev)
    M = R * N
    rows = 0 if app is None else (R if app_kind == "per_ray" else 1)
    a = None if app is None else app.reshape(-1, 32).to(dev).contiguous()
    ws = torch.empty(lib.nerf_param_grads_workspace_bytes(M), dtype=torch.uint8, device=dev)
    runs = []
    for _ in range(2):
        grads = [torch.full_like(t, float("nan")) for t in ts]
        arr = (ctypes.c_void_p * 24)(*[t.data_ptr() for t in grads])
        dapp = torch.full((max(rows, 1), 32), float("nan"), device=dev)
        L.check(lib.nerf_param_grads(L.ptr(save), L.ptr(grad), M, N, L.ptr(a), rows, L.ptr(packed), arr, L.ptr(dapp),
                                     L.ptr(ws), ws.numel(), L.stream()), "param_grads")
        torch.cuda.synchronize()
        runs.append(([g.cpu() for g in grads], dapp.cpu()))
    for k, g1, g2 in zip(O.STATE_KEYS, runs[0][0], runs[1][0]):
        if app is None and k.startswith("appearance_projection"):
            continue                                               # not on the path: left untouched
        assert torch.equal(g1, g2), k
    assert rows == 0 or torch.equal(runs[0][1], runs[1][1])
    # (rays near a ReLU kink are not drawn, _safe_draw; each tensor is held to 2e-4 or twice the CPU
    # fp32 autograd's error, whichever is larger)
    g32 = _oracle_grads_f32(ref_state, app, R, N, draw)
    for k, gt in zip(O.STATE_KEYS, runs[0][0]):
        if app is None and k.startswith("appearance_projection"):
            continue
        exp = r["st64"][k].grad.numpy()
        e_gpu, e_cpu = rel_l2(gt.numpy(), exp), rel_l2(g32[k], exp)
        print(f"{k}: rel-L2 vs float64  gpu {e_gpu:.3g}  cpu fp32 {e_cpu:.3g}")
        assert e_gpu < max(2e-4, 2 * e_cpu), (k, e_gpu, e_cpu)
    if rows:
        # d app_row(r) = W_app^T sum over the ray's samples of d hd (broadcast: over all samples)
        W = r["st64"]["appearance_projection.weight"].detach()
        dhd = r["grad"][:, 2184:2312].double()                        # layout.h kGradHd
        s_r = dhd.reshape(R, N, 128).sum(1) if rows == R else dhd.sum(0, keepdim=True)
        exp_app = (s_r @ W).numpy()
        assert rel_l2(runs[0][1].numpy(), exp_app) < 1e-5, rel_l2(runs[0][1].numpy(), exp_app)


def test_wgrad_generic_shapes():
    """nerf_wgrad on ragged shapes: N, K not multiples of the tile, a sample count that is not a
    multiple of the chunk or of 2, per-row / broadcast x, accumulate."""
    L = _lib()
    lib, dev = L.load(), L.device()
    g = torch.Generator().manual_seed(9)
    for (M, N, K, xdiv) in [(1, 1, 1, 1), (4099, 33, 70, 1), (5000, 3, 128, 1), (3000, 128, 32, 10), (777, 5, 9, 0),
                            # the whole-tile and K <= 64 kernels on a partial chunk / ragged chunks
                            (700, 256, 256, 1), (33, 256, 256, 1), (3000, 160, 256, 1), (5003, 256, 40, 1),
                            (17, 256, 64, 1),
                            # the production step's shapes: 4096 rays x 64 samples = 262,144 rows
                            (262144, 256, 256, 1), (262144, 256, 63, 1), (262144, 3, 128, 1),
                            (262144, 128, 32, 64), (262147, 1, 256, 1),
                            # 3 tiles of 128 x 128 (the dir layer): slot-filling chunk length
                            (262144, 128, 288, 1), (50000, 128, 288, 1),
                            # 256 x 64 tiles on aligned row-major rows with one x row per sample (lda 128, ldx 64);
                            # the shortest chunk, two and a half stages
                            (100, 125, 62, 1), (40, 125, 62, 1)]:
        a = torch.randn(M, N + 3, generator=g)
        xr = 1 if xdiv == 0 else (M + xdiv - 1) // xdiv if xdiv > 1 else M
        x = torch.randn(xr, K + 2, generator=g)
        idx = torch.zeros(M, dtype=torch.long) if xdiv == 0 else torch.arange(M) // xdiv
        exp_w = (a[:, :N].double().T @ x[idx, :K].double()).numpy()
        exp_b = a[:, :N].double().sum(0).numpy()
        ag, xg = a.to(dev), x.to(dev)
        ow, ob = torch.full((N, K), 1.0, device=dev), torch.full((N,), 1.0, device=dev)
        ws = torch.empty(lib.nerf_wgrad_workspace_bytes(M, N, K), dtype=torch.uint8, device=dev)
        for acc in (0, 1):
            L.check(lib.nerf_wgrad(L.ptr(ag), N + 3, N, L.ptr(xg), K + 2, K, xdiv, M, L.ptr(ow), L.ptr(ob), acc,
                                   L.ptr(ws), ws.numel(), L.stream()), "wgrad")
        torch.cuda.synchronize()
        if M < 10000:
            np.testing.assert_allclose(ow.cpu().numpy(), 2 * exp_w, rtol=1e-4, atol=1e-3)
            np.testing.assert_allclose(ob.cpu().numpy(), 2 * exp_b, rtol=1e-4, atol=1e-3)
        else:
            # sums of 50K-262K products: an entry near 0 by cancellation has no relative accuracy in any
            # fp32 order, so each entry's error is measured against its sum of |terms| (the scale of
            # an fp32 summation's error): every entry within 1e-6 of it, and the max and p99.9 of that
            # per-entry error no worse than twice the CPU fp32 GEMM's (a regression in the bf16x6
            # split or the chunk reduction shows up there first)
            ad, xd = a[:, :N].abs().double(), x[idx, :K].abs().double()
            mag_w, mag_b = (ad.T @ xd).numpy(), ad.sum(0).numpy()
            cpu_w = (a[:, :N].T @ x[idx, :K]).double().numpy()
            cpu_b = a[:, :N].sum(0).double().numpy()
            for got, exp, mag, cpu, name in ((ow.cpu().numpy() / 2, exp_w, mag_w, cpu_w, "w"),
                                             (ob.cpu().numpy() / 2, exp_b, mag_b, cpu_b, "b")):
                r_gpu = (np.abs(got - exp) / mag).ravel()
                r_cpu = (np.abs(cpu - exp) / mag).ravel()
                assert r_gpu.max() <= 1e-6, (M, N, K, name, r_gpu.max())
                for stat, f in (("max", np.max), ("p99.9", lambda v: np.quantile(v, 0.999))):
                    g_, c_ = float(f(r_gpu)), float(f(r_cpu))
                    print(f"wgrad M={M} N={N} K={K} {name} {stat}: gpu {g_:.3g} cpu {c_:.3g}")
                    assert g_ <= 2 * c_ + 1e-9, (M, N, K, name, stat, g_, c_)


def test_adam_matches_torch():
    L = _lib()
    lib, dev = L.load(), L.device()
    g = torch.Generator().manual_seed(4)
    p0 = torch.randn(10007, generator=g)
    p_ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p_ref], lr=5e-4)
    p, m, v = p0.to(dev), torch.zeros(10007, device=dev), torch.zeros(10007, device=dev)
    for step in range(1, 6):
        gr = torch.randn(10007, generator=g) * (10.0 ** -step)
        gr[::7] = 0
        p_ref.grad = gr.clone()
        opt.step()
        gg = gr.to(dev)
        L.check(lib.nerf_adam(L.ptr(p), L.ptr(gg), L.ptr(m), L.ptr(v), 10007, 5e-4, 0.9, 0.999, 1e-8, step,
                              L.stream()), "adam")
    torch.cuda.synchronize()
    st = opt.state[p_ref]
    m_ref, v_ref = st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()
    np.testing.assert_allclose(m.cpu().numpy(), m_ref, rtol=1e-6, atol=1e-6 * np.abs(m_ref).max())
    np.testing.assert_allclose(v.cpu().numpy(), v_ref, rtol=1e-6, atol=1e-6 * np.abs(v_ref).max())
    np.testing.assert_allclose(p.cpu().numpy(), p_ref.detach().numpy(), rtol=1e-6, atol=1e-7)


# ------------------------------------------------------------------------------- whole step
def _trainer(ref_state, n_images=100):
    import nerfmi
    from nerfmi.train import Trainer
    torch.manual_seed(0)
    model = nerfmi.NeRF(nerfmi.Config())
    model.load_state_dict(ref_state)
    torch.manual_seed(1)
    table = torch.randn(n_images, 32)
    return Trainer(nerfmi.Config(), model=model, appearance_embeddings=table), table


def _params_close(got, exp, steps, name, frac=0.999, lr=5e-4, rel_g=None, rel_g_max=1e-3):
    """Adam normalises each gradient entry by its own RMS, so an entry whose true gradient is ~0
    (cancellation) moves by up to lr per step in whichever direction its rounding points: require
    almost all entries within 2e-6 and every entry within the 2*lr*steps such a flip can cause.
    With rel_g (per entry, the reference gradient's magnitude over the tensor's largest, the
    smallest over the steps), each entry off by more than 2e-6 must also be one whose reference
    gradient was ~0 (rel_g <= rel_g_max) at some step; frac=None drops the fraction test."""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(exp, np.float64))
    if frac is not None:
        assert (d <= 2e-6).mean() >= frac, (name, (d <= 2e-6).mean())
    if rel_g is not None:
        off = d > 2e-6
        r = np.asarray(rel_g, np.float64).reshape(d.shape)
        assert np.all(r[off] <= rel_g_max), (name, int(off.sum()), float(r[off].max()))
    assert d.max() <= 2 * lr * steps + 2e-6, (name, d.max())


def test_trainer_step_matches_reference_f7(golden, golden_meta, ref_state):
    """One full GPU training step (forward, loss, backward, Adam) on F7's inputs vs the reference's
    own loss, gradient norms, sampled gradients and updated parameters."""
    f7 = golden("f7_train_step.npz")
    meta = golden_meta["F7"]
    tr, _ = _trainer(ref_state)
    t_rand = seeded_uniform(meta["seed_t_rand"], (256, 64), meta["t_rand_sha256"])
    g64, p64 = f7_float64(ref_state, f7, meta)
    dev = tr.dev
    loss, rgb = tr.forward_backward(torch.from_numpy(f7["o"]).to(dev), torch.from_numpy(f7["d"]).to(dev),
                                    torch.from_numpy(f7["target"]).to(dev), 0, t_rand=t_rand)
    grads = {n: tr.view(tr.grad, i).detach().cpu().clone() for i, n in enumerate(meta["names"])}
    tr.optimizer_step()
    torch.cuda.synchronize()
    np.testing.assert_allclose(rgb.cpu().numpy(), f7["rgb"], rtol=1e-4, atol=1e-5)
    assert abs(float(loss) - meta["loss"]) <= 1e-5 * meta["loss"]
    for i, name in enumerate(meta["names"]):
        g = grads[name]
        n_ref = meta["grad_l2"][name]
        assert abs(float(g.double().norm()) - n_ref) <= 2e-4 * n_ref + 1e-12, (name, float(g.norm()), n_ref)
        prm = tr.view(tr.flat, i).detach().cpu()
        if f"idx/{name}" in f7:
            idx = torch.from_numpy(f7[f"idx/{name}"])
            grads_no_worse_than_reference(g.reshape(-1)[idx].numpy(), f7[f"grad/{name}"],
                                          g64[name].reshape(-1)[idx], name)
            params_no_worse_than_reference(prm.reshape(-1)[idx].numpy(), f7[f"param/{name}"],
                                           p64[name].reshape(-1)[idx], name)
        else:
            assert rel_l2(g.numpy(), f7[f"grad/{name}"]) < 5e-4, name
            ga = np.abs(f7[f"grad/{name}"].astype(np.float64))
            _params_close(prm.numpy(), f7[f"param/{name}"], 1, name, frac=None, rel_g=ga / max(ga.max(), 1e-30))


def test_trainer_matches_oracle_over_steps(ref_state):
    """Three consecutive steps on different images/batches against the oracle's torch-CPU
    training (autograd + torch.optim.Adam), including the appearance table."""
    from nerfmi import cameras, get_rays
    tr, table = _trainer(ref_state, n_images=4)
    st = {k: v.clone() for k, v in ref_state.items()}
    tab = table.clone()
    opt = None
    focal = cameras.synthetic_focal(800)
    g = torch.Generator().manual_seed(21)
    st64, tab64, opt64 = {k: v.double().clone() for k, v in ref_state.items()}, table.double().clone(), None
    for step in range(3):
        c2w = cameras.frame_c2w("chair", "circle", 10 * step, 120).float()
        o_all, d_all = get_rays(800, 800, focal, c2w.to(tr.dev))
        sel = torch.randperm(800 * 800, generator=g)[:512]
        o, d = o_all.reshape(-1, 3)[sel.to(tr.dev)], d_all.reshape(-1, 3)[sel.to(tr.dev)]
        target = torch.rand(512, 3, generator=g)
        t_rand = torch.rand(512, 64, generator=g)
        img = step % 4
        loss_o, _, grads_o, opt = O.train_step(st, tab, img, o.cpu(), d.cpu(), target, 2.0, 6.0, 64, t_rand,
                                               optimizer=opt)
        _, _, _, opt64 = O.train_step(st64, tab64, img, o.cpu().double(), d.cpu().double(), target.double(), 2.0, 6.0,
                                      64, t_rand.double(), optimizer=opt64)
        # this step's gradient references at the GPU's own current parameters (the trajectories part
        # by Adam's +-lr moves of ~0 gradients): the oracle's fp32 autograd and float64, each fp32
        # evaluation held to float64 on its own ReLU branches (no_worse_on_own_branches)
        names = list(O.STATE_KEYS) + ["appearance_embeddings"]
        cur = {n: tr.view(tr.flat, i).detach().cpu().clone() for i, n in enumerate(names)}
        loss, _ = tr.forward_backward(o, d, target.to(tr.dev), img, t_rand=t_rand)
        assert abs(float(loss) - float(loss_o)) <= 2e-5 * float(loss_o), step
        m_gpu = gpu_step_masks(tr, o, d, t_rand, img)
        g32, g64c, g64g = step_refs({k: cur[k] for k in O.STATE_KEYS}, cur["appearance_embeddings"], img, o, d, target,
                                    t_rand, m_gpu, name=f"step {step}")
        for i, n in enumerate(names):
            got = tr.view(tr.grad, i).detach().cpu().numpy()
            no_worse_on_own_branches(got, g64g[n], g32[n], g64c[n], f"step {step} {n}")
        tr.optimizer_step()
    torch.cuda.synchronize()
    names = list(O.STATE_KEYS) + ["appearance_embeddings"]
    params = dict(st, appearance_embeddings=tab)
    params64 = dict(st64, appearance_embeddings=tab64)
    for i, n in enumerate(names):
        got = tr.view(tr.flat, i).detach().cpu().numpy()
        exp = params[n].detach().numpy()
        # the GPU's three steps stay as close to the float64 trajectory as the oracle's fp32 CPU steps
        params_no_worse_than_reference(got, exp, params64[n].detach().numpy(), n)
        assert np.abs(got - exp).max() <= 2 * 5e-4 * 3 + 2e-6, n     # and within the flip bound of it


def test_training_reduces_loss_on_teacher_scene():
    """End to end on the synthetic teacher dataset (no dataset exists here): 40 iterations of 1024 rays."""
    import nerfmi
    from nerfmi.dataset import SyntheticNeRFDataset
    from nerfmi.train import Trainer
    cfg = nerfmi.Config()
    np.random.seed(0)
    ds = SyntheticNeRFDataset(cfg, n_images=4, H=64, W=64)
    torch.manual_seed(0)
    tr = Trainer(cfg, appearance_embeddings=ds.appearance_embeddings)
    losses = []
    for i in range(40):
        b = ds.get_rays(batch_size=1024)
        losses.append(float(tr.step(b["rays_o"], b["rays_d"], b["rgb"], b["appearance_idx"], seed=i + 1)))
    assert np.all(np.isfinite(losses))
    assert np.mean(losses[-5:]) < 0.7 * np.mean(losses[:5]), losses


def test_training_is_deterministic():
    """Two trainers from the same seed, 25 production-size steps (4,096 rays x 64 samples) each: the
    parameters, Adam moments and losses are bit-identical.  Every kernel of the step (the LDS-DMA
    weight streams with stores in flight, the two-stream parameter gradients, the side-stream
    packing) must order its memory exactly; a race shows up here as a difference, not as a tolerance
    miss."""
    import nerfmi
    from nerfmi.dataset import SyntheticNeRFDataset
    from nerfmi.train import Trainer
    cfg = nerfmi.Config()
    runs = []
    for _ in range(2):
        np.random.seed(0)
        torch.manual_seed(0)                        # (the dataset draws its appearance table from torch's RNG)
        ds = SyntheticNeRFDataset(cfg, n_images=3, H=96, W=96)
        torch.manual_seed(0)
        tr = Trainer(cfg, appearance_embeddings=ds.appearance_embeddings)
        losses = []
        for i in range(25):
            b = ds.get_rays(batch_size=4096)        # np.random, seeded above: the same batches both runs
            losses.append(float(tr.step(b["rays_o"], b["rays_d"], b["rgb"], b["appearance_idx"], seed=i + 1)))
        torch.cuda.synchronize()
        runs.append((tr.flat.detach().cpu().clone(), tr.exp_avg.detach().cpu().clone(),
                     tr.exp_avg_sq.detach().cpu().clone(), losses))
    assert runs[0][3] == runs[1][3]
    for a_, b_ in zip(runs[0][:3], runs[1][:3]):
        assert torch.equal(a_, b_)


def test_production_batch_matches_oracle(ref_state, app_vec):
    """The production step (config 5, train.py:77-92): 4096 rays x 64 samples = 262,144 MLP rows,
    the regime where the weight gradients run as 128 XCD-grouped chunks x 4 tiles with the
    per-launch chunk lengths and the deterministic chunk reduction.  Loss and every gradient
    against the oracle's autograd on the same rays, jitter and target."""
    from nerfmi import cameras, get_rays
    tr, table = _trainer(ref_state, n_images=3)
    focal = cameras.synthetic_focal(800)
    g = torch.Generator().manual_seed(31)
    c2w = cameras.frame_c2w("chair", "circle", 7, 120).float()
    o_all, d_all = get_rays(800, 800, focal, c2w.to(tr.dev))
    sel = torch.randperm(800 * 800, generator=g)[:4096]
    o, d = o_all.reshape(-1, 3)[sel.to(tr.dev)], d_all.reshape(-1, 3)[sel.to(tr.dev)]
    target = torch.rand(4096, 3, generator=g)
    t_rand = torch.rand(4096, 64, generator=g)
    st = {k: v.clone() for k, v in ref_state.items()}
    loss_o, _, grads_o, _ = O.train_step(st, table.clone(), 2, o.cpu(), d.cpu(), target, 2.0, 6.0, 64, t_rand)
    loss, _ = tr.forward_backward(o, d, target.to(tr.dev), 2, t_rand=t_rand)
    torch.cuda.synchronize()
    assert abs(float(loss) - float(loss_o)) <= 2e-5 * float(loss_o)
    m_gpu = gpu_step_masks(tr, o, d, t_rand, 2)
    g32, g64c, g64g = step_refs(ref_state, table, 2, o, d, target, t_rand, m_gpu, name="production batch")
    for i, n in enumerate(list(O.STATE_KEYS) + ["appearance_embeddings"]):
        got = tr.view(tr.grad, i).detach().cpu().numpy()
        no_worse_on_own_branches(got, g64g[n], g32[n], g64c[n], n)


def test_no_appearance_model_trains_like_the_oracle(noapp_state):
    """use_appearance=False (models.py:99-103): 22 parameters, no appearance table; one step's
    gradients and Adam update against the oracle."""
    import nerfmi
    from nerfmi import cameras, get_rays
    from nerfmi.train import Trainer
    cfg = nerfmi.Config()
    cfg.use_appearance = False
    torch.manual_seed(0)
    model = nerfmi.NeRF(cfg)
    tr = Trainer(cfg, model=model)
    assert tr.param_slots == [i for i, k in enumerate(O.STATE_KEYS) if not k.startswith("appearance_projection")]
    c2w = cameras.frame_c2w("chair", "circle", 3, 120).float()
    o_all, d_all = get_rays(800, 800, cameras.synthetic_focal(800), c2w.to(tr.dev))
    g = torch.Generator().manual_seed(5)
    sel = torch.randperm(800 * 800, generator=g)[:512].to(tr.dev)
    o, d = o_all.reshape(-1, 3)[sel], d_all.reshape(-1, 3)[sel]
    target = torch.rand(512, 3, generator=g)
    t_rand = torch.rand(512, 64, generator=g)
    st = {k: v.clone() for k, v in noapp_state.items()}
    loss_o, _, grads_o, opt = O.train_step(st, None, 0, o.cpu(), d.cpu(), target, 2.0, 6.0, 64, t_rand)
    st64 = {k: v.double().clone() for k, v in noapp_state.items()}
    O.train_step(st64, None, 0, o.cpu().double(), d.cpu().double(), target.double(), 2.0, 6.0, 64, t_rand.double())
    loss, _ = tr.forward_backward(o, d, target.to(tr.dev), 0, t_rand=t_rand)
    assert abs(float(loss) - float(loss_o)) <= 2e-5 * float(loss_o)
    for i, k in enumerate(O.STATE_KEYS):
        if k in noapp_state:
            got = tr.view(tr.grad, i).detach().cpu().numpy()
            assert rel_l2(got, grads_o[k].numpy()) < 5e-4, k
    tr.optimizer_step()
    sd = tr.optimizer_state_dict()
    assert len(sd["param_groups"][0]["params"]) == 22 and sorted(sd["state"]) == list(range(22))
    for k in noapp_state:
        params_no_worse_than_reference(model.state_dict()[k].cpu().numpy(), st[k].detach().numpy(),
                                       st64[k].detach().numpy(), k)
