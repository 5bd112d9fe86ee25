"""The MLP kernels on sample positions beyond the fast sin/cos range (csrc/pe_sin.h, |x| > 16).

Under f16x3 every MLP kernel forms the positional encoding with pe_sin_reduced while |x| 2^9 <= kPeSinMax
and with the library sincosf otherwise, and it chooses PER WAVE: an aligned group of 32 consecutive
samples (in the gathered kernels 32 consecutive compact rows) takes the library path as soon as one of
its samples is far.  The slow branches are hand-written loops of their own (mlp16_body.h; mlp16s_body.h's
`full` branch, which in the persistent render loop also recomputes an encoding the block before had
already prepared), so these tests put far samples where each of them runs.  pe_sin_reduced stays
accurate far beyond its range (9.3e-8 up to |x| = 1024), so accuracy cannot tell which path a wave
took; the targets are the slow branches' plumbing and the block transitions, where an error is gross.

Conditioning.  At |x| = 40 one ulp of x is 3.8e-6, 2e-3 rad at level 9, so a reference is only a
reference on the SAME fp32 positions: the given x for the point-wise forward, o + d z in fp32 (separate
roundings, bit-exact z, the kernels' own normalised directions) for rays, cast to float64 for the
float64 reference and fed as they are to the fp32 CPU oracle.  Hierarchical renders (whose fine depths
are not bit-exact between GPU and CPU) are not compared on far rays.  Bit equality is asserted only
between launches in which every wave compared holds the same samples.

G = the device's CU count; one render block is 128 samples (4 waves of 32)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import check_no_worse_than_cpu
from oracle import nerf_oracle as O
from test_gpu_train import (_mlp_forward_backward, _safe_draw, _draw, data_grads_match_autograd, packed_of,
                            param_grads_ray_path, saves_are_the_activations)
from test_gpu_train_occupancy import SENT, P, S, forward_n1, ok

pytestmark = pytest.mark.gpu

BLOCK = 128
LIMIT = 16.0            # kPeSinMax / 2^9: the kernels' test is |x| > LIMIT


@pytest.fixture(scope="module")
def nerfmi_mod():
    import nerfmi
    return nerfmi


@pytest.fixture(scope="module", autouse=True, params=["f16x3", "f32"])
def arith(request, nerfmi_mod):
    prev = nerfmi_mod.set_mlp_arith(request.param)
    yield request.param
    nerfmi_mod.set_mlp_arith(prev)


@pytest.fixture(scope="module")
def model(nerfmi_mod, ref_state):
    m = nerfmi_mod.NeRF(nerfmi_mod.Config())
    m.load_state_dict(ref_state)
    return m.cuda().eval().requires_grad_(False)


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def forward(model, x, d):
    with torch.no_grad():
        rgb, sigma = model(x.cuda(), d.cuda())
    return rgb.cpu(), sigma.cpu()


def far_mask(pts):
    """Samples the kernels call far (their own test, on the fp32 positions)."""
    return pts.abs().max(dim=-1).values > LIMIT


def wave_any(mask):
    """Per sample: does its wave (aligned 32 consecutive rows, the last one ragged) hold a True?"""
    M = mask.numel()
    pad = torch.zeros((M + 31) // 32 * 32, dtype=torch.bool)
    pad[:M] = mask
    return pad.reshape(-1, 32).any(1).repeat_interleave(32)[:M]


# ============================================================ A. the render forward (mlp16s_kernel / mlp.hip)
@pytest.fixture(scope="module")
def render_case(cus, ref_state):
    """An in-range batch X of 128 (3 G + 1) + 37 samples, its variant Xf with far samples in five chosen
    waves, the threshold variant Xt, and the float64 / fp32 oracle on a fixed subset of 4,096 samples of
    Xf holding every sample of the chosen waves.  Block b runs on workgroup b % G in round b // G."""
    G = cus
    assert G >= 8, G
    M = BLOCK * (3 * G + 1) + 37
    g = torch.Generator().manual_seed(31)
    X = torch.randn(M, 3, generator=g) * 2
    D = F.normalize(torch.randn(M, 3, generator=g), dim=-1)
    assert float(X.abs().max()) < LIMIT
    u = torch.rand(64, generator=g)
    Xf = X.clone()

    def wave_at(block, wave):
        return BLOCK * block + 32 * wave

    def far_val(k, sign):
        return sign * (16.0 + 48.0 * float(u[k]))

    waves = {}
    # a wave of block 0 (a workgroup's first block: the `full` path unconditionally), the only far wave of its
    # four; the far sample in sample tile 0 (the wave's samples 0-15)
    waves["block 0"] = w = wave_at(0, 1)
    Xf[w + 3, 0] = far_val(0, +1)
    # round 1 (reached through beyond_n only), the far sample in sample tile 1; the same workgroup's
    # block of round 2 stays in range, so it returns to the prepared encoding after a recomputed block
    waves["round 1"] = w = wave_at(G + 2, 2)
    Xf[w + 20, 1] = far_val(1, -1)
    # one workgroup, two consecutive rounds: every sample of the first wave far (all coordinates, both
    # signs, two at +-1000), three of the second
    waves["all far"] = w = wave_at(G + 3, 0)
    for i in range(32):
        Xf[w + i, i % 3] = far_val(2 + i, 1 - 2 * ((i // 3) % 2))
    Xf[w + 5, 2] = 1000.0
    Xf[w + 17, 2] = -1000.0
    waves["next round"] = w = wave_at(2 * G + 3, 3)
    Xf[w + 1, 2] = far_val(40, +1)
    Xf[w + 9, 0] = -1000.0
    Xf[w + 30, 1] = far_val(41, +1)
    # the ragged last block: the far sample is M - 1, which the padding lanes repeat
    waves["last"] = w = wave_at(3 * G + 1, 1)
    assert w <= M - 1 < w + 32
    Xf[M - 1, 2] = far_val(42, -1)

    chosen = torch.zeros(M, dtype=torch.bool)
    for w in waves.values():
        chosen[w:min(w + 32, M)] = True
    far = far_mask(Xf)
    assert torch.equal(wave_any(far), chosen)                 # the far samples lie in the chosen waves, in each of them
    assert int(far.sum()) == 1 + 1 + 32 + 3 + 1
    # threshold: a largest coordinate of exactly 16 is not `> 16`; two waves of otherwise untouched blocks
    Xt = X.clone()
    thr = (wave_at(1, 2) + 7, wave_at(G + 5, 1) + 25)
    Xt[thr[0], 0] = LIMIT
    Xt[thr[1], 2] = -LIMIT
    assert not bool(far_mask(Xt).any())

    rest = torch.nonzero(~chosen)[:, 0]
    fill = rest[torch.randperm(rest.numel(), generator=g)[:4096 - int(chosen.sum())]]
    idx = torch.cat([torch.nonzero(chosen)[:, 0], fill]).sort().values
    assert idx.numel() == 4096
    with torch.no_grad():
        rgb32, sig32 = O.nerf_forward(ref_state, Xf[idx], D[idx])
        rgb64, sig64 = O.nerf_forward({k: v.double() for k, v in ref_state.items()}, Xf[idx].double(), D[idx].double())
    return dict(G=G, M=M, X=X, D=D, Xf=Xf, Xt=Xt, thr=thr, waves=waves, chosen=chosen, far=far, idx=idx,
                ref=(rgb64, sig64, rgb32.double(), sig32.double()))


def forward_accuracy(rgb, sigma, ref, sel, what):
    """test_gpu_accuracy.py::test_forward's rule on the samples `sel` of the oracle subset: the largest rgb
    error against float64 within 4x the fp32 CPU oracle's + 1e-7, sigma's (relative, floored at 1e-3 of the
    largest sigma) within 4x + 1e-6."""
    rgb64, sig64, rgb32, sig32 = (t[sel] for t in ref)
    rgb, sigma = rgb[sel].double(), sigma[sel].double()
    e_gpu, e_cpu = float((rgb - rgb64).abs().max()), float((rgb32 - rgb64).abs().max())
    sc = float(sig64.abs().max()) + 1e-30
    s_gpu = float(((sigma - sig64).abs() / (sig64.abs() + 1e-3 * sc)).max())
    s_cpu = float(((sig32 - sig64).abs() / (sig64.abs() + 1e-3 * sc)).max())
    print(f"{what} ({rgb.shape[0]} samples): rgb max err vs f64 {e_gpu:.3g} (cpu f32 {e_cpu:.3g}); "
          f"sigma rel {s_gpu:.3g} (cpu {s_cpu:.3g}); sigma max {sc:.3g}")
    return (e_gpu, e_cpu, s_gpu, s_cpu)


def assert_forward_accuracy(figures, what):
    e_gpu, e_cpu, s_gpu, s_cpu = figures
    assert e_gpu <= 4 * e_cpu + 1e-7, (what, "rgb", e_gpu, e_cpu)
    assert s_gpu <= 4 * s_cpu + 1e-6, (what, "sigma", s_gpu, s_cpu)


@pytest.fixture(scope="module")
def render_runs(model, render_case, arith):
    """The launches on X and Xf, shared by the tests below (per arithmetic)."""
    c = render_case
    return forward(model, c["X"], c["D"]), forward(model, c["Xf"], c["D"])


def test_far_waves_leave_the_other_waves_untouched(render_case, render_runs, arith):
    """Far samples in five waves (a first block, a block reached through beyond_n, two consecutive rounds of
    one workgroup, the ragged tail): every sample of every other wave is bit-equal to the all-in-range
    launch, whatever its workgroup ran before or prepares next.  Under f32 (sincosf everywhere) so are the
    in-range samples of the chosen waves."""
    c = render_case
    (rgb, sigma), (rgb_f, sigma_f) = render_runs
    assert bool(torch.isfinite(rgb_f).all()) and bool(torch.isfinite(sigma_f).all())
    out = ~c["chosen"]
    assert torch.equal(rgb_f[out], rgb[out]) and torch.equal(sigma_f[out], sigma[out])
    mixed = c["chosen"] & ~c["far"]
    assert int(mixed.sum()) == 31 + 31 + 29 + 4
    if arith == "f32":
        assert torch.equal(rgb_f[mixed], rgb[mixed]) and torch.equal(sigma_f[mixed], sigma[mixed])
    else:
        same = int(((rgb_f[mixed] == rgb[mixed]).all(1) & (sigma_f[mixed] == sigma[mixed])[:, 0]).sum())
        print(f"f16x3: {same} of {int(mixed.sum())} in-range samples of the far waves keep the fast path's bits")
    # the far samples did change (the variant is not the base batch by accident)
    assert not torch.equal(rgb_f[c["far"]], rgb[c["far"]])


def test_far_and_neighbouring_samples_vs_float64(render_case, render_runs, arith):
    """Every sample of the chosen waves, far or in range, and ~3,900 others, against float64 on the same
    fp32 inputs by test_gpu_accuracy.py::test_forward's rule: on the whole subset, and again on the far
    samples alone and on their in-range neighbours in the far waves alone, so that the neighbours' sigma
    (below 0.02) is held at its own scale and not at the floor one far sample's sigma sets.  The figures
    of all in-range samples are printed only: almost all of them are bit-equal to the all-in-range launch,
    and with these random-init weights their sigmas stay below 0.025, so on that part the rule's floor of
    1e-3 of the largest sigma sits at fp32 rounding of the density head's sum and measures mlp.hip's
    accumulation order."""
    c = render_case
    idx = c["idx"]
    rgb_f, sigma_f = (t[idx] for t in render_runs[1])
    every = torch.ones(idx.numel(), dtype=torch.bool)
    far, chosen = c["far"][idx], c["chosen"][idx]
    figs = {name: forward_accuracy(rgb_f, sigma_f, c["ref"], sel, f"A/{arith} {name}")
            for name, sel in (("subset", every), ("in range", ~far), ("far", far), ("in range, far wave", chosen & ~far))}
    for name in ("subset", "far", "in range, far wave"):
        assert_forward_accuracy(figs[name], name)


def test_threshold_sample_keeps_its_wave_on_the_fast_path(model, render_case, render_runs):
    """A largest coordinate of exactly +-16.0f is not beyond the range (the kernels test `>`): the other 31
    samples of its wave, and every other sample, are bit-equal to the base launch."""
    c = render_case
    rgb, sigma = render_runs[0]
    rgb_t, sigma_t = forward(model, c["Xt"], c["D"])
    keep = torch.ones(c["M"], dtype=torch.bool)
    keep[list(c["thr"])] = False
    assert torch.equal(rgb_t[keep], rgb[keep]) and torch.equal(sigma_t[keep], sigma[keep])
    assert bool(torch.isfinite(rgb_t).all()) and bool(torch.isfinite(sigma_t).all())
    assert not torch.equal(rgb_t[~keep], rgb[~keep])


def test_far_waves_flipped_and_repeated(model, render_case, render_runs):
    """128 k samples reversed (waves stay waves, in other blocks, rounds and lanes), and the same launch
    twice: bit-equal."""
    c = render_case
    Mk = BLOCK * (3 * c["G"] + 1)
    x, d = c["Xf"][:Mk], c["D"][:Mk]
    assert int(c["far"][:Mk].sum()) == 37
    rgb, sigma = forward(model, x, d)
    rgb_r, sigma_r = forward(model, x.flip(0), d.flip(0))
    assert torch.equal(rgb_r.flip(0), rgb) and torch.equal(sigma_r.flip(0), sigma)
    rgb_2, sigma_2 = forward(model, c["Xf"], c["D"])
    assert torch.equal(rgb_2, render_runs[1][0]) and torch.equal(sigma_2, render_runs[1][1])
    # (the first 128 k samples of the whole launch: the same waves again)
    assert torch.equal(rgb_2[:Mk], rgb) and torch.equal(sigma_2[:Mk], sigma)


def test_a_single_far_sample(model, render_case, arith):
    """M = 1: one far sample, which every lane of the one wave repeats."""
    c = render_case
    s = c["waves"]["block 0"] + 3
    assert bool(c["far"][s])
    rgb, sigma = forward(model, c["Xf"][s:s + 1], c["D"][s:s + 1])
    assert rgb.shape == (1, 3) and sigma.shape == (1, 1)
    assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(sigma).all())
    at = int(torch.nonzero(c["idx"] == s)[0, 0])
    ref = tuple(t[at:at + 1] for t in c["ref"])
    assert_forward_accuracy(forward_accuracy(rgb, sigma, ref, slice(None), f"A/{arith} M = 1"), "M = 1")


# ======================================================= rays with far samples (B, C: training; D: render)
def place_far(o, d, z):
    """_draw's `place`: of every eight rays, ray 1 wholly far (its origin + 40 along an axis), ray 2 crossing
    the threshold (o = 12 e, d = e, z regular in [2, 6] with the draw's jitter: with N = 64 its first wave
    stays within |x| <= 16 and its second lies beyond), the others ordinary (six in a row: with N = 11 some waves hold no far sample).
    The axis cycles through the coordinates and both signs."""
    R, N = z.shape
    o, d, z = o.clone(), d.clone(), z.clone()
    r = torch.arange(R)
    e = torch.zeros(R, 3)
    e[r, (r // 8) % 3] = 1.0 - 2.0 * ((r // 24) % 2)
    far, cross = r % 8 == 1, r % 8 == 2
    o[far] += 40.0 * e[far]
    o[cross], d[cross] = 12.0 * e[cross], e[cross]
    jitter = ((z[cross] - 2.0) / 4.0 * N) % 1.0
    z[cross] = 2.0 + 4.0 * (torch.arange(N) + jitter) / N
    return o, d, z


def ray_kinds(pts, R, N):
    """Per ray: 0 ordinary (no far sample), 1 wholly far, 2 crossing."""
    f = far_mask(pts).reshape(R, N)
    return torch.where(f.all(1), 1, torch.where(f.any(1), 2, 0))


# ================================================================== B. the training forward with saves
@pytest.fixture(scope="module", params=[(40, 64), (96, 11)], ids=lambda p: f"R{p[0]}-N{p[1]}")
def train_case(request, ref_state, app_vec, arith):
    """Forward with saves (and the data gradients) on far, crossing and ordinary rays.  N = 64: a wave lies
    on one ray; N = 11: waves straddle rays, so far and in-range samples share waves."""
    R, N = request.param
    draw = _draw(R, N, 3, place_far)
    r = _mlp_forward_backward(ref_state, app_vec, R=R, N=N, draw=draw)
    kinds = ray_kinds(r["pts"], R, N)
    assert all(int((kinds == k).sum()) >= R // 8 for k in (0, 1, 2)), kinds
    far = far_mask(r["pts"])
    far_wave = wave_any(far)
    assert bool((~far_wave).any()) and (N == 64 or bool((far_wave & ~far).any()))
    if N == 64:   # a crossing ray: the first wave within range, the second beyond
        f2 = far.reshape(R, N)[2]
        assert not bool(f2[:32].any()) and bool(f2[33:].all())
    return dict(R=R, N=N, draw=draw, r=r, far=far, far_wave=far_wave)


def test_saved_encoding_is_sin_cos_of_the_points(train_case, arith):
    """The saved enc_x against float64 sin / cos of the fp32 points, 2^i x exact: waves without a far sample
    under f16x3 within pe_sin.h's documented 1.6e-7 (the device runs the header's IEEE operations), waves on
    the library path and everything under f32 within the project's 2e-6.  The raw-input slots are the
    points bit for bit (which also shows that the reference's positions are the kernel's)."""
    r, far, far_wave = train_case["r"], train_case["far"], train_case["far_wave"]
    pts, save = r["pts"], r["save"]
    assert torch.equal(save[:, 1024:1027], pts)
    p64 = pts.double()
    ref = torch.cat([p64] + [f(p64 * 2 ** i) for i in range(10) for f in (torch.sin, torch.cos)], dim=-1)
    e_gpu = (save[:, 1024:1087].double() - ref).abs().max(dim=1).values
    e_cpu = (O.positional_encoding(pts, 10).double() - ref).abs().max(dim=1).values
    fast = ~far_wave if arith == "f16x3" else torch.zeros_like(far_wave)
    classes = (("fast path", fast, 1.6e-7), ("library path, in range", ~fast & ~far, 2e-6),
               ("library path, far", far, 2e-6))
    for name, sel, bound in classes:
        if bool(sel.any()):
            print(f"B/{arith} R={train_case['R']} N={train_case['N']} enc_x {name} ({int(sel.sum())} samples): "
                  f"max err vs f64 {float(e_gpu[sel].max()):.3g} (cpu f32 torch.sin/cos {float(e_cpu[sel].max()):.3g})")
    for name, sel, bound in classes:
        if bool(sel.any()):
            assert float(e_gpu[sel].max()) <= bound, (name, float(e_gpu[sel].max()), bound)
    # every class is there, except that f32 has no fast path and that at N = 64 (a wave on one ray, far
    # from its first sample to its last or not at all) f16x3 has no in-range sample on the library path
    absent = {"f32": "fast path", "f16x3": "library path, in range" if train_case["N"] == 64 else None}[arith]
    assert all(bool(sel.any()) for name, sel, _ in classes if name != absent)


def test_saves_of_far_rays_are_the_activations(train_case, arith):
    """test_forward_saves_are_the_activations' checks (activations, enc_x, enc_d, block exponent records;
    the mask words in _mlp_forward_backward) on these batches; a far block's enc_x record carries the
    exponent of its largest |x|, not of 1."""
    r, N = train_case["r"], train_case["N"]
    saves_are_the_activations(r, N)
    if arith == "f16x3":
        rec = r["save"][:, 1087].numpy()
        big = r["pts"].abs().max(dim=1).values.reshape(-1, 32).max(dim=1).values.numpy()
        blocks = np.nonzero(big > LIMIT)[0]
        assert len(blocks) >= 8
        e = np.frexp(big[blocks])[1]
        assert np.all(e >= 5)
        np.testing.assert_array_equal(rec[32 * blocks + 8], -(1000.0 + e))


@pytest.mark.parametrize("arith", ["f16x3"], indirect=True)
def test_gathered_forward_on_far_samples(train_case, ref_state, app_vec, arith):
    """mlp16_live_kernel on live lists with far samples equals the dense forward on the gathered inputs
    bit for bit (test_gathered_forward_equals_the_dense_forward_on_the_gathered_inputs' property; a wave
    is 32 consecutive compact rows on both sides): far samples in full groups and as the last entry of the
    ragged last group, and a far sample as the only live one.  The gathered kernel is f16x3 only (under
    f32 the entry point refuses the call, tests/golden/host_error_parity.json), so this test runs under
    f16x3 alone."""
    assert arith == "f16x3"
    from nerfmi import _lib as L
    lib, dev = L.load(), L.device()
    R, N, far = train_case["R"], train_case["N"], train_case["far"]
    M = R * N
    o, d, z = (t.to(dev).contiguous() for t in train_case["draw"][:3])
    packed, _, _ = packed_of(ref_state, dev)
    feat, encd = torch.empty(R, 256, device=dev), torch.empty(R, 32, device=dev)
    a = app_vec.reshape(1, 32).to(dev).contiguous()
    ok(lib.nerf_ray_features_train(P(packed), P(d), R, P(a), 1, P(feat), P(encd), S()), lib)
    c = dict(N=N, o=o, dn=d, z=z, feat=feat, encd=encd, packed=packed)
    fa = torch.nonzero(far)[:, 0]
    g = torch.Generator().manual_seed(7)
    k = 3 * 32 + 5
    head = (torch.randperm(int(fa[-1]) - 1, generator=g)[:k - 1] + 1).sort().values   # (sample 0 stays outside)
    lists = {"groups": torch.cat([head, fa[-1:]]), "only": fa[len(fa) // 2:len(fa) // 2 + 1]}
    in_full = wave_any(far[lists["groups"]])[:96].reshape(3, 32).any(1)
    mixed = (~far[lists["groups"]][:96]).reshape(3, 32).any(1)
    assert bool((in_full & mixed).any()) and bool(far[lists["groups"]][-1])
    for name, idx in lists.items():
        n = idx.numel()
        live = torch.zeros(M, dtype=torch.int32, device=dev)
        live[:n] = idx.to(torch.int32).to(dev)
        save = torch.full((L.tile_rows(n), L.SAVE_ROW), SENT, device=dev)
        masks = torch.full((n, L.MASK_ROW), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        rgb_l, sig_l = torch.full((n, 3), SENT, device=dev), torch.full((n,), SENT, device=dev)
        rgb, sig = torch.full((M, 3), SENT, device=dev), torch.full((M,), SENT, device=dev)
        ok(lib.nerf_mlp_forward_train_live(P(packed), P(o), P(d), P(z), R, N, P(feat), P(encd), P(live), n, P(rgb),
                                           P(sig), P(rgb_l), P(sig_l), P(save), P(masks), S()), lib)
        e_save, e_masks, e_rgb, e_sig = forward_n1(lib, L, c, idx)
        assert torch.equal(save, e_save), name
        assert torch.equal(masks, e_masks), name
        assert torch.equal(rgb_l, e_rgb) and torch.equal(sig_l, e_sig), name
        sel = torch.zeros(M, dtype=torch.bool)
        sel[idx] = True
        sel = sel.to(dev)
        assert torch.equal(rgb[sel], e_rgb) and torch.equal(sig[sel], e_sig), name
        assert bool((rgb[~sel] == SENT).all()) and bool((sig[~sel] == SENT).all()), name
        assert bool(torch.isfinite(e_rgb).all()) and bool((e_sig != SENT).all()), name


# ===================================================================== C. gradients on far samples
@pytest.mark.parametrize("N", [64, 40])
def test_gradients_on_far_rays(ref_state, app_vec, arith, N):
    """test_mlp_backward_matches_autograd's check (d pre_0..7 no worse than the fp32 CPU autograd, each on its
    own ReLU branches) and test_param_grads_ray_path's (each tensor within max(2e-4, 2 e_cpu) of float64,
    two calls bit-identical, the appearance-row gradient) on far, crossing and ordinary rays clear of the
    ReLU kinks where they lie (the rays are placed before _safe_draw filters them).  The encoding is not
    differentiated; layer 0's and the skip layer's weight gradients and the pair kernel's block scales see
    enc_x columns whose magnitudes differ by 2^6 within a chunk.  N = 40: waves straddle rays."""
    R = 48                          # test_param_grads_ray_path's
    draw = _safe_draw(ref_state, app_vec, R, N, seed=3, place=place_far)
    pts = (draw[0][:, None, :] + draw[1][:, None, :] * draw[2][..., None]).reshape(-1, 3)
    kinds = ray_kinds(pts, R, N)
    print(f"C/{arith} N={N}: {[int((kinds == k).sum()) for k in (0, 1, 2)]} ordinary / far / crossing rays")
    assert all(int((kinds == k).sum()) >= 4 for k in (0, 1, 2)), kinds
    r = _mlp_forward_backward(ref_state, app_vec, R=R, N=N, draw=draw)
    assert torch.equal(r["save"][:, 1024:1027], pts)
    data_grads_match_autograd(ref_state, app_vec, r, draw, f"C/{arith} N={N} data gradients")
    param_grads_ray_path(ref_state, app_vec, "broadcast", R, N, draw, r)


# ============================================================ D. coarse render on far and crossing rays
@pytest.fixture(scope="module")
def ray_case(nerfmi_mod, cus, ref_state, app_vec):
    """2 G + 3 rays of a frame, every eighth one moved: alternately wholly far (origin + 40 along an axis)
    and crossing (o = 12 e, d = e: with the unperturbed z of N = 64 its first wave stays in range and its
    second lies beyond).  The reference positions are the kernel's: the directions the render's own
    normalisation gives, O.sample_stratified's fp32 z (bit-equal to the render's) and o + d z in fp32.
    float64 MLP and compositing on those points for 64 of the rays (4,096 samples), half of them moved."""
    from nerfmi import _lib as L
    from nerfmi import cameras
    lib = L.load()
    B, N = 2 * cus + 3, 64
    o, d = nerfmi_mod.get_rays(800, 800, cameras.synthetic_focal(800), cameras.frame_c2w("chair").cuda())
    first = 392 * 800 + 100
    o, d = o.reshape(-1, 3)[first:first + B].cpu().clone(), d.reshape(-1, 3)[first:first + B].cpu().clone()
    moved = torch.arange(0, B, 8)
    for j, r in enumerate(moved.tolist()):
        e = torch.zeros(3)
        e[j % 3] = 1.0 - 2.0 * ((j // 6) % 2)
        if j % 2 == 0:
            o[r] += 40.0 * e
        else:
            o[r], d[r] = 12.0 * e, e
    dn = torch.empty(B, 3, device="cuda")
    ok(lib.nerf_normalize_dirs(P(d.cuda().contiguous()), B, P(dn), S()), lib)
    dn = dn.cpu()
    z, pts = O.sample_stratified(o, dn, 2.0, 6.0, N)
    kinds = ray_kinds(pts.reshape(-1, 3), B, N)
    assert torch.equal(torch.nonzero(kinds)[:, 0], moved)
    assert bool((kinds[moved[0::2]] == 1).all()) and bool((kinds[moved[1::2]] == 2).all())
    f = far_mask(pts[moved[1]])
    assert not bool(f[:32].any()) and bool(f[32:].all())
    sub = torch.cat([moved[:32], moved[:32] + 5]).sort().values
    assert sub.numel() == 64 and int(sub[-1]) < B
    st64 = {k: v.double() for k, v in ref_state.items()}
    with torch.no_grad():
        r32, d32, _ = O._pass(ref_state, pts[sub], dn[sub], z[sub], app_vec)
        r64, d64, _ = O._pass(st64, pts[sub].double(), dn[sub].double(), z[sub].double(), app_vec.double())
    return dict(B=B, N=N, o=o, d=d, z=z, sub=sub, r32=r32, d32=d32, r64=r64, d64=d64)


def coarse(nerfmi_mod, model, app_vec, c, lo, hi, **kw):
    with torch.no_grad():
        return nerfmi_mod.volume_render(model, c["o"][lo:hi].cuda(), c["d"][lo:hi].cuda(), 2.0, 6.0, c["N"], 0,
                                        appearance_embedding=app_vec.cuda(), perturb=False, hierarchical=False, **kw)


def test_coarse_render_of_far_and_crossing_rays(nerfmi_mod, model, app_vec, ray_case, cus, arith):
    """Against float64 on the kernel's own points by test_h1_render_vs_float64's yardstick (no worse than
    the fp32 CPU oracle on the same points, x1.5, in max, p99.9 and median), and bit for bit against two
    calls split at ray G + 1 (N % 32 == 0: a wave never holds two rays, so the split changes no wave)."""
    c = ray_case
    B, sub = c["B"], c["sub"]
    rgb, depth, ex = coarse(nerfmi_mod, model, app_vec, c, 0, B)
    assert torch.equal(ex["z_vals"].cpu(), c["z"])
    assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(depth).all())
    check_no_worse_than_cpu(rgb.cpu()[sub], c["r32"], c["r64"], f"D/{arith} rgb")
    check_no_worse_than_cpu(depth.cpu()[sub], c["d32"], c["d64"], f"D/{arith} depth")
    split = cus + 1
    (rgb_a, depth_a, _), (rgb_b, depth_b, _) = (coarse(nerfmi_mod, model, app_vec, c, 0, split),
                                                coarse(nerfmi_mod, model, app_vec, c, split, B))
    assert torch.equal(torch.cat([rgb_a, rgb_b]), rgb) and torch.equal(torch.cat([depth_a, depth_b]), depth)


def test_all_ones_grid_on_far_rays_is_the_plain_render(nerfmi_mod, model, app_vec, ray_case):
    """test_gpu_occupancy.py's property on these rays, the grid's box enclosing them (|x| <= 70): with every
    cell occupied the live list names every sample in order, so mlp16s_live_kernel's waves are the plain
    kernel's, far ones included."""
    c = ray_case
    ones = nerfmi_mod.OccupancyGrid((-70.0, -70.0, -70.0), (70.0, 70.0, 70.0), 4).from_mask(
        torch.from_numpy(np.ones((4, 4, 4), bool)))
    plain = coarse(nerfmi_mod, model, app_vec, c, 0, c["B"])
    full = coarse(nerfmi_mod, model, app_vec, c, 0, c["B"], occupancy=ones)
    assert torch.equal(full[0], plain[0]) and torch.equal(full[1], plain[1])
    assert set(full[2]) == set(plain[2])
    for k in plain[2]:
        assert torch.equal(full[2][k], plain[2][k]), k
    assert float(plain[0].abs().max()) > 0
