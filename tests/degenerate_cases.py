"""Seeded inputs of the trained-scene regime, and the gradient truth of the composite there — TEST
INFRASTRUCTURE ONLY (tests/test_degenerate_cases_cpu.py shows on the CPU that each generator reaches
the regime it names; tests/test_gpu_degenerate_rays.py and tests/test_gpu_degenerate_train.py feed them
to the kernels).

The regime: surfaces with sigma * dist of 20 and above (alpha == 1 in fp32, every later factor of the
transmittance exactly 1e-10f, the product through float denormals to 0 within five samples), empty
space with sigma == 0 exactly (depth = 0 / (0 + 1e-10), a depth gradient of order 1e10), and coarse
weights that form a near-delta pdf, so the inverse CDF puts many fine samples into one bin, bit-equal
to a coarse z or to each other.  Everything is finite: NaN and Inf inputs are out of scope.

Everything here is CPU-only and drawn from the torch.Generator passed in (or a fixed seed).
"""
import torch

N_PROFILES = 10
U_MAX = 1.0 - 2.0 ** -24          # the largest uniform the in-kernel generator emits (common.h, hash_uniform)
_S0 = (0, 3, 4, 63, 64, -1, -2, 1)   # -1: N - 1, -2: N // 2


def profile_of(b):
    """Ray b's profile: b % 8 over the first 64 rays (8 profiles x 8 start indices); the rays from 64
    on would repeat rays 0.. and carry the two z profiles instead (8: constant z, 9: one descending
    pair), alternating."""
    return b % 8 if b < 64 else 8 + b % 2


def start_of(b, N):
    """Ray b's start index: the lane (3 | 4), round (63 | 64) and last-sample boundaries of the
    composite's 16 lanes x 4 samples layout."""
    s = _S0[(b // 8) % 8]
    return (N - 1 if s == -1 else N // 2 if s == -2 else s) % N


def ray_profiles(B, N, gen):
    """z (B,N), sigma (B,N), rgb (B,N,3), fp32.  z is sorted U(2,6) except in profiles 7-9.

      0        empty: sigma 0 everywhere
      1, 2, 6  wall: sigma 0 before s0 and K from s0 on, K = 1e4, 300, 3e38
      3        shell: sigma 50 on [s0, s0 + 3)
      4        alternating: sigma 1e3 on s0::2, 0 elsewhere
      5        fog: sigma 1e-3 everywhere
      7        sigma = 20 rand, z[s0:s0+4] all equal (dist == 0)
      8        z constant over the ray (near == far), sigma = 1e4 rand
      9        sigma = 20 rand, z[p] and z[p+1] swapped at p = s0 % (N-1) (one descending pair, dist < 0)
               with sigma <= 5 at p and p + 1, so exp(sigma |dist|) stays small
    """
    assert N >= 2
    z = torch.sort(torch.rand(B, N, generator=gen) * 4 + 2, dim=-1).values
    rgb = torch.rand(B, N, 3, generator=gen)
    noise = torch.rand(B, N, generator=gen)
    sigma = torch.zeros(B, N)
    for b in range(B):
        p, s0 = profile_of(b), start_of(b, N)
        if p in (1, 2, 6):
            sigma[b, s0:] = {1: 1e4, 2: 300.0, 6: 3e38}[p]
        elif p == 3:
            sigma[b, s0:s0 + 3] = 50.0
        elif p == 4:
            sigma[b, s0::2] = 1e3
        elif p == 5:
            sigma[b] = 1e-3
        elif p == 7:
            sigma[b] = 20 * noise[b]
            z[b, s0:s0 + 4] = z[b, s0]
        elif p == 8:
            sigma[b] = 1e4 * noise[b]
            z[b] = z[b, N // 2]
        elif p == 9:
            q = s0 % (N - 1)
            sigma[b] = 20 * noise[b]
            sigma[b, q:q + 2] = 5 * noise[b, q:q + 2]
            z[b, q], z[b, q + 1] = z[b, q + 1].clone(), z[b, q].clone()
    return z, sigma, rgb


def sorted_rays(B):
    """Mask of the rays of ray_profiles whose z ascends (all but profile 9)."""
    return torch.tensor([profile_of(b) != 9 for b in range(B)])


def exp_rn(x):
    """fp32 exp, correctly rounded: the kernels' expf_rn (csrc/common.h: exp in double, rounded once).
    torch's vectorised CPU exp is a 1-ulp function and differs from it on a few values per thousand,
    which ones depending on the CPU; where alpha = 1 - exp(-x) is small (fog, the 1e-3 last interval)
    that ulp is up to 1e-3 of alpha."""
    return torch.exp(x.double()).float()


def composite_f64_st(rgb, sigma, z, exp32=torch.exp):
    """The reference's composite (oracle.nerf_oracle.composite, render.py:56-80) in float64 on (B,N,3)
    rgb, (B,N,1) sigma (float64, differentiable) and fp32 z, with alpha and the transmittance factor
    1 - alpha + 1e-10 taking the values the fp32 path rounds them to, straight through:
    value of fp32, gradient of float64.  This is the high-precision truth of the operation the
    kernels implement; plain float64 is another function here (alpha = 1 - 2e-9 where fp32 has 1).
    exp32 is the fp32 path's exp: torch.exp for torch's CPU path (the default), exp_rn for the
    kernels, so each path is measured against the truth at its own rounding of exp and neither is
    charged the other's ulp."""
    z32 = z.float()
    dist32 = torch.cat([z32[..., 1:] - z32[..., :-1], torch.ones_like(z32[..., :1]) * 1e-3], dim=-1).unsqueeze(-1)
    a32 = 1.0 - exp32(-sigma.detach().float() * dist32)
    f32 = 1.0 - a32 + 1e-10
    assert a32.dtype == f32.dtype == torch.float32
    a64 = 1.0 - torch.exp(-sigma * dist32.double())
    f64 = 1.0 - a64 + 1e-10
    alpha = a64 + (a32.double() - a64).detach()
    fac = f64 + (f32.double() - f64).detach()
    trans = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1, :]), fac], dim=1), dim=1)[:, :-1, :]
    weights = alpha * trans
    rgb_map = torch.sum(weights * rgb, dim=1)
    depth_map = torch.sum(weights * z32.double().unsqueeze(-1), dim=1) / (torch.sum(weights, dim=1) + 1e-10)
    return rgb_map, depth_map, weights


def _dist32(z):
    z32 = z.float()
    return torch.cat([z32[..., 1:] - z32[..., :-1], torch.ones_like(z32[..., :1]) * 1e-3], dim=-1)


def acc32_of(sigma, z, exp32=torch.exp):
    """(B,) opacity as the kernels round it (composite_body.h, composite_bwd_body.h): the fp32 weights
    alpha32 * (float) T, T the double product of the fp32 factors, summed in double and rounded once.
    sigma is (B,N) or (B,N,1)."""
    s32 = sigma.detach().float().reshape(z.shape)
    a32 = 1.0 - exp32(-s32 * _dist32(z))
    f32 = 1.0 - a32 + 1e-10
    assert a32.dtype == f32.dtype == torch.float32
    T = torch.cumprod(torch.cat([torch.ones_like(f32[:, :1]).double(), f32.double()], dim=1), dim=1)[:, :-1]
    return (a32 * T.float()).double().sum(-1).float()


def composite_f64_st_bg(rgb, sigma, z, bg=None, bd=None, exp32=torch.exp, gate=None):
    """composite_f64_st with the opacity and the background blend: the same
    straight-through composite (fp32 values of alpha and of 1 - alpha + 1e-10, float64 gradients), and
      acc    = sum w                          (B,1)
      colour = rgb_map + k bg                 (B,3)  bg (B,3) or (1,3), None: black
      depth  = sum w z + k bd                 (B,1)  where bd is given, else the normalised depth
    with k = gate (1 - acc) and gate = [acc32 < 1] a CONSTANT from acc32_of: the kernels' rule is k > 0,
    strict (a saturated ray passes no gradient through k), where torch.clamp's backward passes the
    gradient at exactly 1 - acc == 0.  `gate` (B,) bool overrides the rule (to measure what it changes).
    Returns (rgb_map, depth, weights, acc, colour)."""
    rgb_map, depth_map, weights = composite_f64_st(rgb, sigma, z, exp32)
    acc = torch.sum(weights, dim=1)
    if gate is None:
        gate = acc32_of(sigma, z, exp32) < 1
    k = gate.to(acc.dtype)[:, None] * (1.0 - acc)
    colour = rgb_map if bg is None else rgb_map + k * bg.to(acc.dtype)
    if bd is not None:
        depth_map = torch.sum(weights * z.float().double().unsqueeze(-1), dim=1) + k * bd
    return rgb_map, depth_map, weights, acc, colour


def composite_f32_bg(rgb, sigma, z, bg=None, bd=None, gate=None):
    """The fp32 baseline of composite_f64_st_bg: the oracle's composite (render.py:56-80) with the same
    definitions in fp32 torch, under autograd.  The gate is acc32_of's as well (at torch's exp): torch's
    own float-order sum of the weights lands on the other side of 1 on a few saturated rays."""
    z32 = z.float()
    alpha = 1.0 - torch.exp(-sigma * _dist32(z).unsqueeze(-1))
    trans = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1, :]), 1.0 - alpha + 1e-10], dim=1), dim=1)[:, :-1, :]
    weights = alpha * trans
    rgb_map = torch.sum(weights * rgb, dim=1)
    acc = torch.sum(weights, dim=1)
    if gate is None:
        gate = acc32_of(sigma, z) < 1
    k = gate.to(acc.dtype)[:, None] * (1.0 - acc)
    colour = rgb_map if bg is None else rgb_map + k * bg
    swz = torch.sum(weights * z32.unsqueeze(-1), dim=1)
    depth_map = swz / (acc + 1e-10) if bd is None else swz + k * bd
    assert colour.dtype == depth_map.dtype == torch.float32
    return rgb_map, depth_map, weights, acc, colour


def peaked_weights(B, N, gen):
    """(B,N) coarse weights of surface rays: one weight in [0.1, 1) at a random index, 0 elsewhere;
    odd rays a further 0.3 on the next bin.  Ray 0 peaks at index 0, ray 1 at N-1, ray 2 is all zeros
    (a uniform pdf) and ray 3 holds 1e-12 throughout."""
    idx = torch.randint(0, N, (B,), generator=gen)
    val = 0.1 + 0.9 * torch.rand(B, generator=gen)
    idx[0] = 0
    if B > 1:
        idx[1] = N - 1
    w = torch.zeros(B, N)
    for b in range(B):
        w[b, idx[b]] = val[b]
        if b % 2 == 1 and idx[b] + 1 < N:
            w[b, idx[b] + 1] = 0.3
    if B > 2:
        w[2] = 0.0
    if B > 3:
        w[3] = 1e-12
    return w


def fine_samples(z, w, Nf, u):
    """The oracle's z_fine (sample_importance_h1's expressions up to ray_utils.py:139, before the merge),
    with its cdf, u and searchsorted indices."""
    n = z.shape[-1]
    wp = w + 1e-5
    wp = wp / wp.sum(dim=-1, keepdim=True)
    cdf = torch.cumsum(wp, dim=-1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], dim=-1)
    uu = torch.linspace(0., 1., Nf + 1)[:-1].expand(z.shape[0], Nf) + u / Nf
    inds = torch.searchsorted(cdf, uu.contiguous())
    below, above = torch.clamp_min(inds - 1, 0), torch.clamp_max(inds, n)
    c0, c1 = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    z0, z1 = torch.gather(z, 1, below.clamp_max(n - 1)), torch.gather(z, 1, above.clamp_max(n - 1))
    denom = c1 - c0
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    return z0 + (uu - c0) / denom * (z1 - z0), cdf, uu, inds


def exact_hit_case(N, Nf, B=8):
    """z, w, u_rand with the u_j bit-equal to cdf entries: every u_j where Nf divides N; where N divides
    Nf, u_j at j = k Nf/N hits cdf[k] (every entry below the last) and the others lie inside a bin.
    N and Nf are powers of two, the weights uniform at 1024 (1024 + 1e-5 rounds to 1024 in fp32, so
    the normaliser, the pdf 1/N and the cdf k/N are exact in any summation order), u_rand == 0
    (u_j = j/Nf exact), and z = 2 + b/4 + 4 k/N, dyadic, so the interpolation is exact too: a fine
    sample on a cdf entry equals a coarse z bit for bit ((4, 4): the merged row is 2 2 3 3 4 4 5 5)."""
    assert N & (N - 1) == 0 and Nf & (Nf - 1) == 0 and N >= 1 and Nf >= 1
    z = 2.0 + 0.25 * torch.arange(B, dtype=torch.float32)[:, None] + torch.arange(N, dtype=torch.float32) * (4.0 / N)
    return z.contiguous(), torch.full((B, N), 1024.0), torch.zeros(B, Nf)


def edge_uniforms(B, Nf, gen=None):
    """(B,Nf) uniforms with exact 0 and exact U_MAX mixed into random draws: a quarter of the entries
    each, the first column 0 on even rays and the last column U_MAX on odd ones (the first and the
    last u of the row: the last lands on, or rounds to, the last cdf entry)."""
    gen = gen or torch.Generator().manual_seed(7)
    u = torch.rand(B, Nf, generator=gen)
    pick = torch.rand(B, Nf, generator=gen)
    u[pick < 0.25] = 0.0
    u[pick > 0.75] = U_MAX
    u[0::2, 0] = 0.0
    u[1::2, -1] = U_MAX
    return u


def unsorted_z(z):
    """z with rays b % 3 == 1 holding one swapped adjacent pair (at b % (N-1)) and rays b % 3 == 2
    reversed; rays b % 3 == 0 stay ascending, so sorted and unsorted rays share a launch (a block
    takes 4 rays).  Returns (z, mask of the changed rays); at N == 1 nothing can change."""
    z = z.clone()
    B, N = z.shape
    changed = torch.zeros(B, dtype=torch.bool)
    if N < 2:
        return z, changed
    for b in range(B):
        if b % 3 == 1:
            q = b % (N - 1)
            z[b, q], z[b, q + 1] = z[b, q + 1].clone(), z[b, q].clone()
        elif b % 3 == 2:
            z[b] = z[b].flip(0)
        changed[b] = b % 3 != 0
    return z, changed


SHARP_K, SHARP_SHIFT = 1e5, -0.019


def sharp_state(ref_state, K=SHARP_K, shift=SHARP_SHIFT):
    """The seed-0 model with a trained scene's density range: density_head.weight *= K and
    density_head.bias = (bias + shift) K, i.e. sigma = relu(K (raw + shift)): exactly 0 where the raw
    density is below -shift, and of order K * 1e-3 (opaque within a sample) above it."""
    st = {k: v.clone() for k, v in ref_state.items()}
    st["density_head.weight"] = st["density_head.weight"] * K
    st["density_head.bias"] = (st["density_head.bias"] + shift) * K
    return st


def sharp_rays(golden):
    """The 256 rays of the sharp-scene tests: every 16th of the first 4,096 of fixture F1's chair crop."""
    f1 = golden("f1_get_rays.npz")
    return torch.from_numpy(f1["chair_o"])[:4096:16].contiguous(), torch.from_numpy(f1["chair_d"])[:4096:16].contiguous()
