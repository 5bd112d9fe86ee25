"""The distortion loss of the ray weights in float64, and the composite-plus-distortion truth — TEST
INFRASTRUCTURE ONLY (tests/test_distortion_host.py checks these on the CPU; tests/test_gpu_distortion.py
and tests/test_gpu_train_distortion.py hold the kernels to them).

The definition (include/nerfmi_train.h "distortion"), per ray of T samples, everything in
float64 from the float32 z:
    delta_i = z_{i+1} - z_i  (i < T-1),  delta_{T-1} = (double)1e-3f,  m_i = z_i + delta_i / 2
    l       = inv [ sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i ],  inv = 1 / (far - near)
    dl/dw_k = inv [ 2 sum_j w_j |m_k - m_j| + (2/3) w_k delta_k ]
`definition` is the O(T^2) double sum, written independently of the kernel's closed form;
`closed_form` restates that closed form (prefix sums on sorted m) for the CPU comparison of the two.
"""
import torch

import degenerate_cases as D

LAST_DELTA = float(torch.tensor(1e-3, dtype=torch.float32).double())   # (double)1e-3f


def intervals(z):
    """(delta, m) in float64 from z (B,T) as float32 values."""
    z64 = z.float().double()
    delta = torch.cat([z64[:, 1:] - z64[:, :-1], torch.full_like(z64[:, :1], LAST_DELTA)], dim=1)
    return delta, z64 + delta / 2


def definition(w, z, near, far, want_grad=True):
    """(l (B,), dl/dw (B,T) or None) by the O(T^2) definition in float64; w (B,T) of any float dtype (its
    values are taken as they are), z (B,T).  T = 1: zeros."""
    w64 = w.double()
    B, T = w64.shape
    if T == 1:
        return torch.zeros(B, dtype=torch.float64), (torch.zeros(B, 1, dtype=torch.float64) if want_grad else None)
    inv = 1.0 / (float(far) - float(near))
    delta, m = intervals(z)
    loss = torch.zeros(B, dtype=torch.float64)
    grad = torch.zeros(B, T, dtype=torch.float64) if want_grad else None
    rows = max(1, (1 << 22) // (T * T))                       # rays per slab of the (rows, T, T) table
    for a in range(0, B, rows):
        sl = slice(a, a + rows)
        gap = (m[sl, :, None] - m[sl, None, :]).abs()          # |m_i - m_j|
        pair = torch.einsum("bi,bij,bj->b", w64[sl], gap, w64[sl])
        loss[sl] = inv * (pair + (w64[sl] ** 2 * delta[sl]).sum(-1) / 3.0)
        if want_grad:
            grad[sl] = inv * (2.0 * torch.einsum("bkj,bj->bk", gap, w64[sl]) + (2.0 / 3.0) * w64[sl] * delta[sl])
    return loss, grad


def loss_autograd(w, z, near, far):
    """The definition's loss as a differentiable expression of w (B,T) (requires grad or part of a graph)
    in w's dtype: float64 is what torch differentiates on its own, float32 the fp32 baseline."""
    if w.shape[1] == 1:
        return (w * 0.0).sum(-1)
    inv = 1.0 / (float(far) - float(near))
    delta, m = (t.to(w.dtype) for t in intervals(z))
    gap = (m[:, :, None] - m[:, None, :]).abs()
    return inv * ((w[:, :, None] * w[:, None, :] * gap).sum((1, 2)) + (w * w * delta).sum(-1) / 3.0)


def closed_form(w, z, near, far):
    """(l, dl/dw) in float64 by the O(T) closed form on sorted m: sum_j w_j |m_k - m_j| =
    m_k (W_<k - W_>k) - (M_<k - M_>k) with W, M the prefix and suffix sums of w and w m."""
    w64 = w.double()
    B, T = w64.shape
    if T == 1:
        return torch.zeros(B, dtype=torch.float64), torch.zeros(B, 1, dtype=torch.float64)
    inv = 1.0 / (float(far) - float(near))
    delta, m = intervals(z)
    wm = w64 * m
    Wb, Mb = torch.cumsum(w64, 1) - w64, torch.cumsum(wm, 1) - wm          # sums before k
    Wa, Ma = w64.sum(1, keepdim=True) - Wb - w64, wm.sum(1, keepdim=True) - Mb - wm   # sums after k
    a = m * (Wb - Wa) - (Mb - Ma)
    return inv * ((w64 * a).sum(-1) + (w64 ** 2 * delta).sum(-1) / 3.0), inv * (2.0 * a + (2.0 / 3.0) * w64 * delta)


def bound(ref, T, S):
    """The issue's bound on an output against its float64 reference: 2^-23 |ref| + T 2^-48 S, S per ray
    ((B,) or broadcastable to ref): one float rounding (2^-24) with a margin of 2, plus the double
    sums' cancellation."""
    S = S if S.dim() == ref.dim() else S[:, None]
    return 2.0 ** -23 * ref.abs() + T * 2.0 ** -48 * S


def ray_scale(w, z, near, far, scale=1.0):
    """S = scale inv max z sum w per ray (B,), float64."""
    return float(scale) / (float(far) - float(near)) * z.double().abs().max(-1).values * w.double().sum(-1)


def weights32(sigma, z, exp32=D.exp_rn):
    """(B,T) float32 weights as the kernels round them (composite_body.h): alpha32 * (float)T, T the double
    product of the fp32 factors 1 - alpha + 1e-10."""
    z32 = z.float()
    dist = torch.cat([z32[:, 1:] - z32[:, :-1], torch.full_like(z32[:, :1], 1e-3)], dim=1)
    a32 = 1.0 - exp32(-sigma.float().reshape(z.shape) * dist)
    f32 = 1.0 - a32 + 1e-10
    assert a32.dtype == f32.dtype == torch.float32
    Tr = torch.cumprod(torch.cat([torch.ones_like(f32[:, :1]).double(), f32.double()], dim=1), dim=1)[:, :-1]
    return a32 * Tr.float()


def profile_weights(B, T, seed=0):
    """(w (B,T) float32, z (B,T) float32, sorted mask (B,)) of degenerate_cases.ray_profiles(B, T): walls,
    shells, empty rays, fog, tied z (profiles 7, 8) and the descending pair of profile 9 (mask False)."""
    g = torch.Generator().manual_seed(7919 * T + B + seed)
    z, sigma, _ = D.ray_profiles(B, T, g)
    return weights32(sigma, z).contiguous(), z.contiguous(), D.sorted_rays(B)


def composite_distortion_f64(rgb, sigma, z, near, far, exp32=D.exp_rn):
    """The float64 truth of a part's composite and its distortion loss: degenerate_cases.composite_f64_st
    (fp32 values of alpha and of the transmittance factors, float64 gradients, straight through) and the
    definition's loss on its weights, so the straight-through weights feed the loss.  rgb (B,T,3) and
    sigma (B,T,1) float64 (differentiable).  Returns (rgb_map (B,3), acc (B,), l (B,), weights (B,T))."""
    rgb_map, _, w = D.composite_f64_st(rgb, sigma, z, exp32)
    w = w[..., 0]
    return rgb_map, w.sum(-1), loss_autograd(w, z, near, far), w

