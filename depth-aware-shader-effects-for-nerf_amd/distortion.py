"""The distortion loss of the ray weights as a stage (include/nerfmi_train.h "distortion").

mip-NeRF 360's regulariser: a penalty on the weights alone that is minimal when a ray's weight sits in
one short interval.  Floaters in front of a surface and haze behind it raise it, and they are what pulls
a ray's expected depth off the surface.  ``distortion_loss`` measures it on what a render returned;
training on it is ``Trainer(distortion_weight=)``.
"""
import math

import torch

from . import _lib


def _check_distortion_inputs(weights, z_vals, near, far):
    """(B, T) of the two tensors, checked (no device needed): weights (B,T) or (B,T,1) as
    ``extras['weights']``, z_vals (B,T), T in 1..4096, finite near < far; ValueError otherwise."""
    if weights.dim() == 3 and weights.shape[-1] == 1:
        weights = weights[..., 0]
    if weights.dim() != 2 or z_vals.dim() != 2 or weights.shape != z_vals.shape:
        raise ValueError(f"distortion_loss: weights {tuple(weights.shape)} and z_vals {tuple(z_vals.shape)} "
                         f"must be (B,T) (weights also (B,T,1))")
    B, T = weights.shape
    if not 1 <= T <= 4096:
        raise ValueError(f"distortion_loss: T={T} samples per ray (1..4096)")
    near, far = float(near), float(far)
    if not (math.isfinite(near) and math.isfinite(far) and far > near):
        raise ValueError(f"distortion_loss: near={near!r} far={far!r} (finite, far > near)")
    return weights, B, T, near, far


def distortion_loss(weights, z_vals, near, far, return_grad=False):
    """Per-ray distortion loss l (B,) of ray weights (B,T) (or ``extras['weights']``, (B,T,1)) at the
    non-decreasing sample depths z_vals (B,T), on the device; with ``return_grad`` also dl/dw (B,T).
    Sample i owns the compositor's interval (delta_i = z_{i+1} - z_i, the last 1e-3; midpoint m_i):
    l = [sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i] / (far - near).  Nothing here is
    differentiable by autograd: the gradient is the returned tensor."""
    weights, B, T, near, far = _check_distortion_inputs(weights, z_vals, near, far)
    dev = _lib.device()
    w = weights.detach().to(dev, torch.float32).contiguous()
    z = z_vals.detach().to(dev, torch.float32).contiguous()
    loss = torch.empty(B, device=dev)
    grad = torch.empty(B, T, device=dev) if return_grad else None
    P = _lib.ptr
    _lib.check(_lib.load().nerf_distortion(P(w), P(z), B, T, near, far, 1.0, P(loss), P(grad), _lib.stream()),
               "nerf_distortion")
    return (loss, grad) if return_grad else loss
