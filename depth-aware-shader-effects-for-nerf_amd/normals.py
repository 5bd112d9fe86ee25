"""Density-gradient normals (not a reference feature; include/nerfmi_train.h "position gradient and
normals").

The density's gradient with respect to the sample position is the training kernels' data-gradient
chain with dsigma = 1, drgb = 0, carried through W0^T, the skip layer's encoding columns and the
positional encoding's Jacobian by one more kernel (csrc/normals.hip).  A sample's normal is
n = -g / sqrt(g.g + 1e-30); a ray's normal is sum w_i n_i over the samples and weights a render returned:
world space, pointing out of the surface, not renormalised (its length is at most the ray's opacity).

  density_gradient(model, points)       (sigma (...), grad (...,3)) at points of any leading shape
  composite_normals(grad, weights)      (B,T,3), (B,T) -> (B,3)
  render_normals(model, o, dn, z, w)    the render-side pass on what volume_render returned
                                        (volume_render(..., return_normals=True) calls it)

Inference only: nothing here carries a gradient.
"""
import ctypes

import torch

from . import _lib
from .models import STATE_KEYS, state_tensors


def packed_input_for(model):
    """The packed input-gradient weights (nerf_pack_weights_input) of a model, cached on the module like
    autograd.packed_pair's packedT: re-packed when a parameter changes."""
    dev = _lib.device()
    sd = model.state_dict()
    key = (dev,) + tuple((sd[k].data_ptr(), sd[k]._version) for k in STATE_KEYS if k in sd)
    hit = model.__dict__.get("_nerfmi_packedIn")
    if hit is None or hit[0] != key:
        lib = _lib.load()
        ts = [t.detach().to(dev, torch.float32).contiguous() for t in state_tensors(sd, dev)]
        arr = (ctypes.c_void_p * 24)(*[t.data_ptr() for t in ts])
        packed_in = torch.empty(lib.nerf_packed_input_floats(), device=dev)
        _lib.check(lib.nerf_pack_weights_input(arr, _lib.ptr(packed_in), _lib.stream()), "nerf_pack_weights_input")
        hit = model.__dict__["_nerfmi_packedIn"] = (key, packed_in)
    return hit[1]


@torch.no_grad()
def density_gradient(model, points):
    """(sigma (...), grad (...,3)): the density at `points` (...,3) and its gradient with respect to them,
    exactly 0 where sigma is 0.  One "ray" per point at z = 0, as the differentiable NeRF.forward runs it."""
    from .autograd import packed_pair
    lib, s, P = _lib.load(), _lib.stream(), _lib.ptr
    dev = _lib.device()
    lead = points.shape[:-1]
    x = points.detach().reshape(-1, 3).to(dev, torch.float32).contiguous()
    M = x.shape[0]
    sigma, dx = torch.empty(M, device=dev), torch.empty(M, 3, device=dev)
    if M:
        packed, packedT = packed_pair(model)
        packed_in = packed_input_for(model)
        d = torch.zeros(M, 3, device=dev)
        d[:, 2] = 1.0                               # sigma does not depend on the direction
        z = torch.zeros(M, 1, device=dev)           # pts = x + d*0 = x
        feat, encd = torch.empty(M, 256, device=dev), torch.empty(M, 32, device=dev)
        rgb = torch.empty(M, 3, device=dev)
        save = torch.empty(_lib.tile_rows(M), _lib.SAVE_ROW, device=dev)
        masks = torch.empty(M, _lib.MASK_ROW, dtype=torch.int32, device=dev)
        grad = torch.empty(_lib.tile_rows(M), _lib.GRAD_ROW, device=dev)
        dsigma, drgb = torch.ones(M, device=dev), torch.zeros(M, 3, device=dev)
        _lib.check(lib.nerf_ray_features_train(P(packed), P(d), M, None, 0, P(feat), P(encd), s),
                   "nerf_ray_features_train")
        _lib.check(lib.nerf_mlp_forward_train(P(packed), P(x), P(d), P(z), M, 1, P(feat), P(encd), P(rgb), P(sigma),
                                              P(save), P(masks), s), "nerf_mlp_forward_train")
        _lib.check(lib.nerf_mlp_backward(P(packed), P(packedT), P(save), P(masks), P(sigma), P(rgb), P(dsigma),
                                         P(drgb), M, P(grad), s), "nerf_mlp_backward")
        _lib.check(lib.nerf_mlp_position_grad(P(packed_in), P(save), P(grad), M, P(dx), s), "nerf_mlp_position_grad")
    out = points.device
    return sigma.reshape(lead).to(out), dx.reshape(*lead, 3).to(out)


@torch.no_grad()
def composite_normals(grad, weights):
    """normal_map (B,3) = sum_i w_i n_i from density gradients (B,T,3) and ray weights (B,T) or (B,T,1)."""
    lib = _lib.load()
    dev = _lib.device()
    g = grad.detach().to(dev, torch.float32).contiguous()
    B, T = g.shape[0], g.shape[1]
    w = weights.detach().reshape(B, T).to(dev, torch.float32).contiguous()
    out = torch.empty(B, 3, device=dev)
    _lib.check(lib.nerf_composite_normals(_lib.ptr(g), _lib.ptr(w), B, T, _lib.ptr(out), _lib.stream()),
               "nerf_composite_normals")
    return out.to(grad.device)


@torch.no_grad()
def render_normals(model, o, dn, z_vals, weights):
    """nerf_render_normals on device tensors: origins o (B,3), normalised directions dn (B,3), and the
    z_vals (B,T) and weights (B,T) a render of those rays returned.  (B,3)."""
    from .autograd import packed_pair
    lib, P = _lib.load(), _lib.ptr
    B, T = z_vals.shape
    out = torch.empty(B, 3, device=o.device)
    packed, packedT = packed_pair(model)
    packed_in = packed_input_for(model)
    ws = torch.empty(lib.nerf_render_normals_workspace_bytes(B, T), dtype=torch.uint8, device=o.device)
    _lib.check(lib.nerf_render_normals(P(packed), P(packedT), P(packed_in), P(o), P(dn), P(z_vals), P(weights), B, T,
                                       P(out), P(ws), ws.numel(), _lib.stream()), "nerf_render_normals")
    return out
