"""Soft-argmin heads as one operator and one autograd node (soft_argmin.hip).

GwcNet's disparity head (gwc_main.py:246-276: x4 trilinear up-sampling of the (B,1,48,h,w) cost, softmax over the 192
planes, disparity_regression) is soft_argmin(cost, 4, -1.0) (the reference negates the regression); IGEV's initial
disparity (igev_stereo.py:175-176: softmax over the 48 planes, disparity_regression) is soft_argmin(cost, 1).  The
up-sampled volume never exists.  Forward: dkt_soft_argmin_fwd.  Backward: dkt_soft_argmin_bwd, deterministic, the softmax
recomputed from the cost, the only tensor the node saves."""
import torch
from torch.autograd.function import once_differentiable

from . import _ffi

FACTORS = (1, 4)


def _batch_strided(t):
    """`t` (B, C, h, w) as the kernels read it (scalar accesses: no alignment beyond a float's): (tensor, batch stride);
    copied only when its layout needs it."""
    B, C, h, w = t.shape
    if t.stride(3) == 1 and t.stride(2) == w and t.stride(1) == h * w and (B == 1 or t.stride(0) >= C * h * w):
        return t, (t.stride(0) if B > 1 else C * h * w)
    return t.contiguous(), C * h * w


def _forward(cost, bstride, factor, out_scale):
    B, D, h, w = cost.shape
    out = torch.empty((B, 1, factor * h, factor * w), device=cost.device, dtype=torch.float32)
    _ffi.call("dkt_soft_argmin_fwd", cost, cost.data_ptr(), bstride, out_scale, out.data_ptr(), B, D, h, w, factor)
    return out


class _SoftArgminFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cost, factor, out_scale):
        cost, bstride = _batch_strided(cost)
        ctx.save_for_backward(cost)
        ctx.bstride, ctx.factor, ctx.out_scale = bstride, factor, out_scale
        return _forward(cost, bstride, factor, out_scale)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        (cost,) = ctx.saved_tensors
        B, D, h, w = cost.shape
        _ffi.require_gpu(gout)
        g, gbs = _batch_strided(gout)
        nbytes = _ffi.size("dkt_soft_argmin_bwd_workspace", B, D, h, w, ctx.factor)
        ws = torch.empty(nbytes // 4, device=cost.device, dtype=torch.float32) if nbytes else None
        gcost = torch.empty((B, D, h, w), device=cost.device, dtype=torch.float32)
        _ffi.call("dkt_soft_argmin_bwd", cost, g.data_ptr(), gbs, cost.data_ptr(), ctx.bstride, ctx.out_scale, gcost.data_ptr(),
                  _ffi.ptr(ws), B, D, h, w, ctx.factor)
        return gcost, None, None


def soft_argmin(cost, factor=1, out_scale=1.0):
    """cost (B, D, h, w) or (B, 1, D, h, w) -> out_scale * sum_d d softmax_d(up_f(cost)), (B, 1, f h, f w) fp32; up_f is
    torch's trilinear align_corners=False up-sampling of all three axes by `factor` (1: none, or 4), f D <= 256.
    Differentiable with respect to cost.  Tensors on a HIP device; non-fp32 inputs are cast with .float(); a batch-strided
    cost is read in place."""
    if cost.dim() == 5:
        if cost.shape[1] != 1:
            raise ValueError("soft_argmin: cost %s" % (tuple(cost.shape),))
        cost = cost[:, 0]
    if cost.dim() != 4:
        raise ValueError("soft_argmin: cost %s" % (tuple(cost.shape),))
    if factor not in FACTORS:
        raise _ffi.DktError("soft_argmin: factor %r outside %s" % (factor, FACTORS))
    cost = cost.float()
    _ffi.require_gpu(cost)
    if torch.is_grad_enabled() and cost.requires_grad:
        return _SoftArgminFn.apply(cost, int(factor), float(out_scale))
    return _forward(*_batch_strided(cost), int(factor), float(out_scale))
