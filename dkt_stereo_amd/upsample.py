"""Convex up-sampling as an autograd node (RAFTStereo.upsample_flow on the training path, raft_stereo.py:70-82).

Forward: dkt_convex_upsample_fwd, the leading `channels` channels, bit-identical to the inference kernel's.  Backward:
dkt_convex_upsample_bwd, deterministic, the softmax recomputed from the mask (only flow and mask are saved).

IGEV's context up-sampling (context_upsample_train.hip), the same operator on nine planes at full resolution, as two
nodes: the weights form behind submodule.context_upsample (forward the inference kernel, backward
dkt_context_upsample_bwd) and, from logits (IGEVStereo.upsample_disp, igev_stereo.py:145-147), context_upsample_logits on
dkt_context_upsample_logits_fwd / _bwd.  The three backwards are one call each through _backward; their kernels share
the nine-tap core of csrc/ups9.h."""
import torch

from . import _ffi


def _batch_strided(g):
    """`g` (N, C, H, W) as the kernel reads it: (tensor, batch stride); copied only when its layout needs it."""
    N, C, H, W = g.shape
    if (g.stride(3) == 1 and g.stride(2) == W and g.stride(1) == H * W and g.stride(0) >= C * H * W
            and g.stride(0) % 8 == 0 and g.data_ptr() % 16 == 0):
        return g, g.stride(0)
    g = g.contiguous()
    return g, C * H * W


def _backward(name, gout, coarse, nine, needs, channels, dims, scale=()):
    """The backward of the three nodes: entry `name`(gout, its batch stride, coarse, nine, *scale, gcoarse, gnine, ws, *dims,
    device, stream) -> (gcoarse, gnine), each None unless `needs` asks for it.  `gout` (N, C, fH, fW) is read in place where
    its layout allows; the workspace (N, channels, 9, H, W) exists only beside the gradient of `coarse` (N, D, H, W)."""
    need_coarse, need_nine = needs[:2]
    if not (need_coarse or need_nine):
        return None, None
    _ffi.require_gpu(gout)
    N, _, H, W = coarse.shape
    g, bstride = _batch_strided(gout)
    gcoarse = torch.empty_like(coarse) if need_coarse else None
    gnine = torch.empty_like(nine) if need_nine else None
    ws = torch.empty((N, channels, 9, H, W), device=coarse.device, dtype=torch.float32) if need_coarse else None
    _ffi.call(name, g, g.data_ptr(), bstride, coarse.data_ptr(), nine.data_ptr(), *scale, _ffi.ptr(gcoarse),
              _ffi.ptr(gnine), _ffi.ptr(ws), *dims)
    return gcoarse, gnine


class _ConvexUpsampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flow, mask, factor, channels):
        _ffi.require_gpu(flow, mask)
        N, D, H, W = flow.shape
        if mask.shape != (N, 9 * factor * factor, H, W):
            raise _ffi.DktError("upsample mask %s does not match flow %s at factor %d" % (tuple(mask.shape), tuple(flow.shape), factor))
        flow, mask = flow.contiguous(), mask.contiguous()
        out = torch.empty((N, channels, factor * H, factor * W), device=flow.device, dtype=torch.float32)
        _ffi.call("dkt_convex_upsample_fwd", flow, flow.data_ptr(), mask.data_ptr(), out.data_ptr(), N, D, channels, H, W, factor)
        ctx.save_for_backward(flow, mask)
        ctx.factor, ctx.channels = factor, channels
        return out

    @staticmethod
    def backward(ctx, gout):
        flow, mask = ctx.saved_tensors
        N, D, H, W = flow.shape
        return _backward("dkt_convex_upsample_bwd", gout, flow, mask, ctx.needs_input_grad, ctx.channels,
                         (N, D, ctx.channels, H, W, ctx.factor)) + (None, None)


def convex_upsample(flow, mask, factor, channels=None):
    """flow (N, D, H, W), mask (N, 9 f^2, H, W) -> the leading `channels` (default D) channels of the convex
    up-sampling, (N, channels, f H, f W), differentiable with respect to both.  fp32 tensors on a HIP device."""
    D = flow.shape[1]
    channels = D if channels is None else channels
    if not 1 <= channels <= D:
        raise _ffi.DktError("channels = %d outside 1..%d" % (channels, D))
    return _ConvexUpsampleFn.apply(flow, mask, factor, channels)


def _aligned16(t):
    """`t` (contiguous) at a 16-byte aligned address: the nine-plane tensors are moved 16 bytes at a time."""
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _context_upsample(disp_low, up_weights):
    """dkt_context_upsample on fp32 contiguous tensors."""
    b, _, h, w = disp_low.shape
    out = torch.empty((b, 4 * h, 4 * w), device=disp_low.device, dtype=torch.float32)
    _ffi.call("dkt_context_upsample", out, disp_low.data_ptr(), up_weights.data_ptr(), out.data_ptr(), b, h, w)
    return out


class _ContextUpsampleFn(torch.autograd.Function):
    """context_upsample under autograd: the forward is the inference kernel, the backward dkt_context_upsample_bwd
    (context_upsample_train.hip), deterministic."""

    @staticmethod
    def forward(ctx, disp_low, up_weights):
        ctx.save_for_backward(disp_low, up_weights)
        return _context_upsample(disp_low, up_weights)

    @staticmethod
    def backward(ctx, gout):
        disp_low, up_weights = ctx.saved_tensors
        b, _, h, w = disp_low.shape
        return _backward("dkt_context_upsample_bwd", gout.unsqueeze(1), disp_low, _aligned16(up_weights), ctx.needs_input_grad,
                         1, (b, h, w))


def context_upsample_weights(disp_low, up_weights, differentiable):
    """The weights form on fp32 contiguous tensors (submodule.context_upsample prepares them and decides): (B, 1, h, w),
    (B, 9, 4h, 4w) -> (B, 4h, 4w), the plain kernel call or, when `differentiable`, the same call inside _ContextUpsampleFn."""
    return _ContextUpsampleFn.apply(disp_low, up_weights) if differentiable else _context_upsample(disp_low, up_weights)


class _ContextUpsampleLogitsFn(torch.autograd.Function):
    """The tail of IGEVStereo.upsample_disp (igev_stereo.py:145-147: softmax over the nine planes, disp * scale,
    context_upsample) as one node: dkt_context_upsample_logits_fwd / _bwd, only disp and the logits saved."""

    @staticmethod
    def forward(ctx, disp_low, logits, scale):
        B, _, h, w = disp_low.shape
        out = torch.empty((B, 4 * h, 4 * w), device=disp_low.device, dtype=torch.float32)
        _ffi.call("dkt_context_upsample_logits_fwd", out, disp_low.data_ptr(), logits.data_ptr(), scale, out.data_ptr(), B, h, w)
        ctx.save_for_backward(disp_low, logits)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, gout):
        disp_low, logits = ctx.saved_tensors
        B, _, h, w = disp_low.shape
        return _backward("dkt_context_upsample_logits_bwd", gout.unsqueeze(1), disp_low, logits, ctx.needs_input_grad, 1,
                         (B, h, w), scale=(ctx.scale,)) + (None,)


def context_upsample_logits(disp_low, logits, scale=4.0):
    """disp_low (B, 1, h, w), logits (B, 9, 4h, 4w) -> context_upsample(disp_low * scale, softmax(logits, 1)), (B, 4h, 4w),
    in one pass and differentiable with respect to both.  `scale` is a positive power of two.  Tensors on a HIP device;
    non-fp32 inputs are cast with .float()."""
    disp_low, logits = disp_low.float(), logits.float()
    _ffi.require_gpu(disp_low, logits)
    B, c, h, w = disp_low.shape
    if c != 1 or tuple(logits.shape) != (B, 9, 4 * h, 4 * w):
        raise ValueError("context_upsample_logits: disp_low %s / logits %s" % (tuple(disp_low.shape), tuple(logits.shape)))
    return _ContextUpsampleLogitsFn.apply(disp_low.contiguous(), _aligned16(logits.contiguous()), float(scale))
