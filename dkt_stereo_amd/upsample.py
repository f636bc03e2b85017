"""Convex up-sampling as an autograd node (RAFTStereo.upsample_flow on the training path, raft_stereo.py:70-82).

Forward: dkt_convex_upsample_fwd, the leading `channels` channels, bit-identical to the inference kernel's.  Backward:
dkt_convex_upsample_bwd, deterministic, the softmax recomputed from the mask (only flow and mask are saved)."""
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


class _ConvexUpsampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flow, mask, factor, channels):
        _ffi.require_gpu(flow, mask)
        N, D, H, W = flow.shape
        if mask.shape != (N, 9 * factor * factor, H, W):
            raise _ffi.DktError("upsample mask %s does not match flow %s at factor %d" % (tuple(mask.shape), tuple(flow.shape), factor))
        flow, mask = flow.contiguous(), mask.contiguous()
        out = torch.empty((N, channels, factor * H, factor * W), device=flow.device, dtype=torch.float32)
        rc = _ffi.lib().dkt_convex_upsample_fwd(flow.data_ptr(), mask.data_ptr(), out.data_ptr(), N, D, channels, H, W, factor,
                                                _ffi.device_of(flow), _ffi.stream_of(flow))
        _ffi.check(rc, "dkt_convex_upsample_fwd")
        ctx.save_for_backward(flow, mask)
        ctx.factor, ctx.channels = factor, channels
        return out

    @staticmethod
    def backward(ctx, gout):
        flow, mask = ctx.saved_tensors
        need_flow, need_mask = ctx.needs_input_grad[:2]
        if not (need_flow or need_mask):
            return None, None, None, None
        _ffi.require_gpu(gout)
        N, D, H, W = flow.shape
        gout, bstride = _batch_strided(gout)
        gflow = torch.empty_like(flow) if need_flow else None
        gmask = torch.empty_like(mask) if need_mask else None
        ws = torch.empty((N, ctx.channels, 9, H, W), device=flow.device, dtype=torch.float32) if need_flow else None
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        rc = _ffi.lib().dkt_convex_upsample_bwd(gout.data_ptr(), bstride, flow.data_ptr(), mask.data_ptr(), ptr(gflow), ptr(gmask),
                                                ptr(ws), N, D, ctx.channels, H, W, ctx.factor,
                                                _ffi.device_of(flow), _ffi.stream_of(flow))
        _ffi.check(rc, "dkt_convex_upsample_bwd")
        return gflow, gmask, None, None


def convex_upsample(flow, mask, factor, channels=None):
    """flow (N, D, H, W), mask (N, 9 f^2, H, W) -> the leading `channels` (default D) channels of the convex
    up-sampling, (N, channels, f H, f W), differentiable with respect to both.  fp32 tensors on a HIP device."""
    D = flow.shape[1]
    channels = D if channels is None else channels
    if not 1 <= channels <= D:
        raise _ffi.DktError("channels = %d outside 1..%d" % (channels, D))
    return _ConvexUpsampleFn.apply(flow, mask, factor, channels)
