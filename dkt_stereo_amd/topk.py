"""CGI-Stereo's top-k disparity head as one operator and one autograd node (topk_regress.hip).

regression_topk(cost, disparity_samples, k) keeps the signature of meta_arch/cgi/submodule.py:220-228 (a full descending
sort of every pixel's column, two gathers, a softmax over the k kept values, a product and a sum); disparity_samples=None
stands for the plane index, which is what CGI passes as an arange repeated to (B, D, h, w) (CGI_Stereo.py:256-259).  The
sorted volume never exists.  Forward: dkt_topk_regress_fwd.  Backward: dkt_topk_regress_bwd, deterministic; the node saves
the cost, the samples if given and k bytes per pixel.  cgi_disparity_head restates CGI_Stereo.py:253-268 on it."""
import torch
from torch.autograd.function import once_differentiable

from . import _ffi
from . import upsample as _upsample
from .soft_argmin import _batch_strided

MAX_K = 8
MAX_D = 256


def _forward(cost, cbs, samples, sbs, k, idx=None):
    B, D, h, w = cost.shape
    out = torch.empty((B, 1, h, w), device=cost.device, dtype=torch.float32)
    _ffi.call("dkt_topk_regress_fwd", cost, cost.data_ptr(), cbs, _ffi.ptr(samples), sbs, out.data_ptr(), _ffi.ptr(idx),
              B, D, h, w, k)
    return out


class _TopkRegressFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cost, samples, k):
        cost, cbs = _batch_strided(cost)
        sbs = 0
        if samples is not None:
            samples, sbs = _batch_strided(samples)
        B, D, h, w = cost.shape
        idx = torch.empty((B, k, h, w), device=cost.device, dtype=torch.uint8)
        out = _forward(cost, cbs, samples, sbs, k, idx)
        ctx.save_for_backward(cost, samples, idx)
        ctx.cbs, ctx.sbs, ctx.k = cbs, sbs, k
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        need_cost, need_samples = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not need_cost and not need_samples:
            return None, None, None
        cost, samples, idx = ctx.saved_tensors
        B, D, h, w = cost.shape
        _ffi.require_gpu(gout)
        g, gbs = _batch_strided(gout)
        gcost = torch.empty((B, D, h, w), device=cost.device, dtype=torch.float32) if need_cost else None
        gsamples = torch.empty((B, D, h, w), device=cost.device, dtype=torch.float32) if need_samples else None
        _ffi.call("dkt_topk_regress_bwd", cost, g.data_ptr(), gbs, cost.data_ptr(), ctx.cbs, _ffi.ptr(samples), ctx.sbs,
                  idx.data_ptr(), _ffi.ptr(gcost), _ffi.ptr(gsamples), B, D, h, w, ctx.k)
        return gcost, gsamples, None


def regression_topk(cost, disparity_samples, k):
    """cost (B, D, h, w), disparity_samples (B, D, h, w) or None (the plane index) -> sum_i s_i softmax_i(c)_i over the k
    largest entries c_i of every pixel's column (ties to the lowest plane) and their samples s_i, (B, 1, h, w) fp32.
    1 <= k <= min(D, 8), D <= 256.  Differentiable with respect to cost and the samples.  Tensors on a HIP device; non-fp32
    inputs are cast with .float(); batch-strided inputs are read in place."""
    if cost.dim() != 4:
        raise ValueError("regression_topk: cost %s" % (tuple(cost.shape),))
    if disparity_samples is not None and tuple(disparity_samples.shape) != tuple(cost.shape):
        raise ValueError("regression_topk: cost %s / disparity_samples %s" % (tuple(cost.shape), tuple(disparity_samples.shape)))
    D = cost.shape[1]
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= min(D, MAX_K):
        raise _ffi.DktError("regression_topk: k = %r outside 1..min(D = %d, %d)" % (k, D, MAX_K))
    if D > MAX_D:
        raise _ffi.DktError("regression_topk: D = %d beyond %d" % (D, MAX_D))
    cost = cost.float()
    samples = None if disparity_samples is None else disparity_samples.float()
    _ffi.require_gpu(*((cost,) if samples is None else (cost, samples)))
    if torch.is_grad_enabled() and (cost.requires_grad or (samples is not None and samples.requires_grad)):
        return _TopkRegressFn.apply(cost, samples, int(k))
    cost, cbs = _batch_strided(cost)
    sbs = 0
    if samples is not None:
        samples, sbs = _batch_strided(samples)
    return _forward(cost, cbs, samples, sbs, int(k))


def cgi_disparity_head(cost, spx_logits, k=2, training=False):
    """CGI_Stereo.forward's head (CGI_Stereo.py:253-268) from the hourglass's cost (B, 1, D, h, w) or (B, D, h, w) and the
    logits of the nine up-sampling weights (B, 9, 4h, 4w), before their softmax: two launches, the regression over the k
    largest planes and upsample.context_upsample_logits (softmax, x4, the nine-neighbour blend).  Returns
    [-4 pred (B, 1, h, w), -up (B, 1, 4h, 4w)] when `training`, else -up."""
    if cost.dim() == 5:
        if cost.shape[1] != 1:
            raise ValueError("cgi_disparity_head: cost %s" % (tuple(cost.shape),))
        cost = cost[:, 0]
    pred = regression_topk(cost, None, k)
    up = _upsample.context_upsample_logits(pred, spx_logits, 4.0)
    if training:
        return [-4.0 * pred, -up.unsqueeze(1)]
    return -up.unsqueeze(1)
