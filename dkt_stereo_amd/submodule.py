"""Cost-volume builders with the reference's free-function signatures.

``build_gwc_volume(ref, tgt, maxdisp, num_groups)`` is identical in
meta_arch/igev_stereo/submodule.py:160-170, meta_arch/gwcnet/submodules.py:48-58
and meta_arch/cgi/submodule.py.  ``build_concat_volume`` has two upstream
definitions that differ in the reference half; both are here:

    build_concat_volume          GwcNet semantics (gwcnet/submodules.py:25-36)
    build_concat_volume_igev     IGEV copy       (igev_stereo/submodule.py:207-218)

``build_gwc_concat_volume`` writes both into one (B, G+2C', D, H, W) buffer,
replacing the torch.cat of gwc_main.py:315.

These four builders are differentiable: with grad enabled and an input that requires grad the same forward
kernels run inside a ``torch.autograd.Function`` whose backward is dkt_gwc_volume_bwd / dkt_concat_volume_bwd /
dkt_gwc_concat_volume_bwd (volumes_bwd.hip).  Otherwise nothing changes: the plain call, the same bits.
"""
import torch

from . import _ffi
from . import upsample as _upsample


def _check_pair(ref, tgt):
    _ffi.require_gpu(ref, tgt)
    if ref.shape != tgt.shape:
        raise ValueError("feature maps disagree: %s vs %s" % (tuple(ref.shape), tuple(tgt.shape)))
    return ref.contiguous(), tgt.contiguous()


#: "mfma": the banded matrix product on the exact-fp32 matrix cores (dkt_gwc_volume_mfma) where it applies, else the VALU
#: kernel; "exact": always the VALU kernel, bit-identical to the C restatement's summation order.  (submodule.gwc_mode(...) switches.)
import os as _os
GWC_MODE = "mfma"


import contextlib as _contextlib


@_contextlib.contextmanager
def gwc_mode(mode):
    """Temporarily select the group-wise correlation kernel: "mfma" (default) or "exact" (VALU, the C oracle's order)."""
    global GWC_MODE
    if mode not in ("mfma", "exact"):
        raise ValueError("gwc_mode: 'mfma' or 'exact'")
    prev, GWC_MODE = GWC_MODE, mode
    try:
        yield
    finally:
        GWC_MODE = prev


def _gwc_into(ref, tgt, vol, maxdisp, num_groups, bstride):
    B, C, H, W = ref.shape
    assert C % num_groups == 0  # groupwise_correlation, submodule.py:154
    if GWC_MODE == "mfma":
        # E_UNSUPPORTED: shape outside the MFMA form -> the general kernel
        if _ffi.call("dkt_gwc_volume_mfma", ref, ref.data_ptr(), tgt.data_ptr(), vol.data_ptr(), B, C, H, W,
                     maxdisp, num_groups, bstride, ok=(_ffi.E_UNSUPPORTED,)) == 0:
            return
    _ffi.call("dkt_gwc_volume", ref, ref.data_ptr(), tgt.data_ptr(), vol.data_ptr(), B, C, H, W, maxdisp, num_groups, bstride)


def _concat_into(ref, tgt, vol, maxdisp, ref_masked, bstride):
    B, C, H, W = ref.shape
    _ffi.call("dkt_concat_volume", ref, ref.data_ptr(), tgt.data_ptr(), vol.data_ptr(), B, C, H, W,
              maxdisp, int(ref_masked), bstride)


def _gwc_volume(ref, tgt, maxdisp, num_groups):
    B, C, H, W = ref.shape
    vol = torch.empty((B, num_groups, maxdisp, H, W), device=ref.device, dtype=torch.float32)
    _gwc_into(ref, tgt, vol, maxdisp, num_groups, num_groups * maxdisp * H * W)
    return vol


def _concat_volume(ref, tgt, maxdisp, ref_masked):
    B, C, H, W = ref.shape
    vol = torch.empty((B, 2 * C, maxdisp, H, W), device=ref.device, dtype=torch.float32)
    _concat_into(ref, tgt, vol, maxdisp, ref_masked, 2 * C * maxdisp * H * W)
    return vol


def _gwc_concat_volume(gref, gtgt, cref, ctgt, maxdisp, num_groups):
    B, _, H, W = gref.shape
    Cc = cref.shape[1]
    ch = num_groups + 2 * Cc
    vol = torch.empty((B, ch, maxdisp, H, W), device=gref.device, dtype=torch.float32)
    bstride = ch * maxdisp * H * W
    _gwc_into(gref, gtgt, vol, maxdisp, num_groups, bstride)
    _concat_into(cref, ctgt, vol[:, num_groups:], maxdisp, True, bstride)
    return vol


def _grad_operand(g):
    """(tensor, batch stride) of an upstream gradient: read in place when only its batch stride is unusual
    (a batch-sliced view), else made contiguous."""
    g = g.float()
    B, ch, D, H, W = g.shape
    if g.stride()[1:] != (D * H * W, H * W, W, 1) or (B > 1 and g.stride(0) < ch * D * H * W):
        g = g.contiguous()
    return g, g.stride(0) if B > 1 else ch * D * H * W


def _needs_autograd(*tensors):
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


def _empty_or_none(need, like):
    return torch.empty_like(like) if need else None


class _GwcFn(torch.autograd.Function):
    """build_gwc_volume; backward dkt_gwc_volume_bwd."""

    @staticmethod
    def forward(ctx, ref, tgt, maxdisp, num_groups):
        ctx.meta = (maxdisp, num_groups)
        ctx.save_for_backward(ref, tgt)
        return _gwc_volume(ref, tgt, maxdisp, num_groups)

    @staticmethod
    def backward(ctx, gvol):
        ref, tgt = ctx.saved_tensors
        D, G = ctx.meta
        B, C, H, W = ref.shape
        gv, bstride = _grad_operand(gvol)
        gr = _empty_or_none(ctx.needs_input_grad[0], ref)
        gt = _empty_or_none(ctx.needs_input_grad[1], tgt)
        if gr is None and gt is None:
            return None, None, None, None
        _ffi.call("dkt_gwc_volume_bwd", ref, gv.data_ptr(), bstride, ref.data_ptr(), tgt.data_ptr(), _ffi.ptr(gr), _ffi.ptr(gt),
                  B, C, H, W, D, G)
        return gr, gt, None, None


class _ConcatFn(torch.autograd.Function):
    """build_concat_volume[_igev]; backward dkt_concat_volume_bwd (needs no saved feature maps)."""

    @staticmethod
    def forward(ctx, ref, tgt, maxdisp, ref_masked):
        ctx.meta = (maxdisp, ref_masked)
        ctx.shape = tuple(ref.shape)
        return _concat_volume(ref, tgt, maxdisp, ref_masked)

    @staticmethod
    def backward(ctx, gvol):
        D, ref_masked = ctx.meta
        B, C, H, W = ctx.shape
        gv, bstride = _grad_operand(gvol)
        mk = lambda need: torch.empty(ctx.shape, device=gv.device, dtype=torch.float32) if need else None  # noqa: E731
        gr, gt = mk(ctx.needs_input_grad[0]), mk(ctx.needs_input_grad[1])
        if gr is None and gt is None:
            return None, None, None, None
        _ffi.call("dkt_concat_volume_bwd", gv, gv.data_ptr(), bstride, _ffi.ptr(gr), _ffi.ptr(gt), B, C, H, W, D, int(ref_masked))
        return gr, gt, None, None


class _GwcConcatFn(torch.autograd.Function):
    """build_gwc_concat_volume; backward: both channel ranges of the buffer's gradient in ONE launch
    (dkt_gwc_concat_volume_bwd), read in place."""

    @staticmethod
    def forward(ctx, gref, gtgt, cref, ctgt, maxdisp, num_groups):
        ctx.meta = (maxdisp, num_groups)
        ctx.cat_shape = tuple(cref.shape)
        ctx.save_for_backward(gref, gtgt)
        return _gwc_concat_volume(gref, gtgt, cref, ctgt, maxdisp, num_groups)

    @staticmethod
    def backward(ctx, gvol):
        gref, gtgt = ctx.saved_tensors
        D, G = ctx.meta
        B, C, H, W = gref.shape
        Cc = ctx.cat_shape[1]
        gv, bstride = _grad_operand(gvol)
        need = ctx.needs_input_grad
        gr, gt = _empty_or_none(need[0], gref), _empty_or_none(need[1], gtgt)
        mk = lambda n: torch.empty(ctx.cat_shape, device=gv.device, dtype=torch.float32) if n else None  # noqa: E731
        cr, ct = mk(need[2]), mk(need[3])
        if gr is None and gt is None and cr is None and ct is None:
            return None, None, None, None, None, None
        _ffi.call("dkt_gwc_concat_volume_bwd", gv, gv.data_ptr(), bstride, gref.data_ptr(), gtgt.data_ptr(), _ffi.ptr(gr),
                  _ffi.ptr(gt), B, C, G, _ffi.ptr(cr), _ffi.ptr(ct), Cc, 1, H, W, D)
        return gr, gt, cr, ct, None, None


def build_gwc_volume(refimg_fea, targetimg_fea, maxdisp, num_groups):
    ref, tgt = _check_pair(refimg_fea, targetimg_fea)
    if _needs_autograd(ref, tgt):
        return _GwcFn.apply(ref, tgt, maxdisp, num_groups)
    return _gwc_volume(ref, tgt, maxdisp, num_groups)


def build_concat_volume(refimg_fea, targetimg_fea, maxdisp):
    ref, tgt = _check_pair(refimg_fea, targetimg_fea)
    if _needs_autograd(ref, tgt):
        return _ConcatFn.apply(ref, tgt, maxdisp, True)
    return _concat_volume(ref, tgt, maxdisp, True)


def build_concat_volume_igev(refimg_fea, targetimg_fea, maxdisp):
    ref, tgt = _check_pair(refimg_fea, targetimg_fea)
    if _needs_autograd(ref, tgt):
        return _ConcatFn.apply(ref, tgt, maxdisp, False)
    return _concat_volume(ref, tgt, maxdisp, False)


def build_gwc_concat_volume(gwc_ref, gwc_tgt, cat_ref, cat_tgt, maxdisp, num_groups):
    """GWCNet.forward with use_concat_volume (gwc_main.py:310-315) in one buffer:
    channels [0:G] group-wise correlation, [G:G+2C'] concat volume."""
    gref, gtgt = _check_pair(gwc_ref, gwc_tgt)
    cref, ctgt = _check_pair(cat_ref, cat_tgt)
    if _needs_autograd(gref, gtgt, cref, ctgt):
        return _GwcConcatFn.apply(gref, gtgt, cref, ctgt, maxdisp, num_groups)
    return _gwc_concat_volume(gref, gtgt, cref, ctgt, maxdisp, num_groups)


def _group_l2norm(x, num_groups):
    """x / (||x||_2 per channel group + 1e-05): meta_arch/cgi/submodule.py:149,168."""
    _ffi.require_gpu(x)
    _ffi.require_no_grad(x)
    x = x.float().contiguous()
    B, C, H, W = x.shape
    if C % num_groups != 0:
        raise AssertionError("C %% num_groups != 0")          # the reference asserts (submodule.py:145)
    y = torch.empty_like(x)
    _ffi.call("dkt_group_l2norm", x, x.data_ptr(), y.data_ptr(), B, C, H * W, num_groups, 1e-05)
    return y


def build_gwc_volume_norm(refimg_fea, targetimg_fea, maxdisp, num_groups):
    """meta_arch/cgi/submodule.py:154-164: group-wise correlation of features normalised per
    channel group.  The norm reduces over channels only, so normalising the two maps once and
    running the plain group-wise volume is the same computation as the reference's per-
    disparity slices.  Inference only: inputs that require grad are refused (the normalisation has no
    backward here; CGI is not trainable on this library)."""
    return build_gwc_volume(_group_l2norm(refimg_fea, num_groups), _group_l2norm(targetimg_fea, num_groups),
                            maxdisp, num_groups)


def build_norm_correlation_volume(refimg_fea, targetimg_fea, maxdisp):
    """meta_arch/cgi/submodule.py:171-180 (== igev_stereo/submodule.py:179): (B,1,D,H,W).  Inference only, like
    build_gwc_volume_norm."""
    return build_gwc_volume_norm(refimg_fea, targetimg_fea, maxdisp, 1)


def context_upsample(disp_low, up_weights):
    """meta_arch/igev_stereo/submodule.py:242-254: (B,1,h,w), (B,9,4h,4w) -> (B,4h,4w).  With grad enabled and an input that
    requires grad the same kernel runs inside upsample._ContextUpsampleFn (the same bits, HIP backward); non-fp32 inputs
    are cast with .float() and autograd casts their gradients back."""
    disp_low, up_weights = disp_low.float(), up_weights.float()
    _ffi.require_gpu(disp_low, up_weights)
    b, c, h, w = disp_low.shape
    if c != 1 or tuple(up_weights.shape) != (b, 9, 4 * h, 4 * w):
        raise ValueError("context_upsample: disp_low %s / up_weights %s" % (tuple(disp_low.shape), tuple(up_weights.shape)))
    disp_low = disp_low.contiguous()
    up_weights = up_weights.contiguous()
    return _upsample.context_upsample_weights(disp_low, up_weights, _needs_autograd(disp_low, up_weights))


#: meta_arch/cgi/submodule.py:220-228, one launch (topk_regress.hip); disparity_samples may be None for "the plane index"
from .topk import regression_topk  # noqa: E402,F401


def disparity_regression(x, maxdisp):
    """igev_stereo/submodule.py:220-224 (keepdim=True flavour)."""
    assert len(x.shape) == 4
    disp_values = torch.arange(0, maxdisp, dtype=x.dtype, device=x.device).view(1, maxdisp, 1, 1)
    return torch.sum(x * disp_values, 1, keepdim=True)
