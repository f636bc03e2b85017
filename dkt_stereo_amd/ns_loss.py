"""The NeRF-supervised loss on HIP (csrc/ns_loss.hip): ``ns_loss`` (meta_arch/nerf_stereo/loss.py:128-181) with the
reference's signature, returns, exceptions and assertions, ``trinocular_loss`` (:92-109), its single-prediction term, and
``photometric_planes``, the per-pixel handle of the tests.

One call is three forward launches (loss_2 and the valid plane once; one tiled launch over every prediction; finalize) and
one backward launch.  The predictions are read in place through a pointer table (the students' ``[:, :1]`` views included);
what the backward needs per pixel is one byte per prediction (automask and the branch of the minimum), the warps and window
statistics are recomputed.  The sums are fp64 block partials reduced in a fixed order, so loss and gradients are
bit-identical from run to run.  The reference's data-dependent behaviour (the NaN/Inf assertion) and its Python-float
metrics come from one host read of a small record per call.

The module stands beside loss.py: it is not an entry of ``loss.__losses__`` (INTEGRATION.md shows how to put it into the
reference's own table).
"""
import torch

from . import _ffi
from .loss import _gpu, _plane, _raft_weights


def _image(t, what):
    """fp32 (B,3,H,W) with the three planes of an image contiguous; batch-strided views are read in place."""
    _gpu(t, what)
    assert t.dim() == 4 and t.shape[1] == 3, "%s: a (B,3,H,W) image expected, got %s" % (what, tuple(t.shape))
    if t.dtype != torch.float32:
        t = t.float()
    B, C, H, W = t.shape
    if t.stride(3) != 1 or t.stride(2) != W or t.stride(1) != H * W or (B > 1 and t.stride(0) < C * H * W):
        t = t.contiguous()
    return t


def _map(t, what, shape):
    """fp32 (B,H,W) with contiguous planes."""
    _gpu(t, what)
    assert tuple(t.shape) == shape, [what, tuple(t.shape), shape]
    return _plane(t)


def _no_grad(*tensors):
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise _ffi.DktError("the images, conf and the target must not require grad (the HIP loss differentiates the "
                            "predictions only)")


class _NsLoss(torch.autograd.Function):
    """inputs: (spec, im0, im1, im2, conf, target | valid_in, pred_0 .. pred_{n-1});
    outputs: (loss, valid | None, rec, state | None, planes | None)."""

    @staticmethod
    def forward(ctx, spec, im0, im1, im2, conf, aux, *preds):
        weights, folded, conf_threshold, max_flow, alpha_disp, alpha_photo, want_planes = spec
        n = len(preds)
        B, _, H, W = im1.shape
        dev = im1.device
        d = _ffi.NsLossDesc()
        for i, p in enumerate(preds):
            d.pred[i], d.pred_bstride[i], d.weight[i] = p.data_ptr(), p.stride(0), weights[i]
        d.n = n
        for k, im in enumerate((im0, im1, im2)):
            d.im[k], d.im_bstride[k] = im.data_ptr(), im.stride(0)
        d.conf, d.conf_bstride = conf.data_ptr(), conf.stride(0)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        rec = torch.empty(_ffi.NS_REC, device=dev, dtype=torch.float64)
        valid = state = planes = None
        if folded:
            valid = torch.empty((B, H, W), device=dev, dtype=torch.bool)
            d.target, d.target_bstride, d.valid = aux.data_ptr(), aux.stride(0), valid.data_ptr()
        else:
            d.valid_in = aux.data_ptr()
        if alpha_photo != 0.0:
            state = torch.empty((n, B, H, W), device=dev, dtype=torch.uint8)
            d.state = state.data_ptr()
        if want_planes:
            planes = torch.empty((3, B, H, W), device=dev, dtype=torch.float32)
            d.planes = planes.data_ptr()
        d.conf_threshold, d.max_flow, d.alpha_disp, d.alpha_photo = conf_threshold, max_flow, alpha_disp, alpha_photo
        d.loss, d.rec, d.B, d.H, d.W = loss.data_ptr(), rec.data_ptr(), B, H, W
        ws = torch.empty(_ffi.size("dkt_ns_loss_workspace", B, H, W) // 8, device=dev, dtype=torch.float64)
        with torch.cuda.device(dev):
            _ffi.call("dkt_ns_loss", ws, d, ws.data_ptr())
        ctx.desc, ctx.n = d, n
        ctx.set_materialize_grads(False)
        extra = [t for t in (valid, state, planes) if t is not None]
        ctx.mark_non_differentiable(rec, *extra)
        # (keeps every pointer of the descriptor alive; autograd checks that nothing was modified in place)
        ctx.save_for_backward(im0, im1, im2, conf, aux, rec, *extra, *preds)
        return loss, valid, rec, state, planes

    @staticmethod
    def backward(ctx, gloss, *unused):
        saved = ctx.saved_tensors
        preds = saved[len(saved) - ctx.n:]
        dev = preds[0].device
        if gloss is None:
            return (None,) * 6 + tuple(torch.zeros(p.shape, device=dev, dtype=torch.float32) for p in preds)
        up = gloss.float().contiguous()
        g = _ffi.NsLossGrad()
        g.grad_loss = up.data_ptr()
        out = []
        for i, p in enumerate(preds):
            t = torch.empty(p.shape, device=dev, dtype=torch.float32)
            out.append(t)
            g.grad[i] = t.data_ptr()
        with torch.cuda.device(dev):
            _ffi.call("dkt_ns_loss_bwd", preds[0], ctx.desc, g)
        return (None,) * 6 + tuple(out)


def _predictions(pred_disps, shape):
    n = len(pred_disps)
    if n > _ffi.NS_MAX_PRED:
        raise _ffi.DktError("%d predictions: the loss takes at most DKT_NS_MAX_PRED = %d" % (n, _ffi.NS_MAX_PRED))
    preds = []
    for p in pred_disps:
        _gpu(p, "prediction")
        assert tuple(p.shape) == shape, [tuple(p.shape), shape]
        preds.append(_plane(p))
    return preds


def _ns(pred_disps, target_disp, conf, im0, im1, im2, trinocular_loss, alpha_disp_loss, alpha_photometric, conf_threshold,
        max_flow):
    if alpha_photometric != 0. and not trinocular_loss:
        raise TypeError("binocular_loss() got an unexpected keyword argument 'valid'")
    n = len(pred_disps)
    assert n >= 1
    im0, im1, im2 = _image(im0, "im0"), _image(im1, "im1"), _image(im2, "im2")
    B, _, H, W = im1.shape
    assert im0.shape == im1.shape == im2.shape, [im0.shape, im1.shape, im2.shape]
    target = _map(target_disp, "target_disp", (B, H, W))
    conf = _map(conf, "conf", (B, H, W))
    _no_grad(im0, im1, im2, conf, target)
    preds = _predictions(pred_disps, (B, 1, H, W))
    spec = (_raft_weights(n, 0.9), True, float(conf_threshold), float(max_flow), float(alpha_disp_loss),
            float(alpha_photometric), False)
    loss, valid, rec, state, _ = _NsLoss.apply(spec, im0, im1, im2, conf, target, *preds)
    rec = rec.cpu().tolist()                   # the call's one host read
    assert not rec[5]                          # :155, before the weights of :157
    if n == 1:
        raise ZeroDivisionError("division by zero")             # loss_gamma ** (15 / (n_predictions - 1)), :157
    metrics = {'epe': rec[1], '1px': rec[2], '3px': rec[3], '5px': rec[4]}
    return loss, metrics, valid, state


def ns_loss(pred_disps, target_disp, conf, im0, im1, im2, trinocular_loss=True, alpha_disp_loss=1.0, alpha_photometric=0.1,
            conf_threshold=0.5, max_flow=512):
    """meta_arch/nerf_stereo/loss.py:128-181: (loss, metrics, valid).  pred_disps: n tensors (B,1,H,W), negative
    disparities; target_disp, conf: (B,H,W); im0, im1, im2: (B,3,H,W), im1 the centre view.  One autograd node over the
    predictions, one host read.  Raises what the reference raises: AssertionError for a NaN or Inf in a prediction (:155),
    ZeroDivisionError for a single prediction (:157), TypeError for trinocular_loss=False (:126 passes binocular_loss a
    keyword it does not take)."""
    return _ns(pred_disps, target_disp, conf, im0, im1, im2, trinocular_loss, alpha_disp_loss, alpha_photometric,
               conf_threshold, max_flow)[:3]


def ns_loss_decisions(pred_disps, target_disp, conf, im0, im1, im2, trinocular_loss=True, alpha_disp_loss=1.0,
                      alpha_photometric=0.1, conf_threshold=0.5, max_flow=512):
    """ns_loss with the decisions its kernels took: (loss, metrics, valid, automask, third), the last two bool (n,B,H,W) (None
    when alpha_photometric is 0): where the photometric term counts, and where the third view won the minimum.  The tests
    compare the loss and its gradients with the float64 truth under these decisions."""
    loss, metrics, valid, state = _ns(pred_disps, target_disp, conf, im0, im1, im2, trinocular_loss, alpha_disp_loss,
                                      alpha_photometric, conf_threshold, max_flow)
    if state is None:
        return loss, metrics, valid, None, None
    return loss, metrics, valid, (state & 1).bool(), (state & 2).bool()


def _single(disp, im1, im2, im3, uncertainty, valid, want_planes):
    im1, im2, im3 = _image(im1, "im1"), _image(im2, "im2"), _image(im3, "im3")
    B, _, H, W = im2.shape
    assert im1.shape == im2.shape == im3.shape, [im1.shape, im2.shape, im3.shape]
    unc = _map(uncertainty, "uncertainty", (B, H, W))
    _gpu(valid, "valid")
    mask = valid.squeeze(1).bool().contiguous()
    assert tuple(mask.shape) == (B, H, W), [tuple(mask.shape), (B, H, W)]
    _no_grad(im1, im2, im3, unc)
    (pred,) = _predictions([disp], (B, 1, H, W))
    spec = ([1.0], False, 0.0, 0.0, 0.0, 1.0, want_planes)
    return _NsLoss.apply(spec, im1, im2, im3, unc, mask, pred)


def trinocular_loss(disp, im1, im2, im3, uncertainty, valid=None):
    """meta_arch/nerf_stereo/loss.py:92-109: the mean of min(p12, p23) * uncertainty over (loss_warp < loss_2) & valid, a
    device scalar (NaN for an empty automask).  disp (B,1,H,W); im2 is the centre view; uncertainty (B,H,W); valid
    (B,1,H,W) -- the reference's default of None fails at `valid.squeeze(1)` and does here."""
    if valid is None:
        raise AttributeError("'NoneType' object has no attribute 'squeeze'")
    return _single(disp, im1, im2, im3, uncertainty, valid, False)[0]


def photometric_planes(disp, im1, im2, im3):
    """(p12, p23, loss_2), each (B,H,W) fp32: the photometric losses of the centre view im2 against the two warped views
    (:96-97) and the minimum over the unwarped ones (:100-102), per pixel, from the same launches as the loss with their
    plane output switched on.  Not differentiable; it is the handle the tests hold the kernels by, pixel by pixel."""
    B, _, H, W = im2.shape
    _gpu(disp, "disp")
    with torch.no_grad():
        ones = torch.ones((B, H, W), device=disp.device, dtype=torch.float32)
        planes = _single(disp, im1, im2, im3, ones, ones[:, None], True)[4]
    return planes[0], planes[1], planes[2]
