"""The stereo students' sequence losses on HIP (csrc/stereo_loss.hip): sequence_loss_raft
(meta_arch/raft_stereo/loss.py:3-40) and loss_gwcnet (meta_arch/gwcnet/gwc_loss.py:5-31) with the reference's signatures
and returns, and ``dkt_loss_pair``, the two calls of tools/ft_dkt.py:227-228 (ground truth and pseudo label) fused.

Each call is two forward launches and one backward launch; the predictions are read in place through a pointer table
(the students' ``[:, :1]`` views included), once per direction however many targets there are.  The sums are fp64
block partials reduced in a fixed order, so losses and gradients are bit-identical from run to run.  The reference's
data-dependent returns (``None`` for a NaN prediction, the Inf assertion) and its Python-float metrics come from one
host read of a small record per call; the backward reads the upstream gradients and counts on the device.
"""
import torch

from . import _ffi

#: loss.py:8 / gwc_loss.py:15
GWC_WEIGHTS = (0.5, 0.5, 0.7, 1.0)


def _gpu(t, what):
    if not t.is_cuda:
        raise _ffi.DktError("dkt_stereo_amd operators run on a HIP device only (%s is a %s tensor); there is no CPU path"
                            % (what, t.device))
    return t


def _plane(t):
    """fp32 with contiguous H x W planes (converted or copied once when not; both are differentiable)."""
    if t.dtype != torch.float32:
        t = t.float()
    H, W = t.shape[-2], t.shape[-1]
    if (W > 1 and t.stride(-1) != 1) or (H > 1 and t.stride(-2) != W):
        t = t.contiguous()
    return t


class _SeqLoss(torch.autograd.Function):
    """inputs: (spec, gt_0, valid_0[, gt_1, valid_1], pred_0 .. pred_{n-1}); outputs: (loss_0[, loss_1], mask_0[, mask_1], rec)."""

    @staticmethod
    def forward(ctx, spec, *tensors):
        kind, K, n, n_loss, weights, max_flow = spec
        gts, valids, preds = tensors[0:2 * K:2], tensors[1:2 * K:2], tensors[2 * K:]
        B, _, H, W = gts[0].shape
        dev = gts[0].device
        d = _ffi.SeqLossDesc()
        for i, p in enumerate(preds):
            d.pred[i], d.pred_bstride[i] = p.data_ptr(), p.stride(0)
        for i in range(n_loss):
            d.weight[i] = weights[i]
        d.n, d.n_loss, d.kind, d.ntargets = n, n_loss, kind, K
        losses = [torch.empty((), device=dev, dtype=torch.float32) for _ in range(K)]
        masks = [torch.empty((B, 1, H, W), device=dev, dtype=torch.bool) for _ in range(K)]
        rec = torch.empty(_ffi.LOSS_REC, device=dev, dtype=torch.float64)
        for k in range(K):
            d.gt[k], d.gt_bstride[k] = gts[k].data_ptr(), gts[k].stride(0)
            d.valid[k], d.valid_bstride[k] = valids[k].data_ptr(), valids[k].stride(0)
            d.mask[k], d.loss[k] = masks[k].data_ptr(), losses[k].data_ptr()
        d.max_flow = max_flow
        d.rec, d.B, d.H, d.W = rec.data_ptr(), B, H, W
        ws = torch.empty(_ffi.size("dkt_seq_loss_ws_doubles", K, n, B, H, W), device=dev, dtype=torch.float64)
        with torch.cuda.device(dev):
            _ffi.call("dkt_seq_loss", ws, d, ws.data_ptr())
        ctx.desc, ctx.K, ctx.n = d, K, n
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*masks, rec)
        ctx.save_for_backward(*gts, *preds, *masks, rec)
        return (*losses, *masks, rec)

    @staticmethod
    def backward(ctx, *grads):
        saved = ctx.saved_tensors              # (keeps every pointer of ctx.desc alive; checks nothing was modified in place)
        preds = saved[ctx.K:ctx.K + ctx.n]
        dev = preds[0].device
        g = _ffi.SeqLossGrad()
        ups = []
        for k in range(ctx.K):
            up = grads[k]
            up = torch.zeros((), device=dev, dtype=torch.float32) if up is None else up.float().contiguous()
            ups.append(up)
            g.grad_loss[k] = up.data_ptr()
        out = []
        for i, p in enumerate(preds):
            t = torch.empty(p.shape, device=dev, dtype=torch.float32)
            out.append(t)
            g.grad[i] = t.data_ptr()
        with torch.cuda.device(dev):
            _ffi.call("dkt_seq_loss_bwd", preds[0], ctx.desc, g)
        return (None,) + (None,) * (2 * ctx.K) + tuple(out)


def _raft_weights(n, loss_gamma):
    if n == 1:
        return [1.0]            # never used: the reference raises ZeroDivisionError (or returns None) first
    adjusted_loss_gamma = loss_gamma ** (15 / (n - 1))          # loss.py:25-26, in double as Python computes it
    return [adjusted_loss_gamma ** (n - i - 1) for i in range(n)]


def _run(kind, flow_preds, targets):
    """Checks and prepares `targets` = [(flow_gt, valid), ...] and the predictions: (n, n_loss, GwcNet weights, tensors)."""
    n = len(flow_preds)
    if n > _ffi.LOSS_MAX_PRED:
        raise _ffi.DktError("%d predictions: the loss takes at most DKT_LOSS_MAX_PRED = %d" % (n, _ffi.LOSS_MAX_PRED))
    tensors = []
    for k, (gt, valid) in enumerate(targets):
        _gpu(gt, "flow_gt")
        _gpu(valid, "valid")
        if torch.is_grad_enabled() and (gt.requires_grad or valid.requires_grad):
            raise _ffi.DktError("the loss targets must not require grad (the HIP loss differentiates the predictions only)")
        assert gt.dim() == 4 and gt.shape[1] == 1, "one-channel disparity (B,1,H,W) expected, got %s" % (tuple(gt.shape),)
        assert (valid.shape[0],) + (1,) + tuple(valid.shape[1:]) == tuple(gt.shape), [valid.shape, gt.shape]
        tensors += [_plane(gt), _plane(valid)]
    shape = tuple(targets[0][0].shape)
    for p in flow_preds:
        _gpu(p, "prediction")
        assert tuple(p.shape) == shape, [tuple(p.shape), shape]
        tensors.append(_plane(p))
    if kind == _ffi.LOSS_RAFT:
        n_loss, weights = n, None
    else:
        n_loss = min(n, len(GWC_WEIGHTS))      # zip(flow_preds, weights)
        weights = GWC_WEIGHTS[:n_loss]
    return n, n_loss, weights, tensors


def _apply(kind, K, n, n_loss, weights, max_flow, tensors):
    out = _SeqLoss.apply((kind, K, n, n_loss, weights, float(max_flow)), *tensors)
    losses, masks, rec = out[:K], out[K:2 * K], out[2 * K]
    return losses, masks, rec.cpu().tolist()       # the call's one host read


def _metrics(rec, k):
    r = rec[8 * k:8 * k + 5]
    return {'epe': r[1], '1px': r[2], '3px': r[3], '5px': r[4]}


def sequence_loss_raft(results, flow_gt, valid, loss_gamma=0.9, max_flow=700, args=None):
    """meta_arch/raft_stereo/loss.py:3-40: (flow_loss, metrics, valid) or (None, None, None)."""
    flow_preds = results['disp_preds']
    assert len(flow_preds) >= 1
    n, n_loss, _, tensors = _run(_ffi.LOSS_RAFT, flow_preds, [(flow_gt, valid)])
    (loss,), (mask,), rec = _apply(_ffi.LOSS_RAFT, 1, n, n_loss, _raft_weights(n, loss_gamma), max_flow, tensors)
    if rec[5] or rec[16]:
        return None, None, None
    if n == 1:
        raise ZeroDivisionError("division by zero")            # loss_gamma**(15/(n_predictions - 1)), loss.py:25
    return loss, _metrics(rec, 0), mask


def loss_gwcnet(results, flow_gt, valid, args=None):
    """meta_arch/gwcnet/gwc_loss.py:5-31: (flow_loss, metrics, valid); max_flow = args.maxdisp."""
    flow_preds = results['disp_preds']
    max_flow = args.maxdisp
    if not flow_preds:
        raise IndexError("list index out of range")            # flow_preds[-1], gwc_loss.py:21
    n, n_loss, weights, tensors = _run(_ffi.LOSS_GWC, flow_preds, [(flow_gt, valid)])
    (loss,), (mask,), rec = _apply(_ffi.LOSS_GWC, 1, n, n_loss, weights, max_flow, tensors)
    assert not rec[5]
    return loss, _metrics(rec, 0), mask


#: keyed like meta_arch/__init__.py:15-21 (the two losses whose students this library trains)
__losses__ = {
    "sequence_loss_raft": sequence_loss_raft,
    "loss_gwcnet": loss_gwcnet,
}


def dkt_loss_pair(loss_name, results, gt_aug, valid_gt_aug, pl_aug, valid_pl_aug, args=None):
    """tools/ft_dkt.py:227-228 in one forward (each prediction read once) and one backward launch, one host read:

        loss_GT, metrics, valid_final = loss_func(results, disp_gt_AUG, valid_gt_AUG, args=args)
        loss_PL, _, valid_final_PL = loss_func(results, disp_pl_AUG, valid_pl_AUG, args=args)

    Returns (loss_GT, metrics, valid_final, loss_PL, valid_final_PL), each part what its call returns."""
    if loss_name not in __losses__:
        raise _ffi.DktError("dkt_loss_pair: no HIP loss %r (have %s)" % (loss_name, sorted(__losses__)))
    flow_preds = results['disp_preds']
    targets = [(gt_aug, valid_gt_aug), (pl_aug, valid_pl_aug)]
    if loss_name == "sequence_loss_raft":
        kind, max_flow = _ffi.LOSS_RAFT, 700
        assert len(flow_preds) >= 1
    else:
        kind, max_flow = _ffi.LOSS_GWC, args.maxdisp
        if not flow_preds:
            raise IndexError("list index out of range")
    n, n_loss, weights, tensors = _run(kind, flow_preds, targets)
    if kind == _ffi.LOSS_RAFT:
        weights = _raft_weights(n, 0.9)
    (loss_gt, loss_pl), masks, rec = _apply(kind, 2, n, n_loss, weights, max_flow, tensors)
    out = []
    for k, loss in enumerate((loss_gt, loss_pl)):
        if kind == _ffi.LOSS_RAFT:
            if rec[8 * k + 5] or rec[16]:
                out.append((None, None, None))
                continue
            if n == 1:
                raise ZeroDivisionError("division by zero")
        else:
            assert not rec[8 * k + 5]
        out.append((loss, _metrics(rec, k), masks[k]))
    (loss_GT, metrics, valid_final), (loss_PL, _, valid_final_PL) = out
    return loss_GT, metrics, valid_final, loss_PL, valid_final_PL
