"""DKT's Filter-and-Ensemble (FandE/__init__.py of the reference) on HIP (csrc/fande.hip).

``FandE_Filter`` and ``FandE_Ensemble`` keep the reference's signatures and results and are drop-ins for
``from FandE import FandE_Filter, FandE_Ensemble``.  ``fande_targets`` is the sequence of tools/ft_dkt.py:203-210 (F&E of
the ground truth and of the pseudo label against the EMA teacher) in two launches, with the pseudo label's all-ones mask
never materialised.

Random draws follow the reference's generators in its order and count -- ``torch.rand((B, 1))`` on the CPU default
generator per ``withprob`` Filter, ``random.random()`` per Ensemble -- and travel to the kernel as launch arguments, so
seeding ``random`` and ``torch`` reproduces the reference's pseudo labels bit for bit and no call here synchronises.
The results are bit-identical to the reference's on the same inputs and draws (0/1 masks: the per-image counts of the
``withprob`` ratio are exact).
"""
import random

import torch

from . import _ffi


def _plane(t, shape, what):
    """`t` as an fp32 tensor of `shape` whose H x W planes are contiguous (converted or copied once when not)."""
    if not t.is_cuda:
        raise _ffi.DktError("dkt_stereo_amd operators run on a HIP device only (%s is a %s tensor); there is no CPU path"
                            % (what, t.device))
    if tuple(t.shape) != tuple(shape):
        raise _ffi.DktError("%s: expected shape %s, got %s" % (what, tuple(shape), tuple(t.shape)))
    if t.dtype != torch.float32:
        t = t.float()
    H, W = shape[-2], shape[-1]
    if (W > 1 and t.stride(-1) != 1) or (H > 1 and t.stride(-2) != W):
        t = t.contiguous()
    return t


def _dims(source):
    if source.dim() != 4 or source.shape[1] != 1:
        raise _ffi.DktError("F&E takes one-channel disparity maps (B, 1, H, W), got %s" % (tuple(source.shape),))
    B, _, H, W = source.shape
    if B > _ffi.FANDE_MAX_B:
        raise _ffi.DktError("F&E: batch %d exceeds DKT_FANDE_MAX_B = %d" % (B, _ffi.FANDE_MAX_B))
    return B, H, W


def _job(src, tgt, valid, tau, filt, ensemble, clamp=False, ens_prob=0.0, rand=None):
    """One dkt_fande_job; returns (job, out, out_valid)."""
    B, H, W = src.shape[0], src.shape[-2], src.shape[-1]
    out = torch.empty((B, 1, H, W), device=src.device, dtype=torch.float32)
    out_valid = torch.empty((B, H, W), device=src.device, dtype=torch.float32) if filt else None
    j = _ffi.FandeJob()
    j.src, j.src_bstride = src.data_ptr(), src.stride(0)
    j.tgt, j.tgt_bstride = tgt.data_ptr(), tgt.stride(0)
    if valid is not None:
        j.valid, j.valid_bstride = valid.data_ptr(), valid.stride(0)
    j.out, j.out_bstride = out.data_ptr(), out.stride(0)
    if filt:
        j.out_valid, j.out_valid_bstride = out_valid.data_ptr(), out_valid.stride(0)
    j.tau = float(tau)          # `x < threshold` compares in fp32; ctypes rounds the scalar the same way
    j.filter, j.ensemble = filt, int(ensemble)
    if clamp:                                           # `if clamp:` of the reference: False / 0 / None do not clamp
        j.clamp, j.clamp_max = 1, float(clamp)
    j.ens_prob = ens_prob
    if rand is not None:
        for b, v in enumerate(rand.reshape(-1).tolist()):
            j.rand[b] = v
    return j, out, out_valid


def _launch(jobs, B, H, W, device, inputs):
    _ffi.require_no_grad(*inputs)
    arr = (_ffi.FandeJob * len(jobs))(*jobs)
    ws = torch.empty(_ffi.FANDE_WS_DOUBLES_PER_IMAGE * B * len(jobs), device=device, dtype=torch.float64)
    with torch.cuda.device(device):
        _ffi.call("dkt_fande", ws, arr, len(jobs), B, H, W, ws.data_ptr())


def FandE_Filter(source, target, valid, withprob=False, threshold=3):
    """FandE/__init__.py:24-39: returns (AUG_source (B,1,H,W), Aug_valid (B,H,W)).  Draws torch.rand((B, 1)) when withprob."""
    B, H, W = _dims(source)
    src = _plane(source, (B, 1, H, W), "source")
    tgt = _plane(target, (B, 1, H, W), "target")
    val = _plane(valid, (B, 1, H, W), "valid")
    rand = torch.rand((B, 1)) if withprob else None
    j, out, out_valid = _job(src, tgt, val, threshold, 2 if withprob else 1, False, rand=rand)
    _launch([j], B, H, W, src.device, (src, tgt, val))
    return out, out_valid


def FandE_Ensemble(source, target, valid, clamp=False, threshold=3):
    """FandE/__init__.py:4-21: returns AUG_source (B,1,H,W).  Draws random.random() once."""
    B, H, W = _dims(source)
    src = _plane(source, (B, 1, H, W), "source")
    tgt = _plane(target, (B, 1, H, W), "target")
    val = _plane(valid, (B, 1, H, W), "valid")
    prob = random.random()
    assert prob >= 0 and prob <= 1, [prob]
    j, out, _ = _job(src, tgt, val, threshold, 0, True, clamp=clamp, ens_prob=prob)
    _launch([j], B, H, W, src.device, (src, tgt, val))
    return out


def fande_targets(disp_gt, valid_gt, disp_pl, disp_t_ema, tau_gt, tau_pl, clamp):
    """tools/ft_dkt.py:203-210 in two launches:

        disp_gt_AUG, valid_gt_AUG = FandE_Filter(disp_gt, disp_T_EMA, valid_gt.unsqueeze(1), withprob=True, threshold=tau_gt)
        disp_gt_AUG = FandE_Ensemble(disp_gt_AUG, disp_T_EMA, valid_gt_AUG.unsqueeze(1), clamp=clamp, threshold=tau_gt)
        disp_pl_AUG, valid_pl_AUG = FandE_Filter(disp_pl, disp_T_EMA, ones, withprob=False, threshold=tau_pl)
        disp_pl_AUG = FandE_Ensemble(disp_pl_AUG, disp_T_EMA, valid_pl_AUG.unsqueeze(1), clamp=False, threshold=tau_pl)

    disp_gt, disp_pl, disp_t_ema: (B,1,H,W); valid_gt: (B,H,W).  Returns (disp_gt_AUG, valid_gt_AUG, disp_pl_AUG,
    valid_pl_AUG).  Consumes torch.rand((B, 1)) and two random.random() draws, as the four calls do."""
    B, H, W = _dims(disp_gt)
    gt = _plane(disp_gt, (B, 1, H, W), "disp_gt")
    vgt = _plane(valid_gt, (B, H, W), "valid_gt")
    pl = _plane(disp_pl, (B, 1, H, W), "disp_pl")
    t = _plane(disp_t_ema, (B, 1, H, W), "disp_t_ema")
    rand = torch.rand((B, 1))
    p_gt = random.random()
    assert p_gt >= 0 and p_gt <= 1, [p_gt]
    p_pl = random.random()
    assert p_pl >= 0 and p_pl <= 1, [p_pl]
    j_gt, gt_aug, vgt_aug = _job(gt, t, vgt, tau_gt, 2, True, clamp=clamp, ens_prob=p_gt, rand=rand)
    j_pl, pl_aug, vpl_aug = _job(pl, t, None, tau_pl, 1, True, clamp=False, ens_prob=p_pl)
    _launch([j_gt, j_pl], B, H, W, gt.device, (gt, vgt, pl, t))
    return gt_aug, vgt_aug, pl_aug, vpl_aug
