#!/usr/bin/env python3
"""Generates tests/golden/dkt.npz by RUNNING THE REFERENCE (build container only, needs the reference tree):

    python tests/golden/make_golden_dkt.py

  fande/<case>/...  FandE_Filter / FandE_Ensemble (FandE/__init__.py) and the four calls of tools/ft_dkt.py:203-210, on
                    inputs built to hit every branch: distances below, at and above tau, source == target ties, NaN and
                    Inf in the teacher output, an image with no valid pixel, an image that is entirely consistent.  Each
                    case stores its inputs, outputs, the seeds it ran under and the NEXT draw of both generators after
                    the call (torch.rand(1) on the CPU default generator, random.random()), so a test proves that the
                    library consumed exactly the draws the reference consumed.
  loss/<case>/...   sequence_loss_raft (meta_arch/raft_stereo/loss.py) and loss_gwcnet (meta_arch/gwcnet/gwc_loss.py):
                    predictions, target, valid, the loss, the metrics, the returned mask and the CPU autograd gradient
                    of 1.7 * loss with respect to every prediction; "none" = 1 where the reference returned None.

CPU, fp32.  Only data is stored: no reference source.
"""
import os
import random
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _refimport  # noqa: E402

OUT = os.path.join(HERE, "dkt.npz")


def load_reference():
    _refimport.setup()
    import importlib
    import types
    fande = importlib.import_module("FandE")
    # the reference's meta_arch/gwcnet package __init__ is broken (see _refimport); load the loss module by path
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_gwc_loss", os.path.join(_refimport.REF, "meta_arch", "gwcnet", "gwc_loss.py"))
    gwc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gwc)
    raft = importlib.import_module("meta_arch.raft_stereo.loss")
    return types.SimpleNamespace(Filter=fande.FandE_Filter, Ensemble=fande.FandE_Ensemble,
                                 sequence_loss_raft=raft.sequence_loss_raft, loss_gwcnet=gwc.loss_gwcnet)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def fande_inputs(seed, B, H, W, tau):
    """(source, target, valid (B,1,H,W) 0/1) with offsets below / at / above tau, ties, NaN / Inf in the target;
    image 1 (B >= 2) has no valid pixel, image 2 (B == 3) is entirely consistent."""
    g = np.random.default_rng(seed)
    tgt = g.uniform(-4.0, 60.0, (B, 1, H, W)).astype(np.float32)
    off = g.choice(np.array([0.0, 0.25 * tau, 0.999 * tau, tau, -tau, 1.001 * tau, 2.0 * tau, -5.0 * tau, 40.0], np.float32),
                   size=(B, 1, H, W))
    src = (tgt + off).astype(np.float32)
    valid = (g.uniform(size=(B, 1, H, W)) < 0.75).astype(np.float32)
    flat = tgt.reshape(B, -1)
    flat[0, 3], flat[0, 5], flat[0, 7] = np.nan, np.inf, -np.inf
    if B >= 2:
        valid[1] = 0.0
        flat[1, 2] = np.nan
    if B >= 3:
        src[2] = tgt[2] + np.float32(0.25 * tau)
        src[2, 0, 0, 0] = tgt[2, 0, 0, 0]
        valid[2] = 1.0
    return f32(src), f32(tgt), f32(valid)


def next_draws():
    return np.array([torch.rand(1).item(), random.random()], np.float64)


def main():
    torch.set_num_threads(4)
    ref = load_reference()
    arrays = {}
    T = torch.from_numpy

    # ---- F&E drop-ins -------------------------------------------------------------------------------------------
    shapes = {1: (7, 13), 2: (9, 17), 3: (5, 11)}
    for B in (1, 2, 3):
        H, W = shapes[B]
        for tau in (3.0, 0.5):
            src, tgt, valid = fande_inputs(1000 + 10 * B + int(tau * 2), B, H, W, tau)
            for withprob in (False, True):
                seed = 7 * B + int(withprob) + int(tau * 10)
                torch.manual_seed(seed)
                random.seed(seed)
                out, out_valid = ref.Filter(T(src), T(tgt), T(valid), withprob=withprob, threshold=tau)
                key = "fande/filter_B%d_t%g_p%d/" % (B, tau, int(withprob))
                arrays.update({key + "src": src, key + "tgt": tgt, key + "valid": valid,
                               key + "meta": np.array([seed, tau, float(withprob)], np.float64),
                               key + "out": f32(out.numpy()), key + "out_valid": f32(out_valid.numpy()),
                               key + "next": next_draws()})
            for clamp in (False, 1.0):
                seed = 31 * B + int(bool(clamp)) + int(tau * 10)
                torch.manual_seed(seed)
                random.seed(seed)
                out = ref.Ensemble(T(src), T(tgt), T(valid), clamp=clamp, threshold=tau)
                key = "fande/ensemble_B%d_t%g_c%g/" % (B, tau, float(clamp))
                arrays.update({key + "src": src, key + "tgt": tgt, key + "valid": valid,
                               key + "meta": np.array([seed, tau, float(clamp)], np.float64),
                               key + "out": f32(out.numpy()), key + "next": next_draws()})

    # ---- the fused sequence of tools/ft_dkt.py:203-210 -----------------------------------------------------------
    for B, clamp, tau_gt, tau_pl in ((2, False, 3.0, 3.0), (3, 1.0, 3.0, 0.5), (1, 1.0, 0.5, 3.0)):
        H, W = 11, 19
        gt, t_ema, valid = fande_inputs(2000 + B, B, H, W, tau_gt)
        pl_src, pl_tgt, _ = fande_inputs(3000 + B, B, H, W, tau_pl)
        pl = f32(t_ema + (pl_src - pl_tgt))       # the pseudo label: the teacher's output plus the same kind of offsets
        valid_gt = f32(valid[:, 0])
        seed = 500 + B
        torch.manual_seed(seed)
        random.seed(seed)
        disp_gt, disp_pl, disp_T_EMA, valid_gt_t = T(gt), T(pl), T(t_ema), T(valid_gt)
        valid_pl = torch.ones(disp_pl.shape).squeeze(1)
        disp_gt_AUG, valid_gt_AUG = ref.Filter(disp_gt, disp_T_EMA, valid_gt_t.unsqueeze(1), withprob=True, threshold=tau_gt)
        disp_gt_AUG = ref.Ensemble(disp_gt_AUG, disp_T_EMA, valid_gt_AUG.unsqueeze(1), clamp=clamp, threshold=tau_gt)
        disp_pl_AUG, valid_pl_AUG = ref.Filter(disp_pl, disp_T_EMA, valid_pl.unsqueeze(1), withprob=False, threshold=tau_pl)
        disp_pl_AUG = ref.Ensemble(disp_pl_AUG, disp_T_EMA, valid_pl_AUG.unsqueeze(1), clamp=False, threshold=tau_pl)
        key = "fande/fused_B%d/" % B
        arrays.update({key + "disp_gt": gt, key + "valid_gt": valid_gt, key + "disp_pl": pl, key + "disp_t_ema": t_ema,
                       key + "meta": np.array([seed, tau_gt, tau_pl, float(clamp)], np.float64),
                       key + "disp_gt_aug": f32(disp_gt_AUG.numpy()), key + "valid_gt_aug": f32(valid_gt_AUG.numpy()),
                       key + "disp_pl_aug": f32(disp_pl_AUG.numpy()), key + "valid_pl_aug": f32(valid_pl_AUG.numpy()),
                       key + "next": next_draws()})

    # ---- losses ----------------------------------------------------------------------------------------------------
    def loss_case(name, kind, preds, gt, valid, gamma=0.9, max_flow=700, maxdisp=192):
        pt = [T(p).requires_grad_(True) for p in preds]
        if kind == "raft":
            loss, metrics, vmask = ref.sequence_loss_raft({"disp_preds": pt}, T(gt), T(valid), loss_gamma=gamma, max_flow=max_flow)
        else:
            loss, metrics, vmask = ref.loss_gwcnet({"disp_preds": pt}, T(gt), T(valid), args=SimpleNamespace(maxdisp=maxdisp))
        key = "loss/%s/" % name
        gt, valid = gt.copy(), valid.copy()          # the callers go on editing their arrays for the next case
        arrays.update({key + "preds": f32(np.stack(preds)), key + "gt": gt, key + "valid": valid,
                       key + "meta": np.array([0 if kind == "raft" else 1, gamma, max_flow, maxdisp], np.float64),
                       key + "none": np.array(loss is None)})
        if loss is None:
            return
        (1.7 * loss).backward()
        grads = [p.grad if p.grad is not None else torch.zeros_like(p) for p in pt]
        arrays.update({key + "loss": np.array(loss.item(), np.float32),
                       key + "metrics": np.array([metrics[k] for k in ("epe", "1px", "3px", "5px")], np.float64),
                       key + "mask": vmask.numpy(), key + "grads": f32(torch.stack(grads).numpy())})

    def target(seed, B, H, W, scale=1.0):
        g = np.random.default_rng(seed)
        gt = (g.uniform(0.0, 80.0, (B, 1, H, W)) * scale).astype(np.float32)
        valid = g.choice(np.array([0.0, 0.49, 0.5, 1.0, 1.0, 1.0], np.float32), size=(B, H, W))
        return f32(gt), f32(valid)

    def preds_for(seed, gt, n, spread):
        g = np.random.default_rng(seed)
        return [f32(gt + g.normal(0.0, spread / (i + 1), gt.shape)) for i in range(n)]

    B, H, W = 2, 12, 20
    for n in (2, 3, 16):
        for gamma in (0.9, 0.8):
            gt, valid = target(40 + n, B, H, W)
            loss_case("raft_n%d_g%g" % (n, gamma), "raft", preds_for(50 + n, gt, n, 6.0), gt, valid, gamma=gamma)
    # ground truth around max_flow: magnitudes just below, at and above 700, negative disparities included; an Inf on a
    # pixel marked valid (mag < max_flow excludes it, so neither the None of loss.py:17 nor the assertion of gwc_loss.py:13 fires)
    gt, valid = target(61, B, H, W)
    gflat = gt.reshape(-1)
    gflat[:12] = np.array([699.0, 699.99994, 700.0, 700.00006, 701.0, -699.5, -700.0, -700.5, 1e6, -1e6, np.inf, 0.0], np.float32)
    valid.reshape(-1)[:12] = 1.0
    loss_case("raft_maxflow", "raft", preds_for(62, gt, 3, 4.0), gt, valid)
    # one image without a valid pixel, and a batch without any
    gt, valid = target(63, B, H, W)
    valid[0] = 0.0
    loss_case("raft_empty_image", "raft", preds_for(64, gt, 3, 4.0), gt, valid)
    valid[:] = 0.49
    loss_case("raft_empty", "raft", preds_for(65, gt, 3, 4.0), gt, valid)
    # the None trigger: a NaN and no Inf in a prediction (at an invalid pixel: the reference tests the whole tensor)
    gt, valid = target(66, B, H, W)
    valid[0, 0, 0] = 0.0
    for which, name in ((0, "raft_nan_first"), (2, "raft_nan_last")):
        ps = preds_for(67, gt, 3, 4.0)
        ps[which][0, 0, 0, 0] = np.nan
        loss_case(name, "raft", ps, gt, valid)
    # NaN together with Inf in the same prediction does not trigger it
    ps = preds_for(68, gt, 3, 4.0)
    ps[1][0, 0, 0, 0] = np.nan
    valid[0, 0, 1] = 0.0
    ps[1][0, 0, 0, 1] = np.inf
    loss_case("raft_nan_inf", "raft", ps, gt, valid)
    # GwcNet: |d| below, at and above 1 (beta), four predictions and three
    for n in (4, 3):
        gt, valid = target(70 + n, B, H, W, scale=2.5)
        g = np.random.default_rng(80 + n)
        offs = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 0.999, -1.001, 3.0, -7.0], np.float32)
        ps = [f32(gt + g.choice(offs, size=gt.shape)) for _ in range(n)]
        loss_case("gwc_n%d" % n, "gwc", ps, gt, valid, maxdisp=192)

    np.savez_compressed(OUT, **arrays)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(arrays), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
