#!/usr/bin/env python3
"""The tail of one DKT fine-tuning step (tools/ft_dkt.py:203-235 of the reference) at the recipe shape of
run_scripts/raft-stereo/ft_booster.sh (B = 2, 480 x 896, 16 RAFT predictions) and with GwcNet's four predictions:

  arm a  the reference's torch expression sequence, restated here: F&E of the ground truth and the pseudo label, the two
         loss calls (boolean-mask indexing, `if tensor.any()` tests, .item() metrics), backward() into the predictions;
  arm b  fande_targets + dkt_loss_pair + backward.

The arms alternate in one process after warm-up.  Per arm: wall ms per step (host clock around a step that ends in a
synchronise), the synchronising calls of one step (torch.cuda.set_sync_debug_mode("warn")), and for arm b the library
calls' device time from HIP events with the fraction of 8 TB/s their compulsory bytes would take.  Launch counts come from a
separate `rocprofv3 --kernel-trace --stats` run of `--arms b` / `--arms a`.

    python tools/bench_dkt_loss.py [--steps 20] [--warmup 5] [--arms a,b] [--loss raft,gwc]
"""
import argparse
import json
import os
import random
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dkt_stereo_amd.fande import fande_targets  # noqa: E402
from dkt_stereo_amd.loss import dkt_loss_pair  # noqa: E402

PEAK_BPS = 8e12
B, H, W = 2, 480, 896
TAU_GT, TAU_PL, CLAMP, MAXDISP = 3.0, 3.0, 1.0, 192


# ---- arm a: the reference's expressions, restated ------------------------------------------------------------------------
def _filter(source, target, valid, withprob, threshold):
    vc = torch.sum((target - source) ** 2, dim=1).sqrt() < threshold
    vc = vc.unsqueeze(1) * valid
    source = source * valid
    if withprob:
        ratio = vc.flatten(1).sum(dim=-1, keepdim=True) / valid.flatten(1).sum(dim=-1, keepdim=True)
        prob = torch.rand(ratio.shape).to(ratio.device)
        sel = (prob < ratio).unsqueeze(-1).unsqueeze(-1) * (1 - vc) * valid
        aug_valid = (vc + (1 - vc) * sel) * valid
    else:
        aug_valid = vc
    return source * aug_valid, aug_valid.squeeze(1)


def _ensemble(source, target, valid, clamp, threshold):
    vc = (torch.sum((target - source) ** 2, dim=1).sqrt() < threshold).unsqueeze(1) * valid
    source, target = source * valid, target * valid
    offset = random.random() * torch.sum((source - target) ** 2, dim=1).sqrt().unsqueeze(1)
    if clamp:
        offset = torch.clamp(offset, max=clamp)
    direction = torch.zeros_like(source)
    direction[source < target] = +1.
    direction[source > target] = -1.
    return (source + direction * offset * vc) * valid


def _metrics(pred, gt, valid):
    epe = torch.sum((pred - gt) ** 2, dim=1).sqrt().view(-1)[valid.view(-1)]
    return {'epe': epe.mean().item(), '1px': (epe < 1).float().mean().item(), '3px': (epe < 3).float().mean().item(),
            '5px': (epe < 5).float().mean().item()}


def _raft_loss(preds, gt, valid, gamma=0.9, max_flow=700):
    n = len(preds)
    valid = ((valid >= 0.5) & (torch.sum(gt ** 2, dim=1).sqrt() < max_flow)).unsqueeze(1)
    if torch.isinf(gt[valid.bool()]).any():
        return None, None, None
    loss = 0.0
    for i in range(n):
        if torch.isnan(preds[i]).any() and not torch.isinf(preds[i]).any():
            return None, None, None
        loss += (gamma ** (15 / (n - 1))) ** (n - i - 1) * (preds[i] - gt).abs()[valid.bool()].mean()
    return loss, _metrics(preds[-1], gt, valid), valid


def _gwc_loss(preds, gt, valid, max_flow=MAXDISP):
    valid = ((valid >= 0.5) & (torch.sum(gt ** 2, dim=1).sqrt() < max_flow)).unsqueeze(1)
    assert not torch.isinf(gt[valid.bool()]).any()
    loss = sum(w * torch.nn.functional.smooth_l1_loss(p[valid.bool()], gt[valid.bool()], reduction='mean')
               for p, w in zip(preds, [0.5, 0.5, 0.7, 1.0]))
    return loss, _metrics(preds[-1], gt, valid), valid


def arm_a(kind, data, preds):
    disp_gt, valid_gt, disp_pl, disp_t = data
    gt_aug, vgt_aug = _filter(disp_gt, disp_t, valid_gt.unsqueeze(1), True, TAU_GT)
    gt_aug = _ensemble(gt_aug, disp_t, vgt_aug.unsqueeze(1), CLAMP, TAU_GT)
    ones = torch.ones(disp_pl.shape).to(disp_pl.device).squeeze(1)
    pl_aug, vpl_aug = _filter(disp_pl, disp_t, ones.unsqueeze(1), False, TAU_PL)
    pl_aug = _ensemble(pl_aug, disp_t, vpl_aug.unsqueeze(1), False, TAU_PL)
    fn = _raft_loss if kind == "raft" else _gwc_loss
    loss_gt, _, _ = fn(preds, gt_aug, vgt_aug)
    loss_pl, _, _ = fn(preds, pl_aug, vpl_aug)
    (loss_gt + loss_pl * 1.0).backward()


def arm_b(kind, data, preds, events=None):
    disp_gt, valid_gt, disp_pl, disp_t = data
    rec = (lambda i: events[i].record()) if events else (lambda i: None)
    rec(0)
    targets = fande_targets(disp_gt, valid_gt, disp_pl, disp_t, TAU_GT, TAU_PL, CLAMP)
    rec(1)
    name = "sequence_loss_raft" if kind == "raft" else "loss_gwcnet"
    loss_gt, _, _, loss_pl, _ = dkt_loss_pair(name, {"disp_preds": preds}, *targets, args=argparse.Namespace(maxdisp=MAXDISP))
    rec(2)
    (loss_gt + loss_pl * 1.0).backward()
    rec(3)


def compulsory_bytes(n):
    """Bytes each library call must move at least, from the shapes: F&E reads gt, valid, pl, teacher and writes two maps
    and two masks; the loss forward reads n predictions, two targets and two masks and writes two bool masks; the backward
    reads n predictions, two targets and two bool masks and writes n gradients."""
    plane = B * H * W
    return {"fande": 8 * 4 * plane, "loss_fwd": (n + 4) * 4 * plane + 2 * plane, "loss_bwd": (2 * n + 2) * 4 * plane + 2 * plane}


def make_inputs(kind, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    dev = "cuda"
    disp_t = (torch.rand(B, 1, H, W, generator=g) * 120).to(dev)
    disp_gt = disp_t + (torch.randn(B, 1, H, W, generator=g) * 3).to(dev)
    disp_pl = disp_t + (torch.randn(B, 1, H, W, generator=g)).to(dev)
    valid_gt = (torch.rand(B, H, W, generator=g) < 0.85).float().to(dev)
    n = 16 if kind == "raft" else 4
    bases = [(disp_t.repeat(1, 2, 1, 1) + (torch.randn(B, 2, H, W, generator=g) * 4).to(dev)).requires_grad_(True)
             for _ in range(n)]
    return (disp_gt, valid_gt, disp_pl, disp_t), bases


def count_syncs(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    return sum("called a synchronizing" in str(r.message) for r in rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--arms", default="a,b")
    ap.add_argument("--loss", default="raft,gwc")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dkt_loss.py measures on a HIP device; none is available")
    arms = a.arms.split(",")
    for kind in a.loss.split(","):
        data, bases = make_inputs(kind)
        n = len(bases)

        def step(arm, events=None):
            for b in bases:
                b.grad = None
            preds = [b[:, :1] for b in bases]
            if arm == "a":
                arm_a(kind, data, preds)
            else:
                arm_b(kind, data, preds, events)

        for _ in range(a.warmup):
            for arm in arms:
                step(arm)
        torch.cuda.synchronize()
        wall = {arm: [] for arm in arms}
        dev_us = {"fande": [], "loss_fwd": [], "loss_bwd": []}
        for _ in range(a.steps):
            for arm in arms:
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if arm == "b" else None
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                step(arm, ev)
                torch.cuda.synchronize()
                wall[arm].append((time.perf_counter() - t0) * 1e3)
                if ev:
                    for i, k in enumerate(("fande", "loss_fwd", "loss_bwd")):
                        dev_us[k].append(ev[i].elapsed_time(ev[i + 1]) * 1e3)
        out = {"loss": kind, "B": B, "H": H, "W": W, "n_pred": n, "steps": a.steps}
        for arm in arms:
            w = sorted(wall[arm])
            out["arm_" + arm] = {"wall_ms_median": round(w[len(w) // 2], 3), "wall_ms_min": round(w[0], 3),
                                 "syncs_per_step": count_syncs(lambda: step(arm))}
        if "b" in arms:
            cb = compulsory_bytes(n)
            lib = {}
            for k, v in dev_us.items():
                v = sorted(v)
                med = v[len(v) // 2]
                lib[k] = {"us_median": round(med, 2), "compulsory_MB": round(cb[k] / 1e6, 2),
                          "frac_of_8TBps": round(cb[k] / PEAK_BPS / (med * 1e-6), 3)}
            out["arm_b"]["library_calls"] = lib
        if "a" in arms and "b" in arms:
            out["speedup_b_over_a"] = round(out["arm_a"]["wall_ms_median"] / out["arm_b"]["wall_ms_median"], 2)
        print(json.dumps(out))


if __name__ == "__main__":
    main()
