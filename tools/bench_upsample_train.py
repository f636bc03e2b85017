#!/usr/bin/env python3
"""The 16 convex up-samplings of one RAFT student step (RAFTStereo._forward_train, raft_stereo.py:168 of the reference) at
the recipe shape of run_scripts/raft-stereo/ft_booster.sh (B = 2, 480 x 896, quarter-resolution flow and mask, f = 4),
forward and backward, with a scalar loss on the 16 predictions:

  arm a  the reference's torch expression sequence as training ran it before the node: softmax, unfold, mul, sum,
         permute copy on both channels, then [:, :1];
  arm b  upsample.convex_upsample(flow, mask, 4, channels=1): dkt_convex_upsample_fwd / dkt_convex_upsample_bwd.

The arms alternate in one process after warm-up.  Per arm: wall ms for forward + backward of the 16 up-samplings (host
clock around a step that ends in a synchronise) and torch.cuda.max_memory_allocated over a step; for arm b the device
time of the 16 forward and the 16 backward calls from HIP events and the fraction of 8 TB/s their compulsory bytes
would take, once around the Python calls of a step (host time between the launches included) and once around raw C-ABI
calls issued back to back ("raw_calls": the 16 buffer sets in rotation, 1 GB, so nothing is served from the Infinity
Cache).  Launch counts come from a separate `rocprofv3 --kernel-trace --stats` run of `--arms a` / `--arms b`.

    python tools/bench_upsample_train.py [--steps 20] [--warmup 5] [--arms a,b]
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dkt_stereo_amd import _ffi  # noqa: E402
from dkt_stereo_amd.upsample import convex_upsample  # noqa: E402

PEAK_BPS = 8e12
B, H, W, FACTOR, D, ITERS = 2, 480 // 4, 896 // 4, 4, 2, 16


def torch_sequence(flow, mask, factor):
    """raft_stereo.py:70-82 of the reference."""
    N, C, h, w = flow.shape
    mask = torch.softmax(mask.view(N, 1, 9, factor, factor, h, w), dim=2)
    up = F.unfold(factor * flow, [3, 3], padding=1).view(N, C, 9, 1, 1, h, w)
    up = torch.sum(mask * up, dim=2).permute(0, 1, 4, 2, 5, 3)
    return up.reshape(N, C, factor * h, factor * w)


def compulsory_bytes():
    """Bytes one up-sampling must move at least, from the shapes: forward reads mask and flow and writes one channel;
    backward reads mask, the upstream gradient and flow and writes the mask and flow gradients."""
    mask, flow, out = B * 9 * FACTOR * FACTOR * H * W * 4, B * D * H * W * 4, B * FACTOR * H * FACTOR * W * 4
    return {"fwd": mask + flow + out, "bwd": 2 * mask + out + 2 * flow}


def make_inputs(seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    flows, masks = [], []
    for _ in range(ITERS):
        fl = torch.randn(B, D, H, W, generator=g) * 5
        fl[:, 1] = 0                                             # stereo: the second channel is identically zero
        flows.append(fl.cuda().requires_grad_(True))
        masks.append((torch.randn(B, 9 * FACTOR * FACTOR, H, W, generator=g) * 2).cuda().requires_grad_(True))
    weights = [(torch.randn(B, 1, FACTOR * H, FACTOR * W, generator=g)).cuda() for _ in range(ITERS)]
    return flows, masks, weights


def raw_calls(flows, masks, weights, rounds=12, reps=5):
    """us per dkt_convex_upsample_fwd / _bwd call (the backward's two launches together), back to back on one stream."""
    lib, dev, st = _ffi.lib(), _ffi.device_of(flows[0]), _ffi.stream_of(flows[0])
    Hf, Wf = FACTOR * H, FACTOR * W
    sets = [(fl.detach(), m.detach(), g, torch.empty_like(g), torch.empty_like(fl), torch.empty_like(m),
             torch.empty((B, 1, 9, H, W), device=g.device)) for fl, m, g in zip(flows, masks, weights)]

    def fwd(t):
        return lib.dkt_convex_upsample_fwd(t[0].data_ptr(), t[1].data_ptr(), t[3].data_ptr(), B, D, 1, H, W, FACTOR, dev, st)

    def bwd(t):
        return lib.dkt_convex_upsample_bwd(t[2].data_ptr(), Hf * Wf, t[0].data_ptr(), t[1].data_ptr(), t[4].data_ptr(),
                                           t[5].data_ptr(), t[6].data_ptr(), B, D, 1, H, W, FACTOR, dev, st)

    out = {}
    cb = compulsory_bytes()
    for name, fn in (("fwd", fwd), ("bwd", bwd)):
        for t in sets:
            _ffi.check(fn(t), "dkt_convex_upsample_" + name)
        torch.cuda.synchronize()
        us = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(rounds):
                for t in sets:
                    fn(t)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / (rounds * len(sets)))
        med = sorted(us)[len(us) // 2]
        out[name] = {"us_per_call": round(med, 2), "compulsory_MB": round(cb[name] / 1e6, 2),
                     "frac_of_8TBps": round(cb[name] / PEAK_BPS / (med * 1e-6), 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--arms", default="a,b")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_upsample_train.py measures on a HIP device; none is available")
    arms = a.arms.split(",")
    flows, masks, weights = make_inputs()

    def step(arm, events=None):
        for t in flows + masks:
            t.grad = None
        rec = (lambda i: events[i].record()) if events else (lambda i: None)
        rec(0)
        if arm == "a":
            preds = [torch_sequence(fl, m, FACTOR)[:, :1] for fl, m in zip(flows, masks)]
        else:
            preds = [convex_upsample(fl, m, FACTOR, channels=1) for fl, m in zip(flows, masks)]
        rec(1)
        loss = sum((p * wt).sum() for p, wt in zip(preds, weights))     # a scalar loss with a dense gradient per prediction
        rec(2)
        loss.backward()
        rec(3)

    for _ in range(a.warmup):
        for arm in arms:
            step(arm)
    torch.cuda.synchronize()
    wall = {arm: [] for arm in arms}
    peak = {}
    dev_us = {"fwd": [], "loss": [], "bwd_with_loss_grad": []}
    for _ in range(a.steps):
        for arm in arms:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if arm == "b" else None
            for t in flows + masks:
                t.grad = None                                   # the peak counts what one step allocates, gradients included
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            step(arm, ev)
            torch.cuda.synchronize()
            wall[arm].append((time.perf_counter() - t0) * 1e3)
            peak[arm] = (torch.cuda.max_memory_allocated(), base)
            if ev:
                for i, k in enumerate(dev_us):
                    dev_us[k].append(ev[i].elapsed_time(ev[i + 1]) * 1e3)
    out = {"B": B, "H": 4 * H, "W": 4 * W, "factor": FACTOR, "n_pred": ITERS, "steps": a.steps}
    for arm in arms:
        w = sorted(wall[arm])
        out["arm_" + arm] = {"wall_ms_median": round(w[len(w) // 2], 3), "wall_ms_min": round(w[0], 3),
                             "max_memory_allocated_MB": round(peak[arm][0] / 1e6, 1),
                             "allocated_before_step_MB": round(peak[arm][1] / 1e6, 1)}
    if "b" in arms:
        cb = compulsory_bytes()
        spans = {}
        for k, v in dev_us.items():
            v = sorted(v)
            spans[k] = {"us_median_16_calls": round(v[len(v) // 2], 2)}
        for k, span in (("fwd", "fwd"), ("bwd", "bwd_with_loss_grad")):
            spans[span]["compulsory_MB_per_call"] = round(cb[k] / 1e6, 2)
            spans[span]["frac_of_8TBps"] = round(ITERS * cb[k] / PEAK_BPS / (spans[span]["us_median_16_calls"] * 1e-6), 3)
        out["arm_b"]["event_spans"] = spans
        out["arm_b"]["raw_calls"] = raw_calls(flows, masks, weights)
    if "a" in arms and "b" in arms:
        out["speedup_b_over_a"] = round(out["arm_a"]["wall_ms_median"] / out["arm_b"]["wall_ms_median"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
