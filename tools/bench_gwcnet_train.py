#!/usr/bin/env python3
"""One GwcNet training step (forward in train() + loss_gwcnet-style loss + backward) at a 256x512 crop, B = 2, with the
cost volumes built by this library's HIP kernels (forward volumes.hip, backward volumes_bwd.hip) and by the reference's
pure-torch formula of the builders (per-disparity slices + torch.cat, gwc_main.py:310-315 / submodules.py:25-58) --
in one process, alternating, so both see the same clocks.  Also the volume stage alone (builders forward + backward).

    python tools/bench_gwcnet_train.py [--steps N] [--warmup W]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _cases  # noqa: E402
import _synth  # noqa: E402
from dkt_stereo_amd import gwcnet, submodule  # noqa: E402

DEV = "cuda:0"


def torch_gwc(a, b, D, G):
    B, C, H, W = a.shape
    vol = a.new_zeros((B, G, D, H, W))
    for i in range(min(D, W)):                   # planes d >= W stay zero (the reference's slices are empty)
        if i > 0:
            vol[:, :, i, :, i:] = (a[..., i:] * b[..., :-i]).view(B, G, C // G, H, W - i).mean(2)
        else:
            vol[:, :, i] = (a * b).view(B, G, C // G, H, W).mean(2)
    return vol.contiguous()


def torch_concat(a, b, D):
    B, C, H, W = a.shape
    vol = a.new_zeros((B, 2 * C, D, H, W))
    for i in range(min(D, W)):
        if i > 0:
            vol[:, :C, i, :, i:] = a[..., i:]
            vol[:, C:, i, :, i:] = b[..., :-i]
        else:
            vol[:, :C, i] = a
            vol[:, C:, i] = b
    return vol.contiguous()


def torch_gwc_concat(ga, gb, ca, cb, D, G):
    return torch.cat((torch_gwc(ga, gb, D, G), torch_concat(ca, cb, D)), 1)


LIB = (submodule.build_gwc_concat_volume, submodule.build_gwc_volume)
TORCH = (torch_gwc_concat, torch_gwc)


def use(builders):
    gwcnet.build_gwc_concat_volume, gwcnet.build_gwc_volume = builders


def loss_fn(preds, gt):
    return sum(w * F.smooth_l1_loss(p, gt) for p, w in zip(preds, (0.5, 0.5, 0.7, 1.0)))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    B, H, W = 2, 256, 512
    model = gwcnet.GWCNet(gwcnet.make_args())
    model.load_state_dict(_synth.torch_state_dict(_synth.shapes_of(model), _cases.GWCNET_WEIGHT_SEED), strict=True)
    model.to(DEV).train()
    i1, i2 = (torch.from_numpy(t).to(DEV) for t in _synth.image_pair(1, B, H, W, 16))
    gt = -torch.rand(B, 1, H, W, device=DEV) * 40

    def step():
        model.zero_grad(set_to_none=True)
        loss_fn(model(i1, i2)["disp_preds"], gt).backward()

    Hf, Wf = H // 4, W // 4
    fa, fb = (torch.randn(B, 320, Hf, Wf, device=DEV, requires_grad=True) for _ in range(2))
    ca, cb = (torch.randn(B, 12, Hf, Wf, device=DEV, requires_grad=True) for _ in range(2))
    gvol = torch.randn(B, 64, 48, Hf, Wf, device=DEV)

    def stage(builders):
        def run():
            for t in (fa, fb, ca, cb):
                t.grad = None
            builders[0](fa, fb, ca, cb, 48, 40).backward(gvol)
        return run

    res = {"lib": [], "torch": [], "lib_stage": [], "torch_stage": []}
    for i in range(args.warmup + args.steps):
        for name, builders in (("lib", LIB), ("torch", TORCH)):
            use(builders)
            t_step = timed(step)
            t_stage = timed(stage(builders))
            if i >= args.warmup:
                res[name].append(t_step)
                res[name + "_stage"].append(t_stage)
    use(LIB)
    med = {k: statistics.median(v) for k, v in res.items()}
    print("GwcNet training step, B=%d %dx%d (cost volume B x 64 x 48 x %d x %d), %d steps after %d warm-up, alternating"
          % (B, H, W, Hf, Wf, args.steps, args.warmup))
    print("  full step (fwd + loss + bwd)  library %8.2f ms   torch builders %8.2f ms   (x%.2f)"
          % (med["lib"], med["torch"], med["torch"] / med["lib"]))
    print("  volume stage (builders fwd + bwd) library %6.2f ms   torch builders %8.2f ms   (x%.2f)"
          % (med["lib_stage"], med["torch_stage"], med["torch_stage"] / med["lib_stage"]))
    print("  per-step ms: " + "  ".join("%s %s" % (k, ",".join("%.1f" % x for x in v)) for k, v in res.items()))


if __name__ == "__main__":
    main()
