#!/usr/bin/env python3
"""PCVNet's mixture-parameter update and its four up-samplings in a training step, at the block of configs/pcvnet/base.json of
the reference: gauss_num 4, n_downsample 2, quarter resolution of a 320 x 720 crop (80 x 180 = 14 400 pixels), and the 16
iterations of tools/ft_dkt.py's --train_iters default.  One step is 16 calls forward and one backward through all of them.

  update    arm a  update.py:92-107 + model.py:154 restated in torch on the device, fp32, under autograd;
            arm b  pcvnet_update.parameters_update: one node on dkt_pcv_update_fwd / dkt_pcv_update_bwd.
  upsample  arm a  the four convex_upsample calls of model.py:165-174 on upsample.convex_upsample with the repeated mask;
            arm b  pcvnet_update.mixture_upsample: two calls, no repeated mask.

The arms alternate in one process after warm-up.  Per arm, as median (min .. max) over the steps: device us (HIP events around
the Python calls, host time between launches included), torch.cuda.max_memory_allocated over the step's start, and the kernel
launches of one step as torch.profiler counts them.  The criterion: the node's median below the torch arm's minimum of the
same process.  Then the two entries alone, raw C-ABI calls back to back on rotating buffer sets, against the time their
compulsory bytes (forward: four planes read, three and disp written, one byte per element; backward: four planes and the bytes
read, the four upstream gradients read, four results written) would take at the copy rate measured in the same run.

    python tools/bench_pcv_update.py [--steps 10] [--warmup 3] [--batch 1]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_pcv_train import launches, measure, stats, timed  # noqa: E402
from dkt_stereo_amd import _ffi  # noqa: E402
from dkt_stereo_amd.pcvnet_update import mixture_upsample, parameters_update, parameters_update_torch  # noqa: E402
from dkt_stereo_amd.upsample import convex_upsample  # noqa: E402

DEV = "cuda:0"
G, H, W, FACTOR, ITERS = 4, 80, 180, 4, 16
CONSTS = (0.5, 1e-3, 1.0, 1.0, 1.0)


def draw(B, g):
    rnd = lambda *shape, scale=1.0: (torch.randn(shape, generator=g) * scale).to(DEV)  # noqa: E731
    w = 0.05 + torch.rand((B, G, H, W), generator=g)
    return dict(delta=rnd(B, G, H, W), mu=(48.0 * torch.rand((B, G, H, W), generator=g)).to(DEV),
                sigma=(0.5 + 7.5 * torch.rand((B, G, H, W), generator=g)).to(DEV), w=(w / w.sum(1, keepdim=True)).to(DEV))


def alternate(arms, clear, steps, warmup, title):
    counts = {name: launches(fn, clear) for name, fn in arms.items()}
    rows = {name: ([], []) for name in arms}
    for i in range(warmup + steps):
        for name, fn in arms.items():
            us, peak = measure(fn, clear)
            if i >= warmup:
                rows[name][0].append(us)
                rows[name][1].append(peak)
    print(title)
    out = {}
    for name, (us, peak) in rows.items():
        line, med = stats(us)
        print("  %-6s %s us | %s launches | max_memory_allocated over the start %.1f MB" % (name, line, counts[name], max(peak) / 1e6))
        out[name] = {"us": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1), "launches": counts[name],
                     "peak_MB": round(max(peak) / 1e6, 1)}
    out["node_median_below_torch_min"] = out["node"]["us"] < out["torch"]["us_min"]
    print("  torch / node: x%.2f; node's median below torch's minimum: %s"
          % (out["torch"]["us"] / out["node"]["us"], out["node_median_below_torch_min"]))
    return out


def update_loop(B, steps, warmup):
    g = torch.Generator(device="cpu").manual_seed(0)
    t = draw(B, g)
    leaves = [t[k].requires_grad_(True) for k in ("delta", "mu", "sigma", "w")]
    gs = [torch.randn((ITERS, B, c, H, W), generator=g).to(DEV) for c in (G, G, G, 1)]

    def clear():
        for x in leaves:
            x.grad = None

    def step(fn):
        def run():
            loss = 0.0
            for i in range(ITERS):
                outs = fn(*leaves)
                loss = loss + sum((o * gi[i]).sum() for o, gi in zip(outs, gs))
            loss.backward()
        return run

    # the two arms compute the same thing: the largest difference of each gradient relative to its largest element
    grads = {}
    for name, fn in (("torch", parameters_update_torch), ("node", parameters_update)):
        clear()
        step(fn)()
        grads[name] = [x.grad.clone() for x in leaves]
    agree = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(grads["node"], grads["torch"])]
    print("gradients (delta, mu, sigma, w), node against torch, largest difference / largest element: "
          + ", ".join("%.2e" % v for v in agree))
    out = alternate({"torch": step(parameters_update_torch), "node": step(parameters_update)}, clear, steps, warmup,
                    "update: (%d, %d, %d, %d), %d calls forward + backward, %d steps; median (min .. max) device us"
                    % (B, G, H, W, ITERS, steps))
    out["agree"] = agree
    return out


def upsample_loop(B, steps, warmup):
    g = torch.Generator(device="cpu").manual_seed(2)
    t = draw(B, g)
    disp = (t["w"] * t["mu"]).sum(1, keepdim=True)
    mask = (2.0 * torch.randn((B, 9 * FACTOR ** 2, H, W), generator=g)).to(DEV)
    leaves = [x.requires_grad_(True) for x in (disp, t["mu"], t["sigma"], t["w"], mask)]
    fine = lambda n, c: torch.randn((n, c, FACTOR * H, FACTOR * W), generator=g).to(DEV)  # noqa: E731
    gs = [fine(B, 1), fine(B * G, 1), fine(B * G, 1), fine(B * G, 1)]

    def reference_form(d, m, s, w, k, f):
        rep = lambda: k.repeat(1, G, 1, 1).reshape(B * G, -1, H, W).detach()  # noqa: E731
        return (convex_upsample(d, k, f), convex_upsample(s.reshape(-1, 1, H, W), rep(), f),
                convex_upsample(m.reshape(-1, 1, H, W), rep(), f), convex_upsample(w.reshape(-1, 1, H, W) * (1.0 / f), rep(), f))

    def ours(d, m, s, w, k, f):
        du, mu, su, wu = mixture_upsample(d, m, s, w, k, f)
        return du, su, mu, wu

    def clear():
        for x in leaves:
            x.grad = None

    def step(fn):
        def run():
            loss = 0.0
            for _ in range(ITERS):
                loss = loss + sum((o * gi).sum() for o, gi in zip(fn(*leaves, FACTOR), gs))
            loss.backward()
        return run
    return alternate({"torch": step(reference_form), "node": step(ours)}, clear, steps, warmup,
                     "upsample: disp (%d, 1, %d, %d), mu / sigma / w (%d, %d, %d, %d), factor %d, %d x 4 up-samplings forward + "
                     "backward, %d steps (arm 'torch': four convex_upsample calls with the repeated mask)"
                     % (B, H, W, B, G, H, W, FACTOR, ITERS, steps))


def raw_entries(B, nsets=10):
    g = torch.Generator(device="cpu").manual_seed(1)
    sets = []
    for _ in range(nsets):
        t = draw(B, g)
        for k in ("mu_out", "w_out", "sigma_out", "gdelta", "gmu", "gsigma", "gw"):
            t[k] = torch.empty((B, G, H, W), device=DEV)
        for k in ("gmu_out", "gw_out", "gsigma_out"):
            t[k] = torch.randn((B, G, H, W), generator=g).to(DEV)
        t["disp"], t["gdisp"] = torch.empty((B, 1, H, W), device=DEV), torch.randn((B, 1, H, W), generator=g).to(DEV)
        t["code"] = torch.empty((B, G, H, W), dtype=torch.uint8, device=DEV)
        sets.append(t)
    p = lambda t, *ks: [t[k].data_ptr() for k in ks]  # noqa: E731

    def fwd(t):
        _ffi.call("dkt_pcv_update_fwd", t["delta"], *p(t, "delta", "mu", "sigma", "w", "mu_out", "w_out", "sigma_out", "disp", "code"),
                  B, G, H, W, *CONSTS)

    def bwd(t):
        _ffi.call("dkt_pcv_update_bwd", t["delta"], *p(t, "delta", "mu", "sigma", "w", "code", "gmu_out", "gw_out", "gsigma_out",
                                                      "gdisp", "gdelta", "gmu", "gsigma", "gw"), B, G, H, W, *CONSTS)
    plane, one = 4 * B * G * H * W, 4 * B * H * W
    nbytes = {"dkt_pcv_update_fwd": 7 * plane + one + plane // 4, "dkt_pcv_update_bwd": 11 * plane + one + plane // 4}
    big = [dict(a=torch.empty(64 << 20, device=DEV), b=torch.empty(64 << 20, device=DEV)) for _ in range(3)]
    line, med = stats(timed(lambda t: t["b"].copy_(t["a"]), big, rounds=2))
    rate = 2 * big[0]["a"].numel() * 4 / (med * 1e-6)
    del big
    print("the entries alone, B = %d, %d buffer sets in rotation; median (min .. max) us per call" % (B, nsets))
    print("  copy_ of 256 MB (read + written 512 MB): %s us, %.2f TB/s" % (line, rate / 1e12))
    out = {"copy_TBps": round(rate / 1e12, 3)}
    for name, fn in (("dkt_pcv_update_fwd", fwd), ("dkt_pcv_update_bwd", bwd)):
        us = timed(fn, sets)
        line, med = stats(us)
        floor = nbytes[name] / rate * 1e6
        print("  %-20s %s us; %.2f MB compulsory = %.2f us at the copy rate: %.3f of the copy rate"
              % (name, line, nbytes[name] / 1e6, floor, floor / med))
        out[name] = {"us_per_call": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
                     "compulsory_MB": round(nbytes[name] / 1e6, 2), "of_copy_rate": round(floor / med, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pcv_update.py measures on a HIP device; none is available")
    out = {"update": update_loop(a.batch, a.steps, a.warmup), "upsample": upsample_loop(a.batch, a.steps, a.warmup),
           "entries": raw_entries(a.batch)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
