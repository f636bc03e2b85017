#!/usr/bin/env python3
"""PCVNet's correlation block in a training step, at the block of configs/pcvnet/base.json of the reference: 256 feature
channels, corr_levels 3, n_downsample 2 (compress factor 4), gauss_num 4, sample_num 9, feature maps at quarter resolution of a
320 x 720 crop (80 x 180), and the 16 iterations of tools/ft_dkt.py's --train_iters default (the config names none).  The loop
is the one of tests/_pcv_train_ref.py (model.py:120-142 with a stand-in head: coords detached, sigma carried with its graph):

  arm a  the block restated in torch on the device (einsum, avg_pool2d, grid_sample), forward + backward under autograd;
  arm b  pcvnet_corr.CorrBlock1D: the two autograd nodes on dkt_pcv_lookup_bwd / dkt_pcv_pool_bwd.

The arms alternate in one process after warm-up.  Per arm, as median (min .. max) over the steps: device us (HIP events around
the Python calls, host time between launches included), torch.cuda.max_memory_allocated over the step's start, and the kernel
launches of one step as torch.profiler counts them.  Then dkt_pcv_lookup_bwd alone, raw C-ABI calls back to back on rotating
buffer sets (nothing is served from the Infinity Cache): all three results, the level gradients alone and gcoords + gsigma
alone, against the time its compulsory bytes (grad_out, coords, sigma and the level values read once, the level gradients read
and written once, the two small results written) would take at the copy rate measured in the same run; and torch's zero-fill
of one set of level-shaped gradients, which every lookup's backward pays before the kernel.

    python tools/bench_pcv_train.py [--steps 10] [--warmup 3] [--batch 1]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _pcv_train_ref as R  # noqa: E402
from dkt_stereo_amd import _ffi  # noqa: E402
from dkt_stereo_amd.pcvnet_corr import CorrBlock1D  # noqa: E402

DEV = "cuda:0"
C, H, W, L, S, G, DOWNSAMPLE, ITERS = 256, 80, 180, 3, 9, 4, 2, 16
FACTOR = 4
ARMS = {"a": "torch", "b": "nodes"}
BLOCK = {"a": lambda p, q: R.TorchBlock(p, q, S, L, DOWNSAMPLE),
         "b": lambda p, q: CorrBlock1D(p, q, sample_num=S, num_levels=L, downsample=DOWNSAMPLE)}


def stats(v):
    v = sorted(v)
    return "%.1f (%.1f .. %.1f)" % (v[len(v) // 2], v[0], v[-1]), v[len(v) // 2]


def measure(fn, before):
    before()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, torch.cuda.max_memory_allocated() - base


def launches(fn, before):
    """Kernel launches of one call of fn, or None where the profiler is unavailable."""
    try:
        from torch.profiler import ProfilerActivity, profile
        before()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception:           # noqa: BLE001
        return None


def timed(fn, sets, rounds=3, reps=7):
    """[us per call] of fn over the buffer sets in rotation, back to back on one stream, per repetition."""
    for t in sets:
        fn(t)
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
    return us


def training_loop(B, steps, warmup):
    g = torch.Generator(device="cpu").manual_seed(0)
    rnd = lambda *shape, scale=1.0: (torch.randn(shape, generator=g) * scale).to(DEV)  # noqa: E731
    ch = L * G * S
    f1, f2 = rnd(B, C, H, W).requires_grad_(True), rnd(B, C, H, W).requires_grad_(True)
    hs = rnd(G, ch, scale=0.3 / ch ** 0.5).requires_grad_(True)
    hm = rnd(G, ch, scale=1.0 / ch ** 0.5)
    base = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W).expand(B, G, H, W)
    coords = (base - torch.rand((B, G, H, W), generator=g) * 0.6 * W).to(DEV)
    sigma = (0.25 + 2.75 * torch.rand((B, G, H, W), generator=g)).to(DEV)
    gouts, gsig = rnd(ITERS, B, ch, H, W), rnd(ITERS, B, G, H, W)
    leaves = (f1, f2, hs)

    def clear():
        for t in leaves:
            t.grad = None

    def step(arm, iters=ITERS):
        def run():
            loss, _ = R.loop(BLOCK[arm], f1, f2, coords, sigma, hs, hm, gouts, gsig, iters)
            loss.backward()
        return run

    # the two arms compute the same thing: after one iteration to rounding.  From the second iteration on every lookup's taps
    # depend on the previous lookup through the head, a tap that lands on the other side of an integer changes the derivative
    # there by O(1), and on random maps some of the 1.5 million taps of an iteration always do: the gradients of two fp32
    # evaluations then differ in a few elements by per cent of the largest, whatever computes them -- the torch arm differs
    # from itself in float64 as much as from the nodes.  Per comparison: the largest difference relative to the largest
    # element, and the share of elements that differ by more than 1e-4 of it.
    def differ(xs, ys):
        d = [((x.double() - y.double()).abs() / y.double().abs().max()) for x, y in zip(xs, ys)]
        return [(float(v.max()), float((v > 1e-4).double().mean())) for v in d]

    agree = {}
    for iters in (1, 3, ITERS):
        grads = {}
        for arm in ARMS:
            clear()
            step(arm, iters)()
            grads[arm] = [t.grad.clone() for t in leaves]
        d = [t.detach().double().requires_grad_(t.requires_grad) for t in (f1, f2, coords, sigma, hs, hm, gouts, gsig)]
        R.loop(BLOCK["a"], *d, iters)[0].backward()
        truth = [d[0].grad, d[1].grad, d[4].grad]
        fmt = lambda rows: ", ".join("%.2e (%.2e of the elements)" % r for r in rows)  # noqa: E731
        agree[iters] = {"nodes_vs_torch": differ(grads["b"], grads["a"]), "torch_vs_fp64": differ(grads["a"], truth),
                        "nodes_vs_fp64": differ(grads["b"], truth)}
        print("gradients (fmap1, fmap2, sigma head) after %d iterations:" % iters)
        for k, rows in agree[iters].items():
            print("  %-15s %s" % (k.replace("_", " "), fmt(rows)))
        del d, truth
    counts = {arm: launches(step(arm), clear) for arm in ARMS}
    rows = {arm: ([], []) for arm in ARMS}
    for i in range(warmup + steps):
        for arm in ARMS:
            us, peak = measure(step(arm), clear)
            if i >= warmup:
                rows[arm][0].append(us)
                rows[arm][1].append(peak)
    print("maps (%d, %d, %d, %d), L = %d, factor %d, G = %d, S = %d, %d iterations, forward + backward, %d steps; "
          "median (min .. max) device us" % (B, C, H, W, L, FACTOR, G, S, ITERS, steps))
    out = {"agree_%d" % k: v for k, v in agree.items()}
    for arm, (us, peak) in rows.items():
        line, med = stats(us)
        print("  %-6s %s us | %s launches | max_memory_allocated over the start %.1f MB" % (ARMS[arm], line, counts[arm], max(peak) / 1e6))
        out[arm] = {"us": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1), "launches": counts[arm],
                    "peak_MB": round(max(peak) / 1e6, 1)}
    print("  torch / nodes: x%.2f" % (out["a"]["us"] / out["b"]["us"]))
    return out


def raw_lookup_bwd(B, nsets=10):
    g = torch.Generator(device="cpu").manual_seed(1)
    N, ch = B * H * W, L * G * S
    widths = [W // FACTOR ** i for i in range(L)]
    sets = []
    for _ in range(nsets):
        base = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W).expand(B, G, H, W)
        sets.append(dict(levels=[torch.randn((N, w), generator=g).to(DEV) for w in widths],
                         glevels=[torch.zeros((N, w), device=DEV) for w in widths],
                         coords=(base - torch.rand((B, G, H, W), generator=g) * 0.6 * W).to(DEV),
                         sigma=(0.25 + 2.75 * torch.rand((B, G, H, W), generator=g)).to(DEV),
                         gout=torch.randn((B, ch, H, W), generator=g).to(DEV),
                         gcoords=torch.empty((B, G, H, W), device=DEV), gsigma=torch.empty((B, G, H, W), device=DEV)))
    for t in sets:
        t["pyr"], t["gpyr"] = _ffi.ptr_array(t["levels"]), _ffi.ptr_array(t["glevels"])

    def entry(levels, args):
        def run(t):
            _ffi.call("dkt_pcv_lookup_bwd", t["gout"], t["pyr"], t["coords"].data_ptr(), t["sigma"].data_ptr(), t["gout"].data_ptr(),
                      t["gpyr"] if levels else None, t["gcoords"].data_ptr() if args else None,
                      t["gsigma"].data_ptr() if args else None, B, G, H, W, W, L, S, FACTOR)
        return run

    lv_bytes = 4 * N * sum(widths)
    small = 4 * B * G * H * W
    gout_bytes = 4 * B * ch * H * W
    nbytes = {"all three results": gout_bytes + 2 * small + lv_bytes + 2 * lv_bytes + 2 * small,
              "level gradients alone": gout_bytes + 2 * small + 2 * lv_bytes,
              "gcoords + gsigma alone": gout_bytes + 2 * small + lv_bytes + 2 * small}
    fns = {"all three results": entry(True, True), "level gradients alone": entry(True, False),
           "gcoords + gsigma alone": entry(False, True)}
    big = [dict(a=torch.empty(64 << 20, device=DEV), b=torch.empty(64 << 20, device=DEV)) for _ in range(3)]
    line, med = stats(timed(lambda t: t["b"].copy_(t["a"]), big, rounds=2))
    rate = 2 * big[0]["a"].numel() * 4 / (med * 1e-6)
    del big
    print("dkt_pcv_lookup_bwd alone, B = %d, %d buffer sets in rotation; median (min .. max) us per call" % (B, nsets))
    print("  copy_ of 256 MB (read + written 512 MB): %s us, %.2f TB/s" % (line, rate / 1e12))
    out = {"copy_TBps": round(rate / 1e12, 3)}
    line, fill_us = stats(timed(lambda t: [x.zero_() for x in t["glevels"]], sets))
    print("  zero_ of one set of level gradients (%.2f MB, %d launches): %s us" % (lv_bytes / 1e6, L, line))
    out["fill_us"] = round(fill_us, 2)
    for name, fn in fns.items():
        us = timed(fn, sets)
        line, med = stats(us)
        floor = nbytes[name] / rate * 1e6
        print("  %-24s %s us; %.2f MB compulsory = %.2f us at the copy rate: %.3f of the copy rate"
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
        raise SystemExit("bench_pcv_train.py measures on a HIP device; none is available")
    out = {"loop": training_loop(a.batch, a.steps, a.warmup), "lookup_bwd": raw_lookup_bwd(a.batch)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
