#!/usr/bin/env python3
"""ns_loss (meta_arch/nerf_stereo/loss.py:128-181 of the reference) at the recipe shape of tools/bench_dkt_loss.py (B = 2,
480 x 896) with 16 predictions, forward + backward:

  arm a  the fp32 torch restatement of tests/_ns_loss_ref.py (torch's own grid_sample / avg_pool2d under autograd; the
         reference tree itself is not needed);
  arm b  dkt_stereo_amd.ns_loss.ns_loss: dkt_ns_loss and, under autograd, dkt_ns_loss_bwd (ns_loss.hip).

The arms alternate in one process after warm-up.  Per arm, as median (min .. max) over the steps: device us (HIP events around
the Python calls, host time between launches included), torch.cuda.max_memory_allocated over the step's start, and the kernel
launches of one step as torch.profiler counts them.  For the node also its two entries alone, raw C-ABI calls back to back,
against the time its compulsory bytes (three images, conf, the target and n predictions in; n gradients out) would take at the
copy rate measured in the same run.

    python tools/bench_ns_loss.py [--steps 10] [--warmup 3] [--n 16]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _ns_loss_ref as R  # noqa: E402
from dkt_stereo_amd import _ffi, ns_loss as N  # noqa: E402

DEV = "cuda:0"
B, H, W = 2, 480, 896
ARMS = {"a": "torch chain", "b": "node"}


def scene(n):
    c = dict(seed=77, B=B, H=H, W=W, n=n, dlo=3.0, dhi=60.0)
    return {k: torch.from_numpy(v).to(DEV) for k, v in R.inputs(c).items()}


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


def timed(fn, rounds=4, reps=5):
    fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rounds):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / rounds)
    return us


def raw_calls(a, n):
    """dkt_ns_loss and dkt_ns_loss_bwd alone, against their compulsory bytes at the copy rate of the same run."""
    lib = _ffi.lib()
    preds = list(a["preds"][:n])
    w = R.weights(n)
    d = _ffi.NsLossDesc()
    for i, p in enumerate(preds):
        d.pred[i], d.pred_bstride[i], d.weight[i] = p.data_ptr(), p.stride(0), w[i]
    d.n = n
    for k, im in enumerate((a["im0"], a["im1"], a["im2"])):
        d.im[k], d.im_bstride[k] = im.data_ptr(), im.stride(0)
    keep = dict(valid=torch.empty((B, H, W), device=DEV, dtype=torch.bool), state=torch.empty((n, B, H, W), device=DEV, dtype=torch.uint8),
                loss=torch.empty((), device=DEV), rec=torch.empty(_ffi.NS_REC, device=DEV, dtype=torch.float64),
                ws=torch.empty(lib.dkt_ns_loss_workspace(B, H, W) // 8, device=DEV, dtype=torch.float64),
                grads=[torch.empty_like(p) for p in preds], up=torch.ones((), device=DEV))
    d.conf, d.conf_bstride, d.target, d.target_bstride = a["conf"].data_ptr(), H * W, a["target"].data_ptr(), H * W
    d.valid, d.state, d.loss, d.rec = (keep[k].data_ptr() for k in ("valid", "state", "loss", "rec"))
    d.conf_threshold, d.max_flow, d.alpha_disp, d.alpha_photo, d.B, d.H, d.W = 0.5, 512.0, 1.0, 0.1, B, H, W
    g = _ffi.NsLossGrad()
    for i, t in enumerate(keep["grads"]):
        g.grad[i] = t.data_ptr()
    g.grad_loss = keep["up"].data_ptr()
    dev, st = _ffi.device_of(preds[0]), _ffi.stream_of(preds[0])
    entries = {"dkt_ns_loss": lambda: _ffi.check(lib.dkt_ns_loss(d, keep["ws"].data_ptr(), dev, st), "dkt_ns_loss"),
               "dkt_ns_loss_bwd": lambda: _ffi.check(lib.dkt_ns_loss_bwd(d, g, dev, st), "dkt_ns_loss_bwd")}
    px = B * H * W
    nbytes = {"dkt_ns_loss": 4 * px * (9 + 2 + n), "dkt_ns_loss_bwd": 4 * px * (9 + 2 + 2 * n)}
    big = [torch.empty(64 << 20, device=DEV) for _ in range(6)]
    it = iter(range(10 ** 9))

    def copy():
        k = next(it) % 3
        big[2 * k + 1].copy_(big[2 * k])
    line, med = stats(timed(copy, rounds=6))
    rate = 2 * big[0].numel() * 4 / (med * 1e-6)
    print("  copy_ of 256 MB (read + written 512 MB): %s us, %.2f TB/s" % (line, rate / 1e12))
    out = {"copy_TBps": round(rate / 1e12, 3)}
    for name, fn in entries.items():
        line, med = stats(timed(fn))
        floor = nbytes[name] / rate * 1e6
        print("  %-16s %s us; %.1f MB compulsory = %.1f us at the copy rate: %.4f of the copy rate"
              % (name, line, nbytes[name] / 1e6, floor, floor / med))
        out[name] = {"us_per_call": round(med, 1), "compulsory_MB": round(nbytes[name] / 1e6, 1), "of_copy_rate": round(floor / med, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=16)
    o = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ns_loss.py measures on a HIP device; none is available")
    a = scene(o.n)
    preds = [p.clone().requires_grad_(True) for p in a["preds"]]
    rest = (a["target"], a["conf"], a["im0"], a["im1"], a["im2"])

    def clear():
        for p in preds:
            p.grad = None

    fns = {"a": lambda: R.ns(preds, *rest)["loss"].backward(), "b": lambda: N.ns_loss(preds, *rest)[0].backward()}
    rows = {arm: ([], []) for arm in fns}
    for i in range(o.warmup + o.steps):
        for arm, fn in fns.items():
            us, peak = measure(fn, clear)
            if i >= o.warmup:
                rows[arm][0].append(us)
                rows[arm][1].append(peak)
    print("ns_loss forward + backward, B = %d, %d x %d, %d predictions, %d steps; median (min .. max) device us" % (B, H, W, o.n, o.steps))
    out = {}
    for arm, (us, peak) in rows.items():
        line, med = stats(us)
        k = launches(fns[arm], clear)
        print("  %-12s %s us | max_memory_allocated over the start %.1f MB | kernel launches %s"
              % (ARMS[arm], line, max(peak) / 1e6, "not measured" if k is None else k))
        out[arm] = {"us": round(med, 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1), "peak_MB": round(max(peak) / 1e6, 1),
                    "launches": k}
    print("  torch chain / node: x%.1f in time, x%.1f in memory" % (out["a"]["us"] / out["b"]["us"], out["a"]["peak_MB"] / out["b"]["peak_MB"]))
    got = {}
    for arm, fn in fns.items():
        clear()
        fn()
        got[arm] = [p.grad.clone() for p in preds]
    with torch.no_grad():
        la, lb = float(R.ns(preds, *rest)["loss"]), float(N.ns_loss(preds, *rest)[0])
    # both arms against the float64 restatement on the device under the NODE's decisions (automask, branch): the arms' own
    # decisions differ at a few of the 860 160 pixels, where the loss jumps
    with torch.no_grad():
        _, _, _, am, third = N.ns_loss_decisions(preds, *rest)
    dec = [dict(automask=am[i], third=third[i]) for i in range(o.n)]
    err = {}
    for arm, dt in (("truth", torch.float64), ("a", torch.float32)):
        leaves = [p.detach().to(dt).requires_grad_(True) for p in preds]
        R.ns(leaves, *(t.to(dt) for t in rest), decisions=dec)["loss"].backward()
        if arm == "truth":
            truth = [p.grad for p in leaves]
        else:
            got["a"] = [p.grad for p in leaves]
    for arm in ARMS:
        err[arm] = max(float((g.double() - t).abs().max() / t.abs().max()) for g, t in zip(got[arm], truth))
    print("  loss: torch chain %.7g, node %.7g; gradients against float64 under the node's decisions, largest |error| / max|gradient| "
          "over the predictions: torch chain (fp32, same decisions) %.2e, node %.2e" % (la, lb, err["a"], err["b"]))
    out["loss"] = {"a": la, "b": lb, "grad_err_vs_fp64": err}
    out["raw"] = raw_calls(a, o.n)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
