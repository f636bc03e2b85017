#!/usr/bin/env python3
"""The 16 context up-samplings of one IGEV-Stereo student step (IGEVStereo.upsample_disp, igev_stereo.py:140-148 of the
reference, once per refinement iteration with test_mode=False) at the recipe shape (B = 2, 480 x 896, quarter-resolution
disparity, nine logit planes at full resolution), forward and backward, with a scalar loss on the 16 predictions:

  arm a  the reference's torch expression sequence: F.softmax, disp * 4., unfold, nearest interpolate, mul, sum;
  arm b  submodule.context_upsample(disp * 4., F.softmax(logits, 1)): the weights-form node (dkt_context_upsample /
         dkt_context_upsample_bwd) behind torch's softmax;
  arm c  upsample.context_upsample_logits(disp, logits, 4.0): dkt_context_upsample_logits_fwd / _bwd.

The arms alternate in one process after warm-up.  Per arm, as median (min .. max) over the steps: device us of the forward
and of the backward of the 16 up-samplings (HIP events around the Python calls of a step, host time between launches
included), wall ms of the step, and torch.cuda.max_memory_allocated over a step.  Then every entry alone: raw C-ABI calls
back to back on the 16 buffer sets in rotation (1 GB: nothing is served from the Infinity Cache), against the time its
compulsory bytes would take at the copy rate measured in the same run (a device-to-device copy_ of the same nine-plane
tensors in the same rotation, read + written bytes over its time).  Launch counts come from separate
`rocprofv3 --kernel-trace --stats` runs of `--arms a`, `--arms b`, `--arms c` with `--steps 1 --warmup 0 --no-raw`.

    python tools/bench_context_upsample_train.py [--steps 20] [--warmup 5] [--arms a,b,c] [--no-raw]
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
from dkt_stereo_amd.submodule import context_upsample  # noqa: E402
from dkt_stereo_amd.upsample import context_upsample_logits  # noqa: E402

B, H, W, ITERS, SCALE = 2, 480 // 4, 896 // 4, 16, 4.0
ARMS = {"a": "torch sequence", "b": "node (a) behind torch's softmax", "c": "node (b), logits in"}


def torch_sequence(disp, logits):
    """igev_stereo.py:145-146 and submodule.py:242-254 of the reference."""
    p = F.softmax(logits, 1)
    d = disp * SCALE
    b, c, h, w = d.shape
    u = F.unfold(d.reshape(b, c, h, w), 3, 1, 1).reshape(b, -1, h, w)
    u = F.interpolate(u, (h * 4, w * 4), mode="nearest").reshape(b, 9, h * 4, w * 4)
    return (u * p).sum(1)


def compulsory_bytes():
    """Bytes each entry must move at least, from the shapes."""
    nine, out, disp = B * 9 * 16 * H * W * 4, B * 16 * H * W * 4, B * H * W * 4
    fwd, bwd = nine + disp + out, 2 * nine + out + 2 * disp
    return {"dkt_context_upsample": fwd, "dkt_context_upsample_bwd": bwd, "dkt_context_upsample_logits_fwd": fwd,
            "dkt_context_upsample_logits_bwd": bwd}


def make_inputs(seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    disps = [(torch.randn(B, 1, H, W, generator=g) * 5).cuda().requires_grad_(True) for _ in range(ITERS)]
    logits = [(torch.randn(B, 9, 4 * H, 4 * W, generator=g) * 2).cuda().requires_grad_(True) for _ in range(ITERS)]
    weights = [torch.randn(B, 4 * H, 4 * W, generator=g).cuda() for _ in range(ITERS)]
    return disps, logits, weights


def stats(v):
    v = sorted(v)
    return "%.1f (%.1f .. %.1f)" % (v[len(v) // 2], v[0], v[-1]), v[len(v) // 2]


def timed(fn, sets, rounds=6, reps=5):
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


def raw_calls(disps, logits, weights):
    """Every entry alone against its compulsory bytes at the copy rate of the same run."""
    lib, dev, st = _ffi.lib(), _ffi.device_of(disps[0]), _ffi.stream_of(disps[0])
    sets = [dict(d=d.detach(), n=n.detach(), g=g, out=torch.empty_like(g), gd=torch.empty_like(d.detach()),
                 gn=torch.empty_like(n.detach()), ws=torch.empty((B, 9, H, W), device=g.device))
            for d, n, g in zip(disps, logits, weights)]
    p = lambda t: t.data_ptr()  # noqa: E731
    plane = 16 * H * W
    entries = {
        "dkt_context_upsample": lambda t: lib.dkt_context_upsample(p(t["d"]), p(t["n"]), p(t["out"]), B, H, W, dev, st),
        "dkt_context_upsample_bwd": lambda t: lib.dkt_context_upsample_bwd(p(t["g"]), plane, p(t["d"]), p(t["n"]), p(t["gd"]),
                                                                           p(t["gn"]), p(t["ws"]), B, H, W, dev, st),
        "dkt_context_upsample_logits_fwd": lambda t: lib.dkt_context_upsample_logits_fwd(p(t["d"]), p(t["n"]), SCALE, p(t["out"]),
                                                                                         B, H, W, dev, st),
        "dkt_context_upsample_logits_bwd": lambda t: lib.dkt_context_upsample_logits_bwd(p(t["g"]), plane, p(t["d"]), p(t["n"]),
                                                                                         SCALE, p(t["gd"]), p(t["gn"]), p(t["ws"]),
                                                                                         B, H, W, dev, st),
    }
    for name, fn in entries.items():
        _ffi.check(fn(sets[0]), name)
    copy_us = timed(lambda t: t["gn"].copy_(t["n"]), sets)
    line, med = stats(copy_us)
    copy_bytes = 2 * sets[0]["n"].numel() * 4
    rate = copy_bytes / (med * 1e-6)
    print("copy_ of one nine-plane tensor (%.1f MB read + written): %s us, %.2f TB/s" % (copy_bytes / 1e6, line, rate / 1e12))
    out = {"copy_TBps": round(rate / 1e12, 3)}
    cb = compulsory_bytes()
    for name, fn in entries.items():
        line, med = stats(timed(fn, sets))
        floor = cb[name] / rate * 1e6
        print("%-34s %s us; %.2f MB compulsory = %.1f us at the copy rate: %.2f of the copy rate"
              % (name, line, cb[name] / 1e6, floor, floor / med))
        out[name] = {"us_per_call": round(med, 2), "compulsory_MB": round(cb[name] / 1e6, 2), "of_copy_rate": round(floor / med, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--arms", default="a,b,c")
    ap.add_argument("--no-raw", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_context_upsample_train.py measures on a HIP device; none is available")
    arms = a.arms.split(",")
    disps, logits, weights = make_inputs()

    def step(arm, ev=None):
        for t in disps + logits:
            t.grad = None
        rec = (lambda i: ev[i].record()) if ev else (lambda i: None)
        rec(0)
        if arm == "a":
            preds = [torch_sequence(d, n) for d, n in zip(disps, logits)]
        elif arm == "b":
            preds = [context_upsample(d * SCALE, F.softmax(n, 1)) for d, n in zip(disps, logits)]
        else:
            preds = [context_upsample_logits(d, n, SCALE) for d, n in zip(disps, logits)]
        rec(1)
        loss = sum((q * wt).sum() for q, wt in zip(preds, weights))       # a scalar loss with a dense gradient per prediction
        rec(2)
        loss.backward()
        rec(3)

    for _ in range(a.warmup):
        for arm in arms:
            step(arm)
    torch.cuda.synchronize()
    rows = {arm: {"fwd_us": [], "loss_us": [], "bwd_us": [], "wall_ms": [], "peak_MB": []} for arm in arms}
    for _ in range(a.steps):
        for arm in arms:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            for t in disps + logits:
                t.grad = None                                             # the peak counts what one step allocates, gradients included
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            step(arm, ev)
            torch.cuda.synchronize()
            r = rows[arm]
            r["wall_ms"].append((time.perf_counter() - t0) * 1e3)
            r["peak_MB"].append((torch.cuda.max_memory_allocated() - base) / 1e6)
            for i, k in enumerate(("fwd_us", "loss_us", "bwd_us")):
                r[k].append(ev[i].elapsed_time(ev[i + 1]) * 1e3)
    out = {"B": B, "H": 4 * H, "W": 4 * W, "n_pred": ITERS, "steps": a.steps, "arms": {}}
    print("%d up-samplings forward + backward, B = %d, %d x %d, %d steps; median (min .. max)" % (ITERS, B, 4 * H, 4 * W, a.steps))
    for arm in arms:
        r = rows[arm]
        lines = {k: stats(v) for k, v in r.items()}
        print("arm %s  %-32s fwd %s us | loss %s us | bwd %s us | step %s ms wall | max_memory_allocated over the step's start %s MB"
              % (arm, ARMS[arm], lines["fwd_us"][0], lines["loss_us"][0], lines["bwd_us"][0], lines["wall_ms"][0], lines["peak_MB"][0]))
        out["arms"][arm] = {k: round(v[1], 2) for k, v in lines.items()}
    if not a.no_raw:
        out["raw_calls"] = raw_calls(disps, logits, weights)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
