#!/usr/bin/env python3
"""The optimizer step of tools/ft_dkt.py:243-248 on RAFT-Stereo's parameter list (218 tensors), four ways:

  a  the reference sequence: scaler.unscale_, clip_grad_norm_, scaler.step(torch.optim.AdamW, default implementation), scaler.update
  b  the same with torch.optim.AdamW(fused=True), when the installed torch offers it on this device
  c  scaler.step(optim.AdamW(max_norm=1.0)), scaler.update                  (dkt_adamw_step, no module=)
  d  scaler.step(optim.AdamW(max_norm=1.0, module=model)), scaler.update    (... and the refresh that keeps the model warm)

One process.  Per arm a fresh model of the same seed takes two whole training iterations (forward, scaled backward, the
arm's step) at --size with the HIP training nodes on; the scaled gradients of the last backward are kept.  Then, `reps`
times after `warmup`: the gradients are put back (untimed: unscale_ rewrites them), the device is idle, and ONE step
sequence (at lr = 0: the same work, the parameters stay where they are) is timed twice over -- by the host clock up to a final synchronise (what the training loop waits for) and by device
events around it (which span the host's enqueueing where the host is the slower of the two); the next training forward is
timed by the host clock as well, since that is where a cold model pays.  Reported per arm: the medians and the spread (min .. max) of both, the device
launches of one step (kernel events of torch's profiler in an untimed pass; the native entries by _ffi.launch_log), the
synchronising calls of one step and of the NEXT training forward (torch.cuda.set_sync_debug_mode("warn")) and that forward's
cold packs (conv.pack_scale calls).  For c and d: ten back-to-back calls of dkt_adamw_step alone between device events, and the fraction of 32 B x
parameters (28 B of the update, 4 B of the gradient pass) at the device-to-device copy rate measured in this run that they reach.  One JSON line per arm, then a
table in DESIGN 3.19's format.

    python tools/bench_optim_step.py [--reps 20] [--warmup 3] [--size 64x128] [--arms a,b,c,d]
"""
import argparse
import json
import os
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dkt_stereo_amd import _ffi, conv, extractor, optim  # noqa: E402
from dkt_stereo_amd.raft_stereo import RAFTStereo, make_args  # noqa: E402
from dkt_stereo_amd.update import BasicMultiUpdateBlock  # noqa: E402

DEV = "cuda"
HYPER = dict(lr=2e-4, weight_decay=1e-5, eps=1e-8)
ITERS = 2


def copy_rate(mib=512, rounds=10):
    """Bytes moved per second (read + write) by a device-to-device copy of `mib` MiB."""
    a = torch.empty(mib << 20, device=DEV, dtype=torch.uint8)
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(rounds):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    return 2.0 * a.numel() * rounds / (e0.elapsed_time(e1) * 1e-3)


class _Syncs:
    def __enter__(self):
        torch.cuda.synchronize()
        self.cm = warnings.catch_warnings(record=True)
        self.rec = self.cm.__enter__()
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        return self

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode(0)
        self.n = sum("called a synchronizing" in str(r.message) for r in self.rec)
        return self.cm.__exit__(*exc)


def _stats(us):
    us = sorted(us)
    return dict(median=round(us[len(us) // 2], 1), min=round(us[0], 1), max=round(us[-1], 1))


def _kernels(fn):
    """Device kernel launches of one call of fn, by torch's profiler; None where it records none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception as exc:                                  # (a profiler that cannot start is not a measurement)
        print("profiler unavailable: %s" % exc, file=sys.stderr)
        return None


def arm(name, size, reps, warmup, rate):
    torch.manual_seed(0)
    model = RAFTStereo(make_args()).to(DEV)
    model.train()
    model.freeze_bn()
    params = [p for p in model.parameters() if p.requires_grad]
    nparam = sum(p.numel() for p in params)
    gen = torch.Generator().manual_seed(1)
    i1 = (64.0 + 12.0 * torch.rand((1, 3) + size, generator=gen)).to(DEV)          # (low contrast: a random-init model stays finite)
    i2 = (64.0 + 12.0 * torch.rand((1, 3) + size, generator=gen)).to(DEV)
    if name == "a":
        opt = torch.optim.AdamW(params, **HYPER)
    elif name == "b":
        opt = torch.optim.AdamW(params, fused=True, **HYPER)
    else:
        opt = optim.AdamW(params, max_norm=1.0, module=model if name == "d" else None, **HYPER)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16, growth_interval=10 ** 9)

    def forward():
        return model(i1, i2, iters=ITERS, test_mode=False)["disp_preds"]

    def backward(preds):
        opt.zero_grad(set_to_none=False)
        scaler.scale(sum(p.mean() for p in preds)).backward()

    def step():
        if name in "ab":
            scaler.unscale_(opt)
            torch.nn.utils.clip_grad_norm_(params, 1.0)
        scaler.step(opt)
        scaler.update()

    for _ in range(2):
        backward(forward())
        step()
    backward(forward())
    live = [p for p in params if p.grad is not None]
    saved = [p.grad.clone() for p in live]

    def restore():
        for p, g in zip(live, saved):
            p.grad.copy_(g)
    def set_lr(lr):
        for group in opt.param_groups:
            group["lr"] = lr
    set_lr(0.0)        # the timed steps do all their work and leave the parameters where they are: dozens of steps along one
    wall, dev, fwd = [], [], []                                # gradient would take a randomly initialised model to infinity
    for i in range(warmup + reps):
        restore()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        t2 = time.perf_counter()
        forward()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if i >= warmup:
            wall.append((t1 - t0) * 1e6)
            dev.append(e0.elapsed_time(e1) * 1e3)
            fwd.append((t3 - t2) * 1e6)
    restore()
    kernels = _kernels(step)
    restore()
    set_lr(HYPER["lr"])
    versions = [p._version for p in live]
    with _ffi.launch_log() as native:
        with _Syncs() as s_step:
            step()
    bumped = sum(p._version != v for p, v in zip(live, versions))
    inner = conv.pack_scale
    cold = [0]

    def counted(wmax):
        cold[0] += 1
        return inner(wmax)
    conv.pack_scale = counted
    try:
        with _Syncs() as s_fwd:
            forward()
    finally:
        conv.pack_scale = inner
    out = dict(arm=name, tensors=len(live), parameters=nparam, us_wall=_stats(wall), us_device=_stats(dev), kernels=kernels,
               us_next_forward=_stats(fwd), versions_bumped=bumped, native_launches=len(native), step_syncs=s_step.n, next_forward_syncs=s_fwd.n, next_forward_cold_packs=cold[0])
    if name in "cd":
        # the three launches of dkt_adamw_step alone, back to back between device events (the host enqueues ahead)
        st = [opt.state[p] for p in live]
        args = ([p for p in live], [p.grad for p in live], [s_["exp_avg"] for s_ in st], [s_["exp_avg_sq"] for s_ in st],
                opt._step_t, opt._record, opt._workspace, 0.0, (0.9, 0.999), HYPER["eps"], HYPER["weight_decay"], 1.0)
        alone = []
        for i in range(warmup + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(10):
                optim.adamw_kernel(*args)
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                alone.append(e0.elapsed_time(e1) * 1e2)
        out["us_kernels_alone"] = _stats(alone)
        out["floor_us_at_copy_rate"] = round(32.0 * nparam / rate * 1e6, 1)
        out["fraction_of_copy_rate"] = round(out["floor_us_at_copy_rate"] / out["us_kernels_alone"]["median"], 3)
        out["last_refresh"] = opt.last_refresh
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", default="64x128")
    ap.add_argument("--arms", default="a,b,c,d")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim_step.py measures on a HIP device; none is available")
    size = tuple(int(v) for v in args.size.split("x"))
    extractor.TRAIN_NORM_NODES = extractor.TRAIN_CONV_NODES = True
    BasicMultiUpdateBlock.TRAIN_NODES = True
    conv.GRAD_PREPASS = conv.GRAD_WEIGHT_HIP = True
    rate = copy_rate()
    print(json.dumps(dict(copy_rate_TBps=round(rate / 1e12, 3))), flush=True)
    rows = []
    for name in args.arms.split(","):
        try:
            rows.append(arm(name, size, args.reps, args.warmup, rate))
        except (RuntimeError, ValueError) as exc:
            if name != "b":
                raise
            print(json.dumps(dict(arm="b", unavailable=str(exc).splitlines()[0])), flush=True)
            continue
        print(json.dumps(rows[-1]), flush=True)
    print("\n| arm | us/step, host clock (min .. max) | us/step, device events (min .. max) | us, next forward (min .. max) | kernels | "
          "syncs in the step | syncs / cold packs in the next forward | dkt_adamw_step alone, us | fraction of copy rate |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        w, d = r["us_wall"], r["us_device"]
        f = r["us_next_forward"]
        print("| %s | %.0f (%.0f .. %.0f) | %.0f (%.0f .. %.0f) | %.0f (%.0f .. %.0f) | %s | %d | %d / %d | %s | %s |" % (
            r["arm"], w["median"], w["min"], w["max"], d["median"], d["min"], d["max"], f["median"], f["min"], f["max"],
            "not measured" if r["kernels"] is None else r["kernels"], r["step_syncs"], r["next_forward_syncs"],
            r["next_forward_cold_packs"], r.get("us_kernels_alone", {}).get("median", ""), r.get("fraction_of_copy_rate", "")))


if __name__ == "__main__":
    main()
