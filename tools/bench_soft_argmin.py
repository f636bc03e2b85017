#!/usr/bin/env python3
"""GwcNet's disparity head (gwc_main.py:246-276 of the reference: F.interpolate x4 trilinear, F.softmax over the 192 planes,
disparity_regression, negated) as the reference's torch chain and as the one node of this library (soft_argmin.hip):

  arm a  the torch chain;
  arm b  soft_argmin(cost, 4, -1.0): dkt_soft_argmin_fwd, and under autograd dkt_soft_argmin_bwd.

Two shapes: the inference head of BASELINE config 5 (544 x 960), cost (1, 48, 136, 240), forward only under no_grad; and the
four heads of one training step at the recipe shape (B = 2, 256 x 512), four costs (2, 48, 64, 128), forward + a scalar loss
+ backward.  The arms alternate in one process after warm-up.  Per arm, as median (min .. max) over the steps: device us
(HIP events around the Python calls, host time between launches included) and torch.cuda.max_memory_allocated over the
step's start.  For the node also every entry alone, raw C-ABI calls back to back on rotating buffer sets, against the time
its compulsory bytes (cost in, map out; gout and cost in, gcost out) would take at the copy rate measured in the same run.
Then GwcNet whole: inference at 544 x 960 and a training step at B = 2, 256 x 512, with gwcnet.SOFT_ARGMIN_HIP on and off,
alternating.

    python tools/bench_soft_argmin.py [--steps 20] [--warmup 5] [--no-model]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _cases  # noqa: E402
import _synth  # noqa: E402
from dkt_stereo_amd import _ffi, gwcnet  # noqa: E402
from dkt_stereo_amd.soft_argmin import soft_argmin  # noqa: E402

DEV = "cuda:0"
INFER = (1, 48, 136, 240)
TRAIN = (2, 48, 64, 128)
HEADS = 4
ARMS = {"a": "torch chain", "b": "node"}


def torch_chain(cost):
    """gwc_main.py:250-268 on a (B, 48, h, w) cost."""
    up = F.interpolate(cost[:, None], scale_factor=4, mode="trilinear", align_corners=False)
    pred = F.softmax(torch.squeeze(up, 1), dim=1)
    return -gwcnet.disparity_regression(pred, 192).unsqueeze(1)


HEAD = {"a": torch_chain, "b": lambda cost: soft_argmin(cost, 4, -1.0)}


def stats(v):
    v = sorted(v)
    return "%.1f (%.1f .. %.1f)" % (v[len(v) // 2], v[0], v[-1]), v[len(v) // 2]


def measure(fn, before=lambda: None):
    """(device us, bytes of max_memory_allocated over the start) of one call of fn."""
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


def alternate(fns, steps, warmup, before=lambda: None):
    """{arm: ([us], [bytes])}: the arms take turns, `warmup` unrecorded rounds first."""
    rows = {arm: ([], []) for arm in fns}
    for i in range(warmup + steps):
        for arm, fn in fns.items():
            us, peak = measure(fn, before)
            if i >= warmup:
                rows[arm][0].append(us)
                rows[arm][1].append(peak)
    return rows


def report(title, rows, names=ARMS, unit="us", div=1.0):
    print(title)
    out = {}
    for arm, (us, peak) in rows.items():
        line, med = stats([u / div for u in us])
        print("  %-12s %s %s | max_memory_allocated over the start %.1f MB" % (names[arm], line, unit, max(peak) / 1e6))
        out[arm] = {unit: round(med, 2), "peak_MB": round(max(peak) / 1e6, 2)}
    ks = list(rows)
    if len(ks) == 2:
        print("  %s / %s: x%.2f" % (names[ks[0]], names[ks[1]], out[ks[0]][unit] / out[ks[1]][unit]))
    return out


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


def raw_calls(shape, nsets, backward):
    """Every entry alone at `shape` against its compulsory bytes at the copy rate of the same run (a device-to-device copy_
    of 256 MB buffers in rotation: nothing is served from the Infinity Cache)."""
    lib = _ffi.lib()
    B, Dc, h, w = shape
    g = torch.Generator(device="cpu").manual_seed(1)
    sets = []
    for _ in range(nsets):
        cost = (torch.randn(shape, generator=g) * 3).to(DEV)
        sets.append(dict(cost=cost, out=torch.empty((B, 1, 4 * h, 4 * w), device=DEV), gout=torch.randn((B, 1, 4 * h, 4 * w), generator=g).to(DEV),
                         gcost=torch.empty_like(cost)))
    ws = torch.empty(lib.dkt_soft_argmin_bwd_workspace(B, Dc, h, w, 4) // 4, device=DEV) if backward else None
    dev, st = _ffi.device_of(sets[0]["cost"]), _ffi.stream_of(sets[0]["cost"])
    p = lambda t: t.data_ptr()  # noqa: E731
    entries = {"dkt_soft_argmin_fwd": lambda t: lib.dkt_soft_argmin_fwd(p(t["cost"]), Dc * h * w, -1.0, p(t["out"]), B, Dc, h, w, 4, dev, st)}
    nbytes = {"dkt_soft_argmin_fwd": 4 * (B * Dc * h * w + B * 16 * h * w)}
    if backward:
        entries["dkt_soft_argmin_bwd"] = lambda t: lib.dkt_soft_argmin_bwd(p(t["gout"]), 16 * h * w, p(t["cost"]), Dc * h * w, -1.0,
                                                                          p(t["gcost"]), p(ws), B, Dc, h, w, 4, dev, st)
        nbytes["dkt_soft_argmin_bwd"] = 4 * (2 * B * Dc * h * w + B * 16 * h * w)
    for name, fn in entries.items():
        _ffi.check(fn(sets[0]), name)
    big = [dict(a=torch.empty(64 << 20, device=DEV), b=torch.empty(64 << 20, device=DEV)) for _ in range(3)]
    line, med = stats(timed(lambda t: t["b"].copy_(t["a"]), big, rounds=2))
    rate = 2 * big[0]["a"].numel() * 4 / (med * 1e-6)
    print("  copy_ of 256 MB (read + written 512 MB): %s us, %.2f TB/s" % (line, rate / 1e12))
    out = {"copy_TBps": round(rate / 1e12, 3)}
    for name, fn in entries.items():
        line, med = stats(timed(fn, sets))
        floor = nbytes[name] / rate * 1e6
        print("  %-20s %s us; %.2f MB compulsory = %.2f us at the copy rate: %.3f of the copy rate"
              % (name, line, nbytes[name] / 1e6, floor, floor / med))
        out[name] = {"us_per_call": round(med, 2), "compulsory_MB": round(nbytes[name] / 1e6, 2), "of_copy_rate": round(floor / med, 4)}
    return out


def heads(steps, warmup):
    out = {}
    g = torch.Generator(device="cpu").manual_seed(0)
    cost = (torch.randn(INFER, generator=g) * 3).to(DEV)

    def infer(arm):
        def run():
            with torch.no_grad():
                HEAD[arm](cost)
        return run
    rows = alternate({arm: infer(arm) for arm in ARMS}, steps, warmup)
    out["infer"] = report("inference head, cost %s, forward only, %d steps; median (min .. max) device us" % (INFER, steps), rows)
    out["infer_raw"] = raw_calls(INFER, 24, False)

    costs = [(torch.randn(TRAIN, generator=g) * 3).to(DEV).requires_grad_(True) for _ in range(HEADS)]
    weights = [torch.randn((TRAIN[0], 1, 4 * TRAIN[2], 4 * TRAIN[3]), generator=g).to(DEV) for _ in range(HEADS)]

    def clear():
        for c in costs:
            c.grad = None

    def train(arm):
        def run():
            preds = [HEAD[arm](c) for c in costs]
            sum((q * wt).sum() for q, wt in zip(preds, weights)).backward()    # a scalar loss with a dense gradient per head
        return run
    rows = alternate({arm: train(arm) for arm in ARMS}, steps, warmup, clear)
    out["train"] = report("the %d heads of a training step, costs %s, forward + loss + backward, %d steps; median (min .. max) device us"
                          % (HEADS, TRAIN, steps), rows)
    out["train_raw"] = raw_calls(TRAIN, 40, True)
    return out


def whole_model(steps, warmup):
    """GwcNet's inference at 544 x 960 and a training step at B = 2, 256 x 512 with the handle on and off."""
    names = {"on": "handle on", "off": "handle off"}
    model = gwcnet.GWCNet(gwcnet.make_args())
    model.load_state_dict(_synth.torch_state_dict(_synth.shapes_of(model), _cases.GWCNET_WEIGHT_SEED), strict=True)
    model.to(DEV)

    def with_handle(flag, fn):
        def run():
            was = gwcnet.SOFT_ARGMIN_HIP
            gwcnet.SOFT_ARGMIN_HIP = flag
            try:
                fn()
            finally:
                gwcnet.SOFT_ARGMIN_HIP = was
        return run

    out = {}
    model.eval()
    i1, i2 = (torch.from_numpy(t).to(DEV) for t in _synth.image_pair(1, 1, 544, 960, 16))
    rows = alternate({k: with_handle(k == "on", lambda: model(i1, i2, test_mode=True)) for k in names}, steps, warmup)
    out["model_infer"] = report("GwcNet inference, 1 x 3 x 544 x 960, %d steps; median (min .. max) device ms" % steps, rows, names, "ms", 1e3)
    model.train()
    i1, i2 = (torch.from_numpy(t).to(DEV) for t in _synth.image_pair(1, 2, 256, 512, 16))
    gt = -torch.rand(2, 1, 256, 512, device=DEV) * 40

    def step():
        model.zero_grad(set_to_none=True)
        preds = model(i1, i2)["disp_preds"]
        sum(w * F.smooth_l1_loss(p, gt) for p, w in zip(preds, (0.5, 0.5, 0.7, 1.0))).backward()
    rows = alternate({k: with_handle(k == "on", step) for k in names}, steps, warmup, lambda: model.zero_grad(set_to_none=True))
    out["model_train"] = report("GwcNet training step (forward + loss + backward), B = 2, 256 x 512, %d steps; median (min .. max) device ms" % steps,
                                rows, names, "ms", 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_soft_argmin.py measures on a HIP device; none is available")
    out = heads(a.steps, a.warmup)
    if not a.no_model:
        out.update(whole_model(max(a.steps // 2, 3), max(a.warmup // 2, 2)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
