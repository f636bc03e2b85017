#!/usr/bin/env python3
"""CGI-Stereo's disparity head (CGI_Stereo.py:256-258 of the reference: an arange repeated to the cost's shape, then
regression_topk of cgi/submodule.py:220-228 with k = 2 -- a full descending sort, two gathers, a softmax, a product and a sum)
as the reference's torch chain and as the one node of this library (topk_regress.hip):

  arm a  the torch chain, the samples tensor included;
  arm b  regression_topk(cost, None, 2): dkt_topk_regress_fwd, and under autograd dkt_topk_regress_bwd.

Two shapes: CGI's inference head at 544 x 960, cost (1, 48, 136, 240), forward only under no_grad; and a training batch,
cost (8, 48, 80, 184), forward + a scalar loss + backward.  The arms alternate in one process after warm-up.  Per arm, as
median (min .. max) over the steps: device us (HIP events around the Python calls, host time between launches included),
torch.cuda.max_memory_allocated over the step's start, and the kernel launches of one step as torch.profiler counts them.  For
the node also every entry alone, raw C-ABI calls back to back on rotating buffer sets, against the time its compulsory bytes
(forward: 4 D read and 4 written per pixel; backward: 4 D written per pixel) would take at the copy rate measured in the same
run, against a 256-byte fill launched back to back (what any launch costs there) and, for the backward, against torch's
fill of a buffer of gcost's size.

    python tools/bench_topk.py [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _topk_ref as R  # noqa: E402
from dkt_stereo_amd import _ffi  # noqa: E402
from dkt_stereo_amd.topk import regression_topk  # noqa: E402

DEV = "cuda:0"
INFER = (1, 48, 136, 240)
TRAIN = (8, 48, 80, 184)
K = 2
ARMS = {"a": "torch chain", "b": "node"}
HEAD = {"a": lambda cost: R.torch_chain_graph(cost, R.arange_samples(cost), K), "b": lambda cost: regression_topk(cost, None, K)}


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


def launches(fn, before=lambda: None):
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


def report(title, rows, counts):
    print(title)
    out = {}
    for arm, (us, peak) in rows.items():
        line, med = stats(us)
        print("  %-12s %s us | %s launches | max_memory_allocated over the start %.2f MB" % (ARMS[arm], line, counts[arm], max(peak) / 1e6))
        out[arm] = {"us": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2), "launches": counts[arm],
                    "peak_MB": round(max(peak) / 1e6, 3)}
    print("  %s / %s: x%.2f" % (ARMS["a"], ARMS["b"], out["a"]["us"] / out["b"]["us"]))
    return out


def timed(fn, sets, rounds=6, reps=7):
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
    of 256 MB buffers in rotation: nothing is served from the Infinity Cache), and against one launch of an empty fill."""
    lib = _ffi.lib()
    B, D, h, w = shape
    g = torch.Generator(device="cpu").manual_seed(1)
    sets = []
    for _ in range(nsets):
        cost = (torch.randn(shape, generator=g) * 3).to(DEV)
        sets.append(dict(cost=cost, out=torch.empty((B, 1, h, w), device=DEV), idx=torch.empty((B, K, h, w), device=DEV, dtype=torch.uint8),
                         gout=torch.randn((B, 1, h, w), generator=g).to(DEV), gcost=torch.empty_like(cost)))
    dev, st = _ffi.device_of(sets[0]["cost"]), _ffi.stream_of(sets[0]["cost"])
    p = lambda t: t.data_ptr()  # noqa: E731
    fwd = lambda t: lib.dkt_topk_regress_fwd(p(t["cost"]), D * h * w, None, 0, p(t["out"]), p(t["idx"]), B, D, h, w, K, dev, st)  # noqa: E731
    bwd = lambda t: lib.dkt_topk_regress_bwd(p(t["gout"]), h * w, p(t["cost"]), D * h * w, None, 0, p(t["idx"]), p(t["gcost"]), None,  # noqa: E731
                                             B, D, h, w, K, dev, st)
    entries = {"dkt_topk_regress_fwd": fwd}
    nbytes = {"dkt_topk_regress_fwd": 4 * B * h * w * (D + 1)}
    if backward:
        entries["dkt_topk_regress_bwd"] = bwd
        nbytes["dkt_topk_regress_bwd"] = 4 * B * h * w * D
    for name, fn in entries.items():
        _ffi.check(fn(sets[0]), name)
    big = [dict(a=torch.empty(64 << 20, device=DEV), b=torch.empty(64 << 20, device=DEV)) for _ in range(3)]
    line, med = stats(timed(lambda t: t["b"].copy_(t["a"]), big, rounds=2))
    rate = 2 * big[0]["a"].numel() * 4 / (med * 1e-6)
    print("  copy_ of 256 MB (read + written 512 MB): %s us, %.2f TB/s" % (line, rate / 1e12))
    tiny = [dict(a=torch.empty(64, device=DEV)) for _ in range(4)]
    line, floor_us = stats(timed(lambda t: t["a"].zero_(), tiny, rounds=50))
    print("  zero_ of 256 bytes, back to back: %s us per launch" % line)
    out = {"copy_TBps": round(rate / 1e12, 3), "launch_us": round(floor_us, 2)}
    if backward:                                            # what writing gcost's bytes alone takes, as torch's fill
        line, fill_us = stats(timed(lambda t: t["gcost"].zero_(), sets))
        print("  zero_ of one gcost (%.2f MB), in rotation: %s us" % (nbytes["dkt_topk_regress_bwd"] / 1e6, line))
        out["fill_us"] = round(fill_us, 2)
    for name, fn in entries.items():
        us = timed(fn, sets)
        line, med = stats(us)
        floor = nbytes[name] / rate * 1e6
        print("  %-22s %s us; %.2f MB compulsory = %.2f us at the copy rate: %.3f of the copy rate; x%.2f one empty launch"
              % (name, line, nbytes[name] / 1e6, floor, floor / med, med / floor_us))
        out[name] = {"us_per_call": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
                     "compulsory_MB": round(nbytes[name] / 1e6, 2), "of_copy_rate": round(floor / med, 4)}
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
    counts = {arm: launches(infer(arm)) for arm in ARMS}
    rows = alternate({arm: infer(arm) for arm in ARMS}, steps, warmup)
    out["infer"] = report("inference head, cost %s, k = %d, forward only, %d steps; median (min .. max) device us" % (INFER, K, steps), rows, counts)
    out["infer_raw"] = raw_calls(INFER, 48, False)

    leaf = (torch.randn(TRAIN, generator=g) * 3).to(DEV).requires_grad_(True)
    weight = torch.randn((TRAIN[0], 1) + TRAIN[2:], generator=g).to(DEV)

    def clear():
        leaf.grad = None

    def train(arm):
        def run():
            (HEAD[arm](leaf) * weight).sum().backward()                         # a scalar loss with a dense gradient
        return run
    counts = {arm: launches(train(arm), clear) for arm in ARMS}
    rows = alternate({arm: train(arm) for arm in ARMS}, steps, warmup, clear)
    out["train"] = report("training head, cost %s, k = %d, forward + loss + backward, %d steps; median (min .. max) device us"
                          % (TRAIN, K, steps), rows, counts)
    out["train_raw"] = raw_calls(TRAIN, 12, True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_topk.py measures on a HIP device; none is available")
    print(json.dumps(heads(a.steps, a.warmup)))


if __name__ == "__main__":
    main()
