"""The EMA teacher's step at the DKT recipe's shape (run_scripts/raft-stereo/*.sh: batch 2, 480x896, 32 iterations), both
`mixed_precision` settings, arms alternating in one process:

  (a) the reference's update loop (tools/ft_dkt.py:179-181) + the EMA teacher's forward (tools/ft_dkt.py:199): a cold start
  (b) ema.ema_update_ + the same forward: the loop stays warm
  (c) a steady warm forward alone, for scale

Per arm: ms per step (median), calibrations (trial runs and rescales), graph captures and weight repacks per step.  Then the
bandwidth of dkt_ema_update over the model's parameters against the 8 TB/s HBM roofline.

    python tools/bench_ema_teacher.py [--steps 5] [--rounds 2] [--decay 0.9999]
"""
import argparse
import gc
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _cases  # noqa: E402
import _synth  # noqa: E402
from dkt_stereo_amd import _ffi, ema, loop_c8  # noqa: E402
from dkt_stereo_amd.raft_stereo import RAFTStereo, make_args  # noqa: E402

DEV = "cuda:0"
COUNTS = dict(calibrations=0, captures=0, repacks=0)


def _count(obj, name, what):
    fn = getattr(obj, name)

    def wrapped(*a, **k):
        COUNTS[what] += 1
        return fn(*a, **k)
    setattr(obj, name, wrapped)


def _instrument():
    _count(loop_c8.C8Loop, "calibrate", "calibrations")
    _count(loop_c8.C8Loop, "rescale_from", "calibrations")
    _count(torch.cuda.CUDAGraph, "capture_end", "captures")
    L = _ffi.lib()
    for name in ("dkt_conv_c8_pack_weights", "dkt_conv2d_pack_weights", "dkt_conv2d_stem7_pack"):
        _count(L, name, "repacks")


def _model(mp, seed_shift=0.0):
    m = RAFTStereo(make_args(mixed_precision=mp))
    m.load_state_dict(_synth.torch_state_dict(_synth.shapes_of(m), _cases.E2E_WEIGHT_SEED), strict=True)
    m = m.to(DEV).eval()
    if seed_shift:
        g = torch.Generator(device="cpu").manual_seed(1)
        with torch.no_grad():
            for p in m.parameters():
                p.add_(seed_shift * torch.randn(p.shape, generator=g).to(DEV) * p.abs().mean().clamp_min(1e-3))
    for p in m.parameters():
        p.requires_grad = False
    return m


def _step(arm, teacher, student, pair, iters, decay):
    if arm == "a":
        ema.reference_update_(teacher, student, decay)
    elif arm == "b":
        ema.ema_update_(teacher, student, decay)
    with torch.no_grad():
        teacher(*pair, iters=iters, test_mode=True)


def bench(mp, args):
    B, H, W, iters = 2, 480, 896, 32
    pair = [torch.from_numpy(t).to(DEV) for t in _synth.image_pair(21, B, H, W, 12)]
    student = _model(mp, seed_shift=0.01)
    teachers = {arm: _model(mp) for arm in "abc"}
    for arm, t in teachers.items():                       # warm every arm (first capture, allocator)
        for _ in range(2):
            _step(arm, t, student, pair, iters, args.decay)
    times = {arm: [] for arm in "abc"}
    counts = {arm: dict(calibrations=0, captures=0, repacks=0) for arm in "abc"}
    for _ in range(args.rounds):
        for arm in "abc":
            for _ in range(args.steps):
                before = dict(COUNTS)
                gc.collect()                              # (arm (a) leaves a cyclic graph state per step)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _step(arm, teachers[arm], student, pair, iters, args.decay)
                torch.cuda.synchronize()
                times[arm].append((time.perf_counter() - t0) * 1e3)
                for k in COUNTS:
                    counts[arm][k] += COUNTS[k] - before[k]
    n = len(times["a"])
    label = dict(a="(a) reference update + forward", b="(b) ema_update_ + forward", c="(c) steady forward")
    print("mixed_precision=%s  B=%d %dx%d iters=%d decay=%g  (%d steps per arm, %d rounds alternating)"
          % (mp, B, H, W, iters, args.decay, args.steps, args.rounds))
    for arm in "abc":
        c = counts[arm]
        print("  %-32s %8.2f ms/step (min %.2f)  calibrations %.2f  captures %.2f  repacks %.1f  per step"
              % (label[arm], statistics.median(times[arm]), min(times[arm]), c["calibrations"] / n, c["captures"] / n,
                 c["repacks"] / n))
    return teachers["b"], student


def bench_kernel(teacher, student, reps=30):
    """Each launch timed alone after a 1 GiB read has evicted the parameters from L2 and the MALL (a read: no dirty lines
    left to write back during the timed launch)."""
    ts, ss = list(teacher.parameters()), list(student.parameters())
    n = sum(t.numel() for t in ts)
    flush = torch.ones(1 << 28, device=DEV, dtype=torch.float32)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    with torch.no_grad():
        for _ in range(3):
            ema.ema_kernel(ts, ss, 0.9999)
        for e0, e1 in ev:
            flush.sum()
            e0.record()
            ema.ema_kernel(ts, ss, 0.9999)
            e1.record()
        torch.cuda.synchronize()
    us = statistics.median(e0.elapsed_time(e1) for e0, e1 in ev) * 1e3
    gbs = 12.0 * n / (us * 1e-6) / 1e9
    print("dkt_ema_update: %d tensors, %d parameters (%.1f MB moved), median %.1f us per launch from cold caches, %.0f GB/s = "
          "%.2f of the 8 TB/s roofline" % (len(ts), n, 12.0 * n / 1e6, us, gbs, gbs / 8000.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--decay", type=float, default=0.9999)
    args = ap.parse_args()
    _instrument()
    print("device: %s" % torch.cuda.get_device_name(0))
    last = None
    for mp in (True, False):
        last = bench(mp, args)
    bench_kernel(*last)


if __name__ == "__main__":
    main()
