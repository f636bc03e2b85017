#!/usr/bin/env python3
"""dkt_conv2d_wgrad7 (conv.conv2d_wgrad7: both launches, main kernel + finishing kernel) against the call it replaces,
torch.nn.grad.conv2d_weight fed with the same g' (the vendor weight-gradient convolution with its layout transposes), on the
7x7 layers of a training step:

  convf1  2 -> 64 at 120 x 224, 60 x 112 and 30 x 56 with B = 2 (the rows of DESIGN 3.14's table);
  fnet.conv1 / cnet.conv1  3 -> 64 at the two shapes of tools/bench_encoder_train.py: fnet batch 4 at 480 x 896 and batch 16
  at 320 x 720, cnet half those batches.

One process; per row both calls are warmed up, then timed alternately: device events around `rounds` back-to-back calls on
rotating buffer sets, `reps` times each.  Reported per row: the median us per call of both, their spread (min .. max of the
reps), the time g's compulsory bytes (4 * B * Cout * H * W, read once) take at the 6.29 TB/s measured copy rate of the part,
and the fraction of that rate each call reaches.  One JSON line per row.

    python tools/bench_wgrad7.py [--rounds 4] [--reps 7] [--sets 3] [--rows convf1,fnet,cnet]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dkt_stereo_amd import _ffi, conv  # noqa: E402

COPY_BPS = 6.29e12                        # measured device-to-device copy rate of the part
ROWS = {
    "convf1": [("convf1", 2, 2, 120, 224), ("convf1", 2, 2, 60, 112), ("convf1", 2, 2, 30, 56)],
    "fnet": [("fnet.conv1", 4, 3, 480, 896), ("fnet.conv1", 16, 3, 320, 720)],
    "cnet": [("cnet.conv1", 2, 3, 480, 896), ("cnet.conv1", 8, 3, 320, 720)],
}
COUT = 64


def _events(fn, sets, rounds):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(rounds):
        for t in sets:
            fn(t)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (rounds * len(sets))


def _stats(us):
    us = sorted(us)
    return {"us_median": round(us[len(us) // 2], 1), "us_min": round(us[0], 1), "us_max": round(us[-1], 1)}


def row(name, B, cin, H, W, rounds, reps, nsets):
    torch.manual_seed(0)
    sets = []
    for _ in range(nsets):
        x = torch.rand(B, cin, H, W, device="cuda") * 2 - 1
        gy = torch.randn(B, COUT, H, W, device="cuda") * 1e-4
        g, _, scale = conv.conv_grad_prepass(gy, torch.randn(B, COUT, H, W, device="cuda"), want_bias=False)
        sets.append({"x": x, "g": g, "scale": scale})
    shape = (COUT, cin, 7, 7)
    hip = lambda t: conv.conv2d_wgrad7(t["x"], t["g"], t["scale"])  # noqa: E731
    vendor = lambda t: torch.nn.grad.conv2d_weight(t["x"], shape, t["g"], stride=1, padding=(3, 3))  # noqa: E731
    a, b = hip(sets[0]), vendor(sets[0])
    rel = float((a.double() - b.double()).abs().max() / b.double().abs().max())
    for fn in (hip, vendor):
        for _ in range(2):
            for t in sets:
                fn(t)
    torch.cuda.synchronize()
    us = {"hip": [], "vendor": []}
    for _ in range(reps):                                      # the two calls alternate
        us["hip"].append(_events(hip, sets, rounds))
        us["vendor"].append(_events(vendor, sets, rounds))
    g_bytes = 4 * B * COUT * H * W
    floor_us = g_bytes / COPY_BPS * 1e6
    out = {"layer": name, "shape": [B, cin, H, W], "cout": COUT, "rounds": rounds, "reps": reps, "sets": nsets,
           "ws_MB": round(4 * _ffi.lib().dkt_conv2d_wgrad7_ws_floats(B, cin, COUT, H, W) / 1e6, 2),
           "g_MB": round(g_bytes / 1e6, 2), "g_floor_us": round(floor_us, 1), "hip_vs_vendor_rel": float("%.2e" % rel)}
    for k in ("hip", "vendor"):
        out[k] = _stats(us[k])
        out[k]["fraction_of_copy_rate"] = round(floor_us / out[k]["us_median"], 3)
    out["hip_wins"] = bool(out["hip"]["us_max"] < out["vendor"]["us_min"])
    out["hip_loses"] = bool(out["hip"]["us_min"] > out["vendor"]["us_max"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--rows", default="convf1,fnet,cnet")
    args = ap.parse_args()
    _ffi.lib()
    for key in args.rows.split(","):
        for name, B, cin, H, W in ROWS[key]:
            print(json.dumps(row(name, B, cin, H, W, args.rounds, args.reps, args.sets)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
