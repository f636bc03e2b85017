#!/usr/bin/env python3
"""The update operator alone on the training path (BasicMultiUpdateBlock under autograd, tools/ft_dkt.py:223-242 of the
reference) at the recipe shape of run_scripts/raft-stereo/ft_booster.sh: B = 2, 480 x 896 images, i.e. a 120 x 224 finest
level, 3 GRU layers, 16 calls chained through the hidden states, forward and backward with a scalar loss on the 16 flow
updates and masks; the weights are trainable (their gradient is the vendor library's in arms a to c).

  arm a  BasicMultiUpdateBlock.TRAIN_NODES = False: gates and resamplers as torch's expression sequence (training before
         the nodes);
  arm b  TRAIN_NODES = True: gru_train.gate_zr / gate_out / pool2x / interp (dkt_gru_gate_*_train, dkt_gru_gate_*_bwd,
         dkt_pool2x_bwd, dkt_interp_bilinear_bwd), the convolutions' backward as before conv.GRAD_PREPASS;
  arm c  arm b with conv.GRAD_PREPASS = True: dkt_conv_grad_prepass + the device-scaled dkt_conv2d_f16s_desc, packed images held by their
         owners, conv.GRAD_WEIGHT_HIP = False: the weight gradient on the vendor library (on a tree without the handles arm b
         is that tree's only backward);
  arm d  arm c with conv.GRAD_WEIGHT_HIP = True: dkt_conv2d_wgrad for the 1x1 and 3x3 layers (the default).

The arms alternate in one process after warm-up.  Per arm: wall ms of a step (host clock around a step that ends in a
synchronise; median and minimum), torch.cuda.max_memory_allocated over a step, the library launches of a step's FORWARD by
entry (_ffi.launch_log is per thread; the backward runs on autograd's thread and shows in the rocprofv3 run) and the host
synchronisations torch reports for one more step (torch.cuda.set_sync_debug_mode("warn")).  "raw_calls": every new entry at the
finest level's shape issued back to back through the C ABI on one stream, buffer sets in rotation (past the 256 MiB
Infinity Cache), HIP events around the calls, median of 5: us per call and the fraction of 8 TB/s its compulsory bytes
would take.  Launch counts and kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of `--arms a` /
`--arms b`.

    python tools/bench_gru_train.py [--steps 10] [--warmup 3] [--arms a,b] [--no-raw]
    python tools/bench_gru_train.py --prepass   dkt_conv_grad_prepass alone at (2, 256, 120, 224), with and without y,
                                                against its compulsory bytes
    python tools/bench_gru_train.py --wgrad     one row per (level, layer) of the recipe block, B = 2: us of the vendor weight
                                                gradient (HIP events around the whole torch.nn.grad.conv2d_weight call, its
                                                transposes included, after a warm-up), us of dkt_conv2d_wgrad, algorithmic
                                                GFLOP and the fraction of 833 TFLOP/s the new entry reaches
    python tools/bench_gru_train.py --gx-table  relative error of the input gradient of the z|r layer (1, 256 -> 384, 16 x 24)
                                                against float64 at upstream gradients randn * 2^k, both backward paths
    python tools/bench_gru_train.py --sweep     worst error of the device's sigmoid (dkt_sigmoid) and tanhf against float64
                                                on linspace(-30, 30, 4 000 001): the E_sigma / E_t of tests/_gru_ref.py
"""
import argparse
import json
import os
import sys
import time
import warnings
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dkt_stereo_amd import _ffi, conv  # noqa: E402
from dkt_stereo_amd.update import BasicMultiUpdateBlock  # noqa: E402

PEAK_BPS = 8e12
B, H, W, CH, ITERS = 2, 480 // 4, 896 // 4, 128, 16


def make_block():
    cfg = dict(corr_levels=4, corr_radius=4, n_downsample=2, n_gru_layers=3, hidden_dims=[CH, CH, CH], slow_fast_gru=False)
    torch.manual_seed(0)
    return BasicMultiUpdateBlock(SimpleNamespace(**cfg), hidden_dims=cfg["hidden_dims"]).cuda()


def make_inputs(seed=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    net0 = [torch.tanh(r(B, CH, H >> i, W >> i)).cuda() for i in range(3)]
    # the context features as the model hands them over: three channel slices of one tensor per scale (raft_stereo.py:114)
    inp = [list((0.5 * r(B, 3 * CH, H >> i, W >> i)).cuda().split(CH, dim=1)) for i in range(3)]
    corr, flow = r(B, 36, H, W).cuda(), r(B, 2, H, W).cuda()
    wd = [r(B, 2, H, W).cuda() for _ in range(ITERS)]
    wm = [r(B, 144, H, W).cuda() for _ in range(ITERS)]
    return net0, inp, corr, flow, wd, wm


def compulsory_planes():
    """(B, Ch, HW) planes each entry must move at least (read + written), at the finest level."""
    return {"dkt_gru_gate_zr_train": 5 + 3,      # azr (2), cz, cr, h -> z, r, rh
            "dkt_gru_gate_out_train": 4 + 2,     # aq, cq, z, h -> q, h'
            "dkt_gru_gate_out_bwd": 4 + 3,       # g, z, q, h -> gaq, gz, gh
            "dkt_gru_gate_zr_bwd": 5 + 3,        # gz, grh, z, r, h -> gazr (2), gh
            "dkt_pool2x_bwd": 0.25 + 1,          # gy at half resolution -> gx
            "dkt_interp_bilinear_bwd": 1 + 0.25}  # gy at the finest level -> gx at half resolution


def raw_calls(sets=4, rounds=6, reps=5):
    lib = _ffi.lib()
    HW = H * W
    n = CH * HW
    plane = lambda k=1: torch.randn(B, k * CH, H, W, device="cuda")
    unit = lambda: torch.rand(B, CH, H, W, device="cuda")
    half = lambda: torch.randn(B, CH, H // 2, W // 2, device="cuda")
    bufs = [dict(azr=plane(2), a=plane(), b=plane(), c=plane(), h=plane(), z=unit(), r=unit(), q=unit() * 2 - 1,
                 o1=plane(), o2=plane(), o3=plane(), o4=plane(2), small=half(), small_o=half()) for _ in range(sets)]
    dev, st = _ffi.device_of(bufs[0]["a"]), _ffi.stream_of(bufs[0]["a"])
    p = lambda t: t.data_ptr()
    calls = {
        "dkt_gru_gate_zr_train": lambda t: lib.dkt_gru_gate_zr_train(p(t["azr"]), p(t["a"]), n, p(t["b"]), n, p(t["h"]), n, p(t["o1"]),
                                                                     p(t["o2"]), p(t["o3"]), n, B, CH, HW, dev, st),
        "dkt_gru_gate_out_train": lambda t: lib.dkt_gru_gate_out_train(p(t["a"]), p(t["b"]), n, p(t["z"]), p(t["h"]), n, p(t["o1"]),
                                                                       p(t["o2"]), n, B, CH, HW, dev, st),
        "dkt_gru_gate_out_bwd": lambda t: lib.dkt_gru_gate_out_bwd(p(t["a"]), n, p(t["z"]), p(t["q"]), p(t["h"]), n, p(t["o1"]),
                                                                   p(t["o2"]), p(t["o3"]), B, CH, HW, dev, st),
        "dkt_gru_gate_zr_bwd": lambda t: lib.dkt_gru_gate_zr_bwd(p(t["a"]), p(t["b"]), n, p(t["z"]), p(t["r"]), p(t["h"]), n,
                                                                 p(t["o4"]), p(t["o1"]), B, CH, HW, dev, st),
        "dkt_pool2x_bwd": lambda t: lib.dkt_pool2x_bwd(p(t["small"]), p(t["o1"]), B * CH, H, W, dev, st),
        "dkt_interp_bilinear_bwd": lambda t: lib.dkt_interp_bilinear_bwd(p(t["a"]), p(t["small_o"]), B * CH, H // 2, W // 2, H, W,
                                                                         dev, st),
    }
    out = {}
    plane_bytes = B * n * 4
    for name, fn in calls.items():
        for t in bufs:
            _ffi.check(fn(t), name)
        torch.cuda.synchronize()
        us = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(rounds):
                for t in bufs:
                    fn(t)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / (rounds * len(bufs)))
        med = sorted(us)[len(us) // 2]
        nbytes = compulsory_planes()[name] * plane_bytes
        out[name] = {"us_per_call": round(med, 2), "compulsory_MB": round(nbytes / 1e6, 2),
                     "frac_of_8TBps": round(nbytes / PEAK_BPS / (med * 1e-6), 3)}
    return out


def prepass_alone(sets=6, rounds=4, reps=5):
    """dkt_conv_grad_prepass at the z|r gradient of the recipe shape, buffer sets in rotation past the Infinity Cache."""
    lib = _ffi.lib()
    C, HW = 2 * CH, H * W
    n = C * HW
    bufs = [dict(gy=torch.randn(B, C, H, W, device="cuda"), y=torch.randn(B, C, H, W, device="cuda"),
                 gm=torch.empty(B, C, H, W, device="cuda")) for _ in range(sets)]
    gb, scale = torch.empty(C, device="cuda"), torch.empty(2, device="cuda")
    ws = torch.empty(int(lib.dkt_conv_grad_prepass_ws_floats(B, C, HW)), device="cuda")
    dev, st = _ffi.device_of(gb), _ffi.stream_of(gb)
    p = lambda t: t.data_ptr()
    out = {"shape": [B, C, H, W]}
    for name, with_y, planes in (("without_y", False, 1), ("with_y", True, 3)):
        fn = lambda t: lib.dkt_conv_grad_prepass(p(t["gy"]), n, p(t["y"]) if with_y else None, n, p(t["gm"]), p(gb), p(scale),
                                                 p(ws), B, C, HW, dev, st)
        for t in bufs:
            _ffi.check(fn(t), "dkt_conv_grad_prepass")
        torch.cuda.synchronize()
        us = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(rounds):
                for t in bufs:
                    fn(t)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / (rounds * len(bufs)))
        med = sorted(us)[len(us) // 2]
        nbytes = planes * B * n * 4
        out[name] = {"us_per_call": round(med, 2), "compulsory_MB": round(nbytes / 1e6, 2),
                     "frac_of_8TBps": round(nbytes / PEAK_BPS / (med * 1e-6), 3)}
    print(json.dumps(out))


#: (layer, Cin, Cout, K) of the recipe block's 1x1 and 3x3 layers
WGRAD_LAYERS = [("z|r", 3 * CH, 2 * CH, 3), ("q", 3 * CH, CH, 3), ("flow_head.conv1", CH, 2 * CH, 3), ("flow_head.conv2", 2 * CH, 2, 3),
                ("encoder.convc1", 36, 64, 1), ("encoder.convc2 / convf2", 64, 64, 3), ("encoder.conv", 128, 126, 3)]
PEAK_SPLIT_FLOPS = 833e12


def _event_us(fn, reps=5, rounds=8):
    """Median over `reps` of the HIP-event time of `rounds` back-to-back calls, per call."""
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rounds):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / rounds)
    return sorted(us)[len(us) // 2]


def wgrad_table():
    """One JSON line per (level, layer): the vendor call against dkt_conv2d_wgrad on the same operands."""
    lib = _ffi.lib()
    p = lambda t: t.data_ptr()
    for lvl in range(3):
        h, w = H >> lvl, W >> lvl
        for name, cin, cout, k in WGRAD_LAYERS:
            torch.manual_seed(0)
            x = torch.randn(B, cin, h, w, device="cuda")
            g = torch.randn(B, cout, h, w, device="cuda") * 2.0 ** -10
            _, _, scale = conv.conv_grad_prepass(g, None, want_bias=False)
            gw = torch.empty(cout, cin, k, k, device="cuda")
            ws = torch.empty(int(lib.dkt_conv2d_wgrad_ws_floats(B, cin, cout, h, w, k)), device="cuda")
            dev, st = _ffi.device_of(x), _ffi.stream_of(x)
            vendor = lambda: torch.nn.grad.conv2d_weight(x, (cout, cin, k, k), g, stride=1, padding=k // 2)
            ours = lambda: lib.dkt_conv2d_wgrad(p(x), cin * h * w, p(g), cout * h * w, p(scale), 1.0, p(gw), p(ws), B, cin, cout,
                                                h, w, k, dev, st)
            for _ in range(3):                                  # warm-up: the vendor's kernel search is in neither figure
                want = vendor()
                _ffi.check(ours(), "dkt_conv2d_wgrad")
            torch.cuda.synchronize()
            rel = float((gw.double() - want.double()).abs().max() / want.double().abs().max())
            v_us, o_us = _event_us(vendor), _event_us(ours)
            gflop = 2.0 * B * h * w * cin * cout * k * k / 1e9
            print(json.dumps({"level": "%dx%d" % (h, w), "layer": name, "cin": cin, "cout": cout, "k": k,
                              "vendor_us": round(v_us, 1), "wgrad_us": round(o_us, 1), "gflop": round(gflop, 3),
                              "frac_of_833TFLOPs": round(gflop * 1e9 / (o_us * 1e-6) / PEAK_SPLIT_FLOPS, 4),
                              "ws_MB": round(ws.numel() * 4 / 1e6, 1), "rel_diff_to_vendor": float("%.3g" % rel)}), flush=True)


def gx_table():
    """max|gx - exact| / max|exact| of the z|r layer's input gradient, exact = float64 on the device."""
    import torch.nn.functional as F
    torch.manual_seed(0)
    lay = torch.nn.Conv2d(3 * CH, 2 * CH, 3, padding=1).cuda()
    x0 = torch.randn(1, 3 * CH, 16, 24, device="cuda")
    gy0 = torch.randn(1, 2 * CH, 16, 24, device="cuda")
    wt = lay.weight.detach().transpose(0, 1).flip(2, 3).double()
    out = {}
    for k in (0, -10, -20, -30):
        gy = gy0 * 2.0 ** k
        exact = F.conv2d(gy.double(), wt, padding=1)
        row = {}
        for name, on in (("before", False), ("prepass", True)):
            if not hasattr(conv, "GRAD_PREPASS") and on:
                continue
            conv.GRAD_PREPASS = on
            x = x0.clone().requires_grad_(True)
            gx = torch.autograd.grad(conv.conv2d_autograd(x, lay), [x], grad_outputs=gy)[0]
            row[name] = float("%.3g" % float((gx.double() - exact).abs().max() / exact.abs().max()))
        out["k=%d" % k] = row
    conv.GRAD_PREPASS = True
    print(json.dumps(out))


def sweep():
    """Worst error of dkt_sigmoid and tanhf (through the training entries: x + 0 is exact) in ulp of the true result and
    relative to it in u = 2^-24."""
    lib = _ffi.lib()
    x = torch.linspace(-30.0, 30.0, 4000001, dtype=torch.float64).float()
    n = x.numel()
    xg = x.cuda()
    zero, one = torch.zeros_like(xg), torch.ones_like(xg)
    azr = torch.cat([xg, xg]).contiguous()
    z, r, rh, q, out = (torch.empty_like(xg) for _ in range(5))
    dev, st = _ffi.device_of(xg), _ffi.stream_of(xg)
    p = lambda t: t.data_ptr()
    _ffi.check(lib.dkt_gru_gate_zr_train(p(azr), p(zero), n, p(zero), n, p(one), n, p(z), p(r), p(rh), n, 1, 1, n, dev, st),
               "dkt_gru_gate_zr_train")
    _ffi.check(lib.dkt_gru_gate_out_train(p(xg), p(zero), n, p(one), p(one), n, p(q), p(out), n, 1, 1, n, dev, st),
               "dkt_gru_gate_out_train")
    torch.cuda.synchronize()
    assert torch.equal(z, r)
    xd = x.double()
    res = {"points": n, "range": 30.0}
    for name, got, true in (("sigmoid", z, 1.0 / (1.0 + torch.exp(-xd))), ("tanh", q, torch.tanh(xd))):
        d = (got.double().cpu() - true).abs()
        nz = true != 0
        ulp = torch.exp2(torch.floor(torch.log2(true.abs()[nz])) - 23)
        k = int((d[nz] / ulp).argmax())
        res[name] = {"worst_ulp": round(float((d[nz] / ulp).max()), 3), "at_x": float(x[nz][k]),
                     "worst_relative_u": round(float((d[nz] / (true.abs()[nz] * 2.0 ** -24)).max()), 3)}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--arms", default="a,b")
    ap.add_argument("--no-raw", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--prepass", action="store_true")
    ap.add_argument("--gx-table", action="store_true")
    ap.add_argument("--wgrad", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gru_train.py measures on a HIP device; none is available")
    if a.sweep:
        return sweep()
    if a.prepass:
        return prepass_alone()
    if a.gx_table:
        return gx_table()
    if a.wgrad:
        return wgrad_table()
    arms = a.arms.split(",")
    blk = make_block()
    net0, inp, corr, flow, wd, wm = make_inputs()
    params = list(blk.parameters())

    def step(arm):
        BasicMultiUpdateBlock.TRAIN_NODES = arm != "a"
        conv.GRAD_PREPASS = arm in ("c", "d")
        conv.GRAD_WEIGHT_HIP = arm == "d"
        for t in params:
            t.grad = None
        net = [t.clone().requires_grad_(True) for t in net0]
        loss = 0.0
        for it in range(ITERS):
            net, mask, delta = blk(net, inp, corr, flow)
            loss = loss + (delta * wd[it]).sum() + (mask * wm[it]).sum()
        loss.backward()

    for _ in range(a.warmup):
        for arm in arms:
            step(arm)
    torch.cuda.synchronize()
    wall = {arm: [] for arm in arms}
    peak = {}
    for _ in range(a.steps):
        for arm in arms:
            for t in params:
                t.grad = None                                   # the peak counts what one step allocates, gradients included
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            step(arm)
            torch.cuda.synchronize()
            wall[arm].append((time.perf_counter() - t0) * 1e3)
            peak[arm] = (torch.cuda.max_memory_allocated(), base)
    launches, syncs = {}, {}
    for arm in arms:
        with _ffi.launch_log() as names:
            step(arm)
        launches[arm] = {n: names.count(n) for n in sorted(set(names))}
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            step(arm)
            torch.cuda.set_sync_debug_mode("default")
        syncs[arm] = sum("synchroniz" in str(w.message).lower() for w in seen)
        torch.cuda.synchronize()
    BasicMultiUpdateBlock.TRAIN_NODES = True
    conv.GRAD_PREPASS = True
    conv.GRAD_WEIGHT_HIP = True
    out = {"B": B, "H": 4 * H, "W": 4 * W, "n_gru_layers": 3, "calls": ITERS, "steps": a.steps}
    for arm in arms:
        w = sorted(wall[arm])
        out["arm_" + arm] = {"wall_ms_median": round(w[len(w) // 2], 3), "wall_ms_min": round(w[0], 3),
                             "max_memory_allocated_MB": round(peak[arm][0] / 1e6, 1),
                             "allocated_before_step_MB": round(peak[arm][1] / 1e6, 1),
                             "host_syncs_per_step": syncs[arm], "library_launches_per_step": sum(launches[arm].values()),
                             "library_launches": launches[arm]}
    if "a" in arms and "b" in arms:
        out["speedup_b_over_a"] = round(out["arm_a"]["wall_ms_median"] / out["arm_b"]["wall_ms_median"], 3)
    if "b" in arms and "c" in arms:
        out["speedup_c_over_b"] = round(out["arm_b"]["wall_ms_median"] / out["arm_c"]["wall_ms_median"], 3)
    if "c" in arms and "d" in arms:
        out["speedup_d_over_c"] = round(out["arm_c"]["wall_ms_median"] / out["arm_d"]["wall_ms_median"], 3)
    if "b" in arms and not a.no_raw:
        out["raw_calls"] = raw_calls()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
