#!/usr/bin/env python3
"""The feature encoder of a RAFT student step (BasicEncoder(norm_fn='instance', downsample=2), every weight trainable),
forward + backward with a scalar loss on its output, at the two training shapes: the recipe of
run_scripts/raft-stereo/ft_booster.sh (B = 2, 480 x 896: fnet sees 4 x 3 x 480 x 896) and the default crop of
tools/ft_dkt.py (16 x 3 x 320 x 720):

  arm a  extractor.TRAIN_NORM_NODES = False: torch's InstanceNorm2d, relu and add, forward and backward;
  arm b  extractor.TRAIN_NORM_NODES = True: the nodes of norm_train.py (dkt_instance_norm / _add_relu forward,
         dkt_instance_norm_bwd / dkt_instance_norm_add_relu_bwd backward).

The arms alternate in one process after warm-up; per arm the median and min wall ms of a step (host clock around a step
that ends in a synchronise) and torch.cuda.max_memory_allocated.  Arm a is timed twice per round ("a" and "a2"): the
difference of their medians is the spread an a-to-b difference has to beat.

--norm: each backward entry alone on one full-resolution tensor of the recipe (256 planes x 430 080), device events around
back-to-back calls on rotating buffers: us per call, the compulsory bytes 5 * 4 * planes * HW (the upstream gradient and
the normalised tensor are read by both launches, the gradient is written once; the join reads the output as well and
writes two gradients: 8 * 4 * planes * HW, 7 for gc alone, 3 for ga alone) and the fraction of the 6.29 TB/s measured
copy rate they amount to -- an HBM-bound figure: every tensor is larger than the Infinity Cache.  The same for the
backward of torch's sequence.

--arms conv: the same alternation for extractor.TRAIN_CONV_NODES (arm a off, arm b on, arm a twice), on the feature encoder
and on the context encoder (MultiBasicEncoder(norm_fn='batch', downsample=2) in eval(), every weight trainable, half the
batch: it sees the left images only).

--conv: each stride-2 backward entry alone (dkt_conv2d_dgrad_s2, dkt_conv2d_wgrad_s2 through their wrappers) against the
vendor call it replaces (torch.nn.grad.conv2d_input / conv2d_weight at stride 2) in the same process on the same tensors,
for every stride-2 layer of both encoders at both shapes, and the stride-1 weight gradient of the (64, 64, 3) class at the
encoder's full resolution: device events around back-to-back calls on rotating buffers, us per call.

    python tools/bench_encoder_train.py [--steps 10] [--warmup 3] [--shapes recipe,crop] [--arms norm|conv] [--norm] [--conv]
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

from dkt_stereo_amd import _ffi, conv, extractor  # noqa: E402

COPY_BPS = 6.29e12                        # measured device-to-device copy rate of the part
SHAPES = {"recipe": (4, 480, 896), "crop": (16, 320, 720)}
PLANES, HW = 4 * 64, 480 * 896


def _flat(out):
    return [out] if torch.is_tensor(out) else [t for o in out for t in _flat(o)]


def encoder_arms(name, steps, warmup, handle_name="TRAIN_NORM_NODES", which="fnet"):
    B, H, W = SHAPES[name]
    torch.manual_seed(0)
    if which == "fnet":
        fnet = extractor.BasicEncoder(output_dim=256, norm_fn="instance", downsample=2).cuda().train()
    else:
        B //= 2
        fnet = extractor.MultiBasicEncoder(output_dim=[[128] * 3, [128] * 3], norm_fn="batch", downsample=2).cuda().eval()
    params = list(fnet.parameters())
    x = torch.rand(B, 3, H, W, device="cuda") * 2 - 1
    with torch.no_grad():
        wls = [torch.randn_like(t) for t in _flat(fnet(x))]

    def step(handle):
        setattr(extractor, handle_name, handle)
        for p in params:
            p.grad = None
        sum((t * w).sum() for t, w in zip(_flat(fnet(x)), wls)).backward()

    order = (("a", False), ("b", True), ("a2", False))
    for _ in range(warmup):
        for _, handle in order:
            step(handle)
    torch.cuda.synchronize()
    wall = {k: [] for k, _ in order}
    peak = {}
    for _ in range(steps):
        for k, handle in order:
            for p in params:
                p.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            step(handle)
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            peak[k] = torch.cuda.max_memory_allocated()
    out = {"shape": [B, 3, H, W], "steps": steps, "handle": handle_name, "encoder": which}
    for k, _ in order:
        w = sorted(wall[k])
        out["arm_" + k] = {"wall_ms_median": round(w[len(w) // 2], 3), "wall_ms_min": round(w[0], 3),
                           "max_memory_allocated_MB": round(peak[k] / 1e6, 1)}
    a, b, a2 = (out["arm_" + k]["wall_ms_median"] for k in ("a", "b", "a2"))
    out["a_to_a_spread_ms"] = round(abs(a - a2), 3)
    out["b_gain_ms"] = round(min(a, a2) - b, 3)
    out["b_beats_a_by_more_than_the_spread"] = bool(min(a, a2) - b > abs(a - a2))
    return out


def _timed(fn, sets, rounds, reps):
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
    return sorted(us)[len(us) // 2]


def norm_entries(rounds=4, reps=5, nsets=3):
    """us per backward call on (4, 64, 480, 896) tensors; `nsets` buffer sets in rotation."""
    lib = _ffi.lib()
    shape = (4, 64, 480, 896)
    mk = lambda: torch.randn(shape, device="cuda")  # noqa: E731
    sets = []
    for _ in range(nsets):
        x, g, a = mk(), mk(), mk()
        with torch.no_grad():
            ws = torch.empty(lib.dkt_instance_norm_workspace(PLANES, HW), device="cuda", dtype=torch.uint8)
            out = torch.empty_like(x)
            mi = torch.empty((PLANES, 2), device="cuda")
            dev, st = _ffi.device_of(x), _ffi.stream_of(x)
            _ffi.check(lib.dkt_instance_norm_stats(x.data_ptr(), ws.data_ptr(), PLANES, HW, dev, st), "stats")
            _ffi.check(lib.dkt_instance_norm_add_relu(a.data_ptr(), x.data_ptr(), out.data_ptr(), ws.data_ptr(), PLANES, HW,
                                                      1e-5, dev, st), "join")
            _ffi.check(lib.dkt_instance_norm_finalize(ws.data_ptr(), PLANES, HW, 1e-5, mi.data_ptr(), dev, st), "finalize")
        bws = torch.empty(lib.dkt_instance_norm_bwd_workspace(PLANES, HW), device="cuda", dtype=torch.uint8)
        sets.append(dict(x=x, g=g, out=out, mi=mi, ws=bws, g1=torch.empty_like(x), g2=torch.empty_like(x)))
        del a
    dev, st = _ffi.device_of(sets[0]["x"]), _ffi.stream_of(sets[0]["x"])
    p = lambda t: t.data_ptr()  # noqa: E731

    def norm_bwd(relu):
        return lambda t: lib.dkt_instance_norm_bwd(p(t["g"]), p(t["x"]), p(t["mi"]), relu, p(t["g1"]), p(t["ws"]), PLANES, HW, dev, st)

    def join_bwd(ga, gc):
        return lambda t: lib.dkt_instance_norm_add_relu_bwd(p(t["g"]), p(t["out"]), p(t["x"]), p(t["mi"]), p(t["g1"]) if ga else None,
                                                            p(t["g2"]) if gc else None, p(t["ws"]), PLANES, HW, dev, st)

    plane_bytes = 4 * PLANES * HW
    cases = [("norm_bwd", norm_bwd(0), 5), ("norm_relu_bwd", norm_bwd(1), 5), ("join_bwd_both", join_bwd(True, True), 8),
             ("join_bwd_c_only", join_bwd(False, True), 7), ("join_bwd_a_only", join_bwd(True, False), 3)]
    res = {}
    for name, fn, passes in cases:
        us = _timed(fn, sets, rounds, reps)
        res[name] = {"us_per_call": round(us, 1), "compulsory_MB": round(passes * plane_bytes / 1e6, 1),
                     "frac_of_6.29TBps_HBM_bound": round(passes * plane_bytes / COPY_BPS / (us * 1e-6), 3)}

    # torch's sequence on the same tensors: backward only (the graph is rebuilt outside the timed span by retain_graph)
    def torch_case(build, passes, name):
        graphs = []
        for t in sets[:2]:
            xs = t["x"].detach().requires_grad_(True)
            graphs.append((build(xs, t), xs, t["g"]))
        fn = lambda gr: torch.autograd.grad(gr[0], gr[1], gr[2], retain_graph=True)  # noqa: E731
        us = _timed(fn, graphs, rounds, reps)
        res[name] = {"us_per_call": round(us, 1), "compulsory_MB": round(passes * plane_bytes / 1e6, 1),
                     "frac_of_6.29TBps_HBM_bound": round(passes * plane_bytes / COPY_BPS / (us * 1e-6), 3)}

    torch_case(lambda xs, t: F.relu(F.instance_norm(xs)), 5, "torch_norm_relu_bwd")
    torch_case(lambda xs, t: F.relu(t["g1"] + F.relu(F.instance_norm(xs))), 7, "torch_join_bwd_c_only")
    return res


def conv_entries(shapes, rounds=3, reps=5, nsets=2):
    """us per call of each stride-2 backward entry and of the vendor call it replaces, per (encoder layer, shape)."""
    res = {}
    for name in shapes:
        B, H, W = SHAPES[name]
        # (label, batch, Cin, Cout, K, input height, input width)
        layers = [("fnet.layer2.0.conv1", B, 64, 96, 3, H, W), ("fnet.layer2.0.downsample", B, 64, 96, 1, H, W),
                  ("fnet.layer3.0.conv1", B, 96, 128, 3, H // 2, W // 2), ("fnet.layer3.0.downsample", B, 96, 128, 1, H // 2, W // 2),
                  ("cnet.layer2.0.conv1", B // 2, 64, 96, 3, H, W), ("cnet.layer2.0.downsample", B // 2, 64, 96, 1, H, W),
                  ("cnet.layer3.0.conv1", B // 2, 96, 128, 3, H // 2, W // 2),
                  ("cnet.layer3.0.downsample", B // 2, 96, 128, 1, H // 2, W // 2),
                  ("cnet.layer4.0.conv1", B // 2, 128, 128, 3, H // 4, W // 4),
                  ("cnet.layer4.0.downsample", B // 2, 128, 128, 1, H // 4, W // 4),
                  ("cnet.layer5.0.conv1", B // 2, 128, 128, 3, H // 8, W // 8),
                  ("cnet.layer5.0.downsample", B // 2, 128, 128, 1, H // 8, W // 8)]
        for label, b, cin, cout, k, h, w in layers:
            torch.manual_seed(1)
            lay = torch.nn.Conv2d(cin, cout, k, stride=2, padding=k // 2).cuda()
            ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            sets = []
            with torch.no_grad():
                for _ in range(nsets):
                    x = torch.randn(b, cin, h, w, device="cuda")
                    g = torch.randn(b, cout, ho, wo, device="cuda") * 2.0 ** -10
                    conv.conv2d(x, lay)                                     # the forward image the scale is taken from
                    sets.append(dict(x=x, g=g, scale=conv.conv_grad_prepass(g, None, want_bias=False)[2]))
                shim = conv._grad_layer(lay)
                wd = lay.weight.detach()
                row = {"shape": [b, cin, h, w], "cout": cout, "k": k}
                row["dgrad_s2_us"] = round(_timed(lambda t: conv.conv2d_dgrad_s2(t["g"], shim, t["scale"], (h, w), shim.pack_scale),
                                                  sets, rounds, reps), 1)
                row["vendor_input_us"] = round(_timed(lambda t: torch.nn.grad.conv2d_input(t["x"].shape, wd, t["g"], stride=2,
                                                                                           padding=k // 2), sets, rounds, reps), 1)
                row["wgrad_s2_us"] = round(_timed(lambda t: conv.conv2d_wgrad_s2(t["x"], t["g"], t["scale"], k), sets, rounds, reps), 1)
                row["vendor_weight_us"] = round(_timed(lambda t: torch.nn.grad.conv2d_weight(t["x"], wd.shape, t["g"], stride=2,
                                                                                             padding=k // 2), sets, rounds, reps), 1)
            res["%s@%s" % (label, name)] = row
            print(json.dumps({"%s@%s" % (label, name): row}), flush=True)
            del sets
            torch.cuda.empty_cache()
        # the stride-1 (64, 64, 3) class of layer1 at full resolution (its WGRAD_VENDOR_CLASSES entry was decided at 120 x 224)
        with torch.no_grad():
            sets = []
            for _ in range(nsets):
                x = torch.randn(B, 64, H, W, device="cuda")
                g = torch.randn(B, 64, H, W, device="cuda") * 2.0 ** -10
                sets.append(dict(x=x, g=g, scale=conv.conv_grad_prepass(g, None, want_bias=False)[2]))
            row = {"shape": [B, 64, H, W], "cout": 64, "k": 3}
            row["wgrad_us"] = round(_timed(lambda t: conv.conv2d_wgrad(t["x"], t["g"], t["scale"], 3), sets, rounds, reps), 1)
            row["vendor_weight_us"] = round(_timed(lambda t: torch.nn.grad.conv2d_weight(t["x"], (64, 64, 3, 3), t["g"], stride=1,
                                                                                         padding=1), sets, rounds, reps), 1)
        res["layer1 wgrad (64,64,3)@%s" % name] = row
        print(json.dumps({"layer1 wgrad (64,64,3)@%s" % name: row}), flush=True)
        del sets
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="recipe,crop")
    ap.add_argument("--norm", action="store_true")
    ap.add_argument("--conv", action="store_true")
    ap.add_argument("--arms", default="norm", choices=["norm", "conv"])
    ap.add_argument("--encoders", default="fnet,cnet")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_encoder_train.py measures on a HIP device; none is available")
    default, default_conv = extractor.TRAIN_NORM_NODES, extractor.TRAIN_CONV_NODES
    out = {"default_TRAIN_NORM_NODES": default, "default_TRAIN_CONV_NODES": default_conv}
    if a.norm:
        out["norm_entries"] = norm_entries()
    elif a.conv:
        out["conv_entries"] = conv_entries(a.shapes.split(","))
    elif a.arms == "conv":
        for which in a.encoders.split(","):
            for name in a.shapes.split(","):
                key = "%s@%s" % (which, name)
                out[key] = encoder_arms(name, a.steps, a.warmup, "TRAIN_CONV_NODES", which)
                print(json.dumps({key: out[key]}), flush=True)
                torch.cuda.empty_cache()
    else:
        for name in a.shapes.split(","):
            out[name] = encoder_arms(name, a.steps, a.warmup)
            print(json.dumps({name: out[name]}), flush=True)
            torch.cuda.empty_cache()
    extractor.TRAIN_NORM_NODES, extractor.TRAIN_CONV_NODES = default, default_conv
    print(json.dumps(out))


if __name__ == "__main__":
    main()
