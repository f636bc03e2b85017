#!/usr/bin/env python3
"""PCVNet's sequence loss in a training step, forward + backward, at the crop of configs/pcvnet/base.json of the reference:
320 x 720, gauss_num 4, six predictions (final_disp, mu, w, sigma each) and disp_refine, B = 1 and B = 8.

  single  arm torch  meta_arch/pcvnet/loss.py:4-73 restated in torch on the device, fp32, under autograd, in the reference's
                     own sequence: the eight isnan / isinf .any() tests per prediction, the boolean-index gathers, the 14 .item()s;
          arm node   pcvnet_loss.sequence_loss_pcvnet: dkt_pcv_loss + dkt_pcv_loss_bwd, one host read.
  pair    arm torch  the restatement called twice (ground truth, pseudo label), as tools/ft_dkt.py:227-228 would;
          arm node   pcvnet_loss.pcv_loss_pair: one forward, one backward launch, one host read.

The arms alternate in one process after warm-up.  Per arm, as median (min .. max) over the steps: device us (HIP events around
the Python calls, host time and host round trips between launches included), the kernel launches of one step as
torch.profiler counts them, the synchronising calls of one step (torch.cuda.set_sync_debug_mode("warn")) and
torch.cuda.max_memory_allocated over the step's start.  The torch arm is the yardstick.  Then the two entries alone, raw
C-ABI calls back to back on rotating buffer sets, with the w / sigma check on and off, against the time their compulsory
bytes would take at the copy rate measured in the same run (forward, check on: (3 M + 1) n + 1 prediction planes and two
target planes read per target set, about 80 fp32 planes per image; check off: (M + 1) n + 1).

    python tools/bench_pcv_loss.py [--steps 10] [--warmup 3] [--batches 1,8]
"""
import argparse
import json
import os
import sys
import types
import warnings

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_pcv_train import launches, measure, stats, timed  # noqa: E402
from dkt_stereo_amd import _ffi, pcvnet_loss as P  # noqa: E402

DEV = "cuda:0"
M, H, W, N_PRED = 4, 320, 720, 6
ARGS = types.SimpleNamespace(gauss_num=M)
I_WEIGHTS = [0.4, 0.6, 0.8, 1, 1.2, 1.4]


def torch_loss(results, disp_gt, valid, max_disp=512):
    """The reference's sequence, synchronisations included; the lists are left alone so that it can be called twice."""
    disp_refine, final_disp_preds, mu_preds, w_preds, sigma_preds = results['output_list']
    valid = (disp_gt < max_disp) & (valid[:, None].bool()) & (disp_gt >= 0)
    assert not torch.isinf(disp_gt[valid.bool()]).any()
    N, _, h, w = mu_preds[0].shape
    if (valid == False).all():                                           # noqa: E712
        return 0, {'epe': 0., '1px': 1., '3px': 1., '5px': 1.}, valid
    sel = valid.view(-1)
    loss = 0.0
    for i in range(len(mu_preds)):
        for t in (mu_preds[i], w_preds[i], sigma_preds[i], final_disp_preds[i]):
            assert not torch.isnan(t).any() and not torch.isinf(t).any()
        mu = mu_preds[i].view(N // M, M, 1, h, w)
        l1 = (final_disp_preds[i] - disp_gt).abs()
        l2 = torch.mean((mu - disp_gt[:, None]).abs(), dim=1)
        loss += I_WEIGHTS[i] * (l1.view(-1)[sel].mean() + l2.view(-1)[sel].mean())
    loss += 1.4 * F.smooth_l1_loss(disp_refine[valid], disp_gt[valid], reduction='mean')
    metrics = {}
    for tail, p in (('', final_disp_preds[3]), ('_final', disp_refine)):
        e = torch.abs(p - disp_gt).view(-1)[sel]
        metrics['epe' + tail] = e.mean().item()
        for key, hit in (('1px', e < 1), ('3px', e < 3), ('5px', e < 5), ('bad1', e > 1), ('bad2', e > 2), ('bad5', e > 5)):
            metrics[key + tail] = hit.float().mean().item()
    return loss, metrics, valid


def draw(B, g):
    rnd = lambda *shape, scale=1.0: (torch.randn(shape, generator=g) * scale).to(DEV)                   # noqa: E731
    base = (torch.rand((B, 1, H, W), generator=g) * 120).to(DEV)
    rep = base.repeat(1, M, 1, 1).reshape(B * M, 1, H, W)
    t = dict(gt=base + rnd(B, 1, H, W), pl=base + rnd(B, 1, H, W, scale=0.5),
             valid=(torch.rand((B, H, W), generator=g) < 0.85).float().to(DEV), valid_pl=torch.ones((B, H, W), device=DEV),
             refine=(base + rnd(B, 1, H, W)).requires_grad_(True),
             disp=[(base + rnd(B, 1, H, W, scale=3.0)).requires_grad_(True) for _ in range(N_PRED)],
             mu=[(rep + rnd(B * M, 1, H, W, scale=4.0)).requires_grad_(True) for _ in range(N_PRED)],
             w=[torch.rand((B * M, 1, H, W), generator=g).to(DEV) for _ in range(N_PRED)],
             sigma=[(0.5 + torch.rand((B * M, 1, H, W), generator=g)).to(DEV) for _ in range(N_PRED)])
    return t


def results_of(t):
    return {"output_list": (t["refine"], list(t["disp"]), list(t["mu"]), list(t["w"]), list(t["sigma"]))}


def count_syncs(fn, before):
    before()
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    return sum("called a synchronizing" in str(r.message) for r in rec)


def steps_of(B, steps, warmup):
    g = torch.Generator(device="cpu").manual_seed(0)
    t = draw(B, g)
    leaves = [t["refine"]] + t["disp"] + t["mu"]

    def clear():
        for x in leaves:
            x.grad = None

    def single(fn):
        def run():
            loss, _, _ = fn(results_of(t), t["gt"], t["valid"])
            loss.backward()
        return run

    def pair_torch():
        res = results_of(t)
        l0, _, _ = torch_loss(res, t["gt"], t["valid"])
        l1, _, _ = torch_loss(res, t["pl"], t["valid_pl"])
        (l0 + l1 * 1.0).backward()

    def pair_node():
        l0, _, _, l1, _ = P.pcv_loss_pair(results_of(t), t["gt"], t["valid"], t["pl"], t["valid_pl"], args=ARGS)
        (l0 + l1 * 1.0).backward()

    node = lambda res, gt, valid: P.sequence_loss_pcvnet(res, gt, valid, args=ARGS)                    # noqa: E731
    out = {}
    for title, arms in (("single", {"torch": single(torch_loss), "node": single(node)}), ("pair", {"torch": pair_torch, "node": pair_node})):
        grads = {}
        for name, fn in arms.items():
            clear()
            fn()
            grads[name] = [x.grad.clone() for x in leaves]
        agree = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(grads["node"], grads["torch"]))
        counts = {name: (launches(fn, clear), count_syncs(fn, clear)) for name, fn in arms.items()}
        rows = {name: ([], []) for name in arms}
        for i in range(warmup + steps):
            for name, fn in arms.items():
                us, peak = measure(fn, clear)
                if i >= warmup:
                    rows[name][0].append(us)
                    rows[name][1].append(peak)
        print("%s: B = %d, %d x %d, M = %d, n = %d, forward + backward, %d steps; median (min .. max) device us; gradients agree to %.1e"
              % (title, B, H, W, M, N_PRED, steps, agree))
        res = {}
        for name, (us, peak) in rows.items():
            line, med = stats(us)
            print("  %-6s %s us | %s launches | %d synchronising calls | max_memory_allocated over the start %.1f MB"
                  % (name, line, counts[name][0], counts[name][1], max(peak) / 1e6))
            res[name] = {"us": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1), "launches": counts[name][0],
                         "syncs": counts[name][1], "peak_MB": round(max(peak) / 1e6, 1)}
        res["node_median_below_torch_min"] = res["node"]["us"] < res["torch"]["us_min"]
        print("  torch / node: x%.2f; node's median below torch's minimum: %s"
              % (res["torch"]["us"] / res["node"]["us"], res["node_median_below_torch_min"]))
        out[title] = res
    return out


def raw_entries(B, K, nsets=4):
    g = torch.Generator(device="cpu").manual_seed(1)
    sets = []
    for _ in range(nsets):
        t = draw(B, g)
        for x in [t["refine"]] + t["disp"] + t["mu"]:
            x.requires_grad_(False)
        t["gref"] = torch.empty_like(t["refine"])
        t["gdisp"] = [torch.empty_like(x) for x in t["disp"]]
        t["gmu"] = [torch.empty_like(x) for x in t["mu"]]
        t["mask"] = [torch.empty((B, 1, H, W), dtype=torch.bool, device=DEV) for _ in range(K)]
        t["loss"] = [torch.empty((), device=DEV) for _ in range(K)]
        t["up"] = [torch.ones((), device=DEV) for _ in range(K)]
        t["rec"] = torch.empty(_ffi.PCV_LOSS_REC, dtype=torch.float64, device=DEV)
        t["ws"] = torch.empty(_ffi.size("dkt_pcv_loss_partial_doubles", K, B, H, W), dtype=torch.float64, device=DEV)
        sets.append(t)

    def desc(t, check):
        d = _ffi.PcvLossDesc()
        for i in range(N_PRED):
            d.disp[i], d.disp_bstride[i] = t["disp"][i].data_ptr(), H * W
            d.mu[i], d.mu_bstride[i], d.mu_gstride[i] = t["mu"][i].data_ptr(), M * H * W, H * W
            if check:
                d.w[i], d.w_bstride[i], d.w_gstride[i] = t["w"][i].data_ptr(), M * H * W, H * W
                d.sigma[i], d.sigma_bstride[i], d.sigma_gstride[i] = t["sigma"][i].data_ptr(), M * H * W, H * W
            d.weight[i] = I_WEIGHTS[i]
        d.refine, d.refine_bstride, d.refine_weight = t["refine"].data_ptr(), H * W, 1.4
        d.n, d.n_loss, d.M, d.ntargets, d.max_disp = N_PRED, N_PRED, M, K, 512.0
        for k, (gt, valid) in enumerate((("gt", "valid"), ("pl", "valid_pl"))[:K]):
            d.gt[k], d.gt_bstride[k], d.valid[k], d.valid_bstride[k] = t[gt].data_ptr(), H * W, t[valid].data_ptr(), H * W
            d.mask[k], d.loss[k] = t["mask"][k].data_ptr(), t["loss"][k].data_ptr()
        d.rec, d.B, d.H, d.W = t["rec"].data_ptr(), B, H, W
        gr = _ffi.PcvLossGrad()
        gr.grefine = t["gref"].data_ptr()
        for i in range(N_PRED):
            gr.gdisp[i], gr.gmu[i] = t["gdisp"][i].data_ptr(), t["gmu"][i].data_ptr()
        for k in range(K):
            gr.grad_loss[k] = t["up"][k].data_ptr()
        return d, gr

    for t in sets:
        t["on"], t["off"] = desc(t, True), desc(t, False)
    plane = 4 * B * H * W
    read_on, read_off = (3 * M + 1) * N_PRED + 1 + 2 * K, (M + 1) * N_PRED + 1 + 2 * K
    bwd_planes = 2 * ((M + 1) * N_PRED + 1) + K
    nbytes = {"fwd_check_on": read_on * plane + K * plane // 4, "fwd_check_off": read_off * plane + K * plane // 4,
              "bwd": bwd_planes * plane + K * plane // 4}
    big = [dict(a=torch.empty(64 << 20, device=DEV), b=torch.empty(64 << 20, device=DEV)) for _ in range(3)]
    line, med = stats(timed(lambda t: t["b"].copy_(t["a"]), big, rounds=2))
    rate = 2 * big[0]["a"].numel() * 4 / (med * 1e-6)
    del big
    print("the entries alone, B = %d, %d target(s), %d buffer sets in rotation; median (min .. max) us per call" % (B, K, nsets))
    print("  copy_ of 256 MB (read + written 512 MB): %s us, %.2f TB/s" % (line, rate / 1e12))
    fns = {"fwd_check_on": lambda t: _ffi.call("dkt_pcv_loss", t["ws"], t["on"][0], t["ws"].data_ptr()),
           "fwd_check_off": lambda t: _ffi.call("dkt_pcv_loss", t["ws"], t["off"][0], t["ws"].data_ptr()),
           "bwd": lambda t: _ffi.call("dkt_pcv_loss_bwd", t["ws"], t["on"][0], t["on"][1])}
    out = {"copy_TBps": round(rate / 1e12, 3)}
    for name, fn in fns.items():
        us = timed(fn, sets)
        line, med = stats(us)
        floor = nbytes[name] / rate * 1e6
        print("  %-14s %s us; %.1f MB compulsory (%d fp32 planes per image) = %.2f us at the copy rate: %.3f of the copy rate"
              % (name, line, nbytes[name] / 1e6, nbytes[name] // plane, floor, floor / med))
        out[name] = {"us_per_call": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
                     "compulsory_MB": round(nbytes[name] / 1e6, 2), "of_copy_rate": round(floor / med, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,8")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pcv_loss.py measures on a HIP device; none is available")
    out = {}
    for B in (int(b) for b in a.batches.split(",")):
        out["B%d" % B] = dict(steps_of(B, a.steps, a.warmup), entries_single=raw_entries(B, 1), entries_pair=raw_entries(B, 2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
