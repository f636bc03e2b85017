#!/usr/bin/env python3
"""Generates tests/golden/pcv_loss.npz by RUNNING THE REFERENCE (build container only, needs the reference tree):

    python tests/golden/make_golden_pcv_loss.py

For each case of _pcv_loss_ref.GOLDEN_CASES, the reference's own sequence_loss_pcvnet (meta_arch/pcvnet/loss.py:4-73) on
target 0 of the case under CPU autograd in fp32, on fresh lists every time:

  <case>/raises                                the exception's class name, or "" when the call returns
  <case>/loss, metrics (14 or 4), mask         what it returns (loss 0 for the empty mask; metrics in _pcv_loss_ref.METRIC_KEYS order)
  <case>/grefine, gdisp, gmu                   the gradients of UPSTREAM[0] * loss (stacked over the predictions)

and, as a fact about the reference, `second_call/raises`: what a second call on the same `results` raises (the first call
leaves mu_preds rebound to 5-D views and loss.py:18 unpacks four sizes).  The inputs are those of _pcv_loss_ref.inputs and
are not stored.  Only data is stored: no reference source.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _refimport  # noqa: E402
import _pcv_loss_ref as R  # noqa: E402

OUT = os.path.join(HERE, "pcv_loss.npz")


def results_of(a):
    leaf = lambda v: torch.from_numpy(np.ascontiguousarray(v)).requires_grad_(True)                    # noqa: E731
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v))                                            # noqa: E731
    refine, disps, mus = leaf(a["refine"]), [leaf(v) for v in a["disp"]], [leaf(v) for v in a["mu"]]
    res = {"output_list": (refine, list(disps), list(mus), [t(v) for v in a["w"]], [t(v) for v in a["sigma"]])}
    return res, [refine] + disps + mus


def main():
    _refimport.setup()
    import meta_arch.pcvnet.loss as ref_loss
    out = {}
    for name in R.GOLDEN_CASES:
        a = R.inputs(name)
        res, leaves = results_of(a)
        args = types.SimpleNamespace(gauss_num=a["M"])
        gt, valid = torch.from_numpy(a["gt"][0]), torch.from_numpy(a["valid"][0])
        try:
            loss, metrics, mask = ref_loss.sequence_loss_pcvnet(res, gt, valid, args=args)
        except (AssertionError, IndexError) as e:
            out[name + "/raises"] = np.array(type(e).__name__)
            print("%-14s raises %s" % (name, type(e).__name__))
            continue
        out[name + "/raises"] = np.array("")
        out[name + "/mask"] = mask.numpy()
        out[name + "/metrics"] = np.array([metrics[k] for k in R.METRIC_KEYS if k in metrics], np.float64)
        out[name + "/loss"] = np.array(float(loss), np.float64)
        if torch.is_tensor(loss):
            n = len(a["mu"])
            grads = torch.autograd.grad(loss * R.UPSTREAM[0], leaves, allow_unused=True)
            grads = [torch.zeros_like(l) if g is None else g for l, g in zip(leaves, grads)]
            out[name + "/grefine"] = grads[0].numpy()
            out[name + "/gdisp"] = torch.stack(grads[1:1 + n]).numpy()
            out[name + "/gmu"] = torch.stack(grads[1 + n:]).numpy()
        print("%-14s loss %.6g, %d metrics, %d mask pixels" % (name, float(loss), len(metrics), int(mask.sum())))
    a = R.inputs("ord")
    res, _ = results_of(a)
    args = types.SimpleNamespace(gauss_num=a["M"])
    gt, valid = torch.from_numpy(a["gt"][0]), torch.from_numpy(a["valid"][0])
    ref_loss.sequence_loss_pcvnet(res, gt, valid, args=args)
    try:
        ref_loss.sequence_loss_pcvnet(res, gt, valid, args=args)
        second = ""
    except Exception as e:                                                          # noqa: BLE001  (recorded, whatever it is)
        second = type(e).__name__
    out["second_call/raises"] = np.array(second)
    out["second_call/mu_dim"] = np.array(res["output_list"][2][0].dim())
    print("second call on the same results raises %r; mu_preds[0] is %d-D" % (second, res["output_list"][2][0].dim()))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
