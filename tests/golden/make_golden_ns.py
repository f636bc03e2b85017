#!/usr/bin/env python3
"""Generates tests/golden/ns_loss.npz by RUNNING THE REFERENCE (build container only, needs the reference tree):

    python tests/golden/make_golden_ns.py

  <case>/...   ns_loss (meta_arch/nerf_stereo/loss.py:128-181) on every case of tests/_ns_loss_ref.py: the inputs, the loss,
               the metrics, the returned mask and the CPU autograd gradient of 1.7 * loss with respect to every prediction.
  raises/<k>   the name of the exception the reference raised for: a single prediction, trinocular_loss=False, a NaN in a
               prediction.

CPU, fp32.  The module is loaded by path; disp_warp's `device='cuda'` default is replaced from outside, the module's text
is untouched.  Only data is stored: no reference source.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _refimport  # noqa: E402
import _ns_loss_ref as R  # noqa: E402

OUT = os.path.join(HERE, "ns_loss.npz")


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_ns_loss", os.path.join(_refimport.REF, "meta_arch", "nerf_stereo", "loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.disp_warp.__defaults__ = mod.disp_warp.__defaults__[:-1] + ("cpu",)
    return mod


def tensors(c):
    a = {k: torch.from_numpy(v) for k, v in R.inputs(c).items()}
    return a, [p.clone().requires_grad_(True) for p in a["preds"]]


def raised(fn):
    try:
        fn()
    except Exception as e:          # noqa: BLE001
        return type(e).__name__
    return ""


def main():
    ref = load_reference()
    out = {}
    for name, c in R.CASES.items():
        a, preds = tensors(c)
        loss, metrics, mask = ref.ns_loss(preds, a["target"], a["conf"], a["im0"], a["im1"], a["im2"], **R.params(c))
        grads = torch.autograd.grad(1.7 * loss, preds, allow_unused=True)
        for k, v in a.items():
            out["%s/%s" % (name, k)] = v.numpy()
        out[name + "/loss"] = loss.detach().numpy()
        out[name + "/metrics"] = np.array([metrics[k] for k in ("epe", "1px", "3px", "5px")], np.float64)
        out[name + "/mask"] = mask.numpy()
        out[name + "/grads"] = np.stack([(torch.zeros_like(p) if g is None else g).numpy() for g, p in zip(grads, preds)])
        print("%-8s loss %.7g  automask share %.3f" % (name, float(loss), float(R.run(name, torch.float32)["per"][-1]["automask"].float().mean())
                                                        if R.params(c)["alpha_photometric"] else 0.0))
    a, preds = tensors(R.CASES["h5w9"])
    args = (a["target"], a["conf"], a["im0"], a["im1"], a["im2"])
    out["raises/n1"] = np.array(raised(lambda: ref.ns_loss(preds[:1], *args)))
    out["raises/binocular"] = np.array(raised(lambda: ref.ns_loss(preds, *args, trinocular_loss=False)))
    bad = [preds[0], preds[1].detach().clone()]
    bad[1][0, 0, 1, 2] = float("nan")
    out["raises/nan"] = np.array(raised(lambda: ref.ns_loss(bad, *args)))
    bad[0] = bad[1]
    out["raises/nan_n1"] = np.array(raised(lambda: ref.ns_loss(bad[:1], *args)))
    print({k: str(v) for k, v in out.items() if k.startswith("raises/")})
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
