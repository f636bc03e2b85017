#!/usr/bin/env python3
"""Generates tests/golden/pcv_train.npz by RUNNING THE REFERENCE (build container only, needs the reference tree):

    python tests/golden/make_golden_pcv_train.py

For each case of _pcv_train_ref.GOLDEN_CASES, the reference's own CorrBlock1D (meta_arch/pcvnet/corr.py:18-61) under CPU
autograd in fp32, every input a leaf:

  <case>/fmap1, fmap2, coords, sigma, gout     the inputs (those of _pcv_train_ref.inputs, stored so that the fixture stands alone)
  <case>/out                                   corr_fn(coords, sigma): (B, L G S, H, W)
  <case>/gf1, gf2, gcoords, gsigma             the gradients of sum(out * gout) with respect to the four inputs

Only data is stored: no reference source.
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _refimport  # noqa: E402
import _pcv_train_ref as R  # noqa: E402

OUT = os.path.join(HERE, "pcv_train.npz")


def main():
    ref = _refimport.load().pcv_corr
    out = {}
    for name in R.GOLDEN_CASES:
        c = R.CASES[name]
        a = R.inputs(c)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                 # (torch.range is deprecated)
            got = R.torch_chain(a, c, torch.float32, block=ref.CorrBlock1D)
        for k, v in a.items():
            out["%s/%s" % (name, k)] = v
        for k, v in got.items():
            out["%s/%s" % (name, k)] = v.detach().numpy()
        print("%-6s out in [%.4g, %.4g], |gsigma| up to %.4g" % (name, float(got["out"].min()), float(got["out"].max()),
                                                                float(got["gsigma"].abs().max())))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
