#!/usr/bin/env python3
"""Generates tests/golden/pcv_update.npz by RUNNING THE REFERENCE (build container only, needs the reference tree):

    python tests/golden/make_golden_pcv_update.py

For each case of _pcv_update_ref.GOLDEN_CASES, the reference's own ParametersUpdater (meta_arch/pcvnet/update.py:76-108) with
its head replaced by the identity, so that hidden_state IS delta, and model.py:154's regression, under CPU autograd in fp32:

  <case>/mu, w, sigma, disp                    the three results and sum_j w mu
  <case>/gdelta, gmu, gsigma, gw               the gradients of sum(mu gmu_out + w gw_out + sigma gsigma_out + disp gdisp)

and, when meta_arch.pcvnet.model imports with _refimport's stand-ins, PCVNet.convex_upsample called unbound on a namespace
carrying args, for the four up-samplings of model.py:165-174 on one small case:

  up/disp, mu, sigma, w, mask                  the inputs (drawn here, stored so that the fixture stands alone)
  up/disp_up, mu_up, sigma_up, w_up            the four results

The inputs of the update cases are those of _pcv_update_ref.inputs and are not stored.  Only data is stored: no reference source.
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
import _pcv_update_ref as R  # noqa: E402
import _synth  # noqa: E402

OUT = os.path.join(HERE, "pcv_update.npz")
UP = dict(seed=741, N=1, G=2, H=3, W=5, n_downsample=2)


def up_inputs():
    c = UP
    f = 2 ** c["n_downsample"]
    shp = (c["N"], c["G"], c["H"], c["W"])
    return dict(disp=_synth.normal((c["N"], 1, c["H"], c["W"]), c["seed"], "disp", scale=5.0),
                mu=_synth.normal(shp, c["seed"], "mu", scale=5.0), sigma=_synth.uniform(shp, 0.5, 4.0, c["seed"], "sigma"),
                w=_synth.uniform(shp, 0.0, 1.0, c["seed"], "w"),
                mask=_synth.normal((c["N"], 9 * f * f, c["H"], c["W"]), c["seed"], "mask", scale=2.0))


def main():
    _refimport.setup()
    import meta_arch.pcvnet.update as ref_update
    out = {}
    for name in R.GOLDEN_CASES:
        a = R.inputs(R.CASES[name])
        upd = ref_update.ParametersUpdater(types.SimpleNamespace(gauss_num=R.CASES[name]["M"]), 4, 4)
        upd.head = torch.nn.Identity()

        def fn(delta, mu, sigma, w, **_):
            mu, w, sigma = upd(delta, mu, sigma, w)
            return mu, w, sigma, torch.sum(w * mu, dim=1, keepdim=True)             # model.py:154
        got = R.torch_chain(a, torch.float32, fn=fn)
        for k, v in got.items():
            out["%s/%s" % (name, k)] = v.detach().numpy()
        print("%-8s disp in [%.4g, %.4g], |gw| up to %.4g" % (name, float(got["disp"].min()), float(got["disp"].max()),
                                                             float(got["gw"].abs().max())))
    try:
        import meta_arch.pcvnet.model as ref_model
    except Exception as e:                                                          # the model pulls in the whole network
        print("meta_arch.pcvnet.model does not import (%s: %s): the up-sampling part is left out" % (type(e).__name__, e))
    else:
        c, a = UP, up_inputs()
        t = {k: torch.from_numpy(v) for k, v in a.items()}
        me = types.SimpleNamespace(args=types.SimpleNamespace(n_downsample=c["n_downsample"], gauss_num=c["G"]))
        ups = ref_model.PCVNet.convex_upsample
        N, G, H, W = t["mu"].shape
        rep = t["mask"].repeat(1, G, 1, 1).reshape(N * G, -1, H, W)
        res = dict(disp_up=ups(me, t["disp"], t["mask"]), sigma_up=ups(me, t["sigma"].reshape(-1, 1, H, W), rep),
                   mu_up=ups(me, t["mu"].reshape(-1, 1, H, W), rep), w_up=ups(me, t["w"].reshape(-1, 1, H, W), rep, scale=False))
        for k, v in list(a.items()) + [(k, v.numpy()) for k, v in res.items()]:
            out["up/%s" % k] = v
        print("up       four results of", tuple(res["mu_up"].shape))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
