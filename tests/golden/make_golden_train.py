#!/usr/bin/env python3
"""Generates the training-path fixtures by RUNNING THE REFERENCE (build container only, needs the reference tree):

    python tests/golden/make_golden_train.py

  volumes_bwd.npz   torch autograd gradients of the reference's build_gwc_volume and of both build_concat_volume
                    definitions (gwcnet/submodules.py:25-58, igev_stereo/submodule.py:160-170,207-218) for a seeded
                    upstream gradient.  Each case stores its own parameters under "<kind>/<case>/meta".
  gwcnet_train.npz  the reference GWCNet (gwc_main.py) in train() mode, B = 2 at 64x128, both use_concat_volume
                    settings, weights _synth.torch_state_dict(shapes, GWCNET_WEIGHT_SEED): the four predictions
                    (strided), the loss_gwcnet weighted smooth-L1 loss against a synthetic ground truth, the gradients
                    of a few named parameters and every BatchNorm running statistic after the step.

CPU, fp32, inputs regenerated from seeds (tests/_synth.py).  Only data is stored: no reference source.
"""
import contextlib
import io
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import _cases  # noqa: E402
import _refimport  # noqa: E402
import _synth  # noqa: E402

torch.set_num_threads(8)
T = torch.from_numpy

# (seed, B, C, H, W, D, G): shapes like _cases.GWC_CASES plus a wide row (D = 48, W = 300), one cut into W chunks
# (32 channels per group, W = 200) and one whose tile exceeds the LDS budget (D = 64, 96 channels per group)
GWC_BWD_CASES = {
    "igev":  dict(seed=131, B=2, C=96, H=3, W=24, D=8, G=8),
    "gwc":   dict(seed=132, B=1, C=320, H=2, W=30, D=12, G=40),
    "dgtw":  dict(seed=133, B=1, C=8, H=2, W=6, D=9, G=2),       # D > W
    "g1":    dict(seed=134, B=1, C=5, H=2, W=17, D=4, G=1),
    "cpg40": dict(seed=135, B=2, C=80, H=2, W=21, D=6, G=2),
    "wide":  dict(seed=136, B=1, C=16, H=2, W=300, D=48, G=2),
    "deep":  dict(seed=137, B=1, C=96, H=1, W=80, D=64, G=1),
    "chunk": dict(seed=138, B=1, C=64, H=2, W=200, D=48, G=2),
}
CONCAT_BWD_CASES = {
    "gc":   dict(seed=141, B=2, C=12, H=3, W=24, D=8),
    "dgtw": dict(seed=142, B=1, C=3, H=2, W=5, D=7),
    "wide": dict(seed=143, B=1, C=4, H=2, W=300, D=48),
}
TRAIN_CASES = {
    "concat": dict(seed=61, B=2, H=64, W=128, shift=12, use_concat_volume=True, stride=2),
    "gwc":    dict(seed=62, B=2, H=64, W=128, shift=12, use_concat_volume=False, stride=2),
}
GRAD_PARAMS = ("feature_extraction.firstconv.0.0.weight", "feature_extraction.layer2.0.conv1.0.0.weight",
               "feature_extraction.lastconv.2.weight", "dres0.0.0.weight", "classif0.2.weight")


def save(name, **arrays):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("  wrote %s (%.1f KB)" % (os.path.basename(path), os.path.getsize(path) / 1024))


def train_gt(seed, B, H, W):
    """Synthetic ground truth in the flow convention of the loss (negative disparity) and a validity mask."""
    gt = -_synth.uniform((B, 1, H, W), 0.0, 40.0, seed, "gt")
    valid = (_synth.uniform((B, H, W), 0.0, 1.0, seed, "valid") > 0.2).astype(np.float32)
    return gt, valid


def _grads(fn, a, b, gvol):
    a, b = T(a).requires_grad_(), T(b).requires_grad_()
    vol = fn(a, b)
    vol.backward(T(gvol))
    return a.grad.numpy(), b.grad.numpy()


def gen_volumes_bwd(ref):
    print("cost-volume gradients (reference autograd)")
    out = {}
    for name, c in GWC_BWD_CASES.items():
        a, b = _synth.fmap_pair(c["seed"], c["B"], c["C"], c["H"], c["W"])
        gvol = _synth.normal((c["B"], c["G"], c["D"], c["H"], c["W"]), c["seed"], "gvol")
        ga, gb = _grads(lambda x, y: ref.gwc_sub.build_gwc_volume(x, y, c["D"], c["G"]), a, b, gvol)
        ia, ib = _grads(lambda x, y: ref.igev_sub.build_gwc_volume(x, y, c["D"], c["G"]), a, b, gvol)
        assert np.array_equal(ga, ia) and np.array_equal(gb, ib)
        out["gwc/%s/meta" % name] = np.array([c[k] for k in ("seed", "B", "C", "H", "W", "D", "G")], np.int64)
        out["gwc/%s/grad_ref" % name] = ga
        out["gwc/%s/grad_tgt" % name] = gb
    for name, c in CONCAT_BWD_CASES.items():
        a, b = _synth.fmap_pair(c["seed"], c["B"], c["C"], c["H"], c["W"])
        gvol = _synth.normal((c["B"], 2 * c["C"], c["D"], c["H"], c["W"]), c["seed"], "gvol")
        out["concat/%s/meta" % name] = np.array([c[k] for k in ("seed", "B", "C", "H", "W", "D")], np.int64)
        for kind, mod in (("gwcnet", ref.gwc_sub), ("igev", ref.igev_sub)):
            ga, gb = _grads(lambda x, y: mod.build_concat_volume(x, y, c["D"]), a, b, gvol)
            out["concat_%s/%s/grad_ref" % (kind, name)] = ga
            out["concat_%s/%s/grad_tgt" % (kind, name)] = gb
    save("volumes_bwd", **out)


def gen_gwcnet_train(ref):
    from meta_arch.gwcnet.gwc_loss import loss_gwcnet
    print("GwcNet training step (reference GWCNet.forward in train(), loss_gwcnet, backward)")
    out = {}
    for name, c in TRAIN_CASES.items():
        args = SimpleNamespace(maxdisp=192, use_concat_volume=c["use_concat_volume"], mixed_precision=False)
        with contextlib.redirect_stdout(io.StringIO()):
            model = ref.GWCNet(args)
        model.load_state_dict(_synth.torch_state_dict(_synth.shapes_of(model), _cases.GWCNET_WEIGHT_SEED), strict=True)
        model.train()
        i1, i2 = _synth.image_pair(c["seed"], c["B"], c["H"], c["W"], c["shift"])
        gt, valid = train_gt(c["seed"], c["B"], c["H"], c["W"])
        res = model(T(i1), T(i2))
        preds = res["disp_preds"]
        assert isinstance(preds, list) and len(preds) == 4
        loss, _, _ = loss_gwcnet(res, T(gt), T(valid), args)
        loss.backward()
        s = c["stride"]
        out["%s/meta" % name] = np.array([c["seed"], c["B"], c["H"], c["W"], c["shift"], int(c["use_concat_volume"]), s],
                                         np.int64)
        for i, p in enumerate(preds):
            out["%s/pred%d" % (name, i)] = p.detach().numpy()[:, :, ::s, ::s].copy()
        out["%s/loss" % name] = np.float64(loss.item())
        params = dict(model.named_parameters())
        for k in GRAD_PARAMS:
            if k in params:
                out["%s/grad/%s" % (name, k)] = params[k].grad.numpy().copy()
        for k, v in model.state_dict().items():
            if k.endswith((".running_mean", ".running_var", ".num_batches_tracked")):
                out["%s/bn/%s" % (name, k)] = v.numpy().copy()
        print("   %s: loss %.6f, pred3 range %.2f .. %.2f" % (name, loss.item(), float(preds[3].min()), float(preds[3].max())))
    save("gwcnet_train", **out)


def main():
    if not _refimport.available():
        raise SystemExit("reference tree not found at %s -- fixtures can only be generated in the build container"
                         % _refimport.REF)
    ref = _refimport.load()
    gen_volumes_bwd(ref)
    gen_gwcnet_train(ref)


if __name__ == "__main__":
    main()
