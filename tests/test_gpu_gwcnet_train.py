"""GWCNet training forward + backward (gwc_main.py:279-326 in train()) against the reference's own step
(golden/gwcnet_train.npz, make_golden_train.py): predictions, loss_gwcnet loss, parameter gradients, BatchNorm
running statistics; the return conventions; an optimiser step."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _cases
import _synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = ("concat", "gwc")
GRAD_PARAMS = ("feature_extraction.firstconv.0.0.weight", "feature_extraction.layer2.0.conv1.0.0.weight",
               "feature_extraction.lastconv.2.weight", "dres0.0.0.weight", "classif0.2.weight")
# The reference's own fp32 step is not closer than this to its float64 evaluation (same step on the CPU): predictions
# 3.4e-3 max-abs (values up to ~137: BatchNorm batch statistics of a two-image batch amplify rounding), parameter
# gradients up to 5.5e-3 of each tensor's max.  Observed on MI355X against the fixture: predictions 7.1e-3 (pred3,
# concat), gradients 9.4e-3 (dres0.0.0.weight, concat).  Bounds: 2.8x / 2.1x the observed values.
PRED_BOUND = 2e-2
GRAD_REL_BOUND = 2e-2


def loss_gwcnet(preds, gt, valid, maxdisp=192):
    """gwc_loss.py:5-19: weighted smooth-L1 over the valid pixels of the four predictions."""
    mag = torch.sum(gt ** 2, dim=1).sqrt()
    valid = ((valid >= 0.5) & (mag < maxdisp)).unsqueeze(1)
    return sum(w * F.smooth_l1_loss(p[valid], gt[valid]) for p, w in zip(preds, (0.5, 0.5, 0.7, 1.0)))


def make_model(use_concat_volume):
    from dkt_stereo_amd.gwcnet import GWCNet, make_args
    m = GWCNet(make_args(use_concat_volume=use_concat_volume))
    m.load_state_dict(_synth.torch_state_dict(_synth.shapes_of(m), _cases.GWCNET_WEIGHT_SEED), strict=True)
    return m.to(DEV)


def inputs(g, name):
    seed, B, H, W, shift, cat, stride = (int(v) for v in g["%s/meta" % name])
    i1, i2 = _synth.image_pair(seed, B, H, W, shift)
    gt = -_synth.uniform((B, 1, H, W), 0.0, 40.0, seed, "gt")
    valid = (_synth.uniform((B, H, W), 0.0, 1.0, seed, "valid") > 0.2).astype(np.float32)
    T = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    return T(i1), T(i2), T(gt), T(valid), bool(cat), stride


_STEP = {}


def train_step(golden, name):
    """One reference-style step (forward in train(), loss, backward), cached per case.

    The 2-D and 3-D layers run on the vendor library, whose default algorithm choice is not deterministic: from run to
    run the loss moved in its 7th digit and the gwc case's dres0.0.0.weight gradient ranged from 5e-3 to 2.5e-2 of its
    max away from the fixture.  With deterministic algorithm selection, forward and backward included, repeated runs
    gave the same loss and predictions and gradients within 1e-2 of the fixture, so the step is measured that way."""
    if name not in _STEP:
        g = golden("gwcnet_train")
        i1, i2, gt, valid, cat, stride = inputs(g, name)
        model = make_model(cat).train()
        was = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = True
        try:
            res = model(i1, i2)
            loss = loss_gwcnet(res["disp_preds"], gt, valid)
            loss.backward()
            torch.cuda.synchronize()
        finally:
            torch.backends.cudnn.deterministic = was
        _STEP[name] = (g, model, res, loss, stride)
    return _STEP[name]


@pytest.mark.parametrize("name", CASES)
def test_train_predictions(name, golden):
    g, _, res, _, s = train_step(golden, name)
    preds = res["disp_preds"]
    assert isinstance(preds, list) and len(preds) == 4
    for i, p in enumerate(preds):
        assert tuple(p.shape) == (2, 1, 64, 128)
        d = float(np.abs(p.detach().cpu().numpy()[:, :, ::s, ::s] - g["%s/pred%d" % (name, i)]).max())
        print("%s pred%d: max|d| %.3e" % (name, i, d))
        assert d <= PRED_BOUND


@pytest.mark.parametrize("name", CASES)
def test_train_loss(name, golden):
    g, _, _, loss, _ = train_step(golden, name)
    want = float(g["%s/loss" % name])
    rel = abs(float(loss) - want) / abs(want)
    print("%s loss %.6f vs %.6f: rel %.3e" % (name, float(loss), want, rel))
    assert rel <= 1e-4


@pytest.mark.parametrize("name", CASES)
def test_train_parameter_gradients(name, golden):
    g, model, _, _, _ = train_step(golden, name)
    params = dict(model.named_parameters())
    checked = 0
    for k in GRAD_PARAMS:
        key = "%s/grad/%s" % (name, k)
        if key not in g.files:
            continue
        want = g[key]
        got = params[k].grad.detach().cpu().numpy()
        rel = float(np.abs(got - want).max() / np.abs(want).max())
        print("%s grad %s: rel %.3e" % (name, k, rel))
        checked += 1
        assert rel <= GRAD_REL_BOUND, k
    assert checked >= 4


@pytest.mark.parametrize("name", CASES)
def test_train_bn_running_statistics(name, golden):
    g, model, _, _, _ = train_step(golden, name)
    sd = model.state_dict()
    keys = [k for k in g.files if k.startswith(name + "/bn/")]
    assert len(keys) > 50
    worst = 0.0
    for key in keys:
        k = key[len(name) + 4:]
        want = g[key]
        got = sd[k].cpu().numpy()
        if k.endswith("num_batches_tracked"):
            assert int(got) == int(want), k
            continue
        d = float(np.abs(got - want).max() / max(1.0, float(np.abs(want).max())))
        worst = max(worst, d)
        assert d <= 1e-4, k
    print("%s running statistics: worst rel %.3e" % (name, worst))


def test_return_conventions():
    model = make_model(True)
    i1, i2 = (torch.from_numpy(a).to(DEV) for a in _synth.image_pair(3, 1, 64, 128, 12))
    model.train()
    none, preds = model(i1, i2, test_mode=True)
    assert none is None and isinstance(preds, list) and len(preds) == 4
    res = model(i1, i2)
    assert set(res) == {"disp_preds"} and len(res["disp_preds"]) == 4
    model.eval()
    res = model(i1, i2)
    assert set(res) == {"disp_preds"} and torch.is_tensor(res["disp_preds"])
    assert tuple(res["disp_preds"].shape) == (1, 1, 64, 128)
    none, disp = model(i1, i2, test_mode=True)
    assert none is None and tuple(disp.shape) == (1, 1, 64, 128) and not disp.requires_grad
    assert float((disp - res["disp_preds"]).abs().max()) <= 1e-3


def test_optimiser_step_changes_feature_weights():
    model = make_model(True).train()
    g = _synth
    i1, i2 = (torch.from_numpy(a).to(DEV) for a in g.image_pair(5, 2, 64, 128, 12))
    gt = torch.from_numpy(-g.uniform((2, 1, 64, 128), 0.0, 40.0, 5, "gt")).to(DEV)
    valid = torch.ones((2, 64, 128), device=DEV)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    w0 = model.feature_extraction.firstconv[0][0].weight.detach().clone()
    l0 = model.feature_extraction.layer4[0].conv1[0][0].weight.detach().clone()
    loss = loss_gwcnet(model(i1, i2)["disp_preds"], gt, valid)
    opt.zero_grad()
    loss.backward()
    assert model.feature_extraction.firstconv[0][0].weight.grad.abs().max() > 0
    opt.step()
    assert not torch.equal(model.feature_extraction.firstconv[0][0].weight, w0)
    assert not torch.equal(model.feature_extraction.layer4[0].conv1[0][0].weight, l0)
    assert torch.isfinite(loss)
