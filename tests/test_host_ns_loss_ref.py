"""The test infrastructure of the NeRF-supervised loss, on the CPU: the fp32 restatement of _ns_loss_ref.py reproduces what
the reference itself computed (tests/golden/ns_loss.npz), the yardstick is inside every bound, few pixels may differ in their
decisions, every mutant is outside, and the closed-form SSIM gather the kernel implements equals autograd's in float64."""
import math

import numpy as np
import pytest
import torch

import _ns_loss_ref as R
from dkt_stereo_amd import ns_loss as _module_under_test  # noqa: F401  (the operator these tests belong to)

NAMES = sorted(R.CASES)
PHOTO = [n for n in NAMES if R.params(R.CASES[n])["alpha_photometric"] != 0.0]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference(golden, name):
    g = golden("ns_loss")
    for k, v in R.inputs(R.CASES[name]).items():
        assert np.array_equal(g["%s/%s" % (name, k)], v), k
    y = R.reference(name)["yard"]
    loss = float(g[name + "/loss"])
    if math.isnan(loss):
        assert math.isnan(y["loss"])
    else:
        assert abs(y["loss"] - loss) <= 4e-6 * abs(loss)
    assert np.array_equal(g[name + "/mask"], y["valid"].numpy())
    m = g[name + "/metrics"]
    for k, ref in zip(("epe", "1px", "3px", "5px"), m):
        assert (math.isnan(ref) and math.isnan(y["metrics"][k])) or abs(y["metrics"][k] - ref) <= 1e-6 * max(1.0, abs(ref)), k
    grads = g[name + "/grads"]
    for i, gy in enumerate(y["grads"]):
        scale = max(1e-12, float(np.abs(grads[i]).max()))
        assert float(np.abs(gy.numpy() - grads[i]).max()) <= 2e-4 * scale, i


def test_recorded_exceptions(golden):
    g = golden("ns_loss")
    assert str(g["raises/n1"]) == "ZeroDivisionError"
    assert str(g["raises/binocular"]) == "TypeError"
    assert str(g["raises/nan"]) == "AssertionError"
    assert str(g["raises/nan_n1"]) == "AssertionError"          # the assertion of :155 comes before the weights of :157
    with pytest.raises(ZeroDivisionError):
        R.weights(1)


@pytest.mark.parametrize("name", PHOTO)
def test_yardstick_inside_plane_bounds_and_decision_rule(name):
    ref = R.reference(name)
    t, y = ref["truth"], ref["yard"]
    assert torch.equal(t["valid"], y["valid"])
    for i in range(len(t["per"])):
        b = R.plane_bounds(name, i)
        for k in ("p12", "p23", "loss_2"):
            assert R.worst(y["per"][i][k], t["per"][i][k], b[k]) <= 1.0, (i, k)
        md = R.may_differ(name, i)
        for k in ("automask", "third"):
            diff = y["per"][i][k] != t["per"][i][k]
            assert not bool((diff & ~md[k]).any()), (i, k)
            assert float(md[k].double().mean()) <= R.MAY_DIFFER, (i, k, float(md[k].double().mean()))


@pytest.mark.parametrize("name", NAMES)
def test_yardstick_inside_gradient_bounds_under_its_own_decisions(name):
    y = R.reference(name)["yard"]
    dec = [dict(automask=p["automask"], third=p["third"]) for p in y["per"]] or None
    t = R.run(name, torch.float64, decisions=dec)
    if math.isnan(t["loss"]):
        assert math.isnan(y["loss"])
    else:
        assert abs(y["loss"] - t["loss"]) <= R.loss_bound(y["loss"], t["loss"])
    for gy, gt in zip(y["grads"], t["grads"]):
        assert R.worst(gy, gt, R.grad_bound(gy, gt)) <= 1.0


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_mutant_misses_a_bound(mutant):
    name = R.MUTANTS[mutant]
    ref = R.reference(name)
    t, y = ref["truth"], ref["yard"]
    m = R.run(name, torch.float32, mutant=mutant)
    worst = 0.0
    if not math.isnan(t["loss"]):
        worst = abs(m["loss"] - t["loss"]) / max(R.loss_bound(y["loss"], t["loss"]), 1e-300)
    for gm, gy, gt in zip(m["grads"], y["grads"], t["grads"]):
        worst = max(worst, R.worst(gm, gt, R.grad_bound(gy, gt)))
    b = R.plane_bounds(name, 0)
    for k in ("p12", "p23", "loss_2"):
        worst = max(worst, R.worst(m["per"][0][k], t["per"][0][k], b[k]))
    assert worst > 1.0, worst


@pytest.mark.parametrize("shape", [(1, 3, 4, 4), (2, 3, 5, 9), (1, 2, 12, 17)])
def test_closed_form_ssim_gather_equals_autograd(shape):
    g = torch.Generator().manual_seed(7)
    x = torch.rand(shape, dtype=torch.float64, generator=g).requires_grad_(True)
    y = torch.rand(shape, dtype=torch.float64, generator=g)
    gd = torch.randn(shape, dtype=torch.float64, generator=g)
    dist, _ = R.ssim(x, y)
    (auto,) = torch.autograd.grad((dist * gd).sum(), x)
    closed = R.ssim_grad_closed_form(x.detach(), y, gd)
    assert float((auto - closed).abs().max()) <= 1e-9 * float(auto.abs().max())
