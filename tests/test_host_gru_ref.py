"""The reference module of the update operator's training nodes (_gru_ref.py) checked on the CPU: its closed-form gradients
are torch's float64 autograd of the reference's expression sequences, the reference's own fp32 arithmetic meets the bound
at every fixed case (so the bound asks of the kernels what the reference delivers), the two sweep figures of the function
budgets are reproduced, and the restated interpolation weights are ATen's."""
import numpy as np
import pytest
import torch

import _gru_ref as R

GATE_OUTPUTS = ("z", "rh", "gazr", "gh_zr", "hout", "gaq", "gz", "gh_out")


@pytest.fixture(scope="module")
def gates():
    """Per fixed case: inputs, float64 autograd, closed forms with the reference's budget."""
    out = {}
    for name, c in R.GATE_CASES.items():
        i = R.gate_inputs(c)
        out[name] = (i, R.autograd_gates(i, torch.float64), R.closed_gates(i, R.E_SIGMA_REF, R.E_T_REF))
    return out


@pytest.mark.parametrize("name", list(R.GATE_CASES))
def test_gate_closed_forms_are_float64_autograd(gates, name):
    """Within 2^-40 of the bound's magnitude: float64 autograd forms 1 - z by subtraction, the closed forms do not."""
    _, auto, (truth, cmag, _) = gates[name]
    for k in GATE_OUTPUTS:
        assert bool(((auto[k] - truth[k]).abs() <= 2.0 ** -40 * cmag[k] + R.FLOOR).all()), (name, k)
    ch = truth["z"].shape[1]
    assert torch.equal(auto["gcz"], auto["gazr"][:, :ch]) and torch.equal(auto["gcr"], auto["gazr"][:, ch:])
    assert torch.equal(auto["gcq"], auto["gaq"])


@pytest.mark.parametrize("name", list(R.GATE_CASES))
def test_gate_yardstick_meets_the_bound(gates, name):
    i, _, (truth, cmag, mag) = gates[name]
    y = R.autograd_gates(i, torch.float32)
    line = []
    for k in GATE_OUTPUTS:
        in_u, of_bound = R.worst(y[k], truth[k], cmag[k], mag[k])
        line.append("%s %.2f (%.2f)" % (k, in_u, of_bound))
        assert of_bound <= 1.0, (name, k, in_u, of_bound)
    print("%-8s u*mag (of the bound): " % name + ", ".join(line))


def test_saturated_cases_saturate():
    """The 'sat' cases reach exact 0 and 1 gates in fp32 and stay finite."""
    i = R.gate_inputs(R.GATE_CASES["mid_sat"])
    y = R.autograd_gates(i, torch.float32)
    assert bool((y["z"] == 0).any()) and bool((y["z"] == 1).any())
    assert bool((torch.from_numpy(i["z"]) == 0).any()) and bool((torch.from_numpy(i["z"]) == 1).any())
    assert all(bool(torch.isfinite(v).all()) for v in y.values())


@pytest.mark.parametrize("hw", R.POOL_CASES)
def test_pool_closed_form_and_yardstick(hw):
    H, W = hw
    x, gy = R.pool_inputs(H, W)
    gx, cmag, mag = R.closed_pool(gy, H, W)
    _, auto = R.autograd_pool(x, gy, torch.float64)
    assert bool(((auto - gx).abs() <= 2.0 ** -48 * mag).all())
    _, y32 = R.autograd_pool(x, gy, torch.float32)
    in_u, of_bound = R.worst(y32, gx, cmag, mag)
    print("pool %s: %.2f u*mag (%.2f of the bound)" % (hw, in_u, of_bound))
    assert of_bound <= 1.0


@pytest.mark.parametrize("case", R.INTERP_CASES)
def test_interp_closed_form_weights_and_yardstick(case):
    H, W, Ho, Wo, planes = case
    x, gy = R.interp_inputs(H, W, Ho, Wo, planes)
    # float64 weights: torch's float64 autograd
    gx64, _, mag64 = R.closed_interp(gy, H, W, dtype=np.float64)
    _, auto = R.autograd_interp(x, gy, torch.float64)
    assert bool(((auto - gx64).abs() <= 2.0 ** -44 * mag64).all())
    # fp32 weights: the ones F.interpolate applies in fp32, bit for bit, and its fp32 backward under the bound
    for N, No in ((H, Ho), (W, Wo)):
        assert R.same(R.interp_axis_matrix32(N, No), R.interp_axis_onehot(N, No)), (N, No)
    _, g32 = R.autograd_interp(x, gy, torch.float32)
    gx, cmag, mag = R.closed_interp(gy, H, W)
    in_u, of_bound = R.worst(g32, gx, cmag, mag)
    print("interp %s: %.2f u*mag (%.2f of the bound)" % (case, in_u, of_bound))
    assert of_bound <= 1.0


def test_sweep_figures():
    """torch's CPU sigmoid and tanh against float64 on linspace(-30, 30, 4 000 001): 2.46 and 0.57 ulp, 4.9 u and 1.2 u."""
    x = R.sweep_points()
    (s_ulp, s_u), (t_ulp, t_u) = R.sweep_error(x, torch.sigmoid(x), torch.tanh(x))
    print("sigmoid %.3f ulp %.3f u, tanh %.3f ulp %.3f u" % (s_ulp, s_u, t_ulp, t_u))
    assert abs(s_ulp - R.SIGMOID_CPU_ULP) < 0.01 and abs(t_ulp - R.TANH_CPU_ULP) < 0.01     # the two quoted digits
    assert s_u <= R.SIGMOID_CPU_U + 0.05 and t_u <= R.TANH_CPU_U + 0.05
    assert s_u <= R.E_SIGMA_REF and t_u <= R.E_T_REF


def test_device_budget_is_the_stated_rule():
    """E_SIGMA / E_T = max(twice the CPU figure, the measured device figure + one ulp), in u (1 ulp <= 2 u)."""
    assert R.E_SIGMA == max(2 * R.SIGMOID_CPU_U, 2 * (R.SIGMOID_DEVICE_ULP + 1.0))
    assert R.E_T == max(2 * R.TANH_CPU_U, 2 * (R.TANH_DEVICE_ULP + 1.0))
