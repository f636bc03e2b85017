"""The soft-argmin reference checks itself on the CPU (no device needed): the float64 truth of _soft_argmin_ref.py (built
from the restated taps) equals torch's own float64 chain, the closed-form gradient equals float64 autograd, torch's fp32
chain meets both bounds on every fixed case, and every mutant misses the bound on the case named for it."""
import pytest
import torch

import _soft_argmin_ref as R


def _tensors(name):
    ref = R.reference(name)
    return ref, torch.from_numpy(ref["cost"]), torch.from_numpy(ref["gout"])


@pytest.mark.parametrize("name", list(R.CASES))
def test_truth_is_torchs_float64_chain(name):
    ref, cost, gout = _tensors(name)
    out, gcost = R.torch_chain(cost, gout, R.CASES[name]["f"], 1.0, torch.float64)
    assert out.shape == ref["out"].shape and gcost.shape == ref["gcost"].shape
    assert float((out - ref["out"]).abs().max()) <= 1e-12, name
    assert float((gcost - ref["gcost"]).abs().max()) <= 1e-12, name


def test_restated_taps_at_factor_4():
    """The four phases and the clamps as the header states them."""
    i0, i1, lam = R.taps(3, 4)
    assert i0.tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2]
    assert i1.tolist() == [1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2]
    assert lam.tolist() == [0.0, 0.0, 0.125, 0.375, 0.625, 0.875, 0.125, 0.375, 0.625, 0.875, 0.125, 0.375]
    i0, i1, lam = R.taps(5, 1)
    assert i0.tolist() == [0, 1, 2, 3, 4] and lam.tolist() == [0.0] * 5


@pytest.mark.parametrize("name", list(R.CASES))
def test_torch_fp32_is_inside_both_bounds(name):
    ref, cost, gout = _tensors(name)
    out, gcost = R.torch_chain(cost, gout, R.CASES[name]["f"], 1.0, torch.float32)
    ro, rg = R.worst(out, ref["out"], ref["bound_out"]), R.worst(gcost, ref["gcost"], ref["bound_gcost"])
    print("%-8s torch fp32: out %.4f of the bound, gcost %.4f of the bound" % (name, ro, rg))
    assert ro <= 1.0 and rg <= 1.0, (name, ro, rg)


def test_special_values():
    """Dc = 1: E = (D - 1)/2 and a zero gradient; out_scale = -1 negates both."""
    ref = R.reference("dc1")
    assert bool((ref["out"] == 1.5).all()) and float(ref["gcost"].abs().max()) <= 1e-15
    pos, neg = R.reference("tiles"), R.reference("tiles", -1.0)
    assert torch.equal(pos["out"], -neg["out"]) and torch.equal(pos["gcost"], -neg["gcost"])
    assert torch.equal(pos["bound_out"], neg["bound_out"]) and torch.equal(pos["bound_gcost"], neg["bound_gcost"])


@pytest.mark.parametrize("name", list(R.CASES))
def test_bounds_are_small_beside_the_results(name):
    """A bound can only catch what is larger than it.  Where the gradient is not identically 0 the largest gradient bound is
    below (1e-3 + 5e-5 M) of the largest gradient -- the logits are known to about 8 eps M, and the softmax turns that into a
    relative error of the gradient, so the share a bound can reach grows with M = max|cost| (0.15 at the 1e4 offset, 0.09 at
    the spike, at most 1.3e-3 elsewhere); every forward bound is below its envelope bound_fwd."""
    ref, c = R.reference(name), R.CASES[name]
    D, M = c["f"] * c["Dc"], float(abs(ref["cost"]).max())
    assert float(ref["bound_out"].max()) <= R.bound_fwd(D, M) * (1 + 1e-12)
    gmax = float(ref["gcost"].abs().max())
    share = float(ref["bound_gcost"].max()) / gmax if gmax > 1e-12 else 0.0
    print("%-8s bound_out <= %.3e, bound_gcost <= %.3e = %.2e of max|gcost|" % (name, float(ref["bound_out"].max()), float(ref["bound_gcost"].max()), share))
    assert share <= 1e-3 + 5e-5 * M, name


@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_mutants_miss_the_bound(mutant):
    what, name = R.MUTANTS[mutant]
    ref, cost, gout = _tensors(name)
    got = dict(zip(("out", "gcost"), R.closed_form(cost, gout, R.CASES[name]["f"], 1.0, mutant)))
    ratio = R.worst(got[what], ref[what], ref["bound_" + what])
    print("%-14s %-6s on %-7s %.3g of the bound" % (mutant, what, name, ratio))
    assert ratio > 1.0, (mutant, ratio)


def test_spike_needs_the_fine_maximum():
    """On the spike case torch's fp32 and fp64 chains stay finite, while a shift by the coarse maximum leaves most pixels
    without a single term (zero sums: not a number)."""
    ref, cost, gout = _tensors("spike")
    for dtype in (torch.float32, torch.float64):
        out, gcost = R.torch_chain(cost, gout, 4, 1.0, dtype)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gcost).all())
    out, _ = R.closed_form(cost, gout, 4, 1.0, "coarse_max")
    assert int((~torch.isfinite(out)).sum()) > out.numel() // 2
