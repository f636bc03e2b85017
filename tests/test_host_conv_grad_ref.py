"""The reference of the convolution backward tests (tests/_conv_grad_ref.py) checked on the host: torch's own fp32 arithmetic
meets its bounds, the emulated split-fp16 convolution meets the gx bound at every gradient magnitude WITH the pre-pass's
exponent and misses it at 2^-20 without -- the inputs discriminate -- and the exponent rule's edge values."""
import math

import pytest
import torch
import torch.nn.functional as F

import _conv_grad_ref as R


def _saved_output(case):
    x, w, b, _ = R.inputs(case)
    return torch.relu(F.conv2d(x, w, b, padding=w.shape[2] // 2))


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_torch_fp32_meets_the_bounds(case):
    x, w, b, gy0 = R.inputs(case)
    y = _saved_output(case)
    for k in R.KS:
        gy = gy0 * 2.0 ** k
        gp, gb, gx = R.truth(gy, y, w)
        got_gx = F.conv2d(gp, R.transposed(w), padding=w.shape[2] // 2)
        got_gb = gp.sum(dim=(0, 2, 3))
        err = R.gx_error(got_gx, gx)
        print("case %s k=%d: gx rel %.2e  gb max|d|/bound %.2e" % (case, k, err, float(((got_gb.double() - gb).abs() / R.gb_bound(gp).clamp_min(1e-300)).max())))
        assert err <= R.GX_BOUND
        assert bool(((got_gb.double() - gb).abs() <= R.gb_bound(gp)).all())


def test_gb_bound_sees_a_dropped_term():
    """n <= 2304 in every case: one term left out of the sum exceeds the bound on average (sum|g'| / n > gamma * sum|g'|)."""
    for case in R.CASES:
        n = case[0] * case[1] * case[2]
        assert n <= 2304
        m = (n - 1) * R.U
        assert n == 1 or m / (1 - m) < 1.0 / n


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_emulated_split_with_the_rule_meets_the_bound(case):
    x, w, b, gy0 = R.inputs(case)
    y = _saved_output(case)
    for k in R.KS:
        gp, _, gx = R.truth(gy0 * 2.0 ** k, y, w)
        s = 2.0 ** R.exponent(float(gp.abs().max()))
        err = R.gx_error(R.split_conv(gp, w, s), gx)
        print("case %s k=%d: emulated split, in_scale 2^%d: gx rel %.2e" % (case, k, round(math.log2(s)), err))
        assert err <= R.GX_BOUND


@pytest.mark.parametrize("case", [c for c in R.CASES if c[0] * c[1] * c[2] > 1], ids=[i for c, i in zip(R.CASES, R.CASE_IDS) if c[0] * c[1] * c[2] > 1])
def test_emulated_split_at_unit_scale_misses_small_and_large_gradients(case):
    """in_scale = 1 (the backward before the pre-pass): fine at O(1), beyond the bound at 2^-20, non-finite at 2^+20."""
    x, w, b, gy0 = R.inputs(case)
    y = _saved_output(case)
    gp, _, gx = R.truth(gy0, y, w)
    assert R.gx_error(R.split_conv(gp, w, 1.0), gx) <= R.GX_BOUND
    gp, _, gx = R.truth(gy0 * 2.0 ** -20, y, w)
    err = R.gx_error(R.split_conv(gp, w, 1.0), gx)
    print("case %s k=-20 at in_scale 1: gx rel %.2e" % (case, err))
    assert err > R.GX_BOUND
    gp, _, gx = R.truth(gy0 * 2.0 ** 20, y, w)
    assert not bool(torch.isfinite(R.split_conv(gp, w, 1.0)).all())


def test_exponent_rule_edges():
    assert R.exponent(1.0) == 12 and R.exponent(4096.0) == 0 and R.exponent(8192.0) == -1      # powers of two open a binade
    assert R.exponent(math.nextafter(8192.0, 0.0)) == 0 and R.exponent(math.nextafter(1.0, 0.0)) == 13
    for amax in (1.0, 3.7e-9, 0.75, 6.0e4, 2.0 ** -60, 1.9 * 2.0 ** 30):
        assert 4096.0 <= amax * 2.0 ** R.exponent(amax) < 8192.0
    assert R.exponent(0.0) == 0 and R.exponent(float("inf")) == 0 and R.exponent(float("nan")) == 0
    assert R.exponent(2.0 ** -100) == R.MAX_EXP and R.exponent(1e-45) == R.MAX_EXP             # the clamp (a subnormal too)
    assert R.exponent(2.0 ** 120) == -R.MAX_EXP
    lo, hi = R.scale_pair(2.0 ** -100).tolist()
    assert lo == 2.0 ** 80 and hi == 2.0 ** -80                                                # both normal fp32 values
    assert R.scale_pair(0.0).tolist() == [1.0, 1.0]
    tiny = torch.finfo(torch.float32).tiny
    for e in (-R.MAX_EXP, R.MAX_EXP):
        # out_scale = weight inverse scale * 2^-e stays normal for any weight scale in [2^-46, 2^46]
        assert tiny <= 2.0 ** -46 * 2.0 ** -abs(e) and 2.0 ** 46 * 2.0 ** abs(e) < torch.finfo(torch.float32).max
