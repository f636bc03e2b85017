"""The yardstick of the weight-gradient kernel checked on the CPU (no device): the emulation of its arithmetic and torch's
own fp32 weight gradient meet both bounds of _conv_wgrad_ref.py on every case at every magnitude, the emulation WITHOUT the
pre-pass exponent misses (a) at 2^-20, and a dropped tap, a dropped last column and a dropped slice each miss (b) -- the
bounds hold what is right and catch what is wrong.  Every case prints its figures (run with -s)."""
import functools

import pytest
import torch

import _conv_wgrad_ref as WR


@functools.lru_cache(maxsize=None)
def _ref(case):
    """x, g' (the upstream gradient itself: no ReLU on the CPU side), the fp64 truth and the bound (b) at k = 0, computed
    once: a power-of-two multiple of g' gives that multiple of both exactly."""
    x, _, _, gy = WR.inputs(case)
    k = case[3]
    return x, gy, WR.truth(x, gy, k), WR.b_bound(x, gy, k)


@pytest.mark.parametrize("case", WR.CASES, ids=WR.CASE_IDS)
def test_emulation_and_torch_fp32_meet_both_bounds(case):
    x, gp, exact, bound = _ref(case)
    k = case[3]
    for p in WR.KS:
        s = 2.0 ** p
        for name, got in (("emulation", WR.emulate(x, gp * s, k)), ("torch fp32", WR._cw(x, gp * s, k))):
            ea = WR.a_error(got, exact * s)
            ok, rb = WR.b_ratio(got, exact * s, bound * s)
            print("case %s k=%d %s: (a) %.2e  (b) |d|/bound %.2e" % (case, p, name, ea, rb))
            assert ea <= WR.A_BOUND, (name, p, ea)
            assert ok, (name, p, rb)


@pytest.mark.parametrize("case", WR.CASES, ids=WR.CASE_IDS)
def test_unit_scale_misses_a_at_a_small_gradient(case):
    x, gp, exact, _ = _ref(case)
    s = 2.0 ** -20
    ea = WR.a_error(WR.emulate(x, gp * s, case[3], e=0), exact * s)
    print("case %s: unit scale at 2^-20: (a) %.2e" % (case, ea))
    assert ea > WR.A_BOUND


@pytest.mark.parametrize("case", WR.CASES, ids=WR.CASE_IDS)
def test_a_dropped_tap_column_or_slice_misses_b(case):
    x, gp, exact, bound = _ref(case)
    B, H, W, k, cin, cout = case
    good = WR.emulate(x, gp, k)
    tap = good.clone()
    tap[:, :, k - 1, k - 1] = 0.0                              # the last tap never accumulated
    xc = x.clone()
    xc[:, :, :, W - 1] = 0.0                                   # the last pixel column of x never staged
    rows, bands, _, _ = WR.plan(case)
    gs = gp.clone()
    gs[B - 1, :, (bands - 1) * rows:] = 0.0                    # the last slice never added
    for name, got in (("tap", tap), ("column", WR.emulate(xc, gp, k)), ("slice", WR.emulate(x, gs, k))):
        ok, rb = WR.b_ratio(got, exact, bound)
        print("case %s dropped %s: (b) |d|/bound %.2e" % (case, name, rb))
        assert not ok, name


def test_the_cases_cover_slices_and_blocks():
    """Under the kernel's plan: at least three slices of one weight, two output-channel and two input-channel blocks."""
    plans = {c: WR.plan(c) for c in WR.CASES}
    assert max(c[0] * p[1] for c, p in plans.items()) >= 3
    assert max(p[2] for p in plans.values()) >= 2 and max(p[3] for p in plans.values()) >= 2
    assert all(c[0] * c[1] * c[2] <= 2304 for c in WR.CASES)
