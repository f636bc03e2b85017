"""The yardstick of the 7x7 weight-gradient kernel checked on the CPU (no device): the emulation of its arithmetic and torch's
own fp32 weight gradient meet both bounds of _conv_wgrad_ref.py on every fixed case of _conv_wgrad7_ref.py at 2^0, 2^-20,
2^-40 and 2^+20, and bound (a) on the plan cases; the emulation WITHOUT the pre-pass exponent misses (a) at 2^-20; a zeroed
tap (0, 6) and a dropped last column miss (b) on the fixed cases, a lost 2 x 32 tile and a lost last slice miss (a) on the
plan cases; the plan's regimes are what the restated rule gives.  Every case prints its figures (run with -s).

Measured with these draws: fixed cases (a) <= 6.8e-7 (emulation) / 6.7e-7 (torch fp32), (b) ratio 0.15 / 0.058 on 1x1x1 and
<= 0.025 / 0.018 elsewhere; the walked plan case (a) 2.6e-6 / 3.0e-6 -- the reference's own sequential fp32 sum over
n = 134 400 pixels, inside 5e-6 but not by much: the case must not grow."""
import functools

import pytest
import torch

import _conv_wgrad7_ref as W7


@functools.lru_cache(maxsize=None)
def _ref(case):
    """x, g', the fp64 truth and the bound (b) at 2^0, computed once: a power-of-two multiple of g' gives that multiple of
    both exactly."""
    x, gp = W7.inputs(case)[:2]
    return x, gp, W7.truth(x, gp), W7.b_bound(x, gp)


def _figures(what, got, exact, bound):
    ea = W7.WR.a_error(got, exact)
    ok, rb = W7.WR.b_ratio(got, exact, bound)
    print("%s: (a) %.2e  (b) |d|/bound %.2e" % (what, ea, rb))
    return ea, ok, rb


@pytest.mark.parametrize("case", W7.CASES, ids=W7.CASE_IDS)
def test_emulation_and_torch_fp32_meet_both_bounds(case):
    x, gp, exact, bound = _ref(case)
    for p in W7.KS:
        s = 2.0 ** p
        for name, got in (("emulation", W7.emulate(x, gp * s)), ("torch fp32", W7.torch_fp32(x, gp * s))):
            ea, ok, rb = _figures("case %s k=%d %s" % (case, p, name), got, exact * s, bound * s)
            assert ea <= W7.A_BOUND, (name, p, ea)
            assert ok, (name, p, rb)


@pytest.mark.parametrize("case", W7.PLAN_CASES, ids=W7.PLAN_IDS)
def test_emulation_and_torch_fp32_meet_a_on_the_plan_cases(case):
    x, gp, exact, bound = _ref(case)
    for p in (0, -20):
        s = 2.0 ** p
        for name, got in (("emulation", W7.emulate(x, gp * s)), ("torch fp32", W7.torch_fp32(x, gp * s))):
            ea, _, _ = _figures("plan case %s k=%d %s" % (case, p, name), got, exact * s, bound * s)
            assert ea <= W7.A_BOUND, (name, p, ea)


@pytest.mark.parametrize("case", W7.CASES, ids=W7.CASE_IDS)
def test_unit_scale_misses_a_at_a_small_gradient(case):
    x, gp, exact, _ = _ref(case)
    s = 2.0 ** -20
    ea = W7.WR.a_error(W7.emulate(x, gp * s, e=0), exact * s)
    print("case %s: unit scale at 2^-20: (a) %.2e" % (case, ea))
    assert ea > W7.A_BOUND


@pytest.mark.parametrize("case", [c for c in W7.CASES if c != W7.CENTRE_ONLY],
                         ids=[i for c, i in zip(W7.CASES, W7.CASE_IDS) if c != W7.CENTRE_ONLY])
def test_a_zeroed_tap_or_a_dropped_column_misses_b(case):
    x, gp, exact, bound = _ref(case)
    for name, got in (("tap (0, 6)", W7.zeroed_tap(W7.emulate(x, gp))),
                      ("last column", W7.emulate(W7.without_last_column(x), gp))):
        _, ok, rb = _figures("case %s dropped %s" % (case, name), got, exact, bound)
        assert not ok, (name, rb)


def test_the_centre_only_case_has_one_tap():
    """1x1x1: the truth is zero off the centre tap (so tap (0, 6) is 0 there anyway), and so is the emulation, exactly; the
    centre tap of a channel the mask left is not."""
    x, gp, exact, _ = _ref(W7.CENTRE_ONLY)
    off = torch.ones(7, 7, dtype=torch.bool)
    off[3, 3] = False
    assert not exact[:, :, off].any() and bool(exact[:, :, 3, 3].any())
    assert not W7.emulate(x, gp)[:, :, off].any()


@pytest.mark.parametrize("case", W7.PLAN_CASES, ids=W7.PLAN_IDS)
def test_a_lost_tile_or_slice_misses_a_on_the_plan_cases(case):
    x, gp, exact, _ = _ref(case)
    faults = [("a 2 x 32 tile", W7.without_tile(case, gp))]
    if W7.regime(case)["slices"] > 1:
        faults.append(("the last slice", W7.without_last_slice(case, gp)))
    for name, g1 in faults:
        ea = W7.WR.a_error(W7.emulate(x, g1), exact)
        print("plan case %s lost %s: (a) %.2e" % (case, name, ea))
        assert ea > W7.A_BOUND, (name, ea)


def test_plan_regimes():
    """The regimes the cases are named for, from the restated rule."""
    assert all(W7.plan_T(c)[4] == 1 and c[3] <= W7.MAX_CIN for c in W7.CASES + W7.PLAN_CASES)
    fixed = {c: W7.regime(c) for c in W7.CASES}
    assert all(r["T"] == 512 and r["items"] <= 6 for r in fixed.values())
    assert fixed[(3, 7, 9, 1, 64)]["slices"] == 3
    assert fixed[(2, 24, 40, 3, 64)]["bands"] == 2 and fixed[(2, 24, 40, 3, 64)]["slices"] == 4
    assert fixed[(1, 5, 70, 2, 64)]["tiles_w"] == 3
    assert W7.plan_T((2, 8, 12, 4, 70))[3] == 2 and W7.plan_T((1, 12, 33, 3, 130))[3] == 3
    assert all(c[0] * c[1] * c[2] <= 2304 for c in W7.CASES)
    w = W7.regime(W7.WALKED)
    assert (w["T"], w["band"], w["bands"], w["items"], w["slices"]) == (512, 8, 88, 264, 264)
    assert w["items"] > W7.WR.CUS and w["items"] - W7.WR.CUS == 8        # eight blocks take a second item
    assert w["tiles"][-1] == 4 and w["tiles"][0] == 8                    # the last band is 4 rows (700 = 87 * 8 + 4)
    lr = W7.regime(W7.LONG_ROW)
    assert (lr["items"], lr["slices"], lr["tiles_w"], lr["tiles"]) == (1, 1, 257, [257])
    ms = W7.regime(W7.MANY_SLICES)
    assert (ms["band"], ms["bands"], ms["slices"], ms["items"]) == (12, 2, 14, 14)
    # the two crop shapes of tools/bench_encoder_train.py: 2-row bands, a workspace of about a tenth of g'
    for case in ((4, 480, 896, 3, 64), (16, 320, 720, 3, 64)):
        B, H, W, cin, cout = case
        assert W7.regime(case)["band"] == 2
        assert 0.05 < W7.ws_floats(case) / (B * cout * H * W) < 0.15
