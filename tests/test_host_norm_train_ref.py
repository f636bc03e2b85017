"""The yardstick of the instance-norm training nodes, checked on the CPU before any kernel is held to it: the emulation of
the kernels' arithmetic (_norm_train_ref.emulate: fp64 plane sums in slices, fp32 element-wise) meets the derived bound on
every fixed case, for the norm with and without ReLU and for the join; each way of getting the backward wrong -- no
`mean g` term, no `yh mean(g yh)` term, sums over the unmasked gradient, one slice's partial sum lost -- misses it; and
both reduction terms are large in every non-degenerate case.  torch's own fp32 CPU backward accumulates the plane sums in
fp32 and does NOT meet this bound; its ratio is printed for the record (run with -s)."""
import pytest
import torch

import _norm_train_ref as R

MODES = ("norm", "norm_relu", "join")


def _setup(name, mode):
    """(upstream gradient, normalised tensor, saved statistics, mask or None)."""
    x, gy, a = R.inputs(R.CASES[name])
    mi = R.saved_stats(x)
    if mode == "norm":
        return gy, x, mi, None
    yh_pos = R.yhat32(x, mi) > 0
    if mode == "norm_relu":
        return gy, x, mi, yh_pos
    return gy, x, mi, (R.forward_join(a, x, mi) > 0) & yh_pos


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(R.CASES))
def test_emulation_meets_the_bound(name, mode):
    gup, x, mi, mask = _setup(name, mode)
    exact, bound, rg, rgy = R.truth_and_bound(gup, x, mask)
    ratio = R.worst(R.emulate(gup, x, mi, mask), exact, bound)
    line = "%-14s %-9s emulation %.3f of the bound" % (name, mode, ratio)
    if mode != "join" and x[0, 0].numel() > 1:
        line += ", torch fp32 %.3g" % R.worst(R.torch_norm_grad(gup, x, mode == "norm_relu"), exact, bound)
    print(line)
    assert ratio <= 1.0, (name, mode, ratio)
    if name not in R.DEGENERATE:
        assert rg >= 0.1 and rgy >= 0.1, (name, mode, rg, rgy)


def test_constant_plane():
    """Variance 0: yh is 0 exactly, so with ReLU the gradient is 0 exactly; without, r = 1 / sqrt(eps)."""
    gup, x, mi, _ = _setup("constant", "norm")
    assert float(R.yhat32(x, mi).abs().max()) == 0.0
    assert abs(float(mi[0, 1]) - R.EPS ** -0.5) <= 4 * R.U * R.EPS ** -0.5
    assert float(R.emulate(gup, x, mi, R.yhat32(x, mi) > 0).abs().max()) == 0.0
    assert float(R.emulate(gup, x, mi, None).abs().max()) > 100.0


@pytest.mark.parametrize("mutation", ["no_mean_g", "no_proj", "unmasked_sums", "drop_slice"])
def test_a_wrong_backward_misses_the_bound(mutation):
    modes = ("norm_relu", "join") if mutation == "unmasked_sums" else MODES
    names = R.SPLIT_CASES if mutation == "drop_slice" else [n for n in R.CASES if n not in R.DEGENERATE]
    ratios = {}
    for name in names:
        for mode in modes:
            gup, x, mi, mask = _setup(name, mode)
            exact, bound, _, _ = R.truth_and_bound(gup, x, mask)
            ratios[(name, mode)] = R.worst(R.emulate(gup, x, mi, mask, mutate=mutation), exact, bound)
    print("%s: smallest miss %.3g x the bound" % (mutation, min(ratios.values())))
    assert min(ratios.values()) > 100.0, (mutation, ratios)


def test_split_cases_take_several_slices():
    for name in R.CASES:
        n, c, h, w = R.CASES[name]["shape"]
        assert (R.split(n * c, h * w) > 1) == (name in R.SPLIT_CASES), name
    HW = 100 * 97
    sl = R.slices(HW, R.split(2, HW))
    assert len(sl) == 3 and sl[-1][1] == HW and sl[-1][1] - sl[-1][0] < sl[0][1] - sl[0][0]      # a partial last slice
    assert HW % 4 == 0 and all(lo % 4 == 0 for lo, _ in sl)
