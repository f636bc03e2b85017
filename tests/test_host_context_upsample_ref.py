"""The reference of the context up-sampling tests, checked on the CPU before any kernel is held to it: the closed forms
equal float64 autograd through the reference's expression sequence, the reference's own fp32 arithmetic (the same sequence
under torch autograd in float32) stays inside every bound of _context_upsample_ref on every fixed case, and every mutant
misses the bound it names.  Prints the fp32 sequence's worst error per case in units of u * mag (run with -s)."""
import functools

import pytest
import torch

import _context_upsample_ref as R

KEYS = ("out", "gdisp", "gnine")


@functools.lru_cache(maxsize=None)
def _ref(name, logits):
    """numpy inputs, torch inputs, closed form, magnitudes and constants of one case and form, computed once."""
    disp, lg, gout = R.inputs(R.CASES[name])
    nine = lg if logits else R.weights_of(lg)
    t = tuple(torch.from_numpy(x) for x in (disp, nine, gout))
    mags = R.magnitudes(*t, logits)
    return (disp, nine, gout), t, dict(zip(KEYS, R.closed_form(*t, logits))), mags, R.constants(mags, logits)


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("name", list(R.CASES))
def test_closed_form_is_the_autograd_gradient(name, logits):
    arrays, _, exact, _, _ = _ref(name, logits)
    for what, b in zip(KEYS, R.truth(*arrays, logits)):
        a = exact[what]
        assert a.shape == b.shape
        assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-300), (name, what)


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("name", list(R.CASES))
def test_fp32_sequence_meets_the_bounds(name, logits):
    arrays, _, exact, mags, c = _ref(name, logits)
    got = dict(zip(KEYS, R.yardstick(*arrays, logits)))
    line = []
    for what in KEYS:
        if c[what] is None:
            continue
        in_u, of_bound = R.worst(got[what], exact[what], mags[what], c[what])
        line.append("%s %.2f u*mag (%.3f of the bound)" % (what, in_u, of_bound))
        assert of_bound <= 1.0, (name, what, in_u, of_bound)
    if not logits:
        assert R.same(got["gnine"], R.fp32_product(arrays[0], arrays[2])), name        # one rounding: the same bits
    print("%-9s %-7s " % (name, "logits" if logits else "weights") + ", ".join(line))


@pytest.mark.parametrize("name", R.MUTANT_CASES)
@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_mutants_miss_their_bound(mutant, name):
    what = R.MUTANTS[mutant]
    _, t, exact, mags, c = _ref(name, True)
    wrong = dict(zip(KEYS, R.closed_form(*t, True, mutant=mutant)))[what]
    assert R.worst(wrong, exact[what], mags[what], c[what])[1] > 1.0, (mutant, name)
    if mutant == "skip_sub33":                                                          # the weights form has this one too
        _, t, exact, mags, c = _ref(name, False)
        wrong = R.closed_form(*t, False, mutant=mutant)[1]
        assert R.worst(wrong, exact["gdisp"], mags["gdisp"], c["gdisp"])[1] > 1.0, (mutant, name)
