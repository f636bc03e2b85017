"""The reference of the convex up-sampling tests, checked on the CPU before any kernel is held to it:
the closed-form gradient equals float64 autograd through the reference's expression sequence, and the reference's own
fp32 arithmetic (the same sequence under torch autograd in float32) stays inside the bound of _upsample_ref on every
fixed case.  Prints the fp32 sequence's worst error per case in units of u * mag (run with -s to see it)."""
import pytest
import torch

import _upsample_ref as R


def _tensors(c):
    flow, mask, gout, f, Dout = R.inputs(c)
    return flow, mask, gout, f, Dout, tuple(torch.from_numpy(x) for x in (flow, mask, gout))


@pytest.mark.parametrize("name", list(R.CASES))
def test_closed_form_is_the_autograd_gradient(name):
    flow, mask, gout, f, Dout, (tf, tm, tg) = _tensors(R.CASES[name])
    want = R.truth(flow, mask, gout, f, Dout)
    got = R.closed_form(tf, tm, tg, f, Dout)
    for what, a, b in zip(("out", "gflow", "gmask"), got, want):
        scale = float(b.abs().max())
        assert float((a - b).abs().max()) <= 1e-12 * max(scale, 1e-300), (name, what)
    assert bool((got[1][:, Dout:] == 0).all())


@pytest.mark.parametrize("name", list(R.CASES))
def test_fp32_sequence_meets_the_bound(name):
    flow, mask, gout, f, Dout, (tf, tm, tg) = _tensors(R.CASES[name])
    exact = dict(zip(("out", "gflow", "gmask"), R.closed_form(tf, tm, tg, f, Dout)))
    got = dict(zip(("out", "gflow", "gmask"), R.yardstick(flow, mask, gout, f, Dout)))
    mags = R.magnitudes(tf, tm, tg, f, Dout)
    c = R.constants(mags, f, Dout)
    line = []
    for what in ("out", "gflow", "gmask"):
        in_u, of_bound = R.worst(got[what], exact[what], mags[what], c[what])
        line.append("%s %.2f u*mag (%.3f of the bound)" % (what, in_u, of_bound))
        assert of_bound <= 1.0, (name, what, in_u, of_bound)
    print("%-9s largest R %.1f: " % (name, float(mags["R_mask"].max())) + ", ".join(line))
