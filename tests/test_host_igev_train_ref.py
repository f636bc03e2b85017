"""The reference of the IGEV training-loop test on the CPU: how often an honest fp32 run of the loop is within G_BOUND of
the fp64 truth.  test_gpu_igev_train.py compares the node arm with the truth at the first draw at which the torch arm is
within G_BOUND; this file shows that such draws are not rare: the fp32 restatement (_igev_train_ref.train_forward on an
fp32 state dict) is within G_BOUND on every parameter at no fewer than three of the ten draws.  Prints every draw's worst
parameter (run with -s)."""
import pytest
import torch

import _igev_train_ref as R


def test_fp32_restatement_is_within_the_bound_at_three_draws_or_more():
    inside = []
    for seed in R.DRAWS:
        want, wp = R.truth((), seed)
        got, gp = R.fp32((), seed)
        name, e = R.worst(R.grad_error(got, want))
        pe = max(float((a.double() - b).abs().max() / b.abs().max()) for a, b in zip(gp, wp))
        print("draw %d: worst %s %.2e (G_BOUND %.0e), predictions %.2e" % (seed, name, e, R.G_BOUND, pe))
        if e <= R.G_BOUND:
            inside.append(seed)
    assert len(inside) >= 3, inside


@pytest.mark.parametrize("overrides", R.VARIANTS[1:], ids=lambda o: "+".join(sorted(o)))
def test_variants_have_a_draw_within_the_bound(overrides):
    case = R.key(overrides)
    errs = [R.worst(R.grad_error(R.fp32(case, seed)[0], R.truth(case, seed)[0]))[1] for seed in list(R.DRAWS)[:4]]
    print("%s: %s" % (overrides, ", ".join("%.2e" % e for e in errs)))
    assert min(errs) <= R.G_BOUND, errs


def test_truth_uses_every_parameter_and_every_prediction():
    """At three layers every parameter of the block and the head gets a finite, non-zero gradient."""
    want, preds = R.truth((), 0)
    assert len(preds) == R.ITERS and all(tuple(p.shape) == (1, 1, 4 * R.H, 4 * R.W) for p in preds)
    assert not [k for k, g in want.items() if g is None]
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in want.values())
