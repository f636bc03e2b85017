"""The optimizer step's reference (tests/_optim_ref.py) without a device: torch.optim.AdamW in fp32 and the emulation of
dkt_adamw_step's rounding sequence meet the derived bound on every case, every mutant misses it, a step with an inf or a nan
gradient changes nothing, and the fp64 truth is torch.optim.AdamW's formula."""
import pytest
import torch

import _optim_ref as O


def _run(fn, name, **kw):
    p, g, m, v, c = O.state(name)
    got = fn([t.clone() for t in p], g, [t.clone() for t in m], [t.clone() for t in v], c, **kw)
    return O.excess(got, O.truth(p, g, m, v, c), p, m, v, c["step"]), got


@pytest.mark.parametrize("name", sorted(O.CASES))
def test_torch_adamw_fp32_meets_bound(name):
    p, g, m, v, c = O.state(name)
    got = O.torch_step(p, g, m, v, c)
    tn, got["total_norm"] = got["total_norm"], None      # (clip_grad_norm_ adds its squares in fp32: printed, not held to N_NORM)
    t = O.truth(p, g, m, v, c)
    x = O.excess(got, t, p, m, v, c["step"])
    print("%s: torch.optim.AdamW fp32 at %.3g of the bound; its total_norm %r, truth %.9g" % (name, x, tn, t["total_norm"]))
    assert x <= 1.0


@pytest.mark.parametrize("name", sorted(O.CASES))
def test_emulation_meets_bound(name):
    x, got = _run(O.emulate, name)
    print("%s: emulation at %.3g of the bound (total_norm %r, clip %r, skipped %d)" % (name, x, got["total_norm"], got["clip"], got["skipped"]))
    assert x <= 1.0


@pytest.mark.parametrize("mutant", O.MUTANTS)
def test_mutant_misses_bound(mutant):
    xs = {name: _run(O.emulate, name, mutant=mutant)[0] for name in O.CASES}
    caught = sorted(k for k, x in xs.items() if x > 1.0)
    print("%s: outside the bound on %s (worst %.3g x)" % (mutant, caught, max(xs.values())))
    assert caught


@pytest.mark.parametrize("name", O.POISONED)
def test_non_finite_gradient_changes_nothing(name):
    p, g, m, v, c = O.state(name)
    got = O.emulate(p, g, m, v, c)
    assert got["skipped"] == 1 and got["step"] == c["step"]
    for a, b in zip(got["p"] + got["m"] + got["v"], p + m + v):
        assert torch.equal(a, b)
    t = O.truth(p, g, m, v, c)
    assert t["skipped"] == 1 and t["step"] == c["step"]


@pytest.mark.parametrize("name", O.FINITE)
def test_truth_is_torch_adamw_in_fp64(name):
    """The restated formula is torch's: torch.optim.AdamW in fp64 on the truth's own g * inv_scale * clip."""
    p, g, m, v, c = O.state(name)
    t = O.truth(p, g, m, v, c)
    want = O.torch_step(p, g, m, v, c, dtype=torch.float64, clip=t["clip"])
    worst = 0.0
    for key in "pmv":
        for a, b in zip(t[key], want[key]):
            if b.numel():
                worst = max(worst, float((a - b).abs().max() / b.abs().max()))
    print("%s: truth vs torch.optim.AdamW in fp64: %.3g relative" % (name, worst))
    assert worst <= 1e-15 and t["step"] == want["step"]


@pytest.mark.parametrize("name", [k for k in O.FINITE if O.CASES[k]["max_norm"] is not None])
def test_truth_norm_is_clip_grad_norm_in_fp64(name):
    """total_norm against clip_grad_norm_ in fp64.  torch adds the n = 115217 squares of a tensor list one after another in
    fp64 where the truth's sum is pairwise, so the two may differ by torch's own accumulation error, at most n * 2^-53 =
    1.3e-11 relative (about sqrt(n) * 2^-53 = 4e-14 is typical)."""
    p, g, m, v, c = O.state(name)
    t = O.truth(p, g, m, v, c)
    want = O.torch_step(p, g, m, v, c, dtype=torch.float64)["total_norm"]
    rel = abs(t["total_norm"] - want) / want
    print("%s: total_norm %.17g, clip_grad_norm_ in fp64 %.17g: %.3g relative" % (name, t["total_norm"], want, rel))
    assert rel <= sum(O.SIZES) * 2.0 ** -53
