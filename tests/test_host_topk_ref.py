"""The top-k regression reference checks itself on the CPU (no device needed): the float64 truth of _topk_ref.py (stable sort,
closed-form gradients) equals torch's own float64 chain of the reference's lines, it reproduces what the reference itself
returned (tests/golden/topk.npz), torch's fp32 chain meets every bound on every fixed case, every mutant misses the bound on
the case named for it, and the cases that claim to be tie-free are."""
import os

import numpy as np
import pytest
import torch

import _topk_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "topk.npz")
KEYS = ("out", "gcost", "gsamples")


def _tensors(name):
    ref = R.reference(name)
    t = lambda v: None if v is None else torch.from_numpy(v)  # noqa: E731
    return ref, t(ref["cost"]), t(ref["samples"]), t(ref["gout"])


@pytest.mark.parametrize("name", list(R.CASES))
def test_truth_is_torchs_float64_chain(name):
    ref, cost, samples, gout = _tensors(name)
    chain = R.torch_chain(cost, samples, gout, R.CASES[name]["k"], torch.float64)
    for key in KEYS:
        want = ref["truth"][key]
        if want is None:
            assert chain[key] is None
            continue
        nan = torch.isnan(want)
        assert chain[key].shape == want.shape and torch.equal(torch.isnan(chain[key]), nan), (name, key)
        scale = max(1.0, float(want[~nan].abs().max()))
        assert float((chain[key] - want)[~nan].abs().max()) <= 1e-12 * scale, (name, key)


@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if not c.get("tie")])
def test_truth_reproduces_the_reference(name):
    """The stored fp32 results of the reference's own regression_topk (its unstable sort included) against the truth: the
    same planes, and values inside the bounds."""
    ref, k = R.reference(name), R.CASES[name]["k"]
    z = np.load(GOLDEN)
    truth, bound = ref["truth"], ref["bound"]
    ind = torch.from_numpy(z[name + "/ind"].astype(np.int64))
    assert torch.equal(ind, truth["idx"]), name
    assert float(z[name + "/rest"]) == 0.0
    assert R.worst(torch.from_numpy(z[name + "/out"]), truth["out"], bound["out"]) <= 1.0, name
    for key in ("gcost", "gsamples"):
        if truth[key] is None:
            assert name + "/" + key not in z.files
            continue
        got = torch.from_numpy(z[name + "/" + key])
        assert got.shape[1] == k
        assert R.worst(got, torch.gather(truth[key], 1, ind), torch.gather(bound[key], 1, ind)) <= 1.0, (name, key)


@pytest.mark.parametrize("name", list(R.CASES))
def test_torch_fp32_is_inside_every_bound(name):
    ref, cost, samples, gout = _tensors(name)
    chain = R.torch_chain(cost, samples, gout, R.CASES[name]["k"], torch.float32)
    for key in KEYS:
        if ref["truth"][key] is None:
            continue
        ratio = R.worst(chain[key], ref["truth"][key], ref["bound"][key])
        print("%-8s torch fp32: %-8s %.4f of the bound" % (name, key, ratio))
        assert ratio <= 1.0, (name, key, ratio)


@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_mutants_miss_the_bound(mutant):
    what, name = R.MUTANTS[mutant]
    ref, cost, samples, gout = _tensors(name)
    wide = torch.from_numpy(ref["wide_cost"]) if "wide_cost" in ref else None
    got = R.closed_form(cost, samples, gout, R.CASES[name]["k"], mutant, wide_cost=wide)
    ratio = R.worst(got[what], ref["truth"][what], ref["bound"][what])
    print("%-18s %-6s on %-8s %.3g of the bound" % (mutant, what, name, ratio))
    assert ratio > 1.0, (mutant, ratio)


@pytest.mark.parametrize("name", list(R.CASES))
def test_bounds_are_small_beside_the_results(name):
    """A bound can only catch what is larger than it: every bound is below 1e-4 of the largest magnitude of its result (the
    constants are at most 2 (|t| + T + 2K + 6) u, with |t| up to a few tens on these cases).  Not gcost on "d256": its planted
    maximum lies 28 above the runner-up, the true gradient p_1 (s - pred) is of the order 1e-10, below the rounding u 255 of pred
    that s_i - pred inherits in fp32 whatever the kernel."""
    ref = R.reference(name)
    for key in KEYS:
        want = ref["truth"][key]
        if want is None or (name, key) == ("d256", "gcost"):
            continue
        nan = torch.isnan(want)
        top = float(want[~nan].abs().max())
        assert float(ref["bound"][key][~nan].max()) <= 1e-4 * max(top, 1e-30) or top == 0.0, (name, key)


def test_tie_free_where_claimed():
    """Every case but "tie" has distinct k-th and (k+1)-th values in every column, so the reference's unstable sort has one
    answer; the tie case has none that is tie-free, and the stable sort keeps the planes its construction names."""
    for name, c in R.CASES.items():
        free = R.tie_free(torch.from_numpy(R.reference(name)["cost"]), c["k"])
        assert bool(free.all()) != bool(c.get("tie")), name
        if c.get("tie"):
            assert not bool(free.any())
    idx = R.reference("tie")["truth"]["idx"]
    pix = torch.arange(5 * 67).reshape(5, 67)
    even, odd = pix % 2 == 0, pix % 2 == 1
    assert bool((idx[:, 0][:, even] == 30).all()) and bool((idx[:, 1][:, even] == 7).all())
    assert bool((idx[:, 0][:, odd] == 5).all()) and bool((idx[:, 1][:, odd] == 12).all())


def test_special_values():
    """k = 1: the sample of the largest plane, and a zero gradient to cost; D = 1: plane 0; the NaN pixel is NaN, alone."""
    ref = R.reference("k1")
    assert torch.equal(ref["truth"]["out"][:, 0], torch.from_numpy(ref["cost"]).argmax(1).double())
    assert float(ref["truth"]["gcost"].abs().max()) == 0.0
    assert float(R.reference("d1")["truth"]["out"].abs().max()) == 0.0
    out = R.reference("nan")["truth"]["out"]
    b, _, y, x = R.NAN_AT
    assert bool(torch.isnan(out[b, 0, y, x])) and int(torch.isnan(out).sum()) == 1
    planted = R.reference("d256")["truth"]["idx"][:, 0]
    assert set(planted.unique().tolist()) == {0, 255}
