"""The PCVNet training reference checks itself on the CPU (no device needed): the torch restatement of the block reproduces what
the reference itself returned under autograd (tests/golden/pcv_train.npz); the numpy fp32 restatement of dkt_tap, through
lookup32, equals the C oracle's lookup bit for bit; the float64 closed form equals torch's own float64 autograd where the
floors are not in question; torch's fp32 autograd meets every bound of _pcv_train_ref.py on every case -- on the planted ones
because the truth is evaluated on the fp32 floors, which the float64 floors miss by orders of magnitude; every mutant misses
the bound on the case named for it; and the loop case keeps its taps away from the integers."""
import os

import numpy as np
import pytest
import torch

import _pcv_train_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pcv_train.npz")
INPUTS = ("fmap1", "fmap2", "coords", "sigma", "gout")
KEYS = ("out", "gf1", "gf2", "gcoords", "gsigma")


def _inputs(name):
    ref = R.reference(name)
    return {k: ref[k] for k in INPUTS}


def _levels32(name):
    """The case's pyramid rounded to fp32: the given level values of the lookup's own tests."""
    ref, c = R.reference(name), R.CASES[name]
    pyr = R.pyramid(torch.from_numpy(ref["fmap1"]).double(), torch.from_numpy(ref["fmap2"]).double(), c["L"], R.factor_of(c))
    return [p.float().numpy() for p in pyr]


@pytest.mark.parametrize("name", R.GOLDEN_CASES)
def test_restatement_reproduces_the_reference(name):
    """The stored inputs are the regenerated ones; the reference's fp32 results lie inside the bounds of the truth, and the
    restated block's fp32 results are the reference's to within the same bounds (the same operations: the same bits wherever
    the two ran on one build of torch)."""
    z = np.load(GOLDEN)
    ref, c = R.reference(name), R.CASES[name]
    for k in INPUTS:
        assert np.array_equal(z["%s/%s" % (name, k)], ref[k]), k
    mine = R.torch_chain(_inputs(name), c, torch.float32)
    truth = ref["truth"]
    for k in KEYS:
        stored = torch.from_numpy(z["%s/%s" % (name, k)])
        ratio = R.worst(stored, truth[k], truth["bound"][k])
        print("%-4s reference fp32: %-8s %.4f of the bound" % (name, k, ratio))
        assert ratio <= 1.0, (name, k, ratio)
        assert R.worst(mine[k], stored.double(), truth["bound"][k]) <= 1.0, (name, k)


@pytest.mark.parametrize("name", list(R.CASES))
def test_floor_restatement_is_the_c_oracles_lookup(name, c_oracle):
    ref, c = R.reference(name), R.CASES[name]
    lv = _levels32(name)
    mine = R.lookup32(lv, ref["coords"], ref["sigma"], c["S"], R.factor_of(c))
    want = c_oracle.pcv_lookup(lv, ref["coords"], ref["sigma"], c["S"], R.factor_of(c))
    assert mine.dtype == want.dtype == np.float32 and np.array_equal(mine.view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("name", R.UNPLANTED)
def test_closed_form_is_torchs_float64_autograd(name):
    """Without planted integers the float64 floors are the fp32 ones, and the closed form is what autograd derives."""
    ref, c = R.reference(name), R.CASES[name]
    own = R.truth(_inputs(name), c)
    chain = R.torch_chain(_inputs(name), c, torch.float64)
    for k in KEYS:
        assert torch.equal(own[k], ref["truth"][k]), (name, k)                  # same floors, same truth
        scale = max(1.0, float(own[k].abs().max()))
        assert float((chain[k] - own[k].reshape(chain[k].shape)).abs().max()) <= 1e-11 * scale, (name, k)


@pytest.mark.parametrize("name", list(R.CASES))
def test_torch_fp32_is_inside_every_bound(name):
    """The whole block from the maps, the lookup alone on given levels and the pool chain alone on given level gradients."""
    ref, c = R.reference(name), R.CASES[name]
    truth = ref["truth"]
    chain = R.torch_chain(_inputs(name), c, torch.float32)
    for k in KEYS:
        ratio = R.worst(chain[k], truth[k], truth["bound"][k])
        print("%-8s torch fp32: %-8s %.4f of the bound" % (name, k, ratio))
        assert ratio <= 1.0, (name, k, ratio)
    lv = _levels32(name)
    t = R.truth(_inputs(name), c, floors=ref["floors"], levels=lv)
    y = R.torch_lookup_chain(lv, _inputs(name), c, torch.float32)
    for k in ("out", "gcoords", "gsigma"):
        assert R.worst(y[k], t[k], t["bound"][k]) <= 1.0, (name, k)
    for i in range(c["L"]):
        assert R.worst(y["glevels"][i], t["glevels"][i], t["bound"]["glevels"][i]) <= 1.0, (name, i)
    gl = R.level_grads(c)
    gt = [torch.from_numpy(g) for g in gl]
    div = R.divisor_of(c["C"])
    want = R.pool_bwd_closed(gt, R.factor_of(c), div)
    bound = R.pool_bwd_bound(gt, [torch.zeros_like(g, dtype=torch.float64) for g in gt], R.factor_of(c), div)
    assert R.worst(R.torch_pool_chain(gl, R.factor_of(c), div, torch.float32), want, bound) <= 1.0, name
    assert float((R.torch_pool_chain(gl, R.factor_of(c), div, torch.float64) - want).abs().max()) <= 1e-13, name


@pytest.mark.parametrize("name", R.PLANTED)
def test_planted_cases_need_the_fp32_floors(name):
    """On the planted cases some fp32 floors differ from the float64 ones; out and the map gradients do not notice (they are
    continuous across an integer), the derivative with respect to coords does -- by far more than any bound."""
    ref, c = R.reference(name), R.CASES[name]
    S, f = c["S"], R.factor_of(c)
    dx = (np.arange(S) - S // 2).reshape(1, 1, S, 1, 1)
    x = dx * ref["sigma"][:, :, None].astype(np.float64) + ref["coords"][:, :, None]
    differ = sum(int((np.floor(x / f ** i) != fl).sum()) for i, fl in enumerate(ref["floors"]))
    assert differ > 0, name
    own, truth = R.truth(_inputs(name), c), ref["truth"]
    assert R.worst(own["gcoords"], truth["gcoords"], truth["bound"]["gcoords"]) > 100.0
    for k in ("out", "gf1", "gf2"):
        assert R.worst(own[k], truth[k], truth["bound"][k]) <= 1.0, (name, k)


@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_mutants_miss_the_bound(mutant):
    what, name = R.MUTANTS[mutant]
    ref, c = R.reference(name), R.CASES[name]
    got = R.truth(_inputs(name), c, floors=ref["floors"], mutant=mutant)
    ratio = R.worst(got[what], ref["truth"][what], ref["truth"]["bound"][what])
    print("%-20s %-8s on %-8s %.3g of the bound" % (mutant, what, name, ratio))
    assert ratio > 1.0, (mutant, ratio)


def test_special_values():
    """S = 1: gsigma is exactly 0 and only 0 is admitted; the "beyond" case has taps off both ends and half-inside ones; the
    "odd" case has the floor widths 77, 19, 4 that leave columns out of every window."""
    s1 = R.reference("s1")["truth"]
    assert float(s1["gsigma"].abs().max()) == 0.0 and float(s1["bound"]["gsigma"].max()) == 0.0
    ref, c = R.reference("beyond"), R.CASES["beyond"]
    fl, w = ref["floors"][0], c["W"]
    assert (fl < -1).any() and (fl > w - 1).any() and (fl == -1).any() and (fl == w - 1).any()
    assert R.widths(R.CASES["odd"]) == [77, 19, 4]
    gv = R.reference("odd")["truth"]["gvol"]
    assert gv.shape[-1] == 77 and float(gv[:, 76].abs().max()) > 0.0            # column 76: level 0 only


def test_bounds_are_small_beside_the_results():
    for name in R.CASES:
        truth = R.reference(name)["truth"]
        for k in KEYS:
            top = float(truth[k].abs().max())
            assert top == 0.0 or float(truth["bound"][k].max()) <= 1e-3 * top, (name, k)


def test_loop_case_keeps_its_taps_off_the_integers():
    """The loop of test_gpu_pcv_train.py feeds each lookup a sigma computed from the previous one, so its fp32 tap positions
    differ from the float64 ones by the accumulated error, of the order of 100 u = 6e-6 (the fp32 loop's outputs are within
    1e-5 of the float64 ones here).  Every tap of the float64 loop is at least 1e-4 from an integer: no floor can differ."""
    c, a = R.LOOP, R.loop_inputs()
    T = lambda k: torch.from_numpy(a[k]).double()  # noqa: E731
    margins = []
    watch = lambda co, sg: margins.append(R.tap_margin(co, sg, c["S"], c["L"], R.factor_of(c)))  # noqa: E731
    block = lambda p, q: R.TorchBlock(p, q, c["S"], c["L"], c["downsample"])  # noqa: E731
    with torch.no_grad():
        _, outs = R.loop(block, T("fmap1"), T("fmap2"), T("coords"), T("sigma"), T("head_sigma"), T("head_mu"), T("gouts"),
                         T("gsig"), c["iters"], watch=watch)
        f = lambda k: torch.from_numpy(a[k])  # noqa: E731
        _, outs32 = R.loop(block, f("fmap1"), f("fmap2"), f("coords"), f("sigma"), f("head_sigma"), f("head_mu"), f("gouts"),
                           f("gsig"), c["iters"])
    assert len(margins) == c["iters"] and min(margins) >= 1e-4, margins
    assert max(float((p - q.double()).abs().max()) for p, q in zip(outs, outs32)) <= 1e-5
