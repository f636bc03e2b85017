"""The PCVNet-loss reference checks itself on the CPU (no device needed): the torch restatement reproduces what the
reference's own sequence_loss_pcvnet returned or raised under autograd (tests/golden/pcv_loss.npz); the float64 closed form
equals torch's own float64 autograd; torch's fp32 autograd meets every bound of _pcv_loss_ref.py on every case and equals
the truth on every exact quantity (mask, count, the twelve fractions, the sign pattern of every gradient); every mutant
misses a bound or an equality on the case named for it; and the cases hit what they are named for."""
import os

import numpy as np
import pytest
import torch

import _pcv_loss_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pcv_loss.npz")


@pytest.mark.parametrize("name", R.GOLDEN_CASES)
def test_restatement_reproduces_the_reference(name):
    """Same exception or same return; the stored fp32 results lie inside the bounds of the truth, and the restatement's are
    the reference's to within the same bounds (the same bits wherever the two ran on one build of torch)."""
    z = np.load(GOLDEN)
    ref = R.reference(name)
    mine = ref["fp32"]["targets"][0]
    raises = str(z[name + "/raises"])
    assert (mine["raises"] or "") == raises == (R.expected_exception(ref["a"]) or "") == R.RAISING.get(name, "")
    if raises:
        return
    t = ref["truth"]
    tk = t["targets"][0]
    assert np.array_equal(z[name + "/mask"], mine["mask"].numpy()) and np.array_equal(z[name + "/mask"], tk["mask"].numpy())
    keys = [k for k in R.METRIC_KEYS if k in mine["metrics"]]
    stored = dict(zip(keys, z[name + "/metrics"]))
    assert len(keys) == len(z[name + "/metrics"])
    if tk["loss"] is None:
        assert float(z[name + "/loss"]) == 0 and mine["loss"] == 0 and stored == R.EMPTY_METRICS == mine["metrics"]
        return
    for k in keys:
        if k in R.COUNT_KEYS:
            assert stored[k] == mine["metrics"][k] == tk["metrics"][k], (name, k)
    got = dict(targets=[dict(loss=float(z[name + "/loss"]), metrics=stored, raises=None)], grefine=torch.from_numpy(z[name + "/grefine"]),
               gdisp=list(torch.from_numpy(z[name + "/gdisp"])), gmu=list(torch.from_numpy(z[name + "/gmu"])))
    # the fixture's gradients are of target 0 alone
    t0 = R.truth(dict(ref["a"], gt=ref["a"]["gt"][:1], valid=ref["a"]["valid"][:1]))
    for what, ratio in R.compare(got, t0).items():
        print("%-12s reference fp32: %-10s %.4f of the bound" % (name, what, ratio))
        assert ratio <= 1.0, (name, what, ratio)
    mine0 = R.torch_run(dict(ref["a"], gt=ref["a"]["gt"][:1], valid=ref["a"]["valid"][:1]), torch.float32)
    assert np.array_equal(np.sign(z[name + "/gdisp"]), np.sign(torch.stack(mine0["gdisp"]).numpy()))
    assert np.array_equal(np.sign(z[name + "/gmu"]), np.sign(torch.stack(mine0["gmu"]).numpy()))
    near = lambda x, y: float((torch.as_tensor(x) - torch.as_tensor(y)).abs().max()) <= 8 * R.U * float(torch.as_tensor(y).abs().max())  # noqa: E731
    assert near(torch.stack(mine0["gdisp"]), z[name + "/gdisp"]) and near(torch.stack(mine0["gmu"]), z[name + "/gmu"])
    if np.isfinite(z[name + "/loss"]):
        assert abs(float(mine["loss"]) - float(z[name + "/loss"])) <= 8 * R.U * abs(float(z[name + "/loss"]))
        assert near(mine0["grefine"], z[name + "/grefine"])


def test_the_reference_cannot_be_called_twice():
    """The fact the module's one deviation rests on: the reference's second call on the same results raised ValueError,
    with mu_preds left 5-D by the first."""
    z = np.load(GOLDEN)
    assert str(z["second_call/raises"]) == "ValueError" and int(z["second_call/mu_dim"]) == 5


@pytest.mark.parametrize("name", R.VALUE_CASES)
def test_closed_form_is_torchs_float64_autograd(name):
    ref = R.reference(name)
    t, d = ref["truth"], R.torch_run(ref["a"], torch.float64)
    for g, tk in zip(d["targets"], t["targets"]):
        assert torch.equal(g["mask"], tk["mask"])
        if tk["loss"] is None:
            assert g["loss"] == 0
            continue
        if np.isnan(tk["loss"]):
            assert np.isnan(float(g["loss"]))
        else:
            assert abs(float(g["loss"]) - tk["loss"]) <= 1e-13 * abs(tk["loss"]), name
        for k, v in tk["metrics"].items():
            if k in R.COUNT_KEYS:
                continue                        # (fractions: the truth holds them as fp32 forms them; compared in the fp32 test)
            assert (np.isnan(v) and np.isnan(g["metrics"][k])) or abs(g["metrics"][k] - v) <= 1e-13 * abs(v), (name, k)
    if "gdisp" not in d:
        assert all(tk["loss"] is None for tk in t["targets"])
        return
    pairs = [(d["grefine"], t["grefine"][0])] + list(zip(d["gdisp"], (v for v, _ in t["gdisp"]))) + \
        list(zip(d["gmu"], (v for v, _ in t["gmu"])))
    for got, exact in pairs:
        exact = exact.reshape(got.shape)
        keep = torch.isfinite(exact)
        assert torch.equal(torch.isfinite(got), keep), name
        scale = float(exact[keep].abs().max())
        assert float((got - exact)[keep].abs().max()) <= 1e-13 * max(scale, 1e-300), name


@pytest.mark.parametrize("name", R.VALUE_CASES)
def test_torch_fp32_is_inside_every_bound_and_equal_on_every_exact_quantity(name):
    ref = R.reference(name)
    y, t = ref["fp32"], ref["truth"]
    assert R.exact_facts(y) == R.truth_facts(t, signs="gdisp" in y), name
    for what, ratio in R.compare(y, t).items():
        print("%-12s torch fp32: %-10s %.4f of the bound" % (name, what, ratio))
        assert ratio <= 1.0, (name, what, ratio)


@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_mutants_miss_a_bound_or_an_equality(mutant):
    what, name = R.MUTANTS[mutant]
    ref = R.reference(name)
    t, got = ref["truth"], R.truth(ref["a"], mutant=mutant)
    if what == "mask":
        assert not torch.equal(got["targets"][0]["mask"], t["targets"][0]["mask"])
    elif what == "N":
        assert got["targets"][0]["N"] != t["targets"][0]["N"]
    elif what == "counts":
        assert any(got["targets"][0]["metrics"][k] != t["targets"][0]["metrics"][k] for k in R.COUNT_KEYS)
    elif what == "signs":
        assert R.truth_facts(got) != R.truth_facts(t) and R.truth_facts(got, signs=False) == R.truth_facts(t, signs=False)
    elif what == "loss":
        ratio = R.scalar_ratio(got["targets"][0]["loss"], t["targets"][0]["loss"], t["targets"][0]["loss_bound"])
        print("%-22s loss on %-6s %.3g of the bound" % (mutant, name, ratio))
        assert ratio > 1.0
    elif what == "epe":
        tk = t["targets"][0]
        assert R.scalar_ratio(got["targets"][0]["metrics"]["epe"], tk["metrics"]["epe"], tk["metric_bounds"]["epe"]) > 1.0
    else:
        ratio = max(R.worst(g, v, b) for (g, _), (v, b) in zip(got[what], t[what]))
        print("%-22s %s on %-6s %.3g of the bound" % (mutant, what, name, ratio))
        assert ratio > 1.0
    assert len(R.MUTANTS) >= 8


def test_cases_hit_what_they_are_named_for():
    N = lambda name, k=0: R.reference(name)["truth"]["targets"][k]["N"]                                # noqa: E731
    assert N("one") == 1 and N("empty") == 0 and N("pair", 1) == 0 and N("pair") > 0 and N("pair2") > 0 and N("pair2", 1) > 0
    assert not torch.equal(R.reference("pair2")["truth"]["targets"][0]["mask"], R.reference("pair2")["truth"]["targets"][1]["mask"])
    c = R.CASES
    assert c["ragged"]["H"] * c["ragged"]["W"] == 1221 and 1221 % 4 and 1221 > R.TILE
    assert c["vec"]["H"] * c["vec"]["W"] == 1280 and 1280 % 4 == 0 and 1280 > R.TILE
    mask = R.reference("edges")["truth"]["targets"][0]["mask"]
    assert tuple(bool(mask[0, 0, 5, x]) for x in range(10)) == R.EDGE_IN
    a = R.inputs("edges")
    assert np.signbit(a["gt"][0][0, 0, 5, 1]) and a["gt"][0][0, 0, 5, 3] < 512 and np.isnan(a["valid"][0][0, 5, 9])
    a, t = R.inputs("ties"), R.reference("ties")["truth"]
    for key, row in (("disp", 1), ("refine", 2)):
        p = a["disp"][3] if key == "disp" else a["refine"]
        assert tuple(float(v) for v in (p - a["gt"][0])[0, 0, row, :len(R.TIE_EPE)]) == R.TIE_EPE
    assert float((a["disp"][0] - a["gt"][0])[0, 0, 3, :4].__abs__().max()) == 0.0
    gd = t["gdisp"][0][0]
    assert float(gd[0, 0, 3, :4].abs().max()) == 0.0 and bool(t["targets"][0]["mask"][0, 0, 3, :4].all())
    assert float(R.inputs("big")["refine"].min()) >= 50
    tk = R.reference("nan_refine")["truth"]["targets"][0]
    assert np.isnan(tk["loss"]) and R.expected_exception(R.inputs("nan_refine")) is None
    # inf_w_offmask: the Inf sits where the mask is off
    a = R.inputs("inf_w_offmask")
    where = np.argwhere(~np.isfinite(a["w"][1]))
    assert len(where) == 1 and a["valid"][0][0, where[0][2], where[0][3]] == 0
    # every branch of the smooth-L1 and every threshold is met in the ordinary case
    tk = R.reference("ord")["truth"]["targets"][0]
    assert 0 < tk["metrics"]["1px_final"] < 1 and 0 < tk["metrics"]["bad5"] < 1 and 0 < tk["metrics"]["1px"] < 1


def test_bounds_are_small_beside_the_results():
    for name in R.VALUE_CASES:
        t = R.reference(name)["truth"]
        for tk in t["targets"]:
            if tk["loss"] is None or np.isnan(tk["loss"]):
                continue
            assert tk["loss_bound"] <= 1e-5 * abs(tk["loss"]), name
        for v, b in [t["grefine"]] + t["gdisp"] + t["gmu"]:
            keep = torch.isfinite(v)
            top = float(v[keep].abs().max())
            assert top == 0.0 or float(b[keep].max()) <= 1e-5 * top, name
