"""CPU: the restated refinement loop of _raft_loop_ref.py is the oracle's, its yardsticks leave room under the project's
end-to-end limit, its bound catches every mutant, and the case table reaches every route of RAFTStereo.iterate().

Figures printed by this file on the CPU (fp32 restatement against fp64; -s shows them per case): see DESIGN.md 4.
"""
import math

import pytest
import torch

import _raft_loop_ref as LR
import _raft_train_ref as R
from oracle import torch_oracle as to


@pytest.mark.parametrize("name", LR.NAMES)
def test_iterate_ref_is_the_oracle_loop_bit_for_bit(name):
    """iterate_ref in fp32 against to.raft_iterations on the same fp32 operands: every operation is the same call on the same
    values (the taps are linspace in fp32 either way, the y row is replaced by zeros instead of overwritten), so the results
    are equal bit for bit, flow_init included."""
    cfg, iters = LR.model_of(name)[1], LR.BY_NAME[name][3]
    sd = LR.sd_of(name, torch.float32)
    f1, f2, net, inp = LR.operands_of(name)
    fi = LR.flow_init_of(name)
    lo, up = LR.iterate_ref(sd, cfg, f1, f2, net, inp, iters, fi)
    with torch.no_grad():
        want_lo, want_up = to.raft_iterations(sd, cfg, f1, f2, list(net), inp, iters, flow_init=fi)
    assert torch.equal(lo, want_lo[:, :1]) and torch.equal(up, want_up)
    assert float(want_lo[:, 1].abs().max()) == 0.0 or fi is not None


@pytest.mark.parametrize("name", ["default_64x128", "default_b2_72x136", "l3r2", "ds3_n2_sf_shared", "n1_b2", "hd96", "instance"])
def test_forward_ref_is_the_last_training_prediction(name):
    cfg, iters = LR.model_of(name)[1], LR.BY_NAME[name][3]
    sd = LR.sd_of(name, torch.float32)
    i1, i2 = LR.images_of(name)
    _, up = LR.forward_ref(sd, cfg, i1, i2, iters)
    with torch.no_grad():
        want = R.train_forward(sd, cfg, i1, i2, iters)[-1]
    assert torch.equal(up, want)


def _valid(label, t):
    for k in ("lo", "up"):
        for v in (t[k], t[k + "32"]):
            assert bool(torch.isfinite(v).all()), "%s %s: NaN / Inf in the restatement" % (label, k)
        print("YARD %-40s %s max|truth| %8.3f yardstick %.3e floor %.3e bound %.3e"
              % (label, k, float(t[k].abs().max()), t[k + "_yard"], t[k + "_floor"], t[k + "_bound"]))
        assert t[k + "_bound"] <= LR.CAP, "%s %s: %g * max(yardstick %.3e, floor %.3e) over the cap %.0e: a milder input" % (
            label, k, LR.MARGIN, t[k + "_yard"], t[k + "_floor"], LR.CAP)
        assert float(t[k].abs().max()) > 0.05, "%s %s: a truth of (nearly) zero checks nothing" % (label, k)


@pytest.mark.parametrize("name", LR.NAMES)
def test_yardstick_under_the_cap_loop(name):
    _valid(name + " loop", LR.loop_truth(name))


@pytest.mark.parametrize("name", LR.NAMES)
def test_yardstick_under_the_cap_forward(name):
    _valid(name + " forward", LR.forward_truth(name))
    _valid(name + " forward, second pair", LR.forward_truth(name, 1))
    a, b = LR.forward_truth(name)["up"], LR.forward_truth(name, 1)["up"]
    assert float((a - b).abs().max()) > 100 * LR.forward_truth(name)["up_bound"], "the second pair is not a different one"


@pytest.mark.parametrize("mutant,name", [(m, n) for m, ns in LR.MUTANTS.items() for n in ns])
def test_bound_catches_mutant(mutant, name):
    t = LR.loop_truth(name)
    err = LR.mutant_error(name, mutant)
    print("MUTANT %-24s %-20s err %.3e = %.1f x the bound %.3e" % (mutant, name, err, err / t["up_bound"], t["up_bound"]))
    assert err >= LR.MUTANT_FACTOR * t["up_bound"]


def test_flow_init_leaves_the_row_at_both_ends():
    for name in LR.NAMES:
        fi = LR.flow_init_of(name)
        if not LR.BY_NAME[name][1].get("flow_init"):
            assert fi is None
            continue
        _, overrides, (B, H, W), _, _ = LR.BY_NAME[name]
        h, w = LR.loop_grid(overrides, H, W)
        r = overrides.get("corr_radius", 4)
        assert tuple(fi.shape) == (B, 2, h, w) and float(fi[:, 1].abs().max()) == 0.0
        x = fi[:, :1].double() + torch.arange(w, dtype=torch.float64)
        assert float(x.min()) - r < -1 and float(x.max()) + r > w          # whole taps outside on either side
        assert float(x.min()) < 0 and float(x.max()) > w - 1               # and centres outside
        whole = float((x == x.round()).double().mean())
        assert 0.33 <= whole <= 0.36, whole


def test_table_is_well_formed_and_reaches_every_route():
    assert len(set(LR.NAMES)) == len(LR.NAMES)
    for name, overrides, (B, H, W), iters, route in LR.CASES:
        h, w = LR.loop_grid(overrides, H, W)
        assert h <= 34 and w <= 66 and 1 <= iters <= 7, name
        assert w >> (overrides.get("corr_levels", 4) - 1) >= 2, "%s: the reference divides by W - 1 = 0 on the coarsest level" % name
        hd = overrides.get("hidden_dims", [128] * 3)
        assert len(set(hd)) == 1, "%s: the reference does not run unequal hidden_dims" % name
    for what, pred in LR.ROUTES_REQUIRED.items():
        assert any(pred(c[1], c[4]) for c in LR.CASES), "no case for: " + what
    for mutant, names in LR.MUTANTS.items():
        assert names and all(n in LR.BY_NAME for n in names), mutant
    # odd grids, planes below one 8 x 32 tile, a batch of two on either family of routes
    grids = [LR.loop_grid(c[1], *c[2][1:]) for c in LR.CASES]
    assert any(h % 2 and w % 2 for h, w in grids) and any(h < 8 and w < 32 for h, w in [((g[0] + 3) // 4, (g[1] + 3) // 4) for g in grids])
    assert any(c[2][0] == 2 and c[4].startswith("c8") for c in LR.CASES) and any(c[2][0] == 2 and not c[4].startswith("c8") for c in LR.CASES)


def test_floor_is_one_fp32_spacing():
    for m in (0.6, 2.5, 3.99, 4.0, 150.0):
        f = LR.floor_of(torch.tensor([m, -m / 2], dtype=torch.float64))
        a = torch.tensor(m, dtype=torch.float32)
        assert f == float(torch.nextafter(a, torch.tensor(float("inf"))) - a) and not math.isnan(f)


@pytest.mark.parametrize("name", LR.IGEV_NAMES)
def test_igev_yardstick_under_the_cap(name):
    c = LR.igev_case(name)
    x, cfg = c["x"], c["cfg"]
    K = 2 * cfg["corr_radius"] + 1
    assert c["blk"].encoder.convc1.weight.shape[1] == cfg["corr_levels"] * K * (x["geo"].shape[1] + 1)
    assert (cfg["corr_levels"], x["geo"].shape[1], cfg["corr_radius"]) != (2, 8, 4)         # (what the fused lookup covers)
    assert x["geo"].shape[2] >> (cfg["corr_levels"] - 1) >= 2 and x["geo"].shape[3] % 2 and x["geo"].shape[4] % 2
    for k, t in LR.igev_truth(name).items():
        print("YARD %-40s %-4s max|truth| %8.3f yardstick %.3e floor %.3e bound %.3e"
              % (name, k, float(t["truth"].abs().max()), t["yard"], t["floor"], t["bound"]))
        assert t["bound"] <= LR.CAP
    # the loop moves the disparity by far more than the bound, and taps leave the D axis at both ends
    moved = float((LR.igev_truth(name)["disp"]["truth"] - x["disp"].double()).abs().max())
    assert moved > 1000 * LR.igev_truth(name)["disp"]["bound"], moved
    assert float(x["disp"].min()) - cfg["corr_radius"] < -1 and float(x["disp"].max()) / 2 ** (cfg["corr_levels"] - 1) + cfg["corr_radius"] > (x["geo"].shape[2] >> (cfg["corr_levels"] - 1))


@pytest.mark.parametrize("name", [n for n in LR.NAMES if LR.is_mixed(n)])
def test_mixed_precision_yardstick(name):
    """The fp16-operand restatement is far from the fp32 one (the key is visible), finite, and leaves room under what the
    project allows mixed_precision end to end."""
    for label, t, base in ((name + " loop, fp16 operands", LR.mixed_truth(name, False), LR.loop_truth(name)),
                           (name + " forward, fp16 operands", LR.mixed_truth(name, True), LR.forward_truth(name)),
                           (name + " forward, second pair, fp16 operands", LR.mixed_truth(name, True, 1), LR.forward_truth(name, 1))):
        for k in ("lo", "up"):
            assert bool(torch.isfinite(t[k + "32"]).all())
            print("YARD %-52s %s yardstick %.3e (fp32: %.3e) bound %.3e" % (label, k, t[k + "_yard"], base[k + "_yard"], t[k + "_bound"]))
            assert t[k + "_yard"] > 10 * base[k + "_yard"] and t[k + "_bound"] <= LR.CAP_MIXED
            assert t["margin"] == LR.MIXED_MARGIN and base["margin"] == LR.MARGIN
