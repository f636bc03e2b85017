"""The fp64 truth of the whole RAFT-Stereo training step (_raft_train_ref.py), checked without a device.

* the restatement is the model: in fp32 it agrees with RAFTStereo(...).cpu() called with test_mode=False -- plain torch
  modules on the CPU, except for the correlation block, which the product has on the device only and which a stand-in made
  of the oracle's corr1d_pyramid / corr1d_lookup replaces here -- in every prediction and, at the first draw where the two
  forwards take the same ReLU masks, in every parameter gradient;
* its encode() is _encoder_ref.raft_encode and its last prediction is to.raft_iterations' flow_up, bit for bit;
* in fp32 against itself in fp64 over DRAWS: at least 5 of 20 draws have no flipped activation, and on each of those the
  worst grad_error is <= G_BOUND;
* every mutant exceeds G_BOUND on a flip-free draw, on the parameters MUTANTS names;
* the same for the four variant configurations at their first flip-free draw, with identical None patterns.

The figures are printed (run with -s)."""
import pytest
import torch

import _encoder_ref as E
import _raft_train_ref as R
from oracle import torch_oracle as to


def _first_flip_free(case, shape=R.SHAPE):
    for seed in R.DRAWS:
        fl = R.host_flips(case, seed, shape)
        print("%s draw %d: %s" % (R.case_id(dict(case)), seed, R.flip_line(fl)))
        if R.total(fl) == 0:
            return seed
    raise AssertionError("no flip-free draw in DRAWS for %s" % (case,))


class _TorchCorr:
    """CorrBlock1D's interface on the oracle's stock-torch pyramid and lookup (the product's block has no CPU path)."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
        self.radius = radius
        self.corr_pyramid = to.corr1d_pyramid(fmap1, fmap2, num_levels)

    def __call__(self, coords):
        return to.corr1d_lookup(self.corr_pyramid, coords, self.radius)


def test_restatement_is_the_model(monkeypatch):
    from dkt_stereo_amd import raft_stereo
    monkeypatch.setitem(raft_stereo.CORR_IMPLEMENTATIONS, "reg", _TorchCorr)
    case = ()
    for seed in R.DRAWS:
        model, i1, i2, ws = R.model_and_inputs(case, seed)
        for p in model.parameters():
            assert p.requires_grad
        with R.mask_spy(model) as spy:
            preds, got, masks = R.model_step(model, i1, i2, ws, spy)
        y = R.yardstick(case, seed)
        fl = R.flips(y["record"], masks)
        err = [E.rel_err(p.detach(), q) for p, q in zip(preds, R.truth_forward(case, seed)["preds"])]
        print("draw %d: model on the CPU, predictions against fp64 %s (the fp32 restatement: %s), masks against the fp32 "
              "restatement: %s" % (seed, ["%.1e" % e for e in err], ["%.1e" % e for e in y["pred_err"]], R.flip_line(fl)))
        assert len(preds) == R.ITERS                                       # _encoder_ref.compare's rule
        assert all(e <= E.M * max(ye, E.FLOOR) for e, ye in zip(err, y["pred_err"])), (seed, err, y["pred_err"])
        if R.total(fl) == 0:
            break
    else:
        raise AssertionError("no draw at which the model and the restatement take the same masks")
    errs = R.grad_error(got, R.fp32_grads(case, seed))
    name, e = R.worst(errs)
    print("draw %d: %d parameter gradients, worst %s %.2e (G_BOUND %.0e)" % (seed, len(errs), name, e, R.G_BOUND))
    assert len(errs) == len(list(model.parameters())) and e <= R.G_BOUND, (name, e)


def test_built_from_the_oracle():
    """encode() is raft_encode and the last prediction is raft_iterations' flow_up: the same bits in fp32."""
    for overrides in [{}] + R.VARIANTS:
        case = R.key(overrides)
        model, i1, i2, _ = R.model_and_inputs(case, 0)
        sd, cfg = E.cast_sd(model, torch.float32), R.config(overrides)
        with torch.no_grad():
            want = E.raft_encode(sd, cfg, i1, i2)
            got = R.encode(sd, cfg, i1, i2)
            assert all(torch.equal(a, b) for a, b in zip(E.flatten(got), E.flatten(want))), overrides
            _, up = to.raft_iterations(sd, cfg, *want, R.ITERS)
        assert torch.equal(up, R.yardstick(case, 0)["preds"][-1]), overrides


def test_fp32_against_fp64_over_the_draws():
    case, free, worst = (), [], []
    for seed in R.DRAWS:
        fl = R.host_flips(case, seed)
        y = R.yardstick(case, seed)
        line = "draw %2d: %-60s predictions %.1e %.1e" % (seed, R.flip_line(fl), *y["pred_err"])
        assert max(y["pred_err"]) <= E.CAP, (seed, y["pred_err"])
        if R.total(fl) == 0:
            name, e = R.worst(R.grad_error(R.fp32_grads(case, seed), R.truth_grads(case, seed)))
            free.append(seed)
            worst.append((e, name, seed))
            line += "  worst gradient %s %.2e" % (name, e)
        print(line)
    print("%d of %d draws flip-free; worst flip-free gradient error %.2e (%s, draw %d); G_BOUND %.0e"
          % (len(free), len(R.DRAWS), *max(worst), R.G_BOUND))
    assert len(free) >= 5, free
    assert max(worst)[0] <= R.G_BOUND, max(worst)


@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_mutants_are_caught(mutant):
    case = ()
    seed = _first_flip_free(case)
    model, i1, i2, ws = R.model_and_inputs(case, seed)
    got, _ = R.grads(E.cast_sd(model, torch.float64), R.config(), i1, i2, R.ITERS, ws, R.param_names(model), mutant=mutant)
    want = R.truth_grads(case, seed)
    lost = sorted(k for k, g in got.items() if g is None and want[k] is not None)
    got = {k: (torch.zeros_like(want[k]) if k in lost else g) for k, g in got.items()}      # a lost gradient: all of it is error
    errs = R.grad_error(got, want)
    over = sorted(k for k, e in errs.items() if e > R.G_BOUND)
    print("%-22s draw %d: %d of %d parameters over G_BOUND, %d of them without any gradient; named: %s"
          % (mutant, seed, len(over), len(errs), len(lost), ", ".join("%s %.2e" % (k, errs[k]) for k in R.MUTANTS[mutant])))
    for k in R.MUTANTS[mutant]:
        assert errs[k] > R.G_BOUND, (mutant, k, errs[k])


@pytest.mark.parametrize("overrides", R.VARIANTS, ids=R.case_id)
def test_variants(overrides):
    case = R.key(overrides)
    seed = _first_flip_free(case)
    want = R.truth_grads(case, seed)
    errs = R.grad_error(R.fp32_grads(case, seed), want)          # (asserts identical None patterns)
    name, e = R.worst(errs)
    unused = sorted(k for k, v in want.items() if v is None)
    print("%s draw %d: worst %s %.2e; %d parameters without a gradient" % (R.case_id(overrides), seed, name, e, len(unused)))
    assert e <= R.G_BOUND, (name, e)
    if overrides.get("n_gru_layers") == 2:
        assert unused and all(k.startswith(("update_block.gru32.", "cnet.layer5.", "cnet.outputs32.")) for k in unused), unused
        assert any(k.startswith("update_block.gru32.") for k in unused)
    else:
        assert not unused, unused


def test_small_shape_has_a_flip_free_draw():
    """1 x 3 x 16 x 64 (single-row planes at 1/16, a coarsest correlation level 2 wide): the truth is finite, a flip-free draw
    exists and the fp32 restatement is inside G_BOUND there."""
    case = ()
    seed = _first_flip_free(case, R.SMALL)
    t = R.truth_forward(case, seed, R.SMALL)
    assert all(bool(torch.isfinite(p).all()) for p in t["preds"])
    name, e = R.worst(R.grad_error(R.fp32_grads(case, seed, R.SMALL), R.truth_grads(case, seed, R.SMALL)))
    print("small shape draw %d: worst %s %.2e" % (seed, name, e))
    assert e <= R.G_BOUND, (name, e)
