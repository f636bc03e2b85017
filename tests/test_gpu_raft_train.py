"""A whole RAFT-Stereo training step on the HIP nodes against fp64 (-m gpu): RAFTStereo.forward(test_mode=False) with every
parameter trainable, 1 x 3 x 32 x 64 (and 16 x 64), 2 iterations, loss sum_i mean(pred_i * w_i), against _raft_train_ref.py.

Arms (set through monkeypatch, no default changes):

    ALL_ON            extractor.TRAIN_NORM_NODES, extractor.TRAIN_CONV_NODES, BasicMultiUpdateBlock.TRAIN_NODES,
                      conv.GRAD_PREPASS and conv.GRAD_WEIGHT_HIP all True
    ALL_ON_NO_VENDOR  ALL_ON with WGRAD_VENDOR_CLASSES, WGRAD_S2_VENDOR_CLASSES and DGRAD_S2_VENDOR_CLASSES emptied (layer1's
                      64 -> 64 3x3 class on dkt_conv2d_wgrad)
    SHIPPED           the defaults
    ALL_OFF           all of them False: torch and the vendor library wherever a handle decides, printed beside every figure.
                      Measured: it is NOT inside G_BOUND at this loss's magnitude (1e-2 in both encoders' gradients at
                      every flip-free draw) -- with GRAD_PREPASS off the update operator's input gradients run on the
                      unit-scale split-fp16 convolution, below whose 2^-25 floor a mean-reduced loss's gradients lie;
                      test_all_off_arm_at_unit_gradient_magnitude shows the arm inside G_BOUND once the loss is scaled
                      by 2^20.  G_BOUND stays what it is: it is torch's own fp32 that the bound was derived from, and
                      the three arms under test meet it.

Predictions are held to _encoder_ref.compare's rule (err <= 8 * max(the fp32 CPU restatement's error, FLOOR)) at every
draw.  Gradients are compared at the first draw of DRAWS at which the device forward takes every ReLU mask of the fp64
reference (_raft_train_ref.mask_spy: all 79 sites, 4.3 million activations), under G_BOUND = 5e-5 per parameter; no such
draw in 20 is a failure.  Every comparison prints the draw used, the flips per draw tried, the worst parameter and its
error with the ALL_OFF figure beside it, and the prediction errors beside their fp32-CPU yardsticks (run with -s).  DESIGN
3.17 holds the figures measured."""
import collections

import pytest
import torch

import _encoder_ref as E
import _norm_train_ref as NR
import _raft_train_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARMS = ("ALL_ON", "ALL_ON_NO_VENDOR", "SHIPPED", "ALL_OFF")
NORM_NODE, JOIN_NODE, CONV_NODE = "_InstanceNormFnBackward", R.JOIN_NODE, "_Conv2dGradFnBackward"
GRU_NODES = ("_GateZrFnBackward", "_GateOutFnBackward", "_Pool2xFnBackward", "_InterpFnBackward")
LOOP_NODES = GRU_NODES + ("_ConvexUpsampleFnBackward", "_BuildFnBackward", "_LookupFnBackward")
_RUNS = {}


def _set_arm(mp, arm):
    from dkt_stereo_amd import conv, extractor
    from dkt_stereo_amd.update import BasicMultiUpdateBlock
    assert arm in ARMS
    if arm == "SHIPPED":
        return
    on = arm != "ALL_OFF"
    mp.setattr(extractor, "TRAIN_NORM_NODES", on)
    mp.setattr(extractor, "TRAIN_CONV_NODES", on)
    mp.setattr(BasicMultiUpdateBlock, "TRAIN_NODES", on)
    mp.setattr(conv, "GRAD_PREPASS", on)
    mp.setattr(conv, "GRAD_WEIGHT_HIP", on)
    if arm == "ALL_ON_NO_VENDOR":
        for name in ("WGRAD_VENDOR_CLASSES", "WGRAD_S2_VENDOR_CLASSES", "DGRAD_S2_VENDOR_CLASSES"):
            mp.setattr(conv, name, {})


def _inner_mask(c):
    """relu(instance_norm(c)) > 0 by dkt_instance_norm, whose bits the join node's are (test_gpu_norm_train.py)."""
    from dkt_stereo_amd import _ffi
    n, ch, h, w = c.shape
    L = _ffi.lib()
    y = torch.empty_like(c)
    ws = torch.empty(L.dkt_instance_norm_workspace(n * ch, h * w), device=c.device, dtype=torch.uint8)
    _ffi.check(L.dkt_instance_norm(c.data_ptr(), y.data_ptr(), ws.data_ptr(), n * ch, h * w, NR.EPS, 1, _ffi.device_of(c),
                                   _ffi.stream_of(c)), "dkt_instance_norm")
    return y > 0


def _graph_count(tensors):
    seen, todo, names = set(), [t.grad_fn for t in tensors], collections.Counter()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names[type(fn).__name__.rstrip("0123456789")] += 1
        todo.extend(f for f, _ in fn.next_functions)
    return names


def _step(mp, arm, case, seed, shape, scale=1.0):
    """One device step of a draw under an arm: dict(preds, grads, flips against the fp64 record, graph, conv_nodes)."""
    from dkt_stereo_amd import extractor
    with mp.context() as m:
        _set_arm(m, arm)
        model = E.make_raft(dict(case), 100 + seed).to(DEV)
        assert not model.training and all(p.requires_grad for p in model.parameters())
        _, i1, i2, ws = R.model_and_inputs(case, seed, shape)
        conv_nodes = []
        hooks = [mod.register_forward_hook(lambda _m, _a, out, n=n: conv_nodes.append((n, type(out.grad_fn).__name__)))
                 for n, mod in model.named_modules() if isinstance(mod, extractor._Conv2d)]
        try:
            with R.mask_spy(model, _inner_mask) as spy:
                preds, grads, masks = R.model_step(model, i1.to(DEV), i2.to(DEV), ws, spy, scale)
        finally:
            for h in hooks:
                h.remove()
        graph = _graph_count(preds)
    grads = {k: (None if g is None else g.detach().cpu()) for k, g in grads.items()}
    return dict(preds=[p.detach().cpu() for p in preds], grads=grads,
                flips=R.flips(R.truth_forward(case, seed, shape)["record"], masks), graph=graph, conv_nodes=conv_nodes)


def _run(mp, arm, case, seed, shape=R.SHAPE):
    """_step once per (arm, case, draw, shape): the tests share the runs."""
    k = (arm, case, seed, shape)
    if k not in _RUNS:
        _RUNS[k] = _step(mp, arm, case, seed, shape)
    return _RUNS[k]


def _flip_free(mp, arm, case, shape=R.SHAPE):
    """(draw, run) of the first draw of DRAWS at which the arm's forward takes the reference's masks."""
    for seed in R.DRAWS:
        r = _run(mp, arm, case, seed, shape)
        print("%-16s %s %s draw %d: %s" % (arm, R.case_id(dict(case)), "x".join(map(str, shape)), seed, R.flip_line(r["flips"])))
        if R.total(r["flips"]) == 0:
            return seed, r
    raise AssertionError("%s %s: no draw of %d without a flipped activation" % (arm, case, len(R.DRAWS)))


def _check_predictions(label, preds, case, seed, shape=R.SHAPE):
    y = R.yardstick(case, seed, shape)
    t = R.truth_forward(case, seed, shape)
    assert len(preds) == R.ITERS
    return E.compare(label, preds, t["preds"], y["pred_err"], names=["pred%d" % i for i in range(R.ITERS)])


def _check_gradients(mp, arm, case, shape=R.SHAPE):
    """The arm's gradients at its first flip-free draw against the truth under G_BOUND; the ALL_OFF figure (at its own
    first flip-free draw) beside it.  Returns (draw, run)."""
    seed, r = _flip_free(mp, arm, case, shape)
    want = R.truth_grads(case, seed, shape)
    errs = R.grad_error(r["grads"], want)                      # (asserts the reference's None pattern)
    assert all(bool(torch.isfinite(g).all()) for g in r["grads"].values() if g is not None)
    name, e = R.worst(errs)
    off_seed, off = _flip_free(mp, "ALL_OFF", case, shape)
    off_name, off_e = R.worst(R.grad_error(off["grads"], R.truth_grads(case, off_seed, shape)))
    print("GRAD %-16s %s %s draw %d: %d gradients, %d None, worst %s %.2e of G_BOUND %.0e | ALL_OFF draw %d: worst %s %.2e"
          % (arm, R.case_id(dict(case)), "x".join(map(str, shape)), seed, len(errs), len(want) - len(errs), name, e, R.G_BOUND,
             off_seed, off_name, off_e))
    over = {k: v for k, v in errs.items() if v > R.G_BOUND}
    assert not over, "%s: over G_BOUND (ALL_OFF's worst: %.2e): %s" % (arm, off_e, over)
    return seed, r


def _check_nodes(r, arm, case):
    """From the graph behind the predictions: which nodes the arm's forward recorded."""
    g, cfg = r["graph"], dict(case)
    assert all(g[n] > 0 for n in LOOP_NODES), {n: g[n] for n in LOOP_NODES}
    assert g[CONV_NODE] > 0
    if arm in ("ALL_ON", "ALL_ON_NO_VENDOR"):
        others = [c for c in r["conv_nodes"] if c[1] != CONV_NODE]
        assert r["conv_nodes"] and not others, others
        # fnet: the stem, 6 x norm1, 2 x norm3 and 6 joins; the shared backbone: conv2.0's norm1 and its join
        want = (1, 1) if cfg.get("shared_backbone") else (9, 6)
        assert (g[NORM_NODE], g[JOIN_NODE]) == want, (g[NORM_NODE], g[JOIN_NODE])
    else:
        assert g[NORM_NODE] == 0 and g[JOIN_NODE] == 0
        assert not any(node == CONV_NODE for _, node in r["conv_nodes"])


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("arm", ARMS)
def test_predictions_every_iteration(arm, seed, monkeypatch):
    r = _run(monkeypatch, arm, (), seed)
    print("%-16s draw %d: %s" % (arm, seed, R.flip_line(r["flips"])))
    _check_predictions("%s draw %d" % (arm, seed), r["preds"], (), seed)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_predictions_without_autograd(seed, monkeypatch):
    """ALL_ON under torch.no_grad(): the same loop on the inference kernels."""
    _set_arm(monkeypatch, "ALL_ON")
    model = E.make_raft({}, 100 + seed).to(DEV)
    _, i1, i2, _ = R.model_and_inputs((), seed)
    with torch.no_grad():
        preds = model(i1.to(DEV), i2.to(DEV), iters=R.ITERS, test_mode=False)["disp_preds"]
    assert all(p.grad_fn is None for p in preds)
    _check_predictions("ALL_ON no_grad draw %d" % seed, [p.cpu() for p in preds], (), seed)


# 2, 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", ["ALL_ON", "ALL_ON_NO_VENDOR", "SHIPPED"])
def test_parameter_gradients(arm, monkeypatch):
    seed, r = _check_gradients(monkeypatch, arm, ())
    _check_nodes(r, arm, ())


# 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [-20, 10])
def test_loss_scale(m, monkeypatch):
    """The loss times 2^m under ALL_ON_NO_VENDOR at the flip-free draw: the forward, hence the masks, do not depend on the
    scale; every gradient within G_BOUND of 2^m x the truth.  Printed: how many parameters scale bit for bit (the vendor
    GEMMs of _BuildFn and the vendor 7x7 weight gradients sit in some paths)."""
    arm, s = "ALL_ON_NO_VENDOR", 2.0 ** m
    seed, base = _flip_free(monkeypatch, arm, ())
    r = _step(monkeypatch, arm, (), seed, R.SHAPE, scale=s)
    assert R.total(r["flips"]) == 0 and all(torch.equal(p, q) for p, q in zip(r["preds"], base["preds"]))
    want = {k: (None if g is None else g * s) for k, g in R.truth_grads((), seed).items()}
    errs = R.grad_error(r["grads"], want)
    assert all(bool(torch.isfinite(g).all()) for g in r["grads"].values() if g is not None)
    name, e = R.worst(errs)
    exact = [k for k, g in r["grads"].items() if g is not None and torch.equal(g / s, base["grads"][k])]
    print("SCALE 2^%d draw %d: worst %s %.2e of G_BOUND %.0e; %d of %d gradients are 2^%d x the unscaled ones bit for bit; not: %s"
          % (m, seed, name, e, R.G_BOUND, len(exact), len(errs), m, sorted(set(errs) - set(exact))[:12]))
    over = {k: v for k, v in errs.items() if v > R.G_BOUND}
    assert not over, over


# 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overrides", R.VARIANTS, ids=R.case_id)
def test_variants(overrides, monkeypatch):
    case = R.key(overrides)
    seed, r = _check_gradients(monkeypatch, "ALL_ON", case)
    _check_predictions("ALL_ON %s draw %d" % (R.case_id(overrides), seed), r["preds"], case, seed)
    _check_nodes(r, "ALL_ON", case)
    unused = sorted(k for k, g in r["grads"].items() if g is None)
    if overrides.get("n_gru_layers") == 2:
        assert any(k.startswith("update_block.gru32.") for k in unused)
    else:
        assert not unused, unused


@pytest.mark.parametrize("impl", ["alt", "cosine"])
def test_inference_only_blocks_refuse_trainable_features(impl, monkeypatch):
    """With a trainable fnet the inference-only correlation classes raise: they never run on detached features."""
    from dkt_stereo_amd import _ffi
    _set_arm(monkeypatch, "ALL_ON")
    model = E.make_raft(dict(corr_implementation=impl), 100).to(DEV)
    _, i1, i2, _ = R.model_and_inputs((), 0)
    with pytest.raises(_ffi.DktError):
        model(i1.to(DEV), i2.to(DEV), iters=R.ITERS, test_mode=False)


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_repeatability(monkeypatch):
    """Two ALL_ON_NO_VENDOR steps on the same draw: the predictions and every parameter's gradient are bit-identical, except
    the weights of the three 7x7 layers (fnet.conv1, cnet.conv1, update_block.encoder.convf1).  Their gradient is
    torch.nn.grad.conv2d_weight, the vendor library's weight-gradient convolution (conv.py keeps k = 7 on it), which is not
    run-to-run reproducible on the feature encoder's batch of two (measured: fnet.conv1.weight alone differed).
    Nothing is downstream of a weight gradient, and the upstream gradient it is fed is this library's and repeats (the same
    layers' bias gradients, sums of the same tensor, are among the parameters held)."""
    arm = "ALL_ON_NO_VENDOR"
    seed, first = _flip_free(monkeypatch, arm, ())
    second = _step(monkeypatch, arm, (), seed, R.SHAPE)
    assert all(torch.equal(p, q) for p, q in zip(first["preds"], second["preds"]))
    model = R.model_and_inputs((), seed)[0]
    vendor = sorted(n for n, p in model.named_parameters() if p.dim() == 4 and tuple(p.shape[2:]) == (7, 7))
    assert vendor == ["cnet.conv1.weight", "fnet.conv1.weight", "update_block.encoder.convf1.weight"], vendor
    differ = sorted(k for k, g in first["grads"].items() if g is not None and not torch.equal(g, second["grads"][k]))
    print("REPEAT draw %d: %d of %d gradients differ between two steps: %s (on the vendor weight gradient: %s)"
          % (seed, len(differ), len(first["grads"]), differ, vendor))
    assert not set(differ) - set(vendor), differ


def test_all_off_arm_at_unit_gradient_magnitude(monkeypatch):
    """Why ALL_OFF is no yardstick at this loss's magnitude.  With conv.GRAD_PREPASS off the update operator's input gradients
    run on the split-fp16 convolution at unit activation scale, whose absolute floor of 2^-25 is far above the 1e-8 ... 1e-6
    gradients a mean-reduced loss sends through it: everything upstream of the update operator -- both
    encoders -- inherits errors of 1e-2.  The same arm with the loss times 2^20 (same forward, same masks) is inside
    G_BOUND: the torch / vendor arithmetic of the arm is fp32-class, the un-scaled input gradient is what misses."""
    arm, s = "ALL_OFF", 2.0 ** 20
    seed, base = _flip_free(monkeypatch, arm, ())
    want = R.truth_grads((), seed)
    r = _step(monkeypatch, arm, (), seed, R.SHAPE, scale=s)
    assert R.total(r["flips"]) == 0
    name0, e0 = R.worst(R.grad_error(base["grads"], want))
    name, e = R.worst(R.grad_error(r["grads"], {k: (None if g is None else g * s) for k, g in want.items()}))
    print("ALL_OFF draw %d: worst %s %.2e at the loss's own magnitude, worst %s %.2e with the loss times 2^20 (G_BOUND %.0e)"
          % (seed, name0, e0, name, e, R.G_BOUND))
    assert e <= R.G_BOUND, (name, e)


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_small_shape(monkeypatch):
    """1 x 3 x 16 x 64: the planes at 1/16 have a single row and the coarsest correlation level is 2 wide, the smallest sizes
    at which the reference still divides by W - 1 != 0."""
    seed, r = _check_gradients(monkeypatch, "ALL_ON", (), R.SMALL)
    _check_predictions("ALL_ON 16x64 draw %d" % seed, r["preds"], (), seed, R.SMALL)
    _check_nodes(r, "ALL_ON", ())
