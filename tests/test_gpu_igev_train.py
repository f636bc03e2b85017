"""IGEV-Stereo's training loop on the HIP nodes against fp64 (-m gpu): igev_loop.igev_iterate_train at quarter resolution
16 x 24, B = 1, two iterations, every parameter of the update block and of the (stand-in) up-sampling head trainable, loss
sum_i mean(pred_i * w_i), against _igev_train_ref.py.

Arms, on the same driver, update block, geometry volume and head:

    N   igev_loop.upsample_disp: the softmax, the factor 4 and context_upsample as one node (context_upsample_logits)
    T   the reference's expression sequence in torch (F.softmax, disp * 4., unfold / interpolate / mul / sum)

The prediction feeds nothing but the loss, so both arms go through bit-identical low-resolution disparities, mask features
and hidden states at every iteration (asserted); their ReLU masks are then the same, and the arms are compared at every
draw: every parameter within G_BOUND = 5e-5 (_raft_train_ref.grad_error), every prediction of arm N within the node's
out bound (_context_upsample_ref) of the float64 closed form on the operands it was given.  Against fp64 the arms are
compared at the first draw of DRAWS at which arm T is within G_BOUND of the truth on every parameter (an fp32 forward
may put an activation on the other side of 0 from fp64: test_host_igev_train_ref.py); arm N must be within G_BOUND there
too, and no such draw in ten is a failure.  Figures are printed (run with -s)."""
import pytest
import torch

import _context_upsample_ref as CR
import _igev_train_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_RUNS = {}


def _dev(x):
    d = dict(x)
    for k in ("m1", "m2", "geo", "disp", "coords"):
        d[k] = x[k].to(DEV)
    d["net"] = [t.to(DEV) for t in x["net"]]
    d["inp"] = [[t.to(DEV) for t in s] for s in x["inp"]]
    return d


def _loop(case, seed, arm, grad=True):
    """One step of draw `seed`: dict(preds, disp, net, states = every tensor the update block returned, in order, operands =
    the (disp, logits) of every up-sampling, grads)."""
    from dkt_stereo_amd import igev_loop
    from dkt_stereo_amd.geometry import Combined_Geo_Encoding_Volume
    blk, head = R.make_block(case, seed).to(DEV), R.make_head(seed).to(DEV)
    x = _dev(R.inputs(case, seed))
    states, operands = [], []

    def spy(_module, _args, out):
        flat = out if isinstance(out, list) else list(out[0]) + [t for t in out[1:] if t is not None]
        states.extend(t.detach() for t in flat)

    def spx_gru(t):
        logits = head.spx_gru(t)
        operands.append(logits.detach())
        return logits

    def upsample(disp, mask_feat_4):
        operands.append(disp.detach())
        if arm == "N":
            return igev_loop.upsample_disp(disp, mask_feat_4, None, head.spx_2_gru, spx_gru)
        return CR.sequence_logits(disp, spx_gru(head.spx_2_gru(mask_feat_4, None))).unsqueeze(1)

    handle = blk.register_forward_hook(spy)
    try:
        with torch.set_grad_enabled(grad):
            geo_fn = Combined_Geo_Encoding_Volume(x["m1"], x["m2"], x["geo"], radius=R.RADIUS, num_levels=R.LEVELS)
            preds, disp, net = igev_loop.igev_iterate_train(blk, geo_fn, x["disp"], x["coords"], x["net"], x["inp"], R.ITERS, upsample)
    finally:
        handle.remove()
    out = dict(preds=preds, disp=disp, net=net, states=states, operands=[tuple(operands[i:i + 2]) for i in range(0, len(operands), 2)])
    if grad:
        names = R.param_names(blk, head)
        params = [p for _, p in blk.named_parameters()] + [p for _, p in head.named_parameters()]
        value = R.loss(preds, [w.to(DEV) for w in x["ws"]])
        got = torch.autograd.grad(value, params, allow_unused=True)
        out["grads"] = {k: (None if g is None else g.detach().cpu()) for k, g in zip(names, got)}
        out["nodes"] = [type(p.grad_fn).__name__ for p in preds]
    out["preds"] = [p.detach() for p in preds]
    return out


def _run(case, seed, arm):
    k = (case, seed, arm)
    if k not in _RUNS:
        _RUNS[k] = _loop(case, seed, arm)
    return _RUNS[k]


def _check_arms(case, seed):
    """N against T at one draw: the same low-resolution states bit for bit, gradients within G_BOUND, N's predictions
    within the node's out bound.  Returns (N, T)."""
    n, t = _run(case, seed, "N"), _run(case, seed, "T")
    assert len(n["preds"]) == R.ITERS and len(n["states"]) == len(t["states"]) > 0
    assert all(torch.equal(a, b) for a, b in zip(n["states"], t["states"]))
    assert torch.equal(n["disp"], t["disp"]) and all(torch.equal(a, b) for a, b in zip(n["net"], t["net"]))
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(n["operands"], t["operands"]))
    name, e = R.worst(R.grad_error(n["grads"], t["grads"]))
    line = []
    for pred, (disp, logits) in zip(n["preds"], n["operands"]):
        ops = (disp.cpu(), logits.cpu(), torch.zeros(pred.shape[0], *pred.shape[2:]))
        exact = CR.closed_form(*ops, True)[0]
        mags = CR.magnitudes(*ops, True)
        in_u, of_bound = CR.worst(pred[:, 0], exact, mags["out"], CR.constants(mags, True)["out"])
        line.append("%.2f u*mag (%.3f of the bound)" % (in_u, of_bound))
        assert of_bound <= 1.0, (seed, in_u, of_bound)
    print("N|T  %s draw %d: worst %s %.2e of G_BOUND %.0e; predictions %s" % (dict(case), seed, name, e, R.G_BOUND, ", ".join(line)))
    assert e <= R.G_BOUND, (seed, name, e)
    return n, t


def _check_truth(case):
    """The first draw at which arm T is within G_BOUND of the fp64 truth on every parameter: arm N must be too."""
    for seed in R.DRAWS:
        n, t = _check_arms(case, seed)
        want, wpreds = R.truth(case, seed)
        tn, te = R.worst(R.grad_error(t["grads"], want))
        nn, ne = R.worst(R.grad_error(n["grads"], want))
        print("FP64 %s draw %d: T worst %s %.2e, N worst %s %.2e (G_BOUND %.0e)" % (dict(case), seed, tn, te, nn, ne, R.G_BOUND))
        if te > R.G_BOUND:
            continue
        assert ne <= R.G_BOUND, (seed, nn, ne)
        return seed, n
    raise AssertionError("%s: arm T is within G_BOUND of the truth at none of %d draws" % (dict(case), len(R.DRAWS)))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_node_arm_against_torch_arm(seed):
    n, _ = _check_arms((), seed)
    assert n["nodes"] == ["UnsqueezeBackward0"] * R.ITERS


def test_parameter_gradients_against_fp64():
    seed, n = _check_truth(())
    assert not [k for k, g in n["grads"].items() if g is None]                 # every parameter is reached
    assert all(bool(torch.isfinite(g).all()) for g in n["grads"].values())


@pytest.mark.parametrize("overrides", R.VARIANTS[1:], ids=lambda o: "+".join(sorted(o)))
def test_variants(overrides):
    """The slow-fast schedule and two GRU layers; with two layers the coarsest GRU has no gradient in either arm or the truth
    (grad_error asserts the None pattern)."""
    seed, n = _check_truth(R.key(overrides))
    unused = sorted(k for k, g in n["grads"].items() if g is None)
    if overrides.get("n_gru_layers") == 2:
        assert unused and all(k.startswith("update_block.gru16.") for k in unused), unused
    else:
        assert not unused, unused


def test_graph_holds_the_node():
    """The predictions hang on _ContextUpsampleLogitsFn and, with a geometry volume that requires grad, on the geometry
    lookup's node; none of them on torch's softmax or im2col backward, and the volume's gradient arrives."""
    from dkt_stereo_amd import igev_loop
    from dkt_stereo_amd.geometry import Combined_Geo_Encoding_Volume
    blk, head = R.make_block((), 0).to(DEV), R.make_head(0).to(DEV)
    x = _dev(R.inputs((), 0))
    x["geo"].requires_grad_(True)
    geo_fn = Combined_Geo_Encoding_Volume(x["m1"], x["m2"], x["geo"], radius=R.RADIUS, num_levels=R.LEVELS)
    up = lambda d, m: igev_loop.upsample_disp(d, m, None, head.spx_2_gru, head.spx_gru)  # noqa: E731
    preds, _, _ = igev_loop.igev_iterate_train(blk, geo_fn, x["disp"], x["coords"], x["net"], x["inp"], R.ITERS, up)
    seen, todo, names = set(), [p.grad_fn for p in preds], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__.rstrip("0123456789"))
        todo.extend(f for f, _ in fn.next_functions)
    assert "_ContextUpsampleLogitsFnBackward" in names and "_GeoLookupFnBackward" in names
    assert not {n for n in names if n.startswith(("SoftmaxBackward", "Im2ColBackward", "UpsampleNearest"))}, names
    (g,) = torch.autograd.grad(sum(p.sum() for p in preds), [x["geo"]])
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0


def test_two_runs_bit_for_bit():
    """Predictions, states and every gradient of the update block (this library's nodes end to end) repeat bit for bit.  Not
    held to that: the head's own gradients (torch's transposed-convolution backward) and the weight of the block's one 7x7
    layer, whose gradient conv.py keeps on the vendor library's weight-gradient convolution (the exception of
    test_gpu_raft_train.test_repeatability); those are within G_BOUND of each other."""
    first, second = _run((), 0, "N"), _loop((), 0, "N")
    assert all(torch.equal(a, b) for a, b in zip(first["preds"] + first["states"], second["preds"] + second["states"]))
    differ = sorted(k for k, g in first["grads"].items() if not torch.equal(g, second["grads"][k]))
    vendor = sorted("update_block." + n for n, p in R.make_block((), 0).named_parameters()
                    if p.dim() == 4 and tuple(p.shape[2:]) == (7, 7))
    assert vendor == ["update_block.encoder.convd1.weight"], vendor
    print("REPEAT: %d of %d gradients differ between two steps: %s" % (len(differ), len(first["grads"]), differ))
    assert not [k for k in differ if not k.startswith("head.") and k not in vendor], differ
    assert R.worst(R.grad_error(second["grads"], first["grads"]))[1] <= R.G_BOUND


def test_no_grad_runs_the_inference_operators():
    """Under torch.no_grad(): no graph, and the low-resolution results are igev_iterate's plain loop bit for bit, the last
    prediction the up-sampling of its disparity and mask features."""
    from dkt_stereo_amd import igev_loop
    from dkt_stereo_amd.geometry import Combined_Geo_Encoding_Volume
    got = _loop((), 0, "N", grad=False)
    assert all(p.grad_fn is None and not p.requires_grad for p in got["preds"])
    blk, head = R.make_block((), 0).to(DEV), R.make_head(0).to(DEV)
    x = _dev(R.inputs((), 0))
    with torch.no_grad():
        geo_fn = Combined_Geo_Encoding_Volume(x["m1"], x["m2"], x["geo"], radius=R.RADIUS, num_levels=R.LEVELS)
        disp, mask, net = igev_loop.igev_iterate(blk, geo_fn, x["disp"], x["coords"], x["net"], x["inp"], R.ITERS, use_hip_graph=False)
        last = igev_loop.upsample_disp(disp, mask, None, head.spx_2_gru, head.spx_gru)
    assert torch.equal(got["disp"], disp) and all(torch.equal(a, b) for a, b in zip(got["net"], net))
    assert torch.equal(got["preds"][-1], last)
