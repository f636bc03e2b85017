"""The weight gradient of the 7x7 stem layers on dkt_conv2d_wgrad7 (csrc/conv_wgrad7.hip, conv.GRAD_WEIGHT7_HIP), -m gpu: the
entry and the node's gw against the fp64 truth and BOTH bounds of _conv_wgrad_ref.py on the cases of _conv_wgrad7_ref.py at
2^0, 2^-20, 2^-40 and 2^+20; the plan cases under (a); layouts, scale equivariance, repeatability and non-finite operands
bit for bit; routing (which layers leave the vendor call, and that nothing else changes by a bit); a whole RAFT-Stereo
training step (the helpers of test_gpu_raft_train.py, arm ALL_ON_NO_VENDOR plus the handle) with the vendor weight gradient
made to raise: 218 of 218 gradients repeat and scale bit for bit; IGEV's convd1.  The handle is set by monkeypatch.

Every case prints its figures (run with -s)."""
import functools

import pytest
import torch
import torch.nn as nn

import _conv_grad_ref as R
import _conv_wgrad7_ref as W7

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WR = W7.WR
CONV_NODE = "_Conv2dGradFnBackward"


def _refuse(*a, **k):
    raise AssertionError("torch.nn.grad.conv2d_weight was called")


@pytest.fixture
def handle(monkeypatch):
    from dkt_stereo_amd import conv
    monkeypatch.setattr(conv, "GRAD_WEIGHT7_HIP", True)
    return conv


@functools.lru_cache(maxsize=None)
def _layer(case):
    B, H, W, cin, cout = case
    w, b = W7.inputs(case)[4:]
    lay = nn.Conv2d(cin, cout, 7, padding=3)
    with torch.no_grad():
        lay.weight.copy_(w)
        lay.bias.copy_(b)
    return lay.to(DEV)


def _node_gw(case, relu, gy, x=None):
    from dkt_stereo_amd import conv
    lay = _layer(case)
    x = W7.inputs(case)[0].to(DEV) if x is None else x
    y = conv.conv2d_autograd(x, lay, relu=relu)
    assert type(y.grad_fn).__name__ == CONV_NODE
    return torch.autograd.grad(y, [lay.weight], grad_outputs=gy)[0]


@functools.lru_cache(maxsize=None)
def _entry_ref(case, relu):
    """g' of the entry (the drawn mask with ReLU, the upstream gradient itself without), the fp64 truth and bound (b) at 2^0,
    computed once: a power-of-two multiple of g' gives that multiple of all three exactly."""
    x, gp, gy = W7.inputs(case)[:3]
    g = gp if relu else gy
    return g, W7.truth(x, g), W7.b_bound(x, g)


@functools.lru_cache(maxsize=None)
def _node_ref(case, relu):
    """The same for the node: with ReLU the mask comes from the (deterministic) device forward."""
    from dkt_stereo_amd import conv
    x, _, gy = W7.inputs(case)[:3]
    y = None
    if relu:
        with torch.no_grad():
            y = conv.conv2d(x.to(DEV), _layer(case), relu=True).cpu()
    g = R.mask(gy, y)
    return g, W7.truth(x, g), W7.b_bound(x, g)


def _held(got, exact, bound, what, b=True):
    ea = WR.a_error(got.cpu(), exact)
    ok, rb = WR.b_ratio(got.cpu(), exact, bound)
    print("%s: (a) %.2e  (b) |d|/bound %.2e" % (what, ea, rb))
    assert ea <= W7.A_BOUND, (what, ea)
    assert ok or not b, (what, rb)


def _entry(x, g, amax, x_scale=1.0):
    from dkt_stereo_amd import conv
    return conv.conv2d_wgrad7(x, g, R.scale_pair(amax).to(DEV), x_scale)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", W7.CASES, ids=W7.CASE_IDS)
def test_entry_and_node_against_truth(case, relu, handle):
    x0 = W7.inputs(case)[0]
    g0, exact, bound = _entry_ref(case, relu)
    _, nexact, nbound = _node_ref(case, relu)
    gy0 = W7.inputs(case)[2]
    for k in W7.KS:
        s = 2.0 ** k
        amax = float((g0 * s).abs().max())
        # the entry: dense operands; g' as a view with a longer batch stride; x one float past a 16-byte boundary
        dense = _entry(x0.to(DEV), (g0 * s).to(DEV), amax)
        _held(dense, exact * s, bound * s, "entry %s relu=%d k=%d" % (case, relu, k))
        strided = _entry(x0.to(DEV), R.laid_out(g0 * s, "strided", DEV), amax)
        misaligned = _entry(R.laid_out(x0, "misaligned", DEV), (g0 * s).to(DEV), amax)
        # the order of every sum is a function of the shape alone: the 16-byte and the 4-byte path give the same bits
        assert torch.equal(strided, dense) and torch.equal(misaligned, dense), (case, relu, k)
        # the node: the upstream gradient dense and in both layouts
        got = _node_gw(case, relu, (gy0 * s).to(DEV))
        _held(got, nexact * s, nbound * s, "node  %s relu=%d k=%d" % (case, relu, k))
        for layout in R.LAYOUTS:
            assert torch.equal(_node_gw(case, relu, R.laid_out(gy0 * s, layout, DEV)), got), (case, relu, k, layout)
        if not relu:
            assert torch.equal(got, dense)                     # the node IS the entry on the pre-pass's g' and scale


@pytest.mark.parametrize("case", W7.PLAN_CASES, ids=W7.PLAN_IDS)
def test_plan_cases_under_a(case):
    """Bound (a) at 2^0 and 2^-20 where the plan walks (more items than blocks), where one item walks 257 column tiles and
    where the finishing kernel adds 14 slices; the 4-byte path gives the walked plan's bits too."""
    reg = W7.regime(case)
    if case == W7.WALKED:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        print("walked case: %d items on %d CUs" % (reg["items"], cus))
        assert reg["items"] > cus
    x, gp = W7.inputs(case)[:2]
    exact, bound = W7.truth(x, gp), W7.b_bound(x, gp)
    xd, gd = x.to(DEV), gp.to(DEV)
    got = {}
    for k in (0, -20):
        s = 2.0 ** k
        got[k] = _entry(xd, gd * s, float(gp.abs().max()) * s)
        _held(got[k], exact * s, bound * s, "plan %s k=%d" % (case, k), b=False)
    assert torch.equal(got[-20], got[0] * 2.0 ** -20)
    assert torch.equal(_entry(R.laid_out(x, "misaligned", DEV), gd, float(gp.abs().max())), got[0])
    assert torch.equal(_entry(xd, gd, float(gp.abs().max())), got[0])


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", W7.CASES, ids=W7.CASE_IDS)
def test_scale_equivariance_and_run_to_run_bits(case, relu, handle):
    gy0 = W7.inputs(case)[2].to(DEV)
    gw0 = _node_gw(case, relu, gy0)
    for _ in range(2):                                               # three runs in all
        assert torch.equal(_node_gw(case, relu, gy0), gw0)
    for k in W7.KS[1:]:
        s = 2.0 ** k
        assert torch.equal(_node_gw(case, relu, gy0 * s), gw0 * s), (case, relu, k)


@pytest.mark.parametrize("case", [W7.CASES[0], W7.CASES[7]], ids=[W7.CASE_IDS[0], W7.CASE_IDS[7]])
def test_non_finite_in_non_finite_out(case, handle):
    gy = W7.inputs(case)[2].to(DEV).clone()
    gy.view(-1)[gy.numel() // 2] = float("nan")
    assert not bool(torch.isfinite(_node_gw(case, False, gy)).all())
    gy = W7.inputs(case)[2].to(DEV).clone()
    gy.view(-1)[gy.numel() // 2] = float("inf")
    assert not bool(torch.isfinite(_node_gw(case, False, gy)).all())
    x = W7.inputs(case)[0].to(DEV).clone()
    x.view(-1)[x.numel() // 3] = float("inf")
    g = W7.inputs(case)[1].to(DEV)
    assert not bool(torch.isfinite(_entry(x, g, float(g.abs().max()))).all())
    x.view(-1)[x.numel() // 3] = float("nan")
    assert not bool(torch.isfinite(_entry(x, g, float(g.abs().max()))).all())
    # an all-zero gradient (pair {1, 1}) gives zeros
    assert not _node_gw(case, False, torch.zeros_like(gy)).any()


def test_centre_only_case_stores_exact_zeros(handle):
    case = W7.CENTRE_ONLY
    off = torch.ones(7, 7, dtype=torch.bool)
    off[3, 3] = False
    for relu in (False, True):
        got = _node_gw(case, relu, W7.inputs(case)[2].to(DEV)).cpu()
        assert not got[:, :, off].any() and (relu or bool(got[:, :, 3, 3].any()))
        # +0.0, not -0.0 and not a leftover of the workspace: the bits of the zeros
        assert not got[:, :, off].view(torch.int32).any()


def test_vendor_weight_gradient_is_not_called_for_the_stem_layers(monkeypatch):
    """torch.nn.grad.conv2d_weight raises: a backward through a 2 -> 64 and a 3 -> 64 7x7 layer succeeds with the handle on and
    raises with it off; an 8 -> 6 7x7 layer, GRAD_PREPASS off and GRAD_WEIGHT_HIP off raise with it on as well."""
    from dkt_stereo_amd import conv
    monkeypatch.setattr(torch.nn.grad, "conv2d_weight", _refuse)
    torch.manual_seed(12)

    def backward(lay, x):
        y = conv.conv2d_autograd(x, lay, relu=True)
        return torch.autograd.grad(y.sum(), [lay.weight, lay.bias])
    for cin in (2, 3):
        lay = nn.Conv2d(cin, 64, 7, padding=3).to(DEV)
        x = torch.randn(1, cin, 10, 14, device=DEV)
        with pytest.raises(AssertionError, match="conv2d_weight was called"):
            backward(lay, x)
        with monkeypatch.context() as m:
            m.setattr(conv, "GRAD_WEIGHT7_HIP", True)
            gw, gb = backward(lay, x)
            assert bool(torch.isfinite(gw).all()) and gw.shape == lay.weight.shape
            for name in ("GRAD_WEIGHT_HIP", "GRAD_PREPASS"):
                with m.context() as m2:
                    m2.setattr(conv, name, False)
                    with pytest.raises(AssertionError, match="conv2d_weight was called"):
                        backward(lay, x)
    monkeypatch.setattr(conv, "GRAD_WEIGHT7_HIP", True)
    lay8 = nn.Conv2d(8, 6, 7, padding=3).to(DEV)
    with pytest.raises(AssertionError, match="conv2d_weight was called"):
        backward(lay8, torch.randn(1, 8, 10, 14, device=DEV))


def test_no_host_sync_after_warm_up(handle):
    from dkt_stereo_amd import conv
    torch.manual_seed(7)
    lay = nn.Conv2d(3, 64, 7, padding=3).to(DEV)
    head = nn.Conv2d(64, 2, 1).to(DEV)
    x0 = torch.randn(2, 3, 12, 20, device=DEV)
    gy = torch.randn(2, 2, 12, 20, device=DEV) * 2.0 ** -20

    def step():
        y = conv.conv2d_autograd(conv.conv2d_autograd(x0, lay, relu=True), head)
        return torch.autograd.grad(y, [lay.weight, lay.bias, head.weight, head.bias], grad_outputs=gy)
    want = step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("relu", [False, True])
def test_forward_gx_and_gb_do_not_change_by_a_bit(monkeypatch, relu):
    from dkt_stereo_amd import conv
    case = W7.CASES[0]
    lay = _layer(case)
    gy = W7.inputs(case)[2].to(DEV)

    def run():
        x = W7.inputs(case)[0].to(DEV).requires_grad_(True)
        y = conv.conv2d_autograd(x, lay, relu=relu)
        return (y.detach(), *torch.autograd.grad(y, [x, lay.bias, lay.weight], grad_outputs=gy))
    assert conv.GRAD_WEIGHT7_HIP is False
    y0, gx0, gb0, gw0 = run()
    monkeypatch.setattr(conv, "GRAD_WEIGHT7_HIP", True)
    y1, gx1, gb1, gw1 = run()
    assert torch.equal(y1, y0) and torch.equal(gx1, gx0) and torch.equal(gb1, gb0)
    err = WR.a_error(gw1.cpu(), gw0.double().cpu())
    print("relu=%d: handle on against the vendor call: %.2e" % (relu, err))
    assert err <= 2 * W7.A_BOUND


def test_igev_motion_encoder_convd1(monkeypatch, handle):
    """convd1 (1 -> 64) as BasicMultiUpdateBlock._encoder_autograd runs it: a _Conv2dGradFnBackward node whose weight gradient
    does not touch the vendor call and meets (a) against fp64."""
    from types import SimpleNamespace
    from dkt_stereo_amd import conv
    from dkt_stereo_amd.update import BasicMotionEncoderIGEV
    torch.manual_seed(5)
    enc = BasicMotionEncoderIGEV(SimpleNamespace(corr_levels=2, corr_radius=4)).to(DEV)
    disp = torch.randn(2, 1, 12, 20, device=DEV)
    gy = torch.randn(2, 64, 12, 20, device=DEV)
    with monkeypatch.context() as m:
        m.setattr(torch.nn.grad, "conv2d_weight", _refuse)
        y = conv.conv2d_autograd(disp, enc.convd1, relu=True)
        assert type(y.grad_fn).__name__ == CONV_NODE
        gw = torch.autograd.grad(y, [enc.convd1.weight], grad_outputs=gy)[0]
    gp = R.mask(gy.cpu(), y.detach().cpu())
    _held(gw, W7.truth(disp.cpu(), gp), W7.b_bound(disp.cpu(), gp), "convd1 1 -> 64", b=False)


# ------------------------------------------------------------------------------------------------ the whole training step
_WHOLE = {}


def _whole(monkeypatch):
    """Three ALL_ON_NO_VENDOR + handle steps of _raft_train_ref's 1 x 3 x 32 x 64, 2 iterations, at the arm's first flip-free
    draw (the handle does not touch the forward), torch.nn.grad.conv2d_weight raising throughout: two at the loss's own
    magnitude, one with the loss times 2^-20.  Computed once for the tests below."""
    import _raft_train_ref as RT
    import test_gpu_raft_train as T
    from dkt_stereo_amd import conv
    if not _WHOLE:
        seed, base = T._flip_free(monkeypatch, "ALL_ON_NO_VENDOR", ())
        want = RT.truth_grads((), seed)
        with monkeypatch.context() as m:
            m.setattr(conv, "GRAD_WEIGHT7_HIP", True)
            m.setattr(torch.nn.grad, "conv2d_weight", _refuse)
            runs = [T._step(m, "ALL_ON_NO_VENDOR", (), seed, RT.SHAPE, scale=s) for s in (1.0, 1.0, 2.0 ** -20)]
        _WHOLE.update(seed=seed, base=base, want=want, runs=runs)
    return _WHOLE


def _stem_weights(grads):
    return sorted(k for k, g in grads.items() if g is not None and g.dim() == 4 and tuple(g.shape[2:]) == (7, 7))


def test_whole_step_without_the_vendor_weight_gradient(monkeypatch):
    """The step completes with the vendor weight gradient made to raise; same masks and predictions as with the handle off;
    every gradient inside G_BOUND at the flip-free draw."""
    import _raft_train_ref as RT
    w = _whole(monkeypatch)
    first = w["runs"][0]
    assert RT.total(first["flips"]) == 0
    assert all(torch.equal(p, q) for p, q in zip(first["preds"], w["base"]["preds"]))
    errs = RT.grad_error(first["grads"], w["want"])
    assert len(errs) == 218 and all(bool(torch.isfinite(g).all()) for g in first["grads"].values())
    stem = _stem_weights(first["grads"])
    assert stem == ["cnet.conv1.weight", "fnet.conv1.weight", "update_block.encoder.convf1.weight"]
    name, e = RT.worst(errs)
    print("WHOLE draw %d: worst %s %.2e of G_BOUND %.0e; the 7x7 weights: %s"
          % (w["seed"], name, e, RT.G_BOUND, ", ".join("%s %.2e" % (k, errs[k]) for k in stem)))
    over = {k: v for k, v in errs.items() if v > RT.G_BOUND}
    assert not over, over
    # every other gradient is the handle-off step's, bit for bit
    assert all(torch.equal(g, w["base"]["grads"][k]) for k, g in first["grads"].items() if k not in stem)


def test_whole_step_repeats_every_gradient(monkeypatch):
    """Two steps on one draw: the predictions and all 218 gradients are bit-identical; no parameter is exempted."""
    w = _whole(monkeypatch)
    first, second = w["runs"][:2]
    assert all(torch.equal(p, q) for p, q in zip(first["preds"], second["preds"]))
    differ = sorted(k for k, g in first["grads"].items() if not torch.equal(g, second["grads"][k]))
    print("REPEAT draw %d: %d of %d gradients differ between two steps: %s" % (w["seed"], len(differ), len(first["grads"]), differ))
    assert len(first["grads"]) == 218 and not differ, differ


def test_whole_step_loss_scale_bit_for_bit(monkeypatch):
    """The loss times 2^-20: 2^-20 times every one of the 218 gradients, bit for bit."""
    import _raft_train_ref as RT
    w = _whole(monkeypatch)
    first, small = w["runs"][0], w["runs"][2]
    s = 2.0 ** -20
    assert RT.total(small["flips"]) == 0 and all(torch.equal(p, q) for p, q in zip(small["preds"], first["preds"]))
    inexact = sorted(k for k, g in small["grads"].items() if not torch.equal(g / s, first["grads"][k]))
    print("SCALE 2^-20 draw %d: %d of %d gradients are not 2^-20 x the unscaled ones bit for bit: %s"
          % (w["seed"], len(inexact), len(small["grads"]), inexact))
    assert len(small["grads"]) == 218 and not inexact, inexact
