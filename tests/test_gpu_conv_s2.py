"""The backward of the stride-2 convolutions (-m gpu): dkt_conv2d_dgrad_s2 / dkt_conv2d_wgrad_s2 behind conv.conv2d_dgrad_s2 /
conv2d_wgrad_s2, the conv2d_autograd node on a stride-2 layer, and the encoders' wiring (extractor.TRAIN_CONV_NODES), against
the fp64 truth and the bounds of _conv_s2_ref.py at upstream gradients of magnitude 2^0, 2^-20, 2^-40 and 2^+20 in both
operand layouts.  Every case prints its figures (run with -s)."""
import functools

import pytest
import torch
import torch.nn as nn

import _conv_s2_ref as S
import _synth
from test_gpu_conv_grad import _NoSync, _PackCounter

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NODE = "_Conv2dGradFnBackward"
#: weight draws of test_encoder_wiring, tried in order (see its docstring)
WIRING_SEEDS = tuple(range(5, 25))


@functools.lru_cache(maxsize=None)
def _layer(case):
    B, H, W, k, cin, cout = case
    _, w, b, _, _ = S.inputs(case)
    lay = nn.Conv2d(cin, cout, k, stride=2, padding=k // 2)
    with torch.no_grad():
        lay.weight.copy_(w)
        lay.bias.copy_(b)
    return lay.to(DEV)


@functools.lru_cache(maxsize=None)
def _truth(case):
    """g' at m = 0 and the fp64 truth of it, computed once: a power-of-two multiple of g' gives that multiple exactly."""
    B, H, W, k, cin, cout = case
    x, w, _, _, _ = S.inputs(case)
    gp = S.masked(case)
    return gp, S.truth_gx(gp, w, (H, W)), S.truth_gw(x, gp, k), S.b_bound(x, gp, k)


def _entries(case, m, layout, out=None):
    """Both entries on g' * 2^m in `layout` (read in place: the pre-pass without a mask copies nothing)."""
    from dkt_stereo_amd import conv
    B, H, W, k, cin, cout = case
    lay = _layer(case)
    g = S.R.laid_out(_truth(case)[0] * 2.0 ** m, layout, DEV)
    x = S.R.laid_out(S.inputs(case)[0], layout, DEV)
    gp, _, scale = conv.conv_grad_prepass(g, None, want_bias=False)
    assert gp.data_ptr() == g.data_ptr()
    shim = conv._grad_layer(lay)
    gx = conv.conv2d_dgrad_s2(gp, shim, scale, (H, W), shim.pack_scale, out=out)
    gw = conv.conv2d_wgrad_s2(x, gp, scale, k)
    return gx, gw


@pytest.mark.parametrize("m", S.KS)
@pytest.mark.parametrize("layout", S.LAYOUTS)
@pytest.mark.parametrize("case", S.CASES, ids=S.CASE_IDS)
def test_entries_against_truth(case, layout, m):
    _, gx, gw, bound = _truth(case)
    s = 2.0 ** m
    got_gx, got_gw = _entries(case, m, layout)
    e_gx, e_a = S.gx_error(got_gx.cpu(), gx * s), S.a_error(got_gw.cpu(), gw * s)
    ok_b, r_b = S.b_ratio(got_gw.cpu(), gw * s, bound * s)
    print("case %s %s m=%d: gx %.2e (/bound %.3f)  gw (a) %.2e (/bound %.3f)  (b) ratio %.3f"
          % (case, layout, m, e_gx, e_gx / S.GX_BOUND, e_a, e_a / S.A_BOUND, r_b))
    assert e_gx <= S.GX_BOUND
    assert e_a <= S.A_BOUND
    assert ok_b


@pytest.mark.parametrize("case", S.CASES, ids=S.CASE_IDS)
def test_every_element_is_written_and_runs_repeat(case):
    """gx into a NaN-filled buffer comes back finite everywhere (with exact zeros at a 1x1 layer's odd positions); a second
    run gives the same bits; the 16-byte and the 4-byte path of the weight gradient give the same bits."""
    B, H, W, k, cin, cout = case
    out = torch.full((B, cin, H, W), float("nan"), device=DEV)
    gx, gw = _entries(case, -20, "misaligned", out=out)
    assert gx.data_ptr() == out.data_ptr() and bool(torch.isfinite(out).all())
    if k == 1:
        assert not out[:, :, 1::2].any() and not out[:, :, :, 1::2].any()
        assert torch.equal(out[:, :, 1::2], torch.zeros_like(out[:, :, 1::2]))
    gx2, gw2 = _entries(case, -20, "misaligned")
    assert torch.equal(gx2, gx) and torch.equal(gw2, gw)
    gx3, gw3 = _entries(case, -20, "strided")
    assert torch.equal(gx3, gx) and torch.equal(gw3, gw)


def _node(case, relu, gy):
    """One forward + backward of the node on the case's layer: (y, gx, gw, gb)."""
    from dkt_stereo_amd import conv
    lay = _layer(case)
    x = S.inputs(case)[0].to(DEV).requires_grad_(True)
    y = conv.conv2d_autograd(x, lay, relu=relu)
    assert type(y.grad_fn).__name__ == NODE
    return (y.detach(),) + torch.autograd.grad(y, [x, lay.weight, lay.bias], grad_outputs=gy)


@pytest.mark.parametrize("case", S.CASES, ids=S.CASE_IDS)
def test_scale_equivariance_bit_for_bit(case):
    """gy * 2^m gives gx * 2^m, gw * 2^m and gb * 2^m bit for bit."""
    gy0 = S.inputs(case)[3].to(DEV)
    _, gx0, gw0, gb0 = _node(case, True, gy0)
    for m in S.KS[1:]:
        s = 2.0 ** m
        _, gx, gw, gb = _node(case, True, gy0 * s)
        assert torch.equal(gx, gx0 * s) and torch.equal(gw, gw0 * s) and torch.equal(gb, gb0 * s), (case, m)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", S.CASES, ids=S.CASE_IDS)
def test_node_on_a_stride2_layer(case, relu):
    """conv2d_autograd on a stride-2 nn.Conv2d: the HIP node, the forward of conv2d bit for bit, gradients inside the bounds."""
    from dkt_stereo_amd import conv
    B, H, W, k, cin, cout = case
    x, w, b, gy, _ = S.inputs(case)
    with torch.no_grad():
        y0 = conv.conv2d(x.to(DEV), _layer(case), relu=relu)
    gy = gy * 2.0 ** -20
    y, gx, gw, gb = _node(case, relu, gy.to(DEV))
    assert torch.equal(y, y0)
    gp = S.R.mask(gy, y0.cpu() if relu else None)
    e_gx = S.gx_error(gx.cpu(), S.truth_gx(gp, w, (H, W)))
    want_gw = S.truth_gw(x, gp, k)
    e_a = S.a_error(gw.cpu(), want_gw)
    ok_b, r_b = S.b_ratio(gw.cpu(), want_gw, S.b_bound(x, gp, k))
    d_gb = (gb.double().cpu() - gp.double().sum(dim=(0, 2, 3))).abs()
    print("case %s relu=%d: gx %.2e  gw (a) %.2e (b) ratio %.3f" % (case, relu, e_gx, e_a, r_b))
    assert e_gx <= S.GX_BOUND and e_a <= S.A_BOUND and ok_b
    assert bool((d_gb <= S.R.gb_bound(gp)).all())


def test_packs_once_per_orientation(monkeypatch):
    from dkt_stereo_amd import conv
    torch.manual_seed(5)
    lay = nn.Conv2d(40, 48, 3, stride=2, padding=1).to(DEV)
    x0 = torch.randn(1, 40, 13, 20, device=DEV)
    gy = torch.randn(1, 48, 7, 10, device=DEV)
    count = _PackCounter(monkeypatch)

    def step():
        x = x0.clone().requires_grad_(True)
        return torch.autograd.grad(conv.conv2d_autograd(x, lay, relu=True), [x, lay.weight, lay.bias], grad_outputs=gy)
    for _ in range(3):
        step()
    assert 1 <= count.n <= 2, count.n                      # the forward image and the transposed one
    with torch.no_grad():
        lay.weight.add_(0.05 * torch.randn_like(lay.weight))
    before = count.n
    gx = step()[0]
    assert 1 <= count.n - before <= 2
    with torch.no_grad():
        y = conv.conv2d(x0, lay, relu=True)
    gp = S.R.mask(gy.cpu(), y.cpu())
    want = S.truth_gx(gp, lay.weight.detach().cpu(), (13, 20))
    assert S.gx_error(gx.cpu(), want) <= S.GX_BOUND        # the gradient of the NEW weight
    step()
    assert count.n - before <= 2


def test_no_host_sync_after_warm_up():
    from dkt_stereo_amd import conv
    torch.manual_seed(7)
    lay = nn.Conv2d(40, 48, 3, stride=2, padding=1).to(DEV)
    proj = nn.Conv2d(48, 24, 1, stride=2).to(DEV)
    x0 = torch.randn(2, 40, 13, 20, device=DEV)
    gy = torch.randn(2, 24, 4, 5, device=DEV) * 2.0 ** -20

    def step():
        x = x0.clone().requires_grad_(True)
        y = conv.conv2d_autograd(conv.conv2d_autograd(x, lay, relu=True), proj)
        assert type(y.grad_fn).__name__ == NODE
        return torch.autograd.grad(y, [x, lay.weight, lay.bias, proj.weight, proj.bias], grad_outputs=gy)
    want = step()
    torch.cuda.synchronize()
    with _NoSync() as ns:
        got = step()
    print("host synchronisations looked for with %s: %d" % (ns.mode, ns.count))
    assert ns.count == 0
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def _tensors(out):
    if torch.is_tensor(out):
        return [out]
    return [t for o in out for t in _tensors(o)]


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


@pytest.mark.parametrize("which", ["fnet", "cnet"])
def test_encoder_wiring(monkeypatch, which):
    """BasicEncoder(norm_fn='instance', downsample=2) / MultiBasicEncoder(norm_fn='batch', downsample=2) in eval() with every
    weight trainable at 2 x 3 x 32 x 64: with the handle on every convolution is the HIP node; outputs agree with the
    handle-off (nn.Conv2d) run to the tolerance of test_gpu_norm_train.py::test_encoder_wiring (1e-5), parameter gradients to
    5e-4 -- compared at the first of WIRING_SEEDS at which both forwards took the same ReLU masks: two fp32 encoders that
    put one activation on different sides of 0 differ by 1e-2 in these gradients."""
    from dkt_stereo_amd import extractor
    x = torch.from_numpy(_synth.uniform((2, 3, 32, 64), -1.0, 1.0, 21, "image")).contiguous().to(DEV)
    masks, nodes = [], []
    inner = {n: getattr(extractor, n) for n in ("norm_act", "norm_add_relu", "add_relu")}

    def spy(name, takes_relu):
        def f(*a, **k):
            y = inner[name](*a, **k)
            if not takes_relu or (a[2] if len(a) > 2 else k.get("relu")):
                masks.append((y > 0).detach())
            return y
        return f
    monkeypatch.setattr(extractor, "norm_act", spy("norm_act", True))
    monkeypatch.setattr(extractor, "norm_add_relu", spy("norm_add_relu", False))
    monkeypatch.setattr(extractor, "add_relu", spy("add_relu", False))
    conv_fwd = extractor._Conv2d.forward

    def spy_conv(self, t):
        y = conv_fwd(self, t)
        nodes.append(type(y.grad_fn).__name__)
        return y
    monkeypatch.setattr(extractor._Conv2d, "forward", spy_conv)
    for seed in WIRING_SEEDS:
        torch.manual_seed(seed)
        if which == "fnet":
            net = extractor.BasicEncoder(output_dim=128, norm_fn="instance", downsample=2)
        else:
            net = extractor.MultiBasicEncoder(output_dim=[[128] * 3, [128] * 3], norm_fn="batch", downsample=2)
        net = net.to(DEV).eval()
        params = list(net.parameters())
        assert all(p.requires_grad for p in params)
        n_convs = sum(isinstance(m, extractor._Conv2d) for m in net.modules())
        runs = {}
        for handle in (True, False):
            monkeypatch.setattr(extractor, "TRAIN_CONV_NODES", handle)
            del masks[:], nodes[:]
            outs = _tensors(net(x))
            gen = torch.Generator().manual_seed(3)
            loss = sum((o * torch.randn(o.shape, generator=gen).to(DEV)).sum() for o in outs)
            grads = torch.autograd.grad(loss, params, allow_unused=True)
            runs[handle] = ([o.detach() for o in outs], grads, list(masks), list(nodes))
        assert len(runs[True][3]) == n_convs and all(n == NODE for n in runs[True][3]), runs[True][3]
        assert len(runs[False][3]) == n_convs and NODE not in runs[False][3], runs[False][3]
        err = max(_rel(a, b) for a, b in zip(runs[True][0], runs[False][0]))
        assert [m.shape for m in runs[True][2]] == [m.shape for m in runs[False][2]] and runs[True][2]
        flips = sum(int((p != q).sum()) for p, q in zip(runs[True][2], runs[False][2]))
        print("%s seed %d: forward, nodes against torch %.2e, activations of different sign %d" % (which, seed, err, flips))
        assert err <= 1e-5, (seed, err)
        if flips == 0:
            break
    else:
        raise AssertionError("no draw of WIRING_SEEDS at which the two forwards take the same ReLU masks")
    # A bias in front of an affine-free instance norm has a gradient of exactly 0: both runs return rounding residue for it,
    # held to 5e-4 of the scale of the layer's weight gradient (test_gpu_norm_train.py::test_encoder_wiring's rule).
    named = dict(zip((n for n, _ in net.named_parameters()), zip(runs[True][1], runs[False][1])))
    errs = {}
    for n, (a, b) in named.items():
        assert (a is None) == (b is None), n
        if a is None:
            continue
        if which == "fnet" and n.endswith(".bias") and n != "conv2.bias":
            errs[n] = float((a.double() - b.double()).abs().max()) / float(named[n[:-4] + "weight"][1].abs().max())
        else:
            errs[n] = _rel(a, b)
        print("  %-36s %.2e" % (n, errs[n]))
    assert max(errs.values()) <= 5e-4, {n: e for n, e in errs.items() if e > 5e-4}
    with torch.no_grad():                                   # without autograd nothing changes: the inference kernels
        monkeypatch.setattr(extractor, "TRAIN_CONV_NODES", True)
        on = _tensors(net(x))
        monkeypatch.setattr(extractor, "TRAIN_CONV_NODES", False)
        assert all(torch.equal(a, b) and a.grad_fn is None for a, b in zip(on, _tensors(net(x))))
