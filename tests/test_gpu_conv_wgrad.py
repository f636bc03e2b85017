"""The weight gradient of conv.conv2d_autograd on dkt_conv2d_wgrad (csrc/conv_wgrad.hip), -m gpu: the entry and the node's gw
against the fp64 truth and BOTH bounds of _conv_wgrad_ref.py at upstream gradients of magnitude 2^0, 2^-20, 2^-40 and 2^+20.

What the cases cover under the kernel's plan (_conv_wgrad_ref.plan; 64 x 64 channel blocks, 2 x 32 pixel tiles):
  three or more K-slices of one weight    2x24x40 (two bands of 12 rows x B = 2: four slices), 3x7x9 (B = 3: three slices)
  two or more output-channel blocks       z|r 384 -> 256 (four)
  two or more input-channel blocks        z|r 384 -> 256 (six), 3x7x9 1x1 130 -> 3 (three, the last 2 channels wide)
  channel tails                           64 -> 2, 33 -> 5, 36 -> 64, 130 -> 3, 48 -> 40
  pixel tails                             W = 37, 35, 70 (column tiles that end inside the image), H = 33, 9, 5, 7 (a tile row
                                          past the band), 1x1x1
  the 4-byte path                         odd W, and every "misaligned" layout

Every case prints its figures (run with -s)."""
import functools

import pytest
import torch
import torch.nn as nn

import _conv_grad_ref as R
import _conv_wgrad_ref as WR
import _synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _layer(case):
    B, H, W, k, cin, cout = case
    _, w, b, _ = WR.inputs(case)
    lay = nn.Conv2d(cin, cout, k, padding=k // 2)
    with torch.no_grad():
        lay.weight.copy_(w)
        lay.bias.copy_(b)
    return lay.to(DEV)


def _node_gw(case, relu, gy, x=None):
    from dkt_stereo_amd import conv
    lay = _layer(case)
    x = WR.inputs(case)[0].to(DEV) if x is None else x
    y = conv.conv2d_autograd(x, lay, relu=relu)
    return torch.autograd.grad(y, [lay.weight], grad_outputs=gy)[0]


@functools.lru_cache(maxsize=None)
def _ref(case, relu):
    """g' (the mask comes from the deterministic forward), the fp64 truth and the bound (b) at k = 0, computed once: a
    power-of-two multiple of the upstream gradient gives that multiple of all three exactly."""
    from dkt_stereo_amd import conv
    x, w, b, gy0 = WR.inputs(case)
    k = case[3]
    y = None
    if relu:
        with torch.no_grad():
            y = conv.conv2d(x.to(DEV), _layer(case), relu=True).cpu()
    gp = R.mask(gy0, y)
    return gp, WR.truth(x, gp, k), WR.b_bound(x, gp, k)


def _held(got, exact, bound, what):
    ea = WR.a_error(got.cpu(), exact)
    ok, rb = WR.b_ratio(got.cpu(), exact, bound)
    print("%s: (a) %.2e  (b) |d|/bound %.2e" % (what, ea, rb))
    assert ea <= WR.A_BOUND, (what, ea)
    assert ok, (what, rb)


@pytest.mark.parametrize("k", WR.KS)
@pytest.mark.parametrize("layout", WR.LAYOUTS)
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", WR.CASES, ids=WR.CASE_IDS)
def test_entry_and_node_against_truth(case, relu, layout, k):
    from dkt_stereo_amd import conv
    gp, exact, bound = _ref(case, relu)
    s = 2.0 ** k
    # the entry: g' in the layout, x a channel slice of a wider buffer
    g = R.laid_out(gp * s, layout, DEV)
    x = R.laid_out(WR.inputs(case)[0], "strided", DEV)
    scale = R.scale_pair(float((gp * s).abs().max())).to(DEV)
    got = conv.conv2d_wgrad(x, g, scale, case[3])
    _held(got, exact * s, bound * s, "entry %s relu=%d %s k=%d" % (case, relu, layout, k))
    # the node: the upstream gradient in the layout
    gy = R.laid_out(WR.inputs(case)[3] * s, layout, DEV)
    got_n = _node_gw(case, relu, gy)
    _held(got_n, exact * s, bound * s, "node  %s relu=%d %s k=%d" % (case, relu, layout, k))
    # the order of every sum is a function of the shape alone: the 16-byte and the 4-byte path give the same bits
    assert torch.equal(got_n, got)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", WR.CASES, ids=WR.CASE_IDS)
def test_scale_equivariance_and_run_to_run_bits(case, relu):
    gy0 = WR.inputs(case)[3].to(DEV)
    gw0 = _node_gw(case, relu, gy0)
    for _ in range(2):                                               # three runs in all
        assert torch.equal(_node_gw(case, relu, gy0), gw0)
    for k in WR.KS[1:]:
        s = 2.0 ** k
        assert torch.equal(_node_gw(case, relu, gy0 * s), gw0 * s), (case, relu, k)


@pytest.mark.parametrize("case", [WR.CASES[1], WR.CASES[7]], ids=[WR.CASE_IDS[1], WR.CASE_IDS[7]])
def test_non_finite_in_non_finite_out(case):
    from dkt_stereo_amd import conv
    gy = WR.inputs(case)[3].to(DEV).clone()
    gy.view(-1)[gy.numel() // 2] = float("nan")
    assert not bool(torch.isfinite(_node_gw(case, False, gy)).all())
    x = WR.inputs(case)[0].to(DEV).clone()
    x.view(-1)[x.numel() // 3] = float("inf")
    g = WR.inputs(case)[3].to(DEV)
    got = conv.conv2d_wgrad(x, g, R.scale_pair(float(g.abs().max())).to(DEV), case[3])
    assert not bool(torch.isfinite(got).all())
    # an all-zero gradient (pair {1, 1}) gives zeros
    assert not _node_gw(case, False, torch.zeros_like(gy)).any()


def test_merged_zr_parts_get_their_slices():
    from dkt_stereo_amd import conv
    from dkt_stereo_amd.update import ConvGRU
    torch.manual_seed(11)
    gru = ConvGRU(32, 40).to(DEV)
    x = torch.randn(2, 72, 12, 20, device=DEV)
    gy = torch.randn(2, 64, 12, 20, device=DEV)
    y = conv.conv2d_autograd(x, (gru.convz, gru.convr), owner=gru._merged_zr())
    gz, gr = torch.autograd.grad(y, [gru.convz.weight, gru.convr.weight], grad_outputs=gy)
    exact = WR.truth(x.cpu(), gy.cpu(), 3)
    bound = WR.b_bound(x.cpu(), gy.cpu(), 3)
    assert gz.shape == gru.convz.weight.shape and gr.shape == gru.convr.weight.shape
    _held(torch.cat([gz, gr], 0), exact, bound, "z|r 72 -> 32 | 32")
    _held(gz, exact[:32], bound[:32], "z")
    _held(gr, exact[32:], bound[32:], "r")


def test_vendor_weight_gradient_is_not_called_for_1x1_and_3x3(monkeypatch):
    """torch.nn.grad.conv2d_weight raises: a backward through a 3x3 and a 1x1 layer succeeds, through a 7x7 layer raises."""
    from dkt_stereo_amd import conv

    def refuse(*a, **k):
        raise AssertionError("torch.nn.grad.conv2d_weight was called")
    monkeypatch.setattr(torch.nn.grad, "conv2d_weight", refuse)
    torch.manual_seed(12)
    x = torch.randn(1, 8, 10, 14, device=DEV)
    for k in (3, 1):
        lay = nn.Conv2d(8, 6, k, padding=k // 2).to(DEV)
        gw, gb = torch.autograd.grad(conv.conv2d_autograd(x, lay, relu=True).sum(), [lay.weight, lay.bias])
        assert bool(torch.isfinite(gw).all()) and gw.shape == lay.weight.shape
    lay7 = nn.Conv2d(8, 6, 7, padding=3).to(DEV)
    y = conv.conv2d_autograd(x, lay7, relu=True)
    with pytest.raises(AssertionError, match="conv2d_weight was called"):
        torch.autograd.grad(y.sum(), [lay7.weight])


def test_no_host_sync_after_warm_up():
    from dkt_stereo_amd import conv
    torch.manual_seed(7)
    lay = nn.Conv2d(40, 48, 3, padding=1).to(DEV)
    head = nn.Conv2d(48, 2, 1).to(DEV)
    x0 = torch.randn(2, 40, 12, 20, device=DEV)
    gy = torch.randn(2, 2, 12, 20, device=DEV) * 2.0 ** -20

    def step():
        x = x0.clone().requires_grad_(True)
        y = conv.conv2d_autograd(conv.conv2d_autograd(x, lay, relu=True), head)
        return torch.autograd.grad(y, [x, lay.weight, lay.bias, head.weight, head.bias], grad_outputs=gy)
    want = step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("relu", [False, True])
def test_handle_off_is_the_vendor_call_on_the_same_gradient(monkeypatch, relu):
    """GRAD_WEIGHT_HIP = False: gw IS the result of torch.nn.grad.conv2d_weight(x, shape, g', stride 1, padding 1).  The vendor
    kernel does not repeat its own bits from one call to the next (printed below), so torch.equal is taken with the result of
    the call the node made -- recorded together with its arguments, which are compared bit for bit -- and a second call on
    the same arguments is held to the 2e-6 test_gpu_conv_grad.py uses for this kernel."""
    from dkt_stereo_amd import conv
    case = WR.CASES[1]
    lay = _layer(case)
    x = WR.inputs(case)[0].to(DEV)
    gy = WR.inputs(case)[3].to(DEV)
    real, seen = torch.nn.grad.conv2d_weight, []

    def recorded(*a, **k):
        seen.append((a, k, real(*a, **k)))
        return seen[-1][2]
    monkeypatch.setattr(torch.nn.grad, "conv2d_weight", recorded)
    monkeypatch.setattr(conv, "GRAD_WEIGHT_HIP", False)
    y = conv.conv2d_autograd(x, lay, relu=relu)
    gw = torch.autograd.grad(y, [lay.weight], grad_outputs=gy)[0]
    g = gy * (y.detach() > 0) if relu else gy
    assert len(seen) == 1
    (sx, sshape, sg), kw, res = seen[0]
    assert torch.equal(gw, res)
    assert torch.equal(sx, x) and torch.equal(sg, g) and tuple(sshape) == tuple(lay.weight.shape)
    assert kw == dict(stride=1, padding=(1, 1))
    again = [real(x, lay.weight.shape, g, stride=1, padding=(1, 1)) for _ in range(2)]
    print("vendor call repeats its bits: %s; node against a second call: rel %.2e" % (torch.equal(*again), _rel(gw, again[0])))
    assert _rel(gw, again[0]) <= 2e-6
    monkeypatch.setattr(conv, "GRAD_WEIGHT_HIP", True)
    del seen[:]
    hip = _node_gw(case, relu, gy)
    assert not seen and _rel(hip, again[0]) <= 2 * WR.A_BOUND


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def test_update_block_parameter_gradients(monkeypatch):
    """BasicMultiUpdateBlock (RAFT) at the shape of test_gpu_conv_grad.py: every parameter gradient with the handle on is
    within (a) of the handle-off run; at a 2^-20 loss scale the weight gradients are 2^-20 times the unscaled ones bit for bit."""
    from types import SimpleNamespace
    from dkt_stereo_amd import conv
    from dkt_stereo_amd.update import BasicMultiUpdateBlock
    cfg = dict(corr_levels=4, corr_radius=4, n_downsample=2, n_gru_layers=3, hidden_dims=[128, 128, 128], slow_fast_gru=False)
    blk = BasicMultiUpdateBlock(SimpleNamespace(**cfg), hidden_dims=cfg["hidden_dims"])
    blk.load_state_dict(_synth.torch_state_dict(_synth.shapes_of(blk), 21))
    blk.to(DEV)
    H, W = 16, 24
    torch.manual_seed(8)
    net0 = [torch.tanh(torch.randn(1, 128, H >> i, W >> i)).to(DEV) for i in range(3)]
    inp = [[0.5 * torch.randn(1, 128, H >> i, W >> i).to(DEV) for _ in range(3)] for i in range(3)]
    corr = torch.randn(1, 36, H, W).to(DEV)
    flow = torch.randn(1, 2, H, W).to(DEV)
    wts = [torch.randn(1, 128, H >> i, W >> i).to(DEV) for i in range(3)]
    wd, wm = torch.randn(1, 2, H, W).to(DEV), torch.randn(1, 144, H, W).to(DEV)
    names, params = zip(*blk.named_parameters())

    def grads(scale):
        net, mask, delta = blk([t.clone() for t in net0], inp, corr, flow=flow)
        loss = sum((n * w).sum() for n, w in zip(net, wts)) + (delta * wd).sum() + (mask * wm).sum()
        got = torch.autograd.grad(loss * scale, params, allow_unused=True)
        return {n: g for n, g in zip(names, got) if g is not None}
    on = grads(1.0)
    small = grads(2.0 ** -20)
    monkeypatch.setattr(conv, "GRAD_WEIGHT_HIP", False)
    off = grads(1.0)
    assert set(on) == set(off) and any(n.endswith(".weight") for n in on)
    for n in on:
        err = _rel(on[n], off[n])
        print("%s: rel %.2e" % (n, err))
        assert err <= WR.A_BOUND, (n, err)
    # (the classes conv.WGRAD_VENDOR_CLASSES leaves on the vendor kernel, which does not repeat its own bits, are not held to this)
    hip = [n for n in on if n.endswith(".weight") and on[n].shape[-1] in (1, 3)
           and (on[n].shape[1], on[n].shape[0], on[n].shape[-1]) not in conv.WGRAD_VENDOR_CLASSES]
    assert len(hip) >= 12
    for n in hip:
        assert torch.equal(small[n], on[n] * 2.0 ** -20), n
