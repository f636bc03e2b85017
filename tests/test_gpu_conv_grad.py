"""The backward of conv.conv2d_autograd (-m gpu): the pre-pass (csrc/conv_grad.hip), the device-scaled input-gradient
convolution (dkt_conv_desc.dscale) and the owner-held packed images, against the fp64 truth and the bounds of
_conv_grad_ref.py at upstream gradients of magnitude 2^0, 2^-20, 2^-40 and 2^+20.

Every case prints its figures (run with -s).  Host synchronisations are looked for with
torch.cuda.set_sync_debug_mode("error") where the build honours it (probed with a .item() that has to raise), else by
counting Tensor.item / __float__ / tolist / cpu; the test prints which one it used."""
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

import _conv_grad_ref as R
import _synth
from test_host_conv2d_tile import DSCALE, tile

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


#: the tile of each case's input-gradient convolution (Cout -> Cin channels, device-scaled form), as dkt_conv2d_f16s_tile names
#: it: the 32-channel head tile, the 64-channel four-row tile (3x3 and 1x1, and of a 2-channel gradient), 256 channels x 1 row
DGRAD_TILES = dict(zip(R.CASES, [(0, 1, 1, 4, 1, 1, 1, 2), (0, 3, 1, 4, 1, 2, 1, 2), (0, 1, 1, 4, 1, 2, 1, 2), (0, 3, 1, 4, 1, 2, 1, 2),
                                 (0, 3, 4, 1, 1, 2, 1, 2)]))


@functools.lru_cache(maxsize=None)
def _layer(case):
    B, H, W, k, cin, cout = case
    x, w, b, _ = R.inputs(case)
    lay = nn.Conv2d(cin, cout, k, padding=k // 2)
    with torch.no_grad():
        lay.weight.copy_(w)
        lay.bias.copy_(b)
    return lay.to(DEV)


def _node(case, relu, gy, needs=(True, True, True)):
    """One forward + backward of the node: (y, gx, gw, gb), None for what `needs` leaves out."""
    from dkt_stereo_amd import conv
    lay = _layer(case)
    x = R.inputs(case)[0].to(DEV).requires_grad_(needs[0])
    lay.weight.requires_grad_(needs[1])
    lay.bias.requires_grad_(needs[2])
    try:
        y = conv.conv2d_autograd(x, lay, relu=relu)
        wanted = [t for t, n in zip((x, lay.weight, lay.bias), needs) if n]
        grads = iter(torch.autograd.grad(y, wanted, grad_outputs=gy))
        return (y.detach(),) + tuple(next(grads) if n else None for n in needs)
    finally:
        lay.weight.requires_grad_(True)
        lay.bias.requires_grad_(True)


@functools.lru_cache(maxsize=None)
def _ref(case, relu):
    """The saved output of the case (the forward is deterministic) and the fp64 truth at k = 0, computed once: a power-of-two
    multiple of the upstream gradient gives that multiple of g', gb and gx exactly."""
    from dkt_stereo_amd import conv
    x, w, b, gy0 = R.inputs(case)
    with torch.no_grad():
        y = conv.conv2d(x.to(DEV), _layer(case), relu=relu).cpu()
    gp, gb, gx = R.truth(gy0, y if relu else None, w)
    gw = torch.nn.grad.conv2d_weight(x.double(), w.shape, gp.double(), padding=w.shape[2] // 2)
    return y, gp, gb, gx, gw


def _within_gb_bound(got, exact, gp):
    d = (got.double().cpu() - exact).abs()
    bound = R.gb_bound(gp)
    return bool((d <= bound).all()), float((d / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize("k", R.KS)
@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_node_against_truth(case, relu, layout, k):
    y0, gp, gb, gx, gw = _ref(case, relu)
    s = 2.0 ** k
    gy = R.laid_out(R.inputs(case)[3] * s, layout, DEV)
    B, H, W, ks, cin, cout = case
    assert tile(ks, 1, 3, cin, (cout,), 0, B, H, W, DSCALE) == DGRAD_TILES[case]
    y, got_gx, got_gw, got_gb = _node(case, relu, gy)
    assert torch.equal(y.cpu(), y0)
    e_gx = R.gx_error(got_gx.cpu(), gx * s)
    ok_gb, r_gb = _within_gb_bound(got_gb, gb * s, gp * s)
    e_gw = R.gx_error(got_gw.cpu(), gw * s)
    print("case %s relu=%d %s k=%d: gx rel %.2e  gb |d|/bound %.2e  gw rel %.2e" % (case, relu, layout, k, e_gx, r_gb, e_gw))
    assert e_gx <= R.GX_BOUND
    assert ok_gb
    assert e_gw <= 2e-5            # the vendor weight gradient fed with g' (test_conv2d_autograd_matches_torch's figure)


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_prepass_against_truth(case, relu, layout):
    """dkt_conv_grad_prepass alone: g' exact, gb inside the bound, the scale pair exact -- at every magnitude, with y
    in the same layout as gy."""
    from dkt_stereo_amd import conv
    y0, gp, gb, _, _ = _ref(case, relu)
    y = R.laid_out(y0, layout, DEV) if relu else None
    for k in R.KS:
        s = 2.0 ** k
        gy = R.laid_out(R.inputs(case)[3] * s, layout, DEV)
        g, got_gb, scale = conv.conv_grad_prepass(gy, y, want_bias=True)
        if relu:
            assert g.is_contiguous() and torch.equal(g.cpu(), gp * s)
        else:
            assert g.data_ptr() == gy.data_ptr()                      # nothing copied: the convolution reads gy in place
        ok, r = _within_gb_bound(got_gb, gb * s, gp * s)
        print("case %s relu=%d %s k=%d: gb |d|/bound %.2e  scale %s" % (case, relu, layout, k, r, scale.tolist()))
        assert ok
        assert torch.equal(scale.cpu(), R.scale_pair(float((gp * s).abs().max())))
        _, none_gb, scale2 = conv.conv_grad_prepass(gy, y, want_bias=False)
        assert none_gb is None and torch.equal(scale2, scale)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_scale_equivariance_bit_for_bit(case, relu):
    """gx(gy * 2^k) == 2^k * gx(gy) and gb(gy * 2^k) == 2^k * gb(gy): the rule gives the same fp16 operands, every other
    factor is a power of two."""
    gy0 = R.inputs(case)[3].to(DEV)
    _, gx0, _, gb0 = _node(case, relu, gy0)
    for k in R.KS[1:]:
        s = 2.0 ** k
        _, gx, _, gb = _node(case, relu, gy0 * s)
        assert torch.equal(gx, gx0 * s), (case, relu, k)
        assert torch.equal(gb, gb0 * s), (case, relu, k)


@pytest.mark.parametrize("case", R.CASES[1:], ids=R.CASE_IDS[1:])
def test_determinism_subsets_and_edge_values(case):
    from dkt_stereo_amd import conv
    y0 = _ref(case, True)[0]
    gy0 = R.inputs(case)[3]
    gy = gy0.to(DEV) * 2.0 ** -20
    _, gx, gw, gb = _node(case, True, gy)
    y_dev = y0.to(DEV)
    gp = conv.conv_grad_prepass(gy, y_dev)[0]
    for _ in range(2):                                               # run-to-run bits
        _, gx2, _, gb2 = _node(case, True, gy)
        assert torch.equal(gx2, gx) and torch.equal(gb2, gb)
        assert torch.equal(conv.conv_grad_prepass(gy, y_dev)[0], gp)
    # the order of the bias sum is a function of the shape alone: the 16-byte and the 4-byte path give the same bits
    for layout in R.LAYOUTS:
        assert torch.equal(_node(case, True, R.laid_out(gy, layout))[3], gb), layout
    # needs_input_grad subsets: the same bits, nothing else computed
    for needs in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        _, sx, sw, sb = _node(case, True, gy, needs)
        assert torch.equal(sx, gx) if needs[0] else sx is None, needs
        assert torch.equal(sb, gb) if needs[2] else sb is None, needs
        assert _rel(sw, gw) <= 2e-6 if needs[1] else sw is None, needs              # (the vendor kernel's order is its own)
    # an all-zero gradient gives zeros (e = 0: the scale pair is {1, 1})
    zero = torch.zeros_like(gy)
    _, zx, zw, zb = _node(case, True, zero)
    assert not zx.any() and not zw.any() and not zb.any()
    assert conv.conv_grad_prepass(zero, y_dev)[2].tolist() == [1.0, 1.0]
    # one Inf where the ReLU passes: a non-finite gx, never a finite one (and e = 0)
    i = int((y0.flatten() > 0).nonzero()[0])
    bad = gy.clone()
    bad.view(-1)[i] = float("inf")
    _, bx, _, _ = _node(case, True, bad)
    assert not bool(torch.isfinite(bx).all())
    assert conv.conv_grad_prepass(bad, y_dev)[2].tolist() == [1.0, 1.0]


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


@pytest.mark.parametrize("igev", [False, True])
def test_update_block_gradients_at_a_small_loss_scale(igev):
    """test_update_block_autograd_matches_oracle's set-up with the loss multiplied by 2^-20: the gradients with respect to
    the hidden states and the correlation features are 2^-20 times those at scale 1 bit for bit; the sampled parameter
    gradients stay within that test's 5e-5 of the fp64 oracle's (the vendor weight gradient has its own order)."""
    from oracle import torch_oracle as to
    from dkt_stereo_amd.update import BasicMultiUpdateBlock, BasicMultiUpdateBlockIGEV
    cfg = dict(corr_levels=2 if igev else 4, corr_radius=4, n_downsample=2, n_gru_layers=3, hidden_dims=[128, 128, 128],
               slow_fast_gru=False)
    cls = BasicMultiUpdateBlockIGEV if igev else BasicMultiUpdateBlock
    blk = cls(SimpleNamespace(**cfg), hidden_dims=cfg["hidden_dims"])
    sd = _synth.torch_state_dict(_synth.shapes_of(blk), 21)
    blk.load_state_dict(sd)
    blk.to(DEV)
    H, W = 16, 24
    torch.manual_seed(8)
    net0 = [torch.tanh(torch.randn(1, 128, H >> i, W >> i)) for i in range(3)]
    inp = [[0.5 * torch.randn(1, 128, H >> i, W >> i) for _ in range(3)] for i in range(3)]
    corr0 = torch.randn(1, 162 if igev else 36, H, W)
    aux = torch.randn(1, 1 if igev else 2, H, W)
    wts = [torch.randn(1, 128, H >> i, W >> i) for i in range(3)]
    wd = torch.randn(1, 1 if igev else 2, H, W)
    wm = torch.randn(1, 32 if igev else 144, H, W)
    names = ["encoder.convc1.weight", "encoder.conv.bias", ("gru04" if igev else "gru08") + ".convz.weight",
             ("gru08" if igev else "gru16") + ".convq.weight", ("gru16" if igev else "gru32") + ".convr.bias",
             ("disp_head" if igev else "flow_head") + ".conv2.weight", ("mask_feat_4.0" if igev else "mask.0") + ".weight"]
    S = 2.0 ** -20

    def loss_of(net, mask, delta, to_dev):
        t = lambda a: a.to(to_dev)
        return sum((n * t(w)).sum() for n, w in zip(net, wts)) + (delta * t(wd)).sum() + (mask * t(wm)).sum()

    params = dict(blk.named_parameters())
    kw = dict(disp=aux.to(DEV)) if igev else dict(flow=aux.to(DEV))
    got = {}
    for scale in (1.0, S):
        net_g = [t.to(DEV).requires_grad_(True) for t in net0]
        corr_g = corr0.to(DEV).requires_grad_(True)
        net, mask, delta = blk(list(net_g), [[t.to(DEV) for t in s] for s in inp], corr_g, **kw)
        got[scale] = torch.autograd.grad(loss_of(net, mask, delta, DEV) * scale, net_g + [corr_g] + [params[n] for n in names])
    for name, a, b in zip(["net0", "net1", "net2", "corr"], got[S], got[1.0]):
        assert torch.equal(a, b * S), name
    sdd = {("ub." + k): v.double().requires_grad_(True) for k, v in sd.items()}
    net_c = [t.double().requires_grad_(True) for t in net0]
    corr_c = corr0.double().requires_grad_(True)
    o_net, o_mask, o_delta = to.update_block(sdd, "ub", 3, list(net_c), [[t.double() for t in s] for s in inp], corr_c,
                                             aux.double(), igev=igev)
    want = torch.autograd.grad(loss_of(o_net, o_mask, o_delta, "cpu"), net_c + [corr_c] + [sdd["ub." + n] for n in names])
    for name, a, b in zip(["net0", "net1", "net2", "corr"] + names, got[S], want):
        err = _rel(a.cpu(), b * S)
        print("%s %s: rel %.2e" % ("igev" if igev else "raft", name, err))
        assert err <= 5e-5, (name, err)


class _PackCounter:
    def __init__(self, monkeypatch):
        from dkt_stereo_amd import _ffi
        L = _ffi.lib()
        self.n, real = 0, L.dkt_conv2d_pack_weights

        def counted(*a):
            self.n += 1
            return real(*a)
        monkeypatch.setattr(L, "dkt_conv2d_pack_weights", counted)


def test_one_layer_packs_once_per_orientation(monkeypatch):
    from dkt_stereo_amd import conv
    torch.manual_seed(5)
    lay = nn.Conv2d(40, 48, 3, padding=1).to(DEV)
    x0 = torch.randn(1, 40, 12, 20, device=DEV)
    gy = torch.randn(1, 48, 12, 20, device=DEV)
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
    _, _, want = R.truth(gy.cpu(), y.cpu(), lay.weight.detach().cpu())
    assert R.gx_error(gx.cpu(), want) <= R.GX_BOUND        # the gradient of the NEW weight
    step()
    assert count.n - before <= 2


def test_gru_packs_once_per_orientation(monkeypatch):
    from dkt_stereo_amd.update import BasicMultiUpdateBlock, ConvGRU
    torch.manual_seed(6)
    gru = ConvGRU(64, 64).to(DEV)
    h0 = torch.tanh(torch.randn(1, 64, 12, 20, device=DEV))
    xs = torch.randn(1, 64, 12, 20, device=DEV)
    cz, cr, cq = (torch.randn(1, 64, 12, 20, device=DEV) for _ in range(3))
    count = _PackCounter(monkeypatch)

    def step():
        h = h0.clone().requires_grad_(True)
        out = BasicMultiUpdateBlock._gru_autograd(gru, h, cz, cr, cq, xs)
        return torch.autograd.grad(out.sum(), [h] + list(gru.parameters()))
    first = step()
    for _ in range(2):
        again = step()
    assert torch.equal(first[0], again[0])
    assert 2 <= count.n <= 4, count.n                      # z|r and q, two orientations each
    with torch.no_grad():
        gru.convz.weight.add_(0.05)
    before = count.n
    step()
    step()
    assert 1 <= count.n - before <= 2                      # z|r alone is repacked, once per orientation


class _NoSync:
    """Raises (sync debug mode) or counts (patched readers) host synchronisations inside the block."""

    def __enter__(self):
        self.count, self.mode = 0, None
        torch.cuda.set_sync_debug_mode("error")
        try:
            torch.ones(1, device=DEV).item()
        except RuntimeError:
            self.mode = "torch.cuda.set_sync_debug_mode('error')"
            return self
        torch.cuda.set_sync_debug_mode("default")
        self.mode = "patched Tensor.item / __float__ / tolist / cpu"
        self.saved = {n: getattr(torch.Tensor, n) for n in ("item", "__float__", "tolist", "cpu")}
        for n, fn in self.saved.items():
            def counting(t, *a, _fn=fn, **k):
                self.count += int(t.is_cuda)
                return _fn(t, *a, **k)
            setattr(torch.Tensor, n, counting)
        return self

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode("default")
        for n, fn in getattr(self, "saved", {}).items():
            setattr(torch.Tensor, n, fn)
        return False


def test_no_host_sync_after_warm_up():
    from dkt_stereo_amd import conv
    torch.manual_seed(7)
    lay = nn.Conv2d(40, 48, 3, padding=1).to(DEV)
    head = nn.Conv2d(48, 2, 3, padding=1).to(DEV)          # its forward runs on the direct kernel: no forward image to borrow a scale from
    x0 = torch.randn(2, 40, 12, 20, device=DEV)
    gy = torch.randn(2, 2, 12, 20, device=DEV) * 2.0 ** -20

    def step():
        x = x0.clone().requires_grad_(True)
        y = conv.conv2d_autograd(conv.conv2d_autograd(x, lay, relu=True), head)
        return torch.autograd.grad(y, [x, lay.weight, lay.bias, head.weight, head.bias], grad_outputs=gy)
    want = step()
    torch.cuda.synchronize()
    with _NoSync() as ns:
        got = step()
    print("host synchronisations looked for with %s: %d" % (ns.mode, ns.count))
    assert ns.count == 0
    assert all(torch.equal(got[i], want[i]) for i in (0, 2, 4))          # gx and the bias gradients: this library's kernels
    assert all(_rel(got[i], want[i]) <= 2e-6 for i in (1, 3))            # the vendor weight gradients


@pytest.mark.parametrize("relu", [False, True])
def test_grad_prepass_off_is_the_previous_sequence(monkeypatch, relu):
    """GRAD_PREPASS = False: multiply by (y > 0), the convolution at in_scale = 1 on a weight packed for the call, the vendor
    weight gradient, a torch sum -- bit for bit."""
    from dkt_stereo_amd import conv
    case = R.CASES[1]
    lay = _layer(case)
    gy = R.inputs(case)[3].to(DEV)
    monkeypatch.setattr(conv, "GRAD_PREPASS", False)
    x = R.inputs(case)[0].to(DEV).requires_grad_(True)
    y = conv.conv2d_autograd(x, lay, relu=relu)
    assert type(y.grad_fn).__name__ == "_Conv2dFnBackward"
    gx, gw, gb = torch.autograd.grad(y, [x, lay.weight, lay.bias], grad_outputs=gy)
    with torch.no_grad():
        g = gy * (y > 0) if relu else gy
        wt = lay.weight.detach().transpose(0, 1).flip(2, 3).contiguous()
        want_gx = conv.conv2d(g, conv._LayerShim(wt, None, (1, 1)))
        want_gw = torch.nn.grad.conv2d_weight(x.detach(), lay.weight.shape, g, stride=1, padding=(1, 1))
    assert torch.equal(gx, want_gx) and _rel(gw, want_gw) <= 2e-6 and torch.equal(gb, g.sum(dim=(0, 2, 3)))
    monkeypatch.setattr(conv, "GRAD_PREPASS", True)
    y = conv.conv2d_autograd(x, lay, relu=relu)
    assert type(y.grad_fn).__name__ == "_Conv2dGradFnBackward"
    gx2 = torch.autograd.grad(y, [x], grad_outputs=gy)[0]
    assert _rel(gx2, gx) <= 2 * R.GX_BOUND                 # O(1) gradients: the two paths agree to the last bits
