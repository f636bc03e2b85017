"""-m gpu: the epilogues of conv2d_f16s_kernel (conv.conv2d, conv2d_fused, conv2d_stats, conv2d_pair) where they place
their results: the same three checks tests/test_gpu_conv_epilogues.py makes for conv_c8_kernel.

  * placement: every layer alone, as the first and as the second problem of a pair launch beside a layer of another shape
    and channel count (conv2d_pair; conv2d_fused_pair for the residual epilogue) -- bit for bit equal;
  * a batch against the same layer one batch item at a time -- bit for bit equal (per-tile values: batch base pointers,
    channel-block pointers, the instance-norm parameters of the item);
  * fp64, with the bound tests/test_gpu_round2.py uses for these layers: 1e-5 of the output maximum (max(1, maximum) as there).

Layers: 3x3 64 -> 64 at (2, 64, 40, 72); 3x3 96 -> 96 at (2, 96, 24, 60); 1x1 128 -> 128 at (2, 128, 23, 39); the stride-2
3x3 64 -> 96 at (1, 64, 33, 37).  What the Python side does not offer is not run: in_norm needs a 3x3 layer with 33..128
outputs at stride 1 (the first two), the residual epilogue and pair launches need stride 1 (all but the last).

The statistics of conv2d_stats are sums of fp32 values in an order the tiling decides, so they are compared with fp64 and
not bit for bit: a mean within 1e-5 of the output maximum (the bound round 2 asserts for instance_norm_params), 1 / std
within 2 HW 2^-24 (1 + mean^2 / var) relative -- the worst case of a one-pass fp32 variance over HW values."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

#: name, B, Cin, Cout, k, stride, H, W; partner of a pair launch (Cin, Cout) in the same output-width class
CASES = [("3x3_64", 2, 64, 64, 3, 1, 40, 72, (48, 40)), ("3x3_96", 2, 96, 96, 3, 1, 24, 60, (64, 128)),
         ("1x1_128", 2, 128, 128, 1, 1, 23, 39, (64, 96)), ("3x3_s2_64_96", 1, 64, 96, 3, 2, 33, 37, None)]
IDS = [c[0] for c in CASES]


def _bound(ref):
    return 1e-5 * max(1.0, float(ref.abs().max()))


def _setup(case, seed):
    name, B, cin, cout, k, stride, H, W, partner = case
    torch.manual_seed(seed)
    g = torch.Generator(device=DEV).manual_seed(seed)
    layer = torch.nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2).to(DEV)
    x = torch.randn((B, cin, H, W), device=DEV, generator=g) * 1.5 + 0.3
    other = None
    if partner is not None:
        other = (torch.randn((3 - B, partner[0], 20, 45), device=DEV, generator=g),
                 torch.nn.Conv2d(partner[0], partner[1], k, padding=k // 2).to(DEV))
    return layer, x, other, g


def _ref64(x, layer, relu=False):
    y = F.conv2d(x.double(), layer.weight.double(), layer.bias.double(), stride=layer.stride, padding=layer.padding)
    return y.clamp_min(0) if relu else y


@torch.no_grad()
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_conv2d_alone_in_a_pair_and_item_by_item(case, relu):
    from dkt_stereo_amd import conv
    with conv.use_backend("f16x3"):
        layer, x, other, _ = _setup(case, 11)
        assert conv.hip_eligible(layer)
        alone = conv.conv2d(x, layer, relu=relu)
        ref = _ref64(x, layer, relu)
        assert float((alone.double() - ref).abs().max()) <= _bound(ref)
        for b in range(x.shape[0]):
            assert torch.equal(conv.conv2d(x[b:b + 1], layer, relu=relu)[0], alone[b]), b
        if other is None:
            return
        xo, lo = other
        assert conv.pair_eligible(layer, lo)
        o_alone = conv.conv2d(xo, lo, relu=not relu)
        first, o_second = conv.conv2d_pair((x, layer, relu), (xo, lo, not relu))
        o_first, second = conv.conv2d_pair((xo, lo, not relu), (x, layer, relu))
        assert torch.equal(first, alone) and torch.equal(second, alone)
        assert torch.equal(o_first, o_alone) and torch.equal(o_second, o_alone)


@torch.no_grad()
@pytest.mark.parametrize("case", CASES[:3], ids=IDS[:3])
def test_conv2d_fused_alone_in_a_pair_and_item_by_item(case):
    """The residual epilogue everywhere it is offered, with the instance norm of the input in the staging where that is."""
    from dkt_stereo_amd import conv, extractor
    with conv.use_backend("f16x3"):
        layer, x, other, g = _setup(case, 12)
        B, cin = x.shape[:2]
        res = torch.randn((B, layer.weight.shape[0], *x.shape[2:]), device=DEV, generator=g)
        assert conv.fused_eligible(layer)
        x64 = x.double()
        forms = [(None, x64)]
        if conv.fused_eligible(layer, True):
            params = extractor.instance_norm_params(torch.nn.InstanceNorm2d(cin), x)
            forms.append((params, F.instance_norm(x64).clamp_min(0)))
        for params, xin in forms:
            ref = (res.double() + _ref64(xin, layer, True)).clamp_min(0)
            got = conv.conv2d_fused(x, layer, relu=True, residual=res, in_norm=params)
            assert float((got.double() - ref).abs().max()) <= _bound(ref)
            for b in range(B):
                p_b = None if params is None else params.view(B, cin, 2)[b].reshape(cin, 2).contiguous()
                one = conv.conv2d_fused(x[b:b + 1], layer, relu=True, residual=res[b:b + 1], in_norm=p_b)
                assert torch.equal(one[0], got[b]), (b, params is not None)
            if params is not None:
                plain = conv.conv2d_fused(x, layer, in_norm=params)
                ref_p = _ref64(xin, layer)
                assert float((plain.double() - ref_p).abs().max()) <= _bound(ref_p)
        xo, lo = other
        ro = torch.randn((xo.shape[0], lo.weight.shape[0], *xo.shape[2:]), device=DEV, generator=g)
        alone = conv.conv2d_fused(x, layer, relu=True, residual=res)
        o_alone = conv.conv2d_fused(xo, lo, relu=False, residual=ro)
        first, o_second = conv.conv2d_fused_pair((x, layer, True, res), (xo, lo, False, ro))
        o_first, second = conv.conv2d_fused_pair((xo, lo, False, ro), (x, layer, True, res))
        assert torch.equal(first, alone) and torch.equal(second, alone)
        assert torch.equal(o_first, o_alone) and torch.equal(o_second, o_alone)


@torch.no_grad()
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_conv2d_stats_output_and_statistics(case):
    from dkt_stereo_amd import conv, extractor
    with conv.use_backend("f16x3"):
        layer, x, _, _ = _setup(case, 13)
        B, cin = x.shape[:2]
        cout = layer.weight.shape[0]
        assert conv.stats_eligible(layer)
        forms = [None]
        if conv.fused_eligible(layer, True):
            forms.append(extractor.instance_norm_params(torch.nn.InstanceNorm2d(cin), x))
        for params in forms:
            out, st = conv.conv2d_stats(x, layer, in_norm=params)
            want = conv.conv2d(x, layer) if params is None else conv.conv2d_fused(x, layer, in_norm=params)
            assert torch.equal(out, want)
            xin = x.double() if params is None else F.instance_norm(x.double()).clamp_min(0)
            ref = _ref64(xin, layer)
            assert float((out.double() - ref).abs().max()) <= _bound(ref)
            norm = torch.nn.InstanceNorm2d(cout)
            got = extractor.instance_norm_params(norm, out, stats=st).view(B * cout, 2).double()
            o64 = out.double()
            mean, var = o64.mean((2, 3)).reshape(-1), o64.var((2, 3), unbiased=False).reshape(-1)
            hw = out.shape[2] * out.shape[3]
            assert float((got[:, 0] - mean).abs().max()) <= _bound(ref)
            invstd = (var + norm.eps).rsqrt()
            tol = 2.0 * hw * 2.0 ** -24 * (1.0 + float((mean * mean / var).max()))
            assert float(((got[:, 1] - invstd) / invstd).abs().max()) <= tol
            for b in range(B):
                p_b = None if params is None else params.view(B, cin, 2)[b].reshape(cin, 2).contiguous()
                one, _ = conv.conv2d_stats(x[b:b + 1], layer, in_norm=p_b)
                assert torch.equal(one[0], out[b]), (b, params is not None)
