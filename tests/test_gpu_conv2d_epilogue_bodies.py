"""-m gpu: the epilogue bodies of conv2d_f16s_kernel that tests/test_gpu_conv2d_epilogues.py does not reach.  The kernel picks one
body per tile -- kind (plain, z|r gates, q gate, residual), z or r half, statistics, and whether the wave's channels all exist
and its planes span less than 2^31 bytes -- so every case here makes the two checks of that file:

  * placement, bit for bit: a batch against the same layer one batch item at a time (per-tile values: batch base pointers,
    channel-block pointers, the norm parameters of the item), a layer alone against the first and the second problem of a pair
    launch where pair launches exist;
  * fp64: within 1e-5 of max(1, output maximum) of an fp64 evaluation of the same operands, the bound of
    tests/test_gpu_round2.py that the existing file uses.

Cases: ragged channel blocks (the per-value channel guard: 64 -> 40, 96 -> 80 and the one-block head form 64 -> 2); the wide
tile shapes (8 waves, the 96-channel four-wave form, the few-tile forms); more tiles than resident blocks across batch items
with ragged edges (612 four-row tiles of a 96 -> 96 layer on 512 resident blocks) for conv2d, conv2d_fused and conv2d_stats;
the gate epilogues 1 and 2 alone, in pair launches and with the output aliasing the state; stride 2 and the sub-sampled 1x1
form; the device-scaled form of the input gradient.  Planes of 2^31 bytes and more per wave (the 64-bit lane offsets) are
beyond what a test may allocate and are not run.

The file pins behaviour (it passes on the kernel before its epilogue was split into bodies); nothing here is new function."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_parity import DEV
from test_host_conv2d_tile import DSCALE, NORM, layer_tile

#: what dkt_conv2d_f16s_tile answers, (kernel, KS, WM, WN, NF, MF, ST, CK), for the shapes the cases are named after
TILE_8WAVE = (0, 3, 4, 2, 2, 2, 1, 2)         # 256 channels x 4 rows, 8 waves
TILE_4X96 = (0, 3, 4, 1, 2, 3, 1, 2)          # four waves of 96 channels x 2 rows
TILE_256_FEW = (0, 3, 4, 1, 1, 2, 1, 2)       # 256 channels x 1 row
TILE_96_4ROWS = (0, 3, 1, 4, 1, 3, 1, 2)      # the 96-channel wave tile, four waves on rows
TILE_128_FEW = (0, 3, 2, 2, 1, 2, 1, 2)       # 128 channels x 2 rows

pytestmark = pytest.mark.gpu


def _bound(ref):
    return 1e-5 * max(1.0, float(ref.abs().max()))


def _layer(cin, cout, k, stride, seed):
    torch.manual_seed(seed)
    return torch.nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2).to(DEV)


def _input(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(shape, device=DEV, generator=g) * 1.5 + 0.3, g


def _ref64(x, layer, relu=False, bias=True):
    y = F.conv2d(x.double(), layer.weight.double(), layer.bias.double() if bias else None, stride=layer.stride,
                 padding=layer.padding)
    return y.clamp_min(0) if relu else y


def _close(got, ref):
    d = float((got.double() - ref).abs().max())
    assert d <= _bound(ref), (d, _bound(ref))


# ---- channel guard: the last channel block of a wave is ragged -------------------------------------------------------------
#: name, (B, Cin, H, W), Cout
GUARD = [("64_40", (3, 64, 33, 70), 40), ("96_80", (1, 96, 24, 60), 80), ("head_64_2", (2, 64, 20, 45), 2)]


@torch.no_grad()
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("case", GUARD, ids=[c[0] for c in GUARD])
def test_ragged_channel_blocks(case, relu):
    from dkt_stereo_amd import conv
    with conv.use_backend("f16x3"):
        _, shape, cout = case
        layer = _layer(shape[1], cout, 3, 1, 21)
        x, g = _input(shape, 21)
        assert conv.hip_eligible(layer)
        # a layer conv2d() sends to another kernel (the few-output direct one) reaches this kernel as a problem of a pair launch
        other = (torch.randn((1, 48, 12, 40), device=DEV, generator=g), _layer(48, cout, 3, 1, 22))
        assert conv.pair_eligible(layer, other[1])

        def run(xx):
            first, _ = conv.conv2d_pair((xx, layer, relu), (other[0], other[1], not relu))
            _, second = conv.conv2d_pair((other[0], other[1], not relu), (xx, layer, relu))
            assert torch.equal(first, second)
            if not conv.few_eligible(layer):
                assert torch.equal(conv.conv2d(xx, layer, relu=relu), first)
            return first

        got = run(x)
        _close(got, _ref64(x, layer, relu))
        for b in range(shape[0]):
            assert torch.equal(run(x[b:b + 1])[0], got[b]), b


# ---- the wide tile shapes ---------------------------------------------------------------------------------------------------
#: name, (B, Cin, H, W), Cout: 8 waves (>= 256 four-row tiles), four waves of 96 channels (>= 512 two-row tiles), few tiles
WIDE = [("128_256_8wave", (4, 128, 64, 128), 256, TILE_8WAVE), ("128_384_96ch", (4, 128, 64, 128), 384, TILE_4X96),
        ("128_256_few", (1, 128, 23, 39), 256, TILE_256_FEW)]


@torch.no_grad()
@pytest.mark.parametrize("case", WIDE, ids=[c[0] for c in WIDE])
def test_wide_tiles(case):
    from dkt_stereo_amd import conv
    with conv.use_backend("f16x3"):
        name, shape, cout, want_tile = case
        B, _, H, W = shape
        tiles_w = (W + 31) // 32
        if name == "128_256_8wave":
            assert tiles_w * ((H + 3) // 4) * B >= 256
        if name == "128_384_96ch":
            assert tiles_w * ((H + 1) // 2) * B >= 512
        if name == "128_256_few":
            assert tiles_w * ((H + 1) // 2) * B < 200
        layer = _layer(shape[1], cout, 3, 1, 31)
        x, _ = _input(shape, 31)
        assert conv.hip_eligible(layer)
        assert layer_tile(shape, layer) == want_tile
        for relu in (False, True):
            got = conv.conv2d(x, layer, relu=relu)
            _close(got, _ref64(x, layer, relu))
            for b in range(B):
                assert torch.equal(conv.conv2d(x[b:b + 1], layer, relu=relu)[0], got[b]), (relu, b)


# ---- more tiles than resident blocks ----------------------------------------------------------------------------------------
_MANY = {}


def _many():
    """96 -> 96 at (2, 96, 70, 520): 17 x 18 four-row tiles per item, 612 in all on 512 resident blocks; rows and columns ragged."""
    if not _MANY:
        layer = _layer(96, 96, 3, 1, 41)
        x, g = _input((2, 96, 70, 520), 41)
        res = torch.randn((2, 96, 70, 520), device=DEV, generator=g)
        _MANY.update(layer=layer, x=x, res=res, ref=_ref64(x, layer),
                     ref_n=_ref64(F.instance_norm(x.double()).clamp_min(0), layer))
    return _MANY


@torch.no_grad()
def test_many_tiles_conv2d_and_fused():
    from dkt_stereo_amd import conv
    with conv.use_backend("f16x3"):
        m = _many()
        layer, x, res = m["layer"], m["x"], m["res"]
        assert conv.hip_eligible(layer) and conv.fused_eligible(layer)
        assert ((520 + 31) // 32) * ((70 + 3) // 4) * 2 == 612
        assert layer_tile(x.shape, layer) == layer_tile(x.shape, layer, epilogue=3) == TILE_96_4ROWS      # plain and residual join
        for relu in (False, True):
            got = conv.conv2d(x, layer, relu=relu)
            _close(got, m["ref"].clamp_min(0) if relu else m["ref"])
            for b in range(2):
                assert torch.equal(conv.conv2d(x[b:b + 1], layer, relu=relu)[0], got[b]), (relu, b)
        for relu in (False, True):
            got = conv.conv2d_fused(x, layer, relu=relu, residual=res)
            _close(got, (res.double() + (m["ref"].clamp_min(0) if relu else m["ref"])).clamp_min(0))
            for b in range(2):
                one = conv.conv2d_fused(x[b:b + 1], layer, relu=relu, residual=res[b:b + 1])
                assert torch.equal(one[0], got[b]), (relu, b)


@torch.no_grad()
@pytest.mark.parametrize("normed", [False, True], ids=["plain", "in_norm"])
def test_many_tiles_conv2d_stats(normed):
    from dkt_stereo_amd import conv, extractor
    with conv.use_backend("f16x3"):
        m = _many()
        layer, x = m["layer"], m["x"]
        assert conv.stats_eligible(layer) and conv.fused_eligible(layer, True)
        assert layer_tile(x.shape, layer, form=NORM if normed else 0) == TILE_96_4ROWS
        params = extractor.instance_norm_params(torch.nn.InstanceNorm2d(96), x) if normed else None
        ref = m["ref_n"] if normed else m["ref"]
        out, st = conv.conv2d_stats(x, layer, in_norm=params)
        _close(out, ref)
        want = conv.conv2d_fused(x, layer, in_norm=params) if normed else conv.conv2d(x, layer)
        assert torch.equal(out, want)
        # the statistics: fp32 sums in an order the tiling decides -- the bounds of tests/test_gpu_conv2d_epilogues.py
        norm = torch.nn.InstanceNorm2d(96)
        got = extractor.instance_norm_params(norm, out, stats=st).view(2 * 96, 2).double()
        o64 = out.double()
        mean, var = o64.mean((2, 3)).reshape(-1), o64.var((2, 3), unbiased=False).reshape(-1)
        assert float((got[:, 0] - mean).abs().max()) <= _bound(ref)
        invstd = (var + norm.eps).rsqrt()
        tol = 2.0 * 70 * 520 * 2.0 ** -24 * (1.0 + float((mean * mean / var).max()))
        assert float(((got[:, 1] - invstd) / invstd).abs().max()) <= tol
        for b in range(2):
            p_b = None if params is None else params.view(2, 96, 2)[b].reshape(96, 2).contiguous()
            one, _ = conv.conv2d_stats(x[b:b + 1], layer, in_norm=p_b)
            assert torch.equal(one[0], out[b]), b


# ---- gate epilogues 1 (merged z|r) and 2 (q) --------------------------------------------------------------------------------
_GATE = {}


def _gates():
    """The ConvGRU of core/update.py:23-32 with 128 hidden and 256 input channels at 24 x 60, and a partner of another
    size and input width (128 + 64 channels at 20 x 45) for the pair launches; everything in fp64 once."""
    if not _GATE:
        g = torch.Generator(device=DEV).manual_seed(51)
        rnd = lambda *s: torch.randn(s, device=DEV, generator=g)  # noqa: E731
        for key, cx, H, W in (("a", 256, 24, 60), ("b", 64, 20, 45)):
            d = dict(zr=_layer(128 + cx, 256, 3, 1, 52), q=_layer(128 + cx, 128, 3, 1, 53), h=torch.tanh(rnd(1, 128, H, W)),
                     x=rnd(1, cx, H, W), cz=rnd(1, 128, H, W), cr=rnd(1, 128, H, W), cq=rnd(1, 128, H, W))
            hx = torch.cat([d["h"], d["x"]], 1)
            zr = _ref64(hx, d["zr"])
            d["z64"] = torch.sigmoid(zr[:, :128] + d["cz"].double())
            d["rh64"] = torch.sigmoid(zr[:, 128:] + d["cr"].double()) * d["h"].double()
            _GATE[key] = d
    return _GATE


@torch.no_grad()
def test_gate_zr_alone_and_in_a_pair():
    from dkt_stereo_amd import conv
    with conv.use_backend("f16x3"):
        G = _gates()
        a, b = G["a"], G["b"]
        assert conv.hip_eligible(a["zr"]) and conv.pair_eligible(a["zr"], b["zr"])
        arg = lambda d: ([d["h"], d["x"]], d["zr"], d["cz"], d["cr"], d["h"])  # noqa: E731
        z, rh = conv.conv2d_gate_zr(*arg(a))
        zb, rhb = conv.conv2d_gate_zr(*arg(b))
        _close(z, a["z64"])
        _close(rh, a["rh64"])
        _close(zb, b["z64"])
        _close(rhb, b["rh64"])
        (z1, rh1), (zb2, rhb2) = conv.conv2d_gate_zr_pair(arg(a), arg(b))
        (zb1, rhb1), (z2, rh2) = conv.conv2d_gate_zr_pair(arg(b), arg(a))
        for got in ((z1, rh1), (z2, rh2)):
            assert torch.equal(got[0], z) and torch.equal(got[1], rh)
        for got in ((zb1, rhb1), (zb2, rhb2)):
            assert torch.equal(got[0], zb) and torch.equal(got[1], rhb)


@torch.no_grad()
def test_gate_q_alone_in_a_pair_and_in_place():
    from dkt_stereo_amd import conv
    with conv.use_backend("f16x3"):
        G = _gates()
        a, b = G["a"], G["b"]
        assert conv.hip_eligible(a["q"]) and conv.pair_eligible(a["q"], b["q"])
        outs = {}
        for key, d in G.items():
            z, rh = d["z64"].float(), d["rh64"].float()
            q64 = torch.tanh(_ref64(torch.cat([rh, d["x"]], 1), d["q"]) + d["cq"].double())
            want = (1 - z.double()) * d["h"].double() + z.double() * q64
            got = conv.conv2d_gate_out([rh, d["x"]], d["q"], d["cq"], z, d["h"])
            _close(got, want)
            h2 = d["h"].clone()                          # the state updated in place: out aliases h
            same = conv.conv2d_gate_out([rh, d["x"]], d["q"], d["cq"], z, h2, out=h2)
            assert same.data_ptr() == h2.data_ptr() and torch.equal(h2, got)
            outs[key] = (z, rh, got)
        arg = lambda k, out: ([outs[k][1], G[k]["x"]], G[k]["q"], G[k]["cq"], outs[k][0], out if out is not None else G[k]["h"], out)  # noqa: E731
        first, o_second = conv.conv2d_gate_out_pair(arg("a", None), arg("b", None))
        ha, hb = a["h"].clone(), b["h"].clone()
        o_first, second = conv.conv2d_gate_out_pair(arg("b", hb), arg("a", ha))       # both in place
        assert torch.equal(first, outs["a"][2]) and torch.equal(second, outs["a"][2]) and second.data_ptr() == ha.data_ptr()
        assert torch.equal(o_first, outs["b"][2]) and torch.equal(o_second, outs["b"][2])


# ---- stride 2, and the 1x1 stride-2 layer run on every second pixel of every second row ------------------------------------
#: (the tiles: 128 channels x 2 rows at stride 2; the 1x1 layer as a stride-1 layer, ST = 1, on the 45 x 65 output)
STRIDE2 = [("3x3_s2_96_128", (1, 96, 47, 81), 128, 3, (0, 3, 2, 2, 1, 2, 2, 2)), ("1x1_s2_64_96", (2, 64, 90, 130), 96, 1, (0, 1, 2, 2, 1, 2, 1, 2))]


@torch.no_grad()
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("case", STRIDE2, ids=[c[0] for c in STRIDE2])
def test_stride2_and_subsampled_sources(case, relu):
    from dkt_stereo_amd import conv
    with conv.use_backend("f16x3"):
        _, shape, cout, k, want_tile = case
        layer = _layer(shape[1], cout, k, 2, 61)
        x, _ = _input(shape, 61)
        assert conv.hip_eligible(layer)
        assert layer_tile(shape, layer) == want_tile
        got = conv.conv2d(x, layer, relu=relu)
        assert tuple(got.shape[2:]) == ((shape[2] - 1) // 2 + 1, (shape[3] - 1) // 2 + 1)
        _close(got, _ref64(x, layer, relu))
        for b in range(shape[0]):
            assert torch.equal(conv.conv2d(x[b:b + 1], layer, relu=relu)[0], got[b]), b


# ---- the device-scaled form (the input gradient of a stride-1 convolution) --------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("magnitude", [1.0, 2.0 ** -18], ids=["unit", "tiny"])
def test_device_scaled_form(magnitude):
    from dkt_stereo_amd import conv
    with conv.use_backend("f16x3"):
        layer = _layer(96, 96, 3, 1, 71)
        x, _ = _input((2, 96, 24, 60), 71)
        x = x * magnitude
        assert conv.hip_eligible(layer) and not conv.few_eligible(layer) and not conv.direct_eligible(layer)
        assert layer_tile(x.shape, layer, form=DSCALE) == TILE_128_FEW          # 24 four-row tiles: the half-height form
        g, _, scale = conv.conv_grad_prepass(x, want_bias=False)
        got = conv.conv2d_dscale(g, layer, scale)
        ref = _ref64(x, layer, bias=False)
        d = float((got.double() - ref).abs().max())
        assert d <= 1e-5 * max(magnitude, float(ref.abs().max())), d        # (the bound of the file, at the gradient's own scale)
        for b in range(2):
            assert torch.equal(conv.conv2d_dscale(g[b:b + 1], layer, scale)[0], got[b]), b
