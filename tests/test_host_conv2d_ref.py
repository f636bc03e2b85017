"""No device: what tests/test_gpu_conv2d_reduced_passes.py relies on.

  * tests/_conv2d_ref.py restates the operands correctly: three passes is F.conv2d in fp64, w_hi is the fp16 image at the
    packer's scale at both edges of its [2^12, 2^13) window, hi + lo of the split reproduces w to <= 1e-7 of max|y| on a
    convolution (measured 3.6e-8 .. 6.2e-8);
  * every GPU case is DISCRIMINATING: at the case's channel configuration, on a 21 x 70 image, the one-pass model, the
    two-pass model, the exact convolution and a reduced model that skips one (tap, 16-channel chunk) -- the last tap of the
    last, partial chunk: the smallest step there is -- all lie >= 3e-5 of max|y| apart, ten times the GPU bound of 3e-6
    (the gate cases are measured on the gate's OUTPUT, which the GPU test holds to 1e-5).  Measured: 1.9e-4 .. 5.2e-1, the gate outputs
    9.6e-5 .. 2.1e-1."""
import math

import pytest
import torch
import torch.nn.functional as F

import _conv2d_ref as cr
import test_gpu_conv2d_reduced_passes as rp

H, W = 21, 70


def _x(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * 1.5 + 0.3


@pytest.mark.parametrize("ks,stride,srcs,cout", [(3, 1, (40,), 64), (1, 1, (40,), 112), (3, 2, (40,), 96), (3, 1, (7, 33), 30)])
def test_three_passes_is_the_fp64_convolution(ks, stride, srcs, cout):
    torch.manual_seed(3)
    layer = torch.nn.Conv2d(sum(srcs), cout, ks, stride=stride, padding=ks // 2)
    xs = [_x((2, c, 13, 37), 5 + i) for i, c in enumerate(srcs)]
    want = F.conv2d(torch.cat(xs, 1).double(), layer.weight.double(), layer.bias.double(), stride=stride, padding=ks // 2)
    assert torch.equal(cr.conv_ref(xs, layer, 3), want)
    assert torch.equal(cr.conv_ref(xs, layer, 3, relu=True), want.clamp_min(0))
    assert cr.distance(cr.conv_ref(xs, layer, 3, bias=False), want - layer.bias.double().view(1, -1, 1, 1)) <= 1e-15


def test_round_act_is_the_fp16_image_at_the_range_exponent():
    x = _x((1, 8, 9, 33), 7)
    assert torch.equal(cr.round_act(x), x.half().float())
    for e in (-4, 6):
        xs = x * 2.0 ** -e                             # the tensor a layer with dkt_in_exp = e is meant for
        assert torch.equal(cr.round_act(xs, e), x.half().float() * 2.0 ** -e)
    tiny = torch.tensor([2.0 ** -20, 3 * 2.0 ** -24, 2.0 ** -26])        # fp16 subnormals are kept, not flushed
    assert torch.equal(cr.round_act(tiny), torch.tensor([2.0 ** -20, 3 * 2.0 ** -24, 0.0]))


@pytest.mark.parametrize("wmax", [2.0 ** -3, 2.0 ** -2 * (1 - 2.0 ** -11), 0.0527, 3.7])
def test_w_hi_is_the_fp16_image_at_the_pack_scale(wmax):
    """Maxima at both edges of the window: max|w| * s = 2^12 exactly, and the last fp16 below 2^13."""
    from dkt_stereo_amd.conv import pack_scale
    g = torch.Generator().manual_seed(11)
    w = (torch.rand((24, 40, 3, 3), generator=g) * 2 - 1) * wmax * 0.999
    w[3, 5, 1, 2] = -wmax
    s = pack_scale(wmax)
    assert 2.0 ** 12 <= wmax * s < 2.0 ** 13 and math.log2(s) == int(math.log2(s))
    want = (w * s).half()
    assert float(want.float().abs().max()) < 2.0 ** 13
    assert torch.equal(cr.w_hi(w), want.float() / s)
    hi, lo = cr.w_split(w)
    assert torch.equal(hi, cr.w_hi(w))
    assert float((hi.double() + lo.double() - w.double()).abs().max()) <= 2.0 ** -22 * wmax


@pytest.mark.parametrize("cout,ks", [(64, 3), (112, 1), (300, 3)])
def test_the_split_reproduces_the_weights(cout, ks):
    torch.manual_seed(13)
    layer = torch.nn.Conv2d(40, cout, ks, padding=ks // 2)
    x = _x((1, 40, H, W), 17)
    hi, lo = cr.w_split(layer.weight)
    y = cr.conv_ref(x, layer, 3, bias=False)
    split = F.conv2d(x.double(), hi.double() + lo.double(), None, padding=ks // 2)
    d = cr.distance(split, y)
    print("hi + lo vs w on %d -> %d %dx%d: %.2e" % (40, cout, ks, ks, d))
    assert d <= 1e-7


# ---- validity of the GPU cases ----------------------------------------------------------------------------------------------
def _configs():
    """One entry per channel configuration of the GPU cases: (kind, srcs, cout, ks, stride, in_exp)."""
    seen = {}
    for c in rp.ALL_CASES:
        kind = "norm" if c.form == rp.NORM else "dscale" if c.form == rp.DSCALE else {1: "gate_zr", 2: "gate_q"}.get(c.epi, "plain")
        key = (kind, c.srcs, c.cout, c.ks, c.stride, c.o.get("in_exp", 0))
        seen.setdefault(key, c)
        if "partner" in c.o:
            seen.setdefault(("plain", (rp.PARTNER_SHAPE[1],), c.o["partner"], c.ks, 1, 0), None)
    return sorted(seen, key=str)


CONFIGS = _configs()


def _operands(kind, srcs, in_exp):
    xs = [_x((1, ch, H, W), 19 + i) * 2.0 ** -in_exp for i, ch in enumerate(srcs)]
    if kind == "norm":          # relu((x - mean) / std): half of the operand is zero
        x = xs[0]
        mean, var = x.mean((2, 3), keepdim=True), x.var((2, 3), unbiased=False, keepdim=True)
        params = torch.stack([mean.reshape(-1), (var + 1e-5).rsqrt().reshape(-1)], 1).contiguous()
        xs = [cr.norm_operand(x, params)]
    if kind.startswith("gate"):   # (h, x): a hidden state in (-1, 1) and unit-variance features, as the GPU cases draw them
        xs = [torch.tanh((xs[0] - 0.3) / 1.5), (xs[1] - 0.3) / 1.5]
    return xs


@pytest.mark.parametrize("config", CONFIGS, ids=["-".join(str(v) for v in k).replace(" ", "") for k in CONFIGS])
def test_gpu_case_is_discriminating(config):
    kind, srcs, cout, ks, stride, in_exp = config
    torch.manual_seed(23)
    layer = torch.nn.Conv2d(sum(srcs), cout, ks, stride=stride, padding=ks // 2, bias=kind != "dscale" and in_exp == 0)
    xs = _operands(kind, srcs, in_exp)
    g = torch.Generator().manual_seed(29)
    extra = [torch.randn((1, 128, H, W), generator=g) for _ in range(2)]

    def model(passes, drop=None):
        v = cr.conv_ref(xs, layer, passes, in_exp=in_exp, drop=drop)
        if kind == "gate_zr":
            return torch.cat(cr.gate_zr_ref(v, extra[0], extra[1], xs[0]), 1)
        if kind == "gate_q":
            return cr.gate_out_ref(v, extra[0], torch.sigmoid(extra[1]), xs[0])
        return v
    need = 10 * cr.BOUND
    last = (ks * ks - 1, (sum(srcs) - 1) // 16)
    exact, one, two = model(3), model(1), model(2)
    dist = {"one vs two": cr.distance(one, two), "one vs exact": cr.distance(one, exact), "two vs exact": cr.distance(two, exact),
            "one vs one less a step": cr.distance(model(1, last), one), "two vs two less a step": cr.distance(model(2, last), two)}
    print("VALID %s: %s" % (config, ", ".join("%s %.2e" % kv for kv in dist.items())))
    for name, d in dist.items():
        assert d >= need, (name, d)
