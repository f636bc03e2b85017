"""The C8S format's restatement (tests/_c8_ref.py) and the host-side scale arithmetic, on the CPU.

What the -m gpu file test_gpu_c8_scaled.py relies on is established here: the restatement round-trips with the format's 22
bits, ActC8.absmax / channel_scales / _in_scale_vector agree with direct evaluations, C8Loop._rescale picks the scales the
tests assume, and the format's own error at the operand configurations of the GPU tests sits 15x under their bounds."""
import math
import types

import pytest
import torch

import _c8_ref as R
from dkt_stereo_amd import conv_c8 as c8
from dkt_stereo_amd import loop_c8


@pytest.mark.parametrize("log2max", [6.0, 10.0, 13.9])
def test_pack_ref_roundtrip_keeps_22_bits(log2max):
    """|err| <= 2^-21 * max(|x s|, 2^-3) in scaled units (the form of test_gpu_round3.py::test_c8s_pack_roundtrip_and_border,
    line 42), for scaled maxima at the low edge, the calibrated position and the high edge of the window."""
    torch.manual_seed(0)
    x = torch.randn(2, 70, 33, 37) * torch.logspace(-3, 3, 70).view(1, 70, 1, 1)
    s = 2.0 ** (math.floor(math.log2(2.0 ** log2max / float(x.abs().max()))))
    x = x * (2.0 ** log2max / s / float(x.abs().max()))            # max |x s| = 2^log2max
    a = R.pack_ref(x, s)
    assert a.t.shape == (2, 10, 2, 42, 66, 8) and a.scale == s
    assert math.isclose(float((x * s).abs().max()), 2.0 ** log2max, rel_tol=1e-6)
    y = R.unpack_ref(a)
    err = (y - x.double()).abs() * s / (x.double().abs() * s).clamp_min(2.0 ** -3)
    assert float(err.max()) <= 2.0 ** -21
    assert float(R.outside_interior(a, 0, 70).abs().max()) == 0.0          # border and padding channels
    # the tail decodes with its own scale
    b = R.pack_ref(x, s, tail=6, tail_scale=s * 8)
    assert b.channel_scales() == ((64, s), (6, s * 8))
    x2 = x.clone()
    x2[:, 64:] /= 8
    b = R.pack_ref(x2, s, tail=6, tail_scale=s * 8)
    assert torch.equal(b.t, a.t) and torch.equal(R.unpack_ref(b)[:, :64], y[:, :64]) and torch.equal(R.unpack_ref(b)[:, 64:] * 8, y[:, 64:])
    # a window into a wider destination
    w = R.pack_ref(x[:, :9], s, C_pad=40, ch0=16)
    ch = R.to_channels(w.t)
    assert torch.equal(ch[:, 16:25], R.to_channels(a.t)[:, :9]) and float(ch[:, :16].abs().max()) == 0 and float(ch[:, 25:].abs().max()) == 0
    assert torch.equal(R.from_channels(ch), w.t)


@pytest.mark.parametrize("C,tail", [(128, 2), (128, 1), (24, 0), (40, 8), (20, 5), (9, 1)])
def test_absmax_equals_the_direct_maxima(C, tail):
    """Tails that start inside a group, at a group boundary, and in the last, half-filled group."""
    torch.manual_seed(C + tail)
    x = torch.randn(2, C, 11, 35) * torch.logspace(-2, 2, C).view(1, C, 1, 1)
    x[0, C - tail - 1, 3, 4] = 700.0                  # the body's maximum sits right below the tail
    if tail:
        x[1, C - tail, 5, 6] = 900.0                  # and the tail's in its first channel
    s, ts = 4.0, 0.5
    a = R.pack_ref(x, s, tail=tail, tail_scale=ts)
    body, tmax = a.absmax()
    hi_b = (x[:, :C - tail] * s).half().abs().max().float()
    assert body.dtype == torch.float32 and float(body) == float(hi_b) == 2800.0
    if tail:
        assert float(tmax) == float((x[:, C - tail:] * ts).half().abs().max().float()) == 450.0
    else:
        assert tmax is None
    a.t[0, 0, 0, 1, 1, 0] = float("inf")              # an overflowed hi half is reported as such
    assert math.isinf(float(a.absmax()[0]))


def test_channel_scales_and_in_scale_vector_order():
    a = c8.ActC8(1, 128, 8, 8, "cpu", scale=4.0, tail=2)
    assert a.channel_scales() == ((128, 4.0),)
    a.tail_scale = 0.25
    assert a.channel_scales() == ((126, 4.0), (2, 0.25))
    b = c8.ActC8(1, 40, 8, 8, "cpu", scale=1024.0)
    d = c8.ActC8(1, 128, 8, 8, "cpu", scale=2.0, tail=1)
    d.tail_scale = 64.0
    v = c8._in_scale_vector([t.channel_scales() for t in (b, a, d)], "cpu")
    want = 1.0 / torch.cat([R.scale_vector(t, torch.float32) for t in (b, a, d)])
    assert v.dtype == torch.float32 and torch.equal(v, want)
    assert v.tolist() == [2.0 ** -10] * 40 + [0.25] * 126 + [4.0] * 2 + [0.5] * 127 + [2.0 ** -6]
    assert c8._in_scale_vector([((128, 1.0),), ((64, 1.0),)], "cpu") is None
    # the ConvGRU fold: scales follow the reference's input order [h | x...] in the z|r image and move with the channels to
    # [x... | r*h] in the q image
    from dkt_stereo_amd.update import ConvGRU
    torch.manual_seed(1)
    gru = ConvGRU(128, 40 + 128)
    hs, xs = ((128, 8.0),), (b.channel_scales(), a.channel_scales())
    wzr, wq2, ch = c8._gru_images(gru, [40, 128], hs, xs)
    inv = 1.0 / torch.cat([torch.full((128,), 8.0), R.scale_vector(b, torch.float32), R.scale_vector(a, torch.float32)])
    wz, wr, wq = (w.detach() * inv.view(1, -1, 1, 1) for w in (gru.convz.weight, gru.convr.weight, gru.convq.weight))
    assert ch == 128 and torch.equal(wq2, torch.cat([wq[:, 128:], wq[:, :128]], 1))
    for blk in range(4):
        assert torch.equal(wzr[64 * blk:64 * blk + 32], wz[32 * blk:32 * blk + 32])
        assert torch.equal(wzr[64 * blk + 32:64 * blk + 64], wr[32 * blk:32 * blk + 32])


def _stub():
    A = lambda C=128, tail=0: c8.ActC8(1, C, 8, 8, "cpu", tail=tail)      # noqa: E731
    s = types.SimpleNamespace(hc8=[A(), A(), A()], rh=[A(), A(), A()])
    s.mf = A(128, 2)
    s.others = [A() for _ in range(4)]
    s._scaled = lambda: [*s.hc8, s.mf, *s.others]
    return s


def test_rescale_arithmetic():
    """C8Loop._rescale on a stub: finite, zero and Inf maxima, the tail kept separate, r*h following the state."""
    s = _stub()
    n = len(s._scaled())
    m = [0.0] * (2 * n)
    m[0], m[2], m[4] = 0.7, 1.0, 3000.0               # the three states
    m[6], m[7] = 0.0123, 117.0                        # motion features: body, tail
    m[8] = 0.0                                        # an all-zero tensor keeps its scale
    m[10] = float("inf")
    m[12] = 2047.9
    s.others[0].scale = s.others[0].tail_scale = 32.0
    s.others[1].scale = 2.0 ** 15
    s.others[2].scale = 0.5
    over = loop_c8.C8Loop._rescale(s, m)
    assert over is True
    E = loop_c8.SCALE_EXP
    assert [a.scale for a in s.hc8] == [2.0 ** (E + 1), 2.0 ** E, 2.0 ** (E - 11)]
    assert [a.scale for a in s.rh] == [a.scale for a in s.hc8] and all(a.tail_scale == a.scale for a in s.rh)
    assert s.mf.scale == 2.0 ** (E + 7) and s.mf.tail_scale == 2.0 ** (E - 6)
    assert s.mf.channel_scales() == ((126, 2.0 ** (E + 7)), (2, 2.0 ** (E - 6)))
    assert s.others[0].scale == 32.0 and s.others[0].tail_scale == 32.0
    assert s.others[1].scale == 2.0 ** 3
    assert s.others[2].scale == 0.5 * 2.0 ** (E - 10) and s.others[2].tail_scale == s.others[2].scale
    # every finite positive maximum lands in [2^E, 2^(E+1)) after the rescale, and R.calibrated_scale is that rule from scale 1
    for v in (0.7, 1.0, 3000.0, 0.0123, 2047.9, 2.0 ** -10, 1e3):
        k = 2.0 ** (E - math.floor(math.log2(v)))
        assert 2.0 ** E <= v * k < 2.0 ** (E + 1)
        assert R.calibrated_scale(torch.tensor([v, -v / 3])) == k
    s2 = _stub()
    assert loop_c8.C8Loop._rescale(s2, [1.0] * (2 * n)) is False
    assert s2.mf.tail_scale == s2.mf.scale == 2.0 ** E
    # the window the edge cases of the GPU tests use
    for sh in R.EDGE_SHIFTS:
        assert 2.0 ** loop_c8.RANGE_LO <= 2.0 ** (E + sh) and 2.0 ** (E + 1 + sh) <= 2.0 ** loop_c8.RANGE_HI


#: twice the worst figure of the emulation over magnitudes 1e-3 ... 1e3 and the whole scale window (1.0e-7); the GPU
#: bounds (3e-6 convolution, 4e-6 ConvGRU step) are 15x and 20x above it
FORMAT_FLOOR = 2e-7


@pytest.mark.parametrize("balanced", [True, False])
@pytest.mark.parametrize("name", list(R.OPERAND_CONFIGS))
def test_format_floor_at_the_gpu_tests_operand_configurations(name, balanced):
    e = R.emulate_split_conv(R.OPERAND_CONFIGS[name], balanced=balanced, seed=len(name))
    print("%s balanced=%s: %.2e" % (name, balanced, e))
    assert e <= FORMAT_FLOOR


def test_emulation_sees_the_defects_the_gpu_tests_are_for():
    """The emulation itself discriminates: a dropped scale or one operand's scale far too small is far above the floor."""
    cfg = ((R.M_LO, 0), (R.M_LO, 0))
    assert R.emulate_split_conv(cfg, scales=(1.0, 1.0)) > 20 * FORMAT_FLOOR
    s = R.calibrated_scale(torch.tensor([R.M_LO * 4.0]))
    assert R.emulate_split_conv(cfg, scales=(s * 2.0 ** -20, s)) > 20 * FORMAT_FLOOR
    assert R.emulate_split_conv(cfg) <= FORMAT_FLOOR
