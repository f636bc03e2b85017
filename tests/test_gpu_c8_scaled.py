"""-m gpu: the C8S kernels at calibrated operand scales against fp64.

Every C8S tensor of the refinement loop carries a power-of-two scale (ActC8.scale / tail_scale, loop_c8.SCALE_EXP): producers
multiply by it before the fp16 (hi, lo) split, consumers fold 1 / scale per input channel into their packed weights.  Here
that arithmetic runs against independent references: operands are built with the restatement of the format in _c8_ref.py
(pack_ref), outputs are decoded with unpack_ref, the expected values are torch's fp64 operators.  Operands of one launch get
different magnitudes (2^-10, 1, 2^10) and scales (the calibrated one, and the edges of the window the loop tolerates before
it recalibrates: 2^-4 and 2^+3 times that).

No bound is new.  CONV: 3e-6 relative to the output maximum (test_gpu_round3.py, test_conv_c8_matches_fp64_for_every_tile_shape);
GRU: 4e-6 (test_gpu_round4.py, test_fused_gru_step_matches_fp64_and_the_two_launch_form); STEM: 3e-6 (test_gpu_conv.py,
test_stem7_vs_fp64); LOOKUP: 2e-6 (test_gpu_round2.py, test_lookup_conv1x1_fused; test_gpu_round3.py,
test_geo_lookup_fused_with_convc1); NORM: 2e-6 (test_gpu_round3.py, test_instance_norm_join_c8_matches_torch); HEAD: 2e-5
(test_gpu_round3.py, test_fused_flow_head_matches_two_layers).  All are taken relative to the OUTPUT MAXIMUM, also where the
scale-1 test says max(1, maximum): at magnitude 2^-10 that form would see nothing.  The format's own error at these operand
configurations is below 2e-7 (test_host_c8_ref.py).  Weights are "balanced" (input channels of an operand divided by its
magnitude) where every operand has to matter to the output, and biases / context terms are scaled with the output so that
the products dominate it."""
import math

import pytest
import torch
import torch.nn.functional as F

import _c8_ref as R
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

CONV, GRU, STEM, LOOKUP, NORM, HEAD = 3e-6, 4e-6, 3e-6, 2e-6, 2e-6, 2e-5
#: a second tensor of the same launch sits at the other edge of the window
OTHER = {0: 0, -4: 3, 3: -4}


@pytest.fixture(autouse=True, scope="module")
def _release_cached_blocks():
    """The 184 x 312 cases leave a few GB in torch's caching allocator; hand them back so that the timing assertions of the
    modules that run afterwards see the device as they do without this file."""
    yield
    torch.cuda.empty_cache()


def _c8():
    from dkt_stereo_amd import conv_c8
    return conv_c8


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max())


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _operand(shape, mag, shift, kind="randn", gen=None):
    return R.operand(shape, mag, shift, kind, device=DEV, gen=gen)


def _prefilled(B, Cd, H, W, scale, gen, tail=0, tail_scale=None):
    """A destination whose every channel already holds (finite, random) bytes in the interior."""
    a = _c8().ActC8(B, Cd, H, W, DEV, scale=scale, tail=tail)
    if tail_scale is not None:
        a.tail_scale = float(tail_scale)
    ch = R.to_channels(a.t).clone()
    ch[:, :Cd, :, 1:H + 1, 1:W + 1] = torch.randn((B, Cd, 2, H, W), device=DEV, generator=gen).half()
    a.t = R.from_channels(ch)
    return a, ch


def _assert_rest_untouched(a, before, ch0, C):
    """Border, padding channels and every 8-channel group outside [ch0, ch0 + C) keep their bytes; the channels that fill the
    last written group are zero."""
    now = R.to_channels(a.t)
    c1 = ch0 + (C + 7) // 8 * 8
    m = now.clone()
    m[:, ch0:c1, :, 1:a.H + 1, 1:a.W + 1] = before[:, ch0:c1, :, 1:a.H + 1, 1:a.W + 1]
    assert torch.equal(m, before), "bytes outside the written channels changed"
    assert float(now[:, ch0 + C:c1].float().abs().max() if c1 > ch0 + C else 0.0) == 0.0


# ---- a. pack / unpack -----------------------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("log2s", [-12, -3, 0, 5, 11, 20])
@pytest.mark.parametrize("C", [1, 7, 8, 9, 70, 128])
def test_pack_equals_the_restatement_bit_for_bit(C, log2s):
    c8 = _c8()
    s = 2.0 ** log2s
    g = _gen(C * 100 + log2s + 50)
    B, H, W = 2, 33, 37
    # scaled values over seven decades below 2^12: normal and subnormal lo halves, hi halves down to fp16's subnormals
    x = torch.randn((B, C, H, W), device=DEV, generator=g) * (2.0 ** 10 / s) * torch.logspace(-7, 0, W, device=DEV)
    want = R.pack_ref(x, s)
    got = c8.pack(x, scale=s)
    assert got.scale == s and torch.equal(got.t, want.t)
    assert torch.equal(c8.unpack(got), R.unpack_ref(want).float())
    # a non-contiguous source (the .contiguous() branch) and a batch-strided one (used in place)
    xt = torch.zeros((B, C, H, 2 * W), device=DEV)[..., ::2]
    xt.copy_(x)
    wide = torch.zeros((B, C + 3, H, W), device=DEV)
    wide[:, 1:1 + C] = x
    assert xt.stride(3) == 2 and wide[:, 1:1 + C].stride(0) != C * H * W
    assert torch.equal(c8.pack(xt, scale=s).t, want.t) and torch.equal(c8.pack(wide[:, 1:1 + C], scale=s).t, want.t)
    # into a wider destination whose other channels hold data
    for ch0 in (0, 8, 64):
        dst, before = _prefilled(B, 200, H, W, s, g)
        assert c8.pack(x, dst, ch0) is dst
        assert torch.equal(R.to_channels(dst.t)[:, ch0:ch0 + C], R.to_channels(want.t)[:, :C])
        _assert_rest_untouched(dst, before, ch0, C)
        assert torch.equal(c8.unpack(dst, C, ch0), R.unpack_ref(want).float())


@torch.no_grad()
@pytest.mark.parametrize("C,tail", [(128, 2), (128, 1), (40, 8), (20, 5)])
def test_unpack_decodes_every_channel_with_its_own_scale(C, tail):
    """conv_c8.unpack on a tensor with tail_scale != scale: per channel_scales(), whole and in windows."""
    c8 = _c8()
    g = _gen(C + tail)
    x = torch.randn((1, C, 17, 40), device=DEV, generator=g)
    x[:, C - tail:] *= 100.0
    a = R.pack_ref(x, 2.0 ** 11, tail=tail, tail_scale=2.0 ** 3)
    want = R.unpack_ref(a)
    floor = (2.0 ** -3 / R.scale_vector(a)).view(1, C, 1, 1)                  # (2^-3 in scaled units, test_gpu_round3.py:42)
    assert float(((want - x.double()).abs() / torch.maximum(x.double().abs(), floor)).max()) <= 2.0 ** -21
    assert torch.equal(c8.unpack(a), want.float())
    c0 = (C - tail) // 8 * 8
    assert torch.equal(c8.unpack(a, C - c0, c0), want[:, c0:].float())
    assert torch.equal(c8.unpack(a, 8, 0), want[:, :8].float())


# ---- b. producers into a scaled destination ------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("B,H,W,mag,shift,ch0", [(1, 46, 78, R.M_LO, 0, 0), (2, 33, 37, 1.0, -4, 64), (1, 92, 156, R.M_HI, 3, 8),
                                                 (1, 184, 312, R.M_LO, 3, 0)])
def test_pool_and_interp_into_scaled_destinations(B, H, W, mag, shift, ch0):
    """pool2x_c8 == torch's avg_pool2d followed by the split, bit for bit (test_gpu_round3.py:147-148).  interp_c8 == the fp32 kernel
    followed by the split, bit for bit (test_gpu_round3.py:150), and that within 2e-6 x magnitude of torch's interpolate
    (test_gpu_conv.py:277-278 on the same randn data at magnitude 1; the interpolation weights are computed in another order than
    ATen's: bit-identical only where the size ratio is exact).  resample_pair_c8: both orders, two different scales in one launch."""
    from dkt_stereo_amd.update import interp
    c8 = _c8()
    g = _gen(H * 7 + W)
    fine, _ = _operand((B, 128, 2 * H, 2 * W - 1), mag, 0, gen=g)
    coarse, _ = _operand((B, 128, (H + 1) // 2, (W + 1) // 2), 1.0 / mag, 0, gen=g)
    Hm, Wm = (fine.shape[2] - 1) // 2 + 1, (fine.shape[3] - 1) // 2 + 1
    want_p, want_u = R.pool_ref(fine), interp(coarse, torch.empty((B, 128, Hm, Wm), device=DEV))
    e_u = float((want_u - R.interp_ref(coarse, (Hm, Wm))).abs().max()) * mag
    print("interp vs torch, in units of the magnitude: %.2e" % e_u)
    assert e_u <= 2e-6
    sp, su = R.calibrated_scale(want_p) * 2.0 ** shift, R.calibrated_scale(want_u) * 2.0 ** OTHER[shift]
    assert sp != su
    ref_p, ref_u = R.to_channels(R.pack_ref(want_p, sp).t), R.to_channels(R.pack_ref(want_u, su).t)

    def check(p, bp, u, bu):
        assert torch.equal(R.to_channels(p.t)[:, ch0:ch0 + 128], ref_p[:, :128])
        assert torch.equal(R.to_channels(u.t)[:, ch0:ch0 + 128], ref_u[:, :128])
        _assert_rest_untouched(p, bp, ch0, 128)
        _assert_rest_untouched(u, bu, ch0, 128)

    p, bp = _prefilled(B, 128 + 72, Hm, Wm, sp, g)
    u, bu = _prefilled(B, 128 + 72, Hm, Wm, su, g)
    c8.pool2x_c8(fine, p, ch0)
    c8.interp_c8(coarse, u, ch0)
    check(p, bp, u, bu)
    for order in (0, 1):
        p, bp = _prefilled(B, 128 + 72, Hm, Wm, sp, g)
        u, bu = _prefilled(B, 128 + 72, Hm, Wm, su, g)
        jobs = [("pool", fine, p, ch0), ("interp", coarse, u, ch0)]
        c8.resample_pair_c8(*(jobs if order == 0 else jobs[::-1]))
        check(p, bp, u, bu)


@torch.no_grad()
@pytest.mark.parametrize("B,cin,H,W,mag,shift,ch0", [(1, 2, 33, 37, R.M_LO, 0, 0), (2, 1, 50, 70, 1.0, 3, 64), (1, 2, 46, 78, R.M_HI, -4, 0),
                                                     (1, 2, 184, 312, R.M_LO, -4, 0)])
def test_stem7_into_scaled_destinations(B, cin, H, W, mag, shift, ch0):
    """stem7_c8 and stem7_dual (its fp32 output must not see the scale) against an fp64 convolution."""
    c8 = _c8()
    torch.manual_seed(H + cin)
    g = _gen(H + W)
    stem = torch.nn.Conv2d(cin, 64, 7, padding=3).to(DEV)
    stem.weight.mul_(mag / 5.0)
    stem.bias.mul_(mag if B == 1 else 0.0)
    flow = torch.randn((B, cin, H, W), device=DEV, generator=g) * 5
    for relu in (True, False):
        want = R.conv_ref64([flow], stem.weight, stem.bias, relu=relu, padding=3)
        s = R.calibrated_scale(want) * 2.0 ** shift
        dst, before = _prefilled(B, ch0 + 64, H, W, s, g)
        c8.stem7_c8(flow, stem, dst, relu=relu, ch0=ch0)
        e = _rel(R.unpack_ref(dst, 64, ch0), want)
        print("stem7_c8 relu=%d: %.2e" % (relu, e))
        assert e <= STEM
        _assert_rest_untouched(dst, before, ch0, 64)
        y1, y2 = torch.empty((B, 64, H, W), device=DEV), torch.empty((B, 64, H, W), device=DEV)
        d1, d2 = c8.ActC8(B, 64, H, W, DEV, scale=s), c8.ActC8(B, 64, H, W, DEV, scale=1.0)
        c8.stem7_dual(flow, stem, y1, d1, relu=relu)
        c8.stem7_dual(flow, stem, y2, d2, relu=relu)
        assert torch.equal(y1, y2) and _rel(y1, want) <= STEM
        assert torch.equal(R.unpack_ref(d1), R.unpack_ref(R.pack_ref(y1, s))) and _rel(R.unpack_ref(d1), want) <= STEM
        assert float(R.outside_interior(d1).float().abs().max()) == 0.0


@torch.no_grad()
@pytest.mark.parametrize("B,C,H,W,mag,shift,ch0", [(2, 64, 40, 72, R.M_LO, 0, 0), (1, 20, 33, 37, R.M_HI, 3, 8), (1, 64, 46, 78, 1.0, -4, 64),
                                                   (1, 64, 184, 312, R.M_LO, 3, 0)])
def test_norm_join_into_scaled_destinations(B, C, H, W, mag, shift, ch0):
    from dkt_stereo_amd import extractor as ex
    c8 = _c8()
    g = _gen(C + H)
    norm = torch.nn.InstanceNorm2d(C)
    c = (torch.randn((B, C, H, W), device=DEV, generator=g) * 3 + 1) * mag
    a = (torch.randn((B, C, H, W), device=DEV, generator=g) * 2 - 0.5) * mag
    pc, pa = ex.instance_norm_params(norm, c), ex.instance_norm_params(norm, a)
    nc, na = F.instance_norm(c.double()), F.instance_norm(a.double())
    for want, kw in ((nc.clamp_min(0), dict(c_relu=True)),
                     (nc, dict(c_relu=False)),
                     ((a.double() + nc.clamp_min(0)).clamp_min(0), dict(c_relu=True, a=a)),
                     ((na.clamp_min(0) + nc.clamp_min(0)).clamp_min(0), dict(c_relu=True, a=a, a_params=pa, a_relu=True)),
                     ((na + nc.clamp_min(0)).clamp_min(0), dict(c_relu=True, a=a, a_params=pa, a_relu=False))):
        s = R.calibrated_scale(want) * 2.0 ** shift
        y = torch.empty_like(c)
        d, before = _prefilled(B, ch0 + C + 16, H, W, s, g)
        c8.norm_join_c8(c, pc, y=y, dst=d, ch0=ch0, **kw)
        e = (_rel(y, want), _rel(R.unpack_ref(d, C, ch0), want))
        print("norm_join %s: %.2e %.2e" % (sorted(kw), *e))
        assert max(e) <= NORM, kw.keys()
        assert torch.equal(R.unpack_ref(d, C, ch0), R.unpack_ref(R.pack_ref(y, s)))
        _assert_rest_untouched(d, before, ch0, C)


def _coords(B, H, W, g, spread=30.0):
    xs = torch.arange(W, device=DEV, dtype=torch.float32).view(1, 1, 1, W).expand(B, 1, H, W)
    ys = torch.arange(H, device=DEV, dtype=torch.float32).view(1, 1, H, 1).expand(B, 1, H, W)
    return torch.cat([xs - spread * torch.rand((B, 1, H, W), device=DEV, generator=g), ys], 1).contiguous(), torch.cat([xs, ys], 1).contiguous()


@torch.no_grad()
@pytest.mark.parametrize("B,H,W,r,mag,shift,ch0", [(2, 40, 96, 4, R.M_LO, 0, 0), (1, 33, 130, 3, R.M_HI, 3, 64), (1, 46, 78, 4, 1.0, -4, 0),
                                                   (1, 184, 312, 4, R.M_LO, 3, 0)])
def test_corr_lookup_conv1x1_into_a_scaled_destination(B, H, W, r, mag, shift, ch0):
    from dkt_stereo_amd.corr import CorrBlock1D
    c8 = _c8()
    torch.manual_seed(W)
    g = _gen(W + r)
    f1, f2 = (torch.randn((B, 64, H, W), device=DEV, generator=g) for _ in range(2))
    blk = CorrBlock1D(f1, f2, num_levels=4, radius=r)
    coords, _ = _coords(B, H, W, g)
    c1 = torch.nn.Conv2d(4 * (2 * r + 1), 64, 1).to(DEV)
    c1.weight.mul_(mag)
    c1.bias.mul_(mag if ch0 == 0 else 0.0)
    want = R.conv_ref64([blk(coords)], c1.weight, c1.bias, relu=True, padding=0)
    s = R.calibrated_scale(want) * 2.0 ** shift
    dst, before = _prefilled(B, ch0 + 64, H, W, s, g)
    assert blk.lookup_conv1x1(coords, c1, out_c8=dst, out_c8_ch0=ch0) is dst
    e = _rel(R.unpack_ref(dst, 64, ch0), want)
    print("lookup + convc1: %.2e" % e)
    assert e <= LOOKUP
    _assert_rest_untouched(dst, before, ch0, 64)
    out = blk.lookup_conv1x1(coords, c1)
    assert torch.equal(R.unpack_ref(dst, 64, ch0), R.unpack_ref(R.pack_ref(out, s)))


@torch.no_grad()
@pytest.mark.parametrize("B,H,W,D,mag,shift,ch0", [(1, 40, 72, 48, R.M_LO, 0, 0), (2, 23, 100, 32, R.M_HI, -4, 64), (1, 33, 37, 48, 1.0, 3, 0),
                                                   (1, 184, 312, 48, R.M_LO, -4, 0)])
def test_geo_lookup_conv1x1_into_a_scaled_destination(B, H, W, D, mag, shift, ch0):
    import _synth
    from dkt_stereo_amd.geometry import Combined_Geo_Encoding_Volume
    from test_gpu_parity import G
    c8 = _c8()
    torch.manual_seed(D + W)
    g = _gen(D + W)
    m1, m2 = G(_synth.normal((B, 24, H, W), 11, "m1")), G(_synth.normal((B, 24, H, W), 11, "m2"))
    geo = G(_synth.normal((B, 8, D, H, W), 12, "geo"))
    fn = Combined_Geo_Encoding_Volume(m1, m2, geo, radius=4, num_levels=2)
    coords = torch.arange(W, device=DEV).float().view(1, 1, W, 1).repeat(B, H, 1, 1)
    layer = torch.nn.Conv2d(162, 64, 1).to(DEV)
    layer.weight.mul_(mag)
    layer.bias.mul_(mag if ch0 == 0 else 0.0)
    disp = torch.rand((B, 1, H, W), device=DEV, generator=g) * (D + 10) - 5
    want = R.conv_ref64([fn(disp, coords)], layer.weight, layer.bias, relu=True, padding=0)
    s = R.calibrated_scale(want) * 2.0 ** shift
    dst, before = _prefilled(B, ch0 + 64, H, W, s, g)
    assert fn.lookup_conv1x1(disp, coords, layer, relu=True, out_c8=dst, out_c8_ch0=ch0) is dst
    e = _rel(R.unpack_ref(dst, 64, ch0), want)
    print("geo lookup + convc1: %.2e" % e)
    assert e <= LOOKUP
    _assert_rest_untouched(dst, before, ch0, 64)
    out = fn.lookup_conv1x1(disp, coords, layer, relu=True)
    assert torch.equal(R.unpack_ref(dst, 64, ch0), R.unpack_ref(R.pack_ref(out, s)))


class _Front:
    """The operands of one dkt_motion_front_c8 launch with the hidden state, the correlation features and the flow features at
    magnitudes / scales of their own."""

    def __init__(self, B, H, W, radius, mags, shifts, seed):
        from dkt_stereo_amd.corr import CorrBlock1D
        from dkt_stereo_amd.update import FlowHead, _leading_outputs
        torch.manual_seed(seed)
        g = self.g = _gen(seed)
        m_h, m_c, m_f = mags
        self.fh = FlowHead(128, 256, 2).to(DEV)
        self.fh.conv1.weight.div_(m_h)
        self.h, self.s_h = _operand((B, 128, H, W), m_h, shifts[0], "tanh", gen=g)
        f1, f2 = (torch.randn((B, 64, H, W), device=DEV, generator=g) for _ in range(2))
        self.blk = CorrBlock1D(f1, f2, num_levels=4, radius=radius)
        self.convc1 = torch.nn.Conv2d(4 * (2 * radius + 1), 64, 1).to(DEV)
        self.convf1 = torch.nn.Conv2d(2, 64, 7, padding=3).to(DEV)
        for layer, m in ((self.convc1, m_c), (self.convf1, m_f / 10.0)):
            layer.weight.mul_(m)
            layer.bias.mul_(m)
        self.start, self.coords0 = _coords(B, H, W, g, 20.0)
        self.last = _leading_outputs(self.fh.conv2, 1)
        self.B, self.H, self.W, self.shifts = B, H, W, shifts

    def run(self):
        c8 = _c8()
        B, H, W = self.B, self.H, self.W
        hc8 = R.pack_ref(self.h, self.s_h)
        planes, n_co = c8.head_planes([hc8], self.fh.conv1, self.last, cfg=2)
        # fp64 expectations: coordinate and flow from the head's definition ...
        delta = R.flow_head_ref64(self.fh.conv1, self.fh.conv2, [R.unpack_ref(hc8)])[:, :1]
        want_x = self.start[:, :1].double() + delta
        c_old, c_new = self.start.clone(), torch.full_like(self.start, -7.0)
        flow = torch.zeros((B, 2, H, W), device=DEV)
        flow[:, 1] = 0.25
        # ... and the scales from the expected features (the loop's calibration sees the same tensors)
        x_exp = self.start.clone()
        x_exp[:, :1] = want_x.float()
        f_exp = flow.clone()
        f_exp[:, :1] = x_exp[:, :1] - self.coords0[:, :1]
        s_c = R.calibrated_scale(R.conv_ref64([self.blk(x_exp)], self.convc1.weight, self.convc1.bias, relu=True, padding=0)) * 2.0 ** self.shifts[1]
        s_f = R.calibrated_scale(R.conv_ref64([f_exp], self.convf1.weight, self.convf1.bias, relu=True, padding=3)) * 2.0 ** self.shifts[2]
        cor, flo = c8.ActC8(B, 64, H, W, DEV, scale=s_c), c8.ActC8(B, 64, H, W, DEV, scale=s_f)
        assert c8.motion_front_supported(self.blk, type("E", (), dict(convc1=self.convc1, convf1=self.convf1)))
        c8.motion_front(self.blk, planes, n_co, self.last.bias, c_old[:, :1], c_new[:, :1], self.coords0[:, :1], flow, self.convc1, cor,
                        self.convf1, flo)
        assert torch.equal(c_old, self.start) and bool((c_new[:, 1] == -7.0).all()) and bool((flow[:, 1] == 0.25).all())
        e_x = float((c_new[:, :1].double() - want_x).abs().max()) / max(1.0, float(delta.abs().max()))
        assert torch.equal(flow[:, :1], c_new[:, :1] - self.coords0[:, :1])
        # the feature stages take the coordinate / flow the kernel produced
        c_full = self.start.clone()
        c_full[:, :1] = c_new[:, :1]
        want_c = R.conv_ref64([self.blk(c_full)], self.convc1.weight, self.convc1.bias, relu=True, padding=0)
        want_f = R.conv_ref64([flow], self.convf1.weight, self.convf1.bias, relu=True, padding=3)
        e_c, e_f = _rel(R.unpack_ref(cor), want_c), _rel(R.unpack_ref(flo), want_f)
        print("motion front: coordinate %.2e, cor %.2e (scale 2^%d), flo %.2e (scale 2^%d)" % (e_x, e_c, math.log2(s_c), e_f, math.log2(s_f)))
        assert s_c != s_f
        assert e_x <= HEAD and e_c <= LOOKUP and e_f <= STEM
        assert float(R.outside_interior(cor).float().abs().max()) == 0.0 and float(R.outside_interior(flo).float().abs().max()) == 0.0
        return hc8, cor, flo, flow, c_new


@torch.no_grad()
@pytest.mark.parametrize("B,H,W,radius,mags,shifts", [(1, 46, 78, 4, (1.0, R.M_LO, R.M_HI), (0, 0, 0)),
                                                      (2, 40, 96, 4, (R.M_LO, R.M_HI, 1.0), (3, -4, 3)),
                                                      (1, 33, 130, 3, (1.0, 1.0, R.M_LO), (-4, 3, -4)),
                                                      (1, 184, 312, 4, (1.0, R.M_HI, R.M_LO), (0, 3, -4))])
def test_motion_front_with_cor_and_flo_at_different_scales(B, H, W, radius, mags, shifts):
    """dkt_motion_front_c8 against torch operators (not against the three launches): the coordinate from an fp64 FlowHead on the
    decoded state, cor from an fp64 1x1 layer on the correlation lookup at the coordinate the kernel wrote, flo from an fp64
    7x7 layer on the flow it wrote."""
    _Front(B, H, W, radius, mags, shifts, seed=B * 1000 + W).run()


# ---- c. conv2d_c8 -------------------------------------------------------------------------------------------------------------
def _conv_case(B, H, W, chans, cout, config, balanced, bias, seed, kinds=None):
    torch.manual_seed(seed)
    g = _gen(seed)
    cfgs = R.OPERAND_CONFIGS[config][:len(chans)]
    xs, acts = [], []
    for i, (c, (mag, shift)) in enumerate(zip(chans, cfgs)):
        x, s = _operand((B, c, H, W), mag, shift, (kinds or ["randn", "relu", "tanh"])[i % 3], gen=g)
        xs.append(x)
        acts.append(R.pack_ref(x, s))
    assert len({a.scale for a in acts}) == len(acts)
    layer = torch.nn.Conv2d(sum(chans), cout, 3, padding=1).to(DEV)
    mags = [m for m, _ in cfgs]
    if balanced:
        layer.weight.copy_(R.balance_weights(layer.weight, chans, mags))
        layer.bias.mul_(bias)
    else:
        layer.bias.mul_(bias * max(mags))
    return xs, acts, layer, g


@torch.no_grad()
@pytest.mark.parametrize("case", [
    (1, 33, 37, [16, 48], 40, "lo_hi", True, 1.0), (2, 50, 70, [64, 40, 24], 64, "one_hi_lo", True, 0.0),
    (1, 46, 78, [64, 40, 24], 126, "edge_mixed", True, 1.0), (2, 33, 37, [80], 200, "edge_low", False, 1.0),
    (1, 50, 70, [16, 48], 64, "edge_high", False, 0.0), (1, 46, 78, [64, 40, 24], 128, "edge_low", True, 1.0),
    (1, 184, 312, [64, 64], 126, "lo_hi", True, 1.0)], ids=lambda c: "%s-%s-%d" % (c[5], "x".join(map(str, c[3])), c[4]))
def test_conv_c8_scaled_operands_every_tile_shape(case):
    """conv(cat(srcs)) with two and three operands at different scales: fp32 output and C8S output with a scale of its own at
    channel 0 and 64, ReLU on and off, every tile configuration."""
    c8 = _c8()
    B, H, W, chans, cout, config, balanced, bias = case
    xs, acts, layer, g = _conv_case(B, H, W, chans, cout, config, balanced, bias, seed=H + cout)
    ref = R.conv_ref64([R.unpack_ref(a) for a in acts], layer.weight, layer.bias)
    assert _rel(ref, R.conv_ref64(xs, layer.weight, layer.bias)) <= 2e-7          # (the operands are the values that were packed)
    worst = 0.0
    for relu in (False, True):
        want = ref.clamp_min(0) if relu else ref
        s_out = R.calibrated_scale(want) * 2.0 ** (3 if relu else -4)
        for cfg in (0, 1, 2, 3, 4, 5, 6):
            y = c8.conv2d_c8(acts, layer, relu=relu, cfg=cfg)
            e = [_rel(y, want)]
            for ch0 in (0, 64):
                oc, before = _prefilled(B, ch0 + cout, H, W, s_out, g)
                if ch0 == 0:
                    oc.t.zero_()
                    before = torch.zeros_like(before)
                c8.conv2d_c8(acts, layer, relu=relu, out_c8=oc, out_c8_ch0=ch0, cfg=cfg)
                e.append(_rel(R.unpack_ref(oc, cout, ch0), want))
                _assert_rest_untouched(oc, before, ch0, cout)
            worst = max(worst, *e)
            assert max(e) <= CONV, (case, cfg, relu, e)
    print("conv2d_c8 %s: worst %.2e" % (case, worst))


@torch.no_grad()
@pytest.mark.parametrize("B,H,W,tail,m_feat,shift", [(1, 46, 78, 2, 1.0, 0), (2, 33, 37, 2, R.M_LO, 3), (1, 50, 70, 1, R.M_LO, 0),
                                                     (1, 46, 78, 1, 1.0, -4), (1, 184, 312, 2, R.M_LO, 0)])
def test_conv_c8_tail_with_a_scale_of_its_own_and_as_an_operand(B, H, W, tail, m_feat, shift):
    """The motion encoder's cat([features, flow]) (core/update.py:85; IGEV: 127 + 1) with tail_scale != scale, decoded per
    segment; then that tensor as an operand of the next convolution beside a second one: a two-segment channel_scales() folded
    into the weights."""
    c8 = _c8()
    xs, acts, enc, g = _conv_case(B, H, W, [64, 64], 128 - tail, "lo_hi", True, 1.0, seed=H + tail, kinds=["relu", "relu"])
    enc.weight.mul_(m_feat)
    enc.bias.mul_(m_feat)
    flow = torch.randn((B, tail, H, W), device=DEV, generator=g) * 100.0
    want = R.conv_ref64([R.unpack_ref(a) for a in acts], enc.weight, enc.bias, relu=True)
    s_feat, s_tail = R.calibrated_scale(want) * 2.0 ** shift, R.calibrated_scale(flow) * 2.0 ** OTHER[shift]
    assert s_feat != s_tail
    for cfg in (0, 1, 2, 3, 4, 5, 6):
        mf = c8.ActC8(B, 128, H, W, DEV, scale=s_feat, tail=tail)
        mf.tail_scale = s_tail
        c8.conv2d_c8(acts, enc, relu=True, out_c8=mf, tail=flow, cfg=cfg)
        got = R.unpack_ref(mf)
        e_feat, e_tail = _rel(got[:, :128 - tail], want), _rel(got[:, 128 - tail:], flow)
        assert e_feat <= CONV and e_tail <= CONV, (cfg, e_feat, e_tail)
        assert torch.equal(R.to_channels(mf.t)[:, 128 - tail:128], R.to_channels(R.pack_ref(flow, s_tail).t)[:, :tail]), cfg
        assert float(R.outside_interior(mf).float().abs().max()) == 0.0
        assert torch.equal(c8.unpack(mf), got.float())
    print("tail %d: features %.2e, tail %.2e" % (tail, e_feat, e_tail))
    # as an operand, beside a second one at another scale
    up, s_up = _operand((B, 128, H, W), 1.0, 3, "tanh", gen=g)
    a_up = R.pack_ref(up, s_up)
    nxt = torch.nn.Conv2d(256, 64, 3, padding=1).to(DEV)
    nxt.weight.copy_(R.balance_weights(nxt.weight, [128 - tail, tail, 128], [m_feat, 100.0, 1.0]))
    for order in (0, 1):
        srcs = [mf, a_up] if order == 0 else [a_up, mf]
        w = nxt.weight if order == 0 else torch.cat([nxt.weight[:, 128:], nxt.weight[:, :128]], 1)
        lay = torch.nn.Conv2d(256, 64, 3, padding=1).to(DEV)
        lay.weight.copy_(w)
        lay.bias.copy_(nxt.bias)
        ref = R.conv_ref64([R.unpack_ref(a) for a in srcs], lay.weight, lay.bias)
        # every segment matters to the output: without it the result moves by far more than the bound
        for lo, hi in ((0, 128 - tail), (128 - tail, 128), (128, 256)):
            part = R.unpack_ref(mf)[:, lo:hi] if hi <= 128 else R.unpack_ref(a_up)
            wpart = nxt.weight[:, lo:hi]
            assert float(R.conv_ref64([part], wpart).abs().max() / ref.abs().max()) >= 0.01
        for cfg in (0, 1, 2, 3, 4):
            e = _rel(c8.conv2d_c8(srcs, lay, cfg=cfg), ref)
            assert e <= CONV, (order, cfg, e)
    print("tailed operand: %.2e" % e)


@torch.no_grad()
@pytest.mark.parametrize("case", [(1, 33, 37, 48, 40, R.M_LO, 0), (2, 50, 70, 64, 96, R.M_HI, 3), (1, 46, 78, 64, 64, 1.0, -4),
                                  (1, 184, 312, 64, 64, R.M_LO, 3)])
def test_conv_c8_residual_epilogue_with_a_scaled_destination(case):
    c8 = _c8()
    B, H, W, cin, cout, mag, shift = case
    torch.manual_seed(cin + H)
    g = _gen(cin + H)
    x, s = _operand((B, cin, H, W), mag, OTHER[shift], gen=g)
    res = torch.randn((B, cout, H, W), device=DEV, generator=g) * mag
    layer = torch.nn.Conv2d(cin, cout, 3, padding=1).to(DEV)
    layer.bias.mul_(mag)
    a = R.pack_ref(x, s)
    want = R.conv_ref64([R.unpack_ref(a)], layer.weight, layer.bias, relu=True, residual=res)
    s_out = R.calibrated_scale(want) * 2.0 ** shift
    for cfg in (0, 1, 2, 3, 4, 5, 6):
        r = res.clone()
        oc = c8.ActC8(B, cout, H, W, DEV, scale=s_out)
        y = c8.residual_c8([a], layer, r, relu=True, out=r, out_c8=oc, cfg=cfg)
        assert y is r and _rel(y, want) <= CONV, (case, cfg, _rel(y, want))
        assert _rel(R.unpack_ref(oc), want) <= CONV
        assert torch.equal(R.unpack_ref(oc), R.unpack_ref(R.pack_ref(y, s_out))), (case, cfg)
        assert float(R.outside_interior(oc).float().abs().max()) == 0.0


def _w_hi_folded(w, chans, scales):
    """The hi plane of the packed image of weights with 1 / scale folded per operand, back at the weights' own scale."""
    inv = torch.cat([torch.full((c,), 1.0 / s, device=w.device) for c, s in zip(chans, scales)]).view(1, -1, 1, 1)
    wf = w.float() * inv
    e = 12 - math.floor(math.log2(float(wf.abs().max())))
    return (wf * 2.0 ** e).half().double() * 2.0 ** -e / inv.double()


@torch.no_grad()
@pytest.mark.parametrize("passes", [1, 2])
@pytest.mark.parametrize("case", [(1, [128, 64, 64], 256, 33, 37, 1, "one_hi_lo"), (2, [16, 48], 64, 50, 70, 3, "lo_hi"),
                                  (1, [64, 64], 64, 46, 78, 4, "edge_high"), (1, [128, 128], 128, 23, 39, 2, "edge_low")],
                         ids=lambda c: "%s-cfg%d" % (c[6], c[5]))
def test_conv_c8_reduced_passes_round_the_scaled_operands(case, passes):
    """test_gpu_round5.py, test_conv_c8_reduced_passes_are_the_rounded_operand_convolution, with scaled operands: the rounding
    acts on x * scale (passes 2) and additionally on the folded weights (passes 1); same two bounds."""
    c8 = _c8()
    B, chans, cout, H, W, cfg, config = case
    xs, acts, layer, g = _conv_case(B, H, W, chans, cout, config, True, 1.0, seed=cout + H + passes)
    with c8.passes(passes):
        got = c8.conv2d_c8(acts, layer, relu=False, cfg=cfg)
    rounded = [(x * a.scale).half().double() / a.scale for x, a in zip(xs, acts)]
    w = _w_hi_folded(layer.weight, chans, [a.scale for a in acts]) if passes == 1 else layer.weight
    want = R.conv_ref64(rounded, w, layer.bias)
    full = R.conv_ref64(xs, layer.weight, layer.bias)
    rel, off = _rel(got, want), _rel(got, full)
    print("passes %d %s: vs rounded-operand fp64 %.2e, vs the exact convolution %.2e" % (passes, config, rel, off))
    assert rel <= CONV                # test_gpu_round5.py: rel <= 3e-6
    assert off >= 1e-5                # test_gpu_round5.py: and it IS the reduced arithmetic


@torch.no_grad()
def test_two_c8_destinations_with_different_scales_are_refused():
    c8 = _c8()
    torch.manual_seed(0)
    B, H, W = 1, 16, 32
    zr = torch.nn.Conv2d(256, 256, 3, padding=1).to(DEV)
    h = torch.tanh(torch.randn(B, 128, H, W, device=DEV))
    a_h, a_x = R.pack_ref(h, 1024.0), R.pack_ref(torch.randn(B, 128, H, W, device=DEV), 256.0)
    z = torch.empty_like(h)
    o1, o2 = c8.ActC8(B, 256, H, W, DEV, scale=64.0), c8.ActC8(B, 128, H, W, DEV, scale=1024.0)
    with pytest.raises(ValueError):
        c8.desc([a_h, a_x], zr, out=z, epilogue=1, e0=z, e1=z, h=h, out_c8=o1, out2_c8=o2)
    o1.scale = 1024.0
    assert c8.desc([a_h, a_x], zr, out=z, epilogue=1, e0=z, e1=z, h=h, out_c8=o1, out2_c8=o2).act_scale == 1024.0


# ---- d. gates and the fused ConvGRU launch -----------------------------------------------------------------------------------
class _Gru:
    """One ConvGRU with a state at magnitude `m_h` and operands at magnitudes of their own; the second operand may carry a tail.
    Weights are balanced: every operand contributes alike to the three convolutions, whose results sit at magnitude 1.
    `z_shift` (negative) keeps a state at magnitude 2^-10 there, so that it keeps its (large) scale: in
    h' = (1 - z) h + z q the product z q has to be of h's size, and the smallness is split between the two factors
    (z = sigmoid(. + z_shift) ~ 2^-7.8, q = tanh(Q_SMALL .) ~ 2^-8).  Neither factor alone may carry it when the bound is
    relative to max |h'| ~ 2^-9: the kernels evaluate tanh as (e^2x - 1) / (e^2x + 1), absolute error 3e-8, i.e. 8e-6 of that
    maximum if z were of size 1; and the one-launch form starts its accumulators at (bias + context) / scale, so a context of
    -9.7 (z ~ 2^-14 alone) costs ~216 roundings at that magnitude, 4e-6 in z -- measured: h' off by 5.8e-6 and 8.6e-6 in the one
    launch, 0.7e-6 in the two launches that add the context in their epilogue.  With the split, either effect stays near 1e-6."""

    def __init__(self, B, H, W, xch, config, m_h, sh_h, tail, seed, z_shift=0.0):
        from dkt_stereo_amd.update import ConvGRU
        c8 = _c8()
        torch.manual_seed(seed)
        g = self.g = _gen(seed)
        cfgs = R.OPERAND_CONFIGS[config][:len(xch)]
        self.gru = ConvGRU(128, sum(xch)).to(DEV)
        self.h, self.s_h = _operand((B, 128, H, W), m_h, sh_h, "tanh", gen=g)
        if z_shift:
            self.s_h /= 4.0                                # (room for the new state: z q reaches the size of h)
        self.xs, self.acts, segs = [], [], [(128, m_h)]
        for i, (c, (mag, shift)) in enumerate(zip(xch, cfgs)):
            t = tail if i == len(xch) - 1 else 0
            x, s = _operand((B, c, H, W), mag, shift, "relu" if i else "randn", gen=g)
            if t:
                x[:, c - t:] = torch.randn((B, t, H, W), device=DEV, generator=g) * 100.0
                a = R.pack_ref(x, R.calibrated_scale(x[:, :c - t]) * 2.0 ** shift, tail=t, tail_scale=R.calibrated_scale(x[:, c - t:]))
                assert len(a.channel_scales()) == 2
                segs += [(c - t, mag), (t, 100.0)]
            else:
                a = R.pack_ref(x, s)
                segs += [(c, mag)]
            self.xs.append(x)
            self.acts.append(a)
        assert len({self.s_h} | {a.scale for a in self.acts}) == 1 + len(self.acts)
        ch, mg = [c for c, _ in segs], [m for _, m in segs]
        m_q = Q_SMALL if z_shift else 1.0
        for conv, m_out in ((self.gru.convz, 1.0), (self.gru.convr, 1.0), (self.gru.convq, m_q)):
            conv.weight.copy_(R.balance_weights(conv.weight, ch, mg) * m_out)
            conv.bias.mul_(m_out)
        self.cz, self.cr, self.cq = (torch.randn((B, 128, H, W), device=DEV, generator=g) for _ in range(3))
        self.cq *= m_q
        if z_shift:
            self.cz = self.cz * 0.25 + z_shift
        self.hc8 = R.pack_ref(self.h, self.s_h)
        self.rh = c8.ActC8(B, 128, H, W, DEV, scale=self.s_h)
        self.flags = c8.gru_flags(B, H, W, DEV)
        self.B, self.H, self.W = B, H, W

    def operands64(self):
        return [R.unpack_ref(a) for a in self.acts]

    def desc(self):
        return _c8().gru_desc(self.gru, self.hc8, self.acts, self.rh, self.cz, self.cr, self.cq, self.h, self.flags)


#: the update gate (ln 2^-7.8) and the candidate's magnitude for a state at magnitude 2^-10 (see _Gru)
Z_CLOSED, Q_SMALL = -7.8 * math.log(2.0), 2.0 ** -8
_GRU_CASES = [(1, 23, 39, [128], "lo_hi", 1.0, 0, 0, 0.0), (1, 50, 70, [64, 40, 24], "one_hi_lo", 1.0, 3, 0, 0.0),
              (2, 33, 37, [128, 128], "edge_mixed", 1.0, -4, 2, 0.0), (1, 46, 78, [128, 128], "lo_hi", R.M_LO, 0, 1, Z_CLOSED),
              (1, 33, 37, [128, 128], "edge_high", R.M_LO, 3, 2, Z_CLOSED), (2, 184, 312, [128, 128], "edge_low", 1.0, 0, 2, 0.0)]
_GRU_IDS = ["%s-h%g-%dx%d" % (c[4], c[5], c[1], c[2]) for c in _GRU_CASES]


@torch.no_grad()
@pytest.mark.parametrize("B,H,W,xch,config,m_h,sh_h,tail,z_shift", _GRU_CASES, ids=_GRU_IDS)
def test_gate_launches_with_scaled_state_and_operands(B, H, W, xch, config, m_h, sh_h, tail, z_shift):
    """gate_zr + gate_out: z and r*h against fp64 on the decoded operands, h' against fp64 on the decoded r*h and the z of the first
    launch (stage by stage) and against the whole step; the C8S twin is the split of the fp32 state at the state's scale."""
    c8 = _c8()
    s = _Gru(B, H, W, xch, config, m_h, sh_h, tail, seed=H + len(xch), z_shift=z_shift)
    x64 = s.operands64()
    for cfg_zr, cfg_q in ((1, 2), (4, 4), (0, 0)):
        s.rh.t.zero_()
        z = c8.gate_zr([s.hc8, *s.acts], s.gru._merged_zr(), s.cz, s.cr, s.h, rh_c8=s.rh, cfg=cfg_zr)
        want_z, want_rh = R.gate_zr_ref64(s.gru, s.h, x64, s.cz, s.cr)
        e_z, e_rh = _rel(z, want_z), _rel(R.unpack_ref(s.rh), want_rh)
        out, out_c8 = torch.empty_like(s.h), c8.ActC8(B, 128, H, W, DEV, scale=s.s_h)
        c8.gate_out([s.rh, *s.acts], s.gru.convq, s.cq, z, s.h, out, out_c8=out_c8, cfg=cfg_q)
        e_q = _rel(out, R.gate_out_ref64(s.gru, R.unpack_ref(s.rh), x64, s.cq, z, s.h))
        e_h = _rel(out, R.gru_ref64(s.gru, s.h, x64, s.cz, s.cr, s.cq))
        print("gates cfg %d/%d: z %.2e r*h %.2e h' (stage) %.2e h' (step) %.2e" % (cfg_zr, cfg_q, e_z, e_rh, e_q, e_h))
        assert e_z <= CONV and e_rh <= CONV and e_q <= CONV and e_h <= GRU
        assert torch.equal(out_c8.t, R.pack_ref(out, s.s_h).t)
        assert float(R.outside_interior(s.rh).float().abs().max()) == 0.0


@torch.no_grad()
@pytest.mark.parametrize("B,H,W,xch,config,m_h,sh_h,tail,z_shift", _GRU_CASES, ids=_GRU_IDS)
def test_fused_gru_launch_with_scaled_state_and_operands(B, H, W, xch, config, m_h, sh_h, tail, z_shift):
    """Three dependent steps of the one-launch ConvGRU on the same flag words: h against fp64, the C8S twin bit for bit the split of
    h at the state's scale, r*h decoded against fp64 r*h, error word 0."""
    c8 = _c8()
    s = _Gru(B, H, W, xch, config, m_h, sh_h, tail, seed=H + len(xch) + 1, z_shift=z_shift)
    x64 = s.operands64()
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    for step in range(3):
        h_in = s.h.clone()
        assert torch.equal(s.hc8.t, R.pack_ref(h_in, s.s_h).t)
        want = R.gru_ref64(s.gru, h_in, x64, s.cz, s.cr, s.cq)
        want_rh = R.gate_zr_ref64(s.gru, h_in, x64, s.cz, s.cr)[1]
        assert c8.gru_launch(s.desc(), err=err), "the device declined a launch it must be able to hold"
        e_h, e_rh = _rel(s.h, want), _rel(R.unpack_ref(s.rh), want_rh)
        print("fused step %d: h %.2e r*h %.2e (state scale 2^%d, max |h s| %.0f)" % (step, e_h, e_rh, math.log2(s.s_h), float(s.h.abs().max()) * s.s_h))
        assert e_h <= GRU and e_rh <= GRU, (step, e_h, e_rh)
        assert torch.equal(s.hc8.t, R.pack_ref(s.h, s.s_h).t)
        assert float(R.outside_interior(s.rh).float().abs().max()) == 0.0
    assert int(err.item()) == 0
    assert int(s.flags.min()) == 3 and int(s.flags.max()) == 3


@torch.no_grad()
def test_fused_gru_pair_with_scaled_operands():
    """Two steps in one launch (the finest level with the coarsest riding along), each with scales of its own, against fp64."""
    c8 = _c8()
    big = _Gru(1, 46, 78, [128, 128], "edge_mixed", 1.0, 3, 2, seed=5)
    small = _Gru(1, 23, 39, [128], "lo_hi", R.M_LO, 0, 0, seed=6, z_shift=Z_CLOSED)
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    wants = [R.gru_ref64(t.gru, t.h, t.operands64(), t.cz, t.cr, t.cq) for t in (big, small)]
    assert c8.gru_launch(big.desc(), small.desc(), err=err)
    for t, want in zip((big, small), wants):
        assert _rel(t.h, want) <= GRU, _rel(t.h, want)
        assert torch.equal(t.hc8.t, R.pack_ref(t.h, t.s_h).t)
    assert int(err.item()) == 0


# ---- e. head ----------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("B,H,W,m_h,shift", [(1, 46, 78, 1.0, 0), (2, 33, 37, R.M_LO, 3), (1, 50, 70, R.M_LO, -4), (1, 184, 312, 1.0, 3)])
def test_flow_head_with_a_scaled_state(B, H, W, m_h, shift):
    """head_planes + dkt_head_finish on a scaled state operand: coordinate and flow against an fp64 FlowHead
    (core/update.py:6-14, raft_stereo.py:165-168)."""
    from dkt_stereo_amd.update import FlowHead, _leading_outputs
    c8 = _c8()
    torch.manual_seed(H)
    g = _gen(H)
    fh = FlowHead(128, 256, 2).to(DEV)
    fh.conv1.weight.div_(m_h)
    h, s_h = _operand((B, 128, H, W), m_h, shift, "tanh", gen=g)
    a = R.pack_ref(h, s_h)
    coords0 = torch.randn((B, 2, H, W), device=DEV, generator=g) * 10
    want_d = R.flow_head_ref64(fh.conv1, fh.conv2, [R.unpack_ref(a)])[:, :1]
    want_c = (coords0 + 1.5).double()
    want_c[:, :1] += want_d
    coords1 = coords0.clone() + 1.5
    flow = torch.zeros((B, 2, H, W), device=DEV)
    c8.head([a], fh.conv1, _leading_outputs(fh.conv2, 1), coords1[:, :1], diff=(coords0[:, :1], flow[:, :1]), cfg=2)
    e = float((coords1.double() - want_c).abs().max()) / max(1.0, float(want_d.abs().max()))
    print("head: %.2e (max |delta| %.2f)" % (e, float(want_d.abs().max())))
    assert float(want_d.abs().max()) >= 0.1          # (the head's output matters beside the coordinate's own rounding)
    assert e <= HEAD
    assert torch.equal(flow[:, :1], coords1[:, :1] - coords0[:, :1]) and torch.equal(coords1[:, 1:], coords0[:, 1:] + 1.5)


# ---- f. one loop iteration, stage by stage ----------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("B,H,W,mags", [(1, 46, 78, (1.0, R.M_LO, R.M_HI)), (2, 40, 96, (1.0, R.M_HI, R.M_LO))])
def test_one_iteration_stage_by_stage(B, H, W, mags):
    """motion front -> cor / flo 3x3 layers -> encoder 3x3 with the flow tail -> finest ConvGRU -> flow head, every tensor at its own
    calibrated scale.  Each stage's fp64 reference takes the decoded output of the previous kernel, so each keeps its bound."""
    from dkt_stereo_amd.update import ConvGRU, _leading_outputs
    c8 = _c8()
    front = _Front(B, H, W, 4, mags, (0, 0, 0), seed=H)
    hc8, cor, flo, flow, c_new = front.run()
    g = front.g
    m_c, m_f = mags[1], mags[2]

    def layer(cin, cout, chans, in_mags, out_mag):
        lay = torch.nn.Conv2d(cin, cout, 3, padding=1).to(DEV)
        lay.weight.copy_(R.balance_weights(lay.weight, chans, in_mags) * out_mag)
        lay.bias.mul_(out_mag)
        return lay

    # convc2 / convf2 into the two halves of one tensor (core/update.py:73-77), which therefore carries ONE scale
    c2, f2 = layer(64, 64, [64], [m_c], 3.0), layer(64, 64, [64], [m_f], 3.0)
    want_c2 = R.conv_ref64([R.unpack_ref(cor)], c2.weight, c2.bias, relu=True)
    want_f2 = R.conv_ref64([R.unpack_ref(flo)], f2.weight, f2.bias, relu=True)
    cf = c8.ActC8(B, 128, H, W, DEV, scale=R.calibrated_scale(torch.cat([want_c2, want_f2], 1)))
    c8.conv2d_c8([cor], c2, relu=True, out_c8=cf, out_c8_ch0=0, cfg=4)
    c8.conv2d_c8([flo], f2, relu=True, out_c8=cf, out_c8_ch0=64, cfg=4)
    e_cf = (_rel(R.unpack_ref(cf, 64, 0), want_c2), _rel(R.unpack_ref(cf, 64, 64), want_f2))
    # encoder output + flow tail
    enc = layer(128, 126, [128], [3.0], 0.01)
    want_mf = R.conv_ref64([R.unpack_ref(cf)], enc.weight, enc.bias, relu=True)
    mf = c8.ActC8(B, 128, H, W, DEV, scale=R.calibrated_scale(want_mf), tail=2)
    mf.tail_scale = R.calibrated_scale(flow)
    c8.conv2d_c8([cf], enc, relu=True, out_c8=mf, tail=flow, cfg=3)
    got_mf = R.unpack_ref(mf)
    e_mf = (_rel(got_mf[:, :126], want_mf), _rel(got_mf[:, 126:], flow))
    assert len({hc8.scale, cor.scale, flo.scale, cf.scale, mf.scale, mf.tail_scale}) >= 5
    # finest ConvGRU on [h | motion features + flow | interp(net[1])]
    up, s_up = _operand((B, 128, H, W), 1.0, 0, "tanh", gen=g)
    a_up = R.pack_ref(up, s_up)
    torch.manual_seed(W)
    gru = ConvGRU(128, 256).to(DEV)
    segs, sm = [128, 126, 2, 128], [mags[0], 0.01, float(flow.abs().max()), 1.0]
    for conv in (gru.convz, gru.convr, gru.convq):
        conv.weight.copy_(R.balance_weights(conv.weight, segs, sm))
    cz, cr, cq = (torch.randn((B, 128, H, W), device=DEV, generator=g) for _ in range(3))
    h = front.h.clone()
    x64 = [R.unpack_ref(mf), R.unpack_ref(a_up)]
    want_h = R.gru_ref64(gru, h, x64, cz, cr, cq)
    rh = c8.ActC8(B, 128, H, W, DEV, scale=hc8.scale)
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    assert c8.gru_launch(c8.gru_desc(gru, hc8, [mf, a_up], rh, cz, cr, cq, h, c8.gru_flags(B, H, W, DEV)), err=err)
    e_h = _rel(h, want_h)
    assert torch.equal(hc8.t, R.pack_ref(h, hc8.scale).t) and int(err.item()) == 0
    # flow head on the new state
    want_d = R.flow_head_ref64(front.fh.conv1, front.fh.conv2, [R.unpack_ref(hc8)])[:, :1]
    x1 = c_new[:, :1].clone()
    want_x = x1.double() + want_d
    c8.head([hc8], front.fh.conv1, _leading_outputs(front.fh.conv2, 1), x1, cfg=2)
    e_x = float((x1.double() - want_x).abs().max()) / max(1.0, float(want_d.abs().max()))
    print("iteration: cf %.2e %.2e, mf %.2e tail %.2e, h %.2e, x %.2e" % (*e_cf, *e_mf, e_h, e_x))
    assert max(e_cf) <= CONV and max(e_mf) <= CONV and e_h <= GRU and e_x <= HEAD
