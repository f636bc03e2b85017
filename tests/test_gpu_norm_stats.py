"""-m gpu: normalisation statistics against fp64 on the planes where they go wrong.

The encoders' instance norm (core/extractor.py:21-60) and the folded eval-mode BatchNorm see planes whose mean is far larger
than their spread (a dark or foggy frame normalised to [-1, 1]), spreads near eps, constant planes, planes a ReLU zeroed and
BatchNorm running statistics spread over decades.  The random-init suite never builds those.  Here the convolution itself
makes them: the bias sets a channel's mean M, the norm of its filter the spread sigma (x ~ N(0, 1)).

Bound.  Per plane, the HIP result may be no farther from fp64 than twice what torch's own fp32 arithmetic on the GPU reaches
on the same stored data, plus 1e-6: F.instance_norm for the normalised output (relative to the plane's largest normalised
value, at least 1), torch.var_mean for 1/std.  The normalised outputs also carry the cost of the fp32 mean every consumer
applies (half an ulp of the mean times 1/std; torch applies an fp32 mean too, but its rounding lands elsewhere).  The bound
follows the input's conditioning, not a constant picked for random data.
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

EPS = 1e-5
# 3.9 and 4.1 sit either side of the point above which the statistics are recomputed from the stored output (norm.hip,
# CONV_STATS_TRUST = 16 on mean^2 / var): 3.9 is the worst case the epilogue's fp32 sums are trusted with
RATIOS = (0.0, 1.0, 3.9, 4.1, 1e2, 1e3, 1e4)


def _regime(name, cout):
    """(mean, sigma) per output channel, and whether the layer applies a ReLU."""
    if name == "offset":           # m / sigma over RATIOS, both signs, two spreads
        n = len(RATIOS)
        ms = [(RATIOS[c % n] * s * (-1) ** (c // n), s) for c in range(cout) for s in [(1.0, 0.37)[(c // (2 * n)) % 2]]]
        return ms, False
    if name == "near_eps":         # sigma^2 at 0.1, 1 and 10 times eps, centred and offset by 10 sigma
        ms = []
        for c in range(cout):
            s = (0.1 * EPS, EPS, 10 * EPS)[c % 3] ** 0.5
            ms.append((10 * s * (c // 3 % 2), s))
        return ms, False
    if name == "constant":         # zero filters: exactly constant planes
        return [((0.0, 1.0, -3.5, 128.0, 1e4)[c % 5], 0.0) for c in range(cout)], False
    if name == "relu":             # all zero after the ReLU, mostly zero, half, never clipped at an offset of 10^3
        return [((-100.0, -2.0, 0.0, 1e3)[c % 4], 1.0) for c in range(cout)], True
    raise ValueError(name)


def _hard_layer(cin, cout, k, stride, regime, seed):
    g = torch.Generator().manual_seed(seed)
    layer = nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2)
    ms, relu = _regime(regime, cout)
    w = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64)
    w = w / w.flatten(1).norm(dim=1).view(-1, 1, 1, 1)
    with torch.no_grad():
        layer.weight.copy_(w * torch.tensor([s for _, s in ms], dtype=torch.float64).view(-1, 1, 1, 1))
        layer.bias.copy_(torch.tensor([m for m, _ in ms], dtype=torch.float64))
    return layer.to(DEV), relu


def _in64(t):
    """InstanceNorm2d(affine=False) in fp64 (written out: F.instance_norm refuses 1 x 1 planes)."""
    t = t.double()
    m = t.mean((2, 3), keepdim=True)
    return (t - m) * (t.var((2, 3), unbiased=False, keepdim=True) + EPS).rsqrt()


def _in32(t):
    """torch's own fp32 instance norm on the GPU (a 1 x 1 plane normalises to 0)."""
    return F.instance_norm(t, eps=EPS) if t.shape[2] * t.shape[3] > 1 else torch.zeros_like(t)


def _per_plane(d, ref=None):
    """max |d| per (batch, channel) plane, flattened; with `ref`, relative to the plane's max(1, max |ref|) (a ReLU plane
    that is mostly zero normalises to values of ~80)."""
    e = d.abs().flatten(2).amax(2).reshape(-1)
    return e if ref is None else e / ref.abs().flatten(2).amax(2).reshape(-1).clamp(min=1.0)


def _mean_quantum(*planes):
    """Per plane, what storing the mean as fp32 (the (mean, 1/std) float pairs every consumer applies) costs in the
    normalised output: half an fp32 ulp of the mean times 1/std, summed over the normalised operands."""
    q = 0.0
    for t in planes:
        o = t.double().flatten(2)
        m = o.mean(2).reshape(-1).float()
        ulp = (torch.nextafter(m.abs(), torch.full_like(m, float("inf"))) - m.abs()).double()
        q = q + 0.5 * ulp * (o.var(2, unbiased=False).reshape(-1) + EPS).rsqrt()
    return q


def _istd_err(out, istd):
    o = out.double().flatten(2)
    want = (o.var(2, unbiased=False) + EPS).rsqrt().reshape(-1)
    return (istd.double().reshape(-1) / want - 1).abs()


def _torch_istd(out):
    v, _ = torch.var_mean(out.flatten(2), dim=2, unbiased=False)
    return (v + EPS).rsqrt().reshape(-1)


def _check_params(out, params, what):
    """(mean, 1/std) per plane of `out` against fp64: the normalised output they give (applied in fp64, so that only the
    statistics are judged) and 1/std itself.  Returns the largest 1/std error."""
    y64 = _in64(out)
    mean, istd = params[:, 0].double(), params[:, 1].double()
    B, C = out.shape[:2]
    got = (out.double() - mean.view(B, C, 1, 1)) * istd.view(B, C, 1, 1)
    e_y = _per_plane(got - y64, y64)
    t_y = _per_plane(_in32(out).double() - y64, y64)
    bad = e_y > 2 * t_y + 1e-6 + _mean_quantum(out)
    assert not bool(bad.any()), "%s: normalised output %.3e from fp64 (torch fp32 %.3e) on plane %d" % (
        what, float(e_y[bad].max()), float(t_y[bad][e_y[bad].argmax()]), int(bad.nonzero()[0]))
    e_i = _istd_err(out, istd)
    t_i = _istd_err(out, _torch_istd(out))
    bad = e_i > 2 * t_i + 1e-6
    assert not bool(bad.any()), "%s: 1/std %.3e from fp64 (torch fp32 %.3e) on plane %d" % (
        what, float(e_i[bad].max()), float(t_i[bad][e_i[bad].argmax()]), int(bad.nonzero()[0]))
    return e_i


def _report(regime, out, e_i, ratios):
    """The 1/std error per m / sigma class (what the PR table quotes)."""
    if regime != "offset":
        print("%s: max 1/std error %.3e" % (regime, float(e_i.max())))
        return
    B, C = out.shape[:2]
    cls = torch.tensor([ratios[c % len(ratios)] for c in range(C)] * B, device=e_i.device)
    print("  ".join("m/sigma %g: %.3e" % (r, float(e_i[cls == r].max())) for r in ratios))


# (B, Cin, Cout, H, W, stride, k): the tile shapes of test_gpu_round4's statistics test, 1 x 1 planes, ragged planes
SHAPES = [(2, 64, 64, 96, 160, 1, 3), (2, 64, 96, 96, 160, 2, 3), (1, 96, 128, 47, 81, 2, 3), (2, 64, 96, 90, 130, 2, 1),
          (1, 128, 128, 40, 72, 1, 3), (3, 32, 40, 33, 70, 1, 3), (2, 96, 96, 93, 157, 1, 3), (1, 96, 80, 120, 200, 1, 3),
          (2, 64, 96, 264, 544, 2, 3), (2, 96, 128, 264, 544, 2, 3),
          (2, 64, 64, 1, 1, 1, 3), (1, 64, 96, 2, 1, 2, 1), (2, 48, 72, 1, 37, 1, 3), (1, 64, 64, 40, 50, 1, 3)]
REGIMES = ("offset", "near_eps", "constant", "relu")


def _epilogue_case(shape, regime, seed):
    from dkt_stereo_amd import conv, extractor
    B, cin, cout, H, W, stride, k = shape
    layer, relu = _hard_layer(cin, cout, k, stride, regime, seed)
    x = torch.randn(B, cin, H, W, generator=torch.Generator().manual_seed(seed + 1)).to(DEV)
    norm = nn.InstanceNorm2d(cout, eps=EPS)
    with conv.use_backend("f16x3"):
        assert conv.stats_eligible(layer), "layer not on the statistics epilogue"
        out, st = conv.conv2d_stats(x, layer, relu=relu)
        params = extractor.instance_norm_params(norm, out, st)
        # the consumer that reads the epilogue's partial sums in the encoders: relu(a + relu(norm(out))), a = 0
        joined = extractor.norm_add_relu(norm, torch.zeros_like(out), out, st)
    e_i = _check_params(out, params, regime)
    y64 = _in64(out).relu()
    e_y = _per_plane(joined.double() - y64, y64)
    t_y = _per_plane(_in32(out).relu().double() - y64, y64)
    assert bool((e_y <= 2 * t_y + 1e-6 + _mean_quantum(out)).all()), "%s: norm_add_relu on the epilogue statistics %.3e (torch fp32 %.3e)" % (
        regime, float(e_y.max()), float(t_y.max()))
    return out, e_i


@torch.no_grad()
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", SHAPES)
def test_epilogue_statistics_match_fp64_on_hard_planes(shape, regime, monkeypatch):
    """conv.conv2d_stats on the split-fp16 kernel (dkt_conv_desc.stats_ws) against fp64 statistics of the stored output."""
    monkeypatch.setenv("DKT_CONV_WS", "0")
    out, e_i = _epilogue_case(shape, regime, sum(shape) + len(regime))
    _report(regime, out, e_i, RATIOS)


# 64 -> 64 3x3 stride 1 with at least 192 tiles of 8 x 32 pixels: the weights-stationary kernel (conv_ws.h)
WS_SHAPES = [(3, 64, 64, 64, 256, 1, 3), (4, 64, 64, 93, 157, 1, 3), (1, 64, 64, 184, 312, 1, 3)]


@torch.no_grad()
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", WS_SHAPES)
def test_weights_stationary_epilogue_statistics_match_fp64_on_hard_planes(shape, regime, monkeypatch):
    """The same through conv_ws.h's statistics epilogue.  Its summation order differs from the streaming kernel's, so
    a different output (with the kernel switched off) shows that it ran."""
    from dkt_stereo_amd import conv
    seed = sum(shape) + len(regime)
    monkeypatch.setenv("DKT_CONV_WS", "1")
    out, e_i = _epilogue_case(shape, regime, seed)
    _report(regime, out, e_i, RATIOS)
    if regime == "offset":
        monkeypatch.setenv("DKT_CONV_WS", "0")
        B, cin, cout, H, W, stride, k = shape
        layer, relu = _hard_layer(cin, cout, k, stride, regime, seed)
        x = torch.randn(B, cin, H, W, generator=torch.Generator().manual_seed(seed + 1)).to(DEV)
        with conv.use_backend("f16x3"):
            streaming, _ = conv.conv2d_stats(x, layer, relu=relu)
        assert not torch.equal(streaming, out), "the weights-stationary kernel did not run"


def _planes(B, C, H, W, regime, seed):
    """Hard planes built directly (M + sigma * z in fp32), for the kernels that take statistics in a pass of their own."""
    ms, relu = _regime(regime, C)
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    m = torch.tensor([a for a, _ in ms], dtype=torch.float64).view(1, C, 1, 1)
    s = torch.tensor([b for _, b in ms], dtype=torch.float64).view(1, C, 1, 1)
    t = m + s * z
    return (t.relu() if relu else t).float().to(DEV)


@torch.no_grad()
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("B,C,H,W", [(2, 40, 33, 70), (1, 64, 1, 1), (3, 20, 7, 5), (1, 24, 184, 312)])
def test_statistics_pass_consumers_match_fp64_on_hard_planes(B, C, H, W, regime):
    """dkt_instance_norm (with and without ReLU), dkt_instance_norm_add_relu, dkt_instance_norm_add_relu_lazy and
    dkt_instance_norm_join_c8 on statistics from dkt_instance_norm_stats (fp64 squares): pinned on the same planes."""
    from dkt_stereo_amd import conv_c8, extractor
    norm = nn.InstanceNorm2d(C, eps=EPS)
    seed = B * 1000 + C + H + len(regime)
    c = _planes(B, C, H, W, regime, seed)
    a = _planes(B, C, H, W, REGIMES[(REGIMES.index(regime) + 1) % len(REGIMES)], seed + 1)
    pc = extractor.instance_norm_params(norm, c)
    pa = extractor.instance_norm_params(norm, a)
    _check_params(c, pc, regime + " stats pass")
    n64c, n64a = _in64(c), _in64(a)
    n32c, n32a = _in32(c), _in32(a)

    def check(got, want, torch32, what, *normed):
        e, t = _per_plane(got.double() - want, want), _per_plane(torch32.double() - want, want)
        bad = e > 2 * t + 1e-6 + _mean_quantum(*normed)
        assert not bool(bad.any()), "%s (%s): %.3e from fp64, torch fp32 %.3e" % (what, regime, float(e.max()), float(t[bad].max()))

    for relu in (False, True):
        want = n64c.relu() if relu else n64c
        check(extractor.norm_act(norm, c, relu), want, n32c.relu() if relu else n32c, "dkt_instance_norm relu=%d" % relu, c)
    r = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed + 2)).to(DEV)
    check(extractor.norm_add_relu(norm, r, c), (r.double() + n64c.relu()).relu(), (r + n32c.relu()).relu(),
          "dkt_instance_norm_add_relu", c)
    want = (n64a.relu() + n64c.relu()).relu()
    torch32 = (n32a.relu() + n32c.relu()).relu()
    check(extractor.norm_add_relu(norm, extractor.LazyNorm(norm, a, True), c), want, torch32, "dkt_instance_norm_add_relu_lazy",
          a, c)
    y = torch.empty_like(c)
    conv_c8.norm_join_c8(c, pc, True, a=a, a_params=pa, a_relu=True, y=y)
    check(y, want, torch32, "dkt_instance_norm_join_c8", a, c)


# ---- BatchNorm folded into the convolution (extractor._fold: cnet's frozen statistics, raft_stereo.py:56-59) ----

def _trained_bn(cout, seed):
    """running_var log-uniform in [1e-4, 1e2], |running_mean| up to 10 sigma, gamma of either sign with every fifth channel
    at 1e-4, beta of order 0.5."""
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(cout, eps=EPS)
    var = 10.0 ** (torch.rand(cout, generator=g, dtype=torch.float64) * 6 - 4)
    mean = (torch.rand(cout, generator=g, dtype=torch.float64) * 20 - 10) * var.sqrt()
    gamma = (0.5 + 1.5 * torch.rand(cout, generator=g, dtype=torch.float64)) * torch.where(
        torch.rand(cout, generator=g) < 0.3, -1.0, 1.0).double()
    gamma[::5] = 1e-4
    beta = 0.5 * torch.randn(cout, generator=g, dtype=torch.float64)
    with torch.no_grad():
        bn.running_var.copy_(var)
        bn.running_mean.copy_(mean)
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    return bn.eval()


@torch.no_grad()
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("B,cin,cout,k,stride,H,W", [(2, 3, 64, 7, 1, 40, 72),       # the 7x7 stem (dkt_conv2d_stem7)
                                                     (1, 64, 96, 3, 1, 33, 70),      # split-fp16 3x3
                                                     (2, 96, 96, 3, 2, 46, 78),      # stride 2
                                                     (1, 64, 128, 1, 2, 47, 81)])    # 1x1 stride-2 projection
def test_batchnorm_fold_matches_unfolded_fp64(B, cin, cout, k, stride, H, W, relu):
    """extractor.conv_norm_act (the folded path) against conv -> BatchNorm(running statistics) in fp64, per output channel.
    A channel's error is measured against its own scale |g| * max|conv| + |g * (b - mean)| + |beta| (g = gamma /
    sqrt(var + eps)): the size of the terms its fp32 evaluation adds, whatever the channel's mean cancels."""
    from dkt_stereo_amd import extractor
    seed = cin * 100 + cout + k + stride
    torch.manual_seed(seed)
    conv_l = nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2).to(DEV)
    bn = _trained_bn(cout, seed).to(DEV)
    x = torch.rand(B, cin, H, W, generator=torch.Generator().manual_seed(seed + 1)).to(DEV) * 2 - 1
    y = extractor.conv_norm_act(conv_l, bn, x, relu)
    w, b = conv_l.weight.double(), conv_l.bias.double()
    c64 = F.conv2d(x.double(), w, b, stride=stride, padding=k // 2)
    ref = F.batch_norm(c64, bn.running_mean.double(), bn.running_var.double(), bn.weight.double(), bn.bias.double(),
                       False, 0.0, EPS)
    ref = ref.relu() if relu else ref
    g = bn.weight.double() / (bn.running_var.double() + EPS).sqrt()
    scale = (g.abs() * (c64 - b.view(1, -1, 1, 1)).abs().amax((0, 2, 3)) + (g * (b - bn.running_mean.double())).abs()
             + bn.bias.double().abs())
    err = (y.double() - ref).abs().amax((0, 2, 3))
    rel = err / scale
    print("folded BN: max per-channel error %.3e of the channel's scale (gamma 1e-4 channels: %.3e)" % (
        float(rel.max()), float(rel[::5].max())))
    assert float(rel.max()) <= 4e-6, int(rel.argmax())
