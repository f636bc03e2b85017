"""The arithmetic conv2d_f16s_kernel is DEFINED to do at one, two and three passes, in fp64, and its epilogues.

Written from the definitions -- the head comment of csrc/conv2d.hip (w*s = w_hi + w_lo, x = x_hi + x_lo; three passes
w_hi*x_hi + w_lo*x_hi + w_hi*x_lo, two passes drop w_hi*x_lo, one pass keeps w_hi*x_hi), the range paragraph of conv.py's
docstring -- never by calling the packer or a kernel (those are under test).  ONE product function is used: conv.pack_scale,
the power of two that puts max|w| into [2^12, 2^13); tests/test_host_conv2d_ref.py pins that window at both edges.

    passes 3    the exact convolution of the fp32 operands (what the split approximates to ~22 bits per operand)
    passes 2    activations rounded to fp16 at the layer's range exponent (the x_hi plane), weights exact (w_hi + w_lo)
    passes 1    activations rounded alike, weights rounded to the fp16 image of w * pack_scale(max|w|) (the w_hi plane)

The products of fp16 operands are exact in fp32, so against these references only the fp32 accumulation remains: the
split-fp16 bound 3e-6 of max(1, max|y|) (BOUND) holds at every pass count, where the exact convolution sits 2e-4 away from
the reduced ones.  Everything here is torch and runs on the CPU and on the GPU.

fp16 subnormals: round_act keeps them (conv.py states an absolute resolution below 2^-3, not a flush).  Whether the matrix
cores flush a subnormal x_hi is below what the bound resolves: such a value is < 2^-14 / in_scale, times a weight of at
most max|w| < 0.2, i.e. < 1.3e-5 per product, and of the tests' inputs (randn * 1.5 + 0.3) some 30 in a million are
that small: an estimated < 1e-6 of max|y| where they meet, under the bound either way."""
import torch
import torch.nn.functional as F

from dkt_stereo_amd.conv import pack_scale

#: the project's split-fp16 bound (tests/test_gpu_round5.py, test_gpu_random.py::test_conv_random), relative to max(1, max|y|)
BOUND = 3e-6
#: what a reduced-pass result must at least differ from the exact convolution by, relative to max|exact| (the `off` check of
#: test_conv_c8_reduced_passes_are_the_rounded_operand_convolution)
OFF = 1e-5
#: the bound of the gate epilogues (tests/test_gpu_conv2d_epilogue_bodies.py: hardware exp / rcp in the epilogue)
GATE_BOUND = 1e-5


# ---- operands -------------------------------------------------------------------------------------------------------------
def round_scaled(x, scale, inv_scale):
    """fp32: x_hi of `x` staged at `scale` (a power of two; float or 0-d tensor), back at x's scale.  Subnormals kept."""
    return (x.float() * scale).half().float() * inv_scale


def round_act(x, in_exp=0):
    """The x_hi plane of an activation at range exponent `in_exp` (layer.dkt_in_exp), back at x's scale."""
    return round_scaled(x, 2.0 ** in_exp, 2.0 ** -in_exp)


def w_hi(w):
    """What the packed image's hi plane holds: fp16 of w * s, s = pack_scale(max|w|) (max |w * s| in [2^12, 2^13)), back at
    w's scale."""
    s = pack_scale(float(w.detach().abs().max()))
    return (w.detach().float() * s).half().float() * (1.0 / s)


def w_split(w):
    """(hi, lo) of the packer's split, both back at w's scale: hi = fp16(w s), lo = fp16(w s - hi)."""
    s = pack_scale(float(w.detach().abs().max()))
    ws = w.detach().float() * s
    hi = ws.half()
    lo = (ws - hi.float()).half()
    return hi.float() * (1.0 / s), lo.float() * (1.0 / s)


def norm_operand(x, params):
    """The fp32 tensor an in-norm launch convolves: relu((x - mean) * invstd) as two separately rounded fp32 operations
    (conv2d.hip's staging: __fsub_rn, __fmul_rn -- the arithmetic of instnorm_apply_kernel).  params: (B*C, 2) (mean, 1/std)."""
    B, C = x.shape[:2]
    p = params.view(B, C, 2)
    mean, inv = p[:, :, 0].reshape(B, C, 1, 1), p[:, :, 1].reshape(B, C, 1, 1)
    return ((x.float() - mean) * inv).clamp_min(0)


def dscale_act(scale):
    """The activation rounding of the device-scaled form for the pair conv.conv_grad_prepass returned: g * scale[0] is what
    the kernel splits, scale[1] un-scales the result."""
    s0, s1 = (float(v) for v in scale.detach().cpu())
    return lambda g: round_scaled(g, s0, s1)


# ---- the convolution ------------------------------------------------------------------------------------------------------
def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def conv_ref(xs, layer, passes, relu=False, bias=True, in_exp=None, act=None, drop=None):
    """fp64 [relu](conv(cat(xs)) + bias) of the operands a `passes`-pass launch multiplies, at the layer's stride and padding.
    xs: a tensor or the list of cat operands; in_exp: the range exponent (default layer.dkt_in_exp or 0); act: the
    activation rounding when it is not round_act (dscale_act); drop = (tap, chunk): that filter tap's weights of input
    channels [16 chunk, 16 chunk + 16) removed (what a kernel that skips one step computes)."""
    xs = list(xs) if isinstance(xs, (list, tuple)) else [xs]
    if in_exp is None:
        in_exp = int(getattr(layer, "dkt_in_exp", 0) or 0)
    if passes not in (1, 2, 3):
        raise ValueError("passes %r" % (passes,))
    if passes < 3:
        xs = [act(x) if act is not None else round_act(x, in_exp) for x in xs]
    w = layer.weight.detach()
    w = (w_hi(w) if passes == 1 else w.float()).double()
    if drop is not None:
        tap, chunk = drop
        kw = w.shape[3]
        w = w.clone()
        w[:, 16 * chunk:16 * chunk + 16, tap // kw, tap % kw] = 0
    b = layer.bias.detach().double() if bias and layer.bias is not None else None
    y = F.conv2d(torch.cat([x.double() for x in xs], 1), w, b, stride=_pair(getattr(layer, "stride", 1)),
                 padding=_pair(layer.padding))
    return y.clamp_min(0) if relu else y


# ---- epilogues (v: the fp64 convolution + bias) -----------------------------------------------------------------------------
def residual_ref(v, res, relu=False):
    """ConvArgs.epi 3: relu(res + [relu](v))."""
    return (res.double() + (v.clamp_min(0) if relu else v)).clamp_min(0)


def gate_zr_ref(v, cz, cr, h):
    """ConvArgs.epi 1 on the merged z|r convolution: (z, r*h) = (sigmoid(v[:Ch] + cz), sigmoid(v[Ch:] + cr) * h)."""
    ch = v.shape[1] // 2
    return torch.sigmoid(v[:, :ch] + cz.double()), torch.sigmoid(v[:, ch:] + cr.double()) * h.double()


def gate_out_ref(v, cq, z, h):
    """ConvArgs.epi 2: (1 - z) * h + z * tanh(v + cq)."""
    z = z.double()
    return (1 - z) * h.double() + z * torch.tanh(v + cq.double())


def stats_ref(y, eps):
    """(mean, 1/sqrt(var + eps)) per (batch, channel) plane of y, fp64, flattened as instance_norm_params lays them out."""
    y = y.double()
    mean, var = y.mean((2, 3)).reshape(-1), y.var((2, 3), unbiased=False).reshape(-1)
    return mean, (var + eps).rsqrt(), var


def stats_tolerance(mean, var, hw):
    """Relative bound on 1/std from fp32 sums of hw values in an order the tiling decides (test_gpu_conv2d_epilogues.py)."""
    return 2.0 * hw * 2.0 ** -24 * (1.0 + float((mean * mean / var).max()))


# ---- comparisons ----------------------------------------------------------------------------------------------------------
def distance(a, b):
    """max|a - b| relative to max|b|."""
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max())


def ratio(got, ref, bound=BOUND, floor=1.0):
    """max|got - ref| over bound * max(floor, max|ref|): <= 1 passes."""
    return float((got.double() - ref).abs().max()) / (bound * max(floor, float(ref.abs().max())))
