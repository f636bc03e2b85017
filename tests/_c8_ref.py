"""A plain restatement of the C8S activation format and fp64 references of the operators that consume and produce it.

Written from the layout comment in include/dktstereo.h, not by calling conv_c8.pack / unpack (those are under test):

    C8S tensor of C channels at H x W:  [B][G = 2*ceil(C/16)][2: hi, lo][Hp][Wp][8] fp16,
    Hp = roundup(H, 8) + 2, Wp = roundup(W, 32) + 2; pixel (y, x) lives at (y+1, x+1); border and padding channels are
    zero; value = (hi + lo) / scale, hi = fp16(x * scale), lo = fp16(x * scale - hi), `scale` a power of two.

Everything here is torch and runs on the CPU and on the GPU.  The scale constants come from loop_c8."""
import math

import torch
import torch.nn.functional as F

from dkt_stereo_amd import conv_c8 as c8
from dkt_stereo_amd.loop_c8 import RANGE_HI, RANGE_LO, SCALE_EXP


# ---- the format ---------------------------------------------------------------------------------------------------------
def dims_ref(H, W):
    return (H + 7) // 8 * 8 + 2, (W + 31) // 32 * 32 + 2


def to_channels(t):
    """C8S storage (B, G, 2, Hp, Wp, 8) -> (B, 8 G, 2, Hp, Wp): channel-major copy, [:, c, 0] = hi, [:, c, 1] = lo."""
    B, G, _, Hp, Wp, _ = t.shape
    return t.permute(0, 1, 5, 2, 3, 4).reshape(B, 8 * G, 2, Hp, Wp)


def from_channels(ch):
    B, C8, _, Hp, Wp = ch.shape
    return ch.reshape(B, C8 // 8, 8, 2, Hp, Wp).permute(0, 1, 3, 4, 5, 2).contiguous()


def scale_vector(a, dtype=torch.float64):
    """The scale of every channel of `a`, from a.channel_scales()."""
    return torch.cat([torch.full((n,), sc, dtype=dtype) for n, sc in a.channel_scales()]).to(a.t.device)


def split_ref(xs):
    """fp32 values (already scaled) -> (hi, lo) fp16."""
    xs = xs.float()
    hi = xs.half()
    return hi, (xs - hi.float()).half()


def pack_ref(x, scale, tail=0, tail_scale=None, C_pad=None, ch0=0):
    """fp32 NCHW -> an ActC8 of C_pad (default ch0 + C) channels holding x in channels [ch0, ch0 + C), everything else zero.
    The last `tail` channels of the DESTINATION carry `tail_scale`."""
    B, C, H, W = x.shape
    Cd = ch0 + C if C_pad is None else C_pad
    assert ch0 % 8 == 0 and ch0 + C <= Cd
    a = c8.ActC8(B, Cd, H, W, x.device, scale=scale, tail=tail)
    if tail and tail_scale is not None:
        a.tail_scale = float(tail_scale)
    Hp, Wp = dims_ref(H, W)
    G = 2 * ((Cd + 15) // 16)
    assert tuple(a.t.shape) == (B, G, 2, Hp, Wp, 8)
    s = scale_vector(a, torch.float32)[ch0:ch0 + C].view(1, C, 1, 1)
    hi, lo = split_ref(x.float() * s)                  # (a power of two: the product is exact in fp32)
    ch = torch.zeros((B, 8 * G, 2, Hp, Wp), device=x.device, dtype=torch.float16)
    ch[:, ch0:ch0 + C, 0, 1:H + 1, 1:W + 1] = hi
    ch[:, ch0:ch0 + C, 1, 1:H + 1, 1:W + 1] = lo
    a.t = from_channels(ch)
    return a


def unpack_ref(a, C=None, ch0=0):
    """fp64 NCHW: (hi + lo) / s per channel, s from a.channel_scales()."""
    C = a.C - ch0 if C is None else C
    ch = to_channels(a.t)[:, ch0:ch0 + C, :, 1:a.H + 1, 1:a.W + 1].double()
    return (ch[:, :, 0] + ch[:, :, 1]) / scale_vector(a)[ch0:ch0 + C].view(1, C, 1, 1)


def outside_interior(a, ch0=0, C=None):
    """A copy of a.t with the interior of channels [ch0, ch0 + C) zeroed: what a producer must leave alone."""
    C = a.C - ch0 if C is None else C
    ch = to_channels(a.t).clone()
    ch[:, ch0:ch0 + C, :, 1:a.H + 1, 1:a.W + 1] = 0
    return ch


def calibrated_scale(x):
    """The scale C8Loop._rescale's `pick` chooses from scale 1: max |x * scale| lands in [2^SCALE_EXP, 2^(SCALE_EXP + 1))."""
    v = float(x.detach().abs().max())
    return 2.0 ** (SCALE_EXP - math.floor(math.log2(v)))


#: the window edges a calibrated tensor may drift to before the loop recalibrates: scaled maxima stay inside
#: [2^RANGE_LO, 2^RANGE_HI) for shifts of -4 and +3 from the calibrated position [2^SCALE_EXP, 2^(SCALE_EXP + 1))
EDGE_SHIFTS = (RANGE_LO - SCALE_EXP, RANGE_HI - 1 - SCALE_EXP)
assert EDGE_SHIFTS == (-4, 3)

#: operand configurations of the scaled-operand tests: name -> ((magnitude, shift of the calibrated scale in bits), ...),
#: one entry per operand of a launch.  Operands of one launch get different magnitudes and scales.
M_LO, M_HI = 2.0 ** -10, 2.0 ** 10
OPERAND_CONFIGS = {
    "lo_hi": ((M_LO, 0), (M_HI, 0)),
    "one_hi_lo": ((1.0, 0), (M_HI, 0), (M_LO, 0)),
    "edge_low": ((1.0, EDGE_SHIFTS[0]), (M_LO, EDGE_SHIFTS[0]), (M_HI, 0)),
    "edge_high": ((M_HI, EDGE_SHIFTS[1]), (1.0, EDGE_SHIFTS[1]), (M_LO, 0)),
    "edge_mixed": ((M_LO, EDGE_SHIFTS[1]), (M_HI, EDGE_SHIFTS[0]), (1.0, 0)),
}


def operand(shape, mag, shift, kind="randn", device="cpu", gen=None):
    """(x fp32, scale): magnitude `mag` times randn ("relu": post-ReLU, "tanh": a hidden state), the calibrated scale times
    2^shift."""
    x = torch.randn(shape, generator=gen, device=device)
    x = x.clamp_min(0) if kind == "relu" else torch.tanh(x) if kind == "tanh" else x
    x = (x * mag).float()
    return x, calibrated_scale(x) * 2.0 ** shift


def balance_weights(w, chans, mags):
    """Input channels of operand i divided by its magnitude: every operand contributes alike to the output, so a defect in
    any one operand's scale shows relative to the output maximum."""
    w = w.clone()
    c0 = 0
    for c, m in zip(chans, mags):
        w[:, c0:c0 + c] /= m
        c0 += c
    return w


# ---- fp64 references ----------------------------------------------------------------------------------------------------
def conv_ref64(xs, weight, bias=None, relu=False, residual=None, padding=1):
    """conv(cat(xs)) + bias [ReLU]; with `residual`: relu(residual + [relu](conv + bias)) (core/extractor.py:52-60)."""
    y = F.conv2d(torch.cat([x.double() for x in xs], 1), weight.double(), None if bias is None else bias.double(), padding=padding)
    y = y.clamp_min(0) if relu else y
    return y if residual is None else (residual.double() + y).clamp_min(0)


def gate_zr_ref64(gru, h, xs, cz, cr):
    """core/update.py:27-29: (z, r * h)."""
    p = {k: v.double() for k, v in gru.state_dict().items()}
    hx = torch.cat([h.double()] + [t.double() for t in xs], 1)
    z = torch.sigmoid(F.conv2d(hx, p["convz.weight"], p["convz.bias"], padding=1) + cz.double())
    r = torch.sigmoid(F.conv2d(hx, p["convr.weight"], p["convr.bias"], padding=1) + cr.double())
    return z, r * h.double()


def gate_out_ref64(gru, rh, xs, cq, z, h):
    """core/update.py:30-31."""
    p = {k: v.double() for k, v in gru.state_dict().items()}
    q = torch.tanh(F.conv2d(torch.cat([rh.double()] + [t.double() for t in xs], 1), p["convq.weight"], p["convq.bias"], padding=1)
                   + cq.double())
    return (1 - z.double()) * h.double() + z.double() * q


def gru_ref64(gru, h, xs, cz, cr, cq):
    """core/update.py:23-32 in fp64."""
    p = {k: v.double() for k, v in gru.state_dict().items()}
    h, cz, cr, cq = h.double(), cz.double(), cr.double(), cq.double()
    x = torch.cat([t.double() for t in xs], 1)
    hx = torch.cat([h, x], 1)
    z = torch.sigmoid(F.conv2d(hx, p["convz.weight"], p["convz.bias"], padding=1) + cz)
    r = torch.sigmoid(F.conv2d(hx, p["convr.weight"], p["convr.bias"], padding=1) + cr)
    q = torch.tanh(F.conv2d(torch.cat([r * h, x], 1), p["convq.weight"], p["convq.bias"], padding=1) + cq)
    return (1 - z) * h + z * q


def flow_head_ref64(conv1, conv2, xs):
    """core/update.py:6-14: conv2(relu(conv1(cat(xs))))."""
    hid = conv_ref64(xs, conv1.weight, conv1.bias, relu=True)
    return F.conv2d(hid, conv2.weight.double(), None if conv2.bias is None else conv2.bias.double(), padding=1)


def pool_ref(x):
    return F.avg_pool2d(x, 3, stride=2, padding=1)


def interp_ref(x, size):
    return F.interpolate(x, size, mode="bilinear", align_corners=True)


# ---- the format's own error --------------------------------------------------------------------------------------------
def emulate_split_conv(config, balanced=True, n=1152, outputs=48, pixels=48, seed=0, scales=None):
    """The arithmetic the C8S kernels implement, on the CPU with fp64 accumulation: one segment of `n` products per operand
    of `config` ((magnitude, shift), ...), activations scaled and split into fp16 (hi, lo), weights with 1 / scale folded
    per input channel, scaled to max |w| in [2^12, 2^13) and split alike, products hi*hi + lo*hi + hi*lo.  Returns the
    error against the exact product relative to the output maximum.  `scales`: override the operands' scales."""
    g = torch.Generator().manual_seed(seed)
    xs, ss = [], []
    for i, (mag, shift) in enumerate(config):
        x, s = operand((n, pixels), mag, shift, gen=g)
        xs.append(x)
        ss.append(s if scales is None else scales[i])
    w = torch.randn((outputs, n * len(config)), generator=g) / math.sqrt(n * len(config))
    if balanced:
        w = balance_weights(w, [n] * len(config), [m for m, _ in config])
    want = w.double() @ torch.cat(xs, 0).double()
    inv = torch.cat([torch.full((n,), 1.0 / s) for s in ss])
    wf = w * inv.view(1, -1)
    e = 12 - math.floor(math.log2(float(wf.abs().max())))
    w_hi, w_lo = split_ref(wf * 2.0 ** e)
    halves = [split_ref(x * s) for x, s in zip(xs, ss)]
    x_hi = torch.cat([h for h, _ in halves], 0).double()
    x_lo = torch.cat([l for _, l in halves], 0).double()
    acc = w_hi.double() @ x_hi + w_lo.double() @ x_hi + w_hi.double() @ x_lo
    got = acc * 2.0 ** -e
    return float((got - want).abs().max() / want.abs().max())
