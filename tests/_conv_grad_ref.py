"""Reference for the backward of conv.conv2d_autograd (csrc/conv_grad.hip, dkt_conv_desc.dscale): fp64 truth for the masked
gradient g', the bias gradient gb and the input gradient gx from the SAME fp32 inputs the node sees (the upstream gradient,
the saved ReLU output, the weight), a CPU emulation of the split-fp16 convolution (hi / lo fp16 of x * s, three products,
summed in fp64), the exponent rule of the pre-pass, the fixed cases and the bounds.

Bounds
  gx   max|got - exact| / max|exact| <= 5e-6: what test_conv2d_autograd_matches_torch holds this gradient to at O(1)
       upstream gradients, here at every magnitude.
  gb   |got - exact| <= gamma_{n-1} * sum|g'|, gamma_m = m*u / (1 - m*u), u = 2^-24, n = B*H*W: the classical bound of a
       recursive fp32 sum of n terms in ANY order (Higham, Accuracy and Stability, 4.2).  The cases keep n <= 2304, so
       a dropped term (about sum|g'| / n) exceeds it (gamma_{2303} = 1.4e-4 < 1 / 2304 = 4.3e-4).
  g'   exact.   scale pair: exact.
"""
import functools
import math

import torch
import torch.nn.functional as F

#: (B, H, W, k, Cin, Cout)
CASES = [
    (1, 1, 1, 1, 1, 1),          # smallest shape
    (2, 24, 40, 3, 48, 40),      # mid-size 3x3 layer
    (1, 33, 37, 1, 36, 64),      # odd sizes: the 4-byte path
    (1, 20, 28, 3, 64, 2),       # the flow head: a 2-channel gradient
    (1, 16, 24, 3, 384, 256),    # z|r
]
CASE_IDS = ["x".join(str(v) for v in c) for c in CASES]
#: upstream gradient = randn * 2^k
KS = [0, -20, -40, 20]
LAYOUTS = ["strided", "misaligned"]
GX_BOUND = 5e-6
U = 2.0 ** -24
#: DKT_CONV_GRAD_MAX_EXP of include/dktstereo.h
MAX_EXP = 80


def exponent(amax):
    """e with amax * 2^e in [2^12, 2^13), clamped to +-MAX_EXP; 0 for amax == 0, Inf, NaN."""
    amax = float(amax)
    if not (amax > 0.0) or not math.isfinite(amax):
        return 0
    m, x = math.frexp(amax)                   # amax = m * 2^x, m in [0.5, 1): floor(log2(amax)) = x - 1
    return max(-MAX_EXP, min(MAX_EXP, 12 - (x - 1)))


def scale_pair(amax):
    e = exponent(amax)
    return torch.tensor([2.0 ** e, 2.0 ** -e], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """x, weight, bias and the O(1) upstream gradient of a case (fp32, CPU, seeded by the case)."""
    B, H, W, k, cin, cout = case
    g = torch.Generator().manual_seed(1000 + CASES.index(case))
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    b = 0.1 * torch.randn(cout, generator=g)
    gy = torch.randn(B, cout, H, W, generator=g)
    return x, w, b, gy


def laid_out(t, layout, device=None):
    """A copy of t (B, C, H, W) in the named memory layout on `device`: "strided" = a channel slice of a wider buffer (batch
    stride (C + 3)*H*W, every batch element dense), "misaligned" = contiguous, one float past a 16-byte boundary."""
    B, C, H, W = t.shape
    device = t.device if device is None else device
    if layout == "strided":
        buf = torch.zeros(B, C + 3, H, W, device=device, dtype=t.dtype)
        v = buf[:, 2:2 + C]
    elif layout == "misaligned":
        buf = torch.zeros(t.numel() + 1, device=device, dtype=t.dtype)
        v = buf[1:].view(B, C, H, W)
        assert v.data_ptr() % 16 == 4
    else:
        raise ValueError(layout)
    v.copy_(t)
    return v


def mask(gy, y):
    """g' = (y > 0) ? gy : 0 -- exact in fp32."""
    return gy if y is None else torch.where(y > 0, gy, torch.zeros_like(gy))


def transposed(w):
    """The weight of the input gradient: transposed over (Cout, Cin), rotated by 180 degrees."""
    return w.transpose(0, 1).flip(2, 3).contiguous()


def truth(gy, y, w):
    """(g', gb, gx) of [relu](conv2d(x, w) + b) for the upstream gradient gy and the saved output y (None: no ReLU):
    g' in fp32 (exact), gb and gx in fp64."""
    gp = mask(gy, y)
    gb = gp.double().sum(dim=(0, 2, 3))
    gx = F.conv2d(gp.double(), transposed(w).double(), padding=w.shape[2] // 2)
    return gp, gb, gx


def gx_error(got, exact):
    """max|got - exact| / max|exact| (the absolute error where the exact result is all zero)."""
    d, den = float((got.double() - exact).abs().max()), float(exact.abs().max())
    return d / den if den > 0.0 else d


def gb_bound(gp):
    """Per channel: gamma_{n-1} * sum|g'| for the fp32 sum of n = B*H*W terms in any order."""
    n = gp.shape[0] * gp.shape[2] * gp.shape[3]
    m = (n - 1) * U
    return gp.double().abs().sum(dim=(0, 2, 3)) * (m / (1.0 - m))


def _split(t, scale):
    s = t * scale                                   # fp32, a power of two: exact
    hi = s.half()
    lo = (s - hi.float()).half()
    return hi.double(), lo.double()


def split_conv(g, w, in_scale):
    """The split-fp16 input-gradient convolution restated on the CPU: operands g * in_scale and w * 2^ew (max|w| * 2^ew in
    [2^12, 2^13)) as fp16 hi + lo, w_hi*g_hi + w_lo*g_hi + w_hi*g_lo summed in fp64, un-scaled.  An operand beyond the fp16
    range makes the result non-finite, as on the device."""
    wt = transposed(w)
    ws = 2.0 ** exponent(float(wt.abs().max()))
    ghi, glo = _split(g, in_scale)
    whi, wlo = _split(wt, ws)
    pad = w.shape[2] // 2
    acc = F.conv2d(ghi, whi, padding=pad) + F.conv2d(ghi, wlo, padding=pad) + F.conv2d(glo, whi, padding=pad)
    return acc / (in_scale * ws)


# ------------------------------------------------------------------------------------ the pre-pass beyond one segment
#: csrc/conv_grad.hip: elements per work item, the widest launch, threads of the finish
PRE_SEG, PRE_BLOCKS, PRE_THREADS = 4096, 2048, 256
#: (B, C, H, W) that take dkt_conv_grad_prepass out of "one segment per plane, one item per block, one channel per thread"
PREPASS_PLAN_CASES = [
    (2, 520, 41, 100),           # HW = 4100: two segments, the last 4 elements long; 2080 items; a finish thread owns 3 channels
    (3, 300, 67, 123),           # HW = 8241 = 2 * 4096 + 49, not a multiple of 4: the 4-byte path only; 2700 items with C < 512
    (3, 2, 128, 96),             # HW = 12288: three whole segments
]
PREPASS_PLAN_IDS = ["x".join(str(v) for v in c) for c in PREPASS_PLAN_CASES]


def prepass_regime(case):
    """dict of nseg (segments per plane), last (elements of the last segment), items, per_thread (channels the busiest
    finish thread owns), vec (HW % 4 == 0: the 16-byte path can run)."""
    B, C, H, W = case
    HW = H * W
    nseg = -(-HW // PRE_SEG)
    return dict(nseg=nseg, last=HW - (nseg - 1) * PRE_SEG, items=B * C * nseg, per_thread=-(-C // PRE_THREADS),
                vec=HW % 4 == 0)


@functools.lru_cache(maxsize=None)
def prepass_inputs(case):
    """(gy, y) of a pre-pass case: fp32, CPU, seeded by the case."""
    B, C, H, W = case
    g = torch.Generator().manual_seed(3000 + PREPASS_PLAN_CASES.index(case))
    return torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)


def item_of(case, b, c, e):
    """Work item that reads element e of plane (b, c): (c * B + b) * nseg + e / 4096."""
    return (c * case[0] + b) * prepass_regime(case)["nseg"] + e // PRE_SEG


def emulate_gb(gp):
    """The bias gradient in the summation order the header of csrc/conv_grad.hip states, in fp32 on the CPU (every torch
    add below is one IEEE fp32 addition per element): thread t of 256 adds its 16 elements (k * 256 + t) * 4 + j of a
    4096-element segment, k then j ascending, from 0.0f (elements past the plane are 0.0f); the 64 lanes of a wave fold by
    xor 32, 16, ..., 1; the waves combine as (w0 + w1) + (w2 + w3); the finish adds a channel's B * nseg items in
    ascending (batch, segment) from 0.0f."""
    B, C, H, W = gp.shape
    HW = H * W
    nseg = -(-HW // PRE_SEG)
    v = F.pad(gp.reshape(B, C, HW).float(), (0, nseg * PRE_SEG - HW)).reshape(B, C, nseg, PRE_SEG // 1024, 256, 4)
    t = torch.zeros(B, C, nseg, 256)
    for k in range(PRE_SEG // 1024):
        for j in range(4):
            t = t + v[:, :, :, k, :, j]
    t = t.reshape(B, C, nseg, 4, 64)
    lanes = torch.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        t = t + t[..., lanes ^ d]
    w = t[..., 0]                                   # (B, C, nseg, 4): every lane holds the wave's sum
    items = (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])
    gb = torch.zeros(C)
    for b in range(B):
        for s in range(nseg):
            gb = gb + items[b, :, s]
    return gb
