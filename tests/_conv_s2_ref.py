"""Reference for the backward of the stride-2 convolutions (csrc/conv_dgrad_s2.hip, csrc/conv_wgrad_s2.hip: dkt_conv2d_dgrad_s2,
dkt_conv2d_wgrad_s2): fp64 truth from the SAME fp32 inputs the node sees (torch.nn.grad.conv2d_input / conv2d_weight at stride
2 on .double() inputs), a CPU emulation of each kernel's arithmetic written the way the kernel is -- the input gradient by
output parity, the weight gradient tap by tap over slices added in ascending order --, the band rule of the weight
gradient's plan restated, the cases and the bounds.  The bounds are those of _conv_grad_ref / _conv_wgrad_ref, nothing new:

  gx   max|got - exact| <= GX_BOUND (5e-6) * max|exact|
  gw   (a) the same 5e-6;  (b) |got - exact| <= (3 * 2^-22 + gamma_n) * sum|g'||x| elementwise, n = B*Ho*Wo.

Every case of CASES keeps n <= 1105, so (b) stays discriminating (gamma_1105 = 6.6e-5 against a dropped term's 1 / sqrt(n) = 3e-2).
The emulations take mutants (a dropped parity, a dropped tap, a lost last odd row or column, a lost slice): what
test_host_conv_s2_ref.py shows the bounds to catch.
"""
import functools
import math

import torch
import torch.nn.functional as F

import _conv_grad_ref as R
import _conv_wgrad_ref as WR

#: (B, H, W, k, Cin, Cout); H, W the INPUT size
CASES = [
    (1, 1, 1, 1, 1, 1),          # smallest shape
    (1, 1, 1, 3, 1, 1),          # smallest 3x3
    (1, 2, 3, 3, 3, 2),          # tiny mixed parity
    (2, 24, 40, 3, 64, 96),      # layer2's class, even sizes
    (1, 33, 37, 3, 36, 40),      # odd H and W: the last row and column are even-parity only; 4-byte path
    (1, 18, 70, 3, 8, 40),       # Wo = 35: more than one 32-column tile
    (1, 34, 130, 3, 5, 70),      # Wo = 65: three tiles; Cout tail
    (1, 33, 37, 1, 96, 128),     # a projection: three quarters of gx is zero
    (3, 7, 9, 1, 130, 3),        # B = 3, three input-channel blocks
    (1, 16, 24, 3, 128, 128),    # layer4's class
]
CASE_IDS = ["x".join(str(v) for v in c) for c in CASES]
#: in the three smallest cases tap (0, 0) sees only padding: mutants are evaluated on the other seven
NONDEGENERATE = CASES[3:]
KS = R.KS
LAYOUTS = R.LAYOUTS
GX_BOUND = R.GX_BOUND
A_BOUND = WR.A_BOUND
U = R.U
#: the weight-gradient kernels' tiling (csrc/conv_wgrad_common.h): channels per block, output rows of a pixel tile
BLOCK, TILE_ROWS = WR.BLOCK, WR.TILE_ROWS


def out_size(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


@functools.lru_cache(maxsize=None)
def inputs(case):
    """x, weight, bias, the O(1) upstream gradient and a random saved output (the ReLU mask) of a case: fp32, CPU, seeded."""
    B, H, W, k, cin, cout = case
    Ho, Wo = out_size(H, W)
    g = torch.Generator().manual_seed(2000 + CASES.index(case))
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    b = 0.1 * torch.randn(cout, generator=g)
    gy = torch.randn(B, cout, Ho, Wo, generator=g)
    y = torch.randn(B, cout, Ho, Wo, generator=g)
    return x, w, b, gy, y


def masked(case, m=0):
    """g' = (y > 0) ? gy * 2^m : 0 of the case -- exact in fp32."""
    _, _, _, gy, y = inputs(case)
    return R.mask(gy * 2.0 ** m, y)


#: (B, H, W, k, Cin, Cout) that take dkt_conv2d_wgrad_s2 (and the finishing kernel) out of "one item per block, T = 512":
#: the regimes of _conv_wgrad_ref.PLAN_CASES on the Ho x Wo grid
PLAN_CASES = [
    (2, 83, 512, 3, 260, 257),   # grid 42 x 256: T = 2048, k = 3, walked (300 items), odd H, channel tails on both sides
    (3, 79, 512, 1, 70, 520),    # grid 40 x 256: T = 2048, k = 1, walked (270 items), odd H
    (3, 291, 48, 3, 257, 257),   # grid 146 x 24: T = 1024, one column tile, bands of 21 and 10 tiles, 300 items
    (2, 127, 511, 3, 130, 70),   # grid 64 x 256: T = 512, walked (384 items), odd H and W, channel tails
    (1, 12, 16, 3, 384, 320),    # grid 6 x 8, 1 105 920 weights: the finishing kernel strides
]
PLAN_IDS = ["x".join(str(v) for v in c) for c in PLAN_CASES]
WALKED = PLAN_CASES[:4]
MIXED = PLAN_CASES[2]


def plan_inputs(case):
    """_conv_wgrad_ref.drawn_inputs at stride 2: x, weight, bias, upstream gradient, saved output."""
    return WR.drawn_inputs(case, 2)


def plan_masked(case):
    """g' of a plan or drawn case: the upstream gradient behind the random mask."""
    _, _, _, gy, y = plan_inputs(case)
    return R.mask(gy, y)


def regime_of(case):
    """_conv_wgrad_ref.regime of dkt_conv2d_wgrad_s2 for the case (grid Ho x Wo)."""
    B, H, W, k, cin, cout = case
    return WR.regime(B, *out_size(H, W), cin, cout)


def plan(case):
    """(output rows per band, bands, output-channel blocks, input-channel blocks) of dkt_conv2d_wgrad_s2: the rule of
    dkt_conv2d_wgrad (_conv_wgrad_ref.grid_plan) on the Ho x Wo grid.  Slices of one weight: B * bands."""
    B, H, W, k, cin, cout = case
    return WR.grid_plan(B, *out_size(H, W), cin, cout)


def bands_of(case):
    """[(first output row, one past the last)] of the plan's bands."""
    rows, bands, _, _ = plan(case)
    Ho = out_size(case[1], case[2])[0]
    return [(i * rows, min(Ho, (i + 1) * rows)) for i in range(bands)]


# ---------------------------------------------------------------------------------------------------------------- truth
def truth_gx(gp, w, hw):
    B, cin = gp.shape[0], w.shape[1]
    return torch.nn.grad.conv2d_input((B, cin, hw[0], hw[1]), w.double(), gp.double(), stride=2, padding=w.shape[2] // 2)


def _cw(x, gp, k):
    return torch.nn.grad.conv2d_weight(x, (gp.shape[1], x.shape[1], k, k), gp, stride=2, padding=k // 2)


def truth_gw(x, gp, k):
    return _cw(x.double(), gp.double(), k)


def torch32_gx(gp, w, hw):
    B, cin = gp.shape[0], w.shape[1]
    return torch.nn.grad.conv2d_input((B, cin, hw[0], hw[1]), w, gp, stride=2, padding=w.shape[2] // 2)


def torch32_gw(x, gp, k):
    return _cw(x, gp, k)


gx_error = R.gx_error
a_error = WR.a_error
b_ratio = WR.b_ratio


def b_bound(x, gp, k):
    return WR.b_factor(gp.shape[0] * gp.shape[2] * gp.shape[3]) * _cw(x.double().abs(), gp.double().abs(), k)


# ------------------------------------------------------------------------------------------------------------ emulation
_split32 = WR._split32


def _taps(k, parity):
    """[(filter index, shift on the g' grid)] of one axis: with x = 2 o + kk - p, an even x takes kk = 1 from o = i; an odd
    one kk = 0 from o = i + 1 and kk = 2 from o = i (k = 3).  k = 1: an even x takes kk = 0 from o = i, an odd one nothing."""
    if k == 1:
        return [(0, 0)] if parity == 0 else []
    return [(1, 0)] if parity == 0 else [(0, 1), (2, 0)]


def emulate_gx(gp, w, hw, e=None, drop_parity=None, drop_tap=None, lose_odd=None):
    """dkt_conv2d_dgrad_s2 on the CPU: g' * 2^e (e: the pre-pass exponent of max|g'| unless given; 0 = unit scale) and
    w * 2^ew as fp16 hi + lo carried in fp32 (every product exact), w_hi*g_hi + w_lo*g_hi + w_hi*g_lo accumulated in fp32,
    un-scaled; parity by parity on the Ho x Wo grid.  Mutants: drop_parity = (py, px) is never computed (stays 0),
    drop_tap = (ky, kx) is left out, lose_odd = "row" / "col": the LAST odd output row / column is never stored (reads 0)."""
    H, W = hw
    B, cout, Ho, Wo = gp.shape
    cin, k = w.shape[1], w.shape[2]
    e = R.exponent(float(gp.abs().max())) if e is None else e
    ew = R.exponent(float(w.abs().max()))
    ghi, glo = _split32(gp, 2.0 ** e)
    whi, wlo = _split32(w, 2.0 ** ew)
    ghi, glo = F.pad(ghi, (0, 1, 0, 1)), F.pad(glo, (0, 1, 0, 1))
    gx = torch.zeros(B, cin, H, W)
    for py in (0, 1):
        for px in (0, 1):
            ny, nx = (H - py + 1) // 2, (W - px + 1) // 2
            if ny <= 0 or nx <= 0 or (py, px) == drop_parity:
                continue
            acc = torch.zeros(B, cin, ny, nx)
            for ky, sy in _taps(k, py):
                for kx, sx in _taps(k, px):
                    if (ky, kx) == drop_tap:
                        continue
                    parts = []
                    for gpart, wpart in ((ghi, whi), (ghi, wlo), (glo, whi)):
                        gs = gpart[:, :, sy:sy + ny, sx:sx + nx]
                        parts.append(torch.einsum("bcij,cd->bdij", gs, wpart[:, :, ky, kx]))
                    acc = acc + parts[0] + parts[1] + parts[2]
            gx[:, :, py::2, px::2] = acc
    if lose_odd == "row" and H > 1:
        gx[:, :, (H - 2) | 1] = 0                   # the largest odd index below H
    if lose_odd == "col" and W > 1:
        gx[:, :, :, (W - 2) | 1] = 0
    return gx * (2.0 ** -e * 2.0 ** -ew)


def emulate_gw(case, x, gp, e=None, x_scale=1.0, drop_tap=None, drop_slice=None, lose_odd=None):
    """dkt_conv2d_wgrad_s2 on the CPU: g' * 2^e and x * x_scale as fp16 hi + lo carried in fp32, g_hi*x_hi + g_lo*x_hi +
    g_hi*x_lo in fp32, one partial per slice (batch element, band of the plan), the slices added in ascending order, then
    un-scaled.  Mutants: drop_tap = (ky, kx) stays 0, drop_slice = index of a slice that is not added, lose_odd = "row" /
    "col": the last odd row / column of x reads as zero."""
    B, H, W, k, cin, cout = case
    Ho, Wo = out_size(H, W)
    p = k // 2
    e = R.exponent(float(gp.abs().max())) if e is None else e
    ghi, glo = _split32(gp, 2.0 ** e)
    x = x.clone()
    if lose_odd == "row" and H > 1:
        x[:, :, (H - 2) | 1] = 0                    # the largest odd index below H
    if lose_odd == "col" and W > 1:
        x[:, :, :, (W - 2) | 1] = 0
    xhi, xlo = _split32(x, x_scale)
    # padded so that row 2 oy + ky - p is index 2 oy + ky, for every oy < Ho
    xhi, xlo = (F.pad(t, (p, 2 * Wo + k - W, p, 2 * Ho + k - H)) for t in (xhi, xlo))
    gw = torch.zeros(cout, cin, k, k)
    s = 0
    for b in range(B):
        for r0, r1 in bands_of(case):
            if s != drop_slice:
                part = torch.zeros(cout, cin, k, k)
                for ky in range(k):
                    for kx in range(k):
                        if (ky, kx) == drop_tap:
                            continue
                        sl = lambda t: t[b, :, 2 * r0 + ky:2 * r1 + ky:2, kx:2 * Wo + kx:2]
                        part[:, :, ky, kx] = (torch.einsum("oij,cij->oc", ghi[b, :, r0:r1], sl(xhi))
                                              + torch.einsum("oij,cij->oc", glo[b, :, r0:r1], sl(xhi))
                                              + torch.einsum("oij,cij->oc", ghi[b, :, r0:r1], sl(xlo)))
                gw = gw + part
            s += 1
    return gw * (2.0 ** -e / x_scale)
