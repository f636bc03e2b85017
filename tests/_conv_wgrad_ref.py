"""Reference for the weight gradient of conv.conv2d_autograd (csrc/conv_wgrad.hip, dkt_conv2d_wgrad): fp64 truth from the SAME
fp32 inputs the node sees (the layer input x and the masked gradient g'), the two bounds, a CPU emulation of the kernel's
arithmetic (g' * 2^e with the pre-pass exponent and x * x_scale as fp16 hi + lo, g_hi*x_hi + g_lo*x_hi + g_hi*x_lo, every
product exact in fp32, fp32 accumulation), the slice rule restated, and the fixed cases.

Bounds, both required
  (a)  max|got - exact| <= 5e-6 * max|exact|: GX_BOUND, what the sibling input gradient is held to.
  (b)  |got - exact| <= (3 * 2^-22 + gamma_n) * sum|g'||x| elementwise, n = B*H*W, gamma_n = n*u / (1 - n*u), u = 2^-24.
       3 * 2^-22: each operand keeps 22 bits of its own magnitude in hi + lo (two relative errors of 2^-22) and the dropped
       g_lo*x_lo term is below 2^-22 |g'||x|; gamma_n: an fp32 sum of n terms in ANY order (Higham 4.2).  The cases keep
       n <= 2304, so a dropped tap, pixel or slice (about sum|g'||x| / sqrt(n) or more) exceeds it.
"""
import functools
import math

import torch

import _conv_grad_ref as R

#: (B, H, W, k, Cin, Cout): the five of _conv_grad_ref and
#:   (2, 9, 35, 3, 33, 5)   odd W (the 4-byte path, a column tile that ends at 3 of 32), channel tails on both sides
#:   (1, 5, 70, 3, 8, 40)   a row longer than one pixel tile (three column tiles, the last 6 wide), odd H
#:   (3, 7, 9, 1, 130, 3)   B = 3, 1x1, more than four input-channel fragments (three input-channel blocks)
CASES = list(R.CASES) + [(2, 9, 35, 3, 33, 5), (1, 5, 70, 3, 8, 40), (3, 7, 9, 1, 130, 3)]
CASE_IDS = ["x".join(str(v) for v in c) for c in CASES]
KS = R.KS
LAYOUTS = R.LAYOUTS
A_BOUND = R.GX_BOUND
U = R.U
#: the kernels' tiling (csrc/conv_wgrad_common.h): channels per block on both sides, rows of a pixel tile, the plan's constants
BLOCK, TILE_ROWS, T0, TMIN, ITEMS = 64, 2, 2048, 512, 256


@functools.lru_cache(maxsize=None)
def inputs(case):
    """x, weight, bias and the O(1) upstream gradient of a case (fp32, CPU, seeded by the case)."""
    if case in R.CASES:
        return R.inputs(case)
    B, H, W, k, cin, cout = case
    g = torch.Generator().manual_seed(1000 + CASES.index(case))
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    b = 0.1 * torch.randn(cout, generator=g)
    gy = torch.randn(B, cout, H, W, generator=g)
    return x, w, b, gy


def grid_plan(B, rows, cols, cin, cout):
    """(rows per band, bands, output-channel blocks, input-channel blocks) on a rows x cols reduction grid: the slice rule
    of wgrad_plan restated.  Slices of one weight: B * bands."""
    n_co, n_ci = -(-cout // BLOCK), -(-cin // BLOCK)
    T = T0
    while True:
        band = max(TILE_ROWS, (T // cols) // TILE_ROWS * TILE_ROWS)
        bands = -(-rows // band)
        if n_co * n_ci * B * bands >= ITEMS or T <= TMIN:
            return band, bands, n_co, n_ci
        T //= 2


def plan(case):
    """grid_plan of dkt_conv2d_wgrad for the case: the grid is H x W."""
    B, H, W, k, cin, cout = case
    return grid_plan(B, H, W, cin, cout)


def _cw(x, gp, k):
    return torch.nn.grad.conv2d_weight(x, (gp.shape[1], x.shape[1], k, k), gp, stride=1, padding=k // 2)


def truth(x, gp, k):
    """torch.nn.grad.conv2d_weight in fp64, fed with g'."""
    return _cw(x.double(), gp.double(), k)


def abs_sum(x, gp, k):
    """sum|g'||x| per weight, fp64."""
    return _cw(x.double().abs(), gp.double().abs(), k)


def a_error(got, exact):
    return R.gx_error(got, exact)


def b_factor(n):
    """3 * 2^-22 + gamma_n of bound (b)."""
    return 3.0 * 2.0 ** -22 + n * U / (1.0 - n * U)


def b_bound(x, gp, k):
    return b_factor(x.shape[0] * x.shape[2] * x.shape[3]) * abs_sum(x, gp, k)


def b_ratio(got, exact, bound):
    """(every element inside the bound, max |got - exact| / bound)."""
    d = (got.double() - exact).abs()
    return bool((d <= bound).all()), float((d / bound.clamp_min(1e-300)).max())


def _split32(t, scale):
    s = t * scale                                   # fp32, a power of two: exact
    hi = s.half()
    lo = (s - hi.float()).half()
    return hi.float(), lo.float()


def emulate(x, gp, k, e=None, x_scale=1.0):
    """The kernel's arithmetic on the CPU: e = the pre-pass exponent of max|g'| unless given (0: unit scale).  The fp16
    parts are carried as fp32, so every product is exact and torch's fp32 convolution does the fp32 accumulation."""
    e = R.exponent(float(gp.abs().max())) if e is None else e
    ghi, glo = _split32(gp, 2.0 ** e)
    xhi, xlo = _split32(x, x_scale)
    acc = _cw(xhi, ghi, k) + _cw(xhi, glo, k) + _cw(xlo, ghi, k)
    return acc * (2.0 ** -e / x_scale)
