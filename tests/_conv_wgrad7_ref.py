"""Reference for the weight gradient of the 7x7 stem layers (csrc/conv_wgrad7.hip, dkt_conv2d_wgrad7, conv.GRAD_WEIGHT7_HIP):
the fp64 truth, both bounds and the CPU emulation of the kernel's arithmetic are those of _conv_wgrad_ref.py (they take the
kernel size), with n = B*H*W pixels per weight.  This module adds the cases, their inputs, the slice rule restated for this
entry, and the faults a test has to catch.

Fixed cases (B, H, W, Cin, Cout) -- the smallest shapes at which each mechanism can go wrong:
  (2, 9, 35, 3, 64)    odd W: the 4-byte path; a column tile that ends at 3 of 32; H barely above 7
  (1, 5, 70, 2, 64)    H < 7: taps whose rows are all outside the image; three column tiles; Cin = 2 (convf1)
  (3, 7, 9, 1, 64)     Cin = 1 (IGEV's convd1); B = 3: three slices
  (2, 24, 40, 3, 64)   several bands per batch element
  (2, 8, 12, 4, 70)    Cin = 4; a second output-channel block 6 wide
  (1, 12, 33, 3, 130)  three output-channel blocks
  (1, 1, 1, 3, 5)      only the centre tap is non-zero: every other weight must be stored as an exact 0
  (2, 16, 64, 3, 64)   aligned: the 16-byte path
A case such as 1x3x4 4 -> 70 is too small: with a handful of terms per weight the fp16 lo part is subnormal and the
emulation itself exceeds bound (b) (ratio 5.0) -- the limit _conv_wgrad_ref.drawn_cases describes.
"""
import functools
import math

import torch

import _conv_wgrad_ref as WR

K = 7
#: (B, H, W, Cin, Cout)
CASES = [
    (2, 9, 35, 3, 64),
    (1, 5, 70, 2, 64),
    (3, 7, 9, 1, 64),
    (2, 24, 40, 3, 64),
    (2, 8, 12, 4, 70),
    (1, 12, 33, 3, 130),
    (1, 1, 1, 3, 5),
    (2, 16, 64, 3, 64),
]
CENTRE_ONLY = CASES[6]
#: the plan's other regimes: bound (a) sees a lost tile or slice there (n is 10^4 .. 10^5, beyond what (b) resolves)
PLAN_CASES = [
    (3, 700, 64, 3, 64),         # T = 512, 8-row bands, 88 bands, 264 items: more than 256, eight blocks take a second item
    (1, 2, 8200, 3, 64),         # one slice, 257 column tiles in one item
    (7, 24, 40, 3, 64),          # 14 slices of a small image: the finishing kernel's sum over slices
]
WALKED, LONG_ROW, MANY_SLICES = PLAN_CASES
KS = WR.KS
A_BOUND = WR.A_BOUND
MAX_CIN = 4


def case_id(case):
    return "x".join(str(v) for v in case)


CASE_IDS = [case_id(c) for c in CASES]
PLAN_IDS = [case_id(c) for c in PLAN_CASES]


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(x, g', gy, y, weight, bias) of a case, fp32 on the CPU: generator 7000 + i, drawn in the order x, gy, y, then the
    weight and the bias; g' = gy * (y > 0)."""
    B, H, W, cin, cout = case
    i = (CASES + PLAN_CASES).index(case)
    g = torch.Generator().manual_seed(7000 + i)
    x = torch.randn(B, cin, H, W, generator=g)
    gy = torch.randn(B, cout, H, W, generator=g)
    y = torch.randn(B, cout, H, W, generator=g)
    w = torch.randn(cout, cin, K, K, generator=g) / math.sqrt(cin * K * K)
    b = 0.1 * torch.randn(cout, generator=g)
    return x, gy * (y > 0), gy, y, w, b


def plan_T(case):
    """(T, rows per band, bands, output-channel blocks, 1): wgrad_plan on the H x W grid, restated by
    _conv_wgrad_ref.grid_plan_T (Cin <= 4 is one input-channel block).  An item is (slice, 64 output channels)."""
    B, H, W, cin, cout = case
    return WR.grid_plan_T(B, H, W, cin, cout)


def regime(case):
    """dict of T, band, bands, slices (per weight), items, tiles_w, tiles (pixel tiles per item, band by band)."""
    B, H, W, cin, cout = case
    T, band, bands, n_co, n_ci = plan_T(case)
    assert n_ci == 1
    tiles_w = -(-W // 32)
    tiles = [-(-(min(H, (i + 1) * band) - i * band) // WR.TILE_ROWS) * tiles_w for i in range(bands)]
    return dict(T=T, band=band, bands=bands, slices=B * bands, items=B * bands * n_co, tiles_w=tiles_w, tiles=tiles)


def ws_floats(case):
    """Floats of ws[slice][Cout][Cin][7][7]."""
    B, H, W, cin, cout = case
    return regime(case)["slices"] * cout * cin * K * K


def truth(x, gp):
    return WR.truth(x, gp, K)


def b_bound(x, gp):
    return WR.b_bound(x, gp, K)


def emulate(x, gp, e=None, x_scale=1.0):
    return WR.emulate(x, gp, K, e, x_scale)


def torch_fp32(x, gp):
    return WR._cw(x, gp, K)


# ------------------------------------------------------------------------------------------------------------- faults
def zeroed_tap(gw):
    """Tap (ky, kx) = (0, 6) never accumulated."""
    out = gw.clone()
    out[:, :, 0, 6] = 0.0
    return out


def without_last_column(x):
    """The last pixel column of x never staged."""
    out = x.clone()
    out[:, :, :, -1] = 0.0
    return out


def without_tile(case, gp):
    """g' without one 2 x 32 pixel tile: the first of the last band of the last batch element."""
    reg = regime(case)
    r0 = (reg["bands"] - 1) * reg["band"]
    out = gp.clone()
    out[-1, :, r0:r0 + 2, 0:32] = 0.0
    return out


def without_last_slice(case, gp):
    """g' without the last slice (the last band of the last batch element)."""
    reg = regime(case)
    out = gp.clone()
    out[-1, :, (reg["bands"] - 1) * reg["band"]:] = 0.0
    return out
