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
PLAN_CASES (below the fixed cases) leave that n on purpose -- a launch with more items than blocks needs 10^4 .. 10^5 pixels --
and there it is (a) that sees a lost tile, slice or item (test_host_conv_grad_plans.py).
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


def grid_plan_T(B, rows, cols, cin, cout):
    """(T, rows per band, bands, output-channel blocks, input-channel blocks) on a rows x cols reduction grid: the slice rule
    of wgrad_plan restated, with the pixels per slice T it stopped at.  Slices of one weight: B * bands."""
    n_co, n_ci = -(-cout // BLOCK), -(-cin // BLOCK)
    T = T0
    while True:
        band = max(TILE_ROWS, (T // cols) // TILE_ROWS * TILE_ROWS)
        bands = -(-rows // band)
        if n_co * n_ci * B * bands >= ITEMS or T <= TMIN:
            return T, band, bands, n_co, n_ci
        T //= 2


def grid_plan(B, rows, cols, cin, cout):
    """grid_plan_T without the T."""
    return grid_plan_T(B, rows, cols, cin, cout)[1:]


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


# ------------------------------------------------------------------------------------------- the plan's other regimes
#: the CU count of the part the plan's 256 items are named after: a launch has min(items, CUS) blocks
CUS = 256
#: (B, H, W, k, Cin, Cout) that take the kernel out of "one item per block, T = 512": CASES never does (24 items at most)
PLAN_CASES = [
    (2, 42, 256, 3, 260, 257),   # T = 2048, k = 3, walked: 8-row bands (the last 2 rows), 300 items, channel tails on both sides
    (3, 88, 256, 1, 200, 250),   # T = 2048, k = 1, walked: 528 items, the first 16 blocks take three
    (3, 146, 24, 3, 257, 257),   # T = 1024, one column tile: bands 42/42/42/20 rows = 21 and 10 tiles; 300 items, and the blocks
                                 # that take a second item start it at an odd running tile count
    (2, 64, 255, 3, 130, 70),    # T = 512, walked: 384 items, odd W (column tiles that end at 31 of 32), channel tails
    (1, 6, 8, 3, 384, 320),      # 1 105 920 weights: the finishing kernel strides (48 pixels: see drawn_cases on bound (b))
]
PLAN_IDS = ["x".join(str(v) for v in c) for c in PLAN_CASES]
#: the cases whose launch has more items than blocks
WALKED = PLAN_CASES[:4]
#: the T = 1024 case of mixed tile parity
MIXED = PLAN_CASES[2]
FINISH_STRIDE = 4096 * 256       # weights above which conv_wgrad_finish_kernel strides


def regime(B, rows, cols, cin, cout):
    """What a launch on a rows x cols reduction grid looks like, from grid_plan_T: dict of T (pixels per slice the plan stopped
    at), items, tiles (pixel tiles per item, band by band), slices (per weight), tiles_w."""
    T, band, bands, n_co, n_ci = grid_plan_T(B, rows, cols, cin, cout)
    tiles_w = -(-cols // 32)
    tiles = [-(-(min(rows, (i + 1) * band) - i * band) // TILE_ROWS) * tiles_w for i in range(bands)]
    return dict(T=T, band=band, items=n_co * n_ci * B * bands, tiles=tiles, slices=B * bands, tiles_w=tiles_w,
                blocks=n_co * n_ci)


def regime_of(case):
    """regime of dkt_conv2d_wgrad for the case (grid H x W)."""
    B, H, W, k, cin, cout = case
    return regime(B, H, W, cin, cout)


def odd_start(reg, blocks=CUS):
    """Items a block of a `blocks`-wide launch starts with an odd running tile count (the stride-1 kernel's buffer parity)."""
    out = []
    for first in range(min(blocks, reg["items"])):
        tc = 0
        for item in range(first, reg["items"], blocks):
            if tc & 1:
                out.append(item)
            tc += reg["tiles"][(item // reg["blocks"]) % len(reg["tiles"])]
    return out


def _seed_of(case, stride):
    s = stride
    for v in case:
        s = (s * 1000003 + v) % (2 ** 31 - 1)
    return s


@functools.lru_cache(maxsize=2)
def drawn_inputs(case, stride=1):
    """x, weight, bias, the O(1) upstream gradient and a random saved output (a ReLU mask) of ANY case, seeded by the case
    and the stride: what the plan cases and the drawn cases of both strides use.  (Two cases are kept: the plan cases are
    tens of megabytes each.)"""
    B, H, W, k, cin, cout = case
    Ho, Wo = (H, W) if stride == 1 else ((H - 1) // 2 + 1, (W - 1) // 2 + 1)
    g = torch.Generator().manual_seed(_seed_of(case, stride))
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    b = 0.1 * torch.randn(cout, generator=g)
    gy = torch.randn(B, cout, Ho, Wo, generator=g)
    y = torch.randn(B, cout, Ho, Wo, generator=g)
    return x, w, b, gy, y


def drawn_cases(stride, n=40, seed=20241):
    """n seeded small shapes (B, H, W, k, Cin, Cout): B 1..3, H 1..40, W 1..80, Cin and Cout 1..140, k in {1, 3}; a plain
    numpy generator, so the host file proves the references on exactly the cases the device runs.
    The seed is the first from 20240 on at which the references themselves meet bound (b) on all 2 x 40 (20240 has two
    stride-2 shapes of 6 and 8 grid pixels that do not): x * x_scale below 2^-3 has an fp16 lo part that is subnormal, so
    that operand keeps an ABSOLUTE 2^-25 and not 22 bits of its own magnitude, and a weight whose few terms all have a
    small x exceeds 3 * 2^-22 sum|g'||x| in the emulation as on the device.  test_host_conv_grad_plans.py holds the
    references to the bounds on every drawn case, so another seed is checked there before it reaches a device."""
    import numpy as np
    rng = np.random.default_rng(seed + stride)
    out = []
    for _ in range(n):
        B, H, W = int(rng.integers(1, 4)), int(rng.integers(1, 41)), int(rng.integers(1, 81))
        cin, cout = int(rng.integers(1, 141)), int(rng.integers(1, 141))
        out.append((B, H, W, (1, 3)[int(rng.integers(0, 2))], cin, cout))
    return out


def dropped(x, gp, k, stride, b, rows, cols=None, co=None, ci=None):
    """The fp32 contribution to gw of g'[b, co block, rows[0]:rows[1], cols[0]:cols[1]] on the input channels of block ci
    (None: all of an axis): what a kernel that loses that part of its work leaves out.  A mutant is reference - dropped."""
    g1 = torch.zeros_like(gp[b:b + 1])
    cs = slice(None) if cols is None else slice(*cols)
    os_ = slice(None) if co is None else slice(co * BLOCK, (co + 1) * BLOCK)
    g1[:, os_, rows[0]:rows[1], cs] = gp[b:b + 1, os_, rows[0]:rows[1], cs]
    d = torch.nn.grad.conv2d_weight(x[b:b + 1], (gp.shape[1], x.shape[1], k, k), g1, stride=stride, padding=k // 2)
    if ci is not None:
        keep = torch.zeros_like(d)
        keep[:, ci * BLOCK:(ci + 1) * BLOCK] = d[:, ci * BLOCK:(ci + 1) * BLOCK]
        d = keep
    return d


def mutants(x, gp, k, stride, reg, rows_total):
    """{name: dropped contribution} of the three losses a walked plan can hide: one 2 x 32 pixel tile of g' in the last band
    of the last batch element, one whole slice (the second), every item with index >= 256."""
    B = gp.shape[0]
    band, bands, nb = reg["band"], len(reg["tiles"]), reg["blocks"]
    n_ci = -(-x.shape[1] // BLOCK)
    r0 = (bands - 1) * band
    out = {"a tile": dropped(x, gp, k, stride, B - 1, (r0, min(rows_total, r0 + TILE_ROWS)), (0, 32)),
           "a slice": dropped(x, gp, k, stride, 1 // bands, ((1 % bands) * band, min(rows_total, (1 % bands + 1) * band)))}
    late = torch.zeros_like(out["a tile"])
    for item in range(CUS, reg["items"]):
        s, blk = divmod(item, nb)
        b, bi = divmod(s, bands)
        late += dropped(x, gp, k, stride, b, (bi * band, min(rows_total, (bi + 1) * band)), None, blk // n_ci, blk % n_ci)
    out["items from 256 on"] = late
    return out
