"""TEST INFRASTRUCTURE -- the on-the-fly correlation lookup (csrc/corr_otf.hip, corr.PytorchAlternateCorrBlock1D, the
reference's core/corr.py:64-107) in float64, its error bound, a model of the kernel's per-block path decision, and the fixed
cases of test_host_otf_ref.py / test_gpu_otf.py.

Truth (alt64).  A node is held to the function its forward computes, so the sample positions and the one-axis weights are
the reference's own fp32 numbers, taken as exact inputs: ix = ix32(x / 2^lv + k) per level and iy = ix32(y) with H
(_train_ref.ix32: grid_sample's normalise / unnormalise round trip), w = RN(ix - floor ix), e = RN(1 - w).  (w is inexact
only for floor ix = -1, where e multiplies the padding; ATen's (floor ix + 1) - ix equals e wherever e multiplies a
value.)  Near integral coordinates the round trip lands on row / column -1 with weight 0.99999994, and a real-arithmetic
truth would be ill-conditioned exactly there.  Everything else is float64: the W-pooling of fmap2 (avg_pool2d([1, 2]),
floor width), the channel contraction, the four-tap blend with zero padding (padded VALUES are zero, weights are not
masked: a non-finite weight makes the output NaN, as it does in the reference's arithmetic), the division by the fp32
sqrt(C) taken as exact.  `mag` is the same expression on |f1|, the pooled |f2| and |weights|.

Bound.  |got - truth| <= 2 c u mag + 2^-126 over every element, u = 2^-24, with the roundings a term of the sum can pass
through, counted on corr_otf.hip:

    lv        the fp32 roundings of the pooling chain, one per level (each relative to the pooled |f2|)
    n(C)      the FMA chain of the longest of the eight channel ranges.  A wave owns cq = ceil(C/4) channels and walks
              them in groups of 32, of which half-wave 0 takes the first 16 and half-wave 1 the rest, so the longest chain
              is n(C) = 16 floor(cq/32) + min(16, cq mod 32): 12 at C 48 (not ceil(C/8) = 6: the second half-wave is
              idle), 16 at C 72, 17 at C 132, 32 at C 256.  The general path splits a wave's range evenly,
              ceil(cq/2) <= n(C), and folds the product with f1 into the same chain.
    3         the xor-32 add and the two adds of the four-wave tree
    1         the product of the two one-axis weights
    4         the blend (one product, three FMAs), before the contraction on the general path, after it on the window path
    1         the division by sqrt(C)

so c = n(C) + lv + 9 on both kernel paths; the factor 2 covers the second-order terms.  The oracles have their own counts:
the C oracle (fp32 blend and product, double accumulation, one cast) c = lv + 9, torch's fp32 corr1d_lookup_alt (ATen's
weights from two differences, a seven-operation blend, a channel sum of unspecified order, hence C - 1 adds at the most)
c = C + lv + 8.

NaN rule.  Where the truth and the C oracle are both NaN (non-finite coordinates, H = 1, a level of width 1) the kernel
must be NaN; nowhere else may it be non-finite.  On every fixed case the two NaN patterns are the same (host test).

Paths (block_paths) is a MODEL OF THE CODE UNDER TEST: it conditions inputs (does this case reach that path?) and never
supplies an expected value.

Measured on an MI355X (test_gpu_otf.py -s), the kernel's worst error in u * mag (fraction of the bound) per path over the
fixed cases: window_one_row 2.28 (0.104, chan_1), window_two_rows 0.75 (0.009, half_row), window_empty exact zeros,
general_rows 2.68 (0.122, chan_gather_1), general_wide 1.21 (0.029, span_65), general_irregular 1.36 (0.049).  Per case:
chan_1 2.28 (0.104), chan_3 2.07 (0.103), chan_17 1.73 (0.062), chan_72 0.97 (0.019), chan_132 0.61 (0.012), chan_256 0.61
(0.007), chan_gather_1 2.68 (0.122), _17 1.35 (0.048), _72 0.91 (0.018), _132 0.77 (0.015), half_row 0.75 (0.009),
row_outside 1.41 (0.050), round_trip_rows 0.81 (0.010), empty_left 0.78 (0.010), empty_right 0.33 (0.007), span_64 1.17
(0.028), span_65 1.21 (0.029), clipped_edges 1.21 (0.024), ragged_33 2.00 (0.072), ragged_31 1.49 (0.053), irregular 1.72
(0.061), degenerate_h1 all NaN, degenerate_w1 1.23 (0.044), radius_0 0.84 (0.016), radius_1 0.73 (0.015), radius_8 1.16
(0.022).  The oracles on the CPU (test_host_otf_ref.py -s): C at most 2.73, torch at most 3.35 u * mag.
"""
import functools

import numpy as np
import torch

import _cases
import _synth
from _train_ref import ix32, taps32

U = 2.0 ** -24
FLOOR = 2.0 ** -126
SEG = 32                    # pixels per block (OTF_PX)
WIN = 64                    # staged columns (OTF_WIN)
LABELS = ("window_one_row", "window_two_rows", "window_empty", "general_irregular", "general_rows", "general_wide")
WINDOW = ("window_one_row", "window_two_rows", "window_empty")
#: wrong kernels the bound must tell from the right one: row y0 + 1 dropped; the last channel of wave 0's quarter dropped; the
#: window start off by one column; e and w swapped on x; pooled levels of ceil width; the division by sqrt(C) applied twice
MUTANTS = ("drop_row1", "drop_channel", "window_shift", "swap_ew", "ceil_pool", "div_twice")


def T(a):
    return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))


# ---- the bound ----------------------------------------------------------------------------------------------------------
def chain(C):
    """n(C) of the module docstring: the longest FMA chain of the kernel's eight channel ranges."""
    cq = (C + 3) // 4
    return 16 * (cq // 32) + min(16, cq % 32)


def c_kernel(C, lv):
    return chain(C) + lv + 9


def c_c_oracle(C, lv):
    return lv + 9


def c_torch(C, lv):
    return C + lv + 8


def cmag_of(mag, c_of, C, L, r):
    """c(lv) * mag per element of a (B, L*K, H, W1) magnitude."""
    K = 2 * r + 1
    c = torch.tensor([float(c_of(C, lv)) for lv in range(L) for _ in range(K)], dtype=torch.float64)
    return mag * c.view(1, -1, 1, 1)


def worst(got, truth, cmag, mag):
    """(largest error in units of u * mag, largest fraction of the bound 2 c u mag + 2^-126) over EVERY element where the
    truth is a number; inf if `got` is not finite there."""
    got = T(got).detach().double().cpu()
    assert got.shape == truth.shape == cmag.shape == mag.shape
    ok = ~torch.isnan(truth)
    d = (got - truth).abs()[ok]
    if d.numel() == 0:
        return 0.0, 0.0
    if not bool(torch.isfinite(d).all()):
        return float("inf"), float("inf")
    m, cm = mag[ok], cmag[ok]
    of_bound = d / (2.0 * U * cm + FLOOR)
    over = torch.clamp(d - FLOOR, min=0.0)
    in_u = torch.where(over > 0, over / (U * torch.where(m > 0, m, torch.ones_like(m))), torch.zeros_like(d))
    in_u = torch.where((over > 0) & (m == 0), torch.full_like(d, float("inf")), in_u)
    return float(in_u.max()), float(of_bound.max())


def nan_rule(got, truth, c_or):
    """The NaN rule of the module docstring as (ok, message)."""
    got = T(got).detach().cpu()
    must = torch.isnan(truth) & torch.isnan(T(c_or))
    if not bool(torch.isnan(got[must]).all()):
        return False, "%d elements are numbers where the truth and the C oracle are NaN" % int((~torch.isnan(got[must])).sum())
    if not bool(torch.isfinite(got[~must]).all()):
        return False, "%d elements are not finite where the reference is" % int((~torch.isfinite(got[~must])).sum())
    return True, ""


# ---- the truth ----------------------------------------------------------------------------------------------------------
def _axis(x, n, positions):
    """(floor, weight of the floor tap, weight of the next tap) of coordinates x (fp32) in a row of n, weights float64."""
    if positions == "fp32":
        ix = ix32(x, n)
        fl = torch.floor(ix)
        w = ix - fl                                     # fp32, as the reference forms it
        e = 1.0 - w
        return fl.double(), e.double(), w.double()
    x = x.double()                                      # the whole round trip in float64 (checks the restatement only)
    ix = ((2.0 * x) / (n - 1) - 1.0 + 1.0) * ((n - 1) / 2.0)
    fl = torch.floor(ix)
    w = ix - fl
    return fl, 1.0 - w, w


def _pool(p, ceil=False):
    w = p.shape[-1]
    out = (p[..., 0:w - w % 2:2] + p[..., 1:w:2]) * 0.5
    if ceil and w % 2:
        out = torch.cat([out, p[..., -1:]], -1)         # avg_pool2d(ceil_mode=True): the clipped window's own mean
    return out


def _blend(a1, p, fy, ey, wy, fx, ex, wx):
    """sum_c a1[c] * (four-tap sample of p[c]) -> (B, H, W1, K), padded values zero, weights unmasked."""
    B, C, H, W1 = a1.shape
    wi = p.shape[3]
    vol = torch.einsum('bchw,bcyv->bhwyv', a1, p).reshape(B, H, W1, H * wi)
    out = 0.0
    for dy, wyy in ((0, ey), (1, wy)):
        yi = (fy + dy)[..., None]
        for dx, wxx in ((0, ex), (1, wx)):
            xi = fx + dx
            ok = (yi >= 0) & (yi <= H - 1) & (xi >= 0) & (xi <= wi - 1)
            idx = torch.where(ok, yi * wi + xi, torch.zeros_like(xi)).long()
            val = torch.where(ok, torch.gather(vol, 3, idx), torch.zeros_like(xi))
            out = out + val * (wyy[..., None] * wxx)
    return out


def alt64(f1, f2, coords, L, r, mutant=None, positions="fp32"):
    """(truth, mag), float64 (B, L*K, H, W1), of the module docstring.  `mutant`: one of MUTANTS, a wrong kernel's function.
    positions="fp64" runs the coordinate round trip in float64 too: torch_oracle.corr1d_lookup_alt on float64 tensors."""
    assert mutant is None or mutant in MUTANTS
    f1, f2, coords = T(f1), T(f2), T(coords)
    B, C, H, W1 = f1.shape
    sqrt_c = float(torch.sqrt(torch.tensor(C).float()))
    a1 = f1.double()
    if mutant == "drop_channel":                        # the last channel of wave 0's quarter
        a1 = a1.clone()
        a1[:, (C + 3) // 4 - 1] = 0.0
    cx, cy = coords[:, 0], coords[:, 1]
    if positions == "fp64":
        cx = cx.double()                                # x / 2^lv + k is formed in float64 as well
    fy, ey, wy = _axis(cy, H, positions)
    if mutant == "drop_row1":
        wy = torch.zeros_like(wy)
    p, pa = f2.double(), f2.double().abs()
    outs, mags = [], []
    for lv in range(L):
        x = cx[..., None] / 2 ** lv + taps32(r).view(1, 1, 1, -1)
        fx, ex, wx = _axis(x, p.shape[3], positions)
        if mutant == "swap_ew":
            ex, wx = wx, ex
        if mutant == "window_shift":
            fx = fx + 1.0
        outs.append(_blend(a1, p, fy, ey, wy, fx, ex, wx))
        mags.append(_blend(a1.abs(), pa, fy, ey.abs(), wy.abs(), fx, ex.abs(), wx.abs()))
        p, pa = _pool(p, mutant == "ceil_pool"), _pool(pa, mutant == "ceil_pool")
    div = sqrt_c * sqrt_c if mutant == "div_twice" else sqrt_c
    out = torch.cat(outs, -1).permute(0, 3, 1, 2).contiguous() / div
    mag = torch.cat(mags, -1).permute(0, 3, 1, 2).contiguous() / sqrt_c
    return out, mag


# ---- the kernel's per-block decision ------------------------------------------------------------------------------------
def _clamp_nan(fl, lo, hi):
    """fminf(fmaxf(fl, lo), hi) as the device evaluates it: NaN -> lo."""
    return torch.clamp(torch.nan_to_num(fl, nan=float(lo), posinf=float(hi), neginf=float(lo)), float(lo), float(hi)).long()


def block_paths(coords, H, W1, W2, L, r):
    """An fp32 MODEL OF THE CODE UNDER TEST: the decision corr1d_otf_kernel takes per block -- (batch item, row, 32-pixel
    segment, level) -- between its staged-window and its general path, restated from corr_otf.hip.  It serves only as a
    condition on inputs (which paths does a case reach?), never as a source of expected values; a change to the kernel's
    dispatch must be mirrored here.  Returns arrays (B, H, nseg, L):
      label    one of LABELS.  window_two_rows: both rows y0 and y0 + 1 carry weight for some pixel of the block;
               window_empty: no tap of any pixel is inside the row (ncol 0); the general labels name the first reason in
               the kernel's order (an irregular lane, differing rows, a span of more than 64 columns)
      ncol     columns of the row the block's regular pixels touch (the staged width on the window path)
      outside  a live pixel has one of its 2r + 2 window columns outside the row
      far      a live pixel's whole window is clamped (beyond -(K+2) or W+1)
      live     live lanes of the block"""
    co = T(coords).float()
    B = co.shape[0]
    assert tuple(co.shape) == (B, 2, H, W1)
    K = 2 * r + 1
    nseg = (W1 + SEG - 1) // SEG
    pad = nseg * SEG - W1
    co = torch.cat([co, co[..., -1:].expand(B, 2, H, pad)], -1) if pad else co     # dead lanes replicate the last pixel
    cx, cy = co[:, 0], co[:, 1]
    iy = ix32(cy, H)
    fy = torch.floor(iy)
    wy = iy - fy
    ey = 1.0 - wy
    y0 = _clamp_nan(fy, -2, H + 1).view(B, H, nseg, SEG)
    need = ((ey != 0).view(B, H, nseg, SEG).any(-1).long() | 2 * (wy != 0).view(B, H, nseg, SEG).any(-1).long())
    rows = y0.min(-1).values != y0.max(-1).values
    live = (torch.arange(nseg * SEG) < W1).view(1, 1, nseg, SEG)
    label = np.empty((B, H, nseg, L), dtype=object)
    ncol = np.zeros((B, H, nseg, L), np.int64)
    outside = np.zeros((B, H, nseg, L), bool)
    far_any = np.zeros((B, H, nseg, L), bool)
    big = 0x7fffffff
    for lv in range(L):
        wi = W2 >> lv
        x = cx[..., None] / 2 ** lv + taps32(r).view(1, 1, 1, -1)
        fl = torch.floor(ix32(x, wi))
        fl0 = fl[..., 0]
        far = (fl0 < -(K + 2)) | (fl0 > wi + 1)
        i0 = _clamp_nan(fl0, -(K + 2), wi + 1)
        consec = (fl == fl0[..., None] + torch.arange(K, dtype=torch.float32)).all(-1)
        regular = (fl0 == fl0) & (far | consec)
        c_lo = torch.clamp(i0, min=0)
        c_hi = torch.where(i0 + K >= wi, torch.full_like(i0, wi - 1), i0 + K)
        touch = regular & (c_lo <= c_hi)
        seg = lambda t: t.view(B, H, nseg, SEG)
        lo = torch.where(seg(touch), seg(c_lo), torch.full_like(seg(c_lo), big)).min(-1).values
        hi = torch.where(seg(touch), seg(c_hi), torch.full_like(seg(c_hi), -1)).max(-1).values
        n = torch.where(hi >= lo, hi - lo + 1, torch.zeros_like(hi))
        irregular = (~seg(regular)).any(-1)
        lab = np.where(n.numpy() == 0, "window_empty", np.where(need.numpy() == 3, "window_two_rows", "window_one_row"))
        lab = np.where(n.numpy() > WIN, "general_wide", lab)
        lab = np.where(rows.numpy(), "general_rows", lab)
        lab = np.where(irregular.numpy(), "general_irregular", lab)
        label[..., lv] = lab
        ncol[..., lv] = n.numpy()
        outside[..., lv] = (seg((i0 < 0) | (i0 + K > wi - 1)) & live).any(-1).numpy()
        far_any[..., lv] = (seg(far) & live).any(-1).numpy()
    return dict(label=label, ncol=ncol, outside=outside, far=far_any,
                live=np.broadcast_to(live.sum(-1).numpy()[..., None], label.shape))


# ---- the fixed cases ----------------------------------------------------------------------------------------------------
def _base(B, H, W1):
    c = np.zeros((B, 2, H, W1), np.float32)
    c[:, 0] = np.arange(W1, dtype=np.float32)[None, None, :]
    c[:, 1] = np.arange(H, dtype=np.float32)[None, :, None]
    return c


def _left(seed, spread, dy=0.0):
    def make(c):
        co = _base(c["B"], c["H"], c["W1"])
        co[:, 0] -= _synth.uniform((c["B"], c["H"], c["W1"]), 0.0, spread, seed, "otf_x")
        co[:, 1] += np.float32(dy)
        return co
    return make


def _gather(seed):
    def make(c):
        co = _left(seed, 6.0)(c)
        co[:, 1] += _synth.uniform((c["B"], c["H"], c["W1"]), -0.7, 0.7, seed, "otf_dy")
        return co
    return make


def _shift(dx):
    def make(c):
        co = _base(c["B"], c["H"], c["W1"])
        co[:, 0] += np.float32(dx)
        return co
    return make


def _row_outside(c):
    co = _left(711, 6.0)(c)
    co[0, 1] -= 1.0
    co[1, 1] = c["H"] + 3.0
    return co


def _span(num):
    def make(c):
        co = _base(c["B"], c["H"], c["W1"])
        co[:, 0] = (20.25 + np.arange(c["W1"], dtype=np.float64) * num / 31.0).astype(np.float32)[None, None, :]
        return co
    return make


def _clipped(c):
    co = _base(c["B"], c["H"], c["W1"])
    d = _synth.uniform((c["B"], c["H"], c["W1"]), 0.0, 12.0, 713, "otf_x")
    co[0, 0] -= d[0]
    co[1, 0] += d[1]
    return co


def _irregular(c):
    co = _left(717, 6.0)(c)
    x = co[0, 0]
    W = c["W1"]
    x[0, 3] = np.nan                                    # row 0, segment 0: an irregular lane
    x[0, 33], x[0, 35], x[0, 37] = -1000.0, 3.0 * W + 0.25, 2.0 ** 24 + 1.0     # row 0, segment 1: far lanes only
    x[1, 0:32:7] = np.round(x[1, 0:32:7])               # row 1, segment 0: exact integers
    x[1, 34], x[1, 36] = np.inf, -np.inf                # row 1, segment 1: far and not finite
    return co


def _case(C, make, must=(), only=None, B=1, H=2, W1=40, W2=None, L=2, r=4, seed=700, **kw):
    return dict(B=B, C=C, H=H, W1=W1, W2=W1 if W2 is None else W2, L=L, r=r, seed=seed, make=make, must=tuple(must),
                only=only, **kw)


_WINDOW_FULL = ("window_one_row", "window_two_rows")
CASES = {}
for _c in (1, 3, 17, 72, 132, 256):
    CASES["chan_%d" % _c] = _case(_c, _left(701, 6.0), only=_WINDOW_FULL, seed=720 + _c)
for _c in (1, 17, 72, 132):
    CASES["chan_gather_%d" % _c] = _case(_c, _gather(702), only=("general_rows",), seed=740 + _c)
CASES.update({
    "half_row": _case(256, _left(703, 6.0, 0.5), only=("window_two_rows",), H=6, seed=703),
    "row_outside": _case(17, _row_outside, only=WINDOW, B=2, H=3, seed=704, zeros=True),
    "round_trip_rows": _case(256, lambda c: _synth.coords(705, c["B"], c["H"], c["W1"], spread=8.0),
                             must=("window_two_rows",), H=6, W1=150, L=3, seed=705),
    "empty_left": _case(256, _shift(-48.25), must=("window_empty",), W1=96, L=4, seed=706, zeros=True,
                        empty={0: 2, 1: 2}),
    "empty_right": _case(48, _shift(85.5), must=("window_empty",), W1=72, L=3, seed=707, zeros=True,
                         empty={0: "all", 1: "all"}),
    "span_64": _case(48, _span(54.0), only=("window_one_row",), W1=32, W2=160, L=1, seed=708, ncol=64),
    "span_65": _case(48, _span(55.0), only=("general_wide",), W1=32, W2=160, L=1, seed=709, ncol=65),
    "clipped_edges": _case(72, _clipped, only=WINDOW, W1=72, B=2, seed=710, outside=True),
    "ragged_33": _case(17, _left(711, 6.0), only=WINDOW, W1=33, W2=57, L=3, seed=711, raw=True, one_live=True),
    "ragged_31": _case(17, _left(712, 6.0), only=WINDOW, W1=31, W2=57, L=3, seed=712, raw=True),
    "irregular": _case(17, _irregular, must=("general_irregular", "window_one_row"), seed=717, far=True, nans=True),
    "degenerate_h1": _case(17, _left(718, 6.0), H=1, seed=718, nans=True),
    "degenerate_w1": _case(17, _left(719, 6.0), W2=8, L=4, seed=719, nans=True, torch=False),
})
for _r in (0, 1, 8):
    CASES["radius_%d" % _r] = _case(72, _shift(-3.5), only=WINDOW, B=2, H=3, W1=72, L=6, r=_r, seed=730 + _r,
                                    all_levels=_WINDOW_FULL)
del _c, _r


def case_inputs(name):
    """(f1, f2, coords) numpy fp32 of a fixed case."""
    c = CASES[name]
    f1, f2 = _synth.fmap_pair(c["seed"], c["B"], c["C"], c["H"], c["W1"], c["W2"])
    return f1, f2, c["make"](c)


def case_paths(name):
    c = CASES[name]
    return block_paths(case_inputs(name)[2], c["H"], c["W1"], c["W2"], c["L"], c["r"])


@functools.lru_cache(maxsize=None)
def case_truth(name):
    """(truth, mag, cmag of the kernel) of a fixed case, computed once and shared; callers must not modify them."""
    c = CASES[name]
    f1, f2, co = case_inputs(name)
    truth, mag = alt64(f1, f2, co, c["L"], c["r"])
    return truth, mag, cmag_of(mag, c_kernel, c["C"], c["L"], c["r"])


def existing_inputs():
    """{name: (coords, H, W1, W2, L, r)} of every input the suite ran through the kernel before these cases: CORR_CASES
    (test_corr_alt_and_cosine) and the four modes of test_otf_lookup_paths."""
    out = {}
    for name, c in _cases.CORR_CASES.items():
        out["corr/" + name] = (_cases.corr_inputs(c)[2], c["H"], c["W"], c["W2"], c["L"], c["r"])
    B, H, W = 2, 6, 150
    co = _synth.coords(401, B, H, W, spread=8.0)
    out["otf/rows"] = (co, H, W, W, 3, 4)
    v = co.copy()
    v[:, 1] += 1.0
    out["otf/vertical_shift"] = (v, H, W, W, 3, 4)
    f = co.copy()
    f[:, 1] += _synth.uniform((B, H, W), -0.7, 0.7, 402, "dy")
    out["otf/fractional_y"] = (f, H, W, W, 3, 4)
    out["otf/wide_windows"] = (_synth.coords(403, B, H, W, spread=140.0), H, W, W, 3, 4)
    return out
