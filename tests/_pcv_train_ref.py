"""Float64 truth, fp32 yardstick, closed-form gradients, error bounds, fixed cases and mutants for PCVNet's correlation block
under autograd (pcv_bwd.hip, pcvnet_corr.py; test infrastructure in the layout of _topk_ref.py).

Operator (meta_arch/pcvnet/corr.py:18-61).  fmap1 (B,C,H,W1), fmap2 (B,C,H,W2); coords, sigma (B,G,H,W1); S odd, f in {2,4}.
    vol[n,v] = sum_c fmap1[b,c,h,w] fmap2[b,c,h,v] / sqrt(C)  (the fp32 square root, as the reference divides),  n = (b H + h) W1 + w;   level 0 = vol,
    level i+1 [n,k] = mean of level i [n, f k .. f k + f - 1],  W_{i+1} = W_i // f;
    x = dx_s sigma + coords, dx_s = s - S//2;  ix = x / f^lv;  fl = floor(ix), w = ix - fl, e = 1 - w;
    out[b, lv G S + g S + s, h, w] = v1m w + v0m e,  v0m = level[n, fl], v1m = level[n, fl+1], 0 outside [0, W_lv - 1].
Gradients (closed form), g the upstream gradient of an output element:
    glevel[n, fl] += g e,  glevel[n, fl+1] += g w  (taps inside the row);
    d = g (v1m - v0m) / f^lv;   gcoords[b,g,h,w] = sum_{lv,s} d;   gsigma = sum_{lv,s} dx_s d;
    T_{L-1} = glevel_{L-1};  T_i[c] = glevel_i[c] + (c // f < W_{i+1} ? T_{i+1}[c // f] / f : 0);  gvol = T_0 / sqrt(C);
    gfmap1[b,c,h,w] = sum_v gvol[n,v] fmap2[b,c,h,v];   gfmap2[b,c,h,v] = sum_w gvol[n,v] fmap1[b,c,h,w].

Floors.  d out / d x jumps where ix crosses an integer, so a gradient is only defined once the floor is.  On inputs built like
_cases.pcv_inputs (every seventh coordinate rounded, every fifth sigma 1) the fp32 floor of the kernels' expression and the
float64 floor disagree at a few per cent of the taps (ix is an integer in exact arithmetic and lands on either side).  truth()
therefore takes the floors as an argument: floors32() restates dkt_tap's expression in numpy fp32 (every operation rounded as
the device rounds it; test_host_pcv_train_ref.py shows that lookup32(), built on it, equals c_oracle.pcv_lookup bit for bit),
and the kernels are held to truth(floors=floors32(...)), never to floors read back from the device.  With the floor given, w
and e are continuous in ix: out, glevel move by O(u); d does not depend on ix at all.

Bounds (u = 2^-24; first order in u, the factor 2 in front covers the rest, as in the other _*_ref.py).  Per element, from
magnitudes of the float64 truth.
  ix.  dx sigma rounds once and the sum once: within u (|dx sigma| + |x|) of x, divided by f^lv (exact).  dkt_tap forms
  2 q / (W-1) - 1 + 1 and multiplies by (W-1)/2: the division, the two additions (in units of (W-1)/2 each) and the product,
  each within u of its result; ATen's grid_sample takes as many steps.  With hw = (W_lv - 1) / 2:
      |d ix| <= u A,   A = (|dx sigma| + |x|) / f^lv + 4 |ix| + hw.
  w = ix - fl is exact, e = 1 - w rounds once.
  out.  |v1m| dw + |v0m| (dw + u) + the product and the fma:  bound_out = 2 u (|v0m| + |v1m|) (A + 2) + dv,
      dv = |w| dv1 + |e| dv0 the share of the level values' own error (0 where the levels are the given inputs).
  glevel.  An element receives n products g e or g w, each within |g| (u A + u) + u |g wgt|, and their sum in any order adds
  (n - 1) u sum |g wgt|:   bound_glevel = 2 u (sum |g| (A + 2) + n sum |g wgt|).   Untouched elements admit only 0.
  gcoords, gsigma.  autograd forms v1 g - v0 g (grid_sampler_2d_backward subtracts nw g and adds ne g), scales by (W-1)/2,
  by 2 and by 1 / (W-1), by 1 / f^lv and for sigma by dx: K = 8 roundings of terms bounded by D = |g| (|v0m| + |v1m|) / f^lv
  (the kernel's g (v1m - v0m) / f^lv takes 2, of something smaller).  N = L S summands in any order add (N - 1) u sum D:
      bound_gcoords = 2 u (K + N) sum D + sum |g| (dv0 + dv1) / f^lv,    bound_gsigma the same with |dx| D and K + 1.
  S = 1: dx = 0 and gsigma is exactly 0 (bound 0).
  gvol.  One addition per level and the final division (the divisions by f are exact): with Tabs the chain on |glevel|,
      bound_gvol = 2 u (L + 1) Tabs / sqrt(C) + chain(bound_glevel) / sqrt(C).
  gfmap.  W2 (W1) products and their sum in any order: bound_gf1 = 2 u (W2 + 1) sum_v |gvol| |fmap2| + sum_v bound_gvol |fmap2|.
  level values (only where the block builds them itself): the volume is C products and C - 1 additions in any order and one
  division, dvol = 2 u (C + 2) sum_c |f1| |f2| / sqrt(C); a pooling adds f - 1 additions: dv_{i+1} = mean(dv_i) + 2 u f mean|v_i|.
TINY = 2^-126 is added per unit of |g| for terms below the smallest normal number.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import _cases
import _synth

U = 2.0 ** -24
TINY = 2.0 ** -126
K_ARG = 8.0

#: name -> dict(seed, B, C, H, W, L, S, G, downsample, kind).  kind "planted": inputs of _cases.pcv_inputs (every seventh
#: coordinate an integer, every fifth sigma 1); "smooth": uniformly drawn; "beyond": smooth with taps far beyond both ends
#: of the row planted; "strided": smooth, and the device tests hand coords / sigma over as non-contiguous views.
CASES = {k: dict(v, kind="planted") for k, v in _cases.PCV_CASES.items()}
CASES.update({
    "b2":      dict(seed=601, B=2, C=8, H=9, W=40, L=2, S=3, G=2, downsample=2, kind="smooth"),    # H W = 360 > 256: two blocks
    "g4":      dict(seed=602, B=1, C=8, H=2, W=33, L=2, S=5, G=4, downsample=3, kind="smooth"),    # widths 33, 16
    "s1":      dict(seed=603, B=1, C=4, H=2, W=21, L=2, S=1, G=2, downsample=3, kind="smooth"),    # gsigma exactly 0
    "l1":      dict(seed=604, B=1, C=4, H=2, W=19, L=1, S=9, G=1, downsample=2, kind="smooth"),
    "beyond":  dict(seed=605, B=1, C=8, H=3, W=35, L=3, S=9, G=2, downsample=3, kind="beyond"),    # widths 35, 17, 8
    "planted": dict(seed=606, B=2, C=8, H=2, W=50, L=3, S=9, G=4, downsample=2, kind="planted"),   # widths 50, 12, 3
    "strided": dict(seed=607, B=2, C=8, H=3, W=24, L=2, S=5, G=3, downsample=3, kind="strided"),
})
PLANTED = [n for n, c in CASES.items() if c["kind"] == "planted"]
UNPLANTED = [n for n, c in CASES.items() if c["kind"] != "planted"]
#: the two cases tests/golden/pcv_train.npz holds the reference's own results for
GOLDEN_CASES = ("ds2", "b2")

#: mutant -> (the result whose bound it must miss, the case on which it must)
MUTANTS = {
    "gsigma_drops_level": ("gsigma", "ds2"),
    "no_level_scale": ("gcoords", "ds3"),
    "no_dx": ("gsigma", "odd"),
    "oob_counted": ("gcoords", "beyond"),
    "weights_swapped": ("gf2", "g4"),
    "pool_no_guard": ("gf1", "odd"),
    "no_sqrt_c": ("gf1", "b2"),
}


def factor_of(c):
    return 4 if c["downsample"] == 2 else 2


def widths(c):
    f = factor_of(c)
    return [c["W"] // f ** i for i in range(c["L"])]


def inputs(c):
    """float32 numpy: fmap1, fmap2 (B,C,H,W), coords, sigma (B,G,H,W), gout (B, L G S, H, W)."""
    if c["kind"] == "planted":
        f1, f2, coords, sigma = _cases.pcv_inputs(c)
    else:
        f1, f2 = _synth.fmap_pair(c["seed"], c["B"], c["C"], c["H"], c["W"])
        shp = (c["B"], c["G"], c["H"], c["W"])
        base = np.arange(c["W"], dtype=np.float32).reshape(1, 1, 1, c["W"])
        coords = (base - _synth.uniform(shp, 0.0, 0.6 * c["W"], c["seed"], "pcvc")).astype(np.float32)
        sigma = _synth.uniform(shp, 0.25, 3.0, c["seed"], "pcvs")
        if c["kind"] == "beyond":
            coords[..., 1::5] = -3.0 * c["W"] - 0.375        # every tap of every level left of the row
            coords[..., 3::7] = 2.0 * c["W"] + 0.625         # ... right of it
            coords[..., 2::11] = -0.5                        # fl = -1: only the tap fl + 1 is inside
            coords[..., 4::13] = c["W"] - 0.75               # fl = W - 1 at s = S//2: only the tap fl is inside
    gout = _synth.normal((c["B"], c["L"] * c["G"] * c["S"], c["H"], c["W"]), c["seed"], "gout")
    return dict(fmap1=f1, fmap2=f2, coords=coords, sigma=sigma, gout=gout)


# ---- the kernels' tap arithmetic in numpy fp32 -------------------------------------------------------------------------------

def taps32(coords, sigma, S, L, f, W2):
    """dkt_tap on the forward's expression, every operation an IEEE fp32 one: per level (fl, w, e), float32 (B,G,S,H,W)."""
    f32 = np.float32
    coords, sigma = np.asarray(coords, f32), np.asarray(sigma, f32)
    dx = (np.arange(S, dtype=f32) - f32(S // 2)).reshape(1, 1, S, 1, 1)
    out = []
    wi, div = W2, f32(1.0)
    with np.errstate(all="ignore"):
        x = dx * sigma[:, :, None] + coords[:, :, None]
        for _ in range(L):
            wm1 = f32(wi - 1)
            hwm1 = wm1 / f32(2.0)
            q = x / div
            xg = (f32(2.0) * q) / wm1 - f32(1.0)
            ix = (xg + f32(1.0)) * hwm1
            fl = np.floor(ix)
            w = ix - fl
            e = f32(1.0) - w
            assert x.dtype == q.dtype == ix.dtype == w.dtype == e.dtype == f32
            out.append((fl, w, e))
            wi //= f
            div = div * f32(f)
    return out


def floors32(coords, sigma, S, L, f, W2):
    return [t[0] for t in taps32(coords, sigma, S, L, f, W2)]


def _fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays: the product is exact in float64, the sum is rounded to odd there (TwoSum's error as
    the sticky bit), and an odd 53-bit number rounds to 24 bits as the exact sum does."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    nudge = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    s = np.where((err != 0) & even & np.isfinite(s), nudge, s)
    return s.astype(np.float32)


def _rows(level, B, H, W):
    return level.reshape(B, H, W, -1)


def _gather_np(level, idx, ok, B, H, W):
    """level (B H W, Wi) at integer taps idx (B,G,S,H,W) of the pixel's own row, 0 where not ok."""
    _, G, S = idx.shape[:3]
    wi = level.shape[-1]
    flat = np.clip(idx, 0, wi - 1).astype(np.int64).transpose(0, 3, 4, 1, 2).reshape(B, H, W, G * S)
    v = np.take_along_axis(_rows(level, B, H, W), flat, axis=-1).reshape(B, H, W, G, S).transpose(0, 3, 4, 1, 2)
    return np.where(ok, v, np.float32(0.0))


def lookup32(levels, coords, sigma, S, f):
    """The forward lookup in numpy fp32 on taps32: what dkt_pcv_lookup and the C oracle compute, bit for bit."""
    B, G, H, W = coords.shape
    levels = [np.asarray(l, np.float32).reshape(B * H * W, -1) for l in levels]
    outs = []
    with np.errstate(all="ignore"):
        for level, (fl, w, e) in zip(levels, taps32(coords, sigma, S, len(levels), f, levels[0].shape[-1])):
            wm1 = np.float32(level.shape[-1] - 1)
            v0 = _gather_np(level, fl, (fl >= 0) & (fl <= wm1), B, H, W)
            v1 = _gather_np(level, fl + np.float32(1.0), (fl + np.float32(1.0) >= 0) & (fl + np.float32(1.0) <= wm1), B, H, W)
            outs.append(_fma32(v1, w, v0 * e))
    return np.stack(outs, 1).reshape(B, len(levels) * G * S, H, W)


# ---- float64 closed form -----------------------------------------------------------------------------------------------------

def divisor_of(C):
    """sqrt(C) as the reference and the library form it: torch.sqrt(torch.tensor(C).float()), an fp32 number."""
    return float(np.sqrt(np.float32(C)))


def volume(f1, f2):
    """(B H W1, W2) in the dtype of the maps (torch)."""
    B, C, H, W1 = f1.shape
    return torch.einsum('bchw,bchv->bhwv', f1, f2).reshape(B * H * W1, -1) / divisor_of(C)


def pool(level, f):
    wo = level.shape[-1] // f
    return level[:, :wo * f].reshape(level.shape[0], wo, f).mean(-1)


def pyramid(f1, f2, L, f):
    pyr = [volume(f1, f2)]
    for _ in range(L - 1):
        pyr.append(pool(pyr[-1], f))
    return pyr


def _gather(level, idx, ok, B, H, W):
    _, G, S = idx.shape[:3]
    wi = level.shape[-1]
    flat = idx.clamp(0, wi - 1).long().permute(0, 3, 4, 1, 2).reshape(B, H, W, G * S)
    v = level.reshape(B, H, W, wi).gather(-1, flat).reshape(B, H, W, G, S).permute(0, 3, 4, 1, 2)
    return torch.where(ok, v, torch.zeros_like(v)) if ok is not None else v


def _scatter(val, idx, ok, wi, B, H, W):
    """(B H W, wi): val (B,G,S,H,W) added at the taps idx of each pixel's own row, where ok."""
    _, G, S = idx.shape[:3]
    flat = idx.clamp(0, wi - 1).long().permute(0, 3, 4, 1, 2).reshape(B, H, W, G * S)
    val = torch.where(ok, val, torch.zeros_like(val)).permute(0, 3, 4, 1, 2).reshape(B, H, W, G * S)
    return torch.zeros(B, H, W, wi, dtype=val.dtype).scatter_add_(-1, flat, val).reshape(B * H * W, wi)


def lookup_closed(levels, coords, sigma, gout, S, f, floors=None, mutant=None, dlevels=None):
    """dict(out, glevels [L], gcoords, gsigma) in float64 on the given levels (torch, any float dtype), with the floors given
    (list of (B,G,S,H,W) arrays) or float64's own; and under "bound" the bounds of the module docstring for them, dlevels
    being the error bounds of the level values (None: the levels are exact inputs)."""
    B, G, H, W = coords.shape
    L = len(levels)
    levels = [l.double().reshape(B * H * W, -1) for l in levels]
    coords, sigma = coords.double(), sigma.double()
    g_all = gout.double().reshape(B, L, G, S, H, W)
    dx = (torch.arange(S, dtype=torch.float64) - (S // 2)).reshape(1, 1, S, 1, 1)
    xs = dx * sigma[:, :, None]
    x = xs + coords[:, :, None]
    outs, glevels, b_out, b_gl = [], [], [], []
    gc = torch.zeros(B, G, H, W, dtype=torch.float64)
    gs, b_gc, b_gs = gc.clone(), gc.clone(), gc.clone()
    for lv, level in enumerate(levels):
        wi, div = level.shape[-1], float(f) ** lv
        ix = x / div
        fl = torch.floor(ix) if floors is None else torch.as_tensor(np.asarray(floors[lv], np.float64))
        w = ix - fl
        e = 1.0 - w
        in0 = (fl >= 0) & (fl <= wi - 1)
        in1 = (fl + 1 >= 0) & (fl + 1 <= wi - 1)
        counted = mutant == "oob_counted"
        v0, v1 = _gather(level, fl, None if counted else in0, B, H, W), _gather(level, fl + 1, None if counted else in1, B, H, W)
        g = g_all[:, lv]
        outs.append(v1 * w + v0 * e)
        w0, w1 = (w, e) if mutant == "weights_swapped" else (e, w)
        glevels.append(_scatter(g * w0, fl, in0, wi, B, H, W) + _scatter(g * w1, fl + 1, in1, wi, B, H, W))
        d = g * (v1 - v0) / (1.0 if mutant == "no_level_scale" else div)
        gc += d.sum(2)
        if not (mutant == "gsigma_drops_level" and lv == L - 1):
            gs += (d if mutant == "no_dx" else dx * d).sum(2)
        # the bounds
        A = (xs.abs() + x.abs()) / div + 4.0 * ix.abs() + 0.5 * (wi - 1)
        A = A.clamp(max=1e30)
        if dlevels is None:
            dv0 = dv1 = torch.zeros_like(v0)
        else:
            dl = dlevels[lv].double().reshape(B * H * W, -1)
            dv0, dv1 = _gather(dl, fl, in0, B, H, W), _gather(dl, fl + 1, in1, B, H, W)
        b_out.append(2.0 * U * (v0.abs() + v1.abs()) * (A + 2.0) + w.abs() * dv1 + e.abs() * dv0 + TINY)
        ones = torch.ones_like(g)
        n = _scatter(ones, fl, in0, wi, B, H, W) + _scatter(ones, fl + 1, in1, wi, B, H, W)
        ga = g.abs()
        b_gl.append(2.0 * U * (_scatter(ga * (A + 2.0), fl, in0, wi, B, H, W) + _scatter(ga * (A + 2.0), fl + 1, in1, wi, B, H, W)
                               + n * (_scatter(ga * e.abs(), fl, in0, wi, B, H, W) + _scatter(ga * w.abs(), fl + 1, in1, wi, B, H, W)))
                    + TINY * n)
        D = ga * (v0.abs() + v1.abs()) / div
        N = float(L * S)
        lev = ga * (dv0 + dv1) / div
        b_gc += (2.0 * U * (K_ARG + N) * D + lev + TINY * ga).sum(2)
        b_gs += (dx.abs() * (2.0 * U * (K_ARG + 1.0 + N) * D + lev + TINY * ga)).sum(2)
    out = torch.stack(outs, 1).reshape(B, L * G * S, H, W)
    bound = dict(out=torch.stack(b_out, 1).reshape(B, L * G * S, H, W), glevels=b_gl, gcoords=b_gc, gsigma=b_gs)
    return dict(out=out, glevels=glevels, gcoords=gc, gsigma=gs, bound=bound)


def pool_bwd_closed(glevels, f, divisor, mutant=None):
    """gvol (N, W2) in float64: the chain of the module docstring on the level gradients (torch (N, W_i))."""
    t = glevels[-1].double()
    for g in reversed(glevels[:-1]):
        g = g.double()
        wi, wn = g.shape[-1], t.shape[-1]
        src = torch.arange(wi) // f
        up = t[:, src.clamp(max=wn - 1)] / f
        if mutant != "pool_no_guard":
            up = up * (src < wn).double()
        t = g + up
    return t / (1.0 if mutant == "no_sqrt_c" else divisor)


def products(gvol, f1, f2):
    B, C, H, W1 = f1.shape
    G = gvol.reshape(B, H, W1, -1)
    return torch.einsum('bhwv,bchv->bchw', G, f2), torch.einsum('bhwv,bchw->bchv', G, f1)


def level_error_bounds(f1, f2, L, f):
    """dv_i of the module docstring: what a level built from the maps in fp32 may be off by."""
    C = f1.shape[1]
    pyr = pyramid(f1.double(), f2.double(), L, f)
    dv = [2.0 * U * (C + 2.0) * volume(f1.double().abs(), f2.double().abs())]
    for i in range(L - 1):
        dv.append(pool(dv[-1], f) + 2.0 * U * f * pool(pyr[i].abs(), f))
    return dv


def truth(a, c, floors=None, mutant=None, levels=None):
    """Everything of one case in float64 with its bounds.  levels None: the whole block from the maps (results out, gcoords,
    gsigma, glevels, gvol, gf1, gf2; the level values carry their fp32 error into the bounds).  levels given (fp32 arrays,
    (N, W_i)): the lookup alone on exactly those values."""
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in a.items()}
    S, f, L = c["S"], factor_of(c), c["L"]
    f1, f2 = t["fmap1"].double(), t["fmap2"].double()
    if levels is None:
        lv, dlv = pyramid(f1, f2, L, f), level_error_bounds(f1, f2, L, f)
    else:
        lv, dlv = [torch.from_numpy(np.ascontiguousarray(l)) for l in levels], None
    r = lookup_closed(lv, t["coords"], t["sigma"], t["gout"], S, f, floors, mutant, dlv)
    if levels is not None:
        return r
    divisor = divisor_of(c["C"])
    r["gvol"] = pool_bwd_closed(r["glevels"], f, divisor, mutant)
    r["gf1"], r["gf2"] = products(r["gvol"], f1, f2)
    b = r["bound"]
    b["gvol"] = pool_bwd_bound(r["glevels"], b["glevels"], f, divisor)
    gvabs = r["gvol"].abs()
    p1, p2 = products(gvabs, f1.abs(), f2.abs())
    q1, q2 = products(b["gvol"], f1.abs(), f2.abs())
    b["gf1"] = 2.0 * U * (c["W"] + 1.0) * p1 + q1 + TINY
    b["gf2"] = 2.0 * U * (c["W"] + 1.0) * p2 + q2 + TINY
    return r


def pool_bwd_bound(glevels, dglevels, f, divisor):
    """bound_gvol: 2 u (L + 1) Tabs / divisor, plus the chain on the level gradients' own bounds (zeros: they are inputs)."""
    L = len(glevels)
    tabs = pool_bwd_closed([g.abs() for g in glevels], f, divisor)
    return 2.0 * U * (L + 1.0) * tabs + pool_bwd_closed(dglevels, f, divisor) + TINY


# ---- the block restated in torch (fp32 yardstick, float64 cross-check, device arm of the benchmark) --------------------------

def sample_rows(level, x):
    """bilinear_sampler of pcvnet/utils/utils.py:61-76 on (N,1,1,W) rows at x (N,1,K,1): grid_sample, align_corners, zeros."""
    W = level.shape[-1]
    xgrid = 2 * x / (W - 1) - 1
    return F.grid_sample(level, torch.cat([xgrid, torch.zeros_like(x)], dim=-1), align_corners=True)


class TorchBlock:
    """corr.py:18-61 restated operation for operation, in the dtype and on the device of the maps."""

    def __init__(self, fmap1, fmap2, sample_num, num_levels, downsample):
        B, C, H, W1 = fmap1.shape
        self.S, self.L, self.f = sample_num, num_levels, 4 if downsample == 2 else 2
        corr = torch.einsum('aijk,aijh->ajkh', fmap1, fmap2).reshape(B, H, W1, 1, -1).contiguous()
        corr = corr / torch.sqrt(torch.tensor(C).float()).to(fmap1.dtype)
        corr = corr.reshape(B * H * W1, 1, 1, -1)
        self.corr_pyramid = [corr]
        for _ in range(num_levels - 1):
            corr = F.avg_pool2d(corr, [1, self.f], stride=[1, self.f])
            self.corr_pyramid.append(corr)

    @classmethod
    def on_levels(cls, levels, sample_num, factor):
        """The lookup alone, on given (N,1,1,W_i) levels."""
        self = cls.__new__(cls)
        self.S, self.L, self.f, self.corr_pyramid = sample_num, len(levels), factor, list(levels)
        return self

    def __call__(self, coords, sigma):
        B, G, H, W = coords.shape
        n = B * H * W
        sg = sigma.permute(0, 2, 3, 1).contiguous().reshape(n, 1, G, 1)
        cx = coords.permute(0, 2, 3, 1).contiguous().reshape(n, 1, G, 1)
        dx = (torch.arange(self.S, device=coords.device, dtype=coords.dtype) - (self.S // 2)).view(1, 1, 1, self.S)
        x = dx * sg + cx
        outs = []
        for i, level in enumerate(self.corr_pyramid):
            x0 = (x / self.f ** i).reshape(n, 1, G * self.S, 1)
            outs.append(sample_rows(level.contiguous(), x0.contiguous()).view(B, H, W, -1))
        return torch.cat(outs, dim=-1).permute(0, 3, 1, 2).contiguous()


def torch_chain(a, c, dtype, device="cpu", block=TorchBlock):
    """dict(out, gf1, gf2, gcoords, gsigma) of the block under autograd in `dtype`."""
    leaf = lambda k: torch.from_numpy(np.ascontiguousarray(a[k])).to(device=device, dtype=dtype).requires_grad_(True)  # noqa: E731
    f1, f2, coords, sigma = leaf("fmap1"), leaf("fmap2"), leaf("coords"), leaf("sigma")
    blk = block(f1, f2, sample_num=c["S"], num_levels=c["L"], downsample=c["downsample"])
    out = blk(coords, sigma)
    out.backward(torch.from_numpy(a["gout"]).to(device=device, dtype=out.dtype))
    return dict(out=out.detach(), gf1=f1.grad, gf2=f2.grad, gcoords=coords.grad, gsigma=sigma.grad)


def torch_lookup_chain(levels, a, c, dtype):
    """dict(out, glevels, gcoords, gsigma) of the lookup alone under autograd in `dtype`, on given (N, W_i) level values."""
    leaf = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dtype).requires_grad_(True)  # noqa: E731
    lv = [leaf(l) for l in levels]
    coords, sigma = leaf(a["coords"]), leaf(a["sigma"])
    blk = TorchBlock.on_levels([l.reshape(l.shape[0], 1, 1, -1) for l in lv], c["S"], factor_of(c))
    out = blk(coords, sigma)
    out.backward(torch.from_numpy(a["gout"]).to(dtype))
    return dict(out=out.detach(), glevels=[l.grad for l in lv], gcoords=coords.grad, gsigma=sigma.grad)


def torch_pool_chain(glevels, f, divisor, dtype):
    """gvol of the avg_pool2d chain and the division under autograd in `dtype` (glevels: (N, W_i) arrays)."""
    gl = [torch.from_numpy(np.ascontiguousarray(g)).to(dtype) for g in glevels]
    vol = torch.zeros(gl[0].shape[0], 1, 1, gl[0].shape[-1], dtype=dtype, requires_grad=True)
    level = vol / divisor
    pyr = [level]
    for _ in gl[1:]:
        level = F.avg_pool2d(level, [1, f], stride=[1, f])
        pyr.append(level)
    torch.autograd.backward(pyr, [g.reshape(p.shape) for g, p in zip(gl, pyr)])
    return vol.grad.reshape(gl[0].shape)


def level_grads(c):
    """float32 (N, W_i) upstream gradients of the levels, the inputs of the pool backward's own test."""
    N = c["B"] * c["H"] * c["W"]
    return [_synth.normal((N, w), c["seed"], "glevel%d" % i) for i, w in enumerate(widths(c))]


@functools.lru_cache(maxsize=None)
def reference(name):
    """Everything the tests share of one case, computed once: the inputs (numpy), the fp32 floors of the kernels' expression
    and the float64 truth on them, with its bounds."""
    c = CASES[name]
    a = inputs(c)
    fl = floors32(a["coords"], a["sigma"], c["S"], c["L"], factor_of(c), c["W"])
    return dict(a, floors=fl, truth=truth(a, c, floors=fl))


def worst(got, exact, bound):
    """max |got - exact| / bound over the elements; inf when got is not finite or differs where the bound is 0."""
    got = torch.as_tensor(got).detach().double().cpu().reshape(exact.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - exact).abs()
    if bool(((bound == 0) & (err > 0)).any()):
        return float("inf")
    return float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0


# ---- the three-iteration loop of model.py:120-142 with a stand-in head -------------------------------------------------------

LOOP = dict(seed=614, B=1, C=8, H=3, W=24, L=2, S=5, G=2, downsample=3, iters=3, kind="smooth")


def loop_inputs():
    c = LOOP
    a = inputs(c)
    ch = c["L"] * c["G"] * c["S"]
    a["head_sigma"] = _synth.normal((c["G"], ch), c["seed"], "head_sigma", scale=0.3 / ch ** 0.5)
    a["head_mu"] = _synth.normal((c["G"], ch), c["seed"], "head_mu", scale=1.0 / ch ** 0.5)
    a["gsig"] = _synth.normal((c["iters"],) + a["sigma"].shape, c["seed"], "gsig")
    a["gouts"] = _synth.normal((c["iters"],) + a["gout"].shape, c["seed"], "gouts")
    return a


def tap_margin(coords, sigma, S, L, f):
    """The smallest distance of any tap position ix of any level from an integer (float64)."""
    coords, sigma = coords.detach().double().cpu(), sigma.detach().double().cpu()
    dx = (torch.arange(S, dtype=torch.float64) - (S // 2)).reshape(1, 1, S, 1, 1)
    x = dx * sigma[:, :, None] + coords[:, :, None]
    return min(float((x / f ** i - torch.round(x / f ** i)).abs().min()) for i in range(L))


def loop(block, f1, f2, coords1, sigma, hs, hm, gouts, gsig, iters, watch=None):
    """coords1 detached every iteration, sigma the previous iteration's head output with its graph (model.py:121-122, :141);
    only what the stand-in head is given is detached.  The head: two 1x1 projections of the lookup; sigma stays within
    (0.5, 2.5), the means move by at most 1 and, being detached on their way into the next lookup, carry no gradient.
    watch(coords1, sigma) sees every lookup's arguments.  Returns the scalar loss and the per-iteration lookups."""
    corr_fn = block(f1, f2)
    loss, outs = 0.0, []
    for i in range(iters):
        coords1 = coords1.detach()
        if watch is not None:
            watch(coords1, sigma)
        corr = corr_fn(coords1, sigma)
        outs.append(corr)
        sigma = 1.5 + torch.tanh(torch.einsum('gc,bchw->bghw', hs, corr))
        mu = torch.tanh(torch.einsum('gc,bchw->bghw', hm, corr))
        coords1 = coords1 - mu
        loss = loss + (corr * gouts[i]).sum() + (sigma * gsig[i]).sum()
    return loss, outs
