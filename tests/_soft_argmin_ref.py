"""Float64 truth, fp32 yardstick, closed-form gradient, error bounds, fixed cases and mutants for the soft-argmin heads
(soft_argmin.hip; test infrastructure in the layout of _context_upsample_ref.py).

Operator.  cost (B, Dc, h, w), factor f in {1, 4}, D = f Dc, H = f h, W = f w:

    out[b, 0, Y, X] = out_scale * E,   E = sum_d d p_d,   p = softmax_d(z),   z = up(cost)[b, :, Y, X]

up is torch's trilinear align_corners=False up-sampling at exactly 1/f per axis, restated per axis of coarse length n (taps()):
fine index o reads i0 = floor(src), i1 = min(i0 + 1, n - 1) at lambda = src - i0 with src = max(0, (o + 0.5)/f - 0.5).  The
truth is built from these taps in float64, not from F.interpolate; test_host_soft_argmin_ref.py shows the two agree.

Gradient (closed form).  u_d = out_scale g p_d (d - E) is the gradient of z_d; gcost is u through the transposes of the three
interpolations (index_add of (1 - lambda) u to i0 and lambda u to i1 per axis).

Bounds (eps = 2^-23 = 2 u; every statement to first order, the factor 2 in front covers the rest, as in the other
_*_ref.py).  They are per element, from magnitudes of the float64 truth: per output pixel E and the mean absolute deviation
A = sum_d p_d |d - E|; M = max|cost|.

  logits.  One interpolation, as w0 a + w1 b or as a + lambda (b - a), is at most 4.5 u M off (the difference rounds to
  within 2 u M, the product and the sum add u each on values <= 2 M and M; lambda <= .875).  Three axes, and the subtraction
  of the shift (|z - max| <= 2 M, one rounding): 15.5 u M, so |dz| <= 7.75 eps M.  A perturbation dz of the logits moves E by
  sum_d p_d (d - E) dz_d, at most max|dz| A.  expf (one ulp, 2 u) perturbs a term of both sums alike: another eps A.
  Z is the largest |cost| the pixel reads (its column in the 2 x 2 coarse cells around it; M = max|cost| >= Z): with it in
  place of M the statements above hold pixel by pixel.
  sums.  Each of the two sums takes D - 1 additions, and where it is streamed with a running maximum one product per four
  logits more (the rescale factor itself is common to both sums and cancels in E): n = 1.25 D + 1 roundings, each uniform
  within u of a partial sum that the total bounds, so their sum has a standard deviation of at most u sqrt(n)/3 of the total.
  The worst case n u is never approached by 200 independent roundings; they are counted at six standard deviations,
  2 sqrt(n) u per sum.  A relative error of either sum moves E by that times E.  The product d e and the division: u each.
      e_E = A (7.75 Z + 1) + E (2 sqrt(n) + 1)                       (in units of eps)
      bound_out = 2 eps |out_scale| e_E           <= bound_fwd(D, M) = 2 eps |out_scale| (D - 1) ((7.75 M + 1)/2 + 2 sqrt(n) + 1)
  (A <= (D - 1)/2, E <= D - 1: the envelope has the form eps (D - 1)(a + b M); the GWCNet comparison uses it.)
  gradient.  p_d is relatively within 2 |dz| (its own logit and the normalisation) + eps (expf) + sqrt(n) eps (the sum) +
  eps (reciprocal, product); d - E, the two products of u_d and the factor out_scale: 1.5 eps and the error of E.  So
  |du_d| <= eps |g| p_d (|d - E| (15.5 Z + sqrt(n) + 3.5) + e_E).  An element of gcost adds n_t = 8 (2f)^2 terms at f = 4
  (8 fine logits of each of (2f)^2 output pixels; 1 at f = 1) with three weight products each: (sqrt(n_t) + 1.5) eps of the
  sum of their magnitudes, the additions again at six standard deviations.  With T the transpose of the three interpolations:
      bound_gcost = 2 eps |out_scale| T(|g| p (c_u |d - E| + e_E)),   c_u = 15.5 Z + sqrt(n) + sqrt(n_t) + 5
  It is absolute where it matters: at Dc = 1, f = 4 the true gradient is 0 and the bound is not (at D = 1 both are 0).
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import _synth

EPS = 2.0 ** -23


def n_roundings(D):
    """Roundings of one of the two sums: D - 1 additions and one rescale product per four logits."""
    return 1.25 * D + 1.0


def bound_fwd(D, M, out_scale=1.0):
    """The envelope of bound_out over every distribution on [0, D - 1]."""
    return 2.0 * EPS * abs(out_scale) * (D - 1) * ((7.75 * M + 1.0) / 2.0 + 2.0 * n_roundings(D) ** 0.5 + 1.0)


def bounds(cost, gout, f, out_scale=1.0):
    """(bound_out (B, 1, H, W), bound_gcost (B, Dc, h, w)) from the float64 truth's magnitudes (module docstring)."""
    cost, g = cost.double(), gout.double().abs()
    Z = cost.abs().amax(1, keepdim=True)
    for dim in (2, 3):                                      # the larger of the two coarse cells a fine index reads, per axis
        i0, i1, _ = taps(Z.shape[dim], f)
        Z = torch.maximum(Z.index_select(dim, i0), Z.index_select(dim, i1))
    p = torch.softmax(up(cost, f), 1)
    D = p.shape[1]
    d = torch.arange(D, dtype=torch.float64).view(1, D, 1, 1)
    E = (p * d).sum(1, keepdim=True)
    dev = (d - E).abs()
    A = (p * dev).sum(1, keepdim=True)
    sq = n_roundings(D) ** 0.5
    e_E = A * (7.75 * Z + 1.0) + E * (2.0 * sq + 1.0)
    n_t = 8.0 * (2 * f) ** 2 if f > 1 else 1.0
    c_u = 15.5 * Z + sq + n_t ** 0.5 + 5.0
    mag = g * p * (c_u * dev + e_E)
    for dim in (3, 2, 1):
        mag = interp_T(mag, dim, f)
    k = 2.0 * EPS * abs(out_scale)
    return k * e_E, k * mag


def _case(seed, B, Dc, h, w, f, amp, offset=0.0, **kw):
    return dict(seed=seed, B=B, Dc=Dc, h=h, w=w, f=f, amp=float(amp), offset=float(offset), **kw)


CASES = {
    "batch2": _case(401, 2, 48, 5, 7, 4, 1),
    "tiles": _case(402, 1, 48, 9, 17, 4, 10),               # 5 x 3 tiles of 8 x 32 output pixels (2 x 8 coarse cells), ragged both ways
    "peaked": _case(403, 1, 48, 5, 7, 4, 50),
    "offset": _case(404, 1, 48, 3, 4, 4, 5, 1e4),          # needs the shift by the maximum
    "spike": _case(405, 1, 48, 3, 4, 4, 2, spike=True),    # needs the shift by the maximum of the FINE logits
    "dc1": _case(406, 1, 1, 3, 3, 4, 1),                    # E = (D - 1)/2, zero gradient
    "one": _case(407, 2, 2, 1, 1, 4, 3),
    "dc3": _case(408, 1, 3, 2, 5, 4, 8),
    "tall": _case(409, 1, 12, 33, 3, 4, 3),
    "d256": _case(410, 1, 64, 2, 3, 4, 5),                  # D = 256, the limit
    "f1": _case(411, 2, 48, 6, 10, 1, 5),
    "f1_one": _case(412, 1, 1, 2, 2, 1, 1),
    "strided": _case(413, 2, 48, 5, 7, 4, 3, strided=True),  # the GPU tests pass it as every second image of a batch of four
}

#: mutant -> (the result whose bound it must miss, the case on which it must)
MUTANTS = {
    "align_corners": ("out", "tiles"),
    "unclamped_i1": ("out", "peaked"),
    "no_max0": ("out", "peaked"),
    "d_plus_one": ("out", "batch2"),
    "coarse_max": ("out", "spike"),
    "drop_halo": ("gcost", "dc3"),
    "no_minus_E": ("gcost", "batch2"),
    "drop_halo_w": ("gcost", "tiles"),                      # the mild ones, on 48-plane cases
    "no_last_slot": ("gcost", "batch2"),
}


def inputs(c):
    """cost (B, Dc, h, w), gout (B, 1, f h, f w): float32 numpy."""
    B, Dc, h, w, f = c["B"], c["Dc"], c["h"], c["w"], c["f"]
    cost = _synth.normal((B, Dc, h, w), c["seed"], "cost", scale=c["amp"]) + np.float32(c["offset"])
    if c.get("spike"):
        cost[0, 20, 1, 1] = 2000.0
        cost[0, 30, 1, 2] = -3000.0
    gout = _synth.normal((B, 1, f * h, f * w), c["seed"], "gout")
    return cost.astype(np.float32), gout


def taps(n, f, mutant=None):
    """(i0, i1, lambda) of the f n fine indices of an axis of coarse length n: int64, int64, float64.  The mutants may
    leave [0, n): interp() reads 0 there."""
    o = torch.arange(f * n, dtype=torch.float64)
    if mutant == "align_corners":
        src = o * ((n - 1) / (f * n - 1)) if n > 1 else torch.zeros_like(o)
    else:
        src = (o + 0.5) / f - 0.5
        if mutant != "no_max0":
            src = src.clamp(min=0.0)
    i0 = torch.floor(src)
    lam = src - i0
    i0 = i0.long()
    i1 = i0 + 1 if mutant == "unclamped_i1" else torch.clamp(i0 + 1, max=n - 1)
    return i0, i1, lam


def _shaped(v, dim, t):
    shape = [1] * t.dim()
    shape[dim] = -1
    return v.to(t.dtype).view(shape)


def interp(t, dim, f, mutant=None):
    """One axis of up()."""
    n = t.shape[dim]
    i0, i1, lam = taps(n, f, mutant)
    zero = torch.zeros_like(t.narrow(dim, 0, 1))
    p = torch.cat([zero, t, zero], dim)
    return p.index_select(dim, i0 + 1) * _shaped(1.0 - lam, dim, t) + p.index_select(dim, i1 + 1) * _shaped(lam, dim, t)


def interp_T(u, dim, f, mutant=None):
    """Its transpose: (.., f n, ..) -> (.., n, ..).  drop_halo: the gather of a coarse cell of H or W stops one fine index
    short (it leaves out o = 4c + 5, the last of the eight that read cell c); drop_halo_w: along W only; no_last_slot: the
    two fine logits past the last coarse plane (the slot k = Dc of the kernel) give it nothing."""
    n = u.shape[dim] // f
    i0, i1, lam = taps(n, f)
    w0 = 1.0 - lam
    if ((mutant == "drop_halo" and dim >= 2) or (mutant == "drop_halo_w" and dim == 3)) and f == 4:
        w0 = torch.where(torch.arange(f * n) % 4 == 1, torch.zeros_like(w0), w0)
    if mutant == "no_last_slot" and dim == 1 and f == 4:
        w0 = torch.where(torch.arange(f * n) >= f * n - 2, torch.zeros_like(w0), w0)
        lam = torch.where(torch.arange(f * n) >= f * n - 2, torch.zeros_like(lam), lam)
    shape = list(u.shape)
    shape[dim] = n
    out = torch.zeros(shape, dtype=u.dtype)
    out.index_add_(dim, i0, u * _shaped(w0, dim, u))
    out.index_add_(dim, i1, u * _shaped(lam, dim, u))
    return out


def up(cost, f, mutant=None):
    for dim in (1, 2, 3):
        cost = interp(cost, dim, f, mutant)
    return cost


def closed_form(cost, gout, f, out_scale=1.0, mutant=None):
    """(out (B, 1, H, W), gcost (B, Dc, h, w)) in float64 from the restated taps and the closed-form gradient (torch tensors in)."""
    cost, g = cost.double(), gout.double()
    z = up(cost, f, mutant if mutant in ("align_corners", "unclamped_i1", "no_max0") else None)
    D = z.shape[1]
    d = torch.arange(D, dtype=torch.float64).view(1, D, 1, 1) + (1.0 if mutant == "d_plus_one" else 0.0)
    if mutant == "coarse_max":
        # the shift of a kernel that takes one maximum over the coarse values it has staged (here: the image), in fp32 as it
        # would run; a fine logit lies up to .125 of the spread below every coarse value, and far below a distant one
        shift = cost.amax((1, 2, 3), keepdim=True)
        e = torch.exp((z - shift).float())
        p = (e / e.sum(1, keepdim=True)).double()
    else:
        p = torch.softmax(z, 1)
    E = (p * d).sum(1, keepdim=True)
    u = out_scale * g * p * (d if mutant == "no_minus_E" else d - E)
    for dim in (3, 2, 1):
        u = interp_T(u, dim, f, mutant)
    return out_scale * E, u


def torch_chain_graph(c, f, out_scale):
    """The reference's lines (gwc_main.py:246-276; igev_stereo.py:175-176 at f = 1) on `c` (B, Dc, h, w), any dtype or device."""
    z = c
    if f != 1:
        z = F.interpolate(c[:, None], scale_factor=f, mode="trilinear", align_corners=False).squeeze(1)
    p = F.softmax(z, dim=1)
    d = torch.arange(0, z.shape[1], dtype=c.dtype, device=c.device).view(1, -1, 1, 1)
    return out_scale * torch.sum(p * d, 1, keepdim=True)


def torch_chain(cost, gout, f, out_scale, dtype):
    """(out, gcost) of those lines under autograd in `dtype` on the CPU."""
    c = cost.to(dtype).requires_grad_(True)
    out = torch_chain_graph(c, f, out_scale)
    (gc,) = torch.autograd.grad(out, c, gout.to(dtype))
    return out.detach(), gc


@functools.lru_cache(maxsize=None)
def reference(name, out_scale=1.0):
    """Everything the tests share of one case, computed once: inputs (numpy), the float64 truth, the two bounds."""
    c = CASES[name]
    cost, gout = inputs(c)
    out, gcost = closed_form(torch.from_numpy(cost), torch.from_numpy(gout), c["f"], out_scale)
    bound_out, bound_gcost = bounds(torch.from_numpy(cost), torch.from_numpy(gout), c["f"], out_scale)
    return dict(cost=cost, gout=gout, out=out, gcost=gcost, bound_out=bound_out, bound_gcost=bound_gcost)


def worst(got, exact, bound):
    """max |got - exact| / bound over the elements (bound shaped like them); inf when anything is not finite.  An element
    whose bound is 0 (D = 1) admits only the exact result."""
    got = got.detach().double().cpu()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - exact).abs()
    if bool(((bound == 0) & (err > 0)).any()):
        return float("inf")
    return float((err / bound.clamp(min=1e-300)).max())


def same(a, b):
    """Bit for bit."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
