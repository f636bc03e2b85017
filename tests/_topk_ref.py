"""Float64 truth, fp32 yardstick, closed-form gradients, error bounds, fixed cases and mutants for CGI-Stereo's top-k
disparity head (topk_regress.hip; test infrastructure in the layout of _soft_argmin_ref.py).

Operator.  cost (B, D, h, w), samples (B, D, h, w) or None (the plane index), 1 <= k <= D.  Per pixel, with d_0 .. d_k-1 the
planes of cost.sort(dim=1, descending=True, stable=True)[:k] (NaN above every number, equal values in ascending plane order),
c_i = cost[d_i], s_i = samples[d_i] or float(d_i):

    t_i = c_i - c_0,  e_i = exp(t_i),  S = sum_i e_i,  p_i = e_i / S,  out = pred = sum_i s_i p_i

Gradients (closed form), g the upstream gradient of the pixel:

    gcost[d_i] = g p_i (s_i - pred),   gsamples[d_i] = g p_i,   every other plane of both exactly 0.

Bounds (u = 2^-24; every statement to first order in u, the factor 2 in front covers the rest, as in the other _*_ref.py).
Per element, from magnitudes of the float64 truth.  K = k.
  t_i is one subtraction: within u |t_i|.  expf is within one ulp (2 u) of the exponential of its argument, so e_i is
  relatively within (|t_i| + 2) u.  S takes K - 1 additions, each within u of a partial sum that S bounds, and carries the
  errors of its terms: relatively within (T + 2 + K - 1) u with T = sum_j p_j |t_j| (the spread of the kept values enters
  here and in |t_i|; T <= K/e, a far plane has a small p_j).  The quotient rounds once, or twice where it is formed as
  e_i (1/S), as a vectorised softmax does.  So
      |dp_i| <= c_i u p_i + TINY,   c_i = |t_i| + T + K + 5.
  TINY = 2^-126: a term below the smallest normal number may be flushed or rounded as a subnormal; the relative statement
  does not hold for it, the absolute one (S >= 1) does.
  out.  K products (u each) and K - 1 additions in any order, of terms whose magnitudes sum to sum_j p_j |s_j|:
      e_pred = sum_j p_j |s_j| (c_j + K + 1),     bound_out = 2 u e_pred + TINY sum_j |s_j|.
  (one u more than the forward needs: the gradient below uses the same e_pred for the sum sum_j (g s_j) p_j of autograd.)
  gsamples.  One product:  bound_gsamples[d_i] = 2 u |g| p_i (c_i + 1) + TINY |g|.
  gcost.  As g p_i (s_i - pred): the difference is off by the error of pred and one rounding, the two products add u each:
  u |g| p_i ((c_i + 3) |s_i - pred| + e_pred).  As autograd forms it, p_i (g s_i - sum_j (g s_j) p_j): the product g s_i
  rounds at u |g| |s_i| BEFORE the cancellation, the sum is within u |g| e_pred, the difference and the product add
  (c_i + 2) u |g| |s_i - pred|.  The bound covers both:
      bound_gcost[d_i] = 2 u |g| p_i ((c_i + 4) |s_i - pred| + e_pred + |s_i|) + 2 TINY |g| sum_j |s_j|.
  The unselected planes admit only an exact 0 (bound 0).  K = 1: p = 1, pred = s_0 and gcost = 0 exactly; the bounds are not 0
  there, which costs nothing.  A pixel whose column holds a NaN is NaN in the truth: there a result has to be NaN in exactly
  the truth's places (worst()), and no bound applies.

Envelope.  Where two nodes are chained (cgi_disparity_head) the errors one stage hands to the next are met by the fp32
yardstick too, which runs the same stages: envelope = 8 max(|yardstick - truth|, floor), the project's usual rule, with
floor the first-order form (no factor 2) of the bound of the stage that produces the result, from the truth's magnitudes.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import _context_upsample_ref as CU
import _synth

U = 2.0 ** -24
TINY = 2.0 ** -126


def _case(seed, D, k, B=2, h=5, w=67, amp=3.0, **kw):
    return dict(seed=seed, B=B, D=D, h=h, w=w, k=k, amp=float(amp), **kw)


#: w = 67 crosses a wave (64 pixels) inside a row and a block of 64 threads; 5 x 67 = 335 pixels are 6 blocks, the last ragged
CASES = {
    "k1": _case(501, 48, 1),
    "k2": _case(502, 48, 2),
    "k3": _case(503, 48, 3),
    "k8": _case(504, 48, 8),
    "samples": _case(505, 48, 2, samples=True),             # random, non-monotone samples
    "kD": _case(506, 3, 3),                                 # k = D
    "d1": _case(507, 1, 1),
    "d256": _case(508, 256, 2, planted=True),               # the maximum at plane 255 in even pixels, at plane 0 in odd ones
    "offset": _case(509, 48, 2, offset=3000.0),             # columns at +3000 and at -3000: needs the maximum subtracted
    "nan": _case(510, 48, 2, nan=True),                     # one pixel whose column holds a NaN
    "tie": _case(511, 48, 2, tie=True),                     # exact duplicates straddle the k-th place
    "strided": _case(512, 48, 2, strided=True),             # cost and gout are every second image of buffers of four
    "mem": _case(513, 48, 2, B=1, h=32, w=64),              # the shape of the memory check
}

#: the pixel of the "nan" case that holds the NaN: (b, plane, y, x)
NAN_AT = (1, 17, 2, 65)

#: mutant -> (the result whose bound it must miss, the case on which it must)
MUTANTS = {
    "k_smallest": ("out", "k2"),
    "tie_highest": ("out", "tie"),
    "no_max_sub": ("out", "offset"),
    "index_for_samples": ("out", "samples"),
    "drop_kth": ("out", "k3"),
    "skip_last_plane": ("out", "d256"),
    "grad_plane_off": ("gcost", "k2"),
    "gcost_unwritten": ("gcost", "k2"),
    "no_bstride": ("out", "strided"),
}


def inputs(c):
    """float32 numpy: cost (B, D, h, w), gout (B, 1, h, w), samples (B, D, h, w) or None; for the strided case also
    wide_cost and wide_gout (2B, ...) with cost = wide_cost[::2], gout = wide_gout[::2] and other data in between."""
    B, D, h, w = c["B"], c["D"], c["h"], c["w"]
    nb = 2 * B if c.get("strided") else B
    cost = _synth.normal((nb, D, h, w), c["seed"], "cost", scale=c["amp"])
    gout = _synth.normal((nb, 1, h, w), c["seed"], "gout")
    pix = np.arange(h * w).reshape(h, w)
    if c.get("planted"):
        cost[:, D - 1][:, pix % 2 == 0] = 40.0
        cost[:, 0][:, pix % 2 == 1] = 40.0
    if c.get("offset"):
        # near 3000 a float32 has 2^-12 between neighbours and random values would collide: every column is a permutation
        # of D distinct levels, multiples of 2^-5 with uneven gaps, which the offset leaves exact
        j = np.arange(D)
        levels = (0.25 * j + 0.03125 * (j * j % 7) - 6.0).astype(np.float32)
        perm = _synth.rng(c["seed"], "perm").permuted(np.tile(j, (nb, h, w, 1)), axis=-1)
        cost = np.ascontiguousarray(levels[perm].transpose(0, 3, 1, 2))
        cost += np.where(pix % 2 == 0, np.float32(c["offset"]), np.float32(-c["offset"]))[None, None]
    if c.get("nan"):
        cost[NAN_AT] = np.nan
    if c.get("tie"):
        # even pixels: a single maximum at plane 30, the runner-up twice, at planes 7 and 21 (plane 7 must be kept);
        # odd pixels: the maximum three times, at planes 40, 5 and 12 (planes 5 and 12 must be kept, in that order)
        even, odd = pix % 2 == 0, pix % 2 == 1
        cost[:, 30][:, even] = 50.0
        cost[:, 7][:, even] = 45.0
        cost[:, 21][:, even] = 45.0
        for plane in (40, 5, 12):
            cost[:, plane][:, odd] = 50.0
    out = dict(cost=cost, gout=gout, samples=None)
    if c.get("samples"):
        out["samples"] = _synth.normal((nb, D, h, w), c["seed"], "samples", scale=20.0)
    if c.get("strided"):
        out.update(wide_cost=cost, wide_gout=gout, cost=np.ascontiguousarray(cost[::2]), gout=np.ascontiguousarray(gout[::2]))
    return out


def select(cost, k, mutant=None):
    """(values (B, k, h, w), planes (B, k, h, w) int64) of the k kept entries of every column, best first."""
    if mutant == "k_smallest":
        _, ind = cost.sort(dim=1, descending=False, stable=True)
    elif mutant == "tie_highest":
        _, ind = cost.flip(1).sort(dim=1, descending=True, stable=True)
        ind = cost.shape[1] - 1 - ind
    elif mutant == "skip_last_plane" and cost.shape[1] > k:
        _, ind = cost[:, :-1].sort(dim=1, descending=True, stable=True)
    else:
        _, ind = cost.sort(dim=1, descending=True, stable=True)
    ind = ind[:, :k]
    return torch.gather(cost, 1, ind), ind


def _samples_of(cost, samples, ind, mutant=None):
    if samples is None or mutant == "index_for_samples":
        return ind.to(cost.dtype)
    return torch.gather(samples.to(cost.dtype), 1, ind)


def _scatter(values, ind, D, fill=0.0):
    B, _, h, w = values.shape
    out = torch.full((B, D, h, w), fill, dtype=values.dtype)
    return out.scatter(1, ind, values)


def closed_form(cost, samples, gout, k, mutant=None, wide_cost=None):
    """dict(out (B, 1, h, w), gcost, gsamples (B, D, h, w; None without samples), idx (B, k, h, w) int64) in float64 from the
    stable sort and the closed-form gradients (float32 torch tensors in)."""
    cost, g = cost.double(), gout.double()
    if mutant == "no_bstride":
        cost = wide_cost.double()[:cost.shape[0]]           # image b read at b times one image, not at its stride
    D = cost.shape[1]
    c, ind = select(cost, k, mutant)
    s = _samples_of(cost, samples, ind, mutant)
    if mutant == "no_max_sub":
        e = torch.exp(c.float())                            # in fp32, as it would run
        p = (e / e.sum(1, keepdim=True)).double()
    else:
        p = torch.softmax(c, 1)
    terms = s * p
    pred = (terms[:, :k - 1] if mutant == "drop_kth" else terms).sum(1, keepdim=True)
    where = (ind + 1) % D if mutant == "grad_plane_off" else ind
    gcost = _scatter(g * p * (s - pred), where, D, float("nan") if mutant == "gcost_unwritten" else 0.0)
    gsamples = None if samples is None else _scatter(g * p, ind, D)
    return dict(out=pred, gcost=gcost, gsamples=gsamples, idx=ind)


def bounds(cost, samples, gout, k):
    """dict(out, gcost, gsamples) of the bounds of the module docstring, shaped like the results (float64)."""
    cost, g = cost.double(), gout.double().abs()
    D = cost.shape[1]
    c, ind = select(cost, k)
    s = _samples_of(cost, samples, ind)
    p = torch.softmax(c, 1)
    pred = (s * p).sum(1, keepdim=True)
    t = (c - c[:, :1]).abs()
    T = (p * t).sum(1, keepdim=True)
    ci = t + T + (k + 5.0)
    sabs = s.abs().sum(1, keepdim=True)
    e_pred = (p * s.abs() * (ci + k + 1.0)).sum(1, keepdim=True)
    b_out = 2.0 * U * e_pred + TINY * sabs
    b_gs = 2.0 * U * g * p * (ci + 1.0) + TINY * g
    b_gc = 2.0 * U * g * p * ((ci + 4.0) * (s - pred).abs() + e_pred + s.abs()) + 2.0 * TINY * g * sabs
    return dict(out=b_out, gcost=_scatter(b_gc, ind, D), gsamples=None if samples is None else _scatter(b_gs, ind, D))


def torch_chain_graph(cost, disparity_samples, k):
    """The reference's lines (meta_arch/cgi/submodule.py:220-228) on tensors of any dtype or device; the sort is asked to
    be stable, which selects what the reference's selects wherever the k-th and (k+1)-th values of a column differ."""
    _, ind = cost.sort(dim=1, descending=True, stable=True)
    pool_ind = ind[:, :k]
    cost = torch.gather(cost, 1, pool_ind)
    prob = F.softmax(cost, 1)
    disparity_samples = torch.gather(disparity_samples, 1, pool_ind)
    return torch.sum(disparity_samples * prob, dim=1, keepdim=True)


def arange_samples(cost):
    """CGI_Stereo.py:256-257: the plane index repeated to the cost's shape."""
    B, D, h, w = cost.shape
    return torch.arange(0, D, dtype=cost.dtype, device=cost.device).view(1, D, 1, 1).repeat(B, 1, h, w)


def torch_chain(cost, samples, gout, k, dtype):
    """dict(out, gcost, gsamples) of those lines under autograd in `dtype` on the CPU (gsamples None without samples)."""
    c = cost.to(dtype).requires_grad_(True)
    s = arange_samples(c.detach()) if samples is None else samples.to(dtype).requires_grad_(True)
    out = torch_chain_graph(c, s, k)
    if samples is None:
        (gc,), gs = torch.autograd.grad(out, (c,), gout.to(dtype)), None
    else:
        gc, gs = torch.autograd.grad(out, (c, s), gout.to(dtype))
    return dict(out=out.detach(), gcost=gc, gsamples=gs)


def head_chain(cost, spx_logits, k, training):
    """CGI_Stereo.py:253-268 restated on a (B, D, h, w) cost and the (B, 9, 4h, 4w) output of self.spx, any dtype."""
    spx_pred = F.softmax(spx_logits, 1)
    pred = torch_chain_graph(cost, arange_samples(cost), k)
    pred_up = CU.sequence(pred, spx_pred).unsqueeze(1)
    if training:
        return [-pred * 4, -pred_up * 4]
    return -pred_up * 4


def tie_free(cost, k):
    """True where the k-th and (k+1)-th largest of a column differ (or k = D): (B, h, w) bool."""
    if k == cost.shape[1]:
        return torch.ones(cost[:, 0].shape, dtype=torch.bool)
    v, _ = cost.sort(dim=1, descending=True, stable=True)
    a, b = v[:, k - 1], v[:, k]
    return (a != b) & ~(torch.isnan(a) & torch.isnan(b))


@functools.lru_cache(maxsize=None)
def reference(name):
    """Everything the tests share of one case, computed once: the inputs (numpy), the float64 truth and the bounds."""
    c = CASES[name]
    a = inputs(c)
    t = lambda v: None if v is None else torch.from_numpy(v)  # noqa: E731
    truth = closed_form(t(a["cost"]), t(a["samples"]), t(a["gout"]), c["k"])
    return dict(a, truth=truth, bound=bounds(t(a["cost"]), t(a["samples"]), t(a["gout"]), c["k"]))


def envelope(yard, truth, floor):
    """8 max(|yardstick - truth|, floor), per element."""
    return 8.0 * torch.maximum((yard.detach().double().cpu() - truth).abs(), floor)


def worst(got, exact, bound):
    """max |got - exact| / bound over the elements (bound shaped like them).  inf when got is NaN anywhere but in the truth's
    own NaN places, misses one of them, is otherwise not finite, or differs where the bound is 0 (only the exact result is
    admitted there)."""
    got = got.detach().double().cpu()
    nan = torch.isnan(exact)
    if got.shape != exact.shape or not torch.equal(torch.isnan(got), nan):
        return float("inf")
    got, exact, bound = got[~nan], exact[~nan], bound[~nan]
    if got.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - exact).abs()
    if bool(((bound == 0) & (err > 0)).any()):
        return float("inf")
    return float((err / bound.clamp(min=1e-300)).max())


def same(a, b):
    """Bit for bit, NaNs compared by position."""
    return CU.same(a, b)
