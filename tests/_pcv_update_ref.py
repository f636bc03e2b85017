"""Float64 truth, fp32 yardstick, closed-form gradients, error bounds, fixed cases and mutants for PCVNet's mixture-parameter
update (pcv_update.hip, pcvnet_update.py; test infrastructure in the layout of _pcv_train_ref.py).

Operator (meta_arch/pcvnet/update.py:92-107 and model.py:154).  delta, mu, sigma, w (N,M,H,W); per pixel, j over the M gaussians:
    ds_raw = 0.5 (((1 - M w) s^2 - s0^2 - d^2) / (M s^3) + w s / s0^2)       dm_raw = -0.5 d (1 / (M s^2) + w / s0^2)
    beta = 0.5 (-1 / (M w + eps) + log(s0 M w / s + eps) + (s^2 + d^2) / (2 s0^2) + 0.5)       dw_raw = beta - (sum_j beta) / M
    ds = clip(g1 ds_raw, +-3)   dm = clip(g2 dm_raw, +-128)   dw = clip(g3 dw_raw, +-1/(4M))
    s' = clip(s - ds, 0.1, 16)   mu' = mu - dm   w~ = clip(w - dw, 0, 1)   w' = w~ / T, T = sum_j w~   disp = sum_j w' mu'
Gradients (closed form), c the pass indicators of the five clips (1 inside or ON an edge: torch.clamp's backward), u = s0 M w / s + eps:
    Gmu' = gmu' + gdisp w'   Gw' = gw' + gdisp mu'   Gw~ = (Gw' - sum_k Gw'_k w'_k) / T   A = c_W Gw~   B = -g3 c_w A
    gbeta = B - (sum_k B_k) / M   E = c_S gs'   g_ds = -g1 c_s E   g_dm = -g2 c_m Gmu'
    gd = g_ds (-d / (M s^3)) + g_dm (-0.5 (1 / (M s^2) + w / s0^2)) + gbeta d / (2 s0^2)
    gs = E + g_ds 0.5 (-(1 - M w) / (M s^2) + 3 (s0^2 + d^2) / (M s^4) + w / s0^2) + g_dm d / (M s^3) + gbeta 0.5 (-(s0 M w / s^2) / u + s / s0^2)
    gw = A + g_ds 0.5 (-1 / s + s / s0^2) + g_dm (-0.5 d / s0^2) + gbeta 0.5 (M / (M w + eps)^2 + (s0 M / s) / u)       gmu = Gmu'

Decisions.  Every output jumps (in value or in slope) where a pre-clip value crosses its edge, so a result is only defined
once the five decisions of its element are.  chain() therefore takes them as data (`decisions=`, the byte of the kernel: 0 below,
1 inside or on an edge, 2 above, packed (((ds 3 + dm) 3 + dw) 3 + s') 3 + w~); without them it takes float64's own.  The margin
of a decision is the distance of the pre-clip value from the nearer edge; a decision is OPEN where the margin does not exceed
the bound of that value, and an element is open when one of its five is.  A device must reproduce the truth's byte on every
element that is not open, values and gradients are compared with chain(decisions=the device's), and at most MAY_DIFFER of a
case's elements may be open.  (A later clip of an element sees the earlier one's result; no decision reaches another element.)

Bounds (u = 2^-24, first order; the factor 2 in front covers the rest, as in the other _*_ref.py).  They are a running error
analysis of the float64 chain itself: every number carries the absolute error its fp32 counterpart may have,
    x op y:  the errors of x and y through the operation's partial derivatives at the truth's own values, plus u |result|
    (a product or quotient by a power of two adds nothing; a constant that is no fp32 number enters with u |constant|),
    log: the argument's relative error plus 2 u |log| (logf and ATen's are within one ulp),
    a sum of M terms in any order: the terms' errors plus (M - 1) u sum |term|,
    a clip with its decision given: the value's error inside, the edge's rounding outside; a pass indicator: the error or 0.
A difference therefore carries the absolute sizes of what it cancels: ds_raw's numerator enters with
u (several) ((1 + M w) s^2 + s0^2 + d^2) and is divided by M s^3 like the value, never with u |ds_raw|; w' and disp carry
1 / T from the quotient.  The bound of a result is 2 (running error) + TINY.  It holds for any evaluation that rounds each
of these operations once in some order; torch's autograd takes more steps for the gradients than the closed form (each
reciprocal, square and power its own node), which the yardstick test measures rather than assumes.
The constants must be fp32 numbers for the truth and the device to mean the same operator (sigma0 = 0.5, the gammas);
eps = 1e-3 is none and enters with its rounding.
"""
import functools

import numpy as np
import torch

import _synth

U = 2.0 ** -24
TINY = 2.0 ** -126
#: the share of a case's elements whose decisions may be open (a condition on the draws, as in _ns_loss_ref)
MAY_DIFFER = 0.01
DEFAULTS = dict(sigma0=0.5, eps=1e-3, gammas=(1.0, 1.0, 1.0))
STATES = ("ds", "dm", "dw", "sg", "wt")
RESULTS = ("mu", "w", "sigma", "disp")
GRADS = ("gdelta", "gmu", "gsigma", "gw")


# ---- numbers with a running error ---------------------------------------------------------------------------------------------

def _exact32(c):
    return float(np.float32(c)) == float(c)


def _pow2(c):
    return c != 0 and np.frexp(abs(float(c)))[0] == 0.5


class E:
    """v: the float64 value; e: the absolute error an fp32 evaluation may have accumulated (first order)."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e

    @staticmethod
    def lift(x, like):
        if isinstance(x, E):
            return x
        c = float(x)
        return E(torch.full_like(like.v, c), torch.full_like(like.v, 0.0 if _exact32(c) else U * abs(c)))

    def _round(self, v, e):
        return E(v, e + U * v.abs())

    def __add__(self, o):
        o = E.lift(o, self)
        return self._round(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = E.lift(o, self)
        return self._round(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return E.lift(o, self) - self

    def __neg__(self):
        return E(-self.v, self.e)

    def __mul__(self, o):
        if not isinstance(o, E) and _pow2(o):
            return E(self.v * float(o), self.e * abs(float(o)))
        o = E.lift(o, self)
        return self._round(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        if not isinstance(o, E) and _pow2(o):
            return E(self.v / float(o), self.e / abs(float(o)))
        o = E.lift(o, self)
        v = self.v / o.v
        return self._round(v, self.e / o.v.abs() + v.abs() * o.e / o.v.abs())

    def __rtruediv__(self, o):
        return E.lift(o, self) / self

    def log(self):
        v = torch.log(self.v)
        return E(v, self.e / self.v.abs() + 2.0 * U * v.abs())

    def sum1(self):
        """The sum over the gaussians, kept as a (N,1,H,W) number."""
        m = self.v.shape[1]
        return E(self.v.sum(1, keepdim=True), self.e.sum(1, keepdim=True) + (m - 1) * U * self.v.abs().sum(1, keepdim=True))

    def where(self, cond):
        """The pass indicator: the number where cond, an exact 0 elsewhere."""
        return E(torch.where(cond, self.v, torch.zeros_like(self.v)), torch.where(cond, self.e, torch.zeros_like(self.e)))

    def bound(self):
        return 2.0 * self.e + TINY


def _clip(x, lo, hi, st):
    """(clipped number, decision, margin): st None takes float64's own decision (on an edge: inside)."""
    if st is None:
        st = torch.where(x.v < lo, 0, torch.where(x.v > hi, 2, 1))
    lo_e, hi_e = (0.0 if _exact32(c) else U * abs(c) for c in (lo, hi))
    v = torch.where(st == 0, torch.full_like(x.v, lo), torch.where(st == 2, torch.full_like(x.v, hi), x.v))
    e = torch.where(st == 0, torch.full_like(x.v, lo_e), torch.where(st == 2, torch.full_like(x.v, hi_e), x.e))
    margin = torch.minimum((x.v - lo).abs(), (x.v - hi).abs())
    return E(v, e), st, margin


def pack(st):
    return ((((st["ds"] * 3 + st["dm"]) * 3 + st["dw"]) * 3 + st["sg"]) * 3 + st["wt"]).to(torch.uint8)


def unpack(code):
    c = torch.as_tensor(np.array(code)).long()
    out = {}
    for name in reversed(STATES):
        out[name] = c % 3
        c = c // 3
    return out


# ---- the chain ----------------------------------------------------------------------------------------------------------------

#: mutant -> (the result whose bound it must miss, the case on which it must)
MUTANTS = {
    "no_inv_sigma_in_ds_dw": ("gw", "base"),
    "no_factor_3_in_ds_dsigma": ("gsigma", "base"),
    "gbeta_without_mean": ("gw", "uniform"),
    "dw_clip_ignored": ("gw", "base"),
    "gwt_without_sum": ("gw", "base"),
    "gdisp_not_in_gmu": ("gmu", "base"),
    "no_eps_in_log": ("w", "uniform"),
    "exclusive_edge": ("gw", "edge"),
}


def chain(a, consts=None, decisions=None, mutant=None, upstream=("gmu_out", "gw_out", "gsigma_out", "gdisp"), exact_wt=None):
    """Everything of one case in float64 with its running errors.  a: dict of arrays delta, mu, sigma, w and the upstream
    gradients gmu_out, gw_out, gsigma_out (N,M,H,W), gdisp (N,1,H,W); `upstream`: which of them are not zero.
    `exact_wt`: mask of the elements whose w~ decision is exact by construction (never open).
    Returns dict(value, bound) for mu, w, sigma, disp, gdelta, gmu, gsigma, gw, plus states, code, margins / open per clip."""
    k = dict(DEFAULTS, **(consts or {}))
    s0, eps = float(k["sigma0"]), float(k["eps"])
    g1, g2, g3 = (float(g) for g in k["gammas"])
    t = {n: E(torch.as_tensor(np.asarray(v)).double()) for n, v in a.items()}
    d, mu, s, w = t["delta"], t["mu"], t["sigma"], t["w"]
    M = d.v.shape[1]
    Mf = float(M)
    st_in = None if decisions is None else (decisions if isinstance(decisions, dict) else unpack(decisions))
    given = lambda n: None if st_in is None else st_in[n]                                                  # noqa: E731

    s0sq = E.lift(s0, d) * E.lift(s0, d)
    s2 = s * s
    s3 = s2 * s
    Ms2, Ms3 = Mf * s2, Mf * s3
    Mw = Mf * w
    ds_raw = (((1.0 - Mw) * s2 - s0sq - d * d) / Ms3 + (w * s) / s0sq) * 0.5
    dm_raw = (d * -0.5) * (1.0 / Ms2 + w / s0sq)
    mwe = Mw + eps
    s0M = E.lift(s0, d) * Mf
    u = (s0M * w) / s if mutant == "no_eps_in_log" else (s0M * w) / s + eps
    beta = ((-1.0 / mwe + u.log()) + (s2 + d * d) / (s0sq * 2.0) + 0.5) * 0.5
    dw_raw = beta - beta.sum1() / Mf

    states, margins, opened = {}, {}, {}

    def clip(name, x, lo, hi):
        y, states[name], margins[name] = _clip(x, lo, hi, given(name))
        opened[name] = margins[name] <= x.bound()
        inside = states[name] == 1
        if mutant == "exclusive_edge":
            inside = inside & (x.v != lo) & (x.v != hi)
        return y, inside

    ds, c_s = clip("ds", ds_raw * g1, -3.0, 3.0)
    dm, c_m = clip("dm", dm_raw * g2, -128.0, 128.0)
    wlim = 1.0 / (M * 4)
    dw, c_w = clip("dw", dw_raw * g3, -wlim, wlim)
    if mutant == "dw_clip_ignored":
        c_w = torch.ones_like(c_w)
    sn, c_S = clip("sg", s - ds, 0.1, 16.0)
    mun = mu - dm
    wt, c_W = clip("wt", w - dw, 0.0, 1.0)
    T = wt.sum1()
    wp = wt / T
    disp = (wp * mun).sum1()

    zero = E(torch.zeros_like(d.v))
    gmu_o, gw_o, gs_o = (t[n] if n in upstream else zero for n in ("gmu_out", "gw_out", "gsigma_out"))
    gdisp = t["gdisp"] if "gdisp" in upstream else E(torch.zeros_like(T.v))
    Gmu = gmu_o if mutant == "gdisp_not_in_gmu" else gmu_o + gdisp * wp
    Gw = gw_o + gdisp * mun
    Gwt = Gw / T if mutant == "gwt_without_sum" else (Gw - (Gw * wp).sum1()) / T
    A = Gwt.where(c_W)
    B = (-(A * g3)).where(c_w)
    gbeta = B if mutant == "gbeta_without_mean" else B - B.sum1() / Mf
    Eg = gs_o.where(c_S)
    g_ds = (-(Eg * g1)).where(c_s)
    g_dm = (-(Gmu * g2)).where(c_m)
    w_s0 = w / s0sq
    d_Ms3 = d / Ms3
    three = 1.0 if mutant == "no_factor_3_in_ds_dsigma" else 3.0
    gd = g_ds * -d_Ms3 + g_dm * ((1.0 / Ms2 + w_s0) * -0.5) + gbeta * (d / (s0sq * 2.0))
    gs = (Eg + g_ds * (((-(1.0 - Mw)) / Ms2 + ((s0sq + d * d) * three) / (Ms3 * s) + w_s0) * 0.5) + g_dm * d_Ms3
          + gbeta * (((-((s0M * w) / s2)) / u + s / s0sq) * 0.5))
    inv_s = zero if mutant == "no_inv_sigma_in_ds_dw" else -1.0 / s
    gw = (A + g_ds * ((inv_s + s / s0sq) * 0.5) + g_dm * ((d / s0sq) * -0.5)
          + gbeta * ((Mf / (mwe * mwe) + (s0M / s) / u) * 0.5))

    out = dict(value=dict(mu=mun.v, w=wp.v, sigma=sn.v, disp=disp.v, gdelta=gd.v, gmu=Gmu.v, gsigma=gs.v, gw=gw.v),
               bound=dict(mu=mun.bound(), w=wp.bound(), sigma=sn.bound(), disp=disp.bound(), gdelta=gd.bound(), gmu=Gmu.bound(),
                          gsigma=gs.bound(), gw=gw.bound()),
               states=states, code=pack(states), margins=margins, open=opened, wt=wt.v)
    if exact_wt is not None:
        opened["wt"] = opened["wt"] & ~torch.as_tensor(exact_wt)
    out["open_any"] = functools.reduce(torch.logical_or, opened.values()) & ~torch.isnan(wp.v)
    return out


def truth(a, consts=None, decisions=None, upstream=("gmu_out", "gw_out", "gsigma_out", "gdisp"), exact_wt=None):
    return chain(a, consts, decisions, None, upstream, exact_wt)


# ---- the torch restatement (any dtype) and its autograd -----------------------------------------------------------------------

def restated(delta, mu, sigma, w, sigma0=0.5, eps=1e-3, gammas=(1, 1, 1), regress=True, pre=None):
    """update.py:89-107 and model.py:154 operation for operation; `pre`, a dict, receives the five pre-clip values."""
    M = delta.shape[1]
    g1, g2, g3 = gammas
    delta_sigma = 0.5 * (((1 - M * w) * sigma ** 2 - sigma0 ** 2 - delta ** 2) / (M * sigma ** 3) + w * sigma / (sigma0 ** 2))
    delta_mu = -0.5 * delta * (1 / (M * sigma ** 2) + w / (sigma0 ** 2))
    beta = 0.5 * (-1 / (M * w + eps) + torch.log(sigma0 * M * w / sigma + eps) + (sigma ** 2 + delta ** 2) / (2 * sigma0 ** 2) + 0.5)
    delta_w = beta - torch.sum(beta, dim=1, keepdim=True) / M
    p = dict(ds=delta_sigma * g1, dm=delta_mu * g2, dw=delta_w * g3)
    delta_sigma = torch.clip(p["ds"], min=-3, max=3)
    delta_mu = torch.clip(p["dm"], min=-128, max=128)
    delta_w = torch.clip(p["dw"], min=-1 / (M * 4), max=1 / (M * 4))
    p["sg"], p["wt"] = sigma - delta_sigma, w - delta_w
    sigma = torch.clip(p["sg"], min=0.1, max=16)
    mu = mu - delta_mu
    w = torch.clip(p["wt"], min=0, max=1)
    w = w / torch.sum(w, dim=1, keepdim=True)
    if pre is not None:
        pre.update({n: v.detach() for n, v in p.items()})
    return mu, w, sigma, (torch.sum(w * mu, dim=1, keepdim=True) if regress else None)


def edges(M):
    return dict(ds=(-3.0, 3.0), dm=(-128.0, 128.0), dw=(-1 / (M * 4), 1 / (M * 4)), sg=(0.1, 16.0), wt=(0.0, 1.0))


def decisions_of(pre, M):
    """The byte a chain in the dtype of `pre` decided: the comparisons torch.clip makes, in that dtype."""
    st = {}
    for n, (lo, hi) in edges(M).items():
        x = pre[n]
        st[n] = torch.where(x < lo, 0, torch.where(x > hi, 2, 1))
    return pack(st)


def torch_chain(a, dtype, consts=None, device="cpu", fn=None, upstream=("gmu_out", "gw_out", "gsigma_out", "gdisp")):
    """dict(mu, w, sigma, disp, gdelta, gmu, gsigma, gw, code) of the restatement (or fn) under autograd in `dtype`."""
    k = dict(DEFAULTS, **(consts or {}))
    leaf = lambda n: torch.from_numpy(np.ascontiguousarray(a[n])).to(device=device, dtype=dtype).requires_grad_(True)  # noqa: E731
    ins = [leaf(n) for n in ("delta", "mu", "sigma", "w")]
    pre = {}
    if fn is None:
        outs = restated(*ins, k["sigma0"], k["eps"], k["gammas"], True, pre)
    else:
        outs = fn(*ins, sigma0=k["sigma0"], eps=k["eps"], gammas=k["gammas"], regress=True)
    loss = 0.0
    for o, n in zip(outs, ("gmu_out", "gw_out", "gsigma_out", "gdisp")):
        if n in upstream:
            loss = loss + (o * torch.from_numpy(np.ascontiguousarray(a[n])).to(device=device, dtype=dtype)).sum()
    grads = torch.autograd.grad(loss, ins, allow_unused=True)
    r = dict(zip(RESULTS, (o.detach() for o in outs)))
    r.update(zip(GRADS, (torch.zeros_like(ins[0]) if g is None else g for g in grads)))
    if pre:
        r["code"] = decisions_of(pre, ins[0].shape[1])
    return r


# ---- cases --------------------------------------------------------------------------------------------------------------------

def _case(seed, N, M, H, W, kind):
    return dict(seed=seed, N=N, M=M, H=H, W=W, kind=kind)


CASES = {
    "base":        _case(701, 1, 4, 6, 10, "model"),          # the ordinary path
    "uniform":     _case(702, 1, 4, 6, 10, "uniform"),        # the one regime where dw is not clipped
    "small_sigma": _case(703, 1, 4, 6, 10, "small_sigma"),    # ds at +-3, sigma' at both edges
    "big_delta":   _case(704, 1, 4, 6, 10, "big_delta"),      # dm at +-128
    "edge":        _case(705, 1, 4, 6, 10, "edge"),           # w~ = 0 exactly: the inclusive clamp gradient
    "m1":          _case(706, 2, 1, 5, 7, "model"),           # dw = 0 identically
    "m3":          _case(707, 1, 3, 5, 7, "model"),           # 1/M no power of two
    "m8":          _case(708, 1, 8, 5, 7, "model"),           # the maximum
    "odd":         _case(709, 2, 4, 17, 19, "model"),         # scalar walk, three blocks, a tail
    "vec":         _case(710, 1, 4, 8, 64, "model"),          # 16-byte path
    "zero":        _case(711, 1, 4, 6, 10, "zero"),           # all w = 0 at one pixel: NaN there only
}
GOLDEN_CASES = ("base", "uniform", "edge")
ZERO_PIXEL = (0, 2, 3)                                        # (n, h, w) of the case "zero"
EDGE_SIGMA, EDGE_W = 6.0, 0.0625


def _normalised(shape, seed, lo=0.05, hi=1.0):
    w = _synth.uniform(shape, lo, hi, seed, "w").astype(np.float64)
    return (w / w.sum(1, keepdims=True)).astype(np.float32)


def planted(c):
    """(N,H,W) index of the planted gaussian of each pixel of the case "edge"."""
    return _synth.rng(c["seed"], "planted").integers(0, c["M"], (c["N"], c["H"], c["W"]))


def inputs(c):
    """float32 numpy: delta, mu, sigma, w, gmu_out, gw_out, gsigma_out (N,M,H,W) and gdisp (N,1,H,W)."""
    shp = (c["N"], c["M"], c["H"], c["W"])
    pix = (c["N"], 1, c["H"], c["W"])
    seed, kind = c["seed"], c["kind"]
    delta = _synth.normal(shp, seed, "delta")
    sigma = _synth.uniform(shp, 0.5, 8.0, seed, "sigma")
    w = _normalised(shp, seed)
    mu = _synth.uniform(shp, 0.0, 48.0, seed, "mu")
    if kind == "uniform":
        j1 = _synth.rng(seed, "j1").integers(0, c["M"], pix)
        j2 = _synth.rng(seed, "j2").integers(0, c["M"], pix)
        jj = np.arange(c["M"]).reshape(1, -1, 1, 1)
        sigma = (_synth.uniform(pix, 0.4, 1.2, seed, "sigma") * np.where(jj == j1, 1.02, 1.0)).astype(np.float32)
        delta = (_synth.normal(pix, seed, "delta", scale=0.5) * np.where(jj == j2, 1.05, 1.0)).astype(np.float32)
        w = ((1.0 + _synth.uniform(shp, -0.02, 0.02, seed, "w")) / c["M"]).astype(np.float32)
    elif kind == "small_sigma":
        sigma = _synth.uniform(shp, 0.1, 0.6, seed, "sigma")
        # sigma' below 0.1 needs ds at +3 on a sigma under 3.1 (a heavy, wide gaussian); above 16 a sigma that is already there
        sigma[:, 0, :, 1::5], w[:, 0, :, 1::5], w[:, 1:, :, 1::5] = 2.5, 0.9, 0.1 / max(c["M"] - 1, 1)
        sigma[:, 1, :, 3::5], w[:, 1, :, 3::5] = 16.5, 0.01
    elif kind == "big_delta":
        delta = _synth.normal(shp, seed, "delta", scale=40.0)
        sigma = _synth.uniform(shp, 0.15, 0.4, seed, "sigma")
    elif kind == "edge":
        assert c["M"] == 4
        hit = np.arange(4).reshape(1, -1, 1, 1) == planted(c)[:, None]
        sigma = np.where(hit, np.float32(EDGE_SIGMA), _synth.uniform(shp, 0.45, 0.55, seed, "sigma")).astype(np.float32)
        w = np.where(hit, np.float32(EDGE_W), np.float32((1.0 - EDGE_W) / 3.0)).astype(np.float32)       # 0.0625, 0.3125: fp32 numbers
    elif kind == "zero":
        n, h, x = ZERO_PIXEL
        w[n, :, h, x] = 0.0
        sigma[n, :, h, x] = sigma[n, 0, h, x]         # equal beta there: dw_raw = 0 exactly (M = 4), so every w~ is 0
        delta[n, :, h, x] = delta[n, 0, h, x]
    a = dict(delta=delta, mu=mu, sigma=sigma, w=w)
    for n in ("gmu_out", "gw_out", "gsigma_out"):
        a[n] = _synth.normal(shp, seed, n)
    a["gdisp"] = _synth.normal(pix, seed, "gdisp")
    return a


def exact_wt(name):
    """The elements whose w~ decision is exact by construction, in any arithmetic, and so exempt from the cap: the planted
    gaussians of "edge" (dw saturates at 1/16, an fp32 number, and w is that number: w~ = 0, on the edge) and every element
    of an M = 1 case (dw = beta - beta / 1 = 0 and w = 1: w~ = 1, on the edge).  None for the other cases."""
    c = CASES[name]
    if c["kind"] == "edge":
        return np.arange(c["M"]).reshape(1, -1, 1, 1) == planted(c)[:, None]
    if c["M"] == 1:
        return np.ones((c["N"], 1, c["H"], c["W"]), bool)
    return None


@functools.lru_cache(maxsize=None)
def reference(name):
    """The inputs of a case and its float64 truth on float64's own decisions, computed once and shared."""
    a = inputs(CASES[name])
    return dict(a=a, truth=truth(a, exact_wt=exact_wt(name)))


@functools.lru_cache(maxsize=None)
def truth_on(name, code_bytes, upstream=("gmu_out", "gw_out", "gsigma_out", "gdisp")):
    """truth(decisions=) of a case for the decision bytes a device or a yardstick made (bytes: hashable)."""
    c = CASES[name]
    code = np.frombuffer(code_bytes, np.uint8).reshape(c["N"], c["M"], c["H"], c["W"])
    return truth(reference(name)["a"], decisions=code, upstream=upstream, exact_wt=exact_wt(name))


def off_nan_pixels(exact):
    """Mask of the elements to compare: everything but the pixels where the truth itself is NaN (the case "zero")."""
    return ~torch.isnan(exact)


def worst(got, exact, bound, mask=None):
    """max |got - exact| / bound over the (masked) elements; inf when got is not finite there."""
    got = torch.as_tensor(np.asarray(got.detach().cpu()) if isinstance(got, torch.Tensor) else got).double().reshape(exact.shape)
    mask = off_nan_pixels(exact) if mask is None else mask
    if not bool(torch.isfinite(got[mask]).all()):
        return float("inf")
    err = (got - exact).abs()[mask]
    return float((err / bound[mask]).max()) if err.numel() else 0.0


def code_agrees(code, t):
    """(every element that is not open carries the truth's byte, share of open elements)."""
    code = torch.as_tensor(np.asarray(code)).reshape(t["code"].shape)
    settled = ~t["open_any"] & ~torch.isnan(t["value"]["w"])
    return bool((code[settled] == t["code"][settled]).all()), float(t["open_any"].double().mean())


# ---- the three-iteration loop of model.py:120-174 -----------------------------------------------------------------------------

#: the gammas damp the update (powers of two, so the same operator in fp32 and float64): with 1, 1, 1 and an untrained head the
#: widths jump between the clip edges from the second iteration on and every decision of the third sits on an edge
LOOP = dict(seed=731, B=1, C=8, H=4, W=24, L=2, S=5, G=2, downsample=2, hidden=8, iters=3, gammas=(0.25, 0.5, 0.25))


def loop_inputs():
    """fmap1, fmap2 (B,C,H,W), the projections that stand for PCVNet's motion encoder and GRU (corr -> hidden state, hidden
    state -> up_mask; out of scope here), the real head's weights, and upstream gradients of the four up-sampled results."""
    c = LOOP
    f = 2 ** c["downsample"]
    ch = c["L"] * c["G"] * c["S"]
    seed = c["seed"]
    a = dict(zip(("fmap1", "fmap2"), _synth.fmap_pair(seed, c["B"], c["C"], c["H"], c["W"])))
    a["proj"] = _synth.normal((c["hidden"], ch), seed, "proj", scale=1.0 / ch ** 0.5)
    a["mask_proj"] = _synth.normal((9 * f * f, c["hidden"]), seed, "mask_proj", scale=1.0)
    a["head.conv1.weight"] = _synth.normal((c["hidden"], c["hidden"], 3, 3), seed, "c1w", scale=0.15)
    a["head.conv1.bias"] = _synth.normal((c["hidden"],), seed, "c1b", scale=0.1)
    a["head.conv2.weight"] = _synth.normal((c["G"], c["hidden"], 3, 3), seed, "c2w", scale=0.15)
    a["head.conv2.bias"] = _synth.normal((c["G"],), seed, "c2b", scale=0.1)
    fine = (c["iters"], c["B"], 1, f * c["H"], f * c["W"])
    fine_g = (c["iters"], c["B"] * c["G"], 1, f * c["H"], f * c["W"])
    a["g_disp"] = _synth.normal(fine, seed, "g_disp")
    for n in ("g_mu", "g_sigma", "g_w"):
        a[n] = _synth.normal(fine_g, seed, n)
    return a


def upsample4(disp, mu, sigma, w, up_mask, factor):
    """model.py:62-73 and :165-174 restated: the four convex_upsample calls with the repeated, detached mask."""
    import _upsample_ref
    N, G, H, W = mu.shape
    rep = up_mask.repeat(1, G, 1, 1).reshape(N * G, -1, H, W).detach()
    disp_up = _upsample_ref.sequence(disp, up_mask, factor)
    sigma_up = _upsample_ref.sequence(sigma.reshape(-1, 1, H, W), rep, factor)
    mu_up = _upsample_ref.sequence(mu.reshape(-1, 1, H, W), rep, factor)
    w_up = _upsample_ref.sequence(w.reshape(-1, 1, H, W) / factor, rep, factor)        # scale=False: the factor taken back, exactly
    return disp_up, mu_up, sigma_up, w_up


def loop(block, updater, upsample, t, watch=None):
    """Three iterations of model.py:120-174 (refinement aside): coords1 detached every iteration; mu, w, sigma detached into
    the updater (model.py:141) while sigma reaches the next lookup with its graph (:122).  block(f1, f2) -> corr_fn;
    updater(hidden, mu, sigma, w) -> (mu, w, sigma, disp); upsample(disp, mu, sigma, w, up_mask, factor) -> the four results.
    watch("lookup", i, coords1, sigma) sees every lookup's arguments; the updater is handed watch("update", i, ...) for its own.  Returns (loss, predictions)."""
    c = LOOP
    f = 2 ** c["downsample"]
    B, G, H, W = c["B"], c["G"], c["H"], c["W"]
    dt, dev = t["fmap1"].dtype, t["fmap1"].device
    coords0 = torch.arange(W, dtype=dt, device=dev).view(1, 1, 1, W).expand(B, G, H, W)
    start = torch.tensor([2.25, 9.25], dtype=dt, device=dev).view(1, G, 1, 1)
    coords1 = coords0 - start
    sigma = torch.full((B, G, H, W), 1.3125, dtype=dt, device=dev)
    w = torch.full((B, G, H, W), 1.0 / G, dtype=dt, device=dev)
    corr_fn = block(t["fmap1"], t["fmap2"])
    loss, preds = 0.0, []
    for i in range(c["iters"]):
        coords1 = coords1.detach()
        if watch is not None:
            watch("lookup", i, coords1, sigma)
        corr = corr_fn(coords1, sigma)
        mu = (coords0 - coords1).detach()
        hidden = torch.tanh(torch.einsum('kc,bchw->bkhw', t["proj"], corr))
        up_mask = 0.25 * torch.einsum('mk,bkhw->bmhw', t["mask_proj"], hidden)
        mu, w, sigma, disp = updater(hidden, mu.detach(), sigma.detach(), w.detach(), watch=None if watch is None else
                                     (lambda *args, i=i: watch("update", i, *args)))
        coords1 = coords0 - mu
        ups = upsample(disp, mu, sigma, w, up_mask, f)
        preds.extend(ups)
        for p, n in zip(ups, ("g_disp", "g_mu", "g_sigma", "g_w")):
            loss = loss + (p * t[n][i]).sum()
    return loss, preds


def restated_updater(t):
    """The reference-shaped module on torch ops (head: F.conv2d) in the dtype of `t`, with loop()'s updater signature."""
    import torch.nn.functional as F

    def updater(hidden, mu, sigma, w, watch=None):
        x = F.relu(F.conv2d(hidden, t["head.conv1.weight"], t["head.conv1.bias"], padding=1))
        delta = F.conv2d(x, t["head.conv2.weight"], t["head.conv2.bias"], padding=1)
        pre = {}
        out = restated(delta, mu, sigma, w, gammas=LOOP["gammas"], pre=pre)
        if watch is not None:
            watch(delta, mu, sigma, w, pre)
        return out
    return updater
