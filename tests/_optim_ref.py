"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

The fp64 truth of ONE optimizer step of tools/ft_dkt.py:243-246 (unscale, clip_grad_norm_, AdamW of :58, skip on overflow),
a CPU emulation of dkt_adamw_step's own rounding sequence (csrc/optim.hip), the derived bounds and the mutants
(test_host_optim_ref.py, test_gpu_optim.py).

Every comparison is of a single step from a stated fp32 state (p, g, m, v, step): two fp32 trajectories drift apart by about
an ulp of |p| per step, so trajectories are not compared.

truth()     in fp64, torch.optim.AdamW's own order of operations (test_host_optim_ref.py holds it to torch in fp64 at 1e-15):
                g'    = g * inv_scale * clip,  clip = min(1, max_norm / (total_norm + 1e-6)),  total_norm = |g * inv_scale|_2
                m'    = m + (1 - b1) (g' - m);   v' = v b2 + (1 - b2) g' g'
                p'    = p (1 - lr wd) - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps),   bc = 1 - b^t,  t = step + 1
            and nothing at all (p, m, v, step unchanged, skipped = 1) when an element of g is inf or nan.

The bounds.  eps32 = 2^-24 is the relative error of one fp32 rounding; the counts below are first-order worst cases of the
kernel's sequence, each rounding and each rounded constant counted once; b1 >= 0.75 is assumed.
  total_norm  the tile sums are fp64 (relative error 2^-53 * 2048 terms: nothing here); inv is one rounded constant, the
              product and conversion one rounding:                                   |dn| <= 2 eps32 * n          (N_NORM = 2)
  clip        total_norm 2, the sum with 1e-6 2 (its rounding, the constant), max_norm 1, the division 1:  6 when clip < 1
  g'          inv 1, g * inv 1, * clip 1, clip 6:                                                          9
  m'          d = g' - m: 10 |g'| + 1 |m|;  omb1 (a rounded constant) and the product: (1 - b1)(12 |g'| + 3 |m|);  the sum: 1 on
              |m'| <= M := b1 |m| + (1 - b1) |g'|;  3 (1 - b1) <= b1:               |dm| <= 13 eps32 * M          (B_M = 13)
              M is |m'| with the two terms added in magnitude: where they cancel, the error does not.
  v'          g'^2 18, omb2 and two products 3: 21 on that term;  b2 and its product 2 on the other; the sum 1:
                                                                                     |dv| <= 22 eps32 * v'         (B_V = 22)
  denom       sqrt halves 22 and rounds: 12;  sbc2 and the division: 14;  eps (a constant, <= 1 on the sum) and the sum: 15
  p'          u = step_size * (m' / denom): 13 (m') + 15 (denom) + 1 (division) + 2 (step_size, product) = 31 on
              D := (lr / bc1) M / denom;  p * decay: decay and the product, 2 |p|;  the difference: 1 on |p'| <= |p| + D:
                                                                             |dp| <= eps32 (3 |p| + 32 D)      (A_P = 3, B_P = 32)
  FLOOR = 2^-126, the smallest normal fp32: a result below it may be flushed.
D replaces |dp| = |p' - p (1 - lr wd)| of the form eps (a |p| + b |dp|) + floor by the same expression with the moment's two
terms added in magnitude, for the reason given at m'.

The cases (sizes: those of test_ema_kernel_bit_identical_to_torch -- empty tensors, exact tile multiples, tiles across
boundaries) are chosen so that every term is visible in one step; see CASES.  MUTANTS are wrong versions of the step; each
must leave the bound on at least one case.
"""
import functools
import math

import torch

EPS32 = 2.0 ** -24
N_NORM, B_M, B_V, A_P, B_P = 2, 13, 22, 3, 32
FLOOR = 2.0 ** -126
TILE = 2048
SIZES = [1, 0, 7, 1023, 2048, 4097, 3 * 2048 + 5, 100003, 0, 33]
BETAS = (0.9, 0.999)

#: name -> dict(lr, wd, eps, step, sigma (gradient magnitude before the loss scale), max_norm, inv_scale, warm (random m, v), poison)
CASES = {
    # the recipe's values from a fresh state; |g| = 0.34: clip = 1 exactly
    "recipe": dict(lr=2e-4, wd=1e-5, eps=1e-8, step=0, sigma=1e-3, max_norm=1.0),
    # at the recipe's values the decay term is 2e-9 |p|, below an ulp: here it is 1e-3 |p|
    "decay": dict(lr=1e-2, wd=1e-1, eps=1e-8, step=999, sigma=1e-3, max_norm=1.0, warm=True),
    # |g| ~ 1e-8 with v = 0: sqrt(v') / sqrt(bc2) ~ eps
    "eps": dict(lr=2e-4, wd=1e-5, eps=1e-8, step=0, sigma=1e-8, max_norm=1.0),
    # step 999 -> 1000: bc1 = 1, bc2 = 0.632
    "step1000": dict(lr=1e-3, wd=1e-5, eps=1e-8, step=999, sigma=1e-3, max_norm=1.0, warm=True),
    # |g| = 1e3: clip = 1e-3, with moments of the clipped magnitude so that the clip shows in m' and v'
    "clip": dict(lr=1e-2, wd=1e-1, eps=1e-8, step=999, sigma=1e3 / 339.66, max_norm=1.0, warm=True, warm_sigma=1e-3),
    # gradients scaled by 2^16, inv_scale 2^-16
    "scale": dict(lr=1e-3, wd=1e-5, eps=1e-8, step=999, sigma=1e-3, max_norm=1.0, inv_scale=2.0 ** -16, warm=True),
    # no clipping, no scale: the single-launch step
    "plain": dict(lr=1e-3, wd=1e-2, eps=1e-8, step=0, sigma=1e-3, max_norm=None),
    "plain1000": dict(lr=1e-3, wd=1e-2, eps=1e-8, step=999, sigma=1e-3, max_norm=None, warm=True),
    # one inf / one nan in the last element of the last non-empty tensor
    "inf": dict(lr=1e-2, wd=1e-1, eps=1e-8, step=999, sigma=1e-3, max_norm=1.0, warm=True, poison=math.inf),
    "nan": dict(lr=1e-2, wd=1e-1, eps=1e-8, step=0, sigma=1e-3, max_norm=1.0, poison=math.nan),
}
FINITE = [k for k, c in CASES.items() if "poison" not in c]
POISONED = [k for k, c in CASES.items() if "poison" in c]

MUTANTS = ("no_decay", "l2_decay", "no_bias_correction", "eps_in_sqrt", "clip_unclamped", "norm_tile_dropped",
           "boundary_dropped", "step_on_skip")


@functools.lru_cache(maxsize=None)
def state(name):
    """(p, g, m, v) lists of fp32 CPU tensors and the case's dict; computed once, never written (callers clone)."""
    c = dict(CASES[name])
    gen = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    scale = 1.0 / c.get("inv_scale", 1.0)
    ws = c.get("warm_sigma", c["sigma"])
    p = [torch.randn(n, generator=gen) * (k + 1) for k, n in enumerate(SIZES)]
    g = [torch.randn(n, generator=gen) * (c["sigma"] * scale) for n in SIZES]
    if c.get("warm"):
        m = [torch.randn(n, generator=gen) * (0.5 * ws) for n in SIZES]
        v = [torch.rand(n, generator=gen) * (ws * ws) for n in SIZES]
    else:
        m = [torch.zeros(n) for n in SIZES]
        v = [torch.zeros(n) for n in SIZES]
    if "poison" in c:
        last = max(k for k, n in enumerate(SIZES) if n)
        g[last][-1] = c["poison"]
    return p, g, m, v, c


def hyper(c):
    return dict(lr=c["lr"], betas=BETAS, eps=c["eps"], weight_decay=c["wd"])


def _flat(ts, dtype):
    return torch.cat([t.reshape(-1).to(dtype) for t in ts]) if ts else torch.zeros(0, dtype=dtype)


def truth(p, g, m, v, c):
    """dict(p, m, v: lists in fp64; total_norm, clip, skipped, step; M, D, denom: the bound's magnitudes per tensor)."""
    d = torch.float64
    p, g, m, v = ([t.to(d) for t in ts] for ts in (p, g, m, v))
    inv = c.get("inv_scale", 1.0)
    flat = _flat(g, d)
    tn = float(torch.sqrt((flat * flat).sum())) * inv
    finite = bool(torch.isfinite(flat).all())
    mx = c["max_norm"]
    clip = 1.0 if mx is None else min(1.0, mx / (tn + 1e-6))
    if not finite:
        return dict(p=p, m=m, v=v, total_norm=tn, clip=clip, skipped=1, step=c["step"], M=None, D=None)
    b1, b2 = BETAS
    t = c["step"] + 1
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    out = dict(p=[], m=[], v=[], M=[], D=[], total_norm=tn, clip=clip, skipped=0, step=t)
    for pk, gk, mk, vk in zip(p, g, m, v):
        g2 = gk * inv * clip
        mn = mk + (1 - b1) * (g2 - mk)
        vn = vk * b2 + (1 - b2) * g2 * g2
        denom = vn.sqrt() / math.sqrt(bc2) + c["eps"]
        pn = pk * (1 - c["lr"] * c["wd"]) + (-(c["lr"] / bc1)) * (mn / denom)
        M = b1 * mk.abs() + (1 - b1) * g2.abs()
        out["p"].append(pn)
        out["m"].append(mn)
        out["v"].append(vn)
        out["M"].append(M)
        out["D"].append((c["lr"] / bc1) * M / denom)
    return out


def bounds(p, t):
    """Per tensor (tol_p, tol_m, tol_v) of a finite step's truth `t` from the fp32 parameters `p` (module docstring)."""
    tp = [EPS32 * (A_P * pk.double().abs() + B_P * D) + FLOOR for pk, D in zip(p, t["D"])]
    tm = [EPS32 * B_M * M + FLOOR for M in t["M"]]
    tv = [EPS32 * B_V * vn + FLOOR for vn in t["v"]]
    return tp, tm, tv


def norm_tol(t):
    return N_NORM * EPS32 * abs(t["total_norm"]) + FLOOR


def excess(got, t, p0, m0, v0, step0):
    """How far a result dict(p, m, v, step[, total_norm]) is outside the bounds of the truth `t`: the largest
    |got - want| / tol over p, m, v and total_norm (<= 1: inside); inf when the step counter or a skipped step's bits differ."""
    if got["step"] != t["step"]:
        return math.inf
    worst = 0.0
    if t["skipped"]:
        for name, ref in (("p", p0), ("m", m0), ("v", v0)):
            for a, b in zip(got[name], ref):
                if not torch.equal(a.cpu(), b):
                    return math.inf
        return 0.0
    tols = dict(zip("pmv", bounds(p0, t)))
    for name in "pmv":
        for a, w, tol in zip(got[name], t[name], tols[name]):
            if a.numel():
                e = a.detach().cpu().double()
                if not bool(torch.isfinite(e).all()):
                    return math.inf
                worst = max(worst, float(((e - w).abs() / tol).max()))
    if got.get("total_norm") is not None:
        worst = max(worst, abs(float(got["total_norm"]) - t["total_norm"]) / norm_tol(t))
    return worst


def emulate(p, g, m, v, c, mutant=None):
    """The kernel's rounding sequence (csrc/optim.hip) in fp32 torch operations on the CPU, one rounding each; the tile sums
    and the finalise in fp64 as the kernel takes them.  Returns dict(p, m, v, step, total_norm, clip, skipped)."""
    f = torch.float32
    inv = torch.tensor(c.get("inv_scale", 1.0), dtype=f)
    flat = _flat(g, torch.float64)
    pad = (-flat.numel()) % TILE
    tiles = torch.cat([flat, torch.zeros(pad, dtype=torch.float64)]).reshape(-1, TILE)
    partial = (tiles * tiles).sum(1)
    if mutant == "norm_tile_dropped":
        partial = partial[:-1]
    bad = not bool(torch.isfinite(flat).all())
    full = c["max_norm"] is not None or c.get("inv_scale", 1.0) != 1.0
    tn = (partial.sum().sqrt() * inv.double()).to(f)
    clip = torch.tensor(1.0, dtype=f)
    if c["max_norm"] is not None:
        clip = torch.tensor(c["max_norm"], dtype=f) / (tn + torch.tensor(1e-6, dtype=f))
        if mutant != "clip_unclamped":
            clip = clip.clamp(max=1.0)
    step = c["step"]
    if bad:
        return dict(p=[t.clone() for t in p], m=[t.clone() for t in m], v=[t.clone() for t in v],
                    step=step + (mutant == "step_on_skip"), total_norm=float(tn), clip=float(clip), skipped=1)
    b1, b2 = BETAS
    t = step + 1
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    if mutant == "no_bias_correction":
        bc1 = bc2 = 1.0
    k = lambda x: torch.tensor(x, dtype=f)
    omb1, fb2, omb2, eps = k(1.0 - b1), k(b2), k(1.0 - b2), k(c["eps"])
    decay, sbc2, step_size = k(1.0 - c["lr"] * c["wd"]), k(math.sqrt(bc2)), k(c["lr"] / bc1)
    out = dict(p=[], m=[], v=[], step=t, total_norm=float(tn) if full else None, clip=float(clip), skipped=0)
    for pk, gk, mk, vk in zip(p, g, m, v):
        g2 = (gk * inv) * clip
        if mutant == "l2_decay":
            g2 = g2 + k(c["wd"]) * pk
        mn = mk + omb1 * (g2 - mk)
        vn = fb2 * vk + (omb2 * g2) * g2
        p1 = pk if mutant in ("no_decay", "l2_decay") else pk * decay
        if mutant == "eps_in_sqrt":
            denom = torch.sqrt(vn / (sbc2 * sbc2) + eps)
        else:
            denom = torch.sqrt(vn) / sbc2 + eps
        pn = p1 - step_size * (mn / denom)
        if mutant == "boundary_dropped" and pk.numel():
            pn[-1], mn[-1], vn[-1] = pk[-1], mk[-1], vk[-1]
        out["p"].append(pn)
        out["m"].append(mn)
        out["v"].append(vn)
    return out


def torch_step(p, g, m, v, c, dtype=torch.float32, optimizer=None, clip=None):
    """The reference sequence with torch.optim.AdamW in `dtype`: unscale, clip_grad_norm_, step (skipped on inf / nan as
    GradScaler.step skips it).  `clip`: a coefficient to multiply the gradients by instead of calling clip_grad_norm_.
    Returns dict(p, m, v, step, total_norm)."""
    ps = [torch.nn.Parameter(t.to(dtype).clone()) for t in p]
    for q, gk in zip(ps, g):
        q.grad = gk.to(dtype) * c.get("inv_scale", 1.0)
    opt = (optimizer or torch.optim.AdamW)(ps, **hyper(c))
    for q, mk, vk in zip(ps, m, v):
        opt.state[q] = dict(step=torch.tensor(float(c["step"])), exp_avg=mk.to(dtype).clone(), exp_avg_sq=vk.to(dtype).clone())
    finite = all(bool(torch.isfinite(q.grad).all()) for q in ps)
    tn = None
    if clip is not None:
        for q in ps:
            q.grad = q.grad * clip
    elif c["max_norm"] is not None:
        tn = float(torch.nn.utils.clip_grad_norm_(ps, c["max_norm"]))
    if finite:
        opt.step()
    return dict(p=[q.detach() for q in ps], m=[opt.state[q]["exp_avg"] for q in ps], v=[opt.state[q]["exp_avg_sq"] for q in ps],
                step=int(opt.state[ps[0]]["step"]), total_norm=tn)
