"""Float64 truth, fp32 yardstick, decisions, error bounds, fixed cases and mutants for the NeRF-supervised loss
(ns_loss.hip; test infrastructure in the layout of _soft_argmin_ref.py).

Operator (meta_arch/nerf_stereo/loss.py, restated with torch's own grid_sample / avg_pool2d so that it runs in double; the
reference itself cannot: disp_warp builds its ones in fp32 and grid_sample refuses the mix).  With d a prediction (negative):

    conf' = conf (target < 0);  valid = (conf' > thr) & (|target| < max_flow)
    rec_v = mask_v * sample_v,  sample_v = grid_sample(view_v, x + s_v d, border), mask_v = grid_sample(1, ., zeros),
            s = +1 for the first view and -1 for the third, align_corners=False on norm_grid's (W-1, H-1) normalisation
    p(a, b) = 0.15 mean_c |a - b| + 0.85 mean_c clamp((1 - SSIM(b, a))/2, 0, 1)       (7 x 7, reflection padded)
    loss_warp = min(p12, p23),  loss_2 = min(p(centre, first), p(centre, third)),  automask = (loss_warp < loss_2) & valid
    photo = mean_automask loss_warp (1 - conf'),  disp = mean_valid |d - target| conf'
    loss = a_d sum_i w_i disp_i + a_p sum_i w_i photo_i

Truth: float64.  Yardstick: the same code in float32.  tests/golden/ns_loss.npz, written by the reference itself, pins the
restatement (test_host_ns_loss_ref.py).

Decisions.  The loss jumps with the automask and is kinked at the minimum.  truth(decisions=...) takes valid, automask and
the branch as given instead of deriving them; the device's loss and gradients are compared with the truth under the DEVICE's
decisions, and the device's decisions must equal the truth's wherever the truth's margin (|loss_warp - loss_2|, |p12 - p23|)
exceeds the sum of the two planes' bounds at that pixel.  The share of pixels that may differ is capped at MAY_DIFFER of a
case.  valid has no tolerance: conf' and the threshold are the same fp32 numbers on both sides.  The clamp never acts away
from rounding (|SSIM| <= 1 with C1, C2 > 0); |a - b| = 0 and integer sample positions have measure zero on these scenes, and
where the views are identical the automask is off.  None of those is forced.

Bounds (eps = 2^-23).  Per element, of the form bound = 8 max(|yardstick - truth|, floor):
  planes.  floor = the conditioning of the SSIM quotient from the truth's own parts.  sigma_x, sigma_y, sigma_xy are
  differences of 49-term means of products: each is off by at most e = 16 eps (E[x^2] + E[y^2]) / 2 (the sums at six
  standard deviations, the products and the subtraction).  SSIM = A1 A2 / (B1 B2) with A2 = 2 sigma_xy + C2 and
  B2 = sigma_x + sigma_y + C2 then moves by |SSIM| (2 e / |A2| + 2 e / B2) + 8 eps, and the plane by 0.85/2 of the channel
  mean of that, plus 0.15 * 4 eps for the L1 term.  The warp adds the local slope of the reconstruction times the rounding of
  px, delta = slope * 4 eps (|px| + 1): the floor carries mean_c delta for the L1 term, and for SSIM the window's rms of
  delta through |cov(delta, y)| <= rms(delta) sigma_y (twice that on A2, 2 rms(delta) sigma_x on B2, rms(delta) on a mean).
  gradients and the scalar.  The SSIM gradient is a sum of 49 x 3 cancelling terms; its rounding error is noise of the size
  of the yardstick's own, so floor = max(mean over the plane of |yardstick - truth|, 16 eps max|truth|).  The scalar loss:
  floor = 16 eps |truth|.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import _synth

EPS = 2.0 ** -23
MAY_DIFFER = 0.01
C1, C2 = 0.01 ** 2, 0.03 ** 2


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def texture(seed, u, v):
    """A smooth random texture, three channels in about [0.1, 0.9], at real coordinates u (x) and v (y) (numpy, broadcast)."""
    g = _synth.rng(seed, "texture")
    out = []
    for _ in range(3):
        acc = np.zeros(np.broadcast(u, v).shape)
        for k in range(6):
            fx, fy = g.uniform(0.15, 0.9), g.uniform(-0.5, 0.5)
            acc = acc + g.uniform(0.5, 1.0) * np.sin(fx * u + fy * v + g.uniform(0, 2 * np.pi))
        out.append(0.5 + 0.4 * acc / 4.0)
    return np.clip(np.stack(out, -3), 0.02, 0.98)


def _case(seed, B, H, W, n=2, dlo=3.0, dhi=9.0, **kw):
    return dict(seed=seed, B=B, H=H, W=W, n=n, dlo=float(dlo), dhi=float(dhi), **kw)


CASES = {
    "min4": _case(501, 1, 4, 4, dlo=0.3, dhi=1.2),              # the smallest the reflection pad allows (its automask is empty)
    "h4": _case(543, 1, 4, 12, dlo=2.0, dhi=3.0),              # the smallest height with a full automask: row 0 has a mirror at 6
    "h5w9": _case(502, 1, 5, 9, dlo=1.0, dhi=3.0),
    "b2": _case(503, 2, 12, 40, n=3),
    "odd": _case(504, 2, 17, 53),                              # odd, no multiple of the tile
    "seams": _case(505, 1, 20, 37, dlo=3.0, dhi=7.0),          # 2 x 3 tiles of 16 x 16: windows and warps cross seams
    "far": _case(506, 1, 9, 24, dlo=2.0, dhi=11.0),            # samples past both side borders, never both views at once
    "same": _case(507, 1, 12, 40, same=(10, 30)),              # columns 10..29: three identical views, automask off
    "static": _case(508, 1, 8, 12, static=True),               # identical views everywhere: empty automask, NaN
    "novalid": _case(509, 1, 6, 10, conf_hi=0.4),              # nothing above the threshold
    "n16": _case(510, 1, 12, 40, n=16),
    "views": _case(511, 2, 10, 18, n=2, views=True),           # predictions are [:, :1] of two-channel tensors
    "nophoto": _case(512, 2, 7, 13, n=3, alpha_photometric=0.0),
    "thr": _case(513, 1, 8, 15, conf_at=True),                 # conf at, just under and just over the threshold
    "maxflow": _case(514, 1, 8, 15, target_at=True, max_flow=6.0),   # targets at +-max_flow and around it
}


def inputs(c):
    """dict of float32 numpy arrays: preds (n, B, 1, H, W), target, conf (B, H, W), im0, im1, im2 (B, 3, H, W)."""
    B, H, W, n, seed = c["B"], c["H"], c["W"], c["n"], c["seed"]
    y = np.arange(H, dtype=np.float64)[None, :, None]
    x = np.arange(W, dtype=np.float64)[None, None, :]
    bb = np.arange(B, dtype=np.float64)[:, None, None]
    d = -(c["dlo"] + (c["dhi"] - c["dlo"]) * x / (W - 1) + 0.3 * np.sin(0.7 * y + bb)) + 0 * y      # (B, H, W), negative
    u, v = x + 40.0 * bb, y + 0 * x
    im1 = texture(seed, u + 0 * d, v + 0 * d)
    if c.get("static"):
        im0 = im2 = im1
    else:
        im0, im2 = texture(seed, u - d, v + 0 * d), texture(seed, u + d, v + 0 * d)
        if c.get("same"):
            lo, hi = c["same"]
            im0, im2 = im0.copy(), im2.copy()
            im0[..., lo:hi] = im1[..., lo:hi]
            im2[..., lo:hi] = im1[..., lo:hi]
    # (B, 3, H, W): texture() stacks the channels at axis -3
    g = _synth.rng(seed, "inputs")
    target = d + 0.2 * g.standard_normal(d.shape)
    conf = g.uniform(0.05, c.get("conf_hi", 0.95), d.shape)
    if c.get("conf_at"):
        conf[:, :, 0::3] = 0.5
        conf[:, :, 1::3] = np.nextafter(np.float32(0.5), np.float32(0))
        conf[:, :, 2::3] = np.nextafter(np.float32(0.5), np.float32(1))
    if c.get("target_at"):
        mf = c["max_flow"]
        target[:, 0::4, 0::2] = -mf
        target[:, 1::4, 0::2] = mf
        target[:, 2::4, 0::2] = np.nextafter(np.float32(-mf), np.float32(0))
        target[:, 3::4, 1::3] = 0.0
    preds = np.stack([d + (0.6 * (n - i) / n) * np.sin(0.9 * x + 0.5 * y + i) for i in range(n)])[:, :, None]
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(preds=f(preds), target=f(target), conf=f(conf), im0=f(im0), im1=f(im1), im2=f(im2))


def params(c):
    return dict(alpha_disp_loss=1.0, alpha_photometric=c.get("alpha_photometric", 0.1), conf_threshold=0.5,
                max_flow=c.get("max_flow", 512))


# ---- the operator ----------------------------------------------------------------------------------------------------------
MUTANTS = {                                 # mutant -> the case on which it must miss a bound
    "align_corners": "odd", "no_row_fraction": "odd", "no_mask": "far", "mask_detached": "far", "zero_pad": "odd",
    "window3": "odd", "no_49": "odd", "keep_loser": "odd", "swap_s": "odd", "conf_not_unc": "odd",
    "mean_over_valid": "odd", "loss2_warped": "same",
}


def weights(n):
    g = 0.9 ** (15 / (n - 1))
    return [g ** (n - i - 1) for i in range(n)]


def ssim(x, y, mutant=None):
    md = 1 if mutant == "window3" else 3
    k = 2 * md + 1
    if mutant == "zero_pad":
        x, y = F.pad(x, (md,) * 4), F.pad(y, (md,) * 4)
    else:
        x, y = F.pad(x, (md,) * 4, mode="reflect"), F.pad(y, (md,) * 4, mode="reflect")
    div = 1 if mutant == "no_49" else None
    pool = lambda t: F.avg_pool2d(t, k, 1, 0, divisor_override=div)
    mu_x, mu_y = pool(x), pool(y)
    sx, sy, sxy = pool(x * x) - mu_x ** 2, pool(y * y) - mu_y ** 2, pool(x * y) - mu_x * mu_y
    A1, A2, B1, B2 = 2 * mu_x * mu_y + C1, 2 * sxy + C2, mu_x ** 2 + mu_y ** 2 + C1, sx + sy + C2
    S = A1 * A2 / (B1 * B2)
    parts = dict(S=S, A1=A1, A2=A2, B1=B1, B2=B2, sx=sx, sy=sy, exx=pool(x * x), eyy=pool(y * y))
    return torch.clamp((1 - S) / 2, 0, 1), parts


def photometric(a, b, mutant=None):
    """photometric_loss(a, b): (B, H, W), and the SSIM parts."""
    dist, parts = ssim(b, a, mutant)
    return 0.15 * (a - b).abs().mean(1) + 0.85 * dist.mean(1), parts


def warp(im, disp, s, mutant=None):
    """(reconstruction = mask * sample, px) of disp_warp."""
    B, _, H, W = im.shape
    dt = im.dtype
    xs = torch.arange(W, dtype=dt, device=im.device).view(1, 1, W) + s * disp[:, 0]
    ys = torch.arange(H, dtype=dt, device=im.device).view(1, H, 1).expand(B, H, W)
    grid = torch.stack([2.0 * xs / (W - 1) - 1.0, 2.0 * ys / (H - 1) - 1.0], -1)
    if mutant == "no_row_fraction":
        grid = torch.stack([grid[..., 0], (2.0 * ys + 1.0) / H - 1.0], -1)
    ac = mutant == "align_corners"
    rec = F.grid_sample(im, grid, mode="bilinear", padding_mode="border", align_corners=ac)
    mask = F.grid_sample(torch.ones_like(im), grid, mode="bilinear", padding_mode="zeros", align_corners=ac)
    if mutant == "no_mask":
        mask = torch.ones_like(mask)
    if mutant == "mask_detached":
        mask = mask.detach()
    return mask * rec, (xs * W / (W - 1) - 0.5)


def planes(disp, im0, im1, im2, mutant=None):
    """dict: p12, p23, loss_2 (B, H, W) and what the bounds need."""
    s0, s2 = (-1.0, 1.0) if mutant == "swap_s" else (1.0, -1.0)
    r0, px0 = warp(im0, disp, s0, mutant)
    r2, px2 = warp(im2, disp, s2, mutant)
    p12, q12 = photometric(im1, r0, mutant)
    p23, q23 = photometric(im1, r2, mutant)
    if mutant == "loss2_warped":
        l2 = torch.minimum(p12, p23).detach() * 1.5
    else:
        l2 = torch.minimum(photometric(im1, im0, mutant)[0], photometric(im1, im2, mutant)[0])
    return dict(p12=p12, p23=p23, loss_2=l2, q12=q12, q23=q23, r0=r0, r2=r2, px0=px0, px2=px2)


def fold(target, conf, conf_threshold, max_flow):
    cf = conf * (target < 0).to(conf.dtype)
    valid = (cf > conf_threshold) & (torch.sqrt(target ** 2) < max_flow)
    return cf, valid


def trinocular(disp, im0, im1, im2, unc, valid, decisions=None, mutant=None):
    """(scalar, dict of planes and decisions) of trinocular_loss; decisions = dict(automask=, third=) forces them."""
    pl = planes(disp, im0, im1, im2, mutant)
    third = pl["p23"] < pl["p12"]
    if decisions is not None:
        third = decisions["third"]
    lw = torch.where(third, pl["p23"], pl["p12"])
    if mutant == "keep_loser":
        lw = 0.5 * (pl["p12"] + pl["p23"]) + (lw - 0.5 * (pl["p12"] + pl["p23"])).detach()
    am = (lw < pl["loss_2"]) & valid
    if decisions is not None:
        am = decisions["automask"]
    w = (1 - unc) if mutant == "conf_not_unc" else unc
    sel = valid if mutant == "mean_over_valid" else am
    pl.update(loss_warp=lw, automask=am, third=third)
    return (lw * w)[sel].mean(), pl


def ns(preds, target, conf, im0, im1, im2, alpha_disp_loss=1.0, alpha_photometric=0.1, conf_threshold=0.5, max_flow=512,
       decisions=None, mutant=None, w=None):
    """The loss on tensors of one dtype.  preds: list of (B, 1, H, W) (requires_grad for gradients).  decisions: None or a list
    (one per prediction) of dict(automask=, third=) bool (B, H, W).  Returns dict(loss, disp, photo, valid, per=[planes])."""
    n = len(preds)
    w = weights(n) if w is None else w
    cf, valid = fold(target, conf, conf_threshold, max_flow)
    disp_loss, photo_loss, per = 0.0, 0.0, []
    for i in range(n):
        disp_loss = disp_loss + w[i] * ((preds[i][:, 0] - target).abs() * cf)[valid].mean()
        if alpha_photometric != 0.0:
            t, pl = trinocular(preds[i], im0, im1, im2, 1 - cf, valid, None if decisions is None else decisions[i], mutant)
            photo_loss = photo_loss + w[i] * t
            per.append(pl)
        else:
            photo_loss = torch.zeros_like(disp_loss)
    loss = alpha_disp_loss * disp_loss + alpha_photometric * photo_loss
    epe = torch.sqrt((preds[-1][:, 0] - target) ** 2)[valid]
    metrics = {"epe": epe.mean().item(), "1px": (epe < 1).to(epe.dtype).mean().item(),
               "3px": (epe < 3).to(epe.dtype).mean().item(), "5px": (epe < 5).to(epe.dtype).mean().item()}
    return dict(loss=loss, disp=disp_loss, photo=photo_loss, valid=valid, per=per, metrics=metrics)


def run(name, dtype, decisions=None, mutant=None, up=1.7):
    """The case in `dtype` on the CPU: dict(loss (python float), grads [n x (B, 1, H, W)], valid, per, metrics)."""
    c = CASES[name]
    a = {k: torch.from_numpy(v).to(dtype) for k, v in inputs(c).items()}
    preds = [p.clone().requires_grad_(True) for p in a["preds"]]
    out = ns(preds, a["target"], a["conf"], a["im0"], a["im1"], a["im2"], decisions=decisions, mutant=mutant, **params(c))
    grads = torch.autograd.grad(up * out["loss"], preds, allow_unused=True)
    grads = [torch.zeros_like(p) if g is None else g for g, p in zip(grads, preds)]
    per = [{k: (v.detach() if torch.is_tensor(v) else v) for k, v in pl.items()} for pl in out["per"]]
    return dict(loss=float(out["loss"].detach()), grads=[g.detach() for g in grads], valid=out["valid"], per=per, metrics=out["metrics"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """What the tests share of one case, computed once: the float64 truth and the fp32 yardstick with their own decisions."""
    return dict(truth=run(name, torch.float64), yard=run(name, torch.float32), inputs=inputs(CASES[name]))


# ---- bounds ----------------------------------------------------------------------------------------------------------------
def _box(t):
    return F.avg_pool2d(F.pad(t, (3,) * 4, mode="reflect"), 7, 1, 0)


def plane_floor(pl, which):
    """The derived floor of p12 / p23 (module docstring) from the truth's planes `pl` (one prediction): (B, H, W)."""
    q, r, px = (pl["q12"], pl["r0"], pl["px0"]) if which == "p12" else (pl["q23"], pl["r2"], pl["px2"])
    e = 16.0 * EPS * (q["exx"] + q["eyy"]) / 2.0
    gain = q["A1"].abs() / (q["B1"] * q["B2"])                      # |SSIM / A2|, finite where A2 passes through 0
    d_ssim = 2.0 * e * (gain + q["S"].abs() / q["B2"]) + 8.0 * EPS
    # the local slope of the reconstruction along x, times the rounding of px (six roundings of values <= |px| + 1)
    slope = torch.zeros_like(r)
    slope[..., 1:-1] = torch.maximum((r[..., 2:] - r[..., 1:-1]).abs(), (r[..., 1:-1] - r[..., :-2]).abs())
    slope[..., 0], slope[..., -1] = (r[..., 1] - r[..., 0]).abs(), (r[..., -1] - r[..., -2]).abs()
    d_rec = slope * (4.0 * EPS * (px.abs() + 1.0))[:, None]
    # a perturbation delta of the window's pixels: |cov(delta, y)| <= rms(delta) sigma_y (Cauchy-Schwarz) moves A2 by twice
    # that, B2 by 2 rms(delta) sigma_x, the means by at most rms(delta)
    rms = _box(d_rec ** 2).sqrt()
    sig_x, sig_y = q["sx"].clamp(min=0).sqrt(), q["sy"].clamp(min=0).sqrt()
    d_warp = rms * (2.0 * sig_y * gain + 2.0 * sig_x * q["S"].abs() / q["B2"] + 4.0 * q["S"].abs() / q["B1"].sqrt())
    return 0.15 * (d_rec.mean(1) + 4.0 * EPS) + 0.425 * (d_ssim + d_warp).mean(1)


def plane_bounds(name, i=0):
    """dict p12, p23, loss_2, loss_warp -> (B, H, W) bounds of prediction i's planes."""
    ref = reference(name)
    t, y = ref["truth"]["per"][i], ref["yard"]["per"][i]
    out = {}
    for k in ("p12", "p23"):
        out[k] = 8.0 * torch.maximum((y[k].double() - t[k]).abs(), plane_floor(t, k))
    out["loss_2"] = 8.0 * torch.maximum((y["loss_2"].double() - t["loss_2"]).abs(), torch.minimum(plane_floor(t, "p12"), plane_floor(t, "p23")) +
                                        16.0 * EPS)
    out["loss_warp"] = torch.maximum(out["p12"], out["p23"])
    return out


def may_differ(name, i=0):
    """dict automask, third -> bool (B, H, W): pixels whose decision the truth's margin leaves open."""
    t = reference(name)["truth"]["per"][i]
    b = plane_bounds(name, i)
    third = (t["p12"] - t["p23"]).abs() <= b["p12"] + b["p23"]
    am = ((t["loss_warp"] - t["loss_2"]).abs() <= b["loss_warp"] + b["loss_2"]) | third
    return dict(automask=am & reference(name)["truth"]["valid"], third=third)


def grad_bound(yard, truth):
    """Per element of one prediction's gradient (module docstring)."""
    err = (yard.double() - truth).abs()
    floor = max(float(err.mean()), 16.0 * EPS * float(truth.abs().max()))
    return 8.0 * torch.clamp(err, min=floor)


def loss_bound(yard, truth):
    if math.isnan(truth):
        return 0.0
    return 8.0 * max(abs(yard - truth), 16.0 * EPS * abs(truth))


def worst(got, exact, bound):
    """max |got - exact| / bound; inf when anything is not finite or a zero bound is missed."""
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


# ---- the closed form the kernel implements ---------------------------------------------------------------------------------
def ssim_grad_closed_form(x, y, gdist):
    """d sum(gdist * dist) / d x for dist = clamp((1 - SSIM(x, y))/2, 0, 1), by the gather of ns_loss.hip: per window centre q
    the coefficients (a_q, b_q, c_q) with d SSIM_q / d x_p = (a_q + 2 b_q x_p + c_q y_p) / 49, summed over the windows a
    pixel belongs to, reflection included.  x, y, gdist: (B, C, H, W) float64."""
    H, W = x.shape[-2:]
    pad = lambda t: F.pad(t, (3,) * 4, mode="reflect")
    pool = lambda t: F.avg_pool2d(pad(t), 7, 1, 0)
    mx, my = pool(x), pool(y)
    sx, sy, sxy = pool(x * x) - mx ** 2, pool(y * y) - my ** 2, pool(x * y) - mx * my
    A1, A2, B1, B2 = 2 * mx * my + C1, 2 * sxy + C2, mx ** 2 + my ** 2 + C1, sx + sy + C2
    D = B1 * B2
    S = A1 * A2 / D
    raw = (1 - S) / 2
    k = torch.where((raw >= 0) & (raw <= 1), -0.5 * gdist / 49.0, torch.zeros_like(gdist)) / D
    a = k * (2 * my * A2 - 2 * A1 * my - 2 * S * mx * B2 + 2 * S * B1 * mx)
    b = k * (-S * B1)
    c = k * (2 * A1)

    def gather(t):
        # box sum over the padded domain (windows centred in the image only), then fold the padding back by reflection
        full = F.avg_pool2d(F.pad(t, (6,) * 4), 7, 1, 0, divisor_override=1)          # (.., H + 6, W + 6)
        idx_y = torch.tensor([abs(i) if i < H else 2 * (H - 1) - i for i in range(-3, H + 3)])
        idx_x = torch.tensor([abs(i) if i < W else 2 * (W - 1) - i for i in range(-3, W + 3)])
        out = torch.zeros_like(t)
        tmp = torch.zeros(t.shape[:-2] + (H, W + 6), dtype=t.dtype)
        tmp.index_add_(-2, idx_y, full)
        out.index_add_(-1, idx_x, tmp)
        return out

    return gather(a) + 2 * gather(b) * x + gather(c) * y
