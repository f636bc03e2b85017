"""Float64 truth, fp32 yardstick, closed-form gradients, error bounds, fixed cases and mutants for PCVNet's sequence loss
(pcv_loss.hip, pcvnet_loss.py; test infrastructure in the layout of _pcv_update_ref.py).

Operator (meta_arch/pcvnet/loss.py:4-73).  n predictions of final_disp_i (B,1,H,W) and mu_i, w_i, sigma_i (B M,1,H,W),
disp_refine (B,1,H,W); per target k (gt (B,1,H,W), valid (B,H,W)):
    mask = (gt < max_disp) & (valid != 0) & (gt >= 0)      N = |mask|      an empty mask returns (0, four metrics) at once
    every mu_i, w_i, sigma_i, final_disp_i must be finite everywhere (AssertionError, in order i)
    loss = sum_{i<n} W_i (mean_mask |disp_i - gt| + mean_mask (sum_m |mu_i,m - gt| / M)) + 1.4 mean_mask smoothl1(refine - gt)
    with W = (0.4, 0.6, 0.8, 1, 1.2, 1.4): n > 6 raises IndexError at i = 6 (after prediction 6's assertions), n < 4 at the
    metrics (final_disp_preds[3]).  Metrics: EPE mean and the fractions < 1, < 3, < 5, > 1, > 2, > 5 (strict) of
    final_disp_preds[3] and of disp_refine.  The weights enter as fp32 numbers (a Python float times an fp32 tensor), so the
    operator's constants here are fl32(W_i) and fl32(1.4): the truth and a device then mean the same thing.
Gradients for upstream g_k (closed form), on the mask, 0 off it:
    gdisp_i = sum_k g_k W_i / N_k sgn(disp_i - gt_k)       gmu_i,m = sum_k g_k W_i / (N_k M) sgn(mu_i,m - gt_k)
    grefine = sum_k 1.4 g_k / N_k clamp(refine - gt_k, -1, 1)

What is exact.  The mask tests inputs; the sign and the metric thresholds test one correctly rounded fp32 subtraction
(x - y is > 0, < 0 or = 0 in fp32 exactly when it is in the reals, and |fl(x - y)| < c for an fp32 number c ... is compared
after the same single rounding by every fp32 evaluation).  So the mask, N_k, the twelve count metrics and the sign pattern of
every gradient of a device must EQUAL torch's fp32 restatement; there are no open decisions to cap.  The counts of the truth
itself are taken on the fp32-rounded difference for the same reason.

Bounds (u = 2^-24, first order; bound = 2 (running count) + TINY as in the other _*_ref.py).  The count is of the kernel's own
roundings; the fp64 sums of the partials add nothing at this order:
    |fl(p - gt)|                      1 rounding:  u |term|
    sum_m |fl(mu_m - gt)| / M         each term u, the M - 1 additions at most u (sum) each, the division u:  (M + 1) u |term|
    smooth-L1 term, z = |fl(r - gt)|  z < 1: 0.5 z z, the error of z twice and one product: 3 u |term|;  else z - 0.5: u z + u |term|
    a mean S / N rounded to fp32      the terms' count plus 1
    loss                              both = mean1 + mean2 (+ u |both|), W_i both (+ u |product|), the running sum (+ u |partial|)
                                      per prediction; the same three for 1.4 sl1
    EPE means                         2 u |mean|                       the twelve fractions: exact counts, one division: equal
    gdisp: fl(fl(g W) / N) sgn        2 u per target, + u |sum| when two targets meet:  2 or 3
    gmu:   the same / M               3 u per target, + u |sum|:  3 or 4
    grefine                           norm = fl(1 / N), gw = fl(1.4 g), then |x| > 1: norm gw (3 u);  else x = fl(r - gt) and two
                                      products more (5 u); + u |sum| when two targets meet:  up to 6
torch's own fp32 evaluation sums its means in fp32 (a cascade over up to a few thousand terms); the yardstick test measures it
against these bounds rather than assuming it.
"""
import functools

import numpy as np
import torch

import _synth

U = 2.0 ** -24
TINY = 2.0 ** -126
I_WEIGHTS = (0.4, 0.6, 0.8, 1, 1.2, 1.4)
W32 = tuple(float(np.float32(w)) for w in I_WEIGHTS)
RW32 = float(np.float32(1.4))
EPE_KEYS = ('epe', '1px', '3px', '5px', 'bad1', 'bad2', 'bad5')
METRIC_KEYS = EPE_KEYS + tuple(k + '_final' for k in EPE_KEYS)
COUNT_KEYS = tuple(k for k in METRIC_KEYS if not k.startswith('epe'))
EMPTY_METRICS = {'epe': 0., '1px': 1., '3px': 1., '5px': 1.}
UPSTREAM = (0.75, 1.25)                                   # fp32 numbers
TILE = 1024

MUTANTS = {
    # mutant -> (what it must miss, the case on which it must)
    "valid_ge_half": ("mask", "edges"),
    "le_max_disp": ("mask", "edges"),
    "dropped_gaussian": ("loss", "ord"),
    "no_inv_M": ("loss", "ord"),
    "metrics_from_last": ("epe", "ord"),
    "nonstrict_thresholds": ("counts", "ties"),
    "refine_weight_1": ("loss", "ord"),
    "lost_tile": ("N", "ragged"),
    "other_targets_N": ("gdisp", "pair2"),
    "sgn_zero_is_one": ("signs", "ties"),
}


# ---- the torch restatement (any dtype) -----------------------------------------------------------------------------------

def restated(refine, disps, mus, ws, sigmas, gt, valid, M, max_disp=512, check=True):
    """One call of the loss in the dtype of its arguments: (loss, metrics, mask).  Leaves its lists alone."""
    import torch.nn.functional as F
    mask = (gt < max_disp) & valid[:, None].bool() & (gt >= 0)
    if not bool(mask.any()):
        return 0, dict(EMPTY_METRICS), mask
    B, _, H, W = gt.shape
    sel = mask.view(-1)
    total = 0.0
    for i in range(len(mus)):
        for t in ((mus[i], ws[i], sigmas[i], disps[i]) if check else (mus[i], disps[i])):
            assert bool(torch.isfinite(t).all())
        first = (disps[i] - gt).abs()
        second = (mus[i].reshape(B, M, 1, H, W) - gt[:, None]).abs().mean(dim=1)
        total = total + W32[i] * (first.view(-1)[sel].mean() + second.view(-1)[sel].mean())
    total = total + RW32 * F.smooth_l1_loss(refine[mask], gt[mask])
    metrics = {}
    for tail, p in (('', disps[3]), ('_final', refine)):
        e = (p - gt).abs().view(-1)[sel]
        metrics['epe' + tail] = e.mean().item()
        for key, hit in (('1px', e < 1), ('3px', e < 3), ('5px', e < 5), ('bad1', e > 1), ('bad2', e > 2), ('bad5', e > 5)):
            metrics[key + tail] = hit.to(e.dtype).mean().item()
    return total, metrics, mask


def torch_run(a, dtype, device="cpu", check=True):
    """The restatement on every target of case inputs `a` under autograd in `dtype`, upstream UPSTREAM: dict(per target:
    loss, metrics, mask or the exception's class name; grads gdisp, gmu, grefine of sum_k g_k loss_k)."""
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(device=device, dtype=dtype)              # noqa: E731
    leaf = lambda v: t(v).requires_grad_(True)                                                         # noqa: E731
    refine, disps, mus = leaf(a["refine"]), [leaf(v) for v in a["disp"]], [leaf(v) for v in a["mu"]]
    ws, sigmas = [t(v) for v in a["w"]], [t(v) for v in a["sigma"]]
    out = dict(targets=[])
    total = None
    for k in range(len(a["gt"])):
        try:
            loss, metrics, mask = restated(refine, disps, mus, ws, sigmas, t(a["gt"][k]), t(a["valid"][k]), a["M"], check=check)
        except (AssertionError, IndexError) as e:
            out["targets"].append(dict(raises=type(e).__name__))
            continue
        out["targets"].append(dict(loss=loss, metrics=metrics, mask=mask, raises=None))
        if torch.is_tensor(loss):
            total = loss * UPSTREAM[k] if total is None else total + loss * UPSTREAM[k]
    leaves = [refine] + disps + mus
    if total is not None:
        grads = torch.autograd.grad(total, leaves, allow_unused=True)
        grads = [torch.zeros_like(l) if g is None else g for l, g in zip(leaves, grads)]
        n = len(disps)
        out.update(grefine=grads[0], gdisp=grads[1:1 + n], gmu=grads[1 + n:])
    return out


# ---- the float64 closed form with its running count -------------------------------------------------------------------------

def _f32(x):
    """The fp32 rounding of a float64 tensor, as float64 (for the decisions a single fp32 subtraction makes)."""
    return x.float().double()


def expected_exception(a, k=0):
    """The class name the reference's call on target k raises, or None: from the inputs alone."""
    gt, valid = (torch.from_numpy(np.asarray(a[n][k])) for n in ("gt", "valid"))
    mask = (gt < 512) & (valid[:, None] != 0) & (gt >= 0)
    if not bool(mask.any()):
        return None
    n = len(a["mu"])
    for i in range(min(n, 7)):
        if not all(np.isfinite(a[key][i]).all() for key in ("mu", "w", "sigma", "disp")):
            return "AssertionError"
    return "IndexError" if n > 6 or n < 4 else None


def truth(a, mutant=None):
    """Everything of one case in float64.  Returns dict(targets=[dict(mask, N, loss, loss_bound, metrics, metric_bounds)],
    gdisp, gmu, grefine: lists of (value, bound)) for upstream UPSTREAM; a target with an empty mask contributes no gradient
    and carries loss None."""
    d = lambda v: torch.from_numpy(np.asarray(v)).double()                                             # noqa: E731
    M, n = a["M"], len(a["mu"])
    refine, disps = d(a["refine"]), [d(v) for v in a["disp"]]
    B, _, H, W = refine.shape
    mus = [d(v).reshape(B, M, H, W) for v in a["mu"]]
    n_loss = min(n, 6)
    out = dict(targets=[])
    gdisp = [[torch.zeros(B, 1, H, W, dtype=torch.float64), torch.zeros(B, 1, H, W, dtype=torch.float64)] for _ in range(n)]
    gmu = [[torch.zeros(B, M, H, W, dtype=torch.float64), torch.zeros(B, M, H, W, dtype=torch.float64)] for _ in range(n)]
    gref = [torch.zeros(B, 1, H, W, dtype=torch.float64), torch.zeros(B, 1, H, W, dtype=torch.float64)]
    met = 0                                      # the targets that have contributed a gradient so far
    masks, counts = [], []
    for k in range(len(a["gt"])):
        gt, valid = d(a["gt"][k]), d(a["valid"][k])[:, None]
        vset = valid >= 0.5 if mutant == "valid_ge_half" else valid != 0          # NaN != 0 is True
        below = gt <= 512 if mutant == "le_max_disp" else gt < 512
        mask = below & vset & (gt >= 0)
        if mutant == "lost_tile":
            flat = mask.reshape(B, -1).clone()
            flat[:, TILE:] = False
            mask = flat.reshape(mask.shape)
        masks.append(mask)
        counts.append(float(mask.sum()))
    for k in range(len(a["gt"])):
        gt, mask, N = d(a["gt"][k]), masks[k], counts[k]
        tk = dict(mask=mask, N=N, loss=None)
        out["targets"].append(tk)
        if N == 0:
            continue
        Ng = counts[1 - k] if mutant == "other_targets_N" and len(counts) == 2 else N
        mean = lambda x: float(x[mask].sum()) / N                                                      # noqa: E731
        loss, err = 0.0, 0.0
        for i in range(n_loss):
            t1 = (disps[i] - gt).abs()
            tm = (mus[i] - gt).abs()
            if mutant == "dropped_gaussian":
                tm = tm[:, :M - 1] if M > 1 else tm * 0.0
            t2 = tm.sum(1, keepdim=True) / (1.0 if mutant == "no_inv_M" else M)
            m1, m2 = mean(t1), mean(t2)
            e = 2.0 * U * m1 + (M + 2.0) * U * m2
            both = m1 + m2
            e += U * abs(both)
            prod = W32[i] * both
            e = W32[i] * e + U * abs(prod)
            loss += prod
            err += e + U * abs(loss)
            # gradients
            q = UPSTREAM[k] * W32[i] / Ng
            one = 1.0 if mutant == "sgn_zero_is_one" else 0.0
            sg = lambda x: torch.where(x > 0, 1.0, torch.where(x < 0, -1.0, one)).double()              # noqa: E731
            v = torch.where(mask, q * sg(disps[i] - gt), 0.0)
            gdisp[i][0] = gdisp[i][0] + v
            gdisp[i][1] = gdisp[i][1] + 2.0 * U * v.abs() + (U * gdisp[i][0].abs() if met else 0.0)
            v = torch.where(mask, (q / M) * sg(mus[i] - gt), 0.0)
            gmu[i][0] = gmu[i][0] + v
            gmu[i][1] = gmu[i][1] + 3.0 * U * v.abs() + (U * gmu[i][0].abs() if met else 0.0)
        x = refine - gt
        z = x.abs()
        term = torch.where(z < 1, 0.5 * z * z, z - 0.5)
        term_e = torch.where(z < 1, 3.0 * U * term, U * z + U * term)
        sl1 = mean(term)
        e = float(term_e[mask].sum()) / N + U * abs(sl1)
        rw = 1.0 if mutant == "refine_weight_1" else RW32
        prod = rw * sl1
        e = rw * e + U * abs(prod)
        loss += prod
        err += e + U * abs(loss)
        tk["loss"], tk["loss_bound"] = loss, 2.0 * err + TINY
        inside = _f32(x).abs() <= 1                     # the branch one fp32 subtraction takes
        # (a NaN difference takes neither outer branch: the middle one hands the NaN on)
        v = torch.where(mask, (rw * UPSTREAM[k] / Ng) * torch.where(inside | torch.isnan(x), x, torch.sign(x)), 0.0)
        gref[0] = gref[0] + v
        gref[1] = gref[1] + torch.where(inside, 5.0, 3.0) * U * v.abs() + (U * gref[0].abs() if met else 0.0)
        met += 1
        # metrics
        metrics, mb = {}, {}
        src3 = disps[-1] if mutant == "metrics_from_last" else (disps[3] if n > 3 else None)
        for tail, p in (('', src3), ('_final', refine)):
            if p is None:
                continue
            ep = (p - gt).abs()[mask]
            e32 = _f32(p - gt).abs()[mask]
            metrics['epe' + tail] = float(ep.sum()) / N
            mb['epe' + tail] = 2.0 * (2.0 * U * metrics['epe' + tail]) + TINY
            lt = (lambda c: e32 <= c) if mutant == "nonstrict_thresholds" else (lambda c: e32 < c)
            gtt = (lambda c: e32 >= c) if mutant == "nonstrict_thresholds" else (lambda c: e32 > c)
            for key, hit in (('1px', lt(1)), ('3px', lt(3)), ('5px', lt(5)), ('bad1', gtt(1)), ('bad2', gtt(2)), ('bad5', gtt(5))):
                # the fraction as fp32 forms it: an exact count, one correctly rounded division
                metrics[key + tail] = float(np.float32(float(hit.sum())) / np.float32(N))
        tk["metrics"], tk["metric_bounds"] = metrics, mb
    bound = lambda p: (p[0], 2.0 * p[1] + TINY)                                                        # noqa: E731
    out.update(gdisp=[bound(p) for p in gdisp], gmu=[bound(p) for p in gmu], grefine=bound(gref))
    return out


def worst(got, exact, bound):
    """max |got - exact| / bound over the elements; inf when got is not finite where exact is."""
    got = torch.as_tensor(np.asarray(got.detach().cpu()) if isinstance(got, torch.Tensor) else got).double().reshape(exact.shape)
    keep = torch.isfinite(exact)
    if not bool(torch.isfinite(got[keep]).all()):
        return float("inf")
    err = (got - exact).abs()[keep]
    return float((err / bound[keep]).max()) if err.numel() else 0.0


def scalar_ratio(got, exact, bound):
    got = float(got)
    if np.isnan(exact):                         # (the case "nan_refine": the NaN must come through)
        return 0.0 if np.isnan(got) else float("inf")
    if not np.isfinite(got):
        return float("inf")
    return abs(got - exact) / bound


def compare(got, t, k_list=None):
    """The largest error / bound ratio of a run `got` (torch_run's layout; the device test builds the same) against truth
    `t`, over losses, the two EPE means and the three gradient families: dict(name -> ratio)."""
    r = {}
    for k, (g, tk) in enumerate(zip(got["targets"], t["targets"])):
        if tk["loss"] is None or g.get("raises"):
            continue
        r["loss%d" % k] = scalar_ratio(g["loss"], tk["loss"], tk["loss_bound"])
        for key in ("epe", "epe_final"):
            if key in tk["metrics"]:
                r["%s%d" % (key, k)] = scalar_ratio(g["metrics"][key], tk["metrics"][key], tk["metric_bounds"][key])
    if "gdisp" in got:
        r["gdisp"] = max(worst(g, v, b) for g, (v, b) in zip(got["gdisp"], t["gdisp"]))
        r["gmu"] = max(worst(g, v, b) for g, (v, b) in zip(got["gmu"], t["gmu"]))
        r["grefine"] = worst(got["grefine"], *t["grefine"])
    return r


def exact_facts(run):
    """What must be EQUAL between two fp32 evaluations: per target the mask, N and the twelve count metrics; the sign
    pattern of every gradient.  `run` in torch_run's layout."""
    facts = []
    for g in run["targets"]:
        if g.get("raises"):
            facts.append(g["raises"])
            continue
        mask = np.asarray(g["mask"].detach().cpu()).astype(bool)
        counts = tuple(float(np.float32(g["metrics"][key])) for key in COUNT_KEYS if key in g["metrics"])
        facts.append((mask.tobytes(), int(mask.sum()), counts))
    if "gdisp" in run:
        for x in [run["grefine"]] + list(run["gdisp"]) + list(run["gmu"]):
            facts.append(np.nan_to_num(np.sign(np.asarray(x.detach().cpu(), dtype=np.float64))).astype(np.int8).tobytes())
    return facts


def truth_facts(t, signs=True):
    """exact_facts of a truth."""
    facts = []
    for tk in t["targets"]:
        mask = tk["mask"].numpy()
        if tk["loss"] is None:
            facts.append((mask.tobytes(), 0, tuple(float(np.float32(EMPTY_METRICS[key])) for key in COUNT_KEYS if key in EMPTY_METRICS)))
        else:
            facts.append((mask.tobytes(), int(tk["N"]), tuple(float(np.float32(tk["metrics"][key])) for key in COUNT_KEYS
                                                               if key in tk["metrics"])))
    if signs:
        for v, _ in [t["grefine"]] + t["gdisp"] + t["gmu"]:
            facts.append(np.nan_to_num(np.sign(v.numpy())).astype(np.int8).tobytes())
    return facts


# ---- cases --------------------------------------------------------------------------------------------------------------------

def _case(seed, B, M, n, H, W, kind="model", K=1):
    return dict(seed=seed, B=B, M=M, n=n, H=H, W=W, kind=kind, K=K)


CASES = {
    "ord":           _case(801, 2, 4, 6, 8, 12),
    "n4":            _case(802, 1, 4, 4, 8, 12),
    "n5":            _case(803, 1, 4, 5, 8, 12),
    "m1":            _case(804, 2, 1, 6, 5, 7),
    "m3":            _case(805, 1, 3, 6, 5, 7),                     # 1/M no power of two
    "m8":            _case(806, 1, 8, 6, 5, 7),                     # the maximum
    "ragged":        _case(807, 1, 3, 6, 33, 37),                   # 1221 pixels: two tiles, a partial one, scalar path
    "vec":           _case(808, 2, 4, 6, 16, 80),                   # 1280 pixels: 16-byte path, two tiles
    "one":           _case(809, 2, 4, 6, 8, 12, "one"),             # a single mask pixel
    "empty":         _case(810, 2, 4, 6, 8, 12, "empty"),           # all valid == 0
    "edges":         _case(811, 1, 4, 6, 8, 12, "edges"),
    "ties":          _case(812, 1, 4, 6, 8, 12, "ties"),
    "big":           _case(813, 1, 4, 6, 8, 12, "big"),             # values in the hundreds
    "strided":       _case(814, 2, 4, 6, 8, 12, "strided"),         # (the device test lays the tensors out as views)
    "pair":          _case(815, 2, 4, 6, 8, 12, "pair", K=2),       # different masks, the second empty
    "pair2":         _case(816, 2, 4, 6, 8, 12, "pair2", K=2),      # different masks, both non-empty (for the 1/N mutant)
    "nan_mu":        _case(817, 1, 4, 6, 8, 12, "nan_mu"),
    "inf_w_offmask": _case(818, 1, 4, 6, 8, 12, "inf_w_offmask"),
    "nan_sigma":     _case(819, 1, 4, 6, 8, 12, "nan_sigma"),
    "inf_disp":      _case(820, 1, 4, 6, 8, 12, "inf_disp"),
    "nan_refine":    _case(821, 1, 4, 6, 8, 12, "nan_refine"),
    "n3":            _case(822, 1, 4, 3, 8, 12),
    "n7":            _case(823, 1, 4, 7, 8, 12),
    "n7_nan6":       _case(824, 1, 4, 7, 8, 12, "nan6"),
}
RAISING = {"nan_mu": "AssertionError", "inf_w_offmask": "AssertionError", "nan_sigma": "AssertionError",
           "inf_disp": "AssertionError", "n3": "IndexError", "n7": "IndexError", "n7_nan6": "AssertionError"}
VALUE_CASES = tuple(n for n in CASES if n not in RAISING)
GOLDEN_CASES = ("ord", "m3", "n4", "edges", "ties", "one", "empty", "nan_refine") + tuple(RAISING)
#: positions (h, w) of the case "edges": gt planted at 0, -0.0, 512, the float below 512, -1, NaN, +Inf (valid 1 there), and
#: valid planted at 0.3, -1, NaN (gt in range there); EDGE_IN says which of the ten are on the mask
EDGE_GT = (0.0, -0.0, 512.0, float(np.nextafter(np.float32(512), np.float32(0))), -1.0, float("nan"), float("inf"))
EDGE_VALID = (0.3, -1.0, float("nan"))
EDGE_IN = (True, True, False, True, False, False, False, True, True, True)
#: the offsets |p - gt| planted in "ties" for final_disp_preds[3] and disp_refine, from column 0 of rows 1 and 2
TIE_EPE = (0.0, 1.0, -1.0, 2.0, 3.0, -3.0, 5.0, -5.0)


def inputs(name):
    """float32 numpy of a case: gt [K x (B,1,H,W)], valid [K x (B,H,W)], refine (B,1,H,W), disp [n x (B,1,H,W)], mu, w, sigma
    [n x (B M,1,H,W)], M."""
    c = CASES[name]
    seed, B, M, n, H, W, kind = (c[k] for k in ("seed", "B", "M", "n", "H", "W", "kind"))
    pix, mix = (B, 1, H, W), (B * M, 1, H, W)
    lo, hi, noise = (100.0, 500.0, 30.0) if kind == "big" else (0.0, 60.0, 1.0)
    base = _synth.uniform(pix, lo, hi, seed, "gt")
    if kind == "ties":
        base = (np.round(base * 4) / 4).astype(np.float32)              # multiples of 1/4 below 64: base + 5 is exact
    rep = np.repeat(base.reshape(B, 1, H, W), M, axis=1).reshape(mix)
    a = dict(M=M)
    a["disp"] = [(base + _synth.normal(pix, seed, "disp%d" % i, scale=noise * (4.0 - 0.4 * i))).astype(np.float32) for i in range(n)]
    a["mu"] = [(rep + _synth.normal(mix, seed, "mu%d" % i, scale=noise * 4.0)).astype(np.float32) for i in range(n)]
    a["w"] = [_synth.uniform(mix, 0.05, 1.0, seed, "w%d" % i) for i in range(n)]
    a["sigma"] = [_synth.uniform(mix, 0.5, 4.0, seed, "sigma%d" % i) for i in range(n)]
    a["refine"] = (base + _synth.normal(pix, seed, "refine", scale=noise * 1.2)).astype(np.float32)
    gt = base.copy()
    gt[..., 0, 3] = 600.0                                               # out of range
    gt[..., 1, 4] = -2.5
    valid = (_synth.uniform((B, H, W), 0.0, 1.0, seed, "valid") < 0.8).astype(np.float32)
    valid[:, 2, 2] = 0.0
    gts, valids = [gt], [valid]
    if kind == "one":
        valid[:] = 0.0
        valid[B - 1, 3, 5] = 1.0
    elif kind == "empty":
        valid[:] = 0.0
    elif kind == "edges":
        valid[:, 5] = 1.0
        for x, v in enumerate(EDGE_GT):
            gt[0, 0, 5, x] = v
        for x, v in enumerate(EDGE_VALID):
            gt[0, 0, 5, len(EDGE_GT) + x] = base[0, 0, 5, len(EDGE_GT) + x]
            valid[0, 5, len(EDGE_GT) + x] = v
    elif kind == "ties":
        valid[:, 1:4] = 1.0
        gt[0, 0, 1:4] = base[0, 0, 1:4]
        for x, off in enumerate(TIE_EPE):
            a["disp"][3][0, 0, 1, x] = base[0, 0, 1, x] + np.float32(off)
            a["refine"][0, 0, 2, x] = base[0, 0, 2, x] + np.float32(off)
        for i in range(n):                                              # pred == gt exactly: sgn(0) = 0
            a["disp"][i][0, 0, 3, :4] = base[0, 0, 3, :4]
            a["mu"][i].reshape(B, M, H, W)[0, i % M, 3, :6] = base[0, 0, 3, :6]
    elif kind in ("pair", "pair2"):
        gt2 = (base + _synth.normal(pix, seed, "pl", scale=0.5)).astype(np.float32)
        gt2[..., 4, 1] = 700.0
        valid2 = np.zeros_like(valid) if kind == "pair" else (_synth.uniform((B, H, W), 0.0, 1.0, seed, "valid2") < 0.5).astype(np.float32)
        gts.append(gt2)
        valids.append(valid2)
    elif kind == "nan_mu":
        a["mu"][2][1, 0, 4, 4] = np.nan
    elif kind == "inf_w_offmask":
        a["w"][1][M - 1, 0, 2, 2] = np.inf                                # valid is 0 at (2, 2)
    elif kind == "nan_sigma":
        a["sigma"][0][0, 0, 6, 1] = np.nan
    elif kind == "inf_disp":
        a["disp"][4][0, 0, 7, 11] = -np.inf
    elif kind == "nan_refine":
        valid[0, 3, 3] = 1.0
        a["refine"][0, 0, 3, 3] = np.nan
    elif kind == "nan6":
        a["mu"][6][0, 0, 0, 0] = np.nan
    a["gt"], a["valid"] = gts, valids
    return a


@functools.lru_cache(maxsize=None)
def reference(name):
    """The inputs of a case, its float64 truth and its fp32 yardstick, computed once and shared."""
    a = inputs(name)
    return dict(a=a, truth=None if name in RAISING else truth(a), fp32=torch_run(a, torch.float32))


def expected_flags(a):
    """The flag word of a case: bit i set when mu_i, w_i, sigma_i or final_disp_i holds a NaN or an Inf anywhere."""
    return sum(1 << i for i in range(min(len(a["mu"]), 7))
               if not all(np.isfinite(a[key][i]).all() for key in ("mu", "w", "sigma", "disp")))


# ---- the three-iteration loop of _pcv_update_ref ending in this loss ------------------------------------------------------------

#: a pixel leaves the loop's mask when some plane the loss compares with gt comes closer to it than this in the float64 loop:
#: the fp32 loops' predictions are within 1e-4 of their scale of the float64 ones (test_host_pcv_update_ref.py), so every
#: sign and every smooth-L1 branch of the kept pixels is the float64 loop's
LOOP_MARGIN = 1e-2


def loop_results(preds, dtype=None):
    """The loss's `results` from _pcv_update_ref.loop's predictions [disp_up, mu_up, sigma_up, w_up] x iterations: the last
    iteration stands twice (the loss needs four predictions) and its disparity stands for disp_refine (refineNet is out of scope)."""
    its = [preds[i:i + 4] for i in range(0, len(preds), 4)]
    its.append(its[-1])
    return {"output_list": (its[-1][0], [p[0] for p in its], [p[1] for p in its], [p[3] for p in its], [p[2] for p in its])}


def loop_target(preds64, M, seed=761):
    """(gt, valid) as float32 numpy from the float64 loop's predictions: gt = the last disparity plus an offset of 0.05 .. 3 of
    either sign, valid = 0 on a fifth of the pixels and wherever a compared plane is within LOOP_MARGIN of gt (or the last
    disparity, which the metrics and the smooth-L1 see, of gt +- 1, 2, 3, 5)."""
    last = preds64[-4].detach()
    B, _, H, W = last.shape
    off = _synth.uniform((B, 1, H, W), 0.05, 3.0, seed, "off") * np.where(_synth.uniform((B, 1, H, W), 0, 1, seed, "sign") < 0.5, -1, 1)
    gt = (last.numpy() + off).astype(np.float32)
    g = torch.from_numpy(gt).double()
    valid = torch.from_numpy(_synth.uniform((B, H, W), 0.0, 1.0, seed, "valid") < 0.8)
    for i in range(0, len(preds64), 4):
        valid &= ((preds64[i].detach() - g).abs() > LOOP_MARGIN)[:, 0]
        valid &= ((preds64[i + 1].detach().reshape(B, M, H, W) - g).abs() > LOOP_MARGIN).all(1)
    for c in (1.0, 2.0, 3.0, 5.0):                 # the smooth-L1 branch and the metric thresholds of the last disparity
        valid &= (((last - g).abs() - c).abs() > LOOP_MARGIN)[:, 0]
    return gt, valid.float().numpy()
