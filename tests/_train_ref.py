"""Plain restatements of the training-path operations, shared by test_gpu_dkt.py and test_gpu_train_random.py.

- F&E (FandE/__init__.py) and the RAFT sequence loss in fp32 torch, op for op in the reference's order, with the random
  draws passed in explicitly;
- the GwcNet loss in fp32 torch and both sequence losses in float64;
- the RAFT correlation lookup and the IGEV geometry lookup in float64, differentiable, with the sample positions rounded
  to fp32 the way the reference's grid_sample computes them (align_corners=True), so that a float64 autograd pass
  differs from the library's only by the fp32 roundings of the scatter, the pooling chain and the feature contraction.
"""
import torch
import torch.nn.functional as F

#: unit round-off of fp32
U32 = 2.0 ** -24


# ---- F&E ----------------------------------------------------------------------------------------------------------------
def consistent(s, t, tau):
    return (torch.sqrt((t - s) * (t - s)) < tau).float()


def torch_filter(s, t, v, tau, r=None):
    """FandE_Filter; `r` (B, 1) is the withprob draw, None for withprob=False.  Returns (source, valid (B,1,H,W))."""
    vc = consistent(s, t, tau) * v
    s = s * v
    if r is not None:
        ratio = vc.flatten(1).sum(-1) / v.flatten(1).sum(-1)
        sel = (r.reshape(-1).to(ratio.device) < ratio).float().reshape(-1, 1, 1, 1)
        vc = (vc + (1 - vc) * (sel * (1 - vc) * v)) * v
    return s * vc, vc


def torch_ensemble(s, t, v, tau, p, c):
    """FandE_Ensemble with the draw `p` of random.random()."""
    vc = consistent(s, t, tau) * v
    s, t = s * v, t * v
    off = p * torch.sqrt((s - t) * (s - t))
    if c:
        off = torch.clamp(off, max=c)
    d = (s < t).float() - (s > t).float()
    return (s + d * off * vc) * v


def torch_targets(disp_gt, valid_gt, disp_pl, disp_t, tau_gt, tau_pl, clamp, rand, p_gt, p_pl):
    """tools/ft_dkt.py:203-210 restated in torch with explicit draws."""
    gt_f, vgt = torch_filter(disp_gt, disp_t, valid_gt[:, None], tau_gt, rand)
    gt_aug = torch_ensemble(gt_f, disp_t, vgt, tau_gt, p_gt, clamp)
    pl_f, vpl = torch_filter(disp_pl, disp_t, torch.ones_like(disp_pl), tau_pl)
    pl_aug = torch_ensemble(pl_f, disp_t, vpl, tau_pl, p_pl, False)
    return gt_aug, vgt[:, 0], pl_aug, vpl[:, 0]


# ---- sequence losses ----------------------------------------------------------------------------------------------------
GWC_WEIGHTS = (0.5, 0.5, 0.7, 1.0)


def loss_mask(gt, valid, max_flow):
    return ((valid >= 0.5) & (torch.sqrt(gt[:, 0] * gt[:, 0]) < max_flow))[:, None]


def raft_weights(n, gamma=0.9):
    return [(gamma ** (15 / (n - 1))) ** (n - i - 1) for i in range(n)]


def torch_raft_loss(preds, gt, valid, gamma=0.9, max_flow=700):
    mask = loss_mask(gt, valid, max_flow)
    n = len(preds)
    total = 0.0
    for i, p in enumerate(preds):
        total = total + (gamma ** (15 / (n - 1))) ** (n - i - 1) * (p - gt).abs()[mask].mean()
    return total


def torch_gwc_loss(preds, gt, valid, maxdisp):
    mask = loss_mask(gt, valid, maxdisp)
    total = 0
    for p, w in zip(preds, GWC_WEIGHTS):
        total = total + w * F.smooth_l1_loss(p[mask], gt[mask], reduction="mean")
    return total


def loss64(kind, preds, gt, valid, max_flow):
    """Both losses in float64 from the fp32 inputs: (loss, sum_i |w_i * mean_i|).  kind 'raft' or 'gwc'."""
    mask = loss_mask(gt, valid, max_flow)
    g = gt.double()[mask]
    n = len(preds)
    ws = raft_weights(n) if kind == "raft" else GWC_WEIGHTS[:min(n, 4)]
    total, mag = 0.0, 0.0
    for p, w in zip(preds, ws):
        z = (p.double()[mask] - g).abs()
        term = z if kind == "raft" else torch.where(z < 1, 0.5 * z * z, z - 0.5)
        m = float(term.mean()) if term.numel() else float("nan")
        total += w * m
        mag += abs(w * m)
    return total, mag


# ---- the samplers in float64 --------------------------------------------------------------------------------------------
def ix32(x, width):
    """grid_sample's pixel position of fp32 coordinate(s) `x` in a row of `width` (align_corners=True), in fp32 as the
    reference computes it: normalise 2x/(W-1) - 1, then unnormalise (g + 1) * (W-1)/2.  NaN for width 1 (0/0 or
    Inf * 0): such a tap samples nothing."""
    wm1 = torch.tensor(float(width - 1), dtype=torch.float32)
    xg = (2.0 * x) / wm1 - 1.0
    return (xg + 1.0) * (wm1 / 2.0)


def sample64(rows, ix, width):
    """rows (N, width) float64, ix (N, K) fp32 positions -> (N, K) float64: linear interpolation with zero padding."""
    fl = torch.floor(ix)
    w = (ix - fl).double()                  # exact: ix and its floor share the exponent range
    out = 0.0
    for off, wt in ((0, 1.0 - w), (1, w)):
        idx = fl + off
        ok = (idx >= 0) & (idx <= width - 1)
        j = torch.where(ok, idx, torch.zeros_like(idx)).long()
        out = out + torch.gather(rows, 1, j) * torch.where(ok, wt, torch.zeros_like(wt))
    return out


def pool64(rows, num_levels):
    """avg_pool2d([1, 2], stride [1, 2]) chain of (N, W) rows: num_levels levels."""
    pyr = [rows]
    for _ in range(num_levels - 1):
        pyr.append(F.avg_pool2d(pyr[-1][:, None, None], [1, 2], stride=[1, 2])[:, 0, 0])
    return pyr


def taps32(radius):
    return torch.arange(-radius, radius + 1, dtype=torch.float32).view(1, -1)


def corr_lookup64(f1, f2, x, num_levels, radius, divisor):
    """core/corr.py:111-146 in float64: f1 (B,C,H,W1), f2 (B,C,H,W2) float64, x (B,H,W1) fp32 -> (B, L*K, H, W1).
    `divisor` is the fp32 sqrt(C) of corr.py:156."""
    B, C, H, W1 = f1.shape
    W2 = f2.shape[3]
    vol = torch.einsum('bchw,bchv->bhwv', f1, f2).reshape(B * H * W1, W2) / divisor
    xc = x.reshape(-1, 1)
    outs = []
    for i, lvl in enumerate(pool64(vol, num_levels)):
        outs.append(sample64(lvl, ix32(taps32(radius) + xc / 2 ** i, W2 >> i), W2 >> i))
    return torch.cat(outs, 1).view(B, H, W1, -1).permute(0, 3, 1, 2)


def geo_lookup64(m1, m2, geo, disp, coords, num_levels, radius):
    """meta_arch/igev_stereo/geometry.py:7-58 in float64: m1, m2 (B,Cm,H,W2) and geo (B,C,D,H,W) float64; disp (B,1,H,W)
    and coords (B,H,W,1) fp32 -> (B, L*K*(C+1), H, W)."""
    B, C, D, H, W = geo.shape
    W2 = m2.shape[3]
    N = B * H * W
    init = torch.einsum('bchw,bchv->bhwv', m1, m2).reshape(N, W2)
    gp = pool64(geo.permute(0, 3, 4, 1, 2).reshape(N * C, D), num_levels)
    ip = pool64(init, num_levels)
    dn, cn = disp.reshape(N, 1), coords.reshape(N, 1)
    dx = taps32(radius)
    outs = []
    for i in range(num_levels):
        dl, cl = dn / 2 ** i, cn / 2 ** i
        xg = (dx + dl).repeat_interleave(C, 0)
        g = sample64(gp[i], ix32(xg, D >> i), D >> i).view(N, C * dx.shape[1])
        c0 = sample64(ip[i], ix32((cl - dl) + dx, W2 >> i), W2 >> i)
        outs += [g, c0]
    return torch.cat(outs, 1).view(B, H, W, -1).permute(0, 3, 1, 2)
