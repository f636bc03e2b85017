"""Float64 truth, fp32 yardstick, error bound and fixed cases for the update operator's training nodes
(dkt_stereo_amd/gru_train.py: gate_zr, gate_out, pool2x, interp).  Test infrastructure.

The functions (core/update.py:23-32, :87-96), per node, every node's inputs taken as exact fp32 numbers:

    gate_zr   X = azr[:, :Ch] + cz, Xr = azr[:, Ch:] + cr, z = sigmoid(X), r = sigmoid(Xr), rh = r h
              gazr = [gz z (1 - z) | grh h r (1 - r)],  gh = grh r
    gate_out  q = tanh(aq + cq),  h' = (1 - z) h + z q
              gaq = g z (1 - q^2),  gz = g (q - h),  gh = g (1 - z)
    pool2x    y[oy, ox] = (sum of the 3 x 3 window at (2 oy - 1, 2 ox - 1), zero padded) / 9
              gx[iy, ix] = sum gy[oy, ox] / 9 over |2 oy - iy| <= 1, |2 ox - ix| <= 1
    interp    y[oy, ox] = ly0 (lx0 v00 + lx1 v01) + ly1 (lx0 v10 + lx1 v11) with the forward's own fp32 weights:
              fy = fl(sy oy), y0 = (int)fy, y1 = y0 + (y0 < H - 1), ly1 = fl(fy - y0), ly0 = fl(1 - ly1), sy = fl((H-1)/(Ho-1))
              gx[iy, ix] = sum gy[oy, ox] wy wx, row oy giving ly0 to y0 and ly1 to y1 (columns alike)
The truth of the resamplers' gradients uses those fp32 weights: a node differentiates the function its forward computes.

The bound:  |got - exact| <= 2 c u mag + 2^-126,  u = 2^-24.  To first order in u; the factor 2 covers the higher orders and
what is named below as absorbed.  E_s and E_t are the errors of the sigmoid and tanh implementations relative to their
fp32 argument in units of u (relative to the true value); they cannot be derived, see E_SIGMA / E_T.

  z.  The argument X^ = fl(a + c) is off by |X| u, which sigmoid turns into |X| u z (1 - z); the function adds E_s u z:
        c mag = (E_s + |X| (1 - z)) z                                   =: e_z z
  rh.  One more product:  (e_r + 1) r |h|.
  h'.  fl(1 - z) is within u (1 - z), its product with h adds u, the final sum adds u |h'| <= u ((1 - z)|h| + z |q|):
       3 (1 - z) |h|.  q^ is within (E_t + 1) u |q| (the argument rounding costs |X| (1 - q^2) u <= u |q|, as x / sinh x cosh x <= 1),
       the product z q^ adds u, the sum u:   c mag = 3 (1 - z) |h| + (E_t + 3) z |q|.
  gaq = fl(fl(g z) fl(1 - fl(q^ q^))).  q^ q^ is within (2 (E_t + 1) + 1) u q^2, the difference adds u (1 - q^2), so the second
       factor is off by at most (2 E_t + 3) u in absolute terms (q^2 <= 1) -- the table's 2 E_t + 1 with the argument rounding
       absorbed --, the two products add 2 u (1 - q^2):   c mag = (2 E_t + 3) |g| z.
  gz (gate_out) = fl(g fl(q^ - h)):  (E_t + 1) u |q| from q^, u |q - h| from the difference, u |q - h| from the product:
       c mag = |g| ((E_t + 1) |q| + 2 |q - h|).
  gh (gate_out) = fl(g fl(1 - z)):  2 |g| (1 - z).
  gazr, z half = fl(fl(gz z^) fl(1 - z^)).  z^ (1 - z^) is off by |1 - 2 z| e_z u z <= e_z u z, fl(1 - z^) adds u, two products:
       c mag = (e_z + 3) |g| z.
  gazr, r half = fl(fl(fl(grh h) r^) fl(1 - r^)):  one more product:  (e_r + 4) |g| |h| r.
  gh (gate_zr) = fl(grh r^):  (e_r + 1) |g| r.
  pool2x backward.  n <= 4 terms fl(g / 9), one rounding each, and n - 1 additions of partial sums no larger than
       S = sum |g| / 9:   c mag = (n + 1) S   (n would do; the issue's n + 1 is kept).
  interp backward.  The weights are exact inputs.  A term fl(fl(wy wx) g) carries two roundings, the n - 1 additions at most
       (n - 1) u S with S = sum |wy wx g|:  n + 1; the issue's n + 3 leaves room for another association such as (wy g) wx:
       c mag = (n + 3) S,  n the number of contributing (output, tap) pairs.
  The floor 2^-126 covers gates that underflow: near |X| = 88 and beyond, fp32 returns 0 or a denormal where float64 does not.

E_s, E_t.  torch's CPU functions measured against float64 on the 4 000 001 points linspace(-30, 30): sigmoid 2.46 ulp,
tanh 0.57 ulp, i.e. at most 4.9 u and 1.2 u relative (1 ulp of the result is at most 2 u of it; test_host_gru_ref.py
reproduces both).  The budget for the device kernels is
the larger of twice those figures and the device functions' worst error over the same sweep plus one ulp (2 u: the sweep
is finite); the device figures come from `tools/bench_gru_train.py --sweep` on an MI355X."""
import numpy as np
import torch
import torch.nn.functional as F

import _synth

U = 2.0 ** -24
FLOOR = 2.0 ** -126

#: the reference's budget (torch CPU, rounded up): what the fp32 yardstick is held to
E_SIGMA_REF = 5.0
E_T_REF = 1.2
#: the sweep figures, torch CPU against float64, in ulp of the result and as relative error in u
SWEEP_POINTS, SWEEP_RANGE = 4000001, 30.0
SIGMOID_CPU_ULP, TANH_CPU_ULP = 2.46, 0.57
SIGMOID_CPU_U, TANH_CPU_U = 4.9, 1.2
#: the same sweep through dkt_sigmoid and tanhf on an MI355X (tools/bench_gru_train.py --sweep), in ulp of the result
SIGMOID_DEVICE_ULP = 2.623                                  # at x = -16.678
TANH_DEVICE_ULP = 1.33                                      # at x = -0.644
#: the device budget in u (1 ulp <= 2 u relative): max(2 * CPU figure, device figure + one ulp)
E_SIGMA = max(2 * SIGMOID_CPU_U, 2 * (SIGMOID_DEVICE_ULP + 1.0))        # 9.8 (the CPU branch)
E_T = max(2 * TANH_CPU_U, 2 * (TANH_DEVICE_ULP + 1.0))                  # 4.66 (the device branch)


# ---- fixed cases -----------------------------------------------------------------------------------------------------
def _gate(seed, B, Ch, H, W, scale):
    return dict(seed=seed, B=B, Ch=Ch, H=H, W=W, scale=scale)


#: scale: standard deviation of the pre-activations; "sat": pre-activations of +-30 and +-100
GATE_CASES = {
    "one": _gate(301, 1, 1, 1, 1, 1.0),
    "odd_s1": _gate(302, 3, 5, 3, 7, 1.0),                  # Ch * HW = 105: the scalar path
    "odd_s4": _gate(303, 3, 5, 3, 7, 4.0),
    "odd_s12": _gate(304, 3, 5, 3, 7, 12.0),
    "mid_s1": _gate(305, 2, 128, 16, 24, 1.0),
    "mid_s4": _gate(306, 2, 128, 16, 24, 4.0),
    "mid_s12": _gate(307, 2, 128, 16, 24, 12.0),
    "big_s4": _gate(308, 2, 128, 96, 96, 4.0),              # 589 824 float4 items > 2048 * 256: the grid-stride loop iterates
    "odd_sat": _gate(309, 3, 5, 3, 7, "sat"),
    "mid_sat": _gate(310, 2, 128, 16, 24, "sat"),
}

POOL_PLANES = 3
POOL_CASES = [(1, 1), (1, 2), (2, 1), (3, 3), (4, 6), (7, 10), (15, 28), (5, 600)]

#: (H, W, Ho, Wo, planes)
INTERP_CASES = [(1, 1, 1, 1, 3), (1, 5, 1, 9, 3), (4, 6, 8, 12, 3), (8, 12, 15, 23, 3), (5, 7, 5, 7, 3), (9, 11, 4, 5, 3),
                (3, 4, 1, 8, 3), (1, 300, 1, 600, 3), (30, 56, 60, 112, 256)]


def gate_inputs(c):
    """float32 numpy: azr, cz, cr, h, gz, grh (gate_zr) and aq, cq, z, gout (gate_out; its z is an input of its own)."""
    B, Ch, H, W, s = c["B"], c["Ch"], c["H"], c["W"], c["scale"]
    shp = (B, Ch, H, W)
    n = lambda name, shape=shp, scale=1.0: _synth.normal(shape, c["seed"], name, scale=scale)
    if s == "sat":
        lv = np.array([-100.0, -30.0, 30.0, 100.0], np.float32)
        pick = lambda name, shape: lv[_synth.rng(c["seed"], name).integers(0, 4, shape)]
        azr, aq, zx = pick("azr", (B, 2 * Ch, H, W)), pick("aq", shp), pick("zx", shp).astype(np.float64)
        cz, cr, cq = n("cz"), n("cr"), n("cq")
    else:
        azr, aq = n("azr", (B, 2 * Ch, H, W), 0.8 * s), n("aq", shp, 0.8 * s)
        cz, cr, cq = n("cz", scale=0.6 * s), n("cr", scale=0.6 * s), n("cq", scale=0.6 * s)
        zx = n("zx", scale=s).astype(np.float64)
    z = (1.0 / (1.0 + np.exp(-zx))).astype(np.float32)
    z[z < FLOOR] = 0.0                                       # sigmoid(-100): an exact 0, as the fp32 gate gives
    h = np.tanh(n("h")).astype(np.float32)
    return dict(azr=azr, cz=cz, cr=cr, h=h, gz=n("gz"), grh=n("grh"), aq=aq, cq=cq, z=z, gout=n("gout"))


def pool_inputs(H, W, planes=POOL_PLANES):
    """x (1, planes, H, W), gy (1, planes, Ho, Wo)."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return _synth.normal((1, planes, H, W), 320, "pool_x", H, W), _synth.normal((1, planes, Ho, Wo), 320, "pool_g", H, W)


def interp_inputs(H, W, Ho, Wo, planes):
    return (_synth.normal((1, planes, H, W), 321, "interp_x", H, W, Ho, Wo),
            _synth.normal((1, planes, Ho, Wo), 321, "interp_g", H, W, Ho, Wo))


def _t(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


# ---- the reference's expression sequences (any dtype) and torch autograd through them ----------------------------------
def seq_gate_zr(azr, cz, cr, h):
    ch = h.shape[1]
    z = torch.sigmoid(azr[:, :ch] + cz)
    r = torch.sigmoid(azr[:, ch:] + cr)
    return z, r * h


def seq_gate_out(aq, cq, z, h):
    q = torch.tanh(aq + cq)
    return (1 - z) * h + z * q


def seq_pool(x):
    return F.avg_pool2d(x, 3, stride=2, padding=1)


def seq_interp(x, size):
    return F.interpolate(x, size, mode="bilinear", align_corners=True)


def autograd_gates(i, dtype):
    """dict of every output and gradient of the two gate nodes, torch CPU autograd in `dtype`."""
    azr, cz, cr, h = (_t(i[k], dtype).requires_grad_(True) for k in ("azr", "cz", "cr", "h"))
    z, rh = seq_gate_zr(azr, cz, cr, h)
    gazr, gcz, gcr, gh = torch.autograd.grad([z, rh], [azr, cz, cr, h], [_t(i["gz"], dtype), _t(i["grh"], dtype)])
    aq, cq, zi, h2 = (_t(i[k], dtype).requires_grad_(True) for k in ("aq", "cq", "z", "h"))
    out = seq_gate_out(aq, cq, zi, h2)
    gaq, gcq, gz, gh2 = torch.autograd.grad(out, [aq, cq, zi, h2], _t(i["gout"], dtype))
    return dict(z=z.detach(), rh=rh.detach(), gazr=gazr, gcz=gcz, gcr=gcr, gh_zr=gh,
                hout=out.detach(), gaq=gaq, gcq=gcq, gz=gz, gh_out=gh2)


def autograd_pool(x, gy, dtype):
    a = _t(x, dtype).requires_grad_(True)
    y = seq_pool(a)
    return y.detach(), torch.autograd.grad(y, a, _t(gy, dtype))[0]


def autograd_interp(x, gy, dtype):
    a = _t(x, dtype).requires_grad_(True)
    y = seq_interp(a, gy.shape[2:])
    return y.detach(), torch.autograd.grad(y, a, _t(gy, dtype))[0]


# ---- closed forms in float64 and the bound's magnitudes ----------------------------------------------------------------
def _sig(x):
    return 1.0 / (1.0 + torch.exp(-x))


def closed_gates(i, e_sigma, e_t):
    """(truth, cmag, mag): dicts over z, rh, gazr, gh_zr, hout, gaq, gz, gh_out.  truth: float64 closed forms; cmag: the
    c * mag of the bound with the given function budgets; mag: the magnitude alone (what 'u * mag' refers to)."""
    azr, cz, cr, h, gz, grh, aq, cq, z_in, g = (_t(i[k]) for k in ("azr", "cz", "cr", "h", "gz", "grh", "aq", "cq", "z", "gout"))
    ch = h.shape[1]
    X, Xr = azr[:, :ch] + cz, azr[:, ch:] + cr
    z, omz, r, omr = _sig(X), _sig(-X), _sig(Xr), _sig(-Xr)            # 1 - sigmoid(x) = sigmoid(-x): no cancellation
    ez, er = e_sigma + X.abs() * omz, e_sigma + Xr.abs() * omr
    ah = h.abs()
    truth = dict(z=z, rh=r * h, gazr=torch.cat([gz * z * omz, grh * h * r * omr], 1), gh_zr=grh * r)
    mag = dict(z=z, rh=r * ah, gazr=torch.cat([gz.abs() * z, grh.abs() * ah * r], 1), gh_zr=grh.abs() * r)
    cmag = dict(z=ez * z, rh=(er + 1) * r * ah,
                gazr=torch.cat([(ez + 3) * gz.abs() * z, (er + 4) * grh.abs() * ah * r], 1), gh_zr=(er + 1) * grh.abs() * r)
    Xq = aq + cq
    q, sech2 = torch.tanh(Xq), 1.0 / torch.cosh(Xq) ** 2
    zi, omzi, ag = z_in, 1.0 - z_in, g.abs()                           # z is an input here: 1 - z of an fp32 number is exact in float64
    truth.update(hout=omzi * h + zi * q, gaq=g * zi * sech2, gz=g * (q - h), gh_out=g * omzi)
    mag.update(hout=omzi * ah + zi * q.abs(), gaq=ag * zi, gz=ag * (q.abs() + (q - h).abs()), gh_out=ag * omzi)
    cmag.update(hout=3 * omzi * ah + (e_t + 3) * zi * q.abs(), gaq=(2 * e_t + 3) * ag * zi,
                gz=ag * ((e_t + 1) * q.abs() + 2 * (q - h).abs()), gh_out=2 * ag * omzi)
    return truth, cmag, mag


def closed_pool(gy, H, W):
    """(gx, cmag, mag) in float64 for gy (N, C, Ho, Wo)."""
    g = _t(gy)
    Ho, Wo = g.shape[2:]
    gx, mag, n = (torch.zeros(g.shape[:2] + (H, W), dtype=torch.float64) for _ in range(3))
    for dy in range(3):
        for dx in range(3):
            oy = [o for o in range(Ho) if 0 <= 2 * o - 1 + dy < H]
            ox = [o for o in range(Wo) if 0 <= 2 * o - 1 + dx < W]
            if not oy or not ox:
                continue
            iy, ix = [2 * o - 1 + dy for o in oy], [2 * o - 1 + dx for o in ox]
            sel = g[:, :, oy][:, :, :, ox] / 9.0
            gx[:, :, iy[0]:iy[-1] + 1:2, ix[0]:ix[-1] + 1:2] += sel
            mag[:, :, iy[0]:iy[-1] + 1:2, ix[0]:ix[-1] + 1:2] += sel.abs()
            n[:, :, iy[0]:iy[-1] + 1:2, ix[0]:ix[-1] + 1:2] += 1
    return gx, (n + 1) * mag, mag


def interp_axis(N, No, dtype=np.float32):
    """The forward's source indices and weights of one axis in `dtype` arithmetic: i0, i1 (int), l0, l1."""
    f = dtype
    s = f(N - 1) / f(No - 1) if No > 1 else f(0)
    src = (s * np.arange(No).astype(f)).astype(f)
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < N - 1)
    l1 = (src - i0.astype(f)).astype(f)
    l0 = (f(1) - l1).astype(f)
    return i0, i1, l0, l1


def interp_axis_onehot(N, No):
    """The (No, N) fp32 matrix F.interpolate itself applies along one axis: its response to the N one-hot columns (an
    N x 1 image per input row; every product has a factor 1 or 0, so nothing but the weights is rounded)."""
    eye = torch.eye(N, dtype=torch.float32).view(1, N, N, 1)
    return seq_interp(eye, (No, 1))[0, :, :, 0].t().contiguous()


def interp_axis_matrix32(N, No):
    """The same matrix from the restated weights: fl(l0 [i0 == i] + l1 [i1 == i])."""
    i0, i1, l0, l1 = interp_axis(N, No)
    M = np.zeros((No, N), np.float32)
    o = np.arange(No)
    M[o, i0] = l0
    M[o, i1] = (M[o, i1] + l1).astype(np.float32) * (i1 == i0) + l1 * (i1 != i0)
    return torch.from_numpy(M)


def _axis_matrix(N, No, dtype):
    """(No, N) float64 matrices: the weight each output gives each input, and the number of taps that do so."""
    i0, i1, l0, l1 = interp_axis(N, No, dtype)
    M, C = np.zeros((No, N)), np.zeros((No, N))
    o = np.arange(No)
    np.add.at(M, (o, i0), l0.astype(np.float64))
    np.add.at(M, (o, i1), l1.astype(np.float64))
    np.add.at(C, (o, i0), 1.0)
    np.add.at(C, (o, i1), 1.0)
    return torch.from_numpy(M), torch.from_numpy(C)


def closed_interp(gy, H, W, dtype=np.float32):
    """(gx, cmag, mag) in float64 for gy (N, C, Ho, Wo), the weights computed in `dtype` (float32: the forward's own)."""
    g = _t(gy)
    Ho, Wo = g.shape[2:]
    My, Cy = _axis_matrix(H, Ho, dtype)
    Mx, Cx = _axis_matrix(W, Wo, dtype)
    gx = torch.einsum("oi,ncop,pj->ncij", My, g, Mx)
    mag = torch.einsum("oi,ncop,pj->ncij", My.abs(), g.abs(), Mx.abs())
    n = torch.einsum("oi,pj->ij", Cy, Cx)[None, None]
    return gx, (n + 3) * mag, mag


# ---- comparison -------------------------------------------------------------------------------------------------------
def worst(got, exact, cmag, mag):
    """(largest error in units of u * mag, largest fraction of the bound 2 c u mag + 2^-126) over EVERY element."""
    d = (got.detach().double().cpu() - exact).abs()
    assert d.shape == exact.shape == cmag.shape
    if not bool(torch.isfinite(d).all()):
        return float("inf"), float("inf")
    of_bound = d / (2.0 * U * cmag + FLOOR)
    over = torch.clamp(d - FLOOR, min=0.0)
    in_u = torch.where(over > 0, over / (U * torch.where(mag > 0, mag, torch.ones_like(mag))), torch.zeros_like(d))
    in_u = torch.where((over > 0) & (mag == 0), torch.full_like(d, float("inf")), in_u)
    return float(in_u.max()), float(of_bound.max())


def same(a, b):
    """Bit-for-bit equality of two float32 tensors, NaNs compared by position."""
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int32), b[~nb].view(np.int32))


def sweep_points():
    """The 4 000 001 fp32 arguments of the E_s / E_t sweep."""
    return torch.linspace(-SWEEP_RANGE, SWEEP_RANGE, SWEEP_POINTS, dtype=torch.float64).float()


def sweep_error(x, sig32, tanh32):
    """Worst error of fp32 sigmoid / tanh values at the fp32 arguments x against float64: ((ulp, u) sigmoid, (ulp, u) tanh);
    ulp of the true result, u relative to it."""
    xd = x.double()
    out = []
    for got, true in ((sig32, 1.0 / (1.0 + torch.exp(-xd))), (tanh32, torch.tanh(xd))):
        d = (got.double().cpu() - true).abs()
        nz = true != 0
        ulp = torch.exp2(torch.floor(torch.log2(true.abs()[nz])) - 23)
        out.append((float((d[nz] / ulp).max()), float((d[nz] / (true.abs()[nz] * U)).max())))
    return out
