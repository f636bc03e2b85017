"""Float64 reference, fp32 yardstick, error bounds, fixed cases and mutants for IGEV's context up-sampling nodes (test
infrastructure; the layout of _upsample_ref.py).

Notation: disp (B, 1, h, w), a nine-plane tensor (B, 9, 4h, 4w), fine pixel (Y, X) over coarse pixel (y, x) = (Y/4, X/4),
nb_k = disp[b, 0, y + k/3 - 1, x + k%3 - 1] (0 outside), g the upstream gradient (B, 4h, 4w).

  weights form (context_upsample as written, meta_arch/igev_stereo/submodule.py:242-254):
    out = sum_k w_k nb_k,  gweights_k = g nb_k,  gdisp[y, x] = sum_k C_k[y - k/3 + 1, x - k%3 + 1],  C_k = sum_{i,j<4} w_k g
  logits form (the tail of upsample_disp, igev_stereo.py:145-147):
    p = softmax_k(logits), v_k = scale nb_k, out = sum_k p_k v_k,
    a_k = g v_k, s = sum_k p_k a_k, glogits_k = p_k (a_k - s),  gdisp = scale sum_k C_k[...], C_k = sum_{i,j<4} p_k g

The bounds |got - exact| <= 2 c u mag (u = 2^-24; every statement to first order in u, the factor 2 of the assertions
covers the rest), derived as in _upsample_ref.py with R = max_k - min_k of the nine logits of a fine pixel:

  softmax.  |p^_k - p_k| <= c_p u p_k, c_p = 2 R + 13 (argument of exp R u, expf 2 u, twice because the normalisation carries
  the same error; 8 additions; one division).
  out.  v_k is exact (scale is a power of two).  Nine products and 8 additions in any order:
      c_out = c_p + 9 = 2 R + 22,                       mag_out = sum_k p_k |v_k|.
  glogits.  a_k is one product, u A_k with A_k = |g| |v_k|.  s: products of p^_k and a^_k (c_p + 2) and 8 additions,
  (c_p + 10) u S with S = sum_k p_k A_k.  The subtraction rounds once, u (A_k + S); the last product brings
  (c_p + 1) u |a_k - s| <= (c_p + 1) u (A_k + S).  Together
      c_glogits = 2 c_p + 12 = 4 R + 38,                mag_glogits = p_k (A_k + S).
  gdisp, logits form.  At most 144 products p^ g (c_p + 1 each, with the largest R among the contributing fine pixels: the
  16 of each coarse pixel of the 3 x 3 neighbourhood) and 143 additions in any order; the factor scale is exact:
      c_gdisp = 2 R_max + 13 + 144,                      mag_gdisp = scale sum p |g|.
  weights form.  gweights is one product: it is compared bit for bit with the fp32 product.  gdisp: 144 products (u each)
  and 143 additions never exceed 144 u; the constant keeps one more u:
      c_gdisp = 145,                                     mag_gdisp = sum |w| |g|.

The magnitudes are the same float64 chain on |disp| and |g| with the true p.  The bounds are relative: they hold while no
softmax term underflows in fp32; WIDE_CASES is for bit-for-bit repeatability only."""
import torch
import torch.nn.functional as F

import _synth
from _upsample_ref import U, same, worst  # noqa: F401

SCALE = 4.0


def _case(seed, B, h, w, sigma=2.0):
    return dict(seed=seed, B=B, h=h, w=w, sigma=sigma)


CASES = {
    "one": _case(301, 1, 1, 1),
    "h1": _case(302, 2, 1, 11),
    "w1": _case(303, 1, 9, 1),
    "small": _case(304, 1, 5, 9),
    "tiles": _case(305, 1, 20, 70),                        # several blocks of 256 coarse pixels and a ragged edge
    "sigma0.5": _case(306, 2, 33, 70, sigma=0.5),
    "sigma8": _case(307, 1, 12, 40, sigma=8.0),
}

WIDE_CASES = {"sigma32": _case(308, 1, 12, 40, sigma=32.0)}

#: mutant -> the result whose bound it must miss (gnine: the gradient of the nine-plane tensor)
MUTANTS = {"drop_tap4": "out", "clamp_pad": "out", "swap_k": "out", "no_minus_s": "gnine", "scale_twice": "gdisp",
           "skip_sub33": "gdisp"}
MUTANT_CASES = ("small", "tiles")


def inputs(c):
    """disp (B, 1, h, w), logits (B, 9, 4h, 4w), gout (B, 4h, 4w): float32 numpy."""
    B, h, w = c["B"], c["h"], c["w"]
    disp = _synth.normal((B, 1, h, w), c["seed"], "disp", scale=5.0)
    logits = _synth.normal((B, 9, 4 * h, 4 * w), c["seed"], "logits", scale=c["sigma"])
    gout = _synth.normal((B, 4 * h, 4 * w), c["seed"], "gout")
    return disp, logits, gout


def weights_of(logits):
    """The weights form's second operand as the reference's caller makes it: torch's fp32 softmax of the logits (numpy in, out)."""
    return torch.softmax(torch.from_numpy(logits), 1).numpy()


def sequence(disp_low, up_weights):
    """The reference's expression sequence (meta_arch/igev_stereo/submodule.py:242-254), any dtype."""
    b, c, h, w = disp_low.shape
    disp_unfold = F.unfold(disp_low.reshape(b, c, h, w), 3, 1, 1).reshape(b, -1, h, w)
    disp_unfold = F.interpolate(disp_unfold, (h * 4, w * 4), mode="nearest").reshape(b, 9, h * 4, w * 4)
    return (disp_unfold * up_weights).sum(1)


def sequence_logits(disp, logits, scale=SCALE):
    """igev_stereo.py:145-146 in front of it."""
    return sequence(disp * scale, F.softmax(logits, 1))


def autograd(disp, nine, gout, dtype, logits):
    """(out, gdisp, gnine) of the sequence under torch autograd on the CPU in `dtype` (numpy in)."""
    a = torch.from_numpy(disp).to(dtype).requires_grad_(True)
    b = torch.from_numpy(nine).to(dtype).requires_grad_(True)
    out = sequence_logits(a, b) if logits else sequence(a, b)
    ga, gb = torch.autograd.grad(out, (a, b), torch.from_numpy(gout).to(dtype))
    return out.detach(), ga, gb


def truth(disp, nine, gout, logits):
    return autograd(disp, nine, gout, torch.float64, logits)


def yardstick(disp, nine, gout, logits):
    return autograd(disp, nine, gout, torch.float32, logits)


def neighbours(disp, mutant=None):
    """nb (B, 9, 4h, 4w) in the dtype of disp: every coarse pixel's nine neighbours, repeated over its 16 fine pixels."""
    B, _, h, w = disp.shape
    pad = F.pad(disp, (1, 1, 1, 1), mode="replicate" if mutant == "clamp_pad" else "constant")
    planes = []
    for k in range(9):
        dy, dx = (k % 3, k // 3) if mutant == "swap_k" else (k // 3, k % 3)
        t = pad[:, 0, dy:dy + h, dx:dx + w]
        planes.append(torch.zeros_like(t) if (mutant == "drop_tap4" and k == 4) else t)
    nb = torch.stack(planes, 1)
    return nb.repeat_interleave(4, 2).repeat_interleave(4, 3)


def _gather(C):
    """gdisp[y, x] = sum_k C[k, y - k/3 + 1, x - k%3 + 1] (the adjoint of neighbours), (B, 9, h, w) -> (B, 1, h, w)."""
    B, _, h, w = C.shape
    Cp = F.pad(C, (1, 1, 1, 1))
    out = torch.zeros((B, 1, h, w), dtype=C.dtype)
    for k in range(9):
        out[:, 0] += Cp[:, k, 2 - k // 3:2 - k // 3 + h, 2 - k % 3:2 - k % 3 + w]
    return out


def _blocks(t, mutant=None):
    """sum over the 4 x 4 fine pixels of every coarse pixel: (B, 9, 4h, 4w) -> (B, 9, h, w)."""
    B, K, H4, W4 = t.shape
    t = t.reshape(B, K, H4 // 4, 4, W4 // 4, 4)
    if mutant == "skip_sub33":
        t = t.clone()
        t[:, :, :, 3, :, 3] = 0
    return t.sum(dim=(3, 5))


def closed_form(disp, nine, gout, logits, scale=SCALE, mutant=None):
    """(out, gdisp, gnine) in float64 from the formulas of the module docstring (float32 or float64 torch tensors in)."""
    disp, nine, g = disp.double(), nine.double(), gout.double()[:, None]
    if not logits:
        nb = neighbours(disp, mutant)
        return (nine * nb).sum(1), _gather(_blocks(nine * g, mutant)), g * nb
    p = torch.softmax(nine, 1)
    v = scale * neighbours(disp, mutant)
    a = g * v
    s = (p * a).sum(1, keepdim=True)
    gl = p * a if mutant == "no_minus_s" else p * (a - s)
    gd = scale * _gather(_blocks(p * g, mutant))
    return (p * v).sum(1), (scale * gd if mutant == "scale_twice" else gd), gl


def magnitudes(disp, nine, gout, logits, scale=SCALE):
    """mag of out, gdisp, gnine (shaped like them) and, for the logits form, the spreads R of every fine pixel
    (B, 1, 4h, 4w) and R_max of every gdisp element (B, 1, h, w)."""
    disp, nine, g = disp.double().abs(), nine.double(), gout.double().abs()[:, None]
    if not logits:
        nb = neighbours(disp)
        return dict(out=(nine.abs() * nb).sum(1), gdisp=_gather(_blocks(nine.abs() * g)), gnine=g * nb)
    p = torch.softmax(nine, 1)
    v = scale * neighbours(disp)
    A = g * v
    S = (p * A).sum(1, keepdim=True)
    R = nine.amax(1, keepdim=True) - nine.amin(1, keepdim=True)
    R_max = F.max_pool2d(F.max_pool2d(R, 4), 3, stride=1, padding=1)
    return dict(out=(p * v).sum(1), gdisp=scale * _gather(_blocks(p * g)), gnine=p * (A + S), R=R, R_max=R_max)


def constants(mags, logits):
    """c of |got - exact| <= 2 c u mag (module docstring); the weights form's gnine is exact to one rounding (no c)."""
    if not logits:
        return dict(out=None, gdisp=torch.full_like(mags["gdisp"], 145.0), gnine=None)
    return dict(out=2.0 * mags["R"][:, 0] + 22.0, gdisp=2.0 * mags["R_max"] + 13.0 + 144.0, gnine=4.0 * mags["R"] + 38.0)


def fp32_product(disp, gout):
    """The weights form's gweights to the bit: fl(g * nb_k) in float32 (numpy in, torch out)."""
    return torch.from_numpy(gout)[:, None] * neighbours(torch.from_numpy(disp))
