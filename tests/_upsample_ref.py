"""Float64 reference, fp32 yardstick, error bound and fixed cases for the convex up-sampling node (test infrastructure).

Notation: flow (N, D, H, W), mask (N, 9 f^2, H, W), p_k = softmax_k(mask[n, (k f + i) f + j, h, w]),
v_{d,k} = f * flow[n, d, h + k/3 - 1, w + k%3 - 1] (0 outside), out[n, d, f h + i, f w + j] = sum_k p_k v_{d,k}; only the
leading Dout channels of out are used.  With g the upstream gradient:

    a_k = sum_{d < Dout} g_d v_{d,k},  s = sum_k p_k a_k,  gmask = p_k (a_k - s)
    gflow[n, d, y, x] = f * sum_k sum_{i,j} p_k(i, j, h, w) g[n, d, f h + i, f w + j],  (h, w) = (y - k/3 + 1, x - k%3 + 1)

The bound (u = 2^-24; every statement to first order in u, the factor 2 of headroom of the assertions covers the rest).

  softmax.  t_k = fl(m_k - max) carries a relative error u, so exp's argument is off by |m_k - max| u <= R u, where
  R = max_k m - min_k m is the spread of the nine logits of that fine pixel; expf is within one ulp (2 u).  So
  e_k = exp(m_k - max) (1 + d_k) with |d_k| <= (R + 2) u.  The sum of nine positive terms takes 8 additions (8 u), the
  division one rounding:  p^_k = p_k (1 + d_k - sum_j p_j d_j - (sum rounding) + (division)),
      |p^_k - p_k| <= c_p u p_k,   c_p = 2 (R + 2) + 8 + 1 = 2 R + 13.
  out.  v_{d,k} is exact (f is a power of two).  Nine products (1 each) and 8 additions, whatever their order:
      |out^ - out| <= (c_p + 9) u sum_k p_k |v_k| = (2 R + 22) u mag_out.
  gmask.  a_k: Dout products and Dout - 1 additions, Dout u A_k with A_k = sum_d |g_d| |v_{d,k}|.  s: products of p^_k and
  a^_k (c_p + Dout + 1) and 8 additions, (c_p + Dout + 9) u S with S = sum_k p_k A_k.  The subtraction rounds once more,
  u (A_k + S); the final product brings (c_p + 1) u |a_k - s| <= (c_p + 1) u (A_k + S).  Together
      |gmask^ - gmask| <= (2 c_p + Dout + 11) u p_k (A_k + S) = (4 R + Dout + 37) u mag_gmask.
  gflow.  At most 9 f^2 products p^ g (c_p + 1 each, with the largest R among the contributing fine pixels: all (i, j) of
  the 3 x 3 coarse neighbourhood) and 9 f^2 - 1 additions in any order; the factor f is exact:
      |gflow^ - gflow| <= (2 R_max + 13 + 9 f^2) u mag_gflow,   mag_gflow = f sum p |g|.

The magnitudes are the same float64 chain run on |flow| and |g| with the true p.  The bound is one of relative errors: it
holds while no softmax term underflows in fp32 (a spread R below about 87); WIDE_CASES, whose spreads go beyond that, are
for bit-for-bit comparisons only."""
import numpy as np
import torch
import torch.nn.functional as F

import _cases
import _synth

U = 2.0 ** -24


def _case(seed, N, D, Dout, H, W, f, sigma=2.0):
    return dict(seed=seed, N=N, D=D, Dout=Dout, H=H, W=W, f=f, sigma=sigma)


def _parity(name):
    c = _cases.UPSAMPLE_CASES[name]
    return dict(parity=name, seed=c["seed"], N=c["N"], D=c["D"], Dout=c["D"], H=c["H"], W=c["W"], f=2 ** c["nd"], sigma=2.0)


CASES = {
    "f4": _parity("f4"),                                   # the three parity cases of _cases.UPSAMPLE_CASES, every channel
    "f2": _parity("f2"),
    "f8": _parity("f8"),
    "h1": _case(201, 2, 2, 2, 1, 11, 4),
    "w1": _case(202, 1, 2, 1, 9, 1, 2),
    "one": _case(203, 1, 1, 1, 1, 1, 8),
    "f1": _case(204, 2, 2, 2, 6, 10, 1),
    "dout1of2": _case(205, 2, 2, 1, 7, 13, 4),
    "dout3of4": _case(206, 1, 4, 3, 5, 9, 2),               # more channels than one kernel pass holds
    "tiles": _case(207, 1, 2, 1, 20, 70, 4),                # many 64-pixel tiles, wider and taller than one
    "recipe": _case(208, 2, 2, 1, 120, 224, 4),             # B = 2 at 480 x 896
    "sigma0.5": _case(209, 1, 2, 1, 12, 40, 4, sigma=0.5),
    "sigma8": _case(210, 1, 2, 1, 12, 40, 4, sigma=8.0),
}


#: spreads beyond 69 (terms below 2^-100) and beyond 87 and 103 (denormal terms, terms that are 0 in fp32)
WIDE_CASES = {
    "sigma16": _case(211, 1, 2, 1, 12, 40, 4, sigma=16.0),
    "sigma32": _case(212, 2, 2, 2, 5, 70, 2, sigma=32.0),
}


def inputs(c):
    """flow, mask, gout (float32 numpy), factor, Dout."""
    f = c["f"]
    if "parity" in c:
        flow, mask, f = _cases.upsample_inputs(_cases.UPSAMPLE_CASES[c["parity"]])
    else:
        flow = _synth.normal((c["N"], c["D"], c["H"], c["W"]), c["seed"], "flow", scale=5.0)
        mask = _synth.normal((c["N"], 9 * f * f, c["H"], c["W"]), c["seed"], "mask", scale=c["sigma"])
    gout = _synth.normal((c["N"], c["Dout"], f * c["H"], f * c["W"]), c["seed"], "gout")
    return flow, mask, gout, f, c["Dout"]


def sequence(flow, mask, factor):
    """The reference's expression sequence (meta_arch/raft_stereo/raft_stereo.py:70-82), any dtype."""
    N, D, H, W = flow.shape
    mask = mask.view(N, 1, 9, factor, factor, H, W)
    mask = torch.softmax(mask, dim=2)
    up_flow = F.unfold(factor * flow, [3, 3], padding=1)
    up_flow = up_flow.view(N, D, 9, 1, 1, H, W)
    up_flow = torch.sum(mask * up_flow, dim=2)
    up_flow = up_flow.permute(0, 1, 4, 2, 5, 3)
    return up_flow.reshape(N, D, factor * H, factor * W)


def autograd(flow, mask, gout, factor, Dout, dtype):
    """(out[:, :Dout], gflow, gmask) of the sequence under torch autograd on the CPU in `dtype`."""
    a = torch.from_numpy(flow).to(dtype).requires_grad_(True)
    b = torch.from_numpy(mask).to(dtype).requires_grad_(True)
    out = sequence(a, b, factor)[:, :Dout]
    ga, gb = torch.autograd.grad(out, (a, b), torch.from_numpy(gout).to(dtype))
    return out.detach(), ga, gb


def truth(flow, mask, gout, factor, Dout):
    return autograd(flow, mask, gout, factor, Dout, torch.float64)


def yardstick(flow, mask, gout, factor, Dout):
    return autograd(flow, mask, gout, factor, Dout, torch.float32)


def _parts(flow, mask, gout, f, Dout):
    """p (N, 9, f, f, H, W), v (N, Dout, 9, H, W), g (N, Dout, f, f, H, W) in float64."""
    N, D, H, W = flow.shape
    p = torch.softmax(mask.double().view(N, 9, f, f, H, W), dim=1)
    v = F.unfold(f * flow.double(), [3, 3], padding=1).view(N, D, 9, H, W)[:, :Dout]
    g = gout.double().view(N, Dout, H, f, W, f).permute(0, 1, 3, 5, 2, 4)
    return p, v, g


def closed_form(flow, mask, gout, f, Dout):
    """(out[:, :Dout], gflow, gmask) in float64 from the formulas of the module docstring (torch tensors in)."""
    N, D, H, W = flow.shape
    p, v, g = _parts(flow, mask, gout, f, Dout)
    out = torch.einsum("nkijhw,ndkhw->ndhiwj", p, v).reshape(N, Dout, f * H, f * W)
    a = torch.einsum("ndijhw,ndkhw->nkijhw", g, v)
    s = (p * a).sum(dim=1, keepdim=True)
    gmask = (p * (a - s)).reshape(N, 9 * f * f, H, W)
    c = torch.einsum("nkijhw,ndijhw->ndkhw", p, g)
    gflow = torch.zeros((N, D, H, W), dtype=torch.float64)
    gflow[:, :Dout] = f * F.fold(c.reshape(N, Dout * 9, H * W), (H, W), [3, 3], padding=1)      # fold = unfold's adjoint
    return out, gflow, gmask


def magnitudes(flow, mask, gout, f, Dout):
    """mag_out, mag_gflow, mag_gmask (shaped like out[:, :Dout], flow, mask) and the logit spreads R of every fine pixel
    (shaped like mask, equal over k) and R_max of every gflow element (N, 1, H, W)."""
    N, D, H, W = flow.shape
    p, v, g = _parts(flow.abs(), mask, gout.abs(), f, Dout)
    mag_out = torch.einsum("nkijhw,ndkhw->ndhiwj", p, v).reshape(N, Dout, f * H, f * W)
    A = torch.einsum("ndijhw,ndkhw->nkijhw", g, v)
    S = (p * A).sum(dim=1, keepdim=True)
    mag_gmask = (p * (A + S)).reshape(N, 9 * f * f, H, W)
    c = torch.einsum("nkijhw,ndijhw->ndkhw", p, g)
    mag_gflow = torch.zeros((N, D, H, W), dtype=torch.float64)
    mag_gflow[:, :Dout] = f * F.fold(c.reshape(N, Dout * 9, H * W), (H, W), [3, 3], padding=1)
    m = mask.double().view(N, 9, f, f, H, W)
    R = m.amax(dim=1, keepdim=True) - m.amin(dim=1, keepdim=True)                       # (N, 1, f, f, H, W)
    R_out = R[:, 0].permute(0, 3, 1, 4, 2).reshape(N, 1, f * H, f * W)                  # per output pixel
    R_mask = R.expand(N, 9, f, f, H, W).reshape(N, 9 * f * f, H, W)
    R_flow = F.max_pool2d(R.amax(dim=(2, 3)), 3, stride=1, padding=1)                   # (N, 1, H, W): 3 x 3 neighbourhood
    return dict(out=mag_out, gflow=mag_gflow, gmask=mag_gmask, R_out=R_out, R_mask=R_mask, R_flow=R_flow)


def constants(mags, f, Dout):
    """c of |got - exact| <= 2 c u mag for out, gflow, gmask (module docstring)."""
    return dict(out=2.0 * mags["R_out"] + 22.0,
                gflow=2.0 * mags["R_flow"] + 13.0 + 9.0 * f * f,
                gmask=4.0 * mags["R_mask"] + Dout + 37.0)


def worst(got, exact, mag, c):
    """(largest |got - exact| / (u mag), largest |got - exact| / (2 c u mag)) over the elements; where mag is 0 the
    result must be exact (the ratio is inf otherwise)."""
    d = (got.detach().double().cpu() - exact).abs()
    zero = mag == 0
    if bool((d[zero] != 0).any()):
        return float("inf"), float("inf")
    safe = torch.where(zero, torch.ones_like(mag), mag)
    in_u = d / (U * safe)
    return float(in_u.max()), float((in_u / (2.0 * c)).max())


def same(a, b):
    """Bit-for-bit equality of two float32 tensors, NaNs compared by position."""
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int32), b[~nb].view(np.int32))
