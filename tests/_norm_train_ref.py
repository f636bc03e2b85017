"""Float64 truth, CPU emulation, error bound and fixed cases for the instance-norm training nodes (test infrastructure).

Notation, per (n, c) plane of HW elements: mu and var the plane's mean and biased variance, r = 1 / sqrt(var + eps),
yh = (x - mu) r, g the masked upstream gradient (gy [yh > 0] for the norm with ReLU, gy without; gout [out > 0] [yh_c > 0]
for the join relu(a + relu(yh_c))), mean(.) the plane's mean:

    gx = r (g - mean g - yh mean(g yh))                         ga = gout [out > 0]

Truth is that closed form in float64 with mu, r, yh from x.double() and the masks of the forward under test (the forward
is held to the inference kernel bit for bit, so its masks are the reference's).

What the kernels compute (csrc/norm_train.hip), and what `emulate` reproduces on the CPU: yh^ = fl(fl(x - mean^) invstd^)
with the saved fp32 (mean^, invstd^) of the forward; the plane sums of g and of g yh^ in fp64 (the product of two floats
is exact in fp64), `split` partial sums per plane added in slice order; m1 = fl32(sum g / HW), m2 = fl32(sum g yh^ / HW);
gx^ = fl(invstd^ fl(fl(g - m1) - fl(yh^ m2))).

The bound (U = 2^-24, first order in U).
  Recomputed yh.  mean^ is mu rounded to fp32 (the fp64 statistics put it within U |mu| of mu), the subtraction rounds
  once (U |x - mu|) and the product with invstd^ (within 2 U of r: one rounding of var + eps, a correctly rounded sqrt
  and division) once more.  Where |mu| is large against the spread the error of mean^ is not small against x - mu:
      |yh^ - yh| <= e_y = U (3 |yh| + 2 (|x| + |mu|) r).
  The means.  fp64 sums contribute nothing at this order; m2 inherits mean(|g| e_y) from yh^, and both are rounded to
  fp32 once (U |mean g|, U |mean(g yh)|).
  The element-wise chain.  Four fp32 operations, each rounding a quantity no larger than |g| + |mean g| + |yh| |mean(g yh)|,
  the rounding of the two means, and invstd^ (2 U): at most 8 U r (|g| + |mean g| + |yh| |mean(g yh)|).
  Together
      |gx^ - gx| <= 8 U r (|g| + |mean g| + |yh| |mean(g yh)|)  +  r (e_y |mean(g yh)| + |yh| mean(|g| e_y)).
ga is exact.  The constants come from this count, not from device output; test_host_norm_train_ref.py shows that the
emulation meets the bound on every case and that dropping either reduction term, summing the unmasked gradient or
losing one slice's partial sum misses it."""
import numpy as np
import torch
import torch.nn.functional as F

import _synth

U = 2.0 ** -24
EPS = 1e-5
SPLIT_MAX = 64


def _case(seed, shape, mean=0.0, spread=1.0, const=None):
    return dict(seed=seed, shape=shape, mean=mean, spread=spread, const=const)


CASES = {
    "smallest": _case(301, (1, 2, 1, 2)),                       # torch rejects HW = 1
    "odd": _case(302, (2, 3, 3, 5)),                            # scalar path, every plane after the first unaligned
    "odd_mean": _case(303, (1, 4, 7, 9), mean=0.5),
    "slices": _case(304, (1, 2, 96, 97)),                       # three slices per plane
    "slices_partial": _case(305, (1, 2, 100, 97)),              # float4 path, three slices, the last one shorter
    "aligned": _case(306, (2, 8, 64, 128)),
    "mean100": _case(307, (1, 4, 32, 32), mean=100.0),
    "mean1000": _case(308, (1, 4, 32, 32), mean=1000.0),
    "spread1e-3": _case(309, (1, 4, 32, 32), spread=1e-3),
    "spread1e3": _case(310, (1, 4, 32, 32), spread=1e3),
    "constant": _case(311, (1, 1, 4, 4), const=0.1),            # variance 0
    "quarter": _case(312, (1, 2, 120, 224)),                    # one image's planes at the recipe's quarter resolution
}
#: cases whose planes take more than one slice of the sums launch
SPLIT_CASES = ("slices", "slices_partial", "aligned", "quarter")
DEGENERATE = ("constant",)


def inputs(c):
    """x, gy, a (float32 torch, CPU).  gy = randn + 0.3 + 0.5 (x - mean) / spread: both reduction terms far above the
    bound; a = randn - 0.35: roughly half of a + relu(yh) is negative."""
    shape = c["shape"]
    if c["const"] is not None:
        x = np.full(shape, c["const"], np.float32)
        z = np.zeros(shape, np.float32)
    else:
        z = _synth.normal(shape, c["seed"], "x")
        x = (np.float32(c["mean"]) + np.float32(c["spread"]) * z).astype(np.float32)
    gy = (_synth.normal(shape, c["seed"], "gy") + np.float32(0.3) + np.float32(0.5) * z).astype(np.float32)
    a = (_synth.normal(shape, c["seed"], "a") - np.float32(0.35)).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(gy), torch.from_numpy(a)


def split(planes, HW):
    """Blocks per plane of the sums launch (csrc/norm_split.h norm_split)."""
    S = (2048 + planes - 1) // planes
    S = min(S, (HW + 4095) // 4096, SPLIT_MAX)
    return max(S, 1)


def slices(HW, S):
    per = ((HW + S - 1) // S + 3) & ~3
    return [(min(s * per, HW), min(s * per + per, HW)) for s in range(S)]


def _planes(t):
    return t.reshape(t.shape[0] * t.shape[1], -1)


def saved_stats(x, eps=EPS):
    """(planes, 2) float32 (mean, 1/std) as dkt_instance_norm_finalize leaves them: fp64 sums, fp32 at the end."""
    p = _planes(x).double()
    HW = p.shape[1]
    mean = p.sum(1) / HW
    var = ((p * p).sum(1) / HW - mean * mean).clamp_min(0.0)
    invstd = torch.tensor(1.0, dtype=torch.float32) / torch.sqrt(var.float() + torch.tensor(eps, dtype=torch.float32))
    return torch.stack([mean.float(), invstd], 1)


def yhat32(x, mi):
    """The forward's pre-ReLU value in fp32: fl(fl(x - mean) * invstd)."""
    return ((_planes(x) - mi[:, :1]) * mi[:, 1:]).reshape(x.shape)


def forward_norm(x, mi, relu):
    y = yhat32(x, mi)
    return y.clamp_min(0.0) if relu else y


def forward_join(a, c, mi):
    return (a + yhat32(c, mi).clamp_min(0.0)).clamp_min(0.0)


def emulate(gup, x, mi, mask, mutate=None):
    """The backward kernels' arithmetic on the CPU (module docstring).  gup: upstream gradient, mask: bool, the product of
    the forward's ReLU masks (None: no mask).  mutate: None, 'no_mean_g', 'no_proj', 'unmasked_sums', 'drop_slice'."""
    shape = x.shape
    yh = _planes(yhat32(x, mi))
    gu = _planes(gup)
    g = gu if mask is None else torch.where(_planes(mask), gu, torch.zeros_like(gu))
    planes, HW = g.shape
    S = split(planes, HW)
    gs = gu if mutate == "unmasked_sums" else g
    sl = slices(HW, S)
    if mutate == "drop_slice":
        sl = sl[:-1] if S > 1 else sl
    sg = torch.zeros(planes, dtype=torch.float64)
    sgy = torch.zeros(planes, dtype=torch.float64)
    for lo, hi in sl:                                                # partial sums, added in slice order
        sg = sg + gs[:, lo:hi].double().sum(1)
        sgy = sgy + (gs[:, lo:hi].double() * yh[:, lo:hi].double()).sum(1)
    m1 = (sg / HW).float()[:, None]
    m2 = (sgy / HW).float()[:, None]
    if mutate == "no_mean_g":
        m1 = torch.zeros_like(m1)
    if mutate == "no_proj":
        m2 = torch.zeros_like(m2)
    return (mi[:, 1:] * ((g - m1) - yh * m2)).reshape(shape)         # fp32, one rounding per operation


def truth_and_bound(gup, x, mask, eps=EPS):
    """(gx in float64, the bound of the module docstring, and the size of the two reduction terms in the case: the planes'
    average |mean g| and |mean(g yh)| over the average |g|)."""
    shape = x.shape
    p = _planes(x).double()
    mu = p.mean(1, keepdim=True)
    var = ((p - mu) ** 2).mean(1, keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    yh = (p - mu) * r
    g = _planes(gup).double()
    if mask is not None:
        g = g * _planes(mask).double()
    mg = g.mean(1, keepdim=True)
    mgy = (g * yh).mean(1, keepdim=True)
    gx = r * (g - mg - yh * mgy)
    e_y = U * (3.0 * yh.abs() + 2.0 * (p.abs() + mu.abs()) * r)
    bound = (8.0 * U * r * (g.abs() + mg.abs() + yh.abs() * mgy.abs())
             + r * (e_y * mgy.abs() + yh.abs() * (g.abs() * e_y).mean(1, keepdim=True)))
    mag = max(float(g.abs().mean()), 1e-300)
    return gx.reshape(shape), bound.reshape(shape), float(mg.abs().mean()) / mag, float(mgy.abs().mean()) / mag


def worst(got, exact, bound):
    """Largest |got - exact| / bound over the elements; where the bound is 0 the result must be exact (inf otherwise)."""
    d = (got.detach().double().cpu() - exact).abs()
    zero = bound == 0
    if bool((d[zero] != 0).any()):
        return float("inf")
    return float((d / torch.where(zero, torch.ones_like(bound), bound)).max())


def torch_norm_grad(gy, x, relu, eps=EPS):
    """torch's own fp32 CPU backward of [relu](F.instance_norm(x)): for the record, not a yardstick."""
    x = x.clone().requires_grad_(True)
    y = F.instance_norm(x, eps=eps)
    if relu:
        y = F.relu(y)
    return torch.autograd.grad(y, x, gy)[0]


def same(a, b):
    """Bit-for-bit equality of two float32 tensors, NaNs compared by position."""
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int32), b[~nb].view(np.int32))
