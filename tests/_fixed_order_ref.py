"""CPU restatement (numpy fp64, exact IEEE adds) of the fixed-order sums of csrc/wave_reduce.h and, on top of them, of the
loss scalars of dkt_seq_loss and of dkt_ns_loss's disparity branch, bit for bit from the inputs.  `sequential` / `perm`
are the mutants of tests/test_host_fixed_order_ref.py: another association of the same terms."""
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
_LANES = np.arange(64)


def butterfly(v, sequential=False):
    """wave_sum of (..., 64): every lane adds its xor partner at offsets 32 .. 1; the value of lane 0."""
    if sequential:
        s = np.zeros(v.shape[:-1])
        for l in range(64):
            s = s + v[..., l]
        return s
    for sh in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANES ^ sh]
    return v[..., 0]


def block_sum(v, sequential=False):
    """(..., waves, 64) -> (...): wave sums added in index order.  The loss kernels start from 0.0 and block_sum() of
    wave_reduce.h from slot 0: the same bits unless the total is -0.0, which sums of non-negative terms never are."""
    w = butterfly(v, sequential)
    s = np.zeros(w.shape[:-1])
    for i in range(w.shape[-1]):
        s = s + w[..., i]
    return s


def column_sum(p, perm=None, sequential=False):
    """column_sum of a 1-d array: lane l adds p[l], p[l + 64], ... in order, then the butterfly."""
    p = p if perm is None else p[perm]
    rows = np.concatenate([p, np.zeros(-len(p) % 64)]).reshape(-1, 64)      # (x + 0.0 is x for x >= 0)
    s = np.zeros(64)
    for row in rows:
        s = s + row
    return butterfly(s, sequential)


#: (B, H, W, predictions, skips) of the sequence losses and of ns_loss (tests/test_gpu_fixed_order_sums.py says why these
#: shapes).  skips: per target, which rounding boundary steer() aims at.  On most boundaries a mutant's fp64 total lands
#: on the same side as the right one (the orders differ by an fp64 ulp or two, in a direction the data fixes), so each
#: entry is the smallest of 0, 1, 2, ... at which every assertion of tests/test_host_fixed_order_ref.py holds for that
#: case and target; that test is the check, and a skip that stops satisfying it is replaced the same way.
SEQ_CASES = {"raft": [(1, 5, 7, 2, (3, 3)), (3, 176, 1025, 3, (3, 2))],
             "gwc": [(1, 5, 7, 2, (5, 4)), (3, 176, 1025, 3, (0, 0))]}
NS_CASES = [(1, 40, 56, 2, (1,)), (2, 272, 256, 2, (5,))]
SEED = 1
GWC_WEIGHTS = (0.5, 0.5, 0.7, 1.0)


def raft_weights(n):
    return [(0.9 ** (15 / (n - 1))) ** (n - i - 1) for i in range(n)]


def loss_term(kind, p, g):
    z = np.abs(p - g)                                                          # fp32
    return z if kind == "raft" else np.where(z < 1, (F32(0.5) * z) * z, z - F32(0.5))


def exact_sum(x):
    """The sum of an array of non-negative fp32 values as a Fraction."""
    m, e = np.frexp(x.astype(np.float64).ravel())
    per_exp = np.bincount(e - e.min(), weights=m * 2.0 ** 24)                  # (24-bit integers: exact in fp64)
    return sum(Fraction(int(v)) * Fraction(2) ** int(j + e.min() - 24) for j, v in enumerate(per_exp))


def steer(kind, terms, N, skip):
    """Three differences z whose terms, added to `terms`, put the exact sum on N times a rounding boundary of fp32 (to
    2^-70; `skip` picks the boundary): which side the fp64 sum comes out on, and so the fp32 mean, is then decided by
    the order of the additions."""
    S = exact_sum(terms)
    a, skip, half = F32(float(S / N)), skip // 3, skip % 3 - 1
    while True:                                                                # the skip-th boundary above the sum ...
        up = np.nextafter(a, F32(np.inf))
        T = (Fraction(float(a)) + Fraction(float(up))) / 2 * N
        rest = T - S
        a = up
        if rest > 0:
            skip -= 1
            if skip < 0:
                break
    rest += Fraction(half, 2) * Fraction(math.ulp(float(T)))                   # ... or half an fp64 ulp beside it
    zs = []
    for _ in range(3):
        lo, hi = 0, 0x44000000                                                 # bit patterns of 0 .. 2^9, term() is monotone
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if Fraction(float(loss_term(kind, np.array(mid, np.int32).view(F32), F32(0)))) <= rest:
                lo = mid
            else:
                hi = mid - 1
        zs.append(np.array(lo, np.int32).view(F32))
        rest -= Fraction(float(loss_term(kind, zs[-1], F32(0))))
    return zs


def draw(kind, B, H, W, n, K, skips):
    """K targets and n predictions, fp32 (B, H, W): |target| log-uniform in [2^-40, 2^-20) (negative for kind "ns"; a
    larger target would quantise pred - target to its own ulp and leave nothing for fp64 to round) and |pred| log-uniform
    in [2^-30, 2^9), so that the terms, 24 bits each, span far more than fp64's 53 bits; then three pixels per target
    are steered (see steer; skips[k]: which boundary) against the LAST prediction, which is 0 there.  Also the
    confidence of ns_loss (ones otherwise)."""
    rng = np.random.default_rng(SEED)
    sign = lambda: -1.0 if kind == "ns" else rng.choice([-1.0, 1.0], (B, H, W))
    gts = [(sign() * 2.0 ** rng.uniform(-40, -20, (B, H, W))).astype(F32) for _ in range(K)]
    preds = [(rng.choice([-1.0, 1.0], (B, H, W)) * 2.0 ** rng.uniform(-30, 9, (B, H, W))).astype(F32) for _ in range(n)]
    conf = np.ones((B, H, W), F32) if kind != "ns" else rng.uniform(0.75, 1.0, (B, H, W)).astype(F32)
    preds[-1].flat[3:3 + 3 * K] = 0
    conf.flat[3:3 + 3 * K] = 1
    term = "raft" if kind == "ns" else kind
    for k, g in enumerate(gts):
        at = slice(3 + 3 * k, 6 + 3 * k)
        g.flat[at] = 0
        g.flat[at] = [-z for z in steer(term, loss_term(term, preds[-1], g) * conf, B * H * W, skips[k])]
    return gts, preds, conf


def seq_partials(x, sequential=False):
    """(B, HW) fp64 terms -> dkt_seq_loss's block partials: tiles of 1024, thread t owns t + 256 j, j = 0..3 in order."""
    B, HW = x.shape
    tiles = -(-HW // 1024)
    x = np.concatenate([x, np.zeros((B, tiles * 1024 - HW))], 1).reshape(B, tiles, 4, 256)
    t = ((x[:, :, 0] + x[:, :, 1]) + x[:, :, 2]) + x[:, :, 3]
    return block_sum(t.reshape(B * tiles, 4, 64), sequential)


def ns_partials(x, sequential=False):
    """(B, H, W) fp64 terms -> dkt_ns_loss's block partials: 16 x 16 tiles, one pixel per thread, tid = ly * 16 + lx."""
    B, H, W = x.shape
    gy, gx = -(-H // 16), -(-W // 16)
    p = np.zeros((B, gy * 16, gx * 16))
    p[:, :H, :W] = x
    return block_sum(p.reshape(B, gy, 16, gx, 16).transpose(0, 1, 3, 2, 4).reshape(B * gy * gx, 4, 64), sequential)


def weighted(totals, weights, N):
    """sum_i fl32(w_i) * fl32(t_i / N) in fp32, in order i."""
    loss = F32(0)
    for t, w in zip(totals, weights):
        loss = F32(loss + F32(F32(w) * F32(t / N)))
    return loss


def seq_loss(kind, preds, gts, perm=None, sequential=False):
    """Loss per target of dkt_seq_loss, every pixel valid.  preds, gts: fp32 (B, H, W) arrays."""
    w = raft_weights(len(preds)) if kind == "raft" else GWC_WEIGHTS
    out = []
    for g in gts:
        tot = [column_sum(seq_partials(loss_term(kind, p, g).astype(np.float64).reshape(len(g), -1), sequential), perm, sequential)
               for p in preds]
        out.append(weighted(tot, w, float(g.size)))
    return out


def ns_disp_loss(preds, target, conf, perm=None, sequential=False):
    """dkt_ns_loss with alpha_photometric = 0, alpha_disp_loss = 1, every pixel valid: fp32 |p - t| * conf per pixel."""
    tot = [column_sum(ns_partials((np.abs(p - target) * conf).astype(np.float64), sequential), perm, sequential) for p in preds]
    return weighted(tot, raft_weights(len(preds)), float(target.size))
