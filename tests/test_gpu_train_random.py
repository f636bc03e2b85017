"""Randomised and recipe-sized tests of the training-path kernels (-m gpu): the correlation and geometry lookup backward,
the pooling-chain backward, the cost-volume backward, the sequence losses and F&E.

References: the C oracle (bit-exact where the kernel rounds in the same order), fp32 torch restatements in the kernel's
or the reference's operation order (bit-exact), and float64 restatements (_train_ref.py) with bounds derived from the
operation.  Shapes are drawn so that the branches that only run at real sizes are reached: the 8-wide finalize loop of
the loss (more than 448 blocks), the striding count pass of F&E (more than 65,536 pixels), the grid-stride loop of the
correlation pool backward (more than 16,384 x 256 elements), every radius 0..8 the ABI accepts, width-1 pyramid levels
and the odd last plane of a geometry level.

Feature-gradient bound.  A contraction of length n computed in fp32 is within n u (|A| . |B|) of exact (u = 2^-24),
whatever the summation order.  The volume gradient that enters it carries its own fp32 roundings relative to the
float64 restatement (which uses the same fp32 sample positions): the weight e = 1 - w (1), the product with the upstream
gradient (1), at most two further additions into a level entry (2), L - 1 additions of the pooling chain and the
division by the divisor (L): (L + 4) u of the same magnitudes.  So |got - exact| <= (n + L + 4) u (|G| . |f|), with |G|
the float64 chain run on |upstream|, and a factor 2 of headroom on top."""
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, example, given, settings
from hypothesis import strategies as st

import _synth
import _train_ref as R
from test_gpu_volume_grad import check as vol_check
from test_gpu_volume_grad import concat64, grads64, gwc64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SET = dict(deadline=None, max_examples=60, suppress_health_check=list(HealthCheck), derandomize=True)
U = R.U32


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def same(a, b):
    """Bit-for-bit equality, NaNs compared by position."""
    a, b = host(a), host(b)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int32), b[~nb].view(np.int32))


def within_contraction(got, exact, mag, n, L, what):
    lim = 2.0 * (n + L + 4) * U * mag
    d = (got.detach().double().cpu() - exact).abs()
    assert bool((d <= lim).all()), (what, float((d - lim).max()), float(lim.max()))


def _flat(levels):
    return [t.detach().reshape(t.shape[0], -1) for t in levels]


# ---- CorrBlock1D backward -----------------------------------------------------------------------------------------------
def _corr_backward_case(c_oracle, B, C, H, W1, W2, L, r, seed, strided):
    from dkt_stereo_amd import _ffi
    from dkt_stereo_amd.corr import CorrBlock1D
    K = 2 * r + 1
    f1 = _synth.normal((B, C, H, W1), seed, "f1")
    f2 = _synth.normal((B, C, H, W2), seed, "f2")
    x = _synth.uniform((B, 1, H, W1), -6.0, W2 + 6.0, seed, "x")
    x[..., ::3] = np.round(x[..., ::3])                      # exact integers
    x[..., 1::4] = np.round(x[..., 1::4]) + 0.5              # exact half-integers
    coords = np.concatenate([x, np.zeros_like(x)], 1)
    gout = _synth.normal((B, L * K, H, W1), seed, "gout")
    a, b = G(f1).requires_grad_(True), G(f2).requires_grad_(True)
    blk = CorrBlock1D(a, b, num_levels=L, radius=r)
    if strided:                                              # a batch-strided view of a wider buffer
        buf = torch.full((B, 4, H, W1), 7.0, device=DEV)
        buf[:, 1:3] = G(coords)
        cg = buf[:, 1:3]
    else:
        cg = G(coords)
    out = blk(cg)
    glv = torch.autograd.grad(out, blk.corr_pyramid, G(gout), retain_graph=True)
    want = c_oracle.corr1d_lookup_bwd(gout, coords, r, [W2 >> i for i in range(L)], B * H * W1)
    for i, g in enumerate(_flat(glv)):
        assert same(g, want[i]), ("level", i)                               # scatter: bit exact
    divisor = float(torch.sqrt(torch.tensor(C).float()))
    lv = [g.contiguous() for g in glv]
    gvol = torch.empty((B * H * W1, W2), device=DEV)
    _ffi.check(_ffi.lib().dkt_corr1d_pool_bwd(_ffi.ptr_array(lv), gvol.data_ptr(), B, H, W1, W2, L, divisor,
                                              _ffi.device_of(gvol), _ffi.stream_of(gvol)), "dkt_corr1d_pool_bwd")
    assert same(gvol, c_oracle.corr1d_pool_bwd(want, divisor))              # folded pooling chain: bit exact
    gf1, gf2 = torch.autograd.grad(out, [a, b], G(gout))
    xs = torch.from_numpy(x[:, 0])

    def grads(p, q, up):
        p = torch.from_numpy(p).double().requires_grad_(True)
        q = torch.from_numpy(q).double().requires_grad_(True)
        return torch.autograd.grad(R.corr_lookup64(p, q, xs, L, r, divisor), (p, q), torch.from_numpy(up).double())

    e1, e2 = grads(f1, f2, gout)
    m1, m2 = grads(np.abs(f1), np.abs(f2), np.abs(gout))
    n = max(W1, W2)
    within_contraction(gf1, e1, m1, n, L, "gf1")
    within_contraction(gf2, e2, m2, n, L, "gf2")


@settings(**SET)
@given(B=st.integers(1, 3), C=st.integers(1, 40), H=st.integers(1, 5), W1=st.integers(2, 70), dW=st.integers(-8, 12),
       L=st.integers(1, 8), r=st.integers(0, 8), strided=st.booleans(), seed=st.integers(0, 10 ** 6))
@example(B=2, C=7, H=3, W1=33, dW=4, L=3, r=7, strided=False, seed=1)
@example(B=1, C=5, H=2, W1=20, dW=-3, L=5, r=8, strided=True, seed=2)       # W2 = 17: width-1 last level
@example(B=3, C=3, H=1, W1=9, dW=0, L=4, r=6, strided=True, seed=3)         # W2 = 9: width-1 last level
def test_corr_backward_random(c_oracle, B, C, H, W1, dW, L, r, strided, seed):
    W2 = max(W1 + dW, 1)
    L = min(L, W2.bit_length())                             # the deepest level may be one column wide
    _corr_backward_case(c_oracle, B, C, H, W1, W2, L, r, seed, strided)


def test_corr_backward_raft_training_crop(c_oracle):
    """B = 2 at 320 x 736: quarter resolution 80 x 184, B*H*W1*W2 = 5.4M > 16,384 x 256, so the pool backward's
    grid-stride loop runs."""
    _corr_backward_case(c_oracle, 2, 32, 80, 184, 184, 4, 4, 41, True)


# ---- Combined_Geo_Encoding_Volume -------------------------------------------------------------------------------------
def fold32(levels):
    """T_{L-1} = g_{L-1};  T_i[d] = g_i[d] + T_{i+1}[d/2] / 2 where level i+1 has plane d/2, else g_i[d]: fp32, in the
    order of dkt_geo_pool_bwd.  levels: (M, D_i) float32."""
    t = levels[-1]
    for g in reversed(levels[:-1]):
        nxt = g.copy()
        m = t.shape[1]
        nxt[:, :2 * m] = g[:, :2 * m] + np.repeat(t / np.float32(2), 2, axis=1)
        t = nxt
    return t


@settings(**SET)
@given(B=st.integers(1, 2), Cm=st.integers(1, 24), C=st.integers(1, 12), D=st.integers(2, 48), H=st.integers(1, 4),
       W=st.integers(1, 48), L=st.integers(1, 8), r=st.integers(0, 8), seed=st.integers(0, 10 ** 6))
@example(B=1, Cm=5, C=3, D=23, H=2, W=30, L=3, r=7, seed=4)                  # odd D: odd last planes on levels 0, 1
@example(B=2, Cm=3, C=2, D=9, H=1, W=17, L=4, r=8, seed=5)                   # width-1 last levels
def test_geo_random(c_oracle, B, Cm, C, D, H, W, L, r, seed):
    from dkt_stereo_amd.geometry import Combined_Geo_Encoding_Volume
    L = min(L, D.bit_length(), W.bit_length())
    K = 2 * r + 1
    m1, m2 = _synth.fmap_pair(seed, B, Cm, H, W)
    geo = _synth.normal((B, C, D, H, W), seed, "geo")
    disp = _synth.uniform((B, 1, H, W), -3.0, D + 3.0, seed, "disp")
    disp[..., ::3] = np.round(disp[..., ::3])
    coords = np.broadcast_to(np.arange(W, dtype=np.float32).reshape(1, 1, W, 1), (B, H, W, 1)).copy()
    gout = _synth.normal((B, L * K * (C + 1), H, W), seed, "gout")
    a, b, gv = G(m1).requires_grad_(True), G(m2).requires_grad_(True), G(geo).requires_grad_(True)
    vol = Combined_Geo_Encoding_Volume(a, b, gv, num_levels=L, radius=r)
    out = vol(G(disp), G(coords))
    gp = [p.detach().permute(0, 3, 4, 1, 2).reshape(-1, p.shape[2]) for p in vol.geo_volume_pyramid]
    ip = _flat(vol.init_corr_pyramid)
    assert same(out, c_oracle.geo_lookup([host(p) for p in gp], [host(p) for p in ip], disp, coords, C, r))
    levels = vol.geo_volume_pyramid + vol.init_corr_pyramid
    glv = torch.autograd.grad(out, levels, G(gout), retain_graph=True)
    cg, ci = c_oracle.geo_lookup_bwd(gout, disp, coords, C, D, W, L, r)
    for i in range(L):
        assert same(glv[i].permute(0, 3, 4, 1, 2).reshape(-1, D >> i), cg[i]), ("geo level", i)
        assert same(glv[L + i].reshape(-1, W >> i), ci[i]), ("init level", i)
    ga, gb, gg = torch.autograd.grad(out, [a, b, gv], G(gout))
    want = fold32(cg).reshape(B, H, W, C, D).transpose(0, 3, 4, 1, 2)
    assert same(gg, want)                                                     # pooling chain: bit exact

    def chain64(lv):
        base = torch.zeros((B * H * W * C, D), dtype=torch.float64, requires_grad=True)
        pyr = R.pool64(base.clone(), L)
        return torch.autograd.grad(pyr, base, [torch.from_numpy(g).double() for g in lv])[0]

    e, mag = chain64(cg), chain64([np.abs(g) for g in cg])
    # L - 1 fp32 additions, each within u of the running magnitude; the halvings are exact
    assert bool(((torch.from_numpy(fold32(cg)).double() - e).abs() <= max(L - 1, 0) * U * mag).all())

    def grads(p, q, g3, up):
        ins = [torch.from_numpy(t).double().requires_grad_(True) for t in (p, q, g3)]
        o = R.geo_lookup64(*ins, torch.from_numpy(disp), torch.from_numpy(coords), L, r)
        return torch.autograd.grad(o, ins, torch.from_numpy(up).double())

    e1, e2, _ = grads(m1, m2, geo, gout)
    a1, a2, _ = grads(np.abs(m1), np.abs(m2), np.abs(geo), np.abs(gout))
    within_contraction(ga, e1, a1, W, L, "gm1")
    within_contraction(gb, e2, a2, W, L, "gm2")


# ---- cost-volume backward ------------------------------------------------------------------------------------------------
def _upstream(g, how):
    """The upstream gradient contiguous, W-major (transposed storage) or as a channel slice of a wider buffer."""
    if how == "transposed":
        return g.transpose(3, 4).contiguous().transpose(3, 4)
    if how == "slice":
        buf = torch.full((g.shape[0], g.shape[1] + 3) + tuple(g.shape[2:]), 9.0, device=g.device)
        buf[:, 2:2 + g.shape[1]] = g
        return buf[:, 2:2 + g.shape[1]]
    return g


@settings(**SET)
@given(B=st.integers(1, 2), G_=st.integers(1, 6), cpg=st.integers(1, 24), Cc=st.integers(1, 12), H=st.integers(1, 4),
       W=st.integers(1, 40), D=st.integers(1, 20), kind=st.sampled_from(["gwc", "concat", "igev", "fused"]),
       mode=st.sampled_from(["mfma", "exact"]), up=st.sampled_from(["contiguous", "transposed", "slice"]),
       need=st.sampled_from(["both", "first", "second"]), seed=st.integers(0, 10 ** 6))
@example(B=1, G_=2, cpg=20, Cc=3, H=2, W=1, D=5, kind="fused", mode="mfma", up="slice", need="both", seed=6)
@example(B=2, G_=1, cpg=17, Cc=5, H=3, W=6, D=19, kind="gwc", mode="exact", up="transposed", need="second", seed=7)
def test_volume_backward_random(B, G_, cpg, Cc, H, W, D, kind, mode, up, need, seed):
    from dkt_stereo_amd.submodule import (build_concat_volume, build_concat_volume_igev, build_gwc_concat_volume,
                                          build_gwc_volume, gwc_mode)
    C = G_ * cpg
    a, b = (G(t) for t in _synth.fmap_pair(seed, B, C, H, W))
    ca, cb = (G(t) for t in _synth.fmap_pair(seed + 1, B, Cc, H, W))
    first, second = need in ("both", "first"), need in ("both", "second")
    if kind == "fused":
        ins = [a.clone().requires_grad_(first), b.clone().requires_grad_(second),
               ca.clone().requires_grad_(second), cb.clone().requires_grad_(first)]
        gvol = G(_synth.normal((B, G_ + 2 * Cc, D, H, W), seed, "gvol"))
        with gwc_mode(mode):
            build_gwc_concat_volume(*ins, D, G_).backward(_upstream(gvol, up))
        want = list(grads64(lambda x, y: gwc64(x, y, D, G_), a, b, gvol[:, :G_]))
        want += list(grads64(lambda x, y: concat64(x, y, D, True), ca, cb, gvol[:, G_:]))
    else:
        x, y = (a, b) if kind == "gwc" else (ca, cb)
        ins = [x.clone().requires_grad_(first), y.clone().requires_grad_(second)]
        if kind == "gwc":
            fn, ref = (lambda p, q: build_gwc_volume(p, q, D, G_)), (lambda p, q: gwc64(p, q, D, G_))
            gvol = G(_synth.normal((B, G_, D, H, W), seed, "gvol"))
        else:
            masked = kind == "concat"
            fn = (lambda p, q: build_concat_volume(p, q, D)) if masked else (lambda p, q: build_concat_volume_igev(p, q, D))
            ref = lambda p, q: concat64(p, q, D, masked)  # noqa: E731
            gvol = G(_synth.normal((B, 2 * Cc, D, H, W), seed, "gvol"))
        with gwc_mode(mode):
            fn(*ins).backward(_upstream(gvol, up))
        want = grads64(ref, x, y, gvol)
    for i, (t, w) in enumerate(zip(ins, want)):
        if t.requires_grad:
            vol_check(t.grad, w, "%s input %d" % (kind, i))
        else:
            assert t.grad is None


# ---- sequence losses ----------------------------------------------------------------------------------------------------
LOSS_EDGE_HW = [(1, 1), (15, 17), (16, 16), (31, 33), (32, 32), (25, 41), (17, 241)]     # HW 1 .. 4097 around 256 / 1024


def _loss_inputs(seed, kind, K, B, H, W, n):
    rng = _synth.rng(seed, "loss", kind)
    hi = 230.0 if kind == "gwc" else 760.0                   # some ground truth beyond maxdisp = 192 / max_flow = 700
    targets = []
    first = rng.uniform(-10.0, hi, (B, 1, H, W)).astype(np.float32)
    for k in range(K):                                       # the second target (pseudo label) near the first
        gt = first.copy() if k == 0 else (first + rng.normal(0.0, 2.0, first.shape)).astype(np.float32)
        valid = rng.choice(np.array([0.0, 0.49, 0.5, 1.0], np.float32), (B, H, W))
        inf = (rng.random((B, H, W)) < 0.03) & (valid >= 0.5)
        gt[:, 0][inf] = np.where(rng.random(int(inf.sum())) < 0.5, np.inf, -np.inf)
        targets.append((gt, valid))
    base = first
    preds = [(base + rng.normal(0.0, 3.0, base.shape)).astype(np.float32) for _ in range(n)]
    return preds, targets


def _run_loss(kind, preds, targets, view):
    """The library loss on leaf predictions ([:, :1] views of 3-channel buffers when `view`); returns
    ([(loss, metrics, mask) per target], [grad per prediction] or None)."""
    from dkt_stereo_amd.loss import dkt_loss_pair, loss_gwcnet, sequence_loss_raft
    args = SimpleNamespace(maxdisp=192)
    leaves, ps = [], []
    for p in preds:
        if view:
            base = torch.zeros((p.shape[0], 3) + p.shape[-2:], device=DEV)
            base[:, 1:2] = 5.0
            base[:, :1] = G(p)
            base.requires_grad_(True)
            leaves.append(base)
            ps.append(base[:, :1])
        else:
            leaves.append(G(p).requires_grad_(True))
            ps.append(leaves[-1])
    res = {"disp_preds": ps}
    tg = [(G(gt), G(v)) for gt, v in targets]
    name = "sequence_loss_raft" if kind == "raft" else "loss_gwcnet"
    if len(targets) == 1:
        fn = sequence_loss_raft if kind == "raft" else loss_gwcnet
        outs = [fn(res, *tg[0], args=args)]
    else:
        l_gt, metrics, v_gt, l_pl, v_pl = dkt_loss_pair(name, res, *tg[0], *tg[1], args=args)
        outs = [(l_gt, metrics, v_gt), (l_pl, None, v_pl)]
    if outs[0][0] is None:
        return outs, None
    sum(o[0] for o in outs).backward()
    grads = [(lf.grad[:, :1] if view else lf.grad) for lf in leaves]
    if view:
        assert all(torch.equal(lf.grad[:, 1:], torch.zeros_like(lf.grad[:, 1:])) for lf in leaves)
    return outs, grads


def _check_loss(kind, preds, targets, outs, grads):
    max_flow = 192 if kind == "gwc" else 700
    n = len(preds)
    tp = [torch.from_numpy(p) for p in preds]
    union = None
    for k, ((gt, valid), (loss, metrics, mask)) in enumerate(zip(targets, outs)):
        gt_t, v_t = torch.from_numpy(gt), torch.from_numpy(valid)
        want_mask = R.loss_mask(gt_t, v_t, max_flow)
        assert mask.dtype == torch.bool and torch.equal(mask.cpu(), want_mask), k
        union = want_mask if union is None else union | want_mask
        N = int(want_mask.sum())
        want, mag = R.loss64(kind, tp, gt_t, v_t, max_flow)
        if N == 0:
            assert torch.isnan(loss).item(), k
        else:
            # RAFT: |p - g| (1 rounding), the mean to fp32 (1), fl32(w_i) (1), the product (1), n additions: (n + 4) u,
            # within 4 n u for n >= 2.  GwcNet: smooth-L1 (3), the mean (1), fl32(w_i) (1), the product (1), n_loss
            # additions: (n_loss + 6) u, within 4 max(n, 2) u for n_loss = min(n, 4).
            lim = 4 * max(n, 2) * U * mag
            assert abs(loss.item() - want) <= lim, (k, loss.item(), want, lim)
        if metrics is None:
            continue
        d = tp[-1][:, 0][want_mask[:, 0]] - gt_t[:, 0][want_mask[:, 0]]
        epe = torch.sqrt(d * d)                               # fp32 per pixel, as the reference
        for key, thr in (("1px", 1.0), ("3px", 3.0), ("5px", 5.0)):
            exact = np.float32(int((epe < thr).sum())) / np.float32(N) if N else np.float32("nan")
            assert isinstance(metrics[key], float)
            assert same(np.float32(metrics[key]), exact), (key, metrics[key], exact)
        if N == 0:
            assert np.isnan(metrics["epe"])
        else:
            w = np.float32(float(epe.double().mean()))
            assert abs(np.float32(metrics["epe"]) - w) <= np.spacing(w), (metrics["epe"], w)
    # gradients: exactly zero off the masks, within 3e-7 max|g| of fp32 torch autograd elsewhere
    leaves = [t.clone().requires_grad_(True) for t in tp]
    ref = 0
    for gt, valid in targets:
        gt_t, v_t = torch.from_numpy(gt), torch.from_numpy(valid)
        ref = ref + (R.torch_raft_loss(leaves, gt_t, v_t) if kind == "raft" else R.torch_gwc_loss(leaves, gt_t, v_t, 192))
    wg = torch.autograd.grad(ref, leaves, allow_unused=True)
    wg = [torch.zeros_like(t) if g is None else g for t, g in zip(tp, wg)]
    bound = 3e-7 * max(float(g.abs().max()) for g in wg)
    off = ~union
    n_loss = n if kind == "raft" else min(n, 4)
    for i, (a, b) in enumerate(zip(grads, wg)):
        a = a.cpu()
        assert torch.equal(a[off], torch.zeros_like(a[off])), i
        if i >= n_loss:
            assert torch.equal(a, torch.zeros_like(a)), i
        assert float((a - b).abs().max()) <= bound, (i, float((a - b).abs().max()), bound)


@settings(**SET)
@given(edge=st.one_of(st.sampled_from(LOSS_EDGE_HW), st.tuples(st.integers(1, 40), st.integers(1, 70))),
       B=st.integers(1, 4), n=st.integers(2, 64), K=st.integers(1, 2), view=st.booleans(), seed=st.integers(0, 10 ** 6))
@example(edge=(17, 241), B=2, n=63, K=2, view=True, seed=8)
@example(edge=(25, 41), B=3, n=64, K=1, view=False, seed=9)
@example(edge=(32, 32), B=1, n=64, K=2, view=False, seed=10)
def test_raft_loss_random(edge, B, n, K, view, seed):
    H, W = edge
    preds, targets = _loss_inputs(seed, "raft", K, B, H, W, n)
    outs, grads = _run_loss("raft", preds, targets, view)
    _check_loss("raft", preds, targets, outs, grads)


@settings(**SET)
@given(edge=st.one_of(st.sampled_from(LOSS_EDGE_HW), st.tuples(st.integers(1, 40), st.integers(1, 70))),
       B=st.integers(1, 4), n=st.integers(1, 8), K=st.integers(1, 2), view=st.booleans(), seed=st.integers(0, 10 ** 6))
@example(edge=(31, 33), B=2, n=7, K=2, view=True, seed=11)
def test_gwc_loss_random(edge, B, n, K, view, seed):
    H, W = edge
    preds, targets = _loss_inputs(seed, "gwc", K, B, H, W, n)
    outs, grads = _run_loss("gwc", preds, targets, view)
    _check_loss("gwc", preds, targets, outs, grads)


def test_raft_loss_nan_in_last_prediction():
    """A NaN (and no Inf) in prediction 63, on the last pixel of the last image: the reference returns
    (None, None, None); the pair returns None for both targets.  With an Inf beside it the loss goes on."""
    from dkt_stereo_amd.loss import dkt_loss_pair, sequence_loss_raft
    preds, targets = _loss_inputs(12, "raft", 2, 3, 17, 241, 64)
    preds[63][-1, 0, -1, -1] = np.nan
    res = {"disp_preds": [G(p) for p in preds]}
    (g0, v0), (g1, v1) = [(G(gt), G(v)) for gt, v in targets]
    assert sequence_loss_raft(res, g0, v0) == (None, None, None)
    assert dkt_loss_pair("sequence_loss_raft", res, g0, v0, g1, v1) == (None,) * 5
    preds[63][0, 0, 0, 0] = np.inf
    res = {"disp_preds": [G(p) for p in preds]}
    assert sequence_loss_raft(res, g0, v0)[0] is not None
    assert all(x is not None for x in dkt_loss_pair("sequence_loss_raft", res, g0, v0, g1, v1))


def test_loss_pair_recipe_shape():
    """B = 2 at 480 x 896, 16 predictions, two targets: 840 blocks, so the finalize pass runs its 8-wide loop.
    Checked against float64 and fp32 autograd, and run twice: bit-identical."""
    preds, targets = _loss_inputs(13, "raft", 2, 2, 480, 896, 16)
    runs = []
    for _ in range(2):
        outs, grads = _run_loss("raft", preds, targets, True)
        runs.append(([o[0].item() for o in outs], outs[0][1], [o[2].cpu() for o in outs], [g.cpu() for g in grads]))
    _check_loss("raft", preds, targets, outs, grads)
    (l1, m1, k1, g1), (l2, m2, k2, g2) = runs
    assert l1 == l2 and m1 == m2
    assert all(torch.equal(x, y) for x, y in zip(k1 + g1, k2 + g2))


# ---- F&E ----------------------------------------------------------------------------------------------------------------
def _seed(s):
    torch.manual_seed(s)
    random.seed(s)


def _next_draws():
    return np.array([torch.rand(1).item(), random.random()])


def _fande_inputs(seed, B, H, W):
    """Image b plays role b % 4.  0: valid pixels only past the first 65,536 (only a count pass that strides sees them),
    all consistent but the last, so the ratio is just below 1; 1: no valid pixel (0/0: never selected); 2: consistent
    everywhere; 3: NaN and +-Inf in source and target."""
    assert H * W > 65536
    rng = _synth.rng(seed, "fande")
    t = rng.uniform(0.0, 60.0, (B, 1, H, W)).astype(np.float32)
    gt = (t + rng.normal(0.0, 3.0, t.shape)).astype(np.float32)
    pl = (t + rng.normal(0.0, 1.5, t.shape)).astype(np.float32)
    valid = (rng.random((B, H, W)) < 0.7).astype(np.float32)
    for b in range(B):
        role = b % 4
        if role == 0:
            v, g = valid[b].reshape(-1), gt[b].reshape(-1)
            v[:65536], v[65536:] = 0.0, 1.0
            g[65536:] = t[b].reshape(-1)[65536:]
            g[-1] += 10.0
        elif role == 1:
            valid[b] = 0.0
        elif role == 2:
            gt[b], valid[b] = t[b], 1.0
        else:
            for a in (gt, pl, t):
                flat = a[b].reshape(-1)
                idx = rng.choice(flat.size, 6, replace=False)
                flat[idx] = np.array([np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf], np.float32)
    return gt, pl, t, valid


def _check_stride_images(rand, out_valid, H, W):
    """The role-0 images are selected (their draw is below the ratio), so their inconsistent last pixel stays valid: a
    count pass that stopped at 65,536 pixels would see 0/0 and drop it."""
    for b in range(0, rand.shape[0], 4):
        assert float(rand[b]) < 1.0 - 1.0 / (H * W - 65536), "pick a seed whose draw selects image %d" % b
        assert float(out_valid[b].reshape(-1)[-1]) == 1.0, b


def same_torch(a, b):
    return same(a, b.detach().cpu())


@pytest.mark.parametrize("B,H,W", [(4, 300, 400), (2, 480, 896)])
def test_fande_filter_and_ensemble_multiblock(B, H, W):
    from dkt_stereo_amd.fande import FandE_Ensemble, FandE_Filter
    gt, _, t, valid = _fande_inputs(14, B, H, W)
    s_, t_, v_ = (torch.from_numpy(x) for x in (gt, t, valid[:, None]))
    _seed(3)
    out, out_valid = FandE_Filter(G(gt), G(t), G(valid[:, None]), withprob=True, threshold=3.0)
    got_next = _next_draws()
    _seed(3)
    rand = torch.rand((B, 1))
    ws, wv = R.torch_filter(s_, t_, v_, 3.0, rand)
    assert np.array_equal(got_next, _next_draws())
    assert same_torch(out, ws) and same_torch(out_valid, wv[:, 0])
    _check_stride_images(rand, out_valid, H, W)
    for clamp in (False, 1.0):
        _seed(4)
        out = FandE_Ensemble(G(gt), G(t), G(valid[:, None]), clamp=clamp, threshold=3.0)
        got_next = _next_draws()
        _seed(4)
        want = R.torch_ensemble(s_, t_, v_, 3.0, random.random(), clamp)
        assert np.array_equal(got_next, _next_draws())
        assert same_torch(out, want), clamp


@pytest.mark.parametrize("B,H,W", [(4, 300, 400), (2, 480, 896), (64, 260, 260)])
def test_fande_targets_multiblock(B, H, W):
    """The two-job launch at multi-block shapes; B = 64 is DKT_FANDE_MAX_B."""
    from dkt_stereo_amd.fande import fande_targets
    gt, pl, t, valid = _fande_inputs(15, B, H, W)
    _seed(5)
    outs = fande_targets(G(gt), G(valid), G(pl), G(t), 3.0, 1.0, 1.0)
    got_next = _next_draws()
    _seed(5)
    rand, p_gt, p_pl = torch.rand((B, 1)), random.random(), random.random()
    want = R.torch_targets(*(torch.from_numpy(x) for x in (gt, valid, pl, t)), 3.0, 1.0, 1.0, rand, p_gt, p_pl)
    assert np.array_equal(got_next, _next_draws())
    for i, (a, b) in enumerate(zip(outs, want)):
        assert same_torch(a, b), i
    _check_stride_images(rand, outs[1], H, W)
