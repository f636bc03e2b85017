"""DKT's Filter-and-Ensemble and the stereo sequence losses on the device (dkt_stereo_amd.fande / .loss) against the
reference's own results (tests/golden/dkt.npz, written by make_golden_dkt.py), plus the library's own properties:
determinism, the fused GT + PL pair against two calls, the synchronisation budget, and one tiny DKT step through a RAFT
student.

F&E outputs are compared bit for bit (NaN compared by position: the NaN of a product such as 0 * Inf has no defined sign).
Gt = +-Inf on a pixel whose valid is 1 never reaches the loss (mag < max_flow excludes it), so the reference's None of
loss.py:17 and the assertion of gwc_loss.py:13 cannot fire; the fixture's raft_maxflow case holds such a pixel."""
import random
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from _train_ref import torch_raft_loss as _torch_raft_loss
from _train_ref import torch_targets as _torch_targets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    a = a.detach().cpu().float().contiguous()
    b = torch.as_tensor(np.ascontiguousarray(b)).float()
    if a.shape != b.shape:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32))


def _cases(golden, prefix):
    z = golden("dkt")
    return sorted({k.rsplit("/", 1)[0] for k in z.files if k.startswith(prefix)})


def _get(golden, case):
    z = golden("dkt")
    return lambda name: z[case + "/" + name]


def _seed(s):
    torch.manual_seed(s)
    random.seed(s)


def _next_draws():
    return np.array([torch.rand(1).item(), random.random()])


def _strided(a, channels=3, at=1):
    """`a` (B, ...) as channel `at` of a (B, channels, ...) buffer: a view with a batch stride, planes contiguous."""
    t = G(a)
    buf = torch.full((t.shape[0], channels) + tuple(t.shape[-2:]), 12345.0, device=DEV)
    buf[:, at] = t.reshape(t.shape[0], *t.shape[-2:])
    return buf[:, at:at + 1] if t.dim() == 4 else buf[:, at]


# ---- F&E ----------------------------------------------------------------------------------------------------------------
def test_fande_dropins_match_reference(golden):
    from dkt_stereo_amd.fande import FandE_Ensemble, FandE_Filter
    n = 0
    for case in _cases(golden, "fande/filter_") + _cases(golden, "fande/ensemble_"):
        g = _get(golden, case)
        seed, tau, opt = g("meta")
        for view in (False, True):
            src, tgt, valid = (_strided(g(k)) if view else G(g(k)) for k in ("src", "tgt", "valid"))
            _seed(int(seed))
            if "filter_" in case:
                out, out_valid = FandE_Filter(src, tgt, valid, withprob=bool(opt), threshold=tau)
                assert same_bits(out_valid, g("out_valid")), (case, view)
            else:
                out = FandE_Ensemble(src, tgt, valid, clamp=(opt if opt else False), threshold=tau)
            assert same_bits(out, g("out")), (case, view)
            assert np.array_equal(_next_draws(), g("next")), (case, view)
            n += 1
    assert n == 48


def test_fande_targets_match_reference(golden):
    from dkt_stereo_amd.fande import fande_targets
    cases = _cases(golden, "fande/fused_")
    assert len(cases) == 3
    for case in cases:
        g = _get(golden, case)
        seed, tau_gt, tau_pl, clamp = g("meta")
        for view in (False, True):
            conv = _strided if view else G
            _seed(int(seed))
            outs = fande_targets(conv(g("disp_gt")), conv(g("valid_gt")), conv(g("disp_pl")), conv(g("disp_t_ema")),
                                 tau_gt, tau_pl, clamp if clamp else False)
            for got, name in zip(outs, ("disp_gt_aug", "valid_gt_aug", "disp_pl_aug", "valid_pl_aug")):
                assert same_bits(got, g(name)), (case, name, view)
            assert np.array_equal(_next_draws(), g("next")), case


def _count_syncs(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            out = fn()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    return out, [str(r.message) for r in rec if "called a synchronizing" in str(r.message)]


def test_fande_targets_makes_no_synchronising_call():
    from dkt_stereo_amd.fande import fande_targets
    torch.manual_seed(3)
    B, H, W = 2, 48, 96
    t = torch.rand(B, 1, H, W, device=DEV) * 40
    gt = t + torch.randn(B, 1, H, W, device=DEV) * 3
    pl = t + torch.randn(B, 1, H, W, device=DEV)
    v = (torch.rand(B, H, W, device=DEV) < 0.8).float()
    fande_targets(gt, v, pl, t, 3.0, 3.0, 1.0)                  # warm: library load, allocator
    _, syncs = _count_syncs(lambda: fande_targets(gt, v, pl, t, 3.0, 3.0, 1.0))
    assert syncs == [], syncs


# ---- losses -------------------------------------------------------------------------------------------------------------
def _loss_call(g, view, upstream=1.7):
    """Runs the library loss of fixture case `g` on leaf predictions; returns (result triple, grads of upstream * loss)."""
    from dkt_stereo_amd.loss import loss_gwcnet, sequence_loss_raft
    kind, gamma, max_flow, maxdisp = g("meta")
    leaves, preds = [], []
    for p in g("preds"):
        if view:
            base = torch.zeros((p.shape[0], 2) + p.shape[-2:], device=DEV)
            base[:, :1] = G(p)
            base.requires_grad_(True)
            leaves.append(base)
            preds.append(base[:, :1])
        else:
            leaf = G(p).requires_grad_(True)
            leaves.append(leaf)
            preds.append(leaf)
    res = {"disp_preds": preds}
    if kind == 0:
        out = sequence_loss_raft(res, G(g("gt")), G(g("valid")), loss_gamma=gamma, max_flow=max_flow)
    else:
        out = loss_gwcnet(res, G(g("gt")), G(g("valid")), args=SimpleNamespace(maxdisp=int(maxdisp)))
    if out[0] is None:
        return out, None
    (upstream * out[0]).backward()
    grads = [(lf.grad[:, :1] if view else lf.grad) for lf in leaves]
    if view:
        assert all(torch.equal(lf.grad[:, 1:], torch.zeros_like(lf.grad[:, 1:])) for lf in leaves)
    return out, grads


def test_losses_match_reference(golden):
    cases = _cases(golden, "loss/")
    assert len(cases) >= 14
    for case in cases:
        g = _get(golden, case)
        for view in (False, True):
            (loss, metrics, mask), grads = _loss_call(g, view)
            if bool(g("none")):
                assert loss is None and metrics is None and mask is None, case
                continue
            want = float(g("loss"))
            if np.isnan(want):
                assert torch.isnan(loss).item(), case
            else:
                assert abs(loss.item() - want) <= 2e-6 * abs(want), (case, loss.item(), want)
            for k, w in zip(("epe", "1px", "3px", "5px"), g("metrics")):
                assert isinstance(metrics[k], float)
                if np.isnan(w):
                    assert np.isnan(metrics[k]), (case, k)
                else:
                    assert abs(metrics[k] - w) <= 1e-6 * max(1.0, abs(w)), (case, k, metrics[k], w)
            assert mask.dtype == torch.bool and torch.equal(mask.cpu(), torch.from_numpy(g("mask"))), case
            wg = torch.from_numpy(g("grads"))
            bound = 3e-7 * float(wg.abs().max())
            off = ~torch.from_numpy(g("mask"))
            for i, (a, b) in enumerate(zip(grads, wg)):
                a = a.cpu()
                assert float((a - b).abs().max()) <= bound, (case, view, i, float((a - b).abs().max()), bound)
                assert torch.equal(a[off], torch.zeros_like(a[off])), (case, i)


def test_loss_edge_behaviour():
    from dkt_stereo_amd.loss import loss_gwcnet, sequence_loss_raft
    gt = torch.full((1, 1, 8, 16), 5.0, device=DEV)
    valid = torch.ones(1, 8, 16, device=DEV)
    p = (gt + 1).requires_grad_(True)
    with pytest.raises(ZeroDivisionError):                      # n = 1: loss_gamma**(15/0)
        sequence_loss_raft({"disp_preds": [p]}, gt, valid)
    q = p.detach().clone()
    q[0, 0, 0, 0] = float("nan")
    assert sequence_loss_raft({"disp_preds": [q]}, gt, valid) == (None, None, None)      # None comes first
    with pytest.raises(AssertionError):                         # n_predictions >= 1
        sequence_loss_raft({"disp_preds": []}, gt, valid)
    with pytest.raises(AssertionError):                         # valid must be (B, H, W)
        sequence_loss_raft({"disp_preds": [p, p]}, gt, valid[:, None])
    loss, metrics, mask = loss_gwcnet({"disp_preds": [p] * 5}, gt, valid, args=SimpleNamespace(maxdisp=192))
    assert abs(loss.item() - (0.5 + 0.5 + 0.7 + 1.0) * 0.5) <= 1e-6 and metrics["epe"] == 1.0    # zip() stops at 4 weights
    gt_inf = gt.clone()
    gt_inf[0, 0, 1, 1] = float("inf")                           # excluded by mag < max_flow: no assertion, no None
    l1, _, m1 = loss_gwcnet({"disp_preds": [p]}, gt_inf, valid, args=SimpleNamespace(maxdisp=192))
    l2, _, m2 = sequence_loss_raft({"disp_preds": [p, p]}, gt_inf, valid)
    assert not m1[0, 0, 1, 1] and not m2[0, 0, 1, 1] and l1.item() == 0.25 and np.isfinite(l2.item())
    with pytest.raises(AssertionError):                         # predictions must have the target's shape
        sequence_loss_raft({"disp_preds": [p, p[:, :, :4]]}, gt, valid)


def test_losses_are_deterministic(golden):
    for case in ("loss/raft_n16_g0.9", "loss/gwc_n4"):
        g = _get(golden, case)
        first = None
        for _ in range(20):
            (loss, _, _), grads = _loss_call(g, True)
            got = [loss.detach().cpu()] + [x.cpu() for x in grads]
            if first is None:
                first = got
            else:
                assert all(torch.equal(a, b) for a, b in zip(first, got)), case


def _pair_inputs(seed, B=2, H=40, W=72, n=5):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    R = lambda *s: torch.rand(*s, generator=gen)          # noqa: E731
    gt = (R(B, 1, H, W) * 60).to(DEV)
    pl = (gt.cpu() + torch.randn(B, 1, H, W, generator=gen) * 2).to(DEV)
    vgt = (R(B, H, W) < 0.7).float().to(DEV)
    vpl = (R(B, H, W) < 0.9).float().to(DEV)
    bases = [(gt.cpu().repeat(1, 2, 1, 1) + torch.randn(B, 2, H, W, generator=gen) * 5).to(DEV).requires_grad_(True)
             for _ in range(n)]
    return gt, vgt, pl, vpl, bases


@pytest.mark.parametrize("name", ["sequence_loss_raft", "loss_gwcnet"])
def test_loss_pair_equals_two_calls(name):
    from dkt_stereo_amd.loss import __losses__, dkt_loss_pair
    args = SimpleNamespace(maxdisp=48)
    gt, vgt, pl, vpl, bases = _pair_inputs(5)
    res = {"disp_preds": [b[:, :1] for b in bases]}
    l_gt, metrics, v_gt, l_pl, v_pl = dkt_loss_pair(name, res, gt, vgt, pl, vpl, args=args)
    (l_gt + l_pl * 1.0).backward()
    pair_grads = [b.grad.clone() for b in bases]
    for b in bases:
        b.grad = None
    fn = __losses__[name]
    a_gt, a_metrics, a_v = fn(res, gt, vgt, args=args)
    a_pl, _, a_vpl = fn(res, pl, vpl, args=args)
    assert torch.equal(l_gt, a_gt) and torch.equal(l_pl, a_pl)
    assert metrics == a_metrics and torch.equal(v_gt, a_v) and torch.equal(v_pl, a_vpl)
    g_gt = torch.autograd.grad(a_gt, bases, retain_graph=True)
    g_pl = torch.autograd.grad(a_pl * 1.0, bases)
    for p, a, b in zip(pair_grads, g_gt, g_pl):
        assert torch.equal(p, a + b)


def test_loss_pair_one_synchronising_call():
    from dkt_stereo_amd.loss import dkt_loss_pair
    gt, vgt, pl, vpl, bases = _pair_inputs(6, n=16)
    res = {"disp_preds": [b[:, :1] for b in bases]}

    def step():
        l_gt, _, _, l_pl, _ = dkt_loss_pair("sequence_loss_raft", res, gt, vgt, pl, vpl)
        (l_gt + l_pl * 1.0).backward()

    step()                                                      # warm
    _, syncs = _count_syncs(step)
    assert len(syncs) <= 1, syncs


# ---- a tiny DKT step ----------------------------------------------------------------------------------------------------
def test_dkt_step_end_to_end():
    """Teacher (library test_mode) -> fande_targets -> RAFT student (3 iterations, 64 x 128, under autograd) ->
    dkt_loss_pair -> parameter gradients, against the same student tensors through the torch restatement of _train_ref.py."""
    import _cases
    import _synth
    from dkt_stereo_amd.fande import fande_targets
    from dkt_stereo_amd.loss import dkt_loss_pair
    from dkt_stereo_amd.raft_stereo import RAFTStereo, make_args
    model = RAFTStereo(make_args())
    model.load_state_dict(_synth.torch_state_dict(_synth.shapes_of(model), _cases.E2E_WEIGHT_SEED), strict=True)
    model.to(DEV).eval()
    names = ["update_block.gru08.convz.weight", "update_block.flow_head.conv2.weight", "update_block.mask.2.weight",
             "context_zqr_convs.0.weight"]
    for n, p in model.named_parameters():
        p.requires_grad_(n in names)
    i1, i2 = (G(a) for a in _synth.image_pair(5, 2, 64, 128, 12))
    with torch.no_grad():
        _, disp_t = model(i1, i2, iters=3, test_mode=True)
    gen = torch.Generator(device="cpu").manual_seed(21)
    disp_gt = disp_t + (torch.randn(disp_t.shape, generator=gen) * 2).to(DEV)
    disp_pl = disp_t + (torch.randn(disp_t.shape, generator=gen) * 0.5).to(DEV)
    valid_gt = (torch.rand(disp_t.shape[0], 64, 128, generator=gen) < 0.8).float().to(DEV)
    _seed(17)
    targets = fande_targets(disp_gt, valid_gt, disp_pl, disp_t, 3.0, 1.0, 1.0)
    _seed(17)
    rand, p_gt, p_pl = torch.rand((2, 1)), random.random(), random.random()
    want = _torch_targets(disp_gt, valid_gt, disp_pl, disp_t, 3.0, 1.0, 1.0, rand, p_gt, p_pl)
    for a, b in zip(targets, want):
        assert same_bits(a, b.cpu().numpy())
    preds = model(i1, i2, iters=3, test_mode=False)["disp_preds"]
    params = [dict(model.named_parameters())[n] for n in names]
    l_gt, _, _, l_pl, _ = dkt_loss_pair("sequence_loss_raft", {"disp_preds": preds}, *targets)
    got = torch.autograd.grad(l_gt + l_pl * 1.0, params, retain_graph=True)
    ref = _torch_raft_loss(preds, targets[0], targets[1]) + _torch_raft_loss(preds, targets[2], targets[3]) * 1.0
    assert abs((l_gt + l_pl).item() - ref.item()) <= 2e-6 * abs(ref.item())
    wantg = torch.autograd.grad(ref, params)
    for n, a, b in zip(names, got, wantg):
        rel = float((a - b).abs().max() / b.abs().max())
        assert rel <= 1e-5, (n, rel)
