"""The soft-argmin heads on the device (-m gpu): dkt_soft_argmin_fwd / _bwd through the raw entries and through
soft_argmin's autograd node, against the float64 truth of _soft_argmin_ref.py under its bounds

    bound_out   = 2 eps e_E,                         e_E = A (7.75 Z + 1) + E (2 sqrt(n) + 1),  n = 1.25 D + 1, eps = 2^-23
    bound_gcost = 2 eps T(|g| p (c_u |d - E| + e_E)), c_u = 15.5 Z + sqrt(n) + sqrt(n_t) + 5,    n_t = 8 (2f)^2 (1 at f = 1)

per element, from the truth's own E, A = sum_d p_d |d - E| and Z = the largest |cost| the pixel reads
(test_host_soft_argmin_ref.py shows torch's own fp32 chain inside them and every mutant outside); repeatability and sign to
the bit, the accepted layouts, the peak memory of a forward + backward, and GWCNet with the handle on against off.  Each
case prints the kernels' share of the bounds (run with -s)."""
import copy

import numpy as np
import pytest
import torch

import _cases
import _soft_argmin_ref as R
import _synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cost(name):
    """The case's cost on the device as the case wants it laid out: (tensor, batch stride)."""
    c, cost = R.CASES[name], G(R.reference(name)["cost"])
    if c.get("strided"):
        buf = torch.full((2 * c["B"],) + tuple(cost.shape[1:]), float("nan"), device=DEV)
        buf[::2] = cost
        return buf[::2], 2 * cost[0].numel()
    return cost, cost[0].numel()


def _raw(name, out_scale=1.0):
    """(out, gcost) through the three C entries, every buffer poisoned first."""
    from dkt_stereo_amd import _ffi
    lib, c = _ffi.lib(), R.CASES[name]
    cost, cbs = _cost(name)
    gout = G(R.reference(name)["gout"])
    B, Dc, h, w, f = c["B"], c["Dc"], c["h"], c["w"], c["f"]
    nan = float("nan")
    out = torch.full((B, 1, f * h, f * w), nan, device=DEV)
    gcost = torch.full((B, Dc, h, w), nan, device=DEV)
    nbytes = lib.dkt_soft_argmin_bwd_workspace(B, Dc, h, w, f)
    assert nbytes == (4 * B * Dc * 16 * h * w if f == 4 else 0)
    ws = torch.full((nbytes // 4,), nan, device=DEV) if nbytes else None
    dev, st = _ffi.device_of(cost), _ffi.stream_of(cost)
    _ffi.check(lib.dkt_soft_argmin_fwd(cost.data_ptr(), cbs, out_scale, out.data_ptr(), B, Dc, h, w, f, dev, st), "dkt_soft_argmin_fwd")
    _ffi.check(lib.dkt_soft_argmin_bwd(gout.data_ptr(), f * h * f * w, cost.data_ptr(), cbs, out_scale, gcost.data_ptr(),
                                       _ffi.ptr(ws), B, Dc, h, w, f, dev, st), "dkt_soft_argmin_bwd")
    return out, gcost


def _node(name, out_scale=1.0, five=False):
    """(out, gcost) through soft_argmin under autograd."""
    from dkt_stereo_amd.soft_argmin import soft_argmin
    cost, _ = _cost(name)
    leaf = cost.detach().requires_grad_(True)                                   # (a view of the wider buffer for "strided")
    out = soft_argmin(leaf[:, None] if five else leaf, R.CASES[name]["f"], out_scale)
    assert out.requires_grad and type(out.grad_fn).__name__ == "_SoftArgminFnBackward"
    out.backward(G(R.reference(name)["gout"]))
    return out.detach(), leaf.grad


@pytest.mark.parametrize("name", list(R.CASES))
def test_fixed_cases(name):
    """Forward and backward of every case under the bounds, through the raw entries and through the node; the two give the
    same bits, and so does a second run."""
    ref = R.reference(name)
    raw, node = _raw(name), _node(name)
    for how, (out, gcost) in (("raw", raw), ("node", node)):
        assert out.shape == ref["out"].shape and gcost.shape == ref["gcost"].shape
        ro, rg = R.worst(out, ref["out"], ref["bound_out"]), R.worst(gcost, ref["gcost"], ref["bound_gcost"])
        print("%-8s %-4s out %.4f of the bound (<= %.3e), gcost %.4f of the bound (<= %.3e)"
              % (name, how, ro, float(ref["bound_out"].max()), rg, float(ref["bound_gcost"].max())))
        assert ro <= 1.0 and rg <= 1.0, (name, how, ro, rg)
    assert R.same(raw[0], node[0]) and R.same(raw[1], node[1]), name
    again = _raw(name)
    assert R.same(raw[0], again[0]) and R.same(raw[1], again[1]), name


def test_dc1_is_exact():
    out, gcost = _raw("dc1")
    assert bool((out == 1.5).all()) and bool((gcost == 0).all())


@pytest.mark.parametrize("name", ["tiles", "f1", "spike"])
def test_out_scale_minus_one_negates_the_bits(name):
    pos, neg = _raw(name, 1.0), _raw(name, -1.0)
    assert R.same(neg[0], -pos[0]) and R.same(neg[1], -pos[1]), name
    ref = R.reference(name, -1.0)
    assert R.worst(neg[0], ref["out"], ref["bound_out"]) <= 1.0 and R.worst(neg[1], ref["gcost"], ref["bound_gcost"]) <= 1.0


def _count_backward_calls(monkeypatch):
    """[1 per call of dkt_soft_argmin_bwd], from whichever thread (autograd runs the backward on one of its own, which
    _ffi.launch_log does not see)."""
    from dkt_stereo_amd import _ffi
    lib, calls = _ffi.lib(), []
    real = lib.dkt_soft_argmin_bwd

    def counted(*args):
        calls.append(1)
        return real(*args)
    monkeypatch.setattr(lib, "dkt_soft_argmin_bwd", counted)
    return calls


def test_no_gradient_wanted_launches_no_backward(monkeypatch):
    from dkt_stereo_amd import _ffi
    from dkt_stereo_amd.soft_argmin import soft_argmin
    calls = _count_backward_calls(monkeypatch)
    cost, gout = G(R.reference("tiles")["cost"]), G(R.reference("tiles")["gout"])
    with _ffi.launch_log() as names:
        out = soft_argmin(cost, 4, -1.0)                                        # nothing requires grad: the plain call
        assert out.grad_fn is None and not out.requires_grad
        scale = torch.ones((), device=DEV, requires_grad=True)
        (soft_argmin(cost, 4, -1.0) * scale).backward(gout)                     # a graph around it, none through it
        assert scale.grad is not None
        with torch.no_grad():
            quiet = soft_argmin(cost.clone().requires_grad_(True), 4, -1.0)
        assert quiet.grad_fn is None and R.same(quiet, out)
    torch.cuda.synchronize()
    assert names == ["dkt_soft_argmin_fwd"] * 3 and calls == []
    leaf = cost.clone().requires_grad_(True)
    soft_argmin(leaf, 4, -1.0).backward(gout)
    assert calls == [1] and leaf.grad is not None


@pytest.mark.parametrize("name", ["batch2", "f1"])
def test_layouts_give_the_same_bits(name):
    """(B, 1, D, h, w), a batch-strided view (read in place) and a W-major cost (copied) against the contiguous form; fp16
    inputs are cast and get fp16 gradients."""
    from dkt_stereo_amd.soft_argmin import _batch_strided, soft_argmin
    ref, f = R.reference(name), R.CASES[name]["f"]
    base = _node(name)
    five = _node(name, five=True)
    assert R.same(base[0], five[0]) and R.same(base[1], five[1])
    cost, gout = G(ref["cost"]), G(ref["gout"])
    wide = torch.zeros((cost.shape[0], 3) + tuple(cost.shape[1:]), device=DEV)
    wide[:, 1] = cost
    view, bstride = _batch_strided(wide[:, 1])
    assert view.data_ptr() == wide[:, 1].data_ptr() and bstride == 3 * cost[0].numel()
    for layout in (wide[:, 1], cost.transpose(2, 3).contiguous().transpose(2, 3)):
        leaf = layout.detach().requires_grad_(True)
        out = soft_argmin(leaf, f)
        out.backward(gout)
        assert R.same(out.detach(), base[0]) and R.same(leaf.grad.contiguous(), base[1])
    half = cost.half().requires_grad_(True)
    out = soft_argmin(half, f)
    assert out.dtype == torch.float32
    out.backward(gout)
    assert half.grad.dtype == torch.float16


def test_peak_memory_stays_below_half_an_upsampled_volume():
    """Forward + backward at (1, 48, 16, 32), f = 4: the node allocates the quarter-size workspace and a few maps, the torch
    chain more than two up-sampled volumes (so the first assertion cannot pass vacuously)."""
    from dkt_stereo_amd.soft_argmin import soft_argmin
    volume = 192 * 64 * 128 * 4
    cost = G(_synth.normal((1, 48, 16, 32), 421, "cost", scale=3.0))
    gout = G(_synth.normal((1, 1, 64, 128), 421, "gout"))

    def peak(fn):
        leaf = cost.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn(leaf).backward(gout)
        torch.cuda.synchronize()
        assert leaf.grad is not None
        return torch.cuda.max_memory_allocated() - base

    node = peak(lambda c: soft_argmin(c, 4, -1.0))
    chain = peak(lambda c: R.torch_chain_graph(c, 4, -1.0))
    print("peak over the start: node %.3f, torch chain %.3f up-sampled volumes" % (node / volume, chain / volume))
    assert node < 0.5 * volume
    assert chain > 2.0 * volume


def _gwcnet_pair():
    from dkt_stereo_amd.gwcnet import GWCNet, make_args
    m = GWCNet(make_args(use_concat_volume=True))
    m.load_state_dict(_synth.torch_state_dict(_synth.shapes_of(m), _cases.GWCNET_WEIGHT_SEED), strict=True)
    m = m.to(DEV)
    return m, copy.deepcopy(m)


def _largest_cost(model, store):
    """Hooks that record max|cost| of every head that runs."""
    def hook(_, __, y):
        store.append(float(y.detach().abs().max()))
    return [getattr(model, "classif%d" % i)[2].register_forward_hook(hook) for i in range(4)]


def test_gwcnet_with_the_handle_on_against_off(monkeypatch):
    """GWCNet at 1 x 3 x 64 x 128, same weights, deterministic vendor algorithms.  train(): the four predictions within
    twice bound_fwd (M the largest cost of any head), classif0..3.2.weight.grad within 2e-2 of the tensor's maximum (the
    bound of test_gpu_gwcnet_train.py); eval() / test_mode=True: the prediction within twice bound_fwd."""
    from dkt_stereo_amd import _ffi, gwcnet
    i1, i2 = (G(a) for a in _synth.image_pair(7, 1, 64, 128, 12))
    gt = G(-_synth.uniform((1, 1, 64, 128), 0.0, 40.0, 7, "gt"))
    on, off = _gwcnet_pair()
    calls = _count_backward_calls(monkeypatch)
    costs = []
    hooks = _largest_cost(on, costs) + _largest_cost(off, costs)
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        res = {}
        for flag, model in ((True, on), (False, off)):
            monkeypatch.setattr(gwcnet, "SOFT_ARGMIN_HIP", flag)
            model.train()
            with _ffi.launch_log() as names:
                preds = model(i1, i2)["disp_preds"]
                sum(w * torch.nn.functional.smooth_l1_loss(p, gt) for p, w in zip(preds, (0.5, 0.5, 0.7, 1.0))).backward()
            assert names.count("dkt_soft_argmin_fwd") == (4 if flag else 0) and len(calls) == 4   # (the four of the first pass)
            model.eval()
            with _ffi.launch_log() as names:
                none, disp = model(i1, i2, test_mode=True)
            assert none is None and names.count("dkt_soft_argmin_fwd") == (1 if flag else 0)
            res[flag] = ([p.detach() for p in preds], disp)
        torch.cuda.synchronize()
    finally:
        torch.backends.cudnn.deterministic = was
        for h in hooks:
            h.remove()
    bound = 2.0 * R.bound_fwd(192, max(costs), -1.0)
    for i, (a, b) in enumerate(zip(res[True][0], res[False][0])):
        d = float((a - b).abs().max())
        print("train pred%d: on - off %.3e (twice bound_fwd %.3e, max|cost| %.1f)" % (i, d, bound, max(costs)))
        assert a.shape == b.shape == (1, 1, 64, 128) and d <= bound
    d = float((res[True][1] - res[False][1]).abs().max())
    print("eval: on - off %.3e (twice bound_fwd %.3e)" % (d, bound))
    assert d <= bound
    pon, poff = dict(on.named_parameters()), dict(off.named_parameters())
    for i in range(4):
        k = "classif%d.2.weight" % i
        rel = float((pon[k].grad - poff[k].grad).abs().max() / poff[k].grad.abs().max())
        print("grad %s: on - off %.3e of the maximum" % (k, rel))
        assert rel <= 2e-2, k
