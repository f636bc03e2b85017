"""CGI-Stereo's top-k disparity head on the device (-m gpu): dkt_topk_regress_fwd / _bwd through the raw entries and through
regression_topk's autograd node, against the float64 truth of _topk_ref.py under its bounds

    bound_out      = 2 u e_pred + TINY sum |s|,                  e_pred = sum_j p_j |s_j| (c_j + K + 1),  c_i = |t_i| + T + K + 5
    bound_gcost    = 2 u |g| p_i ((c_i + 4) |s_i - pred| + e_pred + |s_i|) + 2 TINY |g| sum |s|   (0 off the kept planes)
    bound_gsamples = 2 u |g| p_i (c_i + 1) + TINY |g|                                            (0 off the kept planes)

per element, u = 2^-24 (test_host_topk_ref.py shows torch's own fp32 chain inside them and every mutant outside); the saved
plane indices against the stable sort's without any tolerance; repeatability to the bit; the NaN pixel; the refusals; what a
forward under autograd keeps allocated; and cgi_disparity_head against the reference's lines in float64.  Each case prints the
kernels' share of the bounds (run with -s)."""
import numpy as np
import pytest
import torch

import _context_upsample_ref as CU
import _synth
import _topk_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("out", "gcost", "gsamples")


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _operands(name):
    """(cost, samples or None, gout) on the device as the case wants them laid out: the strided case as every second image of
    buffers of four, the images in between being other data."""
    ref = R.reference(name)
    samples = None if ref["samples"] is None else G(ref["samples"])
    if R.CASES[name].get("strided"):
        return G(ref["wide_cost"])[::2], samples, G(ref["wide_gout"])[::2]
    return G(ref["cost"]), samples, G(ref["gout"])


def _bstride(t):
    return t.stride(0) if t.shape[0] > 1 else t[0].numel()


def _raw(name):
    """dict(out, gcost, gsamples, idx) through the two C entries, every output buffer poisoned first."""
    from dkt_stereo_amd import _ffi
    lib, c = _ffi.lib(), R.CASES[name]
    cost, samples, gout = _operands(name)
    B, D, h, w, k = c["B"], c["D"], c["h"], c["w"], c["k"]
    nan = float("nan")
    out = torch.full((B, 1, h, w), nan, device=DEV)
    idx = torch.full((B, k, h, w), 255, device=DEV, dtype=torch.uint8)
    gcost = torch.full((B, D, h, w), nan, device=DEV)
    gsamples = None if samples is None else torch.full((B, D, h, w), nan, device=DEV)
    sbs = 0 if samples is None else _bstride(samples)
    dev, st = _ffi.device_of(cost), _ffi.stream_of(cost)
    _ffi.check(lib.dkt_topk_regress_fwd(cost.data_ptr(), _bstride(cost), _ffi.ptr(samples), sbs, out.data_ptr(), idx.data_ptr(),
                                        B, D, h, w, k, dev, st), "dkt_topk_regress_fwd")
    _ffi.check(lib.dkt_topk_regress_bwd(gout.data_ptr(), _bstride(gout), cost.data_ptr(), _bstride(cost), _ffi.ptr(samples), sbs,
                                        idx.data_ptr(), gcost.data_ptr(), _ffi.ptr(gsamples), B, D, h, w, k, dev, st), "dkt_topk_regress_bwd")
    return dict(out=out, gcost=gcost, gsamples=gsamples, idx=idx)


def _node(name):
    """The same through regression_topk under autograd; idx is what the node saved."""
    from dkt_stereo_amd.topk import regression_topk
    cost, samples, gout = _operands(name)
    leaf = cost.detach().requires_grad_(True)                                   # (a view of the wider buffer for "strided")
    sleaf = None if samples is None else samples.detach().requires_grad_(True)
    out = regression_topk(leaf, sleaf, R.CASES[name]["k"])
    assert out.requires_grad and type(out.grad_fn).__name__ == "_TopkRegressFnBackward"
    saved = [t for t in out.grad_fn.saved_tensors if t is not None and t.dtype == torch.uint8]
    assert len(saved) == 1
    out.backward(gout)
    return dict(out=out.detach(), gcost=leaf.grad, gsamples=None if sleaf is None else sleaf.grad, idx=saved[0])


@pytest.mark.parametrize("name", list(R.CASES))
def test_fixed_cases(name):
    """Forward, gcost and gsamples of every case under the bounds, through the raw entries (into NaN-filled buffers) and
    through the node; the saved planes are the stable sort's; the two routes give the same bits, and so does a second run."""
    ref = R.reference(name)
    truth, bound = ref["truth"], ref["bound"]
    raw, node = _raw(name), _node(name)
    for how, got in (("raw", raw), ("node", node)):
        assert torch.equal(got["idx"].cpu().long(), truth["idx"]), (name, how)
        for key in KEYS:
            if truth[key] is None:
                assert got[key] is None
                continue
            ratio = R.worst(got[key], truth[key], bound[key])
            print("%-8s %-4s %-8s %.4f of the bound" % (name, how, key, ratio))
            assert ratio <= 1.0, (name, how, key, ratio)
    again = _raw(name)
    for key in KEYS:
        if raw[key] is not None:
            assert R.same(raw[key], node[key]) and R.same(raw[key], again[key]), (name, key)
    assert torch.equal(raw["idx"], again["idx"])


@pytest.mark.parametrize("name", ["k2", "samples", "k8", "strided", "nan"])
def test_no_grad_forward_is_the_nodes_forward(name):
    """Without grad: the plain launch, no index buffer, the same bits; a (B, D, h, w) cost in fp16 is cast."""
    from dkt_stereo_amd import _ffi
    from dkt_stereo_amd.topk import regression_topk
    cost, samples, _ = _operands(name)
    k = R.CASES[name]["k"]
    with _ffi.launch_log() as names:
        plain = regression_topk(cost, samples, k)
        with torch.no_grad():
            quiet = regression_topk(cost.detach().requires_grad_(True), samples, k)
    assert names == ["dkt_topk_regress_fwd"] * 2
    assert plain.grad_fn is None and quiet.grad_fn is None and plain.shape == (cost.shape[0], 1) + tuple(cost.shape[2:])
    node = _node(name)["out"]
    assert R.same(plain, node) and R.same(quiet, node)
    half = regression_topk(cost.half(), None, k)
    assert half.dtype == torch.float32


def test_only_the_nan_pixel_is_nan():
    b, _, y, x = R.NAN_AT
    for got in (_raw("nan"), _node("nan")):
        nan = torch.isnan(got["out"])
        assert bool(nan[b, 0, y, x]) and int(nan.sum()) == 1
        gnan = torch.isnan(got["gcost"])
        assert int(gnan.sum()) == R.CASES["nan"]["k"] and int(gnan[b, :, y, x].sum()) == R.CASES["nan"]["k"]


def test_gradient_to_the_samples_alone():
    """cost detached: the node still runs, dkt_topk_regress_bwd is asked for gsamples only."""
    from dkt_stereo_amd.topk import regression_topk
    ref = R.reference("samples")
    cost, samples, gout = _operands("samples")
    sleaf = samples.detach().requires_grad_(True)
    out = regression_topk(cost, sleaf, 2)
    out.backward(gout)
    assert R.same(sleaf.grad, _raw("samples")["gsamples"])
    assert R.worst(sleaf.grad, ref["truth"]["gsamples"], ref["bound"]["gsamples"]) <= 1.0


def test_exceptions():
    from dkt_stereo_amd import _ffi
    from dkt_stereo_amd.topk import regression_topk
    cost = torch.zeros(1, 4, 2, 3, device=DEV)
    for k in (0, 5, -2):
        with pytest.raises(_ffi.DktError):
            regression_topk(cost, None, k)
    with pytest.raises(_ffi.DktError):
        regression_topk(torch.zeros(1, 16, 2, 3, device=DEV), None, 9)
    with pytest.raises(_ffi.DktError):
        regression_topk(torch.zeros(1, 257, 1, 1, device=DEV), None, 2)
    with pytest.raises(_ffi.DktError):
        regression_topk(cost.cpu(), None, 2)
    with pytest.raises(_ffi.DktError):
        regression_topk(cost, torch.zeros(1, 4, 2, 3), 2)
    with pytest.raises(ValueError):
        regression_topk(cost, torch.zeros(1, 4, 2, 4, device=DEV), 2)
    with pytest.raises(ValueError):
        regression_topk(cost[0], None, 2)


def test_a_forward_under_autograd_keeps_less_than_half_a_cost():
    """At (1, 48, 32, 64), k = 2: the node keeps the map and two bytes per pixel beside the cost it was given; the torch chain
    keeps more than two costs (so the first assertion cannot pass vacuously)."""
    from dkt_stereo_amd.topk import regression_topk
    cost = G(R.reference("mem")["cost"])
    size = cost.numel() * 4

    def grown(fn):
        leaf = cost.clone().requires_grad_(True)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        out = fn(leaf)
        torch.cuda.synchronize()
        assert out.requires_grad
        return torch.cuda.memory_allocated() - base

    node = grown(lambda c: regression_topk(c, None, 2))
    chain = grown(lambda c: R.torch_chain_graph(c, R.arange_samples(c.detach()), 2))
    print("allocated after the forward: node %.3f, torch chain %.3f costs" % (node / size, chain / size))
    assert node < 0.5 * size
    assert chain > 2.0 * size


def _head(training, dtype):
    """(outputs, gcost, glogits) of the reference's lines on the CPU in `dtype` for the head case."""
    cost, logits, gouts = _head_inputs()
    c = torch.from_numpy(cost).to(dtype).requires_grad_(True)
    lg = torch.from_numpy(logits).to(dtype).requires_grad_(True)
    outs = R.head_chain(c, lg, 2, training)
    outs = outs if training else [outs]
    gs = gouts if training else gouts[1:]
    gc, gl = torch.autograd.grad(outs, (c, lg), [torch.from_numpy(g).to(dtype) for g in gs])
    return [o.detach() for o in outs], gc, gl


def _head_inputs():
    B, D, h, w = 2, 48, 5, 19
    cost = _synth.normal((B, D, h, w), 521, "cost", scale=3.0)
    logits = _synth.normal((B, 9, 4 * h, 4 * w), 521, "logits", scale=2.0)
    gouts = [_synth.normal((B, 1, h, w), 521, "g0"), _synth.normal((B, 1, 4 * h, 4 * w), 521, "g1")]
    return cost, logits, gouts


@pytest.mark.parametrize("training", [False, True])
def test_cgi_disparity_head(training):
    """cgi_disparity_head against CGI_Stereo.py:253-268 restated in float64, both modes, with the gradients to cost and to the
    spx logits: err <= 8 max(|fp32 CPU chain - truth|, floor).  The floors are the first-order bounds of the stage that
    produces each result, from the truth's magnitudes: the regression's for -4 pred and for gcost (with |g| the true gradient
    that reaches pred), _context_upsample_ref's for the up-sampled map and for glogits; what one stage hands to the next is met
    by the yardstick, which runs the same stages in fp32."""
    from dkt_stereo_amd import _ffi
    from dkt_stereo_amd.topk import cgi_disparity_head
    cost, logits, gouts = _head_inputs()
    t_outs, t_gc, t_gl = _head(training, torch.float64)
    y_outs, y_gc, y_gl = _head(training, torch.float32)
    # the floors
    tc, tl = torch.from_numpy(cost), torch.from_numpy(logits)
    pred = R.closed_form(tc, None, torch.zeros(2, 1, 5, 19), 2)["out"]
    pl = pred.clone().requires_grad_(True)                                      # the true gradient that reaches pred
    up = -4.0 * CU.sequence(pl, torch.softmax(tl.double(), 1)).unsqueeze(1)
    gp = torch.autograd.grad(up, pl, torch.from_numpy(gouts[1]).double())[0]
    if training:
        gp = gp - 4.0 * torch.from_numpy(gouts[0]).double()
    node_bound = R.bounds(tc, None, gp.float(), 2)
    mags = CU.magnitudes(pred.float(), tl, torch.from_numpy(gouts[1][:, 0]), True)
    cs = CU.constants(mags, True)
    floor_up = (cs["out"] * CU.U * mags["out"]).unsqueeze(1)
    floor_gl = cs["gnine"] * CU.U * mags["gnine"]
    floors = ([4.0 * node_bound["out"] / 2.0] if training else []) + [floor_up]

    leaf = G(cost)[:, None].requires_grad_(True)                                # (B, 1, D, h, w), as the hourglass returns it
    lleaf = G(logits).requires_grad_(True)
    with _ffi.launch_log() as names:
        outs = cgi_disparity_head(leaf, lleaf, 2, training)
    assert names == ["dkt_topk_regress_fwd", "dkt_context_upsample_logits_fwd"]
    outs = outs if training else [outs]
    assert len(outs) == len(t_outs)
    torch.autograd.backward(outs, [G(g) for g in (gouts if training else gouts[1:])])
    got = list(outs) + [leaf.grad[:, 0], lleaf.grad]
    want = list(zip(t_outs + [t_gc, t_gl], y_outs + [y_gc, y_gl], floors + [node_bound["gcost"] / 2.0, floor_gl]))
    for i, (g, (truth, yard, floor)) in enumerate(zip(got, want)):
        assert g.shape == truth.shape, i
        env = R.envelope(yard, truth, floor)
        err = (g.detach().double().cpu() - truth).abs()
        assert bool(torch.isfinite(err).all())
        exact = (env == 0) & (err == 0)
        ratio = float((err / env.clamp(min=1e-300))[~exact].max()) if bool((~exact).any()) else 0.0
        print("head training=%s result %d: %.4f of the envelope" % (training, i, ratio))
        assert ratio <= 1.0, (training, i, ratio)
