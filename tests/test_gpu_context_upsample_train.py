"""IGEV's context up-sampling under autograd (-m gpu): submodule.context_upsample as _ContextUpsampleFn (the weights form:
dkt_context_upsample forward, dkt_context_upsample_bwd) and upsample.context_upsample_logits (the logits form:
dkt_context_upsample_logits_fwd / _bwd).

Every result against the float64 closed form of _context_upsample_ref.py under its bounds,

    |got - exact| <= 2 c u mag,  u = 2^-24,
    logits form:   c_out = 2 R + 22,  c_glogits = 4 R + 38,  c_gdisp = 2 R_max + 13 + 144
    weights form:  forward the inference kernel's bits, gweights the fp32 product's bits, c_gdisp = 145,

with R the spread of the nine logits of the fine pixel (R_max: the largest among an element's contributors) and mag the
float64 chain on |disp|, |gout| with the true softmax; test_host_context_upsample_ref.py shows that the reference's own
fp32 arithmetic meets the same bounds.  Each case prints the kernels' worst error in units of u * mag (run with -s)."""
import functools

import numpy as np
import pytest
import torch

import _context_upsample_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("out", "gdisp", "gnine")
NODES = {False: "_ContextUpsampleFnBackward", True: "_ContextUpsampleLogitsFnBackward"}
ALL = {**R.CASES, **R.WIDE_CASES}


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _ref(name, logits):
    """numpy inputs, closed form, magnitudes and constants of one case and form, computed once and shared."""
    disp, lg, gout = R.inputs(ALL[name])
    nine = lg if logits else R.weights_of(lg)
    t = tuple(torch.from_numpy(x) for x in (disp, nine, gout))
    mags = R.magnitudes(*t, logits)
    return (disp, nine, gout), dict(zip(KEYS, R.closed_form(*t, logits))), mags, R.constants(mags, logits)


def _inference(disp, weights):
    from dkt_stereo_amd.submodule import context_upsample
    with torch.no_grad():
        return context_upsample(disp.detach(), weights.detach())


def _upstream(g, how):
    """The upstream gradient contiguous, as a batch-strided view of a wider buffer, or W-major storage."""
    if how == "slice":
        buf = torch.full((g.shape[0], 3) + tuple(g.shape[1:]), 9.0, device=g.device)
        buf[:, 1] = g
        return buf[:, 1]
    if how == "transposed":
        return g.transpose(1, 2).contiguous().transpose(1, 2)
    return g


def _run(arrays, logits, need="both", up="contiguous"):
    """(out, gdisp or None, gnine or None) through the node."""
    from dkt_stereo_amd.submodule import context_upsample
    from dkt_stereo_amd.upsample import context_upsample_logits
    disp, nine, gout = arrays
    a = G(disp).requires_grad_(need in ("both", "disp"))
    b = G(nine).requires_grad_(need in ("both", "nine"))
    out = context_upsample_logits(a, b, R.SCALE) if logits else context_upsample(a, b)
    assert out.requires_grad and type(out.grad_fn).__name__ == NODES[logits]
    out.backward(_upstream(G(gout), up))
    return out.detach(), a.grad, b.grad


def _check(name, logits, need="both", up="contiguous"):
    arrays, exact, mags, c = _ref(name, logits)
    got = dict(zip(KEYS, _run(arrays, logits, need, up)))
    assert (got["gdisp"] is None) == (need == "nine") and (got["gnine"] is None) == (need == "disp"), name
    line = []
    for what in KEYS:
        if got[what] is None or c[what] is None:
            continue
        assert got[what].shape == exact[what].shape
        in_u, of_bound = R.worst(got[what], exact[what], mags[what], c[what])
        line.append("%s %.2f u*mag (%.3f of the bound)" % (what, in_u, of_bound))
        assert of_bound <= 1.0, (name, what, in_u, of_bound)
    if not logits:
        assert torch.equal(got["out"], _inference(G(arrays[0]), G(arrays[1]))), name      # forward: the same bits
        if got["gnine"] is not None:
            assert R.same(got["gnine"], R.fp32_product(arrays[0], arrays[2])), name       # one rounding: the same bits
    print("%-9s %-7s " % (name, "logits" if logits else "weights") + ", ".join(line))
    return tuple(got[k] for k in KEYS)


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("name", list(R.CASES))
def test_fixed_cases(name, logits):
    """Both forms on every fixed case: all three results under their bounds (bit for bit where the arithmetic is one
    rounding), a second run bit-identical."""
    first = _check(name, logits)
    again = _run(_ref(name, logits)[0], logits)
    assert all(R.same(x, y) for x, y in zip(first, again)), name


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("name", list(R.WIDE_CASES))
def test_wide_logits_repeat_bit_for_bit(name, logits):
    """Logit spreads at which softmax terms become denormal or 0: finite, and the same bits from run to run."""
    arrays = _ref(name, logits)[0]
    first = _run(arrays, logits)
    assert all(bool(torch.isfinite(t).all()) for t in first)
    assert all(R.same(x, y) for x, y in zip(first, _run(arrays, logits)))


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("need", ["disp", "nine"])
@pytest.mark.parametrize("name", ["small", "tiles"])
def test_needs_input_grad_subsets(name, need, logits):
    """One gradient alone is bit-identical to the same gradient computed beside the other; the other is None."""
    _, gdisp, gnine = _check(name, logits, need=need)
    _, bdisp, bnine = _run(_ref(name, logits)[0], logits)
    assert R.same(gdisp, bdisp) if need == "disp" else R.same(gnine, bnine)


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("up", ["slice", "transposed"])
@pytest.mark.parametrize("name", ["h1", "tiles"])
def test_non_contiguous_upstream(name, up, logits):
    """A batch-strided view of a wider buffer and a W-major upstream gradient give the contiguous result."""
    got = _check(name, logits, up=up)
    assert all(R.same(x, y) for x, y in zip(got, _run(_ref(name, logits)[0], logits)))


def test_batch_strided_upstream_is_read_in_place():
    """The (B, 4h, 4w) gradient as the kernels take it: a batch-strided view goes as it is, other layouts are copied."""
    from dkt_stereo_amd.upsample import _batch_strided
    buf = torch.zeros((2, 3, 8, 16), device=DEV)
    g, bs = _batch_strided(buf[:, 1].unsqueeze(1))
    assert g.data_ptr() == buf[:, 1].data_ptr() and bs == 3 * 8 * 16
    g, bs = _batch_strided(buf[:, 1, :, 4:12].unsqueeze(1))
    assert g.is_contiguous() and bs == 8 * 8


def test_context_upsample_takes_gradients_and_keeps_the_inference_path():
    """context_upsample(disp.requires_grad_(), w) is differentiable (it used to raise DktError); without a gradient, and
    under torch.no_grad(), it is the plain kernel call with the same bits; fp16 inputs get fp16 gradients."""
    disp, lg, gout = R.inputs(R.CASES["small"])
    w = R.weights_of(lg)
    a, b = G(disp).requires_grad_(True), G(w)
    from dkt_stereo_amd.submodule import context_upsample
    out = context_upsample(a, b)
    assert out.requires_grad and type(out.grad_fn).__name__ == NODES[False]
    plain = context_upsample(G(disp), G(w))
    assert plain.grad_fn is None and not plain.requires_grad and torch.equal(out.detach(), plain)
    with torch.no_grad():
        quiet = context_upsample(a, b)
    assert quiet.grad_fn is None and torch.equal(quiet, plain)
    (ga,) = torch.autograd.grad(out, [a], G(gout))
    assert ga.shape == a.shape and bool(torch.isfinite(ga).all())
    ah, bh = G(disp).half().requires_grad_(True), G(w).half().requires_grad_(True)
    oh = context_upsample(ah, bh)
    assert oh.dtype == torch.float32
    oh.backward(G(gout))
    assert ah.grad.dtype == torch.float16 and bh.grad.dtype == torch.float16


def test_scale_must_be_a_power_of_two():
    from dkt_stereo_amd import _ffi
    from dkt_stereo_amd.upsample import context_upsample_logits
    disp, lg, _ = R.inputs(R.CASES["small"])
    for bad in (3.0, 0.0, -4.0):
        with pytest.raises(_ffi.DktError):
            context_upsample_logits(G(disp).requires_grad_(True), G(lg), bad)
    context_upsample_logits(G(disp), G(lg), 0.5)


@pytest.mark.parametrize("name", ["h1", "tiles", "sigma32"])
def test_logits_form_is_the_convex_form_at_f4(name):
    """context_upsample_logits(disp, logits, 4) is convex_upsample(disp, mask, 4, 1) on the planes re-laid-out as
    mask[b, (k*4 + i)*4 + j, y, x] = logits[b, k, 4y + i, 4x + j]: the nine-tap core of ups9.h runs the same operation
    sequence per element in both (softmax, fl(4 nb), sum_k fl(p_k v_k) from 0 in ascending k; a_k, s, fl(p_k fl(a_k - s));
    C in ascending j, then i; the gather in ascending k, times the factor), so out, the coarse gradient and the nine-plane
    gradient are equal, the wide case (the softmax's rare division path) included.  torch.equal, not R.same: the convex
    kernel adds +0 where the logits kernel does not (its masked second channel, its accumulators starting at 0), which
    can change the sign of a zero and nothing else."""
    from dkt_stereo_amd.upsample import context_upsample_logits, convex_upsample
    disp, logits, gout = (G(x) for x in _ref(name, True)[0])
    B, _, h, w = disp.shape
    mask = logits.view(B, 9, h, 4, w, 4).permute(0, 1, 3, 5, 2, 4).reshape(B, 144, h, w)
    a, b = disp.clone().requires_grad_(True), mask.clone().requires_grad_(True)
    cv = convex_upsample(a, b, 4, 1)
    cv.backward(gout[:, None])
    c, d = disp.clone().requires_grad_(True), logits.clone().requires_grad_(True)
    lg = context_upsample_logits(c, d, 4.0)
    lg.backward(gout)
    assert torch.equal(cv.detach()[:, 0], lg.detach()), name
    assert torch.equal(a.grad, c.grad), name
    assert torch.equal(b.grad.view(B, 9, 4, 4, h, w).permute(0, 1, 4, 2, 5, 3).reshape(B, 9, 4 * h, 4 * w), d.grad), name


def test_logits_form_is_the_weights_form_behind_a_softmax():
    """context_upsample_logits(disp, logits, 4) and context_upsample(4 disp, softmax(logits)) on the device differ by the
    softmax's roundings only: both meet the out bound."""
    from dkt_stereo_amd.submodule import context_upsample
    from dkt_stereo_amd.upsample import context_upsample_logits
    arrays, exact, mags, c = _ref("tiles", True)
    with torch.no_grad():
        one = context_upsample_logits(G(arrays[0]), G(arrays[1]), R.SCALE)
        two = context_upsample(G(arrays[0]) * R.SCALE, torch.softmax(G(arrays[1]), 1))
    for got in (one, two):
        assert R.worst(got, exact["out"], mags["out"], c["out"])[1] <= 1.0
