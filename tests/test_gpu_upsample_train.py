"""The convex up-sampling autograd node (-m gpu): dkt_convex_upsample_fwd / _bwd behind upsample.convex_upsample and
RAFTStereo.upsample_flow(..., channels=).

Forward: bit-identical to the inference kernel's leading channels.  Backward: against the float64 gradient of the
reference's expression sequence under the bound derived in _upsample_ref.py,

    |got - exact| <= 2 c u mag,  u = 2^-24,
    c_gmask = 4 R + Dout + 37,  c_gflow = 2 R_max + 13 + 9 f^2,

with R the spread of the nine logits of the fine pixel (R_max: the largest among an element's contributors) and mag the
float64 chain on |flow|, |gout| with the true softmax; test_host_upsample_ref.py shows that the reference's own fp32
arithmetic meets the same bound.  Each case prints the kernel's worst error in units of u * mag (run with -s)."""
import ctypes

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, example, given, settings
from hypothesis import strategies as st

import _synth
import _upsample_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SET = dict(deadline=None, max_examples=60, suppress_health_check=list(HealthCheck), derandomize=True)
NODE = "_ConvexUpsampleFnBackward"


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _inference(flow, mask, f):
    """The no-grad kernel (dkt_convex_upsample) on the same tensors, every channel."""
    from dkt_stereo_amd import _ffi
    N, D, H, W = flow.shape
    out = torch.empty((N, D, f * H, f * W), device=flow.device)
    _ffi.check(_ffi.lib().dkt_convex_upsample(flow.data_ptr(), mask.data_ptr(), out.data_ptr(), N, D, H, W, f,
                                              _ffi.device_of(flow), _ffi.stream_of(flow)), "dkt_convex_upsample")
    return out


def _upstream(g, how):
    """The upstream gradient contiguous, as a channel slice of a wider buffer (batch-strided), or W-major storage."""
    if how == "slice":
        buf = torch.full((g.shape[0], g.shape[1] + 3) + tuple(g.shape[2:]), 9.0, device=g.device)
        buf[:, 2:2 + g.shape[1]] = g
        return buf[:, 2:2 + g.shape[1]]
    if how == "transposed":
        return g.transpose(2, 3).contiguous().transpose(2, 3)
    return g


def _run(flow, mask, gout, f, Dout, need="both", up="contiguous"):
    """(out, gflow or None, gmask or None) through the node."""
    from dkt_stereo_amd.upsample import convex_upsample
    a = G(flow).requires_grad_(need in ("both", "flow"))
    b = G(mask).requires_grad_(need in ("both", "mask"))
    out = convex_upsample(a, b, f, Dout)
    assert type(out.grad_fn).__name__ == NODE
    out.backward(_upstream(G(gout), up))
    return out.detach(), a.grad, b.grad


def _check(name, flow, mask, gout, f, Dout, need="both", up="contiguous"):
    out, gflow, gmask = _run(flow, mask, gout, f, Dout, need, up)
    assert torch.equal(out, _inference(G(flow), G(mask), f)[:, :Dout]), name                 # forward: the same bits
    tf, tm, tg = (torch.from_numpy(x) for x in (flow, mask, gout))
    _, eflow, emask = R.closed_form(tf, tm, tg, f, Dout)
    mags = R.magnitudes(tf, tm, tg, f, Dout)
    c = R.constants(mags, f, Dout)
    line = []
    assert (gflow is None) == (need == "mask") and (gmask is None) == (need == "flow"), name
    for what, got, exact in (("gflow", gflow, eflow), ("gmask", gmask, emask)):
        if got is None:
            continue
        in_u, of_bound = R.worst(got, exact, mags[what], c[what])
        line.append("%s %.2f u*mag (%.3f of the bound)" % (what, in_u, of_bound))
        assert of_bound <= 1.0, (name, what, in_u, of_bound)
    if gflow is not None:
        assert bool((gflow[:, Dout:] == 0).all()), name
    print("%-9s largest R %.1f: " % (name, float(mags["R_mask"].max())) + ", ".join(line))
    return out, gflow, gmask


@pytest.mark.parametrize("name", list(R.CASES))
def test_fixed_cases(name):
    """Items 1-3 on every fixed case: forward bits, both gradients under the bound, a second run bit-identical."""
    flow, mask, gout, f, Dout = R.inputs(R.CASES[name])
    first = _check(name, flow, mask, gout, f, Dout)
    again = _run(flow, mask, gout, f, Dout)
    assert all(R.same(x, y) for x, y in zip(first, again)), name


@pytest.mark.parametrize("name", list(R.WIDE_CASES))
def test_wide_logits_keep_the_forward_bits(name):
    """Logit spreads at which softmax terms fall below 2^-100, become denormal or 0: the forward is still the inference
    kernel's bit for bit (its divisions take their rare path here), the backward is finite and repeats bit for bit."""
    flow, mask, gout, f, Dout = R.inputs(R.WIDE_CASES[name])
    spread = float(R.magnitudes(*(torch.from_numpy(x) for x in (flow, mask, gout)), f, Dout)["R_mask"].max())
    assert spread > 104.0, spread
    first = _run(flow, mask, gout, f, Dout)
    assert torch.equal(first[0], _inference(G(flow), G(mask), f)[:, :Dout])
    assert all(bool(torch.isfinite(t).all()) for t in first)
    assert all(R.same(x, y) for x, y in zip(first, _run(flow, mask, gout, f, Dout)))


@pytest.mark.parametrize("name", ["f4", "dout3of4", "tiles"])
@pytest.mark.parametrize("need", ["flow", "mask"])
def test_needs_input_grad_subsets(name, need):
    """One gradient alone is bit-identical to the same gradient computed beside the other."""
    flow, mask, gout, f, Dout = R.inputs(R.CASES[name])
    _, gflow, gmask = _check(name, flow, mask, gout, f, Dout, need=need)
    _, bflow, bmask = _run(flow, mask, gout, f, Dout)
    if need == "flow":
        assert R.same(gflow, bflow)
    else:
        assert R.same(gmask, bmask)


@pytest.mark.parametrize("name", ["f4", "f8", "dout3of4", "w1"])
@pytest.mark.parametrize("up", ["slice", "transposed"])
def test_non_contiguous_upstream(name, up):
    flow, mask, gout, f, Dout = R.inputs(R.CASES[name])
    got = _check(name, flow, mask, gout, f, Dout, up=up)
    want = _run(flow, mask, gout, f, Dout)
    assert all(R.same(x, y) for x, y in zip(got, want))


def test_batch_strided_upstream_is_read_in_place():
    """A [:, :Dout] slice of a wider contiguous buffer goes to the kernel as it is; layouts the kernel cannot read are
    made contiguous."""
    from dkt_stereo_amd.upsample import _batch_strided
    buf = torch.zeros((2, 5, 8, 16), device=DEV)
    g, bs = _batch_strided(buf[:, 1:3])
    assert g.data_ptr() == buf[:, 1:3].data_ptr() and bs == 5 * 8 * 16
    g, bs = _batch_strided(buf)
    assert g.data_ptr() == buf.data_ptr() and bs == 5 * 8 * 16
    g, bs = _batch_strided(buf[:, :, :, 1:9])
    assert g.is_contiguous() and bs == 5 * 8 * 8


@settings(**SET)
@given(N=st.integers(1, 3), D=st.integers(1, 4), dcut=st.integers(0, 3), H=st.integers(1, 12), W=st.integers(1, 80),
       nd=st.integers(0, 3), sigma=st.sampled_from([0.5, 2.0, 8.0]), need=st.sampled_from(["both", "flow", "mask"]),
       up=st.sampled_from(["contiguous", "slice", "transposed"]), seed=st.integers(0, 10 ** 6))
@example(N=2, D=2, dcut=1, H=3, W=65, nd=2, sigma=2.0, need="both", up="slice", seed=1)       # one pixel past a tile
@example(N=1, D=4, dcut=0, H=1, W=1, nd=3, sigma=8.0, need="both", up="contiguous", seed=2)
@example(N=3, D=3, dcut=0, H=2, W=64, nd=0, sigma=0.5, need="flow", up="transposed", seed=3)
def test_random_shapes(N, D, dcut, H, W, nd, sigma, need, up, seed):
    f, Dout = 2 ** nd, max(1, D - dcut)
    c = dict(seed=seed, N=N, D=D, Dout=Dout, H=H, W=W, f=f, sigma=sigma)
    flow, mask, gout, f, Dout = R.inputs(c)
    _check("random", flow, mask, gout, f, Dout, need=need, up=up)


def test_abi_names_and_argument_errors():
    """The two entries are exported and refuse bad arguments before any launch."""
    from dkt_stereo_amd import _ffi
    lib = _ffi.lib()
    assert hasattr(lib, "dkt_convex_upsample_fwd") and hasattr(lib, "dkt_convex_upsample_bwd")
    assert {"dkt_convex_upsample_fwd", "dkt_convex_upsample_bwd"} <= set(_ffi.SIGNATURES)
    null = ctypes.c_void_p(0)
    buf = torch.zeros(4096, device=DEV)
    p = ctypes.c_void_p(buf.data_ptr())
    off = ctypes.c_void_p(buf.data_ptr() + 4)
    fwd, bwd = lib.dkt_convex_upsample_fwd, lib.dkt_convex_upsample_bwd
    assert fwd(null, p, p, 1, 2, 1, 2, 2, 4, -1, null) == -1
    assert fwd(p, null, p, 1, 2, 1, 2, 2, 4, -1, null) == -1
    assert fwd(p, p, null, 1, 2, 1, 2, 2, 4, -1, null) == -1
    assert fwd(p, p, p, 0, 2, 1, 2, 2, 4, -1, null) == -2            # N = 0
    assert fwd(p, p, p, 1, 2, 0, 2, 2, 4, -1, null) == -2            # Dout = 0
    assert fwd(p, p, p, 1, 2, 3, 2, 2, 4, -1, null) == -2            # Dout > D
    assert fwd(p, p, p, 1, 2, 1, 2, 0, 4, -1, null) == -2            # W = 0
    assert fwd(p, p, p, 1, 2, 1, 2, 2, 0, -1, null) == -2            # factor = 0
    assert fwd(p, p, p, 1, 2, 1, 2, 2, 3, -1, null) == -7            # factor not a power of two up to 8
    assert fwd(p, p, off, 1, 2, 1, 2, 2, 4, -1, null) == -6          # rows of 4 floats are stored as 16 bytes
    assert bwd(null, 64, p, p, p, p, p, 1, 2, 1, 2, 2, 4, -1, null) == -1
    assert bwd(p, 64, p, p, null, null, p, 1, 2, 1, 2, 2, 4, -1, null) == -1     # neither gradient wanted
    assert bwd(p, 64, p, p, p, p, null, 1, 2, 1, 2, 2, 4, -1, null) == -1        # gflow needs the workspace
    assert bwd(p, 64, p, p, p, p, p, 1, 2, 3, 2, 2, 4, -1, null) == -2           # Dout > D
    assert bwd(p, 63, p, p, p, p, p, 1, 2, 1, 2, 2, 4, -1, null) == -2           # batch stride shorter than an image
    assert bwd(p, 66, p, p, p, p, p, 1, 2, 1, 2, 2, 4, -1, null) == -6           # batch stride not a multiple of f
    assert bwd(off, 64, p, p, p, p, p, 1, 2, 1, 2, 2, 4, -1, null) == -6
    assert bwd(p, 64, p, p, p, p, p, 1, 2, 1, 2, 2, 5, -1, null) == -7
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0                             # nothing ran


def test_upsample_flow_keyword_and_default():
    """upsample_flow under autograd: every channel through the node by default (the same bits as the inference kernel),
    the leading ones with channels=; without a gradient it is the inference kernel as before."""
    from dkt_stereo_amd.raft_stereo import RAFTStereo, make_args
    model = RAFTStereo(make_args())
    flow, mask, gout, f, _ = R.inputs(R.CASES["f4"])
    a, b = G(flow).requires_grad_(True), G(mask).requires_grad_(True)
    full = model.upsample_flow(a, b)
    one = model.upsample_flow(a, b, channels=1)
    assert type(full.grad_fn).__name__ == NODE and type(one.grad_fn).__name__ == NODE
    want = _inference(G(flow), G(mask), f)
    assert torch.equal(full.detach(), want) and torch.equal(one.detach(), want[:, :1])
    with torch.no_grad():
        plain = model.upsample_flow(a, b)
        assert plain.grad_fn is None and torch.equal(plain, want)
        assert torch.equal(model.upsample_flow(a, b, channels=1), want[:, :1])
    assert torch.equal(model.upsample_flow(G(flow), G(mask)), want)


def test_forward_train_predictions_come_from_the_node():
    """_forward_train at 64 x 128, 3 iterations: plain (N, 1, H, W) predictions whose grad_fn is the node, bit-identical
    to upsample_flow(...)[:, :1] of the same flow and mask through the inference kernel."""
    import _cases
    from dkt_stereo_amd.raft_stereo import RAFTStereo, make_args
    model = RAFTStereo(make_args())
    model.load_state_dict(_synth.torch_state_dict(_synth.shapes_of(model), _cases.E2E_WEIGHT_SEED), strict=True)
    model.to(DEV).eval()
    seen = []
    inner = model.upsample_flow

    def spy(flow, mask, channels=None):
        out = inner(flow, mask, channels=channels)
        seen.append((flow.detach(), mask.detach(), channels, out))
        return out

    model.upsample_flow = spy
    i1, i2 = (G(a) for a in _synth.image_pair(5, 2, 64, 128, 12))
    preds = model(i1, i2, iters=3, test_mode=False)["disp_preds"]
    assert len(preds) == 3 and len(seen) == 3
    for pred, (flow, mask, channels, out) in zip(preds, seen):
        assert pred is out and channels == 1
        assert tuple(pred.shape) == (2, 1, 64, 128) and pred.is_contiguous()
        assert type(pred.grad_fn).__name__ == NODE
        with torch.no_grad():
            assert torch.equal(pred, inner(flow, mask)[:, :1])
    # and the graph behind them reaches the mask head
    w = dict(model.named_parameters())["update_block.mask.2.weight"]
    (g,) = torch.autograd.grad(sum(p.sum() for p in preds), [w])
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0
