"""The conv backward kernels where their work plans walk and halve (-m gpu): dkt_conv2d_wgrad, dkt_conv2d_wgrad_s2, their
finishing kernel and dkt_conv_grad_prepass on PLAN_CASES / PREPASS_PLAN_CASES of the three reference modules -- launches
with more items than blocks, slices of 2048 and 1024 pixels, a finish that strides, planes of several segments -- and on the
seeded small shapes of _conv_wgrad_ref.drawn_cases, against the fp64 truth under the bounds the fixed cases use (A_BOUND and
bound (b) for gw, GX_BOUND for gx) and, for the bias gradient, against a bit-exact restatement of its summation order.
test_host_conv_grad_plans.py proves on the CPU that the cases are in the regimes they are named after, that the references
meet the bounds on every one of them and that a lost tile, slice or late item misses them.

Every case prints its figures (run with -s)."""
import functools

import pytest
import torch
import torch.nn as nn

import _conv_grad_ref as R
import _conv_s2_ref as S
import _conv_wgrad_ref as WR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
#: upstream magnitudes 2^m
MS = [0, -20]
PLAN = [(1, c) for c in WR.PLAN_CASES] + [(2, c) for c in S.PLAN_CASES]
WALKED = [(1, c) for c in WR.WALKED] + [(2, c) for c in S.WALKED]
MIXED = [(1, WR.MIXED), (2, S.MIXED)]
#: one walked case per stride for the node: T = 512, 130 -> 70 channels, odd sizes
NODE_CASES = [(1, WR.PLAN_CASES[3]), (2, S.PLAN_CASES[3])]
DRAWN = [(s, c) for s in (1, 2) for c in WR.drawn_cases(s)]
_id = lambda v: "s%d-%s" % (v[0], "x".join(str(n) for n in v[1]))


def _regime(stride, case):
    return WR.regime_of(case) if stride == 1 else S.regime_of(case)


def _walks(stride, case):
    """The launch has more items than blocks on THIS device: otherwise the case does not test what it is there for."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    items = _regime(stride, case)["items"]
    assert items > cus, "%s: %d items on %d CUs, no block takes a second item" % (case, items, cus)


def _gp(stride, case):
    """g' at unit magnitude: the upstream gradient behind the case's random mask."""
    _, _, _, gy, y = WR.drawn_inputs(case, stride)
    return R.mask(gy, y)


@functools.lru_cache(maxsize=None)
def _truth(stride, case):
    """(fp64 gw, bound (b), fp64 gx at stride 2 for the drawn cases) at unit magnitude, computed once: a power-of-two multiple
    of g' gives that multiple of all three exactly.  Only weight-sized results are kept."""
    B, H, W, k, cin, cout = case
    x, w = WR.drawn_inputs(case, stride)[:2]
    gp = _gp(stride, case)
    if stride == 1:
        return WR.truth(x, gp, k), WR.b_bound(x, gp, k), None
    gx = S.truth_gx(gp, w, (H, W)) if (stride, case) in DRAWN else None
    return S.truth_gw(x, gp, k), S.b_bound(x, gp, k), gx


def _held(got, exact, bound, what):
    ea = WR.a_error(got.cpu(), exact)
    ok, rb = WR.b_ratio(got.cpu(), exact, bound)
    print("%s: (a) %.2e  (b) |d|/bound %.2e" % (what, ea, rb))
    assert ea <= WR.A_BOUND, (what, ea)
    assert ok, (what, rb)


def _wgrad(stride, case, gp, layout):
    """The entry on g' in `layout` (x in the same layout), with the device scale pair of the pre-pass."""
    from dkt_stereo_amd import conv
    g = R.laid_out(gp, layout, DEV)
    x = R.laid_out(WR.drawn_inputs(case, stride)[0], layout, DEV)
    g2, _, scale = conv.conv_grad_prepass(g, None, want_bias=False)
    assert g2.data_ptr() == g.data_ptr()
    assert torch.equal(scale.cpu(), R.scale_pair(float(gp.abs().max())))
    return conv.conv2d_wgrad(x, g, scale, case[3], stride=stride)


def _entries_against_truth(stride, case):
    exact, bound, _ = _truth(stride, case)
    gp = _gp(stride, case)
    for m in MS:
        s = 2.0 ** m
        got = {}
        for layout in WR.LAYOUTS:
            got[layout] = _wgrad(stride, case, gp * s, layout)
            _held(got[layout], exact * s, bound * s, "s%d %s %s m=%d" % (stride, case, layout, m))
        # the order of every sum is a function of the shape alone: the 16-byte and the 4-byte path give the same bits
        assert torch.equal(got["strided"], got["misaligned"])


# -------------------------------------------------------------------------------------------------------- the walk check
@pytest.mark.parametrize("sc", WALKED, ids=_id)
def test_walked_cases_walk_on_this_device(sc):
    _walks(*sc)


# ------------------------------------------------------------------------------------------------------------ the entries
@pytest.mark.parametrize("sc", PLAN, ids=_id)
def test_entries_against_truth(sc):
    stride, case = sc
    if sc in WALKED:
        _walks(stride, case)
    _entries_against_truth(stride, case)


@pytest.mark.parametrize("sc", MIXED, ids=_id)
def test_runs_repeat_and_scale_bit_for_bit(sc):
    """Three runs give the same bits; g' * 2^-20 gives 2^-20 times the unit result exactly."""
    stride, case = sc
    _walks(stride, case)
    gp = _gp(stride, case)
    gw0 = _wgrad(stride, case, gp, "strided")
    for _ in range(2):
        assert torch.equal(_wgrad(stride, case, gp, "strided"), gw0)
    assert torch.equal(_wgrad(stride, case, gp * 2.0 ** -20, "strided"), gw0 * 2.0 ** -20)


# --------------------------------------------------------------------------------------------------------------- the node
@pytest.mark.parametrize("sc", NODE_CASES, ids=_id)
def test_node_with_relu_on_a_walked_case(sc):
    """conv2d_autograd with ReLU: the pre-pass (mask, bias gradient, scale pair) and the weight gradient compose on a walked
    plan; the input gradient -- the device-scaled convolution at stride 1, dkt_conv2d_dgrad_s2 at stride 2 -- gets a large
    case.  gb is the restated summation order bit for bit."""
    from dkt_stereo_amd import conv
    stride, case = sc
    _walks(stride, case)
    B, H, W, k, cin, cout = case
    x, w, b, gy, _ = WR.drawn_inputs(case, stride)
    lay = nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2)
    with torch.no_grad():
        lay.weight.copy_(w)
        lay.bias.copy_(b)
    lay = lay.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    y = conv.conv2d_autograd(xd, lay, relu=True)
    assert type(y.grad_fn).__name__ == "_Conv2dGradFnBackward"
    gx, gw, gb = torch.autograd.grad(y, [xd, lay.weight, lay.bias], grad_outputs=gy.to(DEV))
    gp = R.mask(gy, y.detach().cpu())
    if stride == 1:
        want_gx, want_gw, bound = R.truth(gy, y.detach().cpu(), w)[2], WR.truth(x, gp, k), WR.b_bound(x, gp, k)
    else:
        want_gx, want_gw, bound = S.truth_gx(gp, w, (H, W)), S.truth_gw(x, gp, k), S.b_bound(x, gp, k)
    _held(gw, want_gw, bound, "node s%d %s gw" % (stride, case))
    e_gx = R.gx_error(gx.cpu(), want_gx)
    print("node s%d %s: gx %.2e" % (stride, case, e_gx))
    assert e_gx <= R.GX_BOUND
    assert torch.equal(gb.cpu(), R.emulate_gb(gp))


# ----------------------------------------------------------------------------------------------------------- the pre-pass
def _prepass(gy, y, layout):
    from dkt_stereo_amd import conv
    g = R.laid_out(gy, layout, DEV)
    yd = None if y is None else R.laid_out(y, layout, DEV)
    gm, gb, scale = conv.conv_grad_prepass(g, yd, want_bias=True)
    if y is None:
        assert gm.data_ptr() == g.data_ptr()
    return gm.cpu(), gb.cpu(), scale.cpu()


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", R.PREPASS_PLAN_CASES, ids=R.PREPASS_PLAN_IDS)
def test_prepass_is_the_restated_order_bit_for_bit(case, relu):
    """g' and the scale pair equal the truth; gb equals emulate_gb -- the order the kernel's header states -- bit for bit, on
    the 16-byte and on the 4-byte path, at 2^0 and 2^-20."""
    gy0, y = R.prepass_inputs(case)
    y = y if relu else None
    for m in MS:
        gy = gy0 * 2.0 ** m
        gp = R.mask(gy, y)
        want = R.emulate_gb(gp)
        d = (want.double() - gp.double().sum(dim=(0, 2, 3))).abs()
        assert bool((d <= R.gb_bound(gp)).all())
        for layout in R.LAYOUTS:
            gm, gb, scale = _prepass(gy, y, layout)
            assert torch.equal(gm, gp), (case, layout, m)
            assert torch.equal(scale, R.scale_pair(float(gp.abs().max()))), (case, layout, m)
            same = torch.equal(gb, want)
            print("prepass %s relu=%d %s m=%d: gb is the restated order: %s (max |d| %.2e)"
                  % (case, relu, layout, m, same, float((gb - want).abs().max())))
            assert same, (case, relu, layout, m)


def _plants():
    """(name, case, (b, c, e)): where the one largest |g'| is put."""
    c0, c1 = R.PREPASS_PLAN_CASES[0], R.PREPASS_PLAN_CASES[1]
    out = []
    for case in (c0, c1):                                   # the 16-byte and the 4-byte path
        B, C, H, W = case
        out.append(("the last element of the last partial segment", case, (B - 1, 3, H * W - 1)))
    B, C, H, W = c1
    out.append(("an item past the launch's 2048 blocks", c1, (B - 1, C - 1, R.PRE_SEG + 1)))
    out.append(("a channel of the finish's third round", c0, (0, c0[1] - 1, 5)))
    return out


@pytest.mark.parametrize("plant", _plants(), ids=lambda p: p[0].replace(" ", "_") + "-" + "x".join(str(v) for v in p[1]))
def test_scale_pair_follows_a_planted_maximum(plant):
    name, case, (b, c, e) = plant
    B, C, H, W = case
    reg = R.prepass_regime(case)
    if name.startswith("the last"):
        assert reg["nseg"] >= 2 and reg["last"] < 1024 and e == H * W - 1
    elif name.startswith("an item"):
        assert R.item_of(case, b, c, e) >= R.PRE_BLOCKS and c < 2 * R.PRE_THREADS
    else:
        assert c >= 2 * R.PRE_THREADS
    gy0, y0 = R.prepass_inputs(case)
    base = R.scale_pair(float(gy0.abs().max()))
    gy, y = gy0.clone(), y0.clone()
    gy.view(B, C, -1)[b, c, e] = -37.5                      # the draws stay below 8: three binades up
    y.view(B, C, -1)[b, c, e] = 1.0                         # not masked away
    want = R.scale_pair(37.5)
    assert not torch.equal(want, base)
    for yy in (None, y):
        gp = R.mask(gy, yy)
        for layout in R.LAYOUTS:
            gm, gb, scale = _prepass(gy, yy, layout)
            assert torch.equal(scale, want), (name, layout, scale.tolist())
            assert torch.equal(gm, gp) and torch.equal(gb, R.emulate_gb(gp))
    # masked away, the pair falls back
    y.view(B, C, -1)[b, c, e] = -1.0
    _, _, scale = _prepass(gy, y, "strided")
    assert torch.equal(scale, R.scale_pair(float(R.mask(gy, y).abs().max())))


# ------------------------------------------------------------------------------------------------------- the drawn shapes
@pytest.mark.parametrize("sc", DRAWN, ids=_id)
def test_drawn_shapes_against_truth(sc):
    from dkt_stereo_amd import conv
    stride, case = sc
    _entries_against_truth(stride, case)
    if stride == 1:
        return
    B, H, W, k, cin, cout = case
    w = WR.drawn_inputs(case, 2)[1]
    lay = nn.Conv2d(cin, cout, k, stride=2, padding=k // 2)
    with torch.no_grad():
        lay.weight.copy_(w)
    lay = lay.to(DEV)
    shim = conv._grad_layer(lay)
    gp, want = _gp(2, case), _truth(2, case)[2]
    for m in MS:
        s = 2.0 ** m
        got = {}
        for layout in S.LAYOUTS:
            g = R.laid_out(gp * s, layout, DEV)
            _, _, scale = conv.conv_grad_prepass(g, None, want_bias=False)
            got[layout] = conv.conv2d_dgrad_s2(g, shim, scale, (H, W), shim.pack_scale)
            e = S.gx_error(got[layout].cpu(), want * s)
            print("s2 %s %s m=%d: gx %.2e" % (case, layout, m, e))
            assert e <= S.GX_BOUND, (case, layout, m, e)
        assert torch.equal(got["strided"], got["misaligned"])
