"""-m gpu: every route of RAFTStereo.iterate() across configurations against the fp64 restatement of _raft_loop_ref.py.

Per case of _raft_loop_ref.CASES, on one model (built as _encoder_ref.make_raft builds it, images from raft_images):

* the loop alone: model.iterate() on the fp64 encoders' outputs rounded to fp32 against iterate_ref in fp64 on the same
  operands, the up-sampled disparity and the low-resolution flow under  err <= MARGIN * max(yardstick, floor)  (the fp32
  restatement's own error and one fp32 spacing at the largest disparity, both from the CPU), and the route the first call
  of the shape took against the one the table derives from the code;
* the whole test_mode forward against forward_ref in fp64 under that case's own whole-forward yardstick;
* state: the case's pair, a different pair of the same shape, the first pair again through the same model (adopted encoder
  outputs, prebuilt volume, captured units): each within the bound of its own truth, the third result equal to the first
  bit for bit;
* batch: the B = 2 cases against their two items run alone, under the same bound.

The `mixed_precision` cases are held to the same truth under a yardstick of their own, the fp64 restatement with the
operands of every convolution rounded to fp16 (_raft_loop_ref.mixed_truth), with MIXED_MARGIN from their own recorded ratios;
the same weights with the key off are held to the fp32-class bound, and the route (one product per block on the C8S loop,
the `f16` backend elsewhere) is asserted.

Measured on the MI355X, err / max(yardstick, floor), the larger of the two outputs (loop alone / whole forward / state,
second pair / batch against its items):

    default_64x128 1.05/1.10/1.09; default_b2_72x136 1.14/0.93/1.00/0.00; default_40x72 1.00/1.03/1.00;
    default_w16 1.08/1.00/0.73; l2r3 1.06/1.18/1.26; l3r4 1.38/0.98/1.14; l3r2 1.94/1.20/1.18; l1r4 1.00/1.00/1.00;
    ds3_72x136 1.00/1.00/1.20; ds1_36x68 1.02/1.07/1.00; ds3_n2_sf_shared 1.12/1.04/1.02; n1_b2 1.00/1.17/1.15/0.00;
    n2 1.10/1.00/1.03; hd96 1.00/1.09/1.00; hd64_n2 1.00/1.33/1.24; instance 1.00/1.08/0.87; sf_n3 1.00/1.00/0.79;
    pipelined 1.00/1.61/1.00; rotated_128 1.00/1.00/1.09; no_graph 1.12/1.02/1.00; iters2 1.00/1.00/1.00;
    flow_init_default 1.05/1.00/1.16; flow_init_l3r2 1.06/1.00/1.00
    mixed_precision, own yardstick, the largest of loop / forward / second pair: mixed_c8 0.85; mixed_n2 0.85
    IGEV, the largest of disp / mask / net0 / net1 / net2: igev_r3 4.24; igev_l3 3.14; igev_c4 4.61 (net0 each time; the
    disparity itself 1.29 / 0.88 / 0.74)

(Many figures are exactly 1.00: the error of the low-resolution flow is then the rounding of the coordinate x + flow itself,
kept in fp32 with a spacing of 1.9e-6 from x = 16 on, which the restatement and the device round alike.  A batch item run
alone gives the bits it has in the batch.)

MARGIN = 4 (2 x 1.94, rounded up to a power of two), MIXED_MARGIN = 2 (2 x 0.85), IGEV_MARGIN = 16 (2 x 4.61);
FLOOR_ULPS = 1 (derivations: _raft_loop_ref.py).  No case exposed a wrong result.
"""
import copy
import functools

import pytest
import torch

import _raft_loop_ref as LR

pytestmark = pytest.mark.gpu

FP64_CASES = [n for n in LR.NAMES if not LR.is_mixed(n)]
MIXED_CASES = [n for n in LR.NAMES if LR.is_mixed(n)]
BATCH_CASES = [n for n in FP64_CASES if LR.BY_NAME[n][2][0] > 1]


def _dev(t):
    if torch.is_tensor(t):
        return t.cuda()
    return None if t is None else [_dev(u) for u in t]


def _fresh(name, **attrs):
    model = copy.deepcopy(LR.model_of(name)[0]).cuda().eval()
    for k, v in attrs.items():
        setattr(model.args, k, v)
    return model


def _iterate(model, name):
    """model.iterate() on the case's operands; a direct caller repeats the call when the loop asks for it (RAFTStereo.iterate)."""
    from dkt_stereo_amd.raft_stereo import _RetryForward
    ops, iters, fi = _dev(list(LR.operands_of(name))), LR.BY_NAME[name][3], _dev(LR.flow_init_of(name))
    for _ in range(4):
        try:
            with torch.no_grad():
                lo, up = model.iterate(*ops, iters, flow_init=fi)
            return lo.clone(), up.clone()
        except _RetryForward:
            continue
    raise AssertionError("%s: iterate() asked for a fourth repeat" % name)


def _forward(model, name, pair=0, items=None):
    i1, i2 = LR.images_of(name, pair)
    fi = LR.flow_init_of(name)
    if items is not None:
        i1, i2, fi = i1[items], i2[items], None if fi is None else fi[items]
    lo, up = model(i1.cuda(), i2.cuda(), iters=LR.BY_NAME[name][3], flow_init=_dev(fi), test_mode=True)
    return lo.clone(), up.clone()


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's model on the device after the loop alone has run on it, first call of the shape logged:
    dict(model, route, lo, up)."""
    model = _fresh(name)
    with LR.route_log(model) as names:
        lo, up = _iterate(model, name)
    return dict(model=model, route=LR.route_of(names, model), lo=lo, up=up)


@pytest.mark.parametrize("name", FP64_CASES)
def test_loop_alone(name):
    c = _case(name)
    print("ROUTE %-24s %s" % (name, c["route"]))
    ratio = LR.check(name + " loop", c["lo"], c["up"], LR.loop_truth(name))
    print("RATIO %-24s loop %.2f" % (name, ratio))
    assert c["route"] == LR.BY_NAME[name][4], "%s took '%s', the table expects '%s'" % (name, c["route"], LR.BY_NAME[name][4])
    assert float(c["lo"][:, 1:].abs().max()) == 0.0            # the y row of the flow never moves (raft_stereo.py:165)


@pytest.mark.parametrize("name", FP64_CASES)
def test_whole_forward(name):
    model = _case(name)["model"]
    lo, up = _forward(model, name)
    ratio = LR.check(name + " forward", lo, up, LR.forward_truth(name))
    print("RATIO %-24s forward %.2f" % (name, ratio))


@pytest.mark.parametrize("name", FP64_CASES)
def test_state_second_pair_then_first_again(name):
    model = _case(name)["model"]
    first = _forward(model, name)
    second = _forward(model, name, 1)
    third = _forward(model, name)
    LR.check(name + " first", *first, LR.forward_truth(name))
    ratio = LR.check(name + " second pair", *second, LR.forward_truth(name, 1))
    print("RATIO %-24s second %.2f" % (name, ratio))
    LR.check(name + " first again", *third, LR.forward_truth(name))
    assert torch.equal(third[0], first[0]) and torch.equal(third[1], first[1]), "the first pair's result changed after another pair"
    # and the loop alone on the same captured state, after whole forwards have adopted their own buffers
    lo, up = _iterate(model, name)
    c = _case(name)
    assert torch.equal(lo, c["lo"]) and torch.equal(up, c["up"]), "iterate() on the same operands changed after whole forwards"


@pytest.mark.parametrize("name", BATCH_CASES)
def test_batch_against_items_alone(name):
    model = _case(name)["model"]
    lo, up = _forward(model, name)
    t = LR.forward_truth(name)
    worst = 0.0
    for b in range(lo.shape[0]):
        one_lo, one_up = _forward(model, name, items=slice(b, b + 1))
        for k, got, want in (("lo", one_lo[:, :1], lo[b:b + 1, :1]), ("up", one_up, up[b:b + 1])):
            err = float((got - want).abs().max())
            worst = max(worst, err / t[k + "_unit"])
            print("LOOP %-44s %s item %d alone against the batch: err %.3e ratio %.2f" % (name, k, b, err, err / t[k + "_unit"]))
            assert err <= t[k + "_bound"]
    print("RATIO %-24s batch %.2f" % (name, worst))
    # back to the batch: the state of the full shape is built again (scales from this pair this time)
    LR.check(name + " batch again", *_forward(model, name), t)


@pytest.mark.parametrize("name", MIXED_CASES)
def test_mixed_precision(name):
    """The key on: the loop alone, the whole forward and a second pair against the fp64 truth under the bound of their own
    yardstick (fp16-rounded convolution operands), the route asserted.  The key off on the same weights: the fp32-class
    bound; and the key is visible (the two differ by more than test_gpu_round6's 1e-6)."""
    from dkt_stereo_amd import conv
    on = _fresh(name)
    with LR.route_log(on) as names:
        lo_on, up_on = _iterate(on, name)
    route = LR.route_of(names, on)
    print("ROUTE %-24s %s" % (name, route))
    ratio = LR.check(name + " loop", lo_on, up_on, LR.mixed_truth(name, False))
    assert route == LR.BY_NAME[name][4], "%s took '%s', the table expects '%s'" % (name, route, LR.BY_NAME[name][4])
    first = _forward(on, name)
    ratio = max(ratio, LR.check(name + " forward", *first, LR.mixed_truth(name, True)))
    ratio = max(ratio, LR.check(name + " second pair", *_forward(on, name, 1), LR.mixed_truth(name, True, 1)))
    print("RATIO %-24s mixed %.2f" % (name, ratio))
    third = _forward(on, name)
    assert torch.equal(third[0], first[0]) and torch.equal(third[1], first[1])
    assert conv.get_backend() == "f16x3"
    off = _fresh(name, mixed_precision=False)
    lo_off, up_off = _iterate(off, name)
    LR.check(name + " loop, key off", lo_off, up_off, LR.loop_truth(name))
    LR.check(name + " forward, key off", *_forward(off, name), LR.forward_truth(name))
    d = float((up_on - up_off).abs().max())
    print("LOOP %-44s mixed_precision on against off, loop alone: max|d| %.3e" % (name, d))
    assert d > 1e-6


# ---- IGEV: the loop alone where the fused geometry lookup does not apply ---------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("name", LR.IGEV_NAMES)
def test_igev_loop_without_the_fused_lookup(name):
    """igev_loop.igev_iterate at radius 3, three levels and four geometry channels (C8LoopIGEV._motion_front's fall-through:
    lookup tensor, conv2d, pack) on 17 x 27 against _igev_train_ref's loop in fp64, the route asserted; a second pair's
    geometry volume through the same captured state, then the first again."""
    from dkt_stereo_amd import _ffi, igev_loop, loop_c8
    from dkt_stereo_amd.geometry import Combined_Geo_Encoding_Volume
    c = LR.igev_case(name)
    blk, x, cfg = copy.deepcopy(c["blk"]).cuda().eval(), c["x"], c["cfg"]
    net, inp = _dev(x["net"]), _dev(x["inp"])
    assert loop_c8.eligible_igev(blk, net[0].shape)

    def run(geo, disp, cache):
        geo_fn = Combined_Geo_Encoding_Volume(x["m1"].cuda(), x["m2"].cuda(), geo.cuda(), num_levels=cfg["corr_levels"], radius=cfg["corr_radius"])
        d, m, n = igev_loop.igev_iterate(blk, geo_fn, disp.cuda(), x["coords"].cuda(), [t.clone() for t in net], inp, LR.IGEV_ITERS, cache=cache)
        return dict(disp=d.clone(), mask=m.clone(), net0=n[0].clone(), net1=n[1].clone(), net2=n[2].clone())

    cache = {}
    with _ffi.launch_log() as names:
        got = run(x["geo"], x["disp"], cache)
    lp = getattr(cache["state"], "c8", None)
    graphs = [] if lp is None else [d for d in (lp.graph, lp.graph_n, lp.graph_last) if d]
    route = "%s geo %s %s" % ("c8" if lp is not None else "round2", "fused" if "dkt_geo_lookup_conv1x1" in names else
                              "lookup+conv2d" if "dkt_geo_lookup" in names else "?", "captured" if graphs else "eager")
    print("ROUTE %-24s %s" % (name, route))
    ratio = LR.igev_check(name, got, LR.igev_truth(name))
    print("RATIO %-24s igev %.2f" % (name, ratio))
    assert route == LR.IGEV_ROUTE
    other = run(x["geo"].flip(2) * 0.5, (8.0 - x["disp"]), cache)         # another volume and start through the same state
    assert float((other["disp"] - got["disp"]).abs().max()) > 1e-2
    again = run(x["geo"], x["disp"], cache)
    for k in got:
        assert torch.equal(again[k], got[k]), "%s: %s changed after another pair went through the captured state" % (name, k)
