"""Module-level parity of the encoders (-m gpu): BasicEncoder, MultiBasicEncoder and RAFTStereo.encode() on the HIP path
against an fp64 restatement of the same module with stock torch operators (tests/_encoder_ref.py, oracle/torch_oracle.py).

Bound, per output tensor, metric max|got - truth| / max|truth|:

    err_hip <= 8 * max(err_yardstick, 2.9e-7)

where the yardstick is the same restatement in fp32 on the CPU (the error of the reference's own arithmetic on this very
input; the fp64 truth is evaluated with the same stock operators on the device, which is several times faster); a case is valid only if its yardstick is <= 1e-5 (asserted here, proven for the fixed cases without a GPU by
test_host_encoder_ref.py).  Where 8 and 2.9e-7 come from: _encoder_ref's docstring.  f16x2, f16 and args.mixed_precision
are not parity paths and are not tested here: the reduced-pass convolutions are held to the fp64 convolution of their rounded
operands, operator by operator, in tests/test_gpu_conv2d_reduced_passes.py (conv2d_f16s) and tests/test_gpu_round5.py (conv_c8).

Every comparison prints `ENC <case> <tensor> err yardstick ratio` before it asserts.

Which test holds which path to the truth:
  test_basic_encoder_matches_fp64 / test_multi_encoder_matches_fp64   the configuration matrix (norm kind, downsample, size,
      batch, list input, output widths, num_layers, one head, mixed-width heads, dual_inp, begun)
  test_*_random                                                      hypothesis-drawn shapes and configurations (20 examples each)
  test_weights_stationary_kernel_inside_the_encoders                 conv_ws.h inside both encoders, DKT_CONV_WS on / off
  test_every_switch_side_matches_fp64                                FUSE_ENCODER, EPILOGUE_STATS, CNET_STREAMS, PAIR_HEADS on
      and off, C8_ENCODER on
  test_hard_images_match_fp64                                        low contrast, flat halves, flat, raw 0 ... 255
  test_raft_encode_matches_fp64, test_encode_into_the_captured_loop_buffers_matches_fp64, test_benchmark_shape_encode_matches_fp64
  test_stage_by_stage                                                every stage fed the fp32-rounded truth of its input
  test_instance_norm_of_a_single_pixel_plane_is_zero                 what the library does below 32 pixels per plane

Largest err_hip / max(err_yardstick, 2.9e-7) measured on an MI355X (bound: 8):
  BasicEncoder        instance 1.71, batch 1.65, none 1.63, group 2.03
  MultiBasicEncoder   instance 2.19, batch 2.82, none 3.21, group 2.58
  RAFTStereo.encode() 3.90 (cz of the 1/4 scale, 64 x 128; every backbone and switch between 2.7 and 3.9)
  736 x 1248          0.96 against the device's fp32 yardstick, 3.7 against the CPU's
  switch sides <= 2.62 (C8_ENCODER, cnet / batch), weights-stationary cases <= 2.80, hard images <= 1.82, single stages <= 2.96
No case came near the bound, and no kernel or path had to be changed.

Value-only mutants this file was run against once each (built aside, never kept); failing cases of the 92 here, and what the rest
of the -m gpu suite (606 cases) noticed:
  1 instnorm_finalize divides the variance by N - 1      43 here (every instance-norm case); 91 there, operator and e2e tests
  2 ReLU applied to norm3 in the lazy join               44 here; 26 there (the end-to-end fixtures)
  3 folded BatchNorm without eps                         45 here; there only test_batchnorm_fold_matches_unfolded_fp64
  4 epilogue statistics skip the last partial row tile   21 here; there only the statistics operator tests, no end-to-end test
  5 conv_ws residual epilogue reads batch element 0      test_weights_stationary_kernel_inside_the_encoders[cnet-batch-2] and
                                                         test_stage_by_stage[2x203x261-cnet-batch]; there the conv_ws operator test
  6 stem filter taps shifted by one column               79 here; 65 there
  7 dual_inp hands the heads the second half             every dual_inp case and encode()[shared_backbone]; there test_raft_backbone_variants
"""
import contextlib

import pytest
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

import _encoder_ref as er

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SET = dict(deadline=None, max_examples=20, suppress_health_check=list(HealthCheck), derandomize=True)


def _dev(x):
    return [t.to(DEV) for t in x] if isinstance(x, (list, tuple)) else x.to(DEV)


@contextlib.contextmanager
def _parity_backend():
    from dkt_stereo_amd import conv
    with torch.no_grad(), conv.use_backend("f16x3"):
        yield


_REFS = {}


def _ref(key, fn, sd, x):
    """(truth, yardstick errors); kept under `key` when one is given (the switch cases ask for the same three nine times)."""
    if key is None or key not in _REFS:
        truth, _, yerr = er.truth_and_yardstick(fn, sd, x, truth_device=DEV)
        if key is None:
            return truth, yerr
        _REFS[key] = (truth, yerr)
    return _REFS[key]


def _check_basic(label, m, x, norm, ds, pair, key=None):
    """m: BasicEncoder on the CPU; x: tensor, or [left, right] when pair."""
    truth, yerr = _ref(key, lambda sd, v: er.basic(sd, v, norm, ds, pair), er.prefixed(m, "fnet"), x)
    m.to(DEV)
    with _parity_backend():
        got = m(_dev(x))
        torch.cuda.synchronize()
    return er.compare(label, list(got) if pair else [got], truth, yerr, ["fmap1", "fmap2"] if pair else ["fmap"])


def _check_multi(label, m, x, norm, ds, nl, n_heads, dual=False, begun=False, key=None):
    truth, yerr = _ref(key, lambda sd, v: er.multi(sd, v, norm, ds, nl, n_heads, dual), er.prefixed(m, "cnet"), x)
    m.to(DEV)
    with _parity_backend():
        xd = x.to(DEV)
        got = m(xd, dual_inp=dual, num_layers=nl, begun=m._trunk_begin(xd) if begun else None)
        torch.cuda.synchronize()
    assert len(got) == nl + int(dual) and all(len(s) == n_heads for s in got[:nl])
    return er.compare(label, got, truth, yerr, er.multi_names(nl, n_heads, dual))


def _assert_vendor_stem(m):
    """downsample = 3: the 7x7 stride-2 stem is outside dkt_conv2d_stem7 (stride 1) and dkt_conv2d_f16s_desc (1x1 / 3x3) and goes to
    the vendor convolution by design (conv.conv2d); it is compared with the truth like every other layer."""
    from dkt_stereo_amd import conv
    assert m.conv1.stride == (2, 2) and not conv.direct_eligible(m.conv1) and not conv.hip_eligible(m.conv1)


def _assert_torch_norm_path(m, x):
    """Group norm is torch's by design (extractor.norm_act): neither folded into the convolution nor the HIP instance norm."""
    from dkt_stereo_amd import extractor
    assert isinstance(m.norm1, torch.nn.GroupNorm) and not extractor._plain_instance_norm(m.norm1)
    assert not extractor._foldable(m.conv1, m.norm1, x)


# -- a. the configuration matrix ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", er.BASIC_CASES, ids=er.case_id)
def test_basic_encoder_matches_fp64(case):
    norm, ds, B, H, W, pair, odim = case
    m = er.make_basic(norm, ds, odim, 3)
    x = er.images(3, B, H, W)
    if norm == "group":
        _assert_torch_norm_path(m, x[0].to(DEV))
    if ds == 3:
        _assert_vendor_stem(m)
    _check_basic("basic " + er.case_id(case), m, list(x) if pair else x[0], norm, ds, pair)


@pytest.mark.parametrize("case", er.MULTI_CASES, ids=er.case_id)
def test_multi_encoder_matches_fp64(case):
    norm, ds, B, H, W, nl, dims, dual, begun = case
    m = er.make_multi(norm, ds, dims, 3)
    x = er.images(3, B, H, W)[0]
    if norm == "group":
        _assert_torch_norm_path(m, x.to(DEV))
    if ds == 3:
        _assert_vendor_stem(m)
    _check_multi("multi " + er.case_id(case), m, x, norm, ds, nl, len(dims), dual, begun)


# -- b. randomised -----------------------------------------------------------------------------------------------------------
@st.composite
def _configs(draw, multi):
    """(norm, downsample, num_layers, B, H, W), H, W <= 80.  Instance norm: the coarsest normalised plane (h, w with h * w >= 32)
    is drawn first and H, W are built up from it -- times the total stride S, minus a remainder below S, which keeps
    ceil(H / S) = h -- so that no example has to be rejected."""
    norm = draw(st.sampled_from(["instance", "batch", "none", "group"]))
    ds = draw(st.integers(0, 3))
    B = draw(st.integers(1, 3))
    if norm != "instance":
        nl = draw(st.integers(1, 3)) if multi else 0
        return norm, ds, nl, B, draw(st.integers(1, 80)), draw(st.integers(1, 80))
    # total stride <= 8: 80 // 16 = 5 rows and columns cannot hold 32 pixels
    nl = draw(st.integers(1, min(3, 4 - ds))) if multi else 0
    S = 1 << (ds + max(nl - 1, 0))
    top = 80 // S
    h = draw(st.integers(-(-32 // top), top))
    w = draw(st.integers(-(-32 // h), top))
    return norm, ds, nl, B, h * S - draw(st.integers(0, S - 1)), w * S - draw(st.integers(0, S - 1))


@settings(**SET)
@given(cfg=_configs(False), pair=st.booleans(), seed=st.integers(0, 10 ** 6))
def test_basic_encoder_random(cfg, pair, seed):
    norm, ds, _, B, H, W = cfg
    m = er.make_basic(norm, ds, 128, seed)
    x = er.images(seed, B, H, W)
    _check_basic("basic-random %s-%d-%d-%dx%d-%s-%d" % (norm, ds, B, H, W, pair, seed), m, list(x) if pair else x[0], norm, ds, pair)


@settings(**SET)
@given(cfg=_configs(True), one=st.booleans(), dual=st.booleans(), seed=st.integers(0, 10 ** 6))
def test_multi_encoder_random(cfg, one, dual, seed):
    norm, ds, nl, B, H, W = cfg
    m = er.make_multi(norm, ds, er.ONE if one else er.SAME, seed)
    x = er.images(seed, B + (dual and B == 1), H, W)[0]
    _check_multi("multi-random %s-%d-%d-%d-%dx%d-%s-%s-%d" % (norm, ds, nl, x.shape[0], H, W, one, dual, seed), m, x, norm, ds, nl,
                 1 if one else 2, dual)


# -- c. above the weights-stationary gate ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", er.WS_CASES, ids=er.case_id)
def test_weights_stationary_kernel_inside_the_encoders(case, monkeypatch):
    """203 x 261 (26 x 9 tiles of 8 x 32 per image, ragged on both sides, >= 192 with the batch): the 64 -> 64 layers take
    conv_ws.h with DKT_CONV_WS at its default and the streaming kernel with DKT_CONV_WS=0 (read per launch).  The two runs
    differ in bits (below the gate they are bit-identical: test_weights_stationary_conv_is_reproducible_and_gated); each is
    compared with the truth on its own."""
    enc, norm, B = case
    H, W = er.WS_SIZE
    x = er.images(3, B, H, W)
    if enc == "fnet":
        m = er.make_basic(norm, 2, 256, 3)
        fn, sd, xin, names = (lambda s, v: er.basic(s, v, norm, 2, True)), er.prefixed(m, "fnet"), list(x), ["fmap1", "fmap2"]
        run = lambda: list(m(_dev(xin)))
    else:
        m = er.make_multi(norm, 2, er.SAME, 3)
        fn, sd, xin, names = (lambda s, v: er.multi(s, v, norm, 2)), er.prefixed(m, "cnet"), x[0], er.multi_names(3, 2, False)
        run = lambda: er.flatten(m(_dev(xin)))
    truth, _, yerr = er.truth_and_yardstick(fn, sd, xin, truth_device=DEV)
    m.to(DEV)
    outs = {}
    with _parity_backend():
        for ws in ("default", "0"):
            if ws == "default":
                monkeypatch.delenv("DKT_CONV_WS", raising=False)
            else:
                monkeypatch.setenv("DKT_CONV_WS", ws)
            outs[ws] = run()
            torch.cuda.synchronize()
    assert any(not torch.equal(a, b) for a, b in zip(outs["default"], outs["0"])), "both runs took the same 64 -> 64 kernel"
    for ws in outs:
        er.compare("ws %s DKT_CONV_WS=%s" % (er.case_id(case), ws), outs[ws], truth, yerr, names)


# -- d. every switch side against the truth ----------------------------------------------------------------------------------
SWITCHES = [("FUSE_ENCODER", False), ("FUSE_ENCODER", True), ("EPILOGUE_STATS", False), ("EPILOGUE_STATS", True),
            ("CNET_STREAMS", False), ("CNET_STREAMS", True), ("PAIR_HEADS", False), ("PAIR_HEADS", True), ("C8_ENCODER", True)]


@pytest.mark.parametrize("switch,value", SWITCHES, ids=["%s=%d" % s for s in SWITCHES])
def test_every_switch_side_matches_fp64(switch, value, monkeypatch):
    """fnet / instance (B = 2 as [left, right]), cnet / batch and cnet / instance at 96 x 160 with one switch of extractor.py
    set; everything else at its default.  C8_ENCODER: C8_ENCODER_MIN_PIXELS patched to 0 so that this size takes the C8S
    full-resolution stage (asserted)."""
    from dkt_stereo_amd import extractor
    monkeypatch.setattr(extractor, switch, value)
    if switch == "C8_ENCODER":
        monkeypatch.setattr(extractor, "C8_ENCODER_MIN_PIXELS", 0)
    x = er.images(3, 1, 96, 160)
    f = er.make_basic("instance", 2, 256, 3)
    cb = er.make_multi("batch", 2, er.SAME, 3)
    ci = er.make_multi("instance", 2, er.SAME, 3)
    if switch == "C8_ENCODER":
        with _parity_backend():
            assert f.to(DEV)._layer1_c8_kind(torch.cat(x).to(DEV)) == "instance" and cb.to(DEV)._layer1_c8_kind(x[0].to(DEV)) == "batch"
    label = "switch %s=%d " % (switch, value)
    _check_basic(label + "fnet/instance", f, list(x), "instance", 2, True, key="switch fnet")
    _check_multi(label + "cnet/batch", cb, x[0], "batch", 2, 3, 2, key="switch cnet/batch")
    if switch != "C8_ENCODER":          # (cnet / instance has no C8S form beyond the one fnet / instance shows)
        _check_multi(label + "cnet/instance", ci, x[0], "instance", 2, 3, 2, key="switch cnet/instance")


# -- e. hard images ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", er.HARD_IMAGES)
def test_hard_images_match_fp64(kind):
    """The inputs on which deferred normalisation and epilogue statistics differ most from a separate pass."""
    H, W = er.HARD_SIZE
    x = er.hard_image(kind, 3, 1, H, W)
    _check_basic("hard %s fnet/instance" % kind, er.make_basic("instance", 2, 256, 3), x, "instance", 2, False)
    _check_multi("hard %s cnet/instance" % kind, er.make_multi("instance", 2, er.SAME, 3), x, "instance", 2, 3, 2)


# -- f. RAFTStereo.encode() ------------------------------------------------------------------------------------------------------
def _raft_names(n):
    return ["fmap1", "fmap2"] + ["net%d" % i for i in range(n)] + ["c%s%d" % (g, i) for i in range(n) for g in "zrq"]


def _check_encode(label, model, i1, i2, ref_device="cpu", **attrs):
    truth, _, yerr = er.truth_and_yardstick(lambda sd, v: er.raft_encode(sd, vars(model.args), v[0], v[1]), model, [i1, i2],
                                            ref_device, DEV)
    model.to(DEV)
    for k, v in attrs.items():
        setattr(model, k, v)
    worst = 0.0
    with _parity_backend():
        for rep in range(2 if attrs.get("graph_encoders") else 1):      # graph_encoders: the eager capture call, then a replay
            got = model.encode(i1.to(DEV), i2.to(DEV))
            torch.cuda.synchronize()
            worst = max(worst, er.compare(label + (" replay" if rep else ""), list(got), truth, yerr, _raft_names(model.args.n_gru_layers)))
    return worst


@pytest.mark.parametrize("cfg", er.RAFT_CASES, ids=er.case_id)
def test_raft_encode_matches_fp64(cfg):
    """encode() on images in 0 ... 255 (dkt_normalize_pair inside the comparison) against raft_prepare / the restated
    variants: default backbone, shared_backbone, 'interpolate'; n_gru_layers 1 ... 3; B 1 and 2."""
    kw, B = cfg
    _check_encode("encode " + er.case_id(cfg), er.make_raft(kw, 3), *er.raft_images(3, B, 64, 128))


ENCODE_SWITCHES = [dict(encoder_streams=False), dict(cnet_first=False), dict(graph_encoders=True),
                   dict(encoder_streams=True, cnet_first=True, graph_encoders=False)]


@pytest.mark.parametrize("attrs", ENCODE_SWITCHES, ids=lambda a: "+".join("%s=%d" % kv for kv in a.items()))
def test_raft_encode_switches_match_fp64(attrs):
    """encoder_streams / cnet_first / graph_encoders on and off (the last entry: every one at its default, set explicitly),
    default backbone, 100 x 187, B = 1.  With graph_encoders the second call is the captured pass's replay."""
    _check_encode("encode " + "+".join("%s=%d" % kv for kv in attrs.items()), er.make_raft({}, 4), *er.raft_images(4, 1, 100, 187),
                  **attrs)


def test_encode_into_the_captured_loop_buffers_matches_fp64():
    """After forward() has built the captured loop for a shape, encode() on ANOTHER pair writes the hidden states and context
    terms straight into the loop's buffers (RAFTStereo._context_targets): those buffers against the truth of that pair."""
    model = er.make_raft({}, 5)
    a1, a2 = er.raft_images(5, 1, 64, 128)
    b1, b2 = er.raft_images(6, 1, 64, 128)
    truth, _, yerr = er.truth_and_yardstick(lambda sd, v: er.raft_encode(sd, vars(model.args), v[0], v[1]), model, [b1, b2],
                                            truth_device=DEV)
    model.to(DEV)
    with _parity_backend():
        for _ in range(2):
            model(a1.to(DEV), a2.to(DEV), iters=3, test_mode=True)
        f1, f2, net, inp = model.encode(b1.to(DEV), b2.to(DEV))
        torch.cuda.synchronize()
        state = model._graph_state
        assert state is not None and [t.data_ptr() for t in net] == [t.data_ptr() for t in state["net"]]
        assert [t.data_ptr() for s in inp for t in s] == [t.data_ptr() for s in state["inp"] for t in s]
        er.compare("encode into loop buffers", [f1, f2, list(state["net"]), [list(s) for s in state["inp"]]], truth, yerr, _raft_names(3))


# -- g. the benchmark shape -------------------------------------------------------------------------------------------------------
def test_benchmark_shape_encode_matches_fp64():
    """1 x 3 x 736 x 1248, default configuration, through encode().  Truth (fp64) and yardstick (fp32) are computed with stock
    torch operators ON THE DEVICE, vendor convolution library off (_encoder_ref.truth_and_yardstick): on a CPU they take two
    minutes.  Every other case computes them on the CPU.  The device's fp32 sums are less accurate than the CPU's (yardstick
    1.6e-6 ... 3.3e-6 against 4.7e-7 ... 2.3e-6 for this input on a CPU), so this case's bound is the looser one; measured on
    an MI355X: err_hip 1.3e-6 ... 2.1e-6, at most 0.96 x the device yardstick and 3.7 x the CPU one (cz0)."""
    _check_encode("encode 736x1248", er.make_raft({}, 3), *er.raft_images(3, 1, 736, 1248), ref_device=DEV)


# -- stage tests, so that a failure names a place -------------------------------------------------------------------------------
def _hip_stage(m, name, x, n_heads=2):
    from dkt_stereo_amd import extractor
    if name == "stem":              # (the LazyNorm the fused path hands to layer1, materialised: the same separate pass)
        return extractor.conv_norm_act(m.conv1, m.norm1, x, True)
    if name == "stem+layer1":
        return m._trunk_begin(x)
    if name.startswith("outputs"):
        return m._heads(getattr(m, name), x)
    return getattr(m, name)(x)


@pytest.mark.parametrize("enc,norm", [("fnet", "instance"), ("cnet", "batch")])
@pytest.mark.parametrize("size", [(1, 64, 128), (2,) + er.WS_SIZE], ids=["64x128", "2x203x261"])
def test_stage_by_stage(enc, norm, size):
    """The default fnet and cnet: every stage (stem + norm + ReLU; layer1; layer2; layer3; conv2 or each scale's heads; layer4;
    layer5) is fed the fp32-rounded TRUTH of its input and compared with the truth of that stage on that input, under the
    same bound with the yardstick of that stage (its fp32 restatement on the same input).  The fused path hands layer1 a
    LazyNorm instead of the stem's output: the stem is compared materialised, and stem + layer1 are also run together."""
    B, H, W = size
    m = er.make_basic(norm, 2, 256, 3) if enc == "fnet" else er.make_multi(norm, 2, er.SAME, 3)
    sd = er.prefixed(m, enc)
    sd64 = er.cast_sd(sd, torch.float64)
    x = er.images(3, B, H, W)[0]
    stages = er.stages(enc, norm, 2)
    m.to(DEV)
    feeds, failures = {"image": x}, []
    for name, src, fn in stages:
        xin = feeds[src]
        truth, _, yerr = er.truth_and_yardstick(fn, sd, xin, truth_device=DEV)
        feeds[name] = truth[0].float().cpu() if len(truth) == 1 else None
        with _parity_backend():
            got = _hip_stage(m, name, xin.to(DEV))
            torch.cuda.synchronize()
        try:
            er.compare("stage %s/%s %dx%dx%d %s" % (enc, norm, B, H, W, name), got, truth, yerr)
        except AssertionError as e:
            failures.append(str(e))
    both = lambda s, v: stages[1][2](s, stages[0][2](s, v))
    truth, _, yerr = er.truth_and_yardstick(both, sd, x, truth_device=DEV)
    with _parity_backend():
        got = _hip_stage(m, "stem+layer1", x.to(DEV))
        torch.cuda.synchronize()
    try:
        er.compare("stage %s/%s %dx%dx%d stem+layer1" % (enc, norm, B, H, W), got, truth, yerr)
    except AssertionError as e:
        failures.append(str(e))
    assert not failures, "\n".join(failures)


# -- small planes ----------------------------------------------------------------------------------------------------------------
def test_instance_norm_of_a_single_pixel_plane_is_zero():
    """Below 32 pixels per plane an instance norm is ill-conditioned in any arithmetic and no tolerance is claimed; this pins
    what the library does at the end of that range.  On a 1 x 1 plane the formula gives exactly (x - mean) * rsqrt(0 + eps)
    = 0 (stock torch refuses such a plane).  dkt_instance_norm, the lazy join and the in_norm staging all return that:
    norm -> 0, join -> relu(residual), convolution of the normalised input -> its bias; a whole residual block -> relu(x)."""
    from dkt_stereo_amd import conv, extractor
    torch.manual_seed(9)
    norm = torch.nn.InstanceNorm2d(64)
    x = (torch.randn(3, 64, 1, 1) * 5 + 2).to(DEV)
    c = (torch.randn(3, 64, 1, 1) * 3 - 1).to(DEV)
    layer = extractor._Conv2d(64, 64, 3, padding=1).to(DEV)
    blk = extractor.ResidualBlock(64, 64, "instance").to(DEV).eval()
    with _parity_backend():
        for relu in (False, True):
            y = extractor.norm_act(norm, x, relu)
            assert y.shape == x.shape and bool((y == 0).all())
        p = extractor.instance_norm_params(norm, x)
        assert bool(torch.isfinite(p).all()) and torch.equal(p[:, 0].view_as(x), x)
        assert torch.equal(extractor.norm_add_relu(norm, x, c), torch.relu(x))                               # eager residual
        for relu in (False, True):                                                                           # lazy residual -> 0
            y = extractor.norm_add_relu(norm, extractor.LazyNorm(norm, x, relu), c)
            assert bool((y == 0).all())
        assert conv.fused_eligible(layer, True)
        y = conv.conv2d_fused(x, layer, in_norm=p)
        assert torch.equal(y, layer.bias.view(1, -1, 1, 1).expand_as(y))
        if conv.stats_eligible(layer):
            y, s = conv.conv2d_stats(x, layer, in_norm=p)
            q = extractor.instance_norm_params(norm, y, s)
            assert torch.equal(y, layer.bias.view(1, -1, 1, 1).expand_as(y)) and torch.equal(q[:, 0].view_as(y), y)
        y = blk(x)
        assert bool(torch.isfinite(y).all()) and torch.equal(y, torch.relu(x))
        y = blk(extractor.LazyNorm(norm, x, True))
        assert bool((y == 0).all())
        torch.cuda.synchronize()
