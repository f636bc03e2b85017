"""The encoder restatement (tests/_encoder_ref.py, oracle/torch_oracle.py) without a GPU.

* In fp32 it equals the `extractor` modules on the CPU (their torch path: the same stock operators) for the four norm kinds,
  the four downsample values, dual_inp, one head and num_layers 1 ... 3, at two odd sizes.
* The yardstick (fp32 restatement against the fp64 one) of every fixed case of test_gpu_encoders.py is <= 1e-5: the
  validity condition of the GPU bound, checked where no GPU is needed.  The RAFT-Stereo cases run at a reduced size here
  (the 736 x 1248 case is not part of this file).
"""
import pytest
import torch

import _encoder_ref as er
import _synth

SIZES = [(37, 53), (33, 47)]


def _close(label, got, want):
    got, want = er.flatten(got), er.flatten(want)
    assert len(got) == len(want), label
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (label, i)
        assert float((g - w).abs().max()) <= 1e-5 * float(w.abs().max()), (label, i)


@pytest.mark.parametrize("norm", ["instance", "batch", "none", "group"])
@pytest.mark.parametrize("ds", [0, 1, 2, 3])
@torch.no_grad()
def test_restatement_equals_the_modules_on_the_cpu(norm, ds):
    H, W = SIZES[ds % 2]
    if norm == "instance":                      # at least 32 pixels in the coarsest normalised plane
        H, W = H << max(ds - 1, 0), W << max(ds - 1, 0)
        H, W = H - (ds > 1), W - (ds > 1)
    x, y = er.images(3, 2, H, W)
    fnet = er.make_basic(norm, ds, 128 + 128 * (ds % 2), 11 + ds)
    sd = er.cast_sd(er.prefixed(fnet, "fnet"), torch.float32)
    _close("tensor", [fnet(x)], er.basic(sd, x, norm, ds))
    _close("pair", fnet([x, y]), er.basic(sd, [x, y], norm, ds, pair=True))
    for dims, nl, dual in ((er.SAME, 3, False), (er.ONE, 2, False), (er.MIXED, 1, True), (er.MIXED, 2 if norm == "instance" else 3, True)):
        cnet = er.make_multi(norm, ds, dims, 17 + ds)
        sd = er.cast_sd(er.prefixed(cnet, "cnet"), torch.float32)
        _close((dims, nl, dual), cnet(x, dual_inp=dual, num_layers=nl), er.multi(sd, x, norm, ds, nl, len(dims), dual))


@pytest.mark.parametrize("cfg", [dict(shared_backbone=True), dict(backbone_type="interpolate", n_gru_layers=2),
                                 dict(shared_backbone=True, n_gru_layers=1, context_norm="instance")],
                         ids=["shared", "interpolate-two", "shared-one-instance"])
@torch.no_grad()
def test_raft_encode_restatement_equals_the_model_parts_on_the_cpu(cfg):
    """The non-default backbones and the context post-processing against the model's own modules on the CPU
    (RAFTStereo._variant_features is plain torch there; _context_post itself has no CPU path, so its three operators are
    applied with the model's nn.Conv2d).  The default backbone is torch_oracle.raft_prepare, pinned by test_oracle.py."""
    model = er.make_raft(cfg, 5)
    i1, i2 = (torch.from_numpy(a) for a in _synth.image_pair(4, 2, 45, 75, 12))
    a, b, _ = model._normalized_pair(i1, i2)
    scales, f1, f2 = model._variant_features(a, b, model.args.n_gru_layers)
    net = [torch.tanh(s[0]) for s in scales]
    inp = [list(model.context_zqr_convs[i](torch.relu(s[1])).split(model.args.hidden_dims[i], 1)) for i, s in enumerate(scales)]
    want = er.raft_encode(er.cast_sd(model, torch.float32), vars(model.args), i1, i2)
    _close(str(cfg), [f1, f2, net, inp], want)


def _under_cap(label, fn, sd, x):
    _, _, errs = er.truth_and_yardstick(fn, sd, x)
    print("YARDSTICK %-50s %s" % (label, " ".join("%.2e" % e for e in errs)))
    assert max(errs) <= er.CAP, (label, errs)


@pytest.mark.parametrize("case", er.BASIC_CASES, ids=er.case_id)
def test_yardstick_of_the_basic_encoder_cases_is_under_the_cap(case):
    norm, ds, B, H, W, pair, odim = case
    m = er.make_basic(norm, ds, odim, 3)
    x = er.images(3, B, H, W)
    _under_cap(er.case_id(case), lambda sd, v: er.basic(sd, v, norm, ds, pair), er.prefixed(m, "fnet"), list(x) if pair else x[0])


@pytest.mark.parametrize("case", er.MULTI_CASES, ids=er.case_id)
def test_yardstick_of_the_multi_encoder_cases_is_under_the_cap(case):
    norm, ds, B, H, W, nl, dims, dual, _ = case
    m = er.make_multi(norm, ds, dims, 3)
    x = er.images(3, B, H, W)[0]
    _under_cap(er.case_id(case), lambda sd, v: er.multi(sd, v, norm, ds, nl, len(dims), dual), er.prefixed(m, "cnet"), x)


@pytest.mark.parametrize("case", er.WS_CASES, ids=er.case_id)
def test_yardstick_above_the_weights_stationary_gate_is_under_the_cap(case):
    enc, norm, B = case
    H, W = er.WS_SIZE
    x = er.images(3, B, H, W)
    if enc == "fnet":
        m = er.make_basic(norm, 2, 256, 3)
        _under_cap(er.case_id(case), lambda sd, v: er.basic(sd, v, norm, 2, True), er.prefixed(m, "fnet"), list(x))
    else:
        m = er.make_multi(norm, 2, er.SAME, 3)
        _under_cap(er.case_id(case), lambda sd, v: er.multi(sd, v, norm, 2), er.prefixed(m, "cnet"), x[0])


@pytest.mark.parametrize("kind", er.HARD_IMAGES)
def test_yardstick_of_the_hard_images_is_under_the_cap(kind):
    H, W = er.HARD_SIZE
    x = er.hard_image(kind, 3, 1, H, W)
    f = er.make_basic("instance", 2, 256, 3)
    _under_cap("fnet " + kind, lambda sd, v: er.basic(sd, v, "instance", 2), er.prefixed(f, "fnet"), x)
    c = er.make_multi("instance", 2, er.SAME, 3)
    _under_cap("cnet " + kind, lambda sd, v: er.multi(sd, v, "instance", 2), er.prefixed(c, "cnet"), x)


@pytest.mark.parametrize("cfg", er.RAFT_CASES, ids=er.case_id)
def test_yardstick_of_the_raft_encode_cases_is_under_the_cap(cfg):
    """The cases of test_raft_encode_matches_fp64 at their own size; with the default configuration also the inputs of the
    switch cases (100 x 187) and of the captured-loop case, and the benchmark shape's input at 92 x 156."""
    kw, B = cfg
    model = er.make_raft(kw, 3)
    fn = lambda sd, v: er.raft_encode(sd, vars(model.args), v[0], v[1])
    _under_cap(er.case_id(cfg) + " 64x128", fn, model, list(er.raft_images(3, B, 64, 128)))
    if not kw and B == 1:
        _under_cap("benchmark input at 92x156", fn, model, list(er.raft_images(3, 1, 92, 156)))
        _under_cap("switch cases 100x187", fn, er.make_raft({}, 4), list(er.raft_images(4, 1, 100, 187)))
        _under_cap("captured-loop case 64x128", fn, er.make_raft({}, 5), list(er.raft_images(6, 1, 64, 128)))
