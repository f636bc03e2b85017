"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

The fp64 truth of a whole RAFT-Stereo training step (test_host_raft_train_ref.py, test_gpu_raft_train.py).

train_forward() restates RAFTStereo._forward_train line for line on a state dict, in the dtype of that state dict: encode,
pyramid, then per iteration coords1.detach(), lookup, the optional slow-fast calls, the update block, the y component of the
update replaced by zeros without an in-place write, convex_upsample(...)[:, :1].  It is built from oracle/torch_oracle.py
(_conv, _norm, conv_gru, pool2x, interp, corr1d_pyramid, _sample_rows, convex_upsample); what the oracle forces to fp32
(raft_prepare's and corr1d_lookup's .float(), the fp32 taps) or writes in place (raft_iterations' delta[:, 1] = 0.0) is
restated here, and so are the functions that hold a ReLU, because every ReLU records its mask:

    record.append((site, input > 0))

in the order RAFTStereo._forward_train evaluates them: the context encoder (per residual block norm1, norm2 -- the join's
inner ReLU --, join), the feature encoder (or the shared backbone's conv2.0 block), relu(x[1]) in front of each
context_zqr_convs.i, then per iteration the motion encoder's five and the two heads.  Site names are state-dict prefixes.

Why masks: the network's gradient is discontinuous where a ReLU input changes sign, and an fp32 forward puts a few of the
4.3 million activations on the other side of 0 from fp64.  Measured on the CPU, this restatement in fp32 against itself in
fp64 (test_host_raft_train_ref.py prints the figures): 10 of the 20 draws have no such flip, and on those the worst
parameter gradient error is 5.2e-6 ... 1.8e-5; with a flip it is typically 1.6e-3 ... 9.5e-2 (one flip inside the encoder:
1.5e-4).  So gradients are compared at the first draw of DRAWS at which the forward under test takes the reference's masks
(the rule of DESIGN 3.15), under

    G_BOUND = 5e-5      test_wiring_and_oracle's gradient tolerance against the same oracle: 2.8 x the worst honest fp32
                        figure, 3 x below the mildest flip seen.  On the device the node arms reach 1.3e-5 of it and it was
                        not remeasured (the ALL_OFF arm's 2e-2 is the unit-scale input gradient of
                        GRAD_PREPASS = False at this loss's magnitude, not torch's fp32).

loss(preds, ws) = sum_i mean(pred_i * w_i) is linear on purpose (|.| would add kinks of its own); the mean gives the
upstream gradient the 1 / (H W) magnitude of a real loss.

grad_error(got, want): max|got - want| / max|want| per parameter.  The exception is a bias in front of an affine-free
instance norm (every fnet.*.bias except fnet.conv2.bias, and the conv2.0.* block of shared_backbone): its true gradient is
0, what any implementation returns is rounding residue, and it is measured against max|want| of its layer's weight -- the
rule of test_gpu_norm_train.py.

MUTANTS are wrong versions of the step, each with the parameters it must push over G_BOUND; test_host_raft_train_ref.py
shows that the bound catches every one of them.
"""
import contextlib
import functools

import torch
import torch.nn.functional as F

import _encoder_ref as E
from oracle import torch_oracle as to

G_BOUND = 5e-5
DRAWS = range(20)
SHAPE = (1, 32, 64)             # B, H, W of the images
SMALL = (1, 16, 64)             # planes at 1/16 have a single row, the coarsest correlation level is 2 wide
ITERS = 2
#: the configurations of RAFTStereo run under autograd besides the default
VARIANTS = [dict(n_gru_layers=2), dict(slow_fast_gru=True), dict(shared_backbone=True), dict(corr_implementation="reg_cuda")]

#: name -> the parameters on which the mutant must exceed G_BOUND (see mutant handling in train_forward / loss / grads)
MUTANTS = {
    "no_detach": ["update_block.flow_head.conv2.weight", "fnet.conv2.weight"],     # coords1 keeps its history
    "y_not_zeroed": ["update_block.flow_head.conv2.weight"],                       # delta_flow's y row reaches coords1
    "skip_first": ["update_block.mask.2.weight"],                                  # the first prediction is not in the loss
    "gru16_interp_dropped": ["update_block.gru32.convq.weight"],                   # no gradient through interp(net[2]) into gru16
    "wgrad_tap": ["fnet.layer2.0.conv1.weight"],                                   # that layer's weight gradient, tap (0, 0) = 0
    "fmap2_dropped": ["fnet.conv2.weight"],                                        # no gradient into the right feature map
}


def config(overrides=None):
    from dkt_stereo_amd.raft_stereo import BASE_CONFIG
    cfg = dict(BASE_CONFIG)
    cfg.update(overrides or {})
    return cfg


def case_id(overrides):
    return "+".join("%s=%s" % kv for kv in sorted(overrides.items())) or "default"


# -- the forward ---------------------------------------------------------------------------------------------------------------
def _relu(rec, site, x):
    if rec is not None:
        rec.append((site, (x > 0).detach()))
    return F.relu(x)


def _res_block(sd, pre, x, kind, stride, rec):
    """to._res_block with its three ReLUs recorded."""
    y = _relu(rec, pre + ".norm1", to._norm(sd, pre + ".norm1", to._conv(sd, pre + ".conv1", x, stride), kind))
    y = _relu(rec, pre + ".norm2", to._norm(sd, pre + ".norm2", to._conv(sd, pre + ".conv2", y), kind))
    if (pre + ".downsample.0.weight") in sd:
        x = to._norm(sd, pre + ".norm3", to._conv(sd, pre + ".downsample.0", x, stride), kind)
    return _relu(rec, pre + ".join", x + y)


def _layer(sd, pre, x, kind, stride, rec):
    return _res_block(sd, pre + ".1", _res_block(sd, pre + ".0", x, kind, stride, rec), kind, 1, rec)


def _trunk(sd, pre, x, kind, ds, rec):
    x = _relu(rec, pre + ".norm1", to._norm(sd, pre + ".norm1", to._conv(sd, pre + ".conv1", x, 1 + (ds > 2)), kind))
    x = _layer(sd, pre + ".layer1", x, kind, 1, rec)
    x = _layer(sd, pre + ".layer2", x, kind, 1 + (ds > 1), rec)
    return _layer(sd, pre + ".layer3", x, kind, 1 + (ds > 0), rec)


def _heads(sd, pre, x, kind, num_layers, rec):
    """to.multi_heads (two heads per scale)."""
    def block_heads(name, t):
        return [to._conv(sd, "%s.%s.%d.1" % (pre, name, j), _res_block(sd, "%s.%s.%d.0" % (pre, name, j), t, kind, 1, rec))
                for j in range(2)]
    scales = [block_heads("outputs08", x)]
    if num_layers >= 2:
        y = _layer(sd, pre + ".layer4", x, kind, 2, rec)
        scales.append(block_heads("outputs16", y))
    if num_layers >= 3:
        z = _layer(sd, pre + ".layer5", y, kind, 2, rec)
        scales.append([to._conv(sd, "%s.outputs32.%d" % (pre, j), z) for j in range(2)])
    return scales


def encode(sd, cfg, image1, image2, rec=None):
    """E.raft_encode (the default and the shared backbone) without its .float(): [fmap1, fmap2, net_list, inp_list]."""
    image1 = (2 * (image1 / 255.0) - 1.0).contiguous()
    image2 = (2 * (image2 / 255.0) - 1.0).contiguous()
    n, ds, kind, B = cfg["n_gru_layers"], cfg["n_downsample"], cfg["context_norm"], image1.shape[0]
    both = torch.cat([image1, image2], 0)
    if cfg.get("shared_backbone", False):
        v = _trunk(sd, "cnet", both, kind, ds, rec)
        scales = _heads(sd, "cnet", v[:B], kind, n, rec)
        y = to._conv(sd, "conv2.1", _res_block(sd, "conv2.0", v, "instance", 1, rec))
    else:
        scales = _heads(sd, "cnet", _trunk(sd, "cnet", image1, kind, ds, rec), kind, n, rec)
        y = to._conv(sd, "fnet.conv2", _trunk(sd, "fnet", both, "instance", ds, rec))
    fmap1, fmap2 = y.split(B, 0)
    net = [torch.tanh(s[0]) for s in scales]
    inp = [list(to._conv(sd, "context_zqr_convs.%d" % i, _relu(rec, "context_zqr_convs.%d.in" % i, s[1]))
                .split(cfg["hidden_dims"][i], 1)) for i, s in enumerate(scales)]
    return [fmap1, fmap2, net, inp]


def lookup(pyr, coords, radius):
    """to.corr1d_lookup in the dtype of its operands (taps included)."""
    b, _, h, w = coords.shape
    cx = coords[:, :1].permute(0, 2, 3, 1).reshape(b * h * w, 1, 1, 1)
    dx = torch.linspace(-radius, radius, 2 * radius + 1, dtype=coords.dtype).view(2 * radius + 1, 1)
    outs = [to._sample_rows(lvl, dx + cx / 2 ** i).view(b, h, w, -1) for i, lvl in enumerate(pyr)]
    return torch.cat(outs, dim=-1).permute(0, 3, 1, 2).contiguous()


def _motion_encoder(sd, pre, flow, corr, rec):
    """to.motion_encoder, the five ReLUs recorded in the order BasicMultiUpdateBlock._encoder_autograd runs them."""
    cor = _relu(rec, pre + ".convc1", to._conv(sd, pre + ".convc1", corr))
    cor = _relu(rec, pre + ".convc2", to._conv(sd, pre + ".convc2", cor))
    flo = _relu(rec, pre + ".convf1", to._conv(sd, pre + ".convf1", flow))
    flo = _relu(rec, pre + ".convf2", to._conv(sd, pre + ".convf2", flo))
    out = _relu(rec, pre + ".conv", to._conv(sd, pre + ".conv", torch.cat([cor, flo], dim=1)))
    return torch.cat([out, flow], dim=1)


def _update_block(sd, n, net, inp, corr=None, flow=None, fine=True, mid=True, coarse=True, update=True, rec=None, mutant=None):
    """to.update_block(..., igev=False) on a copy of `net`."""
    pre = "update_block"
    net = list(net)
    if coarse:
        net[2] = to.conv_gru(sd, pre + ".gru32", net[2], *inp[2], to.pool2x(net[1]))
    if mid:
        xs = [to.pool2x(net[0])]
        if n > 2:
            up = to.interp(net[2], net[1])
            xs.append(up.detach() if mutant == "gru16_interp_dropped" else up)
        net[1] = to.conv_gru(sd, pre + ".gru16", net[1], *inp[1], *xs)
    if fine:
        xs = [_motion_encoder(sd, pre + ".encoder", flow, corr, rec)] + ([to.interp(net[1], net[0])] if n > 1 else [])
        net[0] = to.conv_gru(sd, pre + ".gru08", net[0], *inp[0], *xs)
    if not update:
        return net
    hidden = _relu(rec, pre + ".flow_head.conv1", to._conv(sd, pre + ".flow_head.conv1", net[0]))
    delta = to._conv(sd, pre + ".flow_head.conv2", hidden)
    mask = .25 * to._conv(sd, pre + ".mask.2", _relu(rec, pre + ".mask.0", to._conv(sd, pre + ".mask.0", net[0])))
    return net, mask, delta


def train_forward(sd, cfg, image1, image2, iters, record=None, mutant=None):
    """The list of all up-sampled predictions of RAFTStereo._forward_train (raft_stereo.py:85-187, test_mode=False) in the
    dtype of `sd`; `record` (a list) receives every ReLU's (site, input > 0)."""
    dtype = next(v for v in sd.values() if v.is_floating_point()).dtype
    n, L, r = cfg["n_gru_layers"], cfg["corr_levels"], cfg["corr_radius"]
    slow_fast = cfg.get("slow_fast_gru", False)
    image1, image2 = image1.to(dtype), image2.to(dtype)
    fmap1, fmap2, net, inp = encode(sd, cfg, image1, image2, record)
    if mutant == "fmap2_dropped":
        fmap2 = fmap2.detach()
    pyr = to.corr1d_pyramid(fmap1, fmap2, L)
    b, _, h, w = net[0].shape
    coords0 = to.coords_grid(b, h, w).to(dtype)
    coords1 = coords0.clone()
    held = [fmap1, fmap2] + list(net) + [t for s in inp for t in s] + list(pyr)
    preds = []
    for _ in range(iters):
        if mutant != "no_detach":
            coords1 = coords1.detach()
        corr = lookup(pyr, coords1, r)
        flow = coords1 - coords0
        if n == 3 and slow_fast:
            net = _update_block(sd, n, net, inp, coarse=True, mid=False, fine=False, update=False, mutant=mutant)
        if n >= 2 and slow_fast:
            net = _update_block(sd, n, net, inp, coarse=(n == 3), mid=True, fine=False, update=False, mutant=mutant)
        net, mask, delta = _update_block(sd, n, net, inp, corr, flow, coarse=(n == 3), mid=(n >= 2), rec=record, mutant=mutant)
        if mutant != "y_not_zeroed":
            delta = torch.cat([delta[:, :1], torch.zeros_like(delta[:, 1:])], dim=1)
        coords1 = coords1 + delta
        preds.append(to.convex_upsample(coords1 - coords0, mask, 2 ** cfg["n_downsample"])[:, :1])
        held += [corr, mask, delta, coords1] + list(net)
    for t in held + preds:
        assert t.dtype == dtype, "an intermediate left %s for %s" % (dtype, t.dtype)
    return preds


# -- loss and gradients --------------------------------------------------------------------------------------------------------
def loss(preds, ws, mutant=None):
    terms = [(p * w.to(p.dtype)).mean() for p, w in zip(preds, ws)]
    return sum(terms[1:] if mutant == "skip_first" else terms)


def loss_weights(seed, iters, B, H, W):
    g = torch.Generator().manual_seed(7000 + seed)
    return [torch.randn((B, 1, H, W), generator=g, dtype=torch.float64) for _ in range(iters)]


def grads(sd, cfg, image1, image2, iters, ws, names, record=None, mutant=None, scale=1.0):
    """({parameter name: gradient or None} of scale * loss for the parameters `names` of the state dict, predictions)."""
    sd = dict(sd)
    for k in names:
        sd[k] = sd[k].detach().clone().requires_grad_(True)
    preds = train_forward(sd, cfg, image1, image2, iters, record, mutant)
    got = torch.autograd.grad(scale * loss(preds, ws, mutant), [sd[k] for k in names], allow_unused=True)
    out = dict(zip(names, got))
    if mutant == "wgrad_tap":
        k = MUTANTS[mutant][0]
        out[k] = out[k].clone()
        out[k][:, :, 0, 0] = 0
    return out, [p.detach() for p in preds]


def zero_gradient_bias(name):
    """A bias in front of an affine-free instance norm: its true gradient is exactly 0."""
    if not name.endswith(".bias"):
        return False
    return (name.startswith("fnet.") and name != "fnet.conv2.bias") or name.startswith("conv2.0.")


def grad_error(got, want):
    """{name: error} of two {name: gradient or None} maps (module docstring); the None patterns must be identical."""
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    none_g, none_w = {k for k, v in got.items() if v is None}, {k for k, v in want.items() if v is None}
    assert none_g == none_w, "parameters without a gradient differ: %s" % sorted(none_g ^ none_w)
    out = {}
    for k, w in want.items():
        if w is None:
            continue
        g = got[k].detach().double().cpu()
        w = w.detach().double().cpu()
        assert tuple(g.shape) == tuple(w.shape), (k, tuple(g.shape), tuple(w.shape))
        ref = want[k[:-4] + "weight"].detach().double().cpu() if zero_gradient_bias(k) else w
        scale = float(ref.abs().max())
        out[k] = float((g - w).abs().max()) / (scale if scale > 0 else 1.0)
    return out


def worst(errs):
    k = max(errs, key=errs.get)
    return k, errs[k]


def flips(rec_a, rec_b):
    """[(site, elements of different sign)] of two records; lengths, shapes and order must agree.  rec_a carries the names
    when rec_b's entries are bare masks."""
    assert len(rec_a) == len(rec_b), "%d ReLU sites against %d" % (len(rec_a), len(rec_b))
    out = []
    for i, (a, b) in enumerate(zip(rec_a, rec_b)):
        site, ma = a
        mb = b[1] if isinstance(b, tuple) else b
        assert tuple(ma.shape) == tuple(mb.shape), "site %d (%s): mask %s against %s" % (i, site, tuple(ma.shape), tuple(mb.shape))
        out.append((site, int((ma.cpu() != mb.cpu()).sum())))
    return out


def flip_line(fl):
    bad = ["%s: %d" % sf for sf in fl if sf[1]]
    return "%d flips at %d sites%s" % (sum(f for _, f in fl), len(fl), (" (" + ", ".join(bad) + ")") if bad else "")


# -- the cases -----------------------------------------------------------------------------------------------------------------
def param_names(model):
    return [n for n, p in model.named_parameters() if p.requires_grad]


@functools.lru_cache(maxsize=None)
def model_and_inputs(case, seed, shape=SHAPE):
    """(model on the CPU in eval(), image1, image2, loss weights) of a draw; `case` = tuple(sorted(overrides.items()))."""
    model = E.make_raft(dict(case), 100 + seed)
    i1, i2 = E.raft_images(seed, *shape)
    return model, i1, i2, loss_weights(seed, ITERS, *shape)


@functools.lru_cache(maxsize=None)
def truth_forward(case, seed, shape=SHAPE):
    """The fp64 forward of a draw, computed once: dict(record, preds)."""
    model, i1, i2, _ = model_and_inputs(case, seed, shape)
    rec = []
    with torch.no_grad():
        preds = train_forward(E.cast_sd(model, torch.float64), config(dict(case)), i1, i2, ITERS, rec)
    return dict(record=rec, preds=preds)


@functools.lru_cache(maxsize=None)
def truth_grads(case, seed, shape=SHAPE):
    """The fp64 parameter gradients of a draw, computed once: {name: gradient or None}."""
    model, i1, i2, ws = model_and_inputs(case, seed, shape)
    return grads(E.cast_sd(model, torch.float64), config(dict(case)), i1, i2, ITERS, ws, param_names(model))[0]


@functools.lru_cache(maxsize=None)
def yardstick(case, seed, shape=SHAPE):
    """The fp32 CPU restatement of the same draw: dict(record, preds, pred_err = its error against the truth per prediction)."""
    model, i1, i2, _ = model_and_inputs(case, seed, shape)
    rec = []
    with torch.no_grad():
        preds = train_forward(E.cast_sd(model, torch.float32), config(dict(case)), i1, i2, ITERS, rec)
    t = truth_forward(case, seed, shape)
    return dict(record=rec, preds=preds, pred_err=[E.rel_err(p, q) for p, q in zip(preds, t["preds"])])


@functools.lru_cache(maxsize=None)
def fp32_grads(case, seed, shape=SHAPE):
    """The fp32 CPU restatement's parameter gradients of a draw."""
    model, i1, i2, ws = model_and_inputs(case, seed, shape)
    return grads(E.cast_sd(model, torch.float32), config(dict(case)), i1, i2, ITERS, ws, param_names(model))[0]


@functools.lru_cache(maxsize=None)
def host_flips(case, seed, shape=SHAPE):
    """[(site, flips)] of the fp32 CPU restatement against the truth."""
    return flips(truth_forward(case, seed, shape)["record"], yardstick(case, seed, shape)["record"])


def total(fl):
    return sum(f for _, f in fl)


# -- the masks of the model itself ---------------------------------------------------------------------------------------------
JOIN_NODE = "_InstanceNormAddReluFnBackward"


class MaskSpy:
    """Every ReLU mask of one RAFTStereo._forward_train call, in the order of train_forward's record."""

    def __init__(self):
        self.enc, self.ctx, self.upd = [], [], []

    def reset(self):
        del self.enc[:], self.ctx[:], self.upd[:]

    def masks(self):
        return list(self.enc) + list(self.ctx) + list(self.upd)


@contextlib.contextmanager
def mask_spy(model, join_inner=None):
    """Wraps extractor.norm_act / add_relu / norm_add_relu (the encoders' norm ReLUs and joins, node or torch), the
    relu=True calls of update.conv2d_autograd (the motion encoder's five and the two heads) and hooks model.cnet for
    relu(x[1]).  `join_inner(c)`: the inner mask relu(norm(c)) > 0 of a fused join node, which never materialises it."""
    from dkt_stereo_amd import extractor, update
    spy = MaskSpy()
    act, add, join, conv = extractor.norm_act, extractor.add_relu, extractor.norm_add_relu, update.conv2d_autograd

    def norm_act(norm, x, relu):
        y = act(norm, x, relu)
        if relu:
            spy.enc.append((y > 0).detach())
        return y

    def add_relu(a, b):
        y = add(a, b)
        spy.enc.append((y > 0).detach())
        return y

    def norm_add_relu(norm, x, c, c_stats=None):
        y = join(norm, x, c, c_stats)
        if type(y.grad_fn).__name__ == JOIN_NODE:       # (the torch form has gone through the two wrappers above)
            spy.enc.append(join_inner(c.detach().contiguous()))
            spy.enc.append((y > 0).detach())
        return y

    def conv2d_autograd(x, layer, relu=False, owner=None):
        y = conv(x, layer, relu=relu, owner=owner)
        if relu:
            spy.upd.append((y > 0).detach())
        return y

    def cnet_hook(module, args, out):
        spy.ctx.extend((s[1] > 0).detach() for s in out if isinstance(s, (list, tuple)))

    handle = model.cnet.register_forward_hook(cnet_hook)
    extractor.norm_act, extractor.add_relu, extractor.norm_add_relu = norm_act, add_relu, norm_add_relu
    update.conv2d_autograd = conv2d_autograd
    try:
        yield spy
    finally:
        extractor.norm_act, extractor.add_relu, extractor.norm_add_relu = act, add, join
        update.conv2d_autograd = conv
        handle.remove()


def model_step(model, i1, i2, ws, spy, scale=1.0):
    """One training step of the model itself: (predictions, {name: gradient or None}, masks)."""
    spy.reset()
    preds = model(i1, i2, iters=ITERS, test_mode=False)["disp_preds"]
    masks = spy.masks()
    names = param_names(model)
    params = dict(model.named_parameters())
    value = scale * loss(preds, [w.to(preds[0].device) for w in ws])
    got = torch.autograd.grad(value, [params[n] for n in names], allow_unused=True)
    return preds, dict(zip(names, got)), masks


def key(overrides):
    return tuple(sorted(overrides.items()))
