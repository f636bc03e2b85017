"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

The fp64 truth of RAFTStereo.iterate() / forward(test_mode=True) across configurations, and the table of cases that sends
every route of the refinement loop through it (test_host_raft_loop_ref.py, test_gpu_raft_loop_configs.py).

iterate_ref() restates oracle/torch_oracle.raft_iterations in the dtype of its operands, from the pieces _raft_train_ref.py
already restates (lookup, _update_block) and the oracle's corr1d_pyramid / coords_grid / convex_upsample -- train_forward
without the detach and with flow_init.  forward_ref() is _raft_train_ref.encode followed by iterate_ref().  In fp32 both
are pinned bit for bit (test_host_raft_loop_ref.py) against to.raft_iterations and train_forward(...)[-1].

The bound of a case, for the up-sampled disparity and for the low-resolution flow alike (absolute, in pixels):

    err = max|got - truth|  <=  MARGIN * max(yardstick, floor)

yardstick   the same restatement in fp32 against fp64 on the same operands (CPU; never the code under test);
floor       FLOOR_ULPS = 1 spacing of fp32 at the largest magnitude of the truth, 2^(floor(log2 max|truth|) - 23): no fp32
            result can be expected to resolve its own largest value more finely (2.4e-7 for the disparities of 2 ... 4 px
            of most cases, 1.5e-5 for the 128 ... 256 px of the flow_init cases);
MARGIN      the largest err / max(yardstick, floor) recorded on the MI355X over all cases and all four tests, times two,
            rounded up to a power of two (the figures: test_gpu_raft_loop_configs.py's docstring and DESIGN.md 4); the IGEV
            cases at the end of this file, whose hidden states and mask features are compared as well, have IGEV_MARGIN by
            the same rule from their own figures.

The `mixed_precision` cases have a yardstick of their own: the restatement in fp64 with the operands of every convolution
(input and weight, not the bias) rounded to fp16 -- what the key means in this library (RAFTStereo._mixed: one fp16 product
per block, fp32 accumulation, fp32 tensors between the layers; the loop's convolutions for the loop alone, the encoders' as
well for the whole forward) -- against the unrounded fp64 truth, MIXED_MARGIN by the same rule from their own recorded
ratios, CAP_MIXED = 1e-1.  It is a yardstick of magnitude, not a bit-level model: the device keeps the fused lookup + convc1
on the exact-fp32 matrix pipe and rounds C8S operands after their power-of-two scales.

A case is valid only while MARGIN * max(yardstick, floor) <= CAP = 1e-3, the project's end-to-end limit
(test_raft_stereo_end_to_end).  MUTANTS are wrong versions of iterate_ref, each with the cases on which it must exceed three
times the bound.

A row of CASES: (name, overrides, (B, H, W) of the images, iterations, expected route).  `overrides` are RAFTStereo config
keys, except the keys of SWITCHES (attributes set on the model) and "flow_init" (True: the case passes flow_init_of()).
The route is what route_of() reports for the first call of the shape on a fresh model, derived by hand from
RAFTStereo._iterate / _iterate_fp / _iterate_graphed, loop_c8._eligible_block, conv_c8.motion_front_supported and
CorrBlock1D.lookup_conv1x1:

    "c8 front t1 p3 captured"      the C8S loop: with ("front") or without ("nofront") the one-launch motion front, the
                                    tier of C8Loop._motion_front that ran (t1 fused lookup + 1x1 straight into C8S -- the
                                    prologue's with the front --, t2 the same fused to fp32 and packed, t3 lookup tensor,
                                    conv2d, pack), the MFMA products per block of the captured units
    "rotated f16x3 captured"       _iterate_rotated; likewise "pipelined" (_one_iteration_pipelined), "plain"
                                    (_one_iteration) and "eager" (the loop of _iterate_fp), with the convolution backend
                                    _iterate_fp ran under
"""
import contextlib
import functools
import math

import torch
import torch.nn.functional as F

import _encoder_ref as E
import _raft_train_ref as R
from oracle import torch_oracle as to

MARGIN = 4.0             # RAFT-Stereo: the largest recorded ratio is 1.94 (l3r2, the loop alone, low-resolution flow)
IGEV_MARGIN = 16.0       # the IGEV loop: 4.61 (igev_c4, the finest hidden state, which the loop keeps as C8S split-fp16 pairs)
MIXED_MARGIN = 2.0       # the mixed_precision cases against their own yardstick (below): 0.85 (both cases)
FLOOR_ULPS = 1.0
CAP = 1e-3
CAP_MIXED = 1e-1         # what the project allows mixed_precision end to end (test_gpu_round6.test_mixed_precision_flag)
MUTANT_FACTOR = 3.0

SWITCHES = ("use_c8", "rotate", "use_hip_graph")

C8_FRONT = "c8 front t1 p3 captured"
C8_T2 = "c8 nofront t2 p3 captured"
C8_T3 = "c8 nofront t3 p3 captured"
PLAIN = "plain f16x3 captured"

#: (name, overrides, (B, H, W), iters, route).  Loop grids: ceil(H / 2^n_downsample), then halved (rounding up) per scale; every
#: case keeps W_loop >> (corr_levels - 1) >= 2 (below that the reference itself divides by W - 1 = 0)
CASES = [
    # the default configuration
    ("default_64x128", {}, (1, 64, 128), 4, C8_FRONT),                                  # 16x32 / 8x16 / 4x8
    ("default_b2_72x136", {}, (2, 72, 136), 7, C8_FRONT),                               # 18x34 / 9x17 / 5x9, 7 units: both parities
    ("default_40x72", {}, (1, 40, 72), 5, C8_FRONT),                                    # 10x18 / 5x9 / 3x5
    ("default_w16", {}, (1, 36, 64), 4, C8_FRONT),                                      # 9x16 / 5x8 / 3x4: the narrowest front
    # the C8S loop without the front, on 9x17 / 5x9 / 3x5
    ("l2r3", dict(corr_levels=2, corr_radius=3), (1, 36, 68), 4, C8_T2),
    ("l3r4", dict(corr_levels=3, corr_radius=4), (1, 36, 68), 5, C8_T2),
    ("l3r2", dict(corr_levels=3, corr_radius=2), (1, 36, 68), 4, C8_T3),
    ("l1r4", dict(corr_levels=1, corr_radius=4), (1, 36, 68), 4, C8_T3),
    # down-sampling (mask heads of 576, 36 and 576 channels)
    ("ds3_72x136", dict(n_downsample=3), (1, 72, 136), 4, C8_FRONT),                    # 9x17 / 5x9 / 3x5
    ("ds1_36x68", dict(n_downsample=1), (1, 36, 68), 4, C8_FRONT),                      # 18x34 / 9x17 / 5x9
    ("ds3_n2_sf_shared", dict(n_downsample=3, n_gru_layers=2, slow_fast_gru=True, shared_backbone=True),
     (1, 136, 264), 4, PLAIN),                                                          # 17x33 / 9x17
    # GRU layers, hidden widths, the context norm
    ("n1_b2", dict(n_gru_layers=1), (2, 36, 68), 4, PLAIN),                             # 9x17
    ("n2", dict(n_gru_layers=2), (1, 36, 68), 4, PLAIN),                                # 9x17 / 5x9
    ("hd96", dict(hidden_dims=[96, 96, 96]), (1, 36, 68), 4, "rotated f16x3 captured"),
    ("hd64_n2", dict(hidden_dims=[64, 64, 64], n_gru_layers=2), (1, 36, 68), 4, PLAIN),
    ("instance", dict(context_norm="instance"), (1, 72, 136), 4, C8_FRONT),             # (>= 32 pixels in the coarsest plane)
    ("sf_n3", dict(slow_fast_gru=True), (1, 40, 72), 4, PLAIN),                         # both slow-fast calls
    # model switches on the default configuration
    ("pipelined", dict(use_c8=False, rotate=False), (1, 40, 72), 5, "pipelined f16x3 captured"),
    ("rotated_128", dict(use_c8=False), (1, 40, 72), 5, "rotated f16x3 captured"),
    ("no_graph", dict(use_hip_graph=False), (1, 40, 72), 4, "eager f16x3 eager"),
    ("iters2", {}, (1, 40, 72), 2, "eager f16x3 eager"),
    ("mixed_c8", dict(mixed_precision=True), (1, 40, 72), 4, "c8 front t1 p1 captured"),
    ("mixed_n2", dict(mixed_precision=True, n_gru_layers=2), (1, 36, 68), 4, "plain f16 captured"),
    # an initial flow
    ("flow_init_default", dict(flow_init=True), (1, 40, 72), 4, C8_FRONT),
    ("flow_init_l3r2", dict(flow_init=True, corr_levels=3, corr_radius=2), (1, 36, 68), 4, C8_T3),
]

NAMES = [c[0] for c in CASES]
BY_NAME = {c[0]: c for c in CASES}

#: mutant -> the cases it must break
MUTANTS = {
    "interp_align_corners": ["default_b2_72x136", "default_40x72", "n2"],
    "pool_count_inside": ["default_64x128", "hd96"],
    "level_not_scaled": ["default_64x128", "l2r3"],
    "taps_reversed": ["default_64x128", "l3r2"],
    "mask_quarter_dropped": ["default_64x128", "ds3_72x136"],
    "factor_dropped": ["default_64x128", "ds1_36x68"],
    "y_kept": ["default_64x128", "n1_b2"],
    "slow_fast_call_dropped": ["ds3_n2_sf_shared", "sf_n3"],
    "flow_init_ignored": ["flow_init_default", "flow_init_l3r2"],
}
#: not expressed: "gru16 fed net[0] un-pooled" -- the concatenation of two planes of different sizes does not exist


def split(overrides):
    """(config overrides, {model attribute: value}, the case passes a flow_init)."""
    cfg = {k: v for k, v in overrides.items() if k not in SWITCHES and k != "flow_init"}
    return cfg, {k: v for k, v in overrides.items() if k in SWITCHES}, bool(overrides.get("flow_init"))


def is_mixed(name):
    return bool(BY_NAME[name][1].get("mixed_precision"))


def loop_grid(overrides, H, W):
    ds = overrides.get("n_downsample", 2)
    for _ in range(ds):
        H, W = (H + 1) // 2, (W + 1) // 2
    return H, W


# -- the restatement -----------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _oracle_with(**fns):
    keep = {k: getattr(to, k) for k in fns}
    for k, v in fns.items():
        setattr(to, k, v)
    try:
        yield
    finally:
        for k, v in keep.items():
            setattr(to, k, v)


def _lookup(pyr, coords, radius, mutant):
    if mutant not in ("level_not_scaled", "taps_reversed"):
        return R.lookup(pyr, coords, radius)
    b, _, h, w = coords.shape
    cx = coords[:, :1].permute(0, 2, 3, 1).reshape(b * h * w, 1, 1, 1)
    dx = torch.linspace(-radius, radius, 2 * radius + 1, dtype=coords.dtype).view(2 * radius + 1, 1)
    if mutant == "taps_reversed":
        dx = dx.flip(0)
    div = (lambda i: 1) if mutant == "level_not_scaled" else (lambda i: 2 ** i)
    outs = [to._sample_rows(lvl, dx + cx / div(i)).view(b, h, w, -1) for i, lvl in enumerate(pyr)]
    return torch.cat(outs, dim=-1).permute(0, 3, 1, 2).contiguous()


def _fp16_conv(sd, name, x, stride=1):
    """to._conv with input and weight rounded to fp16 (kept in their dtype), exact accumulation in that dtype."""
    w = sd[name + ".weight"]
    b = sd.get(name + ".bias")
    return F.conv2d(x.half().to(x.dtype), w.half().to(w.dtype), b, stride=stride, padding=(w.shape[2] // 2, w.shape[3] // 2))


def _conv_oracle(fp16_convs):
    return _oracle_with(_conv=_fp16_conv) if fp16_convs else contextlib.nullcontext()


def _mutant_oracle(mutant):
    if mutant == "interp_align_corners":
        return _oracle_with(interp=lambda x, dest: F.interpolate(x, dest.shape[2:], mode="bilinear", align_corners=False))
    if mutant == "pool_count_inside":
        return _oracle_with(pool2x=lambda x: F.avg_pool2d(x, 3, stride=2, padding=1, count_include_pad=False))
    return contextlib.nullcontext()


def iterate_ref(sd, cfg, fmap1, fmap2, net, inp, iters, flow_init=None, mutant=None, fp16_convs=False):
    """to.raft_iterations (raft_stereo.py:118-183, test_mode) in the dtype of its operands: (flow_lo[:, :1], flow_up).
    fp16_convs: every convolution's input and weight rounded to fp16 (the yardstick of the mixed_precision cases)."""
    assert mutant is None or mutant in MUTANTS, mutant
    dtype = fmap1.dtype
    n, L, r = cfg["n_gru_layers"], cfg["corr_levels"], cfg["corr_radius"]
    slow_fast = cfg.get("slow_fast_gru", False)
    pyr = to.corr1d_pyramid(fmap1, fmap2, L)
    b, _, h, w = net[0].shape
    coords0 = to.coords_grid(b, h, w).to(dtype)
    coords1 = coords0.clone()
    if flow_init is not None and mutant != "flow_init_ignored":
        coords1 = coords1 + flow_init.to(dtype)
    net = list(net)
    mask = None
    with torch.no_grad(), _mutant_oracle(mutant), _conv_oracle(fp16_convs):
        for _ in range(iters):
            corr = _lookup(pyr, coords1, r, mutant)
            flow = coords1 - coords0
            if n == 3 and slow_fast:
                net = R._update_block(sd, n, net, inp, coarse=True, mid=False, fine=False, update=False)
            if n >= 2 and slow_fast and mutant != "slow_fast_call_dropped":
                net = R._update_block(sd, n, net, inp, coarse=(n == 3), mid=True, fine=False, update=False)
            net, mask, delta = R._update_block(sd, n, net, inp, corr, flow, coarse=(n == 3), mid=(n >= 2))
            if mutant != "y_kept":
                delta = torch.cat([delta[:, :1], torch.zeros_like(delta[:, 1:])], dim=1)
            coords1 = coords1 + delta
        flow = coords1 - coords0
        factor = 2 ** cfg["n_downsample"]
        if mutant == "mask_quarter_dropped":
            mask = 4 * mask
        if mutant == "factor_dropped":
            flow_up = to.convex_upsample(flow / factor, mask, factor)[:, :1]
        else:
            flow_up = to.convex_upsample(flow, mask, factor)[:, :1]
    for t in [corr, mask, coords1, flow_up] + net + list(pyr):
        assert t.dtype == dtype, "an intermediate left %s for %s" % (dtype, t.dtype)
    return flow[:, :1], flow_up


def forward_ref(sd, cfg, image1, image2, iters, flow_init=None, mutant=None, fp16_convs=False):
    dtype = next(v for v in sd.values() if v.is_floating_point()).dtype
    with torch.no_grad(), _conv_oracle(fp16_convs):
        fmap1, fmap2, net, inp = R.encode(sd, cfg, image1.to(dtype), image2.to(dtype))
    return iterate_ref(sd, cfg, fmap1, fmap2, net, inp, iters, flow_init, mutant, fp16_convs)


# -- inputs, truths and yardsticks of the cases (computed once) ------------------------------------------------------------------
def seed_of(name):
    return 40 + NAMES.index(name)


def flow_init_of(name):
    """(B, 2, h, w): the x coordinate of every pixel is sent to a position drawn uniformly from -(r + 1) ... w + r, so that
    taps leave the row at both ends; every third one is a whole number; y stays 0."""
    _, overrides, (B, H, W), _, _ = BY_NAME[name]
    if not overrides.get("flow_init"):
        return None
    h, w = loop_grid(overrides, H, W)
    r = overrides.get("corr_radius", 4)
    g = torch.Generator().manual_seed(9000 + seed_of(name))
    target = torch.rand((B, 1, h, w), generator=g, dtype=torch.float64) * (w + 2 * r + 1) - (r + 1)
    whole = (torch.arange(B * h * w).view(B, 1, h, w) % 3) == 0
    target = torch.where(whole, target.round(), target)
    x = torch.arange(w, dtype=torch.float64).view(1, 1, 1, w)
    return torch.cat([target - x, torch.zeros_like(target)], dim=1).float()


@functools.lru_cache(maxsize=None)
def model_of(name):
    """The case's model on the CPU in eval() (switches set) and its config dict."""
    cfg_over, switches, _ = split(BY_NAME[name][1])
    model = E.make_raft(cfg_over, 100 + seed_of(name))
    for k, v in switches.items():
        setattr(model, k, v)
    return model, R.config(cfg_over)


@functools.lru_cache(maxsize=None)
def images_of(name, pair=0):
    """Pair 0 is the case's own; pair 1 a different one of the same shape."""
    return E.raft_images(seed_of(name) + 1000 * pair, *BY_NAME[name][2])


@functools.lru_cache(maxsize=None)
def sd_of(name, dtype):
    return E.cast_sd(model_of(name)[0], dtype)


@functools.lru_cache(maxsize=None)
def operands_of(name):
    """fmap1, fmap2, net, inp of the fp64 encoders on the CPU, rounded to fp32."""
    cfg = model_of(name)[1]
    i1, i2 = images_of(name)
    with torch.no_grad():
        f1, f2, net, inp = R.encode(sd_of(name, torch.float64), cfg, i1.double(), i2.double())
    return f1.float(), f2.float(), [t.float() for t in net], [[t.float() for t in s] for s in inp]


def _cast_ops(ops, dtype):
    f1, f2, net, inp = ops
    return f1.to(dtype), f2.to(dtype), [t.to(dtype) for t in net], [[t.to(dtype) for t in s] for s in inp]


def floor_of(truth):
    """FLOOR_ULPS spacings of fp32 at the largest magnitude of `truth`."""
    m = float(truth.abs().max())
    return FLOOR_ULPS * 2.0 ** (math.floor(math.log2(m)) - 23) if m > 0 else 0.0


def _measure(lo32, up32, lo64, up64, margin=None):
    margin = MARGIN if margin is None else margin
    out = dict(lo=lo64, up=up64, lo32=lo32, up32=up32, margin=margin)
    for k, a, t in (("lo", lo32, lo64), ("up", up32, up64)):
        out[k + "_yard"] = float((a.double() - t).abs().max())
        out[k + "_floor"] = floor_of(t)
        out[k + "_bound"] = margin * max(out[k + "_yard"], out[k + "_floor"])
        out[k + "_unit"] = max(out[k + "_yard"], out[k + "_floor"])
    return out


@functools.lru_cache(maxsize=None)
def loop_truth(name):
    """The loop alone on operands_of(name): dict(lo, up: the fp64 truth; lo32, up32: the fp32 restatement; per output
    *_yard, *_floor, *_unit = max(yard, floor), *_bound = MARGIN * unit)."""
    cfg, iters, fi = model_of(name)[1], BY_NAME[name][3], flow_init_of(name)
    ops = operands_of(name)
    lo32, up32 = iterate_ref(sd_of(name, torch.float32), cfg, *ops, iters, fi)
    lo64, up64 = iterate_ref(sd_of(name, torch.float64), cfg, *_cast_ops(ops, torch.float64), iters, fi)
    return _measure(lo32, up32, lo64, up64)


@functools.lru_cache(maxsize=None)
def forward_truth(name, pair=0):
    """The whole forward on images_of(name, pair): as loop_truth."""
    cfg, iters, fi = model_of(name)[1], BY_NAME[name][3], flow_init_of(name)
    i1, i2 = images_of(name, pair)
    lo32, up32 = forward_ref(sd_of(name, torch.float32), cfg, i1, i2, iters, fi)
    lo64, up64 = forward_ref(sd_of(name, torch.float64), cfg, i1, i2, iters, fi)
    return _measure(lo32, up32, lo64, up64)


@functools.lru_cache(maxsize=None)
def mixed_truth(name, whole, pair=0):
    """A mixed_precision case against its own yardstick (module docstring): as loop_truth (whole = False) / forward_truth
    (True), with lo32 / up32 the fp64 restatement on fp16-rounded convolution operands and MIXED_MARGIN."""
    assert is_mixed(name)
    cfg, iters, fi = model_of(name)[1], BY_NAME[name][3], flow_init_of(name)
    sd = sd_of(name, torch.float64)
    if whole:
        i1, i2 = images_of(name, pair)
        t = forward_truth(name, pair)
        lo, up = forward_ref(sd, cfg, i1, i2, iters, fi, fp16_convs=True)
    else:
        t = loop_truth(name)
        lo, up = iterate_ref(sd, cfg, *_cast_ops(operands_of(name), torch.float64), iters, fi, fp16_convs=True)
    return _measure(lo, up, t["lo"], t["up"], MIXED_MARGIN)


def mutant_error(name, mutant):
    """max|mutant - truth| of the up-sampled disparity, the loop alone in fp64."""
    cfg, iters, fi = model_of(name)[1], BY_NAME[name][3], flow_init_of(name)
    ops = _cast_ops(operands_of(name), torch.float64)
    _, up = iterate_ref(sd_of(name, torch.float64), cfg, *ops, iters, fi, mutant)
    return float((up - loop_truth(name)["up"]).abs().max())


def check(label, got_lo, got_up, t, log=print):
    """A device result against a *_truth dict under the bound; prints err, yardstick, floor and err / max(yardstick, floor)
    per output before asserting; returns the larger ratio."""
    worst, failed = 0.0, []
    for k, g in (("lo", got_lo[:, :1]), ("up", got_up)):
        want = t[k]
        assert tuple(g.shape) == tuple(want.shape), "%s %s: shape %s, expected %s" % (label, k, tuple(g.shape), tuple(want.shape))
        assert g.dtype == torch.float32 and bool(torch.isfinite(g).all()), "%s %s: %s / non-finite" % (label, k, g.dtype)
        err = float((g.detach().cpu().double() - want).abs().max())
        ratio = err / t[k + "_unit"]
        worst = max(worst, ratio)
        log("LOOP %-44s %s err %.3e yardstick %.3e floor %.3e ratio %6.2f" % (label, k, err, t[k + "_yard"], t[k + "_floor"], ratio))
        if not err <= t[k + "_bound"]:
            failed.append("%s %s: err %.3e > %g * max(yardstick %.3e, floor %.3e)" % (label, k, err, t["margin"], t[k + "_yard"], t[k + "_floor"]))
    assert not failed, "; ".join(failed)
    return worst


# -- the route a forward took ----------------------------------------------------------------------------------------------------
_ENTRY_POINTS = ("_iterate_c8", "_iterate_rotated", "_one_iteration_pipelined", "_one_iteration", "_iterate_fp")


@contextlib.contextmanager
def route_log(model):
    """_ffi.launch_log() with the schedules' entry points of `model` marked in it ("py:<method>", and "py:backend=<name>"
    where _iterate_fp starts)."""
    from dkt_stereo_amd import _ffi, conv
    with _ffi.launch_log() as names:
        def wrap(attr):
            fn = getattr(model, attr)

            def marked(*a, **k):
                names.append("py:" + attr)
                if attr == "_iterate_fp":
                    names.append("py:backend=" + conv.get_backend())
                return fn(*a, **k)
            return marked
        for attr in _ENTRY_POINTS:
            setattr(model, attr, wrap(attr))
        try:
            yield names
        finally:
            for attr in _ENTRY_POINTS:
                delattr(model, attr)


def route_of(names, model):
    """The route string (module docstring) of the forward whose route_log() is `names`, on `model` afterwards."""
    names = set(names)
    st = model._graph_state
    backend = next((n.split("=", 1)[1] for n in names if n.startswith("py:backend=")), "?")
    if "py:_iterate_c8" in names:
        lp = st["c8"]
        assert st.get("c8_ran")
        front = "front" if "dkt_motion_front_c8" in names else "nofront"
        looked = {"dkt_corr1d_lookup_skew", "dkt_corr1d_lookup"} & names
        tier = 3 if looked else 2 if "dkt_corr1d_lookup_conv1x1" in names else 1 if "dkt_corr1d_lookup_conv1x1_c8" in names else 0
        graphs = [d for d in (lp.graph, lp.graph_n, lp.graph_last) if d]
        passes = sorted({k[0] for d in graphs for k in d})
        return "c8 %s t%d p%s %s" % (front, tier, "".join(str(p) for p in passes) or "?", "captured" if graphs else "eager")
    if "py:_iterate_rotated" in names:
        kind = "rotated"
    elif "py:_one_iteration_pipelined" in names:
        kind = "pipelined"
    elif "py:_one_iteration" in names:
        kind = "plain"
    else:
        kind = "eager"
    captured = st is not None and st.get("graph") is not None
    return "%s %s %s" % (kind, backend, "captured" if captured else "eager")


#: what "Why this is next" lists -> the predicate a case's (overrides, route) must satisfy for it
ROUTES_REQUIRED = {
    "C8S loop with the one-launch motion front": lambda o, r: r.startswith("c8 front t1 p3"),
    "C8S loop without the front, fused lookup to fp32 and packed": lambda o, r: r.startswith("c8 nofront t2"),
    "C8S loop without the front, lookup tensor + conv2d + pack": lambda o, r: r.startswith("c8 nofront t3"),
    "rotated round-2 pipeline": lambda o, r: r.startswith("rotated"),
    "pipelined, non-rotated schedule": lambda o, r: r.startswith("pipelined"),
    "plain captured iteration without slow-fast": lambda o, r: r == PLAIN and not o.get("slow_fast_gru"),
    "plain captured iteration with one slow-fast call": lambda o, r: r == PLAIN and o.get("slow_fast_gru") and o.get("n_gru_layers") == 2,
    "plain captured iteration with both slow-fast calls": lambda o, r: r == PLAIN and o.get("slow_fast_gru") and o.get("n_gru_layers", 3) == 3,
    "eager loop (no graph)": lambda o, r: r.startswith("eager") and o.get("use_hip_graph") is False,
    "eager loop (iters = 2)": lambda o, r: r.startswith("eager") and "use_hip_graph" not in o,
    "mixed_precision on the C8S loop": lambda o, r: r.startswith("c8") and " p1 " in r and o.get("mixed_precision"),
    "mixed_precision on a round-2 loop (f16 backend)": lambda o, r: " f16 " in r and o.get("mixed_precision"),
    "up-sampling factor 2": lambda o, r: o.get("n_downsample") == 1,
    "up-sampling factor 4": lambda o, r: o.get("n_downsample", 2) == 2,
    "up-sampling factor 8": lambda o, r: o.get("n_downsample") == 3,
    "hidden_dims other than 128 on three layers": lambda o, r: o.get("hidden_dims", [128])[0] != 128 and o.get("n_gru_layers", 3) == 3,
    "n_gru_layers = 1 without slow-fast": lambda o, r: o.get("n_gru_layers") == 1 and not o.get("slow_fast_gru"),
    "n_gru_layers = 2 without slow-fast": lambda o, r: o.get("n_gru_layers") == 2 and not o.get("slow_fast_gru"),
    "flow_init on the front": lambda o, r: o.get("flow_init") and r.startswith("c8 front"),
    "flow_init without the front": lambda o, r: o.get("flow_init") and r.startswith("c8 nofront"),
}


# -- IGEV: the loop alone where the fused geometry lookup does not apply ---------------------------------------------------------
#: (name, config overrides, geometry channels): C8LoopIGEV._motion_front falls through to the lookup tensor, conv2d and a pack
#: for anything but two levels, eight channels and radius 4 (geometry.Combined_Geo_Encoding_Volume.lookup_conv1x1).  Quarter
#: resolution 17 x 27 (then 9 x 14, 5 x 7), D = 12 (12 / 6 / 3 per level), IGEV_ITERS iterations, initial disparities of
#: 0 ... 8: taps leave the D axis and the row at both ends.  The truth is _igev_train_ref.train_forward's loop (its final
#: low-resolution disparity and hidden states; the mask features are the oracle's relu(conv) of the final finest state).  The
#: reference hard-codes 8 + 1 channels per tap in the motion encoder (igev_stereo/update.py:73-78): the C = 4 case gives the
#: block a convc1 of L * K * 5 inputs, which the state-dict restatement takes as it is
IGEV_CASES = [("igev_r3", dict(corr_radius=3), 8), ("igev_l3", dict(corr_levels=3), 8), ("igev_c4", {}, 4)]
IGEV_NAMES = [c[0] for c in IGEV_CASES]
IGEV_GRID, IGEV_D, IGEV_ITERS = (17, 27), 12, 4
IGEV_ROUTE = "c8 geo lookup+conv2d captured"


@functools.lru_cache(maxsize=None)
def igev_case(name):
    """dict(blk: the update block on the CPU, cfg, x: the inputs as _igev_train_ref.inputs names them, sd(dtype))."""
    from types import SimpleNamespace

    import _igev_train_ref as I
    import _synth
    from dkt_stereo_amd.update import BasicMultiUpdateBlockIGEV
    _, overrides, C = IGEV_CASES[IGEV_NAMES.index(name)]
    seed = 60 + IGEV_NAMES.index(name)
    cfg = I.config(tuple(sorted(overrides.items())))
    blk = BasicMultiUpdateBlockIGEV(SimpleNamespace(**cfg), hidden_dims=cfg["hidden_dims"])
    if C != 8:
        blk.encoder.convc1 = torch.nn.Conv2d(cfg["corr_levels"] * (2 * cfg["corr_radius"] + 1) * (C + 1), 64, 1)
    blk.load_state_dict(_synth.torch_state_dict(_synth.shapes_of(blk), 21 + seed))
    blk.eval()
    head = I.make_head(seed)
    g = torch.Generator().manual_seed(8000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    sizes = [IGEV_GRID]
    for _ in range(2):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    h, w = IGEV_GRID
    x = dict(net=[torch.tanh(rn(1, 128, *s)) for s in sizes], inp=[[0.5 * rn(1, 128, *s) for _ in range(3)] for s in sizes],
             m1=rn(1, 16, h, w), m2=rn(1, 16, h, w), geo=rn(1, C, IGEV_D, h, w), disp=8.0 * torch.rand(1, 1, h, w, generator=g),
             coords=torch.arange(w).float().reshape(1, 1, w, 1).repeat(1, h, 1, 1))
    return dict(blk=blk, cfg=cfg, x=x, sd=lambda dtype: I.state_dict(blk, head, dtype))


def _igev_loop(c, dtype):
    import _igev_train_ref as I
    sd = c["sd"](dtype)
    with torch.no_grad():
        _, disps, net = I.train_forward(sd, c["cfg"], c["x"], IGEV_ITERS)
        mask = F.relu(to._conv(sd, "update_block.mask_feat_4.0", net[0]))
    return dict(disp=disps[-1], mask=mask, net0=net[0], net1=net[1], net2=net[2])


@functools.lru_cache(maxsize=None)
def igev_truth(name):
    """{output: dict(truth, yard, floor, unit, bound)} of the loop alone: disp, mask, net0, net1, net2."""
    c = igev_case(name)
    t64, t32 = _igev_loop(c, torch.float64), _igev_loop(c, torch.float32)
    out = {}
    for k, t in t64.items():
        assert bool(torch.isfinite(t).all()) and bool(torch.isfinite(t32[k]).all()), (name, k)
        yard, floor = float((t32[k].double() - t).abs().max()), floor_of(t)
        out[k] = dict(truth=t, yard=yard, floor=floor, unit=max(yard, floor), bound=IGEV_MARGIN * max(yard, floor))
    return out


def igev_check(label, got, truth, log=print):
    """{output: tensor} from the device against igev_truth(); returns the largest err / max(yardstick, floor)."""
    worst, failed = 0.0, []
    for k, t in truth.items():
        g = got[k].detach().cpu()
        assert tuple(g.shape) == tuple(t["truth"].shape) and g.dtype == torch.float32 and bool(torch.isfinite(g).all()), (label, k)
        err = float((g.double() - t["truth"]).abs().max())
        worst = max(worst, err / t["unit"])
        log("LOOP %-44s %-4s err %.3e yardstick %.3e floor %.3e ratio %6.2f" % (label, k, err, t["yard"], t["floor"], err / t["unit"]))
        if not err <= t["bound"]:
            failed.append("%s %s: err %.3e > %g * max(yardstick %.3e, floor %.3e)" % (label, k, err, IGEV_MARGIN, t["yard"], t["floor"]))
    assert not failed, "; ".join(failed)
    return worst
