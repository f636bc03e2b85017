"""Single entry point for every 2-D convolution on the hot path.

``conv2d(x, layer, relu=False)``: ``x`` is a tensor or a LIST of tensors that the
reference would ``torch.cat`` along channels first (core/update.py:24-25,29,83);
``layer`` is anything with ``weight``/``bias``/``padding`` (an ``nn.Conv2d`` or
the merged z|r pair built by ``ConvGRU``).

Backends (``set_backend``; default "f16x3"):
  "f16x3"    dkt_conv2d_f16s_desc, passes=3: fp32 emulated on the fp16 matrix cores
             with split operands (w_hi*x_hi + w_lo*x_hi + w_hi*x_lo, fp32
             accumulate) -- ~22 bits per operand, 1.5e-6 relative to an fp64
             convolution (the vendor fp32 path: 0.9e-6); list inputs are read in
             place.  Meets the 1e-3 final-disparity bound with 25x margin.
  "miopen"   vendor fp32 convolution via torch (concatenates list inputs).
  "f16x2"    passes=2: activations rounded to fp16, weights split.
  "f16"      passes=1: plain fp16 operands, fp32 accumulate.
1x1 / 3x3 layers with padding K/2, stride 1 or 2, groups 1 and dilation 1 run on the kernel; the
7x7 stems on dkt_conv2d_stem7; anything else on the vendor path.

Activation range of the split-fp16 backends.  An activation x is represented as fp16 hi + fp16 lo
of ``x * 2**layer.dkt_in_exp`` (``dkt_in_exp`` = 0 unless set): 22 significant bits for
2^-3 <= |x * 2^e| < 65520, an ABSOLUTE resolution of 2^-25 below that (harmless next to O(1)
activations, a loss of relative precision for tensors that are tiny throughout), and NON-FINITE
results above it -- an out-of-range, Inf or NaN activation is never saturated silently, it shows up
as Inf/NaN in the output (``RAFTStereo.forward`` checks its result).  Layers whose inputs live far
from O(1) get an exponent: by hand (``layer.dkt_in_exp = -4``) or from ``calibrate()``.

Thread safety (the reference drives replicas from one Python thread per GPU, tools/ft_dkt.py:119):
the packed-weight caches are keyed per device and guarded by a lock, the backend can be overridden
per thread (``use_backend``), nothing here mutates shared module state during a forward.
"""
import contextlib
import ctypes
import math
import threading

import torch
import torch.nn.functional as F

from . import _ffi, wcache

import os as _os

_PASSES = {"f16x3": 3, "f16x2": 2, "f16": 1}
_FEW_DIRECT = True
_BACKEND = "f16x3"
_TLS = threading.local()


def _check_backend(name):
    if name != "miopen" and name not in _PASSES:
        raise ValueError("unknown conv backend %r" % (name,))


def set_backend(name):
    """Process-wide default backend (threads may override it with ``use_backend``)."""
    global _BACKEND
    _check_backend(name)
    _BACKEND = name


def get_backend():
    return getattr(_TLS, "backend", None) or _BACKEND


@contextlib.contextmanager
def use_backend(name):
    """Backend override for the calling thread only."""
    _check_backend(name)
    prev = getattr(_TLS, "backend", None)
    _TLS.backend = name
    try:
        yield
    finally:
        _TLS.backend = prev


def in_exp_of(layer):
    return int(getattr(layer, "dkt_in_exp", 0) or 0)


@contextlib.contextmanager
def calibrate(margin_bits=2):
    """Records max|x| of every convolution input inside the ``with`` block (synchronising: run it
    once, on representative inputs, outside any timed region or stream capture) and sets
    ``layer.dkt_in_exp`` so that the largest activation seen lands ``margin_bits`` binades below the
    fp16 limit.  Layers whose inputs are already comfortably inside [2^-3, 2^13] keep exponent 0."""
    rec = {}
    _TLS.calib = rec
    try:
        yield rec
    finally:
        _TLS.calib = None
        for layer, amax in rec.values():
            if not (amax > 0.0) or not math.isfinite(amax):
                continue
            e = (15 - margin_bits) - math.floor(math.log2(amax)) - 1        # amax * 2^e in [2^(14-m), 2^(15-m))
            layer.dkt_in_exp = 0 if (-2 <= e <= 16 - margin_bits) else e


def calibrating():
    """True inside ``with calibrate():`` on this thread (range recording synchronises: no stream capture then)."""
    return getattr(_TLS, "calib", None) is not None


def _vendor(x, layer, relu):
    if isinstance(x, (list, tuple)):
        x = x[0] if len(x) == 1 else torch.cat(list(x), dim=1)
    y = F.conv2d(x, layer.weight, layer.bias, stride=_stride_of(layer), padding=layer.padding,
                 dilation=getattr(layer, "dilation", 1), groups=getattr(layer, "groups", 1))
    return torch.relu_(y) if relu else y


def _record_range(layer, srcs):
    rec = getattr(_TLS, "calib", None)
    if rec is None:
        return
    amax = max(float(s.detach().abs().max()) for s in srcs)
    prev = rec.get(id(layer))
    rec[id(layer)] = (layer, amax if prev is None else max(amax, prev[1]))


class _Packed:
    __slots__ = ("key", "src_channels", "hi", "lo", "inv_scale", "bias")


def pack_scale(wmax):
    """The power-of-two weight scale of a cold pack: max|w| lands in [2^12, 2^13), which keeps w_lo out of the fp16
    subnormals."""
    return 2.0 ** (12 - math.floor(math.log2(wmax))) if wmax > 0 else 1.0


def _copy_unaliased(dst, src):
    """dst <- src unless dst IS src's memory (a cached fp32 contiguous copy is often the parameter itself: writing it would
    bump the parameter's version counter)."""
    if dst.data_ptr() != src.data_ptr():
        dst.copy_(src.detach())


def _new_packed(key, w, b, elems):
    p = _Packed()
    p.key = key
    p.hi = torch.empty(elems, device=w.device, dtype=torch.float16)
    p.lo = torch.empty(elems, device=w.device, dtype=torch.float16)
    p.bias = None if b is None else b.detach().float().contiguous()
    return p


def _write_packed(p, layer, scale):
    """The split-fp16 image of `layer`'s weight at `scale` into p's buffers, the bias into p.bias."""
    w = layer.weight
    n = len(p.src_channels)
    ch = (ctypes.c_int * n)(*p.src_channels)
    cout, _, kh, kw = w.shape
    wc = w.detach().float().contiguous()
    _ffi.call("dkt_conv2d_pack_weights", w, wc.data_ptr(), ch, n, cout, kh, kw, scale, p.hi.data_ptr(), p.lo.data_ptr())
    p.inv_scale = 1.0 / scale
    if p.bias is not None:
        _copy_unaliased(p.bias, layer.bias)


def _packed_weights(layer, src_channels, scale=None):
    """Split-fp16 weight image for dkt_conv2d_f16s_desc, cached on the layer per device and operand split and rebuilt when the
    parameter tensor is replaced or written.  `scale`: the power-of-two weight scale when the caller already knows it (a
    rearrangement of a packed weight), else it is read from max|w| (a host sync)."""
    w = layer.weight
    src_channels = tuple(src_channels)
    key = wcache.key_of(w, layer.bias, extra=src_channels)
    slot = (str(w.device), src_channels)
    with wcache.LOCK:
        hit = wcache.lookup(layer, "_dkt_packed", slot, key)
        if hit is not None:
            return hit
        cout, cin, kh, kw = w.shape
        if cin != sum(src_channels):
            raise ValueError("conv operands carry %d channels, layer expects %d" % (sum(src_channels), cin))
        n = len(src_channels)
        elems = _ffi.size("dkt_conv2d_packed_elems", (ctypes.c_int * n)(*src_channels), n, cout, kh, kw)
        if elems == 0:
            raise _ffi.DktError("dkt_conv2d_packed_elems rejected the layer shape")
        if scale is None:
            scale = pack_scale(float(w.detach().abs().max()))
        p = _new_packed(key, w, layer.bias, elems)
        p.src_channels = src_channels
        _write_packed(p, layer, scale)
        return wcache.store(layer, "_dkt_packed", slot, p)


def _refresh_packed(layer, cache, R):
    """ema.ema_update_: rewrite the current split-fp16 images of `layer` in place, same buffers and scales."""
    for p, drop in R.each(cache):
        R.window(R.amax(layer.weight), p.inv_scale, drop)
        _write_packed(p, layer, 1.0 / p.inv_scale)
        p.key = R.rekey(p.key)


wcache.register("_dkt_packed", _refresh_packed)


def _write_stem7(pk, layer, scale):
    """The 7x7 stem image of `layer`'s weight at `scale` into pk's buffers, the bias into pk.bias."""
    w = layer.weight
    wc = w.detach().float().contiguous()
    _ffi.call("dkt_conv2d_stem7_pack", w, wc.data_ptr(), w.shape[0], w.shape[1], scale, pk.hi.data_ptr(), pk.lo.data_ptr())
    pk.inv_scale = 1.0 / scale
    if pk.bias is not None:
        _copy_unaliased(pk.bias, layer.bias)


def stem7_packed(layer):
    """Split-fp16 image of a 7x7 stem for dkt_conv2d_stem7 and its C8S variants, cached on the layer per device."""
    w = layer.weight
    key = wcache.key_of(w, layer.bias)
    slot = str(w.device)
    with wcache.LOCK:
        pk = wcache.lookup(layer, "_dkt_stem7", slot, key)
        if pk is None:
            scale = pack_scale(float(w.detach().abs().max()))
            pk = _new_packed(key, w, layer.bias, _ffi.size("dkt_conv2d_stem7_packed_elems", w.shape[0]))
            _write_stem7(pk, layer, scale)
            wcache.store(layer, "_dkt_stem7", slot, pk)
    return pk


def _refresh_stem7(layer, cache, R):
    """ema.ema_update_: the 7x7 stem images of `layer` in place (see stem7_packed)."""
    for pk, drop in R.each(cache):
        R.window(R.amax(layer.weight), pk.inv_scale, drop)
        _write_stem7(pk, layer, 1.0 / pk.inv_scale)
        pk.key = R.rekey(pk.key)


wcache.register("_dkt_stem7", _refresh_stem7)


def clear_weight_cache(module):
    """Drops every cached weight derivative below `module` -- packed images of every kind, folded and merged layers, views,
    copied weights, all that wcache's registry lists -- (needed only after writes that bypass the Parameter's version
    counter, e.g. ``weight.data.mul_()``).  It used to leave the C8S step and ConvGRU images, the head weights, the merged
    heads, the scaled layers and the encoder's C8S buffers in place, so the refinement loop kept running stale images."""
    wcache.clear(module)


def _dense(t):
    hw = t.shape[2] * t.shape[3]
    return t.stride(3) == 1 and t.stride(2) == t.shape[3] and t.stride(1) == hw


def _stride_of(layer):
    st = getattr(layer, "stride", 1)
    st = (st, st) if isinstance(st, int) else tuple(st)
    return st


def _padding_of(layer):
    pad = layer.padding
    return (pad, pad) if isinstance(pad, int) else tuple(pad)


def _plain_conv(layer):
    """groups == 1, dilation == 1, zero padding (what the kernels implement)."""
    dil = getattr(layer, "dilation", 1)
    dil = (dil, dil) if isinstance(dil, int) else tuple(dil)
    return (getattr(layer, "groups", 1) == 1 and dil == (1, 1)
            and getattr(layer, "padding_mode", "zeros") == "zeros")


def hip_eligible(layer):
    """True when `layer` runs on dkt_conv2d_f16s_desc under the current backend:
    1x1 / 3x3, padding K/2, stride 1 or 2, no groups / dilation."""
    kh, kw = layer.weight.shape[2:]
    pad = _padding_of(layer)
    return (get_backend() in _PASSES and kh == kw and kh in (1, 3) and pad == (kh // 2, kw // 2)
            and _stride_of(layer) in ((1, 1), (2, 2)) and _plain_conv(layer))


def direct_eligible(layer):
    """The 7x7 stems (Cin <= 4, stride 1) run on dkt_conv2d_stem7 (matrix cores, K laid out over the
    taps).  The exact-fp32 direct kernel (dkt_conv2d_direct, 26 us for 2->64 @184x312) stays available
    as _conv2d_direct."""
    if get_backend() not in _PASSES or not _plain_conv(layer):
        return False
    cout, cin, kh, kw = layer.weight.shape
    pad = _padding_of(layer)
    if kh != kw or pad != (kh // 2, kw // 2) or _stride_of(layer) != (1, 1):
        return False
    return kh == 7 and cin <= 4


def few_eligible(layer):
    """3x3, stride 1, padding 1, at most 4 output channels (flow_head.conv2 256 -> 2, disp_head.conv2 256 -> 1):
    an HBM-bound layer that runs on the exact-fp32 DMA-staged kernel (dkt_conv2d_direct) instead of padding its
    outputs to a 32-channel matrix-core tile.  (`_FEW_DIRECT = False` sends it back to dkt_conv2d_f16s_desc.)"""
    if get_backend() not in _PASSES or not _plain_conv(layer) or not _FEW_DIRECT:
        return False
    cout, cin, kh, kw = layer.weight.shape
    pad = _padding_of(layer)
    if not (kh == 3 and kw == 3 and pad == (1, 1) and _stride_of(layer) == (1, 1) and cout <= 4):
        return False
    # what launch_few (conv_direct.hip) can stage in 160 KB of LDS: 110592 B of patches + 384 B per (8-channel slice, output);
    # wider layers (Cin > 1104 / 552 / 272 for 1 / 2 / 3-4 outputs) stay on dkt_conv2d_f16s_desc
    to = 1 if cout <= 1 else 2 if cout <= 2 else 4
    return 110592 + 384 * ((cin + 7) // 8) * to <= 160 * 1024


def _conv2d_direct(x, layer, relu, out):
    _ffi.require_gpu(x)
    _ffi.require_no_grad(x)
    if not _dense(x):
        x = x.contiguous()
    B, cin, H, W = x.shape
    cout, _, kh, kw = layer.weight.shape
    if out is None:
        out = torch.empty((B, cout, H, W), device=x.device, dtype=torch.float32)
    w = layer.weight.detach()
    w = w if w.is_contiguous() else w.contiguous()
    b = layer.bias
    _ffi.call("dkt_conv2d_direct", x, x.data_ptr(), x.stride(0), w.data_ptr(), None if b is None else b.data_ptr(),
              out.data_ptr(), out.stride(0), B, cin, cout, H, W, kh, kw, int(bool(relu)))
    return out


def conv2d_accumulate(x, layer, out, diff=None):
    """out += conv(x) + bias for a few-output 3x3 layer (``few_eligible``): the head layer of the refinement loop adds its
    result to the running coordinates / disparity in its epilogue (one elementwise launch less per iteration).
    `out`: (B, Cout, H, W) view, dense per batch element."""
    _ffi.require_gpu(x, out)
    _ffi.require_no_grad(x)
    if not _dense(x):
        x = x.contiguous()
    B, cin, H, W = x.shape
    cout, _, kh, kw = layer.weight.shape
    if not _dense(out) or out.dtype != torch.float32 or tuple(out.shape) != (B, cout, H, W):
        raise ValueError("conv2d_accumulate(out=...) must be a dense-per-batch fp32 tensor of the result shape")
    w = layer.weight.detach()
    w = w if w.is_contiguous() else w.contiguous()
    b = layer.bias
    if diff is not None:
        # diff = (ref, dst): dst = out_new - ref, both shaped like `out` (dense per batch element)
        ref, dst = diff
        for t in (ref, dst):
            if not _dense(t) or t.dtype != torch.float32 or tuple(t.shape) != (B, cout, H, W):
                raise ValueError("conv2d_accumulate(diff=(ref, dst)): both must be dense-per-batch fp32 tensors shaped like out")
        _ffi.call(
            "dkt_conv2d_direct_accumulate_diff", x,
            x.data_ptr(), x.stride(0), w.data_ptr(), None if b is None else b.data_ptr(), out.data_ptr(), out.stride(0),
            ref.data_ptr(), ref.stride(0), dst.data_ptr(), dst.stride(0), B, cin, cout, H, W, kh, kw)
        return out
    _ffi.call("dkt_conv2d_direct_accumulate", x, x.data_ptr(), x.stride(0), w.data_ptr(), None if b is None else b.data_ptr(),
              out.data_ptr(), out.stride(0), B, cin, cout, H, W, kh, kw)
    return out


def _conv2d_stem7(x, layer, relu, out):
    """7x7 stem (Cin <= 4) on the matrix cores (dkt_conv2d_stem7); packed weights cached on the layer."""
    _ffi.require_gpu(x)
    _ffi.require_no_grad(x)
    if not _dense(x):
        x = x.contiguous()
    B, cin, H, W = x.shape
    cout = layer.weight.shape[0]
    _record_range(layer, [x])
    pk = stem7_packed(layer)
    in_scale = 2.0 ** in_exp_of(layer)
    if out is None:
        out = torch.empty((B, cout, H, W), device=x.device, dtype=torch.float32)
    _ffi.call("dkt_conv2d_stem7", x, x.data_ptr(), x.stride(0), pk.hi.data_ptr(), pk.lo.data_ptr(),
              None if pk.bias is None else pk.bias.data_ptr(), pk.inv_scale / in_scale, in_scale,
              out.data_ptr(), out.stride(0), B, cin, cout, H, W, int(bool(relu)))
    return out


class _Operands:
    """The cat operands of one convolution and its packed weights (keeps them alive)."""

    def __init__(self, x, layer, pack_scale=None):
        srcs = list(x) if isinstance(x, (list, tuple)) else [x]
        if len(srcs) > 4:
            srcs = srcs[:3] + [torch.cat(srcs[3:], dim=1)]
        _ffi.require_gpu(*srcs)
        _ffi.require_no_grad(*srcs)
        self.srcs = srcs = [s if _dense(s) else s.contiguous() for s in srcs]
        _record_range(layer, srcs)
        self.B, _, self.H, self.W = srcs[0].shape
        self.n = len(srcs)
        self.pk = _packed_weights(layer, [int(s.shape[1]) for s in srcs], pack_scale)
        self.kh, self.kw = layer.weight.shape[2:]
        self.cout = layer.weight.shape[0]
        self.bias = None if self.pk.bias is None else self.pk.bias.data_ptr()
        self.device = srcs[0].device
        self.in_scale = 2.0 ** in_exp_of(layer)
        self.passes = _PASSES[get_backend()]


def _desc(op, out, relu=False, epilogue=0, e0=None, e1=None, h=None, out2=None, stride=0):
    """dkt_conv_desc of one convolution, the one marshaller of every dkt_conv2d_f16s_desc / _pair launch (keeps `op` and the
    tensors alive through the returned object; `passes` rides along for _launch).  Field by field: one constructor call with
    every field as a keyword measured 0.6 .. 1.5 us per call slower (profiles/conv2d_one_entry.txt)."""
    d = _ffi.ConvDesc()
    for i in range(op.n):
        d.src[i] = op.srcs[i].data_ptr()
        d.src_bstride[i] = op.srcs[i].stride(0)
        d.src_channels[i] = int(op.srcs[i].shape[1])
    d.nsrc = op.n
    d.w_hi, d.w_lo = op.pk.hi.data_ptr(), op.pk.lo.data_ptr()
    d.bias = op.bias
    d.out_scale, d.in_scale = op.pk.inv_scale / op.in_scale, op.in_scale
    d.out, d.out_bstride = out.data_ptr(), out.stride(0)
    d.B, d.H, d.W, d.Cout, d.KH, d.KW, d.relu = op.B, op.H, op.W, op.cout, op.kh, op.kw, int(bool(relu))
    d.epilogue, d.stride = epilogue, stride
    if e0 is not None:
        d.e0, d.e0_bstride = e0.data_ptr(), e0.stride(0)
    if e1 is not None:
        d.e1, d.e1_bstride = e1.data_ptr(), e1.stride(0)
    if h is not None:
        d.h, d.h_bstride = h.data_ptr(), h.stride(0)
    if out2 is not None:
        d.out2, d.out2_bstride = out2.data_ptr(), out2.stride(0)
    d.passes = op.passes
    d._keep = (op, out, e0, e1, h, out2)
    return d


def _launch(descs, passes, ref):
    """One descriptor goes to dkt_conv2d_f16s_desc, two go to dkt_conv2d_f16s_pair, on `ref`'s device and current stream."""
    name = "dkt_conv2d_f16s_desc" if len(descs) == 1 else "dkt_conv2d_f16s_pair"
    _ffi.call(name, ref, *[ctypes.byref(d) for d in descs], passes)


# One job builder per operation: each returns (descriptor, result) and serves the single call and its *_pair twin.
def _plain_job(x, layer, relu=False, out=None):
    """[relu](conv(x) + bias) at the layer's stride, into `out` when given."""
    op = _Operands(x, layer)
    stride = _stride_of(layer)[0]
    shape = (op.B, op.cout, (op.H - 1) // stride + 1, (op.W - 1) // stride + 1)
    if out is None:
        out = torch.empty(shape, device=op.device, dtype=torch.float32)
    elif not _dense(out) or out.dtype != torch.float32 or tuple(out.shape) != shape:
        raise ValueError("conv2d(out=...) must be a dense-per-batch fp32 tensor of the result shape")
    return _desc(op, out, relu=relu, stride=stride), out


def _set_in_norm(d, in_norm):
    """The (mean, 1/std) planes of conv2d_fused / conv2d_stats into a stride-1 descriptor."""
    op = d._keep[0]
    if d.stride == 2 or op.n != 1 or in_norm.dtype != torch.float32 or in_norm.numel() != 2 * op.B * int(op.srcs[0].shape[1]):
        raise ValueError("in_norm must hold (mean, 1/std) for every (batch, channel) plane of one stride-1 operand")
    in_norm = in_norm.contiguous()
    d.in_norm = in_norm.data_ptr()
    d._keep = d._keep + (in_norm,)


def _fused_job(x, layer, relu=False, residual=None, in_norm=None):
    """conv2d_fused: a stride-1 layer with the residual join in its epilogue and / or the input's instance norm."""
    op = _Operands(x, layer)
    out = torch.empty((op.B, op.cout, op.H, op.W), device=op.device, dtype=torch.float32)
    if residual is not None:
        if tuple(residual.shape) != tuple(out.shape):
            raise ValueError("conv2d_fused: residual shape %s != result shape %s" % (tuple(residual.shape), tuple(out.shape)))
        residual = residual if _dense(residual) else residual.contiguous()
        _ffi.require_gpu(residual)
        _ffi.require_no_grad(residual)
    d = _desc(op, out, relu=relu, epilogue=3 if residual is not None else 0, e0=residual)
    if in_norm is not None:
        _set_in_norm(d, in_norm)
    return d, out


def _gate_zr_job(x, zr_layer, cz, cr, h):
    op = _Operands(x, zr_layer)
    z = torch.empty((op.B, op.cout // 2, op.H, op.W), device=op.device, dtype=torch.float32)
    rh = torch.empty_like(z)
    return _desc(op, z, epilogue=1, e0=cz, e1=cr, h=h, out2=rh), (z, rh)


def _gate_out_job(x, q_layer, cq, z, h, out=None):
    op = _Operands(x, q_layer)
    if out is None:
        out = torch.empty((op.B, op.cout, op.H, op.W), device=op.device, dtype=torch.float32)
    return _desc(op, out, epilogue=2, e0=cq, e1=z, h=h), out


def fused_eligible(layer, in_norm=False):
    """`layer` can take a residual operand (epilogue 3) and, with in_norm, the instance norm of its input in the
    staging (dkt_conv2d_f16s_desc): stride 1, 1x1 / 3x3 on the split-fp16 kernel; in_norm: 3x3, 33..128 outputs."""
    if not hip_eligible(layer) or _stride_of(layer) != (1, 1):
        return False
    cout, _, kh, _ = layer.weight.shape
    return (kh == 3 and 32 < cout <= 128) if in_norm else True


def conv2d_fused(x, layer, relu=False, residual=None, in_norm=None):
    """One stride-1 convolution with the neighbouring streaming passes folded in (core/extractor.py:46-60):
      in_norm : (B*Cin, 2) float (mean, 1/std) per input plane -> the layer reads relu((x - mean) * invstd);
      residual: tensor shaped like the result -> relu(residual + [relu](conv(x) + bias)).
    Bit-identical to the separate passes (same arithmetic, same order)."""
    d, out = _fused_job(x, layer, relu, residual, in_norm)
    _launch([d], d.passes, out)
    return out


class OutStats:
    """Instance-norm statistics of a convolution's output, accumulated in its epilogue: `part` is the partial-sum workspace
    the dkt_instance_norm_* kernels read (what dkt_instance_norm_stats would have written in a pass of its own)."""
    __slots__ = ("part", "planes", "hw")

    def __init__(self, part, planes, hw):
        self.part, self.planes, self.hw = part, planes, hw


def stats_eligible(layer):
    """`layer` can accumulate its output's instance-norm statistics in the epilogue (dkt_conv_desc.stats_ws): the split-fp16
    kernel's plain epilogue, stride 1 or 2."""
    return hip_eligible(layer) and _stride_of(layer) in ((1, 1), (2, 2)) and not direct_eligible(layer) and not few_eligible(layer)


def conv2d_stats(x, layer, in_norm=None, _ws=None, relu=False):
    """conv(x) + bias [ReLU] with the statistics of its OWN output for the InstanceNorm2d that follows it
    (core/extractor.py:46-50): returns (out, OutStats).  `in_norm` as in conv2d_fused (stride 1 only).
    `_ws`: the per-(tile, wave row) scratch of dkt_conv2d_stats_ws_floats floats, handed in by the guarded-buffer test."""
    d, out = _plain_job(x, layer, relu)
    B, cout, Ho, Wo = out.shape
    n_ws = _ffi.size("dkt_conv2d_stats_ws_floats", B, cout, Ho, Wo)
    ws = torch.empty(n_ws, device=out.device, dtype=torch.float32) if _ws is None else _ws
    if ws.numel() < n_ws or ws.dtype != torch.float32 or not ws.is_contiguous():
        raise ValueError("conv2d_stats: scratch of dkt_conv2d_stats_ws_floats floats expected")
    part = torch.empty(_ffi.size("dkt_instance_norm_workspace", B * cout, Ho * Wo), device=out.device, dtype=torch.uint8)
    d.stats_ws, d.stats_part = ws.data_ptr(), part.data_ptr()
    d._keep = d._keep + (ws, part)
    if in_norm is not None:
        _set_in_norm(d, in_norm)
    _launch([d], d.passes, out)
    return out, OutStats(part, B * cout, Ho * Wo)


def pair_eligible(layer_a, layer_b):
    """Two stride-1 layers can share a launch (dkt_conv2d_f16s_pair): same filter size, same output-width class."""
    def cls(c):
        return 0 if c <= 32 else 1 if c <= 64 else 2 if c <= 128 else 3
    wa, wb = layer_a.weight, layer_b.weight
    return (hip_eligible(layer_a) and hip_eligible(layer_b) and _stride_of(layer_a) == (1, 1) == _stride_of(layer_b)
            and wa.shape[2] == wb.shape[2] and cls(wa.shape[0]) == cls(wb.shape[0]))


def conv2d_pair(a, b):
    """Two independent stride-1 convolutions (bias + optional ReLU) in one launch.  a, b = (x, layer, relu);
    the layers must satisfy ``pair_eligible``.  Returns (y_a, y_b)."""
    (da, ya), (db, yb) = _plain_job(*a), _plain_job(*b)
    _launch([da, db], db.passes, ya)
    return [ya, yb]


def conv2d_fused_pair(a, b):
    """conv2d_fused (residual epilogue) for two independent layers in one launch.  a, b = (x, layer, relu, residual);
    the layers must satisfy ``pair_eligible`` and ``fused_eligible``.  Returns (y_a, y_b)."""
    (da, ya), (db, yb) = _fused_job(*a), _fused_job(*b)
    _launch([da, db], db.passes, ya)
    return [ya, yb]


def conv2d_gate_zr_pair(a, b):
    """conv2d_gate_zr for two independent GRUs in one launch.  a, b = (x, zr_layer, cz, cr, h);
    returns ((z_a, rh_a), (z_b, rh_b))."""
    (da, ya), (db, yb) = _gate_zr_job(*a), _gate_zr_job(*b)
    _launch([da, db], db.passes, ya[0])
    return [ya, yb]


def conv2d_gate_out_pair(a, b):
    """conv2d_gate_out for two independent GRUs in one launch.  a, b = (x, q_layer, cq, z, h, out)."""
    (da, ya), (db, yb) = _gate_out_job(*a), _gate_out_job(*b)
    _launch([da, db], db.passes, ya)
    return [ya, yb]


def conv2d(x, layer, relu=False, out=None):
    """`out`: optional (B,Cout,H,W) fp32 destination whose batch elements are dense (e.g. a
    channel slice of a wider buffer -- replaces a torch.cat of the result)."""
    if isinstance(x, (list, tuple)) and len(x) == 1:
        x = x[0]
    if direct_eligible(layer) and not isinstance(x, (list, tuple)):
        return _conv2d_stem7(x, layer, relu, out)
    if few_eligible(layer) and not isinstance(x, (list, tuple)):
        return _conv2d_direct(x, layer, relu, out)
    if not hip_eligible(layer):
        y = _vendor(x, layer, relu)
        if out is not None:
            out.copy_(y)
            return out
        return y
    d, out = _plain_job(x, layer, relu, out)
    _launch([d], d.passes, out)
    return out


def conv2d_gate_zr(x, zr_layer, cz, cr, h):
    """ConvGRU first stage with the gates in the convolution epilogue:
    returns (z, r*h) = (sigmoid(convz(x)+cz), sigmoid(convr(x)+cr)*h); `zr_layer` is the
    merged convz|convr pair.  cz, cr, h: (B,Ch,H,W), dense per batch element."""
    d, (z, rh) = _gate_zr_job(x, zr_layer, cz, cr, h)
    _launch([d], d.passes, z)
    return z, rh


def conv2d_gate_out(x, q_layer, cq, z, h, out=None):
    """ConvGRU second stage: (1-z)*h + z*tanh(convq(x)+cq), written to `out` (default: new
    tensor; `out` may be `h` itself for an in-place state update)."""
    d, out = _gate_out_job(x, q_layer, cq, z, h, out)
    _launch([d], d.passes, out)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Autograd of the stride-1 "same" convolution (training through the update operator, tools/ft_dkt.py:223-242): forward and
# the input gradient run on this library's convolution kernels (the input gradient of a stride-1 same convolution is the
# same convolution with the weights transposed over (Cout, Cin) and rotated by 180 degrees), the weight gradient -- a
# reduction over all pixels, a different loop nest -- on dkt_conv2d_wgrad for 1x1 and 3x3 layers (GRAD_WEIGHT_HIP) and on the
# vendor library (torch.nn.grad.conv2d_weight) for 7x7 ones (on dkt_conv2d_wgrad7 with GRAD_WEIGHT7_HIP, for the stem layers'
# 1..4 input channels), the bias gradient is a sum.
#
# Backward with GRAD_PREPASS (default): one streaming pre-pass (dkt_conv_grad_prepass) masks the upstream gradient with the
# saved ReLU output, sums the bias gradient in a fixed order and leaves the RANGE of the masked gradient in device memory;
# the input-gradient convolution (dkt_conv_desc.dscale) takes its activation scale from there, so a gradient of any
# magnitude -- 1e-6 from a mean-reduced loss, 1e+6 under a loss scale -- keeps the ~22 bits of the split instead of the
# format's absolute 2^-25 floor, and a power-of-two multiple of the upstream gradient gives that multiple of gx and gb bit
# for bit.  The host reads nothing back.  The packed images of both orientations live on a persistent OWNER (the nn.Module,
# or ConvGRU._merged_zr() for z|r), keyed on the weight's wcache.Key: packed once per optimizer step, not per call.
# ---------------------------------------------------------------------------------------------------------------------
#: backward of conv2d_autograd: True = pre-pass + device-scaled input gradient + owner-held packs; False = the sequence
#: before them (the A/B handle of tools/bench_gru_train.py, in the style of BasicMultiUpdateBlock.TRAIN_NODES)
GRAD_PREPASS = True


class _LayerShim:
    """Duck-types the `layer` argument of conv2d() for detached tensors inside the autograd function."""

    def __init__(self, weight, bias, padding, stride=(1, 1)):
        self.weight, self.bias, self.padding = weight, bias, padding
        self.stride, self.dilation, self.groups, self.padding_mode = stride, (1, 1), 1, "zeros"


class _Conv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        kh, kw = weight.shape[2:]
        pad = (kh // 2, kw // 2)
        with torch.no_grad():
            y = conv2d(x.detach(), _LayerShim(weight.detach(), None if bias is None else bias.detach(), pad), relu=relu)
        ctx.relu, ctx.pad, ctx.has_bias = bool(relu), pad, bias is not None
        ctx.save_for_backward(x, weight, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, y = ctx.saved_tensors
        gy = gy.contiguous().float()
        if ctx.relu:
            gy = gy * (y > 0)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            with torch.no_grad():
                wt = weight.detach().transpose(0, 1).flip(2, 3).contiguous()
                gx = conv2d(gy, _LayerShim(wt, None, ctx.pad))
        if ctx.needs_input_grad[1]:
            gw = torch.nn.grad.conv2d_weight(x.detach(), weight.shape, gy, stride=1, padding=ctx.pad)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = gy.sum(dim=(0, 2, 3))
        return gx, gw, gb, None


def _forward_pack_scale(owner, key):
    """The scale of `owner`'s current forward image (None when its forward runs on a kernel without one)."""
    scale = None
    for lst in owner.__dict__.get("_dkt_packed", {}).values():
        for p in lst:
            if p.key.tensors[0] == key.tensors[0]:
                scale = 1.0 / p.inv_scale
    return scale


def _grad_weight(w, out=None):
    """`w` transposed over (Cout, Cin) and rotated by 180 degrees, fp32 and dense (into `out` when given)."""
    wt = w.detach().float().transpose(0, 1).flip(2, 3)
    return wt.contiguous() if out is None else out.copy_(wt)


def _grad_layer(owner):
    """The layer of the input gradient -- `owner`'s weight transposed over (Cout, Cin) and rotated by 180 degrees -- as a
    persistent object on `owner`, per device, keyed on the weight's wcache.Key; its own packed image hangs off it
    (_packed_weights) and takes the scale of the forward image (the same max|w|: no host read)."""
    w = owner.weight
    key = wcache.key_of(w)
    slot = str(w.device)
    with wcache.LOCK:
        hit = wcache.lookup(owner, "_dkt_grad", slot, key)
        if hit is not None:
            hit.value.pack_scale = _forward_pack_scale(owner, key)
            return hit.value
        kh, kw = w.shape[2:]
        with torch.no_grad():
            shim = _LayerShim(_grad_weight(w), None, (kh // 2, kw // 2))
        shim.pack_scale = _forward_pack_scale(owner, key)
        wcache.store(owner, "_dkt_grad", slot, wcache.Entry(key, shim))
        return shim


def _refresh_grad(owner, cache, R):
    """ema.refresh_written: the input-gradient layers of `owner` rewritten in place from its updated weight.  Returns them:
    their own packed images are refreshed next, at their existing scales, so the next backward packs nothing."""
    out = []
    for e, _ in R.each(cache):
        shim = e.value
        R.write(shim.weight, lambda: _grad_weight(owner.weight, shim.weight))
        hit = R.index.get(owner.weight.data_ptr())
        if hit is not None and owner.weight.dtype == torch.float32:          # (the same elements: the same max|w|)
            R.index[shim.weight.data_ptr()] = hit
        e.key = R.rekey(e.key)
        out.append(shim)
    return out


wcache.register("_dkt_grad", _refresh_grad, derived=True)


def _dscale_eligible(shim):
    """The input gradient runs on the device-scaled form: what conv2d() would send to dkt_conv2d_f16s_desc."""
    return hip_eligible(shim) and not few_eligible(shim) and not direct_eligible(shim)


def _batch_stride(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1] * t.shape[2] * t.shape[3]


def _dense_per_batch(t):
    """`t` itself when its batch elements are dense and do not overlap (a longer batch stride is fine), else a copy."""
    B, C, H, W = t.shape
    return t.contiguous() if not _dense(t) or (B > 1 and t.stride(0) < C * H * W) else t


def conv_grad_prepass(gy, y=None, want_bias=True):
    """dkt_conv_grad_prepass on a dense-per-batch fp32 gradient: returns (g', gb, scale) -- g' = gy masked by y > 0 (gy
    itself without y), gb the per-channel sum of g' (None unless wanted), scale the device pair {2^e, 2^-e} of max|g'|."""
    _ffi.require_gpu(gy, *([] if y is None else [y]))
    B, C, H, W = gy.shape
    gy = _dense_per_batch(gy)
    y = None if y is None else _dense_per_batch(y)
    gm = None if y is None else torch.empty((B, C, H, W), device=gy.device, dtype=torch.float32)
    gb = torch.empty(C, device=gy.device, dtype=torch.float32) if want_bias else None
    scale = torch.empty(2, device=gy.device, dtype=torch.float32)
    ws = torch.empty(_ffi.size("dkt_conv_grad_prepass_ws_floats", B, C, H * W), device=gy.device, dtype=torch.float32)
    _ffi.call("dkt_conv_grad_prepass", gy, gy.data_ptr(), _batch_stride(gy), None if y is None else y.data_ptr(),
              0 if y is None else _batch_stride(y), None if gm is None else gm.data_ptr(),
              None if gb is None else gb.data_ptr(), scale.data_ptr(), ws.data_ptr(), B, C, H * W)
    return (gy if gm is None else gm), gb, scale


def conv2d_dscale(g, layer, scale, pack_scale=None):
    """Stride-1 convolution of `g` with `layer`'s weight (no bias) whose activation scale is the device pair `scale`
    (dkt_conv_desc.dscale): in_scale = scale[0], the result is un-scaled by scale[1] in the epilogue."""
    op = _Operands(g, layer, pack_scale)
    out = torch.empty((op.B, op.cout, op.H, op.W), device=op.device, dtype=torch.float32)
    d = _desc(op, out)
    d.bias = None                                    # (the input gradient has none, whatever the layer carries)
    d.out_scale, d.in_scale = op.pk.inv_scale, 1.0
    d.dscale = scale.data_ptr()
    d._keep = d._keep + (scale,)
    _launch([d], d.passes, out)
    return out


#: weight gradient of conv2d_autograd's 1x1 and 3x3 layers: True = dkt_conv2d_wgrad (csrc/conv_wgrad.hip), False = the vendor
#: library (torch.nn.grad.conv2d_weight) fed with the same g' -- an A/B handle like GRAD_PREPASS; 7x7 layers (but for
#: GRAD_WEIGHT7_HIP below), GRAD_PREPASS = False, CPU tensors and other dtypes stay on the vendor call either way
GRAD_WEIGHT_HIP = True
#: (Cin, Cout, K) classes that stay on the vendor call with the handle on: rows of `tools/bench_gru_train.py --wgrad` that lost
#: to it at B = 2 (us of dkt_conv2d_wgrad vs us of the vendor call)
WGRAD_VENDOR_CLASSES = {(64, 64, 3): "73.8 vs 71.0 at 120x224, 55.0 vs 51.7 at 60x112, 49.4 vs 38.6 at 30x56"}


def _out_size_s2(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def conv2d_wgrad(x, g, scale, k, x_scale=1.0, stride=1):
    """dkt_conv2d_wgrad / dkt_conv2d_wgrad_s2: the (Cout, Cin, k, k) weight gradient of a k x k convolution with padding k/2
    (k in {1, 3}) and `stride` 1 or 2 from its input `x` (B, Cin, H, W) and the masked gradient `g` (B, Cout, H, W), at
    stride 2 (B, Cout, Ho, Wo), both fp32 with dense batch elements (`g` may be a view with a longer batch stride); `scale`
    is the device pair {2^e, 2^-e} conv_grad_prepass left for `g`, `x_scale` the host power of two of the layer's forward
    activations.  Nothing is read back on the host."""
    if stride not in (1, 2):
        raise ValueError("conv2d_wgrad: stride %r is not 1 or 2" % (stride,))
    name = "dkt_conv2d_wgrad" if stride == 1 else "dkt_conv2d_wgrad_s2"
    _ffi.require_gpu(x, g, scale)
    B, cin, H, W = x.shape
    cout = g.shape[1]
    if stride == 1 and tuple(g.shape) != (B, cout, H, W):
        raise ValueError("conv2d_wgrad: g %s does not match x %s" % (tuple(g.shape), tuple(x.shape)))
    if stride == 2 and tuple(g.shape) != (B, cout, *_out_size_s2(H, W)):
        raise ValueError("conv2d_wgrad_s2: g %s is not the stride-2 gradient of x %s" % (tuple(g.shape), tuple(x.shape)))
    x, g = _dense_per_batch(x), _dense_per_batch(g)
    n = _ffi.size(name + "_ws_floats", B, cin, cout, H, W, k)
    gw = torch.empty((cout, cin, k, k), device=x.device, dtype=torch.float32)
    ws = torch.empty(n, device=x.device, dtype=torch.float32)
    _ffi.call(name, x, x.data_ptr(), _batch_stride(x), g.data_ptr(), _batch_stride(g), scale.data_ptr(), float(x_scale),
              gw.data_ptr(), ws.data_ptr(), B, cin, cout, H, W, k)
    return gw


def conv2d_wgrad_s2(x, g, scale, k, x_scale=1.0):
    """conv2d_wgrad at stride 2."""
    return conv2d_wgrad(x, g, scale, k, x_scale, stride=2)


#: weight gradient of conv2d_autograd's 7x7 stride-1 layers with at most WGRAD7_MAX_CIN input channels (the encoders' conv1,
#: the motion encoders' convf1 / convd1): True = dkt_conv2d_wgrad7 (csrc/conv_wgrad7.hip), False = the vendor library fed with
#: the same g'.  Needs GRAD_WEIGHT_HIP and the pre-pass; wider or stride-2 7x7 layers, CPU tensors and other dtypes stay on
#: the vendor call either way.  Off: an A/B handle in the manner of extractor.TRAIN_CONV_NODES
GRAD_WEIGHT7_HIP = False
WGRAD7_MAX_CIN = 4


def conv2d_wgrad7(x, g, scale, x_scale=1.0):
    """dkt_conv2d_wgrad7: the (Cout, Cin, 7, 7) weight gradient of a 7x7, stride-1, padding-3 convolution with Cin <= 4 from
    its input `x` (B, Cin, H, W) and the masked gradient `g` (B, Cout, H, W), both fp32 with dense batch elements (`g` may be a
    view with a longer batch stride); `scale` is the device pair {2^e, 2^-e} conv_grad_prepass left for `g`, `x_scale` the
    host power of two of the layer's forward activations.  Nothing is read back on the host."""
    _ffi.require_gpu(x, g, scale)
    B, cin, H, W = x.shape
    cout = g.shape[1]
    if tuple(g.shape) != (B, cout, H, W):
        raise ValueError("conv2d_wgrad7: g %s does not match x %s" % (tuple(g.shape), tuple(x.shape)))
    x, g = _dense_per_batch(x), _dense_per_batch(g)
    n = _ffi.size("dkt_conv2d_wgrad7_ws_floats", B, cin, cout, H, W)
    gw = torch.empty((cout, cin, 7, 7), device=x.device, dtype=torch.float32)
    ws = torch.empty(n, device=x.device, dtype=torch.float32)
    _ffi.call("dkt_conv2d_wgrad7", x, x.data_ptr(), _batch_stride(x), g.data_ptr(), _batch_stride(g), scale.data_ptr(),
              float(x_scale), gw.data_ptr(), ws.data_ptr(), B, cin, cout, H, W)
    return gw


#: stride-2 (Cin, Cout, K) classes whose weight gradient stays on the vendor call with the handle on: rows of
#: `tools/bench_encoder_train.py --conv` that lost to it (us of dkt_conv2d_wgrad_s2 vs us of the vendor call)
WGRAD_S2_VENDOR_CLASSES = {}
#: ... and whose input gradient does (us of dkt_conv2d_dgrad_s2 vs us of torch.nn.grad.conv2d_input)
DGRAD_S2_VENDOR_CLASSES = {}


def conv2d_dgrad_s2(g, layer, scale, hw, pack_scale=None, out=None):
    """dkt_conv2d_dgrad_s2: the (B, Cin, H, W) input gradient of a stride-2, padding k/2, k x k convolution (k in {1, 3}) from
    the masked gradient `g` (B, Cout, Ho, Wo), fp32 with dense batch elements (a view with a longer batch stride is read in
    place).  `layer` is the input-gradient layer (_grad_layer(owner): the weight transposed over (Cout, Cin) and rotated by
    180 degrees, packed once per weight version at `pack_scale`, the forward image's scale), `scale` the device pair
    conv_grad_prepass left for `g`, `hw` = (H, W) of the forward input, `out` an optional (B, Cin, H, W) fp32 destination
    with dense batch elements (every element is written).  Nothing is read back on the host."""
    _ffi.require_gpu(g, scale)
    B, cout, Ho, Wo = g.shape
    H, W = int(hw[0]), int(hw[1])
    cin, wc, k, kw = layer.weight.shape
    if wc != cout or k != kw or k not in (1, 3):
        raise ValueError("conv2d_dgrad_s2: g %s does not match the layer %s" % (tuple(g.shape), tuple(layer.weight.shape)))
    if (Ho, Wo) != _out_size_s2(H, W):
        raise ValueError("conv2d_dgrad_s2: g %s is not the stride-2 output of a %d x %d input" % (tuple(g.shape), H, W))
    g = _dense_per_batch(g)
    pk = _packed_weights(layer, [cout], pack_scale)
    if out is None:
        gx = torch.empty((B, cin, H, W), device=g.device, dtype=torch.float32)
    elif (not _dense(out) or out.dtype != torch.float32 or tuple(out.shape) != (B, cin, H, W) or out.device != g.device
          or (B > 1 and out.stride(0) < cin * H * W)):
        raise ValueError("conv2d_dgrad_s2(out=...) must be a dense-per-batch fp32 tensor of the input's shape")
    else:
        gx = out
    _ffi.call("dkt_conv2d_dgrad_s2", g, g.data_ptr(), _batch_stride(g), pk.hi.data_ptr(), pk.lo.data_ptr(), pk.inv_scale,
              scale.data_ptr(), gx.data_ptr(), _batch_stride(gx), B, cin, cout, H, W, k)
    return gx


class _Conv2dGradFn(torch.autograd.Function):
    """conv2d_autograd with GRAD_PREPASS.  apply(x, relu, owner, nparts, *params): `owner` holds the (detached) weight and
    bias the kernels read and every packed image; `params` are the tensors autograd differentiates -- nparts weights, then
    nparts biases or none -- whose concatenations along the output channels are owner.weight / owner.bias."""

    @staticmethod
    def forward(ctx, x, relu, owner, nparts, *params):
        with torch.no_grad():
            y = conv2d(x.detach(), owner, relu=relu)
        ctx.owner, ctx.relu, ctx.nparts, ctx.has_bias = owner, bool(relu), nparts, len(params) > nparts
        ctx.stride = _stride_of(owner)[0]
        ctx.splits = [int(p.shape[0]) for p in params[:nparts]]
        ctx.save_for_backward(x, owner.weight, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        n = ctx.nparts
        need_x = ctx.needs_input_grad[0]
        need_w = any(ctx.needs_input_grad[4:4 + n])
        need_b = ctx.has_bias and any(ctx.needs_input_grad[4 + n:])
        kh, kw = w.shape[2:]
        gx = gw = gb = None
        with torch.no_grad():
            gy = gy if gy.dtype == torch.float32 else gy.float()
            shim = _grad_layer(ctx.owner) if need_x else None
            cls = (x.shape[1], w.shape[0], kh)
            if ctx.stride == 2:
                # stride 2 (k in {1, 3}, _autograd_eligible): dkt_conv2d_dgrad_s2 / dkt_conv2d_wgrad_s2
                dscale = need_x and get_backend() in _PASSES and cls not in DGRAD_S2_VENDOR_CLASSES
                vendor_classes = WGRAD_S2_VENDOR_CLASSES
            else:
                dscale = need_x and _dscale_eligible(shim)
                vendor_classes = WGRAD_VENDOR_CLASSES
            wgrad = (need_w and GRAD_WEIGHT_HIP and kh == kw and kh in (1, 3) and x.is_cuda and gy.is_cuda
                     and x.dtype == torch.float32 and cls not in vendor_classes)
            wgrad7 = (need_w and GRAD_WEIGHT7_HIP and GRAD_WEIGHT_HIP and kh == kw == 7 and ctx.stride == 1
                      and x.shape[1] <= WGRAD7_MAX_CIN and x.is_cuda and gy.is_cuda and x.dtype == torch.float32)
            g, scale = gy, None
            if ctx.relu or need_b or dscale or wgrad or wgrad7:
                g, gb, scale = conv_grad_prepass(gy, y if ctx.relu else None, want_bias=need_b)
            if need_x and ctx.stride == 2:
                gx = (conv2d_dgrad_s2(g, shim, scale, x.shape[2:], shim.pack_scale) if dscale else
                      torch.nn.grad.conv2d_input(x.shape, w, g, stride=2, padding=(kh // 2, kw // 2)))
            elif need_x:
                gx = conv2d_dscale(g, shim, scale, shim.pack_scale) if dscale else conv2d(g, shim)
            if wgrad:
                gw = conv2d_wgrad(x.detach(), g, scale, kh, 2.0 ** in_exp_of(ctx.owner), ctx.stride)
            elif wgrad7:
                gw = conv2d_wgrad7(x.detach(), g, scale, 2.0 ** in_exp_of(ctx.owner))
            elif need_w:
                gw = torch.nn.grad.conv2d_weight(x.detach(), w.shape, g, stride=ctx.stride, padding=(kh // 2, kw // 2))
        gws = [None] * n if gw is None else list(gw.split(ctx.splits, 0)) if n > 1 else [gw]
        gbs = [None] * n if gb is None else list(gb.split(ctx.splits, 0)) if n > 1 else [gb]
        gws = [t if ctx.needs_input_grad[4 + i] else None for i, t in enumerate(gws)]
        gbs = [t if ctx.needs_input_grad[4 + n + i] else None for i, t in enumerate(gbs)] if ctx.has_bias else []
        return (gx, None, None, None, *gws, *gbs)


def _autograd_eligible(x, layer):
    """fp32 HIP tensor, padding k/2, no groups / dilation: a stride-1 layer with an odd square kernel, or a stride-2 layer
    with k in {1, 3} (the encoders' down-sampling layers; backward on dkt_conv2d_dgrad_s2 / dkt_conv2d_wgrad_s2, which
    needs the pre-pass: GRAD_PREPASS = False leaves stride 2 to plain torch)."""
    kh, kw = layer.weight.shape[2:]
    pad = _padding_of(layer)
    st = _stride_of(layer)
    return (x.is_cuda and x.dtype == torch.float32 and kh == kw and kh % 2 == 1 and pad == (kh // 2, kw // 2)
            and (st == (1, 1) or (st == (2, 2) and kh in (1, 3) and GRAD_PREPASS and GRAD_WEIGHT_HIP))
            and _plain_conv(layer))


def conv2d_autograd(x, layer, relu=False, owner=None):
    """[relu](conv(x) + bias) for a stride-1 "same" layer (odd square kernel, no groups / dilation) or a stride-2 1x1 / 3x3
    layer with padding k/2 as an autograd node:
    `x` a tensor or a list of tensors (the reference's torch.cat operands).  Other layers run as plain torch.
    `layer` may be a tuple of layers that share input and geometry (ConvGRU's convz, convr): their outputs are
    concatenated along channels, one convolution, and `owner` is then required.
    `owner`: a PERSISTENT Conv2d-like object whose weight / bias hold the values of `layer`'s (of the concatenation, for a
    tuple) and on which the packed images of the forward and of the input gradient are cached, keyed on the version of
    its weight; default `layer` itself when it is an nn.Module.  Without either the images are packed per call."""
    if isinstance(x, (list, tuple)):
        x = x[0] if len(x) == 1 else torch.cat(list(x), dim=1)
    if isinstance(layer, (list, tuple)):
        parts = list(layer)
        if owner is None:
            raise ValueError("conv2d_autograd: a tuple of layers needs the owner that holds their concatenation")
        if GRAD_PREPASS and _autograd_eligible(x, owner):
            params = [p.weight for p in parts] + ([] if parts[0].bias is None else [p.bias for p in parts])
            return _Conv2dGradFn.apply(x.contiguous(), relu, owner, len(parts), *params)
        merged = _LayerShim(torch.cat([p.weight for p in parts], 0),
                            None if parts[0].bias is None else torch.cat([p.bias for p in parts], 0), parts[0].padding)
        return conv2d_autograd(x, merged, relu=relu)
    w = layer.weight
    if not _autograd_eligible(x, layer):
        y = F.conv2d(x, w, layer.bias, stride=_stride_of(layer), padding=layer.padding,
                     dilation=getattr(layer, "dilation", 1), groups=getattr(layer, "groups", 1))
        return F.relu(y) if relu else y
    kh, kw = w.shape[2:]
    pad = (kh // 2, kw // 2)
    if GRAD_PREPASS:
        if owner is None:
            # a persistent module owns its images; anything else (a namespace around temporaries) packs per call, on an
            # object that dies with the call
            owner = layer if isinstance(layer, torch.nn.Module) else _LayerShim(
                w.detach(), None if layer.bias is None else layer.bias.detach(), pad, _stride_of(layer))
        return _Conv2dGradFn.apply(x.contiguous(), relu, owner, 1, *([w] if layer.bias is None else [w, layer.bias]))
    return _Conv2dFn.apply(x.contiguous(), w, layer.bias, relu)
