"""Drop-in replacement for PCVNet's correlation block, ``meta_arch/pcvnet/corr.py:18-61``
(SURVEY.md 8f-3), on the HIP kernels of libdktstereo.so:

    corr_fn = CorrBlock1D(fmap1, fmap2, sample_num=9, num_levels=4, downsample=2)
    corr = corr_fn(coords1, sigma)      # coords, sigma (B,G,H,W) -> (B, L*G*S, H, W) float32

The all-pairs volume is the RAFT one (dkt_corr1d_build); the pyramid is pooled by the
reference's compress factor (4 when ``downsample == 2``, else 2: dkt_pool_rows) and the lookup
samples ``sample_num`` taps spaced by the per-pixel ``sigma`` around each of the G gaussian
means (dkt_pcv_lookup).

Differentiable like the reference's: with grad enabled, feature maps that require grad make the
pyramid one autograd node (backward: dkt_pcv_pool_bwd and the two products of ``corr._BuildFn``),
and a level, ``sigma`` or ``coords`` that requires grad makes the lookup one node (backward:
dkt_pcv_lookup_bwd).  ``sigma`` is the previous iteration's head output and arrives with its graph
(``model.py:141`` -> ``:122``), so the loss reaches the sigma head through the next lookup.  Under
``no_grad``, or with nothing requiring grad, the same forward kernels run without any node.
"""
import torch

from . import _ffi
from .corr import _BuildFn, _build_pyramid, _volume_grads


def _pool_levels(lvl, num_levels, factor):
    """[lvl, dkt_pool_rows(lvl), ...]: the pyramid of corr.py:29-31 on a (N,1,1,W2) level 0."""
    pyr = [lvl]
    for _ in range(num_levels - 1):
        w = lvl.shape[-1]
        if w // factor < 1:
            raise ValueError("width %d cannot be pooled by %d" % (w, factor))
        nxt = torch.empty((lvl.shape[0], 1, 1, w // factor), device=lvl.device, dtype=torch.float32)
        _ffi.call("dkt_pool_rows", lvl, lvl.data_ptr(), nxt.data_ptr(), lvl.shape[0], w, factor)
        pyr.append(nxt)
        lvl = nxt
    return pyr


def _lookup(pyramid, coords, sigma, w2, S, factor):
    B, G, H, W1 = coords.shape
    Lv = len(pyramid)
    out = torch.empty((B, Lv * G * S, H, W1), device=coords.device, dtype=torch.float32)
    _ffi.call("dkt_pcv_lookup", coords, _ffi.ptr_array(pyramid), coords.data_ptr(), sigma.data_ptr(),
              out.data_ptr(), B, G, H, W1, w2, Lv, S, factor)
    return out


def _require_sampled_width(w2, num_levels, factor):
    """The reference's sampler divides by W_i - 1: a level of width 1 has no gradient (and NaN values)."""
    if w2 // factor ** (num_levels - 1) < 2:
        raise _ffi.DktError("PCVNet CorrBlock1D: the last of %d levels of a width-%d volume pooled by %d is narrower than 2; "
                            "the reference divides by zero there and no gradient exists" % (num_levels, w2, factor))


class _PyramidFn(torch.autograd.Function):
    """(fmap1, fmap2) -> pyramid levels.  Backward: avg-pool chain + 1/sqrt(C) folded by dkt_pcv_pool_bwd, then the two
    products of corr._BuildFn."""

    @staticmethod
    def forward(ctx, fmap1, fmap2, num_levels, factor, divisor):
        lvl0, = _build_pyramid(fmap1, fmap2, 1, divisor)
        ctx.save_for_backward(fmap1, fmap2)
        ctx.meta = (num_levels, factor, divisor)
        return tuple(_pool_levels(lvl0, num_levels, factor))

    @staticmethod
    def backward(ctx, *glv):
        f1, f2 = ctx.saved_tensors
        L, factor, divisor = ctx.meta
        B, _, H, W1 = f1.shape
        W2 = f2.shape[3]
        N = B * H * W1
        glv = [g.contiguous().float() if g is not None
               else torch.zeros((N, 1, 1, W2 // factor ** i), device=f1.device, dtype=torch.float32) for i, g in enumerate(glv)]
        gvol = torch.empty((N, W2), device=f1.device, dtype=torch.float32)
        _ffi.call("dkt_pcv_pool_bwd", gvol, _ffi.ptr_array(glv), gvol.data_ptr(), B, H, W1, W2, L, factor, float(divisor))
        return _volume_grads(gvol, f1, f2, ctx.needs_input_grad[0], ctx.needs_input_grad[1]) + (None, None, None)


class _LookupFn(torch.autograd.Function):
    """(coords, sigma, levels...) -> lookup.  Backward: dkt_pcv_lookup_bwd; the level gradients scatter into zeroed
    level-shaped tensors, and only what requires grad is allocated or computed."""

    @staticmethod
    def forward(ctx, coords, sigma, w2, S, factor, *levels):
        ctx.save_for_backward(coords, sigma, *levels)
        ctx.meta = (w2, S, factor)
        return _lookup(list(levels), coords, sigma, w2, S, factor)

    @staticmethod
    def backward(ctx, gout):
        coords, sigma, *levels = ctx.saved_tensors
        w2, S, factor = ctx.meta
        B, G, H, W1 = coords.shape
        gout = gout.contiguous().float()
        need = ctx.needs_input_grad
        gcoords = torch.empty_like(coords) if need[0] else None
        gsigma = torch.empty_like(sigma) if need[1] else None
        glv = [torch.zeros_like(l) for l in levels] if any(need[5:]) else None
        _ffi.call("dkt_pcv_lookup_bwd", gout, _ffi.ptr_array(levels), coords.data_ptr(), sigma.data_ptr(), gout.data_ptr(),
                  None if glv is None else _ffi.ptr_array(glv), _ffi.ptr(gcoords), _ffi.ptr(gsigma),
                  B, G, H, W1, w2, len(levels), S, factor)
        if glv is None:
            glv = [None] * len(levels)
        return (gcoords, gsigma, None, None, None) + tuple(g if n else None for g, n in zip(glv, need[5:]))


class CorrBlock1D:
    def __init__(self, fmap1, fmap2, sample_num, num_levels=4, downsample=2):
        self.sample_num = sample_num
        self.num_levels = num_levels
        self.compress_factor = 4 if downsample == 2 else 2
        # corr.py:25 -- the reference keeps the tap offsets as a tensor attribute
        half = sample_num // 2
        self.index = torch.arange(-half, half + 1, dtype=torch.float32)
        if self.index.numel() != sample_num:
            raise ValueError("sample_num must be odd (the reference's view(1,1,1,sample_num) needs it)")
        self._w2 = fmap2.shape[3]
        if torch.is_grad_enabled() and (fmap1.requires_grad or fmap2.requires_grad):
            _require_sampled_width(self._w2, num_levels, self.compress_factor)
            divisor = float(torch.sqrt(torch.tensor(fmap1.shape[1]).float()))
            self.corr_pyramid = list(_PyramidFn.apply(fmap1.float().contiguous(), fmap2.float().contiguous(), num_levels,
                                                      self.compress_factor, divisor))
            return
        corr = CorrBlock1D.corr(fmap1, fmap2)
        batch, h1, w1, _, w2 = corr.shape
        self.corr_pyramid = _pool_levels(corr.reshape(batch * h1 * w1, 1, 1, w2), num_levels, self.compress_factor)

    def __call__(self, coords, sigma, test_mode=False):
        _ffi.require_gpu(coords, sigma)
        if coords.shape != sigma.shape:
            raise ValueError("coords %s and sigma %s disagree" % (tuple(coords.shape), tuple(sigma.shape)))
        S, f = self.sample_num, self.compress_factor
        if torch.is_grad_enabled() and (coords.requires_grad or sigma.requires_grad
                                        or any(p.requires_grad for p in self.corr_pyramid)):
            _require_sampled_width(self._w2, self.num_levels, f)
            # casts and copies stay outside the node: autograd undoes them
            return _LookupFn.apply(coords.float().contiguous(), sigma.float().contiguous(), self._w2, S, f,
                                   *[p.float().contiguous() for p in self.corr_pyramid])
        return _lookup(self.corr_pyramid, coords.float().contiguous(), sigma.float().contiguous(), self._w2, S, f)

    @staticmethod
    def corr(fmap1, fmap2):
        B, D, H, W1 = fmap1.shape
        W2 = fmap2.shape[3]
        divisor = float(torch.sqrt(torch.tensor(D).float()))
        if torch.is_grad_enabled() and (fmap1.requires_grad or fmap2.requires_grad):
            lvl0, = _BuildFn.apply(fmap1.float(), fmap2.float(), 1, divisor)
        else:
            lvl0, = _build_pyramid(fmap1.float(), fmap2.float(), 1, divisor)
        return lvl0.view(B, H, W1, 1, W2)
