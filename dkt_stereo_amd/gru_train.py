"""The update operator's gates and resamplers as autograd nodes (BasicMultiUpdateBlock under autograd; core/update.py:23-32
== meta_arch/igev_stereo/update.py:33-41, and core/update.py:87-96).

    gate_zr(azr, cz, cr, h) -> (z, rh)    z = sigmoid(azr[:, :Ch] + cz), r = sigmoid(azr[:, Ch:] + cr), rh = r * h
    gate_out(aq, cq, z, h)  -> h'         q = tanh(aq + cq), h' = (1 - z) * h + z * q
    pool2x(x)                             F.avg_pool2d(x, 3, stride=2, padding=1)
    interp(x, size)                       F.interpolate(x, size, mode="bilinear", align_corners=True)

Forward: the inference kernels' arithmetic, bit for bit (dkt_gru_gate_zr_train / _out_train write the one extra plane the
backward needs, r and q; the resamplers are dkt_pool2x / dkt_interp_bilinear themselves).  Backward: one launch per node,
deterministic, no atomics.  fp32 tensors on a HIP device; anything else is an error (no fallback)."""
import torch

from . import _ffi


def _strided(t):
    """`t` (B, C, H, W) as the gate kernels read it: (tensor, batch stride).  A channel slice of a wider buffer is read
    in place; any other layout is copied."""
    B, C, H, W = t.shape
    if t.stride(3) == 1 and t.stride(2) == W and t.stride(1) == H * W and (B == 1 or t.stride(0) >= C * H * W):
        return t, t.stride(0)
    t = t.contiguous()
    return t, C * H * W


def _require_f32(*tensors):
    _ffi.require_gpu(*tensors)
    for t in tensors:
        if t.dtype != torch.float32:
            raise _ffi.DktError("the update operator's training nodes take fp32 tensors (got %s)" % t.dtype)


class _GateZrFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, azr, cz, cr, h):
        _require_f32(azr, cz, cr, h)
        B, Ch, H, W = h.shape
        if azr.shape != (B, 2 * Ch, H, W) or cz.shape != h.shape or cr.shape != h.shape:
            raise _ffi.DktError("gate_zr: azr %s, cz %s, cr %s do not match h %s"
                                % (tuple(azr.shape), tuple(cz.shape), tuple(cr.shape), tuple(h.shape)))
        azr = azr.contiguous()
        (cz, cz_bs), (cr, cr_bs), (h, h_bs) = _strided(cz), _strided(cr), _strided(h)
        z, r, rh = (torch.empty((B, Ch, H, W), device=h.device, dtype=torch.float32) for _ in range(3))
        _ffi.call("dkt_gru_gate_zr_train", h, azr.data_ptr(), cz.data_ptr(), cz_bs, cr.data_ptr(), cr_bs, h.data_ptr(), h_bs,
                  z.data_ptr(), r.data_ptr(), rh.data_ptr(), Ch * H * W, B, Ch, H * W)
        ctx.save_for_backward(z, r, h)
        ctx.h_bs = h_bs
        return z, rh

    @staticmethod
    def backward(ctx, gz, grh):
        z, r, h = ctx.saved_tensors
        need_a = any(ctx.needs_input_grad[:3])
        need_h = ctx.needs_input_grad[3]
        if not (need_a or need_h):
            return None, None, None, None
        _require_f32(gz, grh)
        B, Ch, H, W = z.shape
        gz = gz.contiguous()
        grh, grh_bs = _strided(grh)
        gazr = torch.empty((B, 2 * Ch, H, W), device=z.device, dtype=torch.float32) if need_a else None
        gh = torch.empty_like(z) if need_h else None
        _ffi.call("dkt_gru_gate_zr_bwd", z, gz.data_ptr(), grh.data_ptr(), grh_bs, z.data_ptr(), r.data_ptr(), h.data_ptr(),
                  ctx.h_bs, _ffi.ptr(gazr), _ffi.ptr(gh), B, Ch, H * W)
        na, ncz, ncr = ctx.needs_input_grad[:3]
        # the gradients of cz and cr are the halves of gazr: views, no further writes
        return (gazr if na else None, gazr[:, :Ch] if ncz else None, gazr[:, Ch:] if ncr else None, gh)


class _GateOutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, aq, cq, z, h):
        _require_f32(aq, cq, z, h)
        B, Ch, H, W = h.shape
        if aq.shape != h.shape or cq.shape != h.shape or z.shape != h.shape:
            raise _ffi.DktError("gate_out: aq %s, cq %s, z %s do not match h %s"
                                % (tuple(aq.shape), tuple(cq.shape), tuple(z.shape), tuple(h.shape)))
        aq, z = aq.contiguous(), z.contiguous()
        (cq, cq_bs), (h, h_bs) = _strided(cq), _strided(h)
        q, out = (torch.empty((B, Ch, H, W), device=h.device, dtype=torch.float32) for _ in range(2))
        _ffi.call("dkt_gru_gate_out_train", h, aq.data_ptr(), cq.data_ptr(), cq_bs, z.data_ptr(), h.data_ptr(), h_bs,
                  q.data_ptr(), out.data_ptr(), Ch * H * W, B, Ch, H * W)
        ctx.save_for_backward(z, q, h)
        ctx.h_bs = h_bs
        return out

    @staticmethod
    def backward(ctx, gout):
        z, q, h = ctx.saved_tensors
        naq, ncq, nz, nh = ctx.needs_input_grad
        if not (naq or ncq or nz or nh):
            return None, None, None, None
        _require_f32(gout)
        B, Ch, H, W = z.shape
        gout, g_bs = _strided(gout)
        gaq = torch.empty_like(z) if (naq or ncq) else None
        gz = torch.empty_like(z) if nz else None
        gh = torch.empty_like(z) if nh else None
        _ffi.call("dkt_gru_gate_out_bwd", z, gout.data_ptr(), g_bs, z.data_ptr(), q.data_ptr(), h.data_ptr(), ctx.h_bs,
                  _ffi.ptr(gaq), _ffi.ptr(gz), _ffi.ptr(gh), B, Ch, H * W)
        return gaq if naq else None, gaq if ncq else None, gz, gh


class _Pool2xFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _require_f32(x)
        x = x.contiguous()
        B, C, H, W = x.shape
        y = torch.empty((B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), device=x.device, dtype=torch.float32)
        _ffi.call("dkt_pool2x", x, x.data_ptr(), y.data_ptr(), B * C, H, W)
        ctx.shape = (B, C, H, W)
        return y

    @staticmethod
    def backward(ctx, gy):
        if not ctx.needs_input_grad[0]:
            return None
        _require_f32(gy)
        B, C, H, W = ctx.shape
        gy = gy.contiguous()
        gx = torch.empty(ctx.shape, device=gy.device, dtype=torch.float32)
        _ffi.call("dkt_pool2x_bwd", gy, gy.data_ptr(), gx.data_ptr(), B * C, H, W)
        return gx


class _InterpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, Ho, Wo):
        _require_f32(x)
        x = x.contiguous()
        B, C, H, W = x.shape
        y = torch.empty((B, C, Ho, Wo), device=x.device, dtype=torch.float32)
        _ffi.call("dkt_interp_bilinear", x, x.data_ptr(), y.data_ptr(), B * C, H, W, Ho, Wo)
        ctx.shape = (B, C, H, W)
        return y

    @staticmethod
    def backward(ctx, gy):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        _require_f32(gy)
        B, C, H, W = ctx.shape
        gy = gy.contiguous()
        gx = torch.empty(ctx.shape, device=gy.device, dtype=torch.float32)
        _ffi.call("dkt_interp_bilinear_bwd", gy, gy.data_ptr(), gx.data_ptr(), B * C, H, W, gy.shape[2], gy.shape[3])
        return gx, None, None


def gate_zr(azr, cz, cr, h):
    """azr (B, 2Ch, H, W), cz, cr, h (B, Ch, H, W) -> (z, rh).  Saves z, r, h."""
    return _GateZrFn.apply(azr, cz, cr, h)


def gate_out(aq, cq, z, h):
    """aq, cq, z, h (B, Ch, H, W) -> h'.  Saves z, q, h."""
    return _GateOutFn.apply(aq, cq, z, h)


def pool2x(x):
    """update.pool2x with a gradient.  Saves nothing but the shape."""
    return _Pool2xFn.apply(x)


def interp(x, size):
    """update.interp(x, dest) for dest.shape[2:] == size, with a gradient.  Saves nothing but the shape."""
    Ho, Wo = size
    return _InterpFn.apply(x, int(Ho), int(Wo))
