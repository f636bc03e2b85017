"""The feature encoder's instance norms as autograd nodes (BasicEncoder(norm_fn='instance') under autograd;
core/extractor.py:21-60 with the affine-free InstanceNorm2d that keeps no running statistics).

    instance_norm(x, eps, relu)      -> [relu]((x - mean) * invstd) per (n, c) plane, invstd = 1 / sqrt(var_biased + eps)
    instance_norm_add_relu(a, c, eps) -> relu(a + relu((c - mean_c) * invstd_c)), the tail of a residual block

Forward: the inference kernels themselves (dkt_instance_norm; dkt_instance_norm_stats + dkt_instance_norm_add_relu), the
same bits, plus dkt_instance_norm_finalize on the same workspace for the (planes, 2) tensor of (mean, 1/std) the backward
recomputes the normalised value from -- no further pass over the activation.  Backward: dkt_instance_norm_bwd /
dkt_instance_norm_add_relu_bwd, two launches, fp64 plane sums added in slice order, no atomics.  Once differentiable.
fp32 tensors on a HIP device; anything else is an error (no fallback)."""
import torch
from torch.autograd.function import once_differentiable

from . import _ffi


def _require_f32(*tensors):
    _ffi.require_gpu(*tensors)
    for t in tensors:
        if t.dtype != torch.float32:
            raise _ffi.DktError("the instance-norm training nodes take fp32 tensors (got %s)" % t.dtype)


def _require_planes(x):
    if x.dim() != 4 or x.numel() == 0:
        raise _ffi.DktError("the instance-norm training nodes take non-empty (N, C, H, W) tensors (got %s)" % (tuple(x.shape),))


def _workspace(query, planes, HW, device):
    return torch.empty(_ffi.size(query, planes, HW), device=device, dtype=torch.uint8)


def _finalize(ws, planes, HW, eps, x):
    mi = torch.empty((planes, 2), device=x.device, dtype=torch.float32)
    _ffi.call("dkt_instance_norm_finalize", x, ws.data_ptr(), planes, HW, eps, mi.data_ptr())
    return mi


class _InstanceNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps, relu):
        _require_f32(x)
        _require_planes(x)
        x = x.contiguous()
        n, c, h, w = x.shape
        planes, HW = n * c, h * w
        ws = _workspace("dkt_instance_norm_workspace", planes, HW, x.device)
        y = torch.empty_like(x)
        _ffi.call("dkt_instance_norm", x, x.data_ptr(), y.data_ptr(), ws.data_ptr(), planes, HW, eps, int(relu))
        ctx.save_for_backward(x, _finalize(ws, planes, HW, eps, x))
        ctx.relu = bool(relu)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        x, mi = ctx.saved_tensors
        _require_f32(gy)
        gy = gy.contiguous()
        n, c, h, w = x.shape
        planes, HW = n * c, h * w
        ws = _workspace("dkt_instance_norm_bwd_workspace", planes, HW, x.device)
        gx = torch.empty_like(x)
        _ffi.call("dkt_instance_norm_bwd", x, gy.data_ptr(), x.data_ptr(), mi.data_ptr(), int(ctx.relu), gx.data_ptr(),
                  ws.data_ptr(), planes, HW)
        return gx, None, None


class _InstanceNormAddReluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, c, eps):
        _require_f32(a, c)
        _require_planes(c)
        if a.shape != c.shape:
            raise _ffi.DktError("instance_norm_add_relu: a %s does not match c %s" % (tuple(a.shape), tuple(c.shape)))
        a, c = a.contiguous(), c.contiguous()
        n, ch, h, w = c.shape
        planes, HW = n * ch, h * w
        ws = _workspace("dkt_instance_norm_workspace", planes, HW, c.device)
        out = torch.empty_like(c)
        _ffi.call("dkt_instance_norm_stats", c, c.data_ptr(), ws.data_ptr(), planes, HW)
        _ffi.call("dkt_instance_norm_add_relu", c, a.data_ptr(), c.data_ptr(), out.data_ptr(), ws.data_ptr(), planes, HW, eps)
        # `a` is not kept: the sign of the output carries the outer ReLU's mask
        ctx.save_for_backward(c, out, _finalize(ws, planes, HW, eps, c))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        need_a, need_c = ctx.needs_input_grad[:2]
        if not (need_a or need_c):
            return None, None, None
        c, out, mi = ctx.saved_tensors
        _require_f32(gout)
        gout = gout.contiguous()
        n, ch, h, w = c.shape
        planes, HW = n * ch, h * w
        ga = torch.empty_like(c) if need_a else None
        gc = torch.empty_like(c) if need_c else None
        ws = _workspace("dkt_instance_norm_bwd_workspace", planes, HW, c.device) if need_c else None
        _ffi.call("dkt_instance_norm_add_relu_bwd", c, gout.data_ptr(), out.data_ptr(), c.data_ptr(), mi.data_ptr(), _ffi.ptr(ga),
                  _ffi.ptr(gc), _ffi.ptr(ws), planes, HW)
        return ga, gc, None


def instance_norm(x, eps=1e-5, relu=False):
    """x (N, C, H, W) -> [relu](instance_norm(x)), affine-free, instance statistics.  Saves x and (mean, 1/std)."""
    return _InstanceNormFn.apply(x, float(eps), bool(relu))


def instance_norm_add_relu(a, c, eps=1e-5):
    """a, c (N, C, H, W) -> relu(a + relu(instance_norm(c))).  Saves c, the output and (mean, 1/std)."""
    return _InstanceNormAddReluFn.apply(a, c, float(eps))
