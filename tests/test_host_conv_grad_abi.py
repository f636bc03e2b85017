"""Host-side checks of the convolution backward (no device needed): the new ABI entries refuse bad arguments before any
launch, _ffi.SIGNATURES matches the header's declarations, the GRAD_PREPASS handle, and conv2d_autograd(..., owner=) on CPU
tensors, which stays plain torch."""
import ctypes
import os
import re

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["dkt_conv_grad_prepass_ws_floats", "dkt_conv_grad_prepass", "dkt_conv2d_f16s_dscale"]
_CTYPES = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float}


def _declared(name):
    """(return type, [argument ctypes]) of `name` as include/dktstereo.h declares it."""
    hdr = open(os.path.join(HERE, "..", "include", "dktstereo.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\b(int|long)\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
    assert m, name
    args = []
    for a in m.group(2).split(","):
        a = " ".join(a.split())
        if "*const *" in a or "* const *" in a:
            args.append(ctypes.POINTER(ctypes.c_void_p))
        elif "*" in a:
            base = a.replace("const", "").split("*")[0].strip()
            args.append({"int": ctypes.POINTER(ctypes.c_int), "long": ctypes.POINTER(ctypes.c_long)}.get(base, ctypes.c_void_p))
        else:
            args.append(_CTYPES[a.split()[0]])
    return m.group(1), args


def test_signatures_match_the_header():
    from dkt_stereo_amd import _ffi
    lib = _ffi.lib()
    for name in NAMES:
        ret, args = _declared(name)
        assert _ffi.SIGNATURES[name] == args, name
        assert _ffi.RESTYPES.get(name, ctypes.c_int) is (ctypes.c_long if ret == "long" else ctypes.c_int), name
        assert hasattr(lib, name)
    hdr = open(os.path.join(HERE, "..", "include", "dktstereo.h")).read()
    assert re.search(r"#define\s+DKT_CONV_GRAD_MAX_EXP\s+80\b", hdr)


def test_entries_refuse_bad_arguments_before_launch():
    from dkt_stereo_amd import _ffi
    lib = _ffi.lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 256)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    ws, pre, conv = (getattr(lib, n) for n in NAMES)
    # the workspace: 2 floats per (batch, channel, 4096-element segment)
    assert ws(2, 3, 5000) == 2 * 2 * 3 * 2 and ws(1, 1, 1) == 2 and ws(1, 1, 4096) == 2 and ws(1, 1, 4097) == 4
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1)):
        assert ws(*bad) == -2, bad
    # dkt_conv_grad_prepass(gy, bs, y, bs, gmask, gb, scale, ws, B, C, HW, device, stream)
    tail = (1, 2, 4, -1, null)
    assert pre(null, 8, null, 0, null, p, p, p, *tail) == -1            # gy
    assert pre(p, 8, null, 0, null, p, null, p, *tail) == -1            # scale
    assert pre(p, 8, null, 0, null, p, p, null, *tail) == -1            # ws
    assert pre(p, 8, p, 8, null, p, p, p, *tail) == -1                  # y without a destination for g'
    for bad in ((0, 2, 4), (1, 0, 4), (1, 2, 0), (1, -2, 4)):
        assert pre(p, 8, null, 0, null, null, p, p, *bad, -1, null) == -2, bad
    assert pre(p, 7, null, 0, null, null, p, p, *tail) == -2            # a batch stride shorter than C*HW
    assert pre(p, 8, p, 7, p, null, p, p, *tail) == -2
    # dkt_conv2d_f16s_dscale(src, ch, bs, nsrc, w_hi, w_lo, w_inv_scale, scale, out, out_bs, B, H, W, Cout, KH, KW, passes, ...)
    src = (ctypes.c_void_p * 1)(p.value)
    ch = (ctypes.c_int * 1)(2)
    bs = (ctypes.c_long * 1)(8)
    good = [src, ch, bs, 1, p, p, 1.0, p, p, 8, 1, 2, 2, 2, 3, 3, 3]
    for k in (4, 5, 7, 8):
        assert conv(*[null if i == k else a for i, a in enumerate(good)], -1, null) == -1, k
    assert conv(ctypes.cast(null, ctypes.POINTER(ctypes.c_void_p)), *good[1:], -1, null) == -1
    for i, v, want in ((10, 0, -2), (11, 0, -2), (13, -1, -2), (3, 5, -2), (6, 0.0, -2), (14, 5, -7), (15, 1, -7), (16, 4, -7)):
        args = list(good)
        args[i] = v
        assert conv(*args, -1, null) == want, (i, v)
    assert all(v == 0.0 for v in buf)                                   # nothing was written


def test_grad_prepass_handle():
    from dkt_stereo_amd import conv
    assert conv.GRAD_PREPASS is True


def test_owner_on_cpu_tensors_is_plain_torch():
    """CPU tensors: torch nodes only, whatever the owner -- a module, a tuple of layers with the object that holds their
    concatenation -- with values and gradients equal to the torch expression's."""
    from types import SimpleNamespace
    from dkt_stereo_amd import conv
    torch.manual_seed(3)
    lay = nn.Conv2d(5, 7, 3, padding=1)
    x = torch.randn(2, 5, 6, 9, requires_grad=True)
    for relu in (False, True):
        y = conv.conv2d_autograd(x, lay, relu=relu, owner=lay)
        assert type(y.grad_fn).__name__ in ("ConvolutionBackward0", "ReluBackward0")
        want = torch.relu(lay(x)) if relu else lay(x)
        assert torch.equal(y, want)
        got = torch.autograd.grad(y.square().sum(), [x, lay.weight, lay.bias])
        ref = torch.autograd.grad(want.square().sum(), [x, lay.weight, lay.bias])
        assert all(torch.equal(a, b) for a, b in zip(got, ref))
    assert "_dkt_grad" not in lay.__dict__ and "_dkt_packed" not in lay.__dict__
    a, b = nn.Conv2d(5, 4, 3, padding=1), nn.Conv2d(5, 4, 3, padding=1)
    owner = SimpleNamespace(weight=torch.cat([a.weight, b.weight], 0).detach(), bias=torch.cat([a.bias, b.bias], 0).detach(),
                            padding=(1, 1))
    y = conv.conv2d_autograd(x, (a, b), owner=owner)
    want = torch.cat([a(x), b(x)], 1)
    assert torch.allclose(y, want, rtol=0, atol=1e-6)
    got = torch.autograd.grad(y.square().sum(), [x, a.weight, b.weight, a.bias, b.bias])
    ref = torch.autograd.grad(want.square().sum(), [x, a.weight, b.weight, a.bias, b.bias])
    assert all(torch.allclose(g, r, rtol=1e-5, atol=1e-5) for g, r in zip(got, ref))
