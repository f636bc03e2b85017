"""Host-side checks of the convolution backward (no device needed): the new ABI entries refuse bad arguments before any
launch, _ffi.SIGNATURES matches the header's declarations, the GRAD_PREPASS handle, and conv2d_autograd(..., owner=) on CPU
tensors, which stays plain torch."""
import ctypes

import torch
import torch.nn as nn

import _abi_header

NAMES = ["dkt_conv_grad_prepass_ws_floats", "dkt_conv_grad_prepass"]


def test_header_facts():
    """dkt_conv_desc ends with the device scale and opens with its four operand pointers (the whole struct against _ffi.ConvDesc:
    test_host_abi_mirror.py); the exponent clamp of the pre-pass."""
    want = _abi_header.structs()["dkt_conv_desc"]
    assert want[-1] == ("dscale", ctypes.c_void_p, 0) and want[0] == ("src", ctypes.c_void_p, 4)
    assert _abi_header.defines()["DKT_CONV_GRAD_MAX_EXP"] == 80


def test_entries_refuse_bad_arguments_before_launch():
    from dkt_stereo_amd import _ffi
    lib = _ffi.lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 256)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    ws, pre = (getattr(lib, n) for n in NAMES)
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
    assert all(v == 0.0 for v in buf)                                   # nothing was written


def _conv_desc(p, **fields):
    """A dkt_conv_desc nothing is wrong with (2 -> 2 channels, 3x3, B = 1, 2 x 2 pixels, every tensor at `p`) but for `fields`;
    src / src_channels set the first operand's."""
    from dkt_stereo_amd import _ffi
    d = _ffi.ConvDesc()
    d.src[0], d.src_bstride[0], d.src_channels[0], d.nsrc = p, 8, 2, 1
    d.w_hi = d.w_lo = d.out = p
    d.out_scale = d.in_scale = 1.0
    d.out_bstride = 8
    d.B, d.H, d.W, d.Cout, d.KH, d.KW = 1, 2, 2, 2, 3, 3
    for k, v in fields.items():
        if k in ("src", "src_channels"):
            getattr(d, k)[0] = v
        else:
            setattr(d, k, v)
    return d


def test_conv_desc_refuses_bad_arguments_before_launch():
    """dkt_conv2d_f16s_desc / _pair, the one validator of the split-fp16 convolution.  The codes of a descriptor that says what
    a positional entry of the parent commit said (dkt_conv2d_f16s, _strided, _gate_zr, _gate_out, _dscale) are the codes that
    entry gave to the same arguments, taken from the parent's library (profiles/conv2d_one_entry.txt)."""
    from dkt_stereo_amd import _ffi
    lib = _ffi.lib()
    buf = (ctypes.c_float * 256)()
    p = ctypes.addressof(buf)

    def run(passes=3, **fields):
        return lib.dkt_conv2d_f16s_desc(ctypes.byref(_conv_desc(p, **fields)), passes, -1, None)

    assert lib.dkt_conv2d_f16s_desc(None, 3, -1, None) == -1
    # the device-scaled form: what dkt_conv2d_f16s_dscale refused (out_scale carries w_inv_scale)
    for k in ("w_hi", "w_lo", "out", "src"):
        assert run(dscale=p, **{k: None}) == -1, k
    for k, v, want in (("B", 0, -2), ("H", 0, -2), ("Cout", -1, -2), ("nsrc", 5, -2), ("out_scale", 0.0, -2), ("KH", 5, -7),
                       ("KW", 1, -7)):
        assert run(dscale=p, **{k: v}) == want, (k, v)
    assert run(passes=4, dscale=p) == -7
    # ... and what it had no argument for
    gate = dict(e0=p, e1=p, h=p, out2=p)
    for extra in (dict(bias=p), dict(relu=1), dict(in_norm=p), dict(stats_ws=p, stats_part=p), dict(stats_ws=p), dict(stats_part=p),
                  dict(stride=2), dict(epilogue=1, Cout=128, **gate), dict(epilogue=2, **gate), dict(epilogue=3, e0=p)):
        assert run(dscale=p, **extra) == -7, extra
    assert run(dscale=p, in_scale=0.0) == -2
    # the plain and strided forms (dkt_conv2d_f16s, dkt_conv2d_f16s_strided)
    for k in ("w_hi", "w_lo", "out", "src"):
        assert run(**{k: None}) == -1, k
    for k, v, want in (("B", 0, -2), ("H", 0, -2), ("W", 0, -2), ("Cout", 0, -2), ("Cout", -1, -2), ("nsrc", 0, -2), ("nsrc", 5, -2),
                       ("B", 65536, -2), ("out_scale", 0.0, -2), ("in_scale", 0.0, -2), ("src_channels", 0, -1), ("KH", 5, -7),
                       ("KW", 1, -7), ("stride", 3, -7), ("stride", -1, -7), ("epilogue", 4, -7), ("epilogue", -1, -7)):
        assert run(**{k: v}) == want, (k, v)
    assert run(passes=4) == -7 and run(passes=0) == -7
    assert run(stride=2, B=0) == -2 and run(stride=2, KH=5) == -7
    # epilogue 1 (dkt_conv2d_f16s_gate_zr: Cout = 2 * Ch, Ch a multiple of 64) and epilogue 2 (dkt_conv2d_f16s_gate_out)
    for k in ("e0", "e1", "h", "out2"):
        assert run(epilogue=1, Cout=128, **dict(gate, **{k: None})) == -1, k
    for cout in (192, 64, 2):
        assert run(epilogue=1, Cout=cout, **gate) == -7, cout
    for k in ("e0", "e1", "h"):
        assert run(epilogue=2, **dict(gate, **{k: None})) == -1, k
    assert run(epilogue=2, Cout=0, **gate) == -2 and run(epilogue=3) == -1
    for epi in (1, 2, 3):
        assert run(epilogue=epi, Cout=128, stride=2, **gate) == -7, epi
    for epi in (1, 2, 3):
        assert run(epilogue=epi, Cout=128, stats_ws=p, stats_part=p, **gate) == -7, epi
    assert run(stats_ws=p) == -1 and run(stats_part=p) == -1
    # the pair launch: either descriptor is checked the same way, and neither may carry dscale, in_norm or stride 2
    good = _conv_desc(p)
    pair = lib.dkt_conv2d_f16s_pair
    for bad, want in ((_conv_desc(p, dscale=p), -7), (_conv_desc(p, dscale=p, bias=p), -7), (_conv_desc(p, in_norm=p), -7),
                      (_conv_desc(p, stride=2), -7), (_conv_desc(p, KH=1, KW=1), -7), (_conv_desc(p, Cout=33), -7),
                      (_conv_desc(p, out=None), -1), (_conv_desc(p, H=0), -2)):
        assert pair(ctypes.byref(bad), ctypes.byref(good), 3, -1, None) == want
        assert pair(ctypes.byref(good), ctypes.byref(bad), 3, -1, None) == want
    assert pair(None, ctypes.byref(good), 3, -1, None) == -1 and pair(ctypes.byref(good), None, 3, -1, None) == -1
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
