"""Host-side checks of the weight-gradient entries (no device needed): they refuse bad arguments before any launch, the
workspace size follows the slice rule _conv_wgrad_ref.plan restates, _ffi.SIGNATURES matches the header's declarations, the
GRAD_WEIGHT_HIP handle, and conv2d_autograd on CPU tensors, which stays plain torch."""
import ctypes

import torch
import torch.nn as nn

import _abi_header
import _conv_wgrad_ref as WR


def test_header_cites_the_reference():
    hdr = _abi_header.raw()
    block = hdr[hdr.index("/* dkt_conv2d_wgrad:"):hdr.index("long dkt_conv2d_wgrad_ws_floats")]
    assert "core/update.py:9-10, 19-21, 72-76, 111-113" in block


def test_workspace_follows_the_slice_rule():
    from dkt_stereo_amd import _ffi
    ws = _ffi.lib().dkt_conv2d_wgrad_ws_floats
    for case in WR.CASES + [(2, 120, 224, 3, 384, 256), (2, 60, 112, 3, 384, 128), (2, 30, 56, 1, 36, 64)]:
        B, H, W, k, cin, cout = case
        _, bands, _, _ = WR.plan(case)
        assert ws(B, cin, cout, H, W, k) == B * bands * cout * cin * k * k, case
    for bad in ((0, 1, 1, 1, 1, 1), (1, 0, 1, 1, 1, 1), (1, 1, 0, 1, 1, 1), (1, 1, 1, 0, 1, 1), (1, 1, 1, 1, 0, 1),
                (1, 1, 1, 1, 1, 0), (1, 1, 1, 1, 1, 2), (1, 1, 1, 1, 1, 5), (1, 1, 1, 1, 1, 7), (-1, 1, 1, 1, 1, 3)):
        assert ws(*bad) == -2, bad


def test_entry_refuses_bad_arguments_before_launch():
    from dkt_stereo_amd import _ffi
    fn = _ffi.lib().dkt_conv2d_wgrad
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 256)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    # dkt_conv2d_wgrad(x, x_bs, g, g_bs, scale, x_scale, gw, ws, B, Cin, Cout, H, W, K, device, stream)
    good = [p, 16, p, 24, p, 1.0, p, p, 1, 2, 3, 2, 4, 3]
    for i in (0, 2, 4, 6, 7):                                            # x, g, scale, gw, ws
        assert fn(*[null if j == i else a for j, a in enumerate(good)], -1, null) == -1, i
    for i, v in ((8, 0), (9, 0), (10, 0), (11, 0), (12, 0), (8, -1), (13, 0), (13, 2), (13, 5), (13, 7),
                 (1, 15), (3, 23),                                       # a batch stride shorter than C*H*W
                 (5, 0.0), (5, -1.0), (5, 3.0), (5, 0.75), (5, float("inf")), (5, float("nan")), (5, 2.0 ** -140)):
        args = list(good)
        args[i] = v
        assert fn(*args, -1, null) == -2, (i, v)
    assert all(v == 0.0 for v in buf)                                    # nothing was written


def test_grad_weight_handle():
    from dkt_stereo_amd import conv
    assert conv.GRAD_WEIGHT_HIP is True
    assert conv.GRAD_PREPASS is True


def test_cpu_tensors_are_plain_torch():
    """CPU tensors: torch nodes only, with the handle on -- values and gradients equal to the torch expression's."""
    from dkt_stereo_amd import conv
    torch.manual_seed(3)
    for k in (1, 3):
        lay = nn.Conv2d(5, 7, k, padding=k // 2)
        x = torch.randn(2, 5, 6, 9, requires_grad=True)
        for relu in (False, True):
            y = conv.conv2d_autograd(x, lay, relu=relu)
            assert type(y.grad_fn).__name__ in ("ConvolutionBackward0", "ReluBackward0")
            want = torch.relu(lay(x)) if relu else lay(x)
            assert torch.equal(y, want)
            got = torch.autograd.grad(y.square().sum(), [x, lay.weight, lay.bias])
            ref = torch.autograd.grad(want.square().sum(), [x, lay.weight, lay.bias])
            assert all(torch.equal(a, b) for a, b in zip(got, ref))
