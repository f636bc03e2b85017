"""Host-side checks of the stride-2 backward entries (no device needed): the three symbols exist and _ffi.SIGNATURES matches the
header's declarations; every argument error returns its code before any device is touched (device -1, host buffers that stay
untouched); the workspace size is positive, monotone and follows the plan _conv_s2_ref restates; conv2d_autograd on a CPU
stride-2 layer and extractor._Conv2d under autograd on the CPU -- handle off and on -- stay plain torch."""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

import _abi_header
import _conv_s2_ref as S


def test_header_cites_the_reference():
    hdr = _abi_header.raw()
    block = hdr[hdr.index("backward of the encoders' stride-2 convolutions"):hdr.index("int dkt_conv2d_dgrad_s2")]
    assert "core/extractor.py:6-60, :122-175" in block


def test_workspace_is_positive_monotone_and_follows_the_plan():
    from dkt_stereo_amd import _ffi
    ws = _ffi.lib().dkt_conv2d_wgrad_s2_ws_floats
    for case in S.CASES + [(2, 320, 720, 3, 64, 96), (2, 160, 360, 1, 96, 128), (2, 80, 180, 3, 128, 128)]:
        B, H, W, k, cin, cout = case
        _, bands, _, _ = S.plan(case)
        n = ws(B, cin, cout, H, W, k)
        assert n == B * bands * cout * cin * k * k and n > 0, case
    # monotone in every size at a fixed band height: the fixed cases stay far below the 256 work items at which the plan
    # stops halving, so their bands are those of the smallest slice throughout
    for B, H, W, k, cin, cout in S.CASES:
        n = ws(B, cin, cout, H, W, k)
        for grown in ((B + 1, cin, cout, H, W, k), (B, cin + 1, cout, H, W, k), (B, cin, cout + 1, H, W, k),
                      (B, cin, cout, H + 1, W, k), (B, cin, cout, H + 2, W, k), (B, cin, cout, H + 9, W, k)):
            assert ws(*grown) >= n, grown
    for bad in ((0, 1, 1, 1, 1, 1), (1, 0, 1, 1, 1, 1), (1, 1, 0, 1, 1, 1), (1, 1, 1, 0, 1, 1), (1, 1, 1, 1, 0, 1),
                (1, 1, 1, 1, 1, 0), (1, 1, 1, 1, 1, 2), (1, 1, 1, 1, 1, 5), (1, 1, 1, 1, 1, 7), (-1, 1, 1, 1, 1, 3)):
        assert ws(*bad) == -2, bad


def test_wgrad_refuses_bad_arguments_before_launch():
    from dkt_stereo_amd import _ffi
    fn = _ffi.lib().dkt_conv2d_wgrad_s2
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 256)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    # dkt_conv2d_wgrad_s2(x, x_bs, g, g_bs, scale, x_scale, gw, ws, B, Cin, Cout, H, W, K, device, stream): Ho x Wo = 2 x 3
    good = [p, 40, p, 18, p, 1.0, p, p, 1, 2, 3, 4, 5, 3]
    for i in (0, 2, 4, 6, 7):                                            # x, g, scale, gw, ws
        assert fn(*[null if j == i else a for j, a in enumerate(good)], -1, null) == -1, i
    for i, v in ((8, 0), (9, 0), (10, 0), (11, 0), (12, 0), (8, -1), (13, 0), (13, 2), (13, 5), (13, 7),
                 (1, 39), (3, 17),                                       # a batch stride shorter than C*H*W / C*Ho*Wo
                 (5, 0.0), (5, -1.0), (5, 3.0), (5, float("inf")), (5, float("nan"))):
        args = list(good)
        args[i] = v
        assert fn(*args, -1, null) == -2, (i, v)
    assert all(v == 0.0 for v in buf)                                    # nothing was written


def test_dgrad_refuses_bad_arguments_before_launch():
    from dkt_stereo_amd import _ffi
    fn = _ffi.lib().dkt_conv2d_dgrad_s2
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 256)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    # dkt_conv2d_dgrad_s2(g, g_bs, w_hi, w_lo, w_inv_scale, scale, gx, gx_bs, B, Cin, Cout, H, W, K, device, stream)
    good = [p, 18, p, p, 0.5, p, p, 40, 1, 2, 3, 4, 5, 3]
    for i in (0, 2, 3, 5, 6):                                            # g, w_hi, w_lo, scale, gx
        assert fn(*[null if j == i else a for j, a in enumerate(good)], -1, null) == -1, i
    for i, v in ((8, 0), (9, 0), (10, 0), (11, 0), (12, 0), (8, -1), (13, 0), (13, 2), (13, 5), (13, 7),
                 (1, 17), (7, 39),                                       # a batch stride shorter than C*Ho*Wo / C*H*W
                 (4, 0.0), (4, -1.0), (4, float("inf")), (4, float("nan"))):
        args = list(good)
        args[i] = v
        assert fn(*args, -1, null) == -2, (i, v)
    assert all(v == 0.0 for v in buf)


def test_cpu_stride2_layer_is_plain_torch():
    """conv2d_autograd on a CPU stride-2 layer: F.conv2d under plain autograd, values and gradients equal."""
    from dkt_stereo_amd import conv
    torch.manual_seed(4)
    for k in (1, 3):
        lay = nn.Conv2d(5, 7, k, stride=2, padding=k // 2)
        x = torch.randn(2, 5, 7, 10, requires_grad=True)
        for relu in (False, True):
            y = conv.conv2d_autograd(x, lay, relu=relu)
            assert type(y.grad_fn).__name__ in ("ConvolutionBackward0", "ReluBackward0")
            want = F.conv2d(x, lay.weight, lay.bias, stride=2, padding=k // 2)
            want = torch.relu(want) if relu else want
            assert torch.equal(y, want)
            got = torch.autograd.grad(y.square().sum(), [x, lay.weight, lay.bias])
            ref = torch.autograd.grad(want.square().sum(), [x, lay.weight, lay.bias])
            assert all(torch.equal(a, b) for a, b in zip(got, ref))


def test_cpu_encoder_conv_is_plain_torch_with_the_handle_off_and_on(monkeypatch):
    from dkt_stereo_amd import extractor
    assert extractor.TRAIN_CONV_NODES in (False, True)
    torch.manual_seed(5)
    for k, stride in ((3, 1), (3, 2), (1, 2), (7, 1)):
        lay = extractor._Conv2d(4, 6, kernel_size=k, stride=stride, padding=k // 2)
        x = torch.randn(2, 4, 9, 12, requires_grad=True)
        want = F.conv2d(x, lay.weight, lay.bias, stride=stride, padding=k // 2)
        ref = torch.autograd.grad(want.square().sum(), [x, lay.weight, lay.bias])
        for handle in (False, True):
            monkeypatch.setattr(extractor, "TRAIN_CONV_NODES", handle)
            y = lay(x)
            assert type(y.grad_fn).__name__ == "ConvolutionBackward0", (k, stride, handle)
            assert torch.equal(y, want)
            got = torch.autograd.grad(y.square().sum(), [x, lay.weight, lay.bias])
            assert all(torch.equal(a, b) for a, b in zip(got, ref))
