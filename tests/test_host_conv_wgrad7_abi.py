"""Host-side checks of dkt_conv2d_wgrad7 (no device needed): the entries refuse bad arguments before any launch,
_ffi.SIGNATURES matches the header's declarations, the workspace sizes are the recorded ones and follow the slice rule
_conv_wgrad7_ref.py restates, the GRAD_WEIGHT7_HIP handle is off, and conv2d_autograd on CPU tensors stays plain torch with
the handle on."""
import ctypes

import pytest
import torch
import torch.nn as nn

import _abi_header
import _conv_wgrad7_ref as W7

#: (B, H, W, Cin, Cout): dkt_conv2d_wgrad7_ws_floats, recorded by hand from the rule (slices * Cout * Cin * 49)
TABLE = {
    (2, 9, 35, 3, 64): 2 * 1 * 64 * 147,
    (1, 5, 70, 2, 64): 1 * 1 * 64 * 98,
    (3, 7, 9, 1, 64): 3 * 1 * 64 * 49,
    (2, 24, 40, 3, 64): 37632,               # 2 x 2 bands of 12 rows
    (2, 8, 12, 4, 70): 27440,
    (1, 12, 33, 3, 130): 19110,
    (1, 1, 1, 3, 5): 735,
    (2, 16, 64, 3, 64): 37632,               # 2 x 2 bands of 8 rows
    (3, 700, 64, 3, 64): 2483712,            # 264 slices
    (1, 2, 8200, 3, 64): 9408,
    (7, 24, 40, 3, 64): 131712,              # 14 slices
    # the layers at the training recipe's sizes: convf1 at B = 2, fnet.conv1 / cnet.conv1 at the two crops
    (2, 120, 224, 2, 64): 752640,            # 60 bands of 2 rows
    (2, 60, 112, 2, 64): 188160,             # 15 bands of 4 rows
    (2, 30, 56, 2, 64): 50176,               # 4 bands of 8 rows
    (4, 480, 896, 3, 64): 9031680,           # 240 bands of 2 rows (T = 2048)
    (16, 320, 720, 3, 64): 24084480,
    (2, 480, 896, 3, 64): 4515840,
    (8, 320, 720, 3, 64): 12042240,
}


def test_header_cites_the_reference():
    hdr = _abi_header.raw()
    block = hdr[hdr.index("weight gradient of the 7x7 stem layers"):hdr.index("long dkt_conv2d_wgrad7_ws_floats")]
    for cite in ("core/extractor.py:140, :217", "core/update.py:73", "igev_stereo/update.py:80"):
        assert cite in block, cite


def test_workspace_sizes_are_the_recorded_ones_and_follow_the_rule():
    from dkt_stereo_amd import _ffi
    ws = _ffi.lib().dkt_conv2d_wgrad7_ws_floats
    assert set(W7.CASES) | set(W7.PLAN_CASES) <= set(TABLE)
    for case, want in TABLE.items():
        B, H, W, cin, cout = case
        assert ws(B, cin, cout, H, W) == want, case
        assert W7.ws_floats(case) == want, case
    for bad in ((0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1, 0), (-1, 3, 64, 8, 8),
                (1, 5, 64, 8, 8), (1, 64, 64, 8, 8)):
        assert ws(*bad) == -2, bad


def test_entry_refuses_bad_arguments_before_launch():
    from dkt_stereo_amd import _ffi
    fn = _ffi.lib().dkt_conv2d_wgrad7
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 512)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    # dkt_conv2d_wgrad7(x, x_bs, g, g_bs, scale, x_scale, gw, ws, B, Cin, Cout, H, W, device, stream)
    good = [p, 16, p, 24, p, 1.0, p, p, 1, 2, 3, 2, 4]
    for i in (0, 2, 4, 6, 7):                                            # x, g, scale, gw, ws
        assert fn(*[null if j == i else a for j, a in enumerate(good)], -1, null) == -1, i
    for i, v in ((8, 0), (9, 0), (10, 0), (11, 0), (12, 0), (8, -1), (12, -3),
                 (9, 5), (9, 8), (9, 64),                                # Cin > 4 (with a batch stride that would fit)
                 (1, 15), (3, 23),                                       # a batch stride shorter than C*H*W
                 (5, 0.0), (5, -1.0), (5, 3.0), (5, 0.75), (5, float("inf")), (5, float("nan")), (5, 2.0 ** -140)):
        args = list(good)
        args[i] = v
        if i == 9:
            args[1] = v * 8
        assert fn(*args, -1, null) == -2, (i, v)
    assert all(v == 0.0 for v in buf)                                    # nothing was written


def test_the_3x3_entry_still_refuses_k7():
    from dkt_stereo_amd import _ffi
    assert _ffi.lib().dkt_conv2d_wgrad_ws_floats(1, 3, 64, 8, 8, 7) == -2


def test_handle_is_off_and_the_wrapper_exists():
    from dkt_stereo_amd import conv
    assert conv.GRAD_WEIGHT7_HIP is False
    assert conv.WGRAD7_MAX_CIN == W7.MAX_CIN
    assert callable(conv.conv2d_wgrad7)
    x = torch.zeros(1, 3, 4, 4)
    with pytest.raises(Exception):                                       # CPU tensors are refused, not computed elsewhere
        conv.conv2d_wgrad7(x, torch.zeros(1, 5, 4, 4), torch.ones(2))


def test_cpu_tensors_are_plain_torch_with_the_handle_on(monkeypatch):
    """CPU tensors: torch nodes only -- values and gradients equal to the torch expression's."""
    from dkt_stereo_amd import conv
    monkeypatch.setattr(conv, "GRAD_WEIGHT7_HIP", True)
    torch.manual_seed(3)
    for cin in (1, 2, 3, 5):
        lay = nn.Conv2d(cin, 7, 7, padding=3)
        x = torch.randn(2, cin, 6, 9, requires_grad=True)
        for relu in (False, True):
            y = conv.conv2d_autograd(x, lay, relu=relu)
            assert type(y.grad_fn).__name__ in ("ConvolutionBackward0", "ReluBackward0")
            want = torch.relu(lay(x)) if relu else lay(x)
            assert torch.equal(y, want)
            got = torch.autograd.grad(y.square().sum(), [x, lay.weight, lay.bias])
            ref = torch.autograd.grad(want.square().sum(), [x, lay.weight, lay.bias])
            assert all(torch.equal(a, b) for a, b in zip(got, ref))
