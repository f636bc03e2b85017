"""Host-side checks of the soft-argmin entries (no device needed): the three symbols, the header's declarations against
_ffi.SIGNATURES, their argument errors before any device call, the workspace rule on a literal table, the refusal of CPU
tensors, and GWCNet's handle with the torch lines still behind it on the CPU."""
import ctypes

import pytest
import torch

NAMES = {"dkt_soft_argmin_fwd": "int", "dkt_soft_argmin_bwd": "int", "dkt_soft_argmin_bwd_workspace": "long"}
E_NULL, E_SHAPE, E_ALIGN, E_UNSUPPORTED = -1, -2, -6, -7


def test_entries_refuse_bad_arguments_before_any_device_call():
    from dkt_stereo_amd import _ffi
    lib = _ffi.lib()
    fwd, bwd, wsb = (getattr(lib, n) for n in NAMES)
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    p, off = ctypes.c_void_p(base), ctypes.c_void_p(base + 2)
    big = 1 << 40
    # fwd(cost, cost_bstride, out_scale, out, B, Dc, h, w, factor, device, stream) at B = 1, Dc = 2, h = 1, w = 2
    assert fwd(null, 4, 1.0, p, 1, 2, 1, 2, 4, -1, null) == E_NULL
    assert fwd(p, 4, 1.0, null, 1, 2, 1, 2, 4, -1, null) == E_NULL
    for dims in ((0, 2, 1, 2), (1, 0, 1, 2), (1, 2, -1, 2), (1, 2, 1, 0)):
        assert fwd(p, 4, 1.0, p, *dims, 4, -1, null) == E_SHAPE, dims
    assert fwd(p, 3, 1.0, p, 1, 2, 1, 2, 4, -1, null) == E_SHAPE                      # batch stride shorter than an image
    for factor in (0, 2, 3, 8, -4):
        assert fwd(p, 4, 1.0, p, 1, 2, 1, 2, factor, -1, null) == E_UNSUPPORTED, factor
    assert fwd(p, big, 1.0, p, 1, 65, 1, 2, 4, -1, null) == E_UNSUPPORTED               # D = 260
    assert fwd(p, big, 1.0, p, 1, 257, 1, 2, 1, -1, null) == E_UNSUPPORTED              # D = 257
    assert fwd(p, big, 1.0, p, 65536, 2, 1, 2, 4, -1, null) == E_UNSUPPORTED            # B beyond the grid
    assert fwd(p, big, 1.0, p, 1, 1, 1 << 14, 1 << 14, 4, -1, null) == E_UNSUPPORTED    # H * W = 2^32
    assert fwd(p, big, 1.0, p, 1, 1, 1 << 20, 1, 1, -1, null) == E_UNSUPPORTED          # more tile rows than the grid holds
    assert fwd(off, 4, 1.0, p, 1, 2, 1, 2, 4, -1, null) == E_ALIGN
    assert fwd(p, 4, 1.0, off, 1, 2, 1, 2, 4, -1, null) == E_ALIGN
    # bwd(gout, gout_bstride, cost, cost_bstride, out_scale, gcost, ws, B, Dc, h, w, factor, device, stream): 32 output pixels
    assert bwd(null, 32, p, 4, 1.0, p, p, 1, 2, 1, 2, 4, -1, null) == E_NULL
    assert bwd(p, 32, null, 4, 1.0, p, p, 1, 2, 1, 2, 4, -1, null) == E_NULL
    assert bwd(p, 32, p, 4, 1.0, null, p, 1, 2, 1, 2, 4, -1, null) == E_NULL
    assert bwd(p, 32, p, 4, 1.0, p, null, 1, 2, 1, 2, 4, -1, null) == E_NULL            # factor 4 needs the workspace
    assert bwd(p, 32, p, 4, 1.0, p, p, 0, 2, 1, 2, 4, -1, null) == E_SHAPE
    assert bwd(p, 32, p, 3, 1.0, p, p, 1, 2, 1, 2, 4, -1, null) == E_SHAPE
    assert bwd(p, 31, p, 4, 1.0, p, p, 1, 2, 1, 2, 4, -1, null) == E_SHAPE              # gout's batch stride shorter than a map
    assert bwd(p, 1, p, 4, 1.0, p, p, 1, 2, 1, 2, 1, -1, null) == E_SHAPE
    assert bwd(p, 32, p, 4, 1.0, p, p, 1, 2, 1, 2, 2, -1, null) == E_UNSUPPORTED
    assert bwd(p, 32, p, big, 1.0, p, p, 1, 65, 1, 2, 4, -1, null) == E_UNSUPPORTED
    assert bwd(p, 32, p, 4, 1.0, p, p, 65536, 2, 1, 2, 4, -1, null) == E_UNSUPPORTED
    for bad in range(4):
        args = [p, 32, p, 4, 1.0, p, p, 1, 2, 1, 2, 4, -1, null]
        args[(0, 2, 5, 6)[bad]] = off
        assert bwd(*args) == E_ALIGN, bad
    # the workspace: 4 B Dc (4h)(4w) bytes at factor 4, none at factor 1, the entries' error codes otherwise
    table = {(1, 48, 16, 32, 4): 4 * 48 * 64 * 128, (2, 48, 64, 128, 4): 4 * 2 * 48 * 256 * 512, (1, 1, 1, 1, 4): 64,
             (3, 64, 2, 5, 4): 4 * 3 * 64 * 8 * 20, (2, 48, 6, 10, 1): 0, (1, 256, 7, 9, 1): 0,
             (0, 48, 1, 1, 4): E_SHAPE, (1, 48, 1, -1, 1): E_SHAPE, (1, 48, 1, 1, 2): E_UNSUPPORTED,
             (1, 65, 1, 1, 4): E_UNSUPPORTED, (1, 257, 1, 1, 1): E_UNSUPPORTED, (65536, 1, 1, 1, 1): E_UNSUPPORTED}
    for dims, want in table.items():
        assert wsb(*dims) == want, dims


def test_cpu_tensors_are_refused_with_and_without_gradients():
    from dkt_stereo_amd import _ffi
    from dkt_stereo_amd.soft_argmin import soft_argmin
    for cost in (torch.zeros(1, 4, 2, 3), torch.zeros(1, 1, 4, 2, 3), torch.zeros(1, 4, 2, 3, requires_grad=True)):
        for factor in (1, 4):
            with pytest.raises(_ffi.DktError):
                soft_argmin(cost, factor)
    with pytest.raises(_ffi.DktError):
        soft_argmin(torch.zeros(1, 4, 2, 3), 2)


def test_gwcnet_keeps_the_torch_lines_behind_the_handle():
    """gwcnet.SOFT_ARGMIN_HIP exists and is a bool; a CPU cost takes the reference's torch lines whatever it says."""
    import torch.nn.functional as F
    from dkt_stereo_amd import gwcnet
    assert isinstance(gwcnet.SOFT_ARGMIN_HIP, bool)
    net = gwcnet.GWCNet(gwcnet.make_args(maxdisp=16)).eval()
    feat = torch.randn(1, 32, 4, 3, 5, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        got = net._predict(net.classif3, feat)
        cost = net.classif3[2](gwcnet._cbn3(net.classif3[0], feat, True))
        up = F.interpolate(cost, scale_factor=4, mode="trilinear", align_corners=False)
        want = -gwcnet.disparity_regression(F.softmax(up.squeeze(1), dim=1), 16).unsqueeze(1)
    assert got.shape == (1, 1, 12, 20) and torch.equal(got, want)
