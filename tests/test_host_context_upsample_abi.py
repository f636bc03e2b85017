"""Host-side checks of the context up-sampling training entries (no device needed): the three symbols, the header's
declarations against _ffi.SIGNATURES, their argument errors before any device call, and the refusal of CPU tensors."""
import ctypes

import pytest
import torch

NAMES = ("dkt_context_upsample_bwd", "dkt_context_upsample_logits_fwd", "dkt_context_upsample_logits_bwd")
E_NULL, E_SHAPE, E_ALIGN, E_UNSUPPORTED = -1, -2, -6, -7


def test_entries_refuse_bad_arguments_before_any_device_call():
    from dkt_stereo_amd import _ffi
    lib = _ffi.lib()
    bwd, lfwd, lbwd = (getattr(lib, n) for n in NAMES)
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 256)()
    base = ctypes.addressof(buf)
    base += -base % 16                                               # a 16-byte aligned address inside the buffer
    p, off = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    # (gout, gout_bstride, disp, nine, [scale,] gdisp, gnine, ws, B, h, w, device, stream) at B = 1, h = 1, w = 2: 32 fine pixels
    for fn, s in ((bwd, ()), (lbwd, (4.0,))):
        assert fn(null, 32, p, p, *s, p, p, p, 1, 1, 2, -1, null) == E_NULL
        assert fn(p, 32, null, p, *s, p, p, p, 1, 1, 2, -1, null) == E_NULL
        assert fn(p, 32, p, null, *s, p, p, p, 1, 1, 2, -1, null) == E_NULL
        assert fn(p, 32, p, p, *s, null, null, p, 1, 1, 2, -1, null) == E_NULL       # neither gradient wanted
        assert fn(p, 32, p, p, *s, p, p, null, 1, 1, 2, -1, null) == E_NULL          # gdisp needs the workspace
        assert fn(p, 32, p, p, *s, p, p, p, 0, 1, 2, -1, null) == E_SHAPE
        assert fn(p, 32, p, p, *s, p, p, p, 1, -1, 2, -1, null) == E_SHAPE
        assert fn(p, 32, p, p, *s, p, p, p, 1, 1, 0, -1, null) == E_SHAPE
        assert fn(p, 31, p, p, *s, p, p, p, 1, 1, 2, -1, null) == E_SHAPE            # batch stride shorter than an image
        assert fn(p, 34, p, p, *s, p, p, p, 1, 1, 2, -1, null) == E_ALIGN            # batch stride not a multiple of 4
        assert fn(off, 32, p, p, *s, p, p, p, 1, 1, 2, -1, null) == E_ALIGN          # gout is read 16 bytes at a time
        assert fn(p, 32, p, off, *s, p, p, p, 1, 1, 2, -1, null) == E_ALIGN          # and so are the nine planes
        assert fn(p, 32, p, p, *s, p, off, p, 1, 1, 2, -1, null) == E_ALIGN
        assert fn(p, 32, p, p, *s, p, p, p, 65536, 1, 2, -1, null) == E_UNSUPPORTED  # B beyond the grid
        assert fn(p, 1 << 36, p, p, *s, p, p, p, 1, 1 << 16, 1 << 15, -1, null) == E_UNSUPPORTED     # h * w beyond int
    assert lfwd(null, p, 4.0, p, 1, 1, 2, -1, null) == E_NULL
    assert lfwd(p, null, 4.0, p, 1, 1, 2, -1, null) == E_NULL
    assert lfwd(p, p, 4.0, null, 1, 1, 2, -1, null) == E_NULL
    assert lfwd(p, p, 4.0, p, 1, 0, 2, -1, null) == E_SHAPE
    assert lfwd(p, p, 4.0, off, 1, 1, 2, -1, null) == E_ALIGN
    assert lfwd(p, p, 4.0, p, 65536, 1, 2, -1, null) == E_UNSUPPORTED
    for bad in (3.0, 0.0, -4.0, float("inf"), float("nan")):                          # scale: a finite positive power of two
        assert lfwd(p, p, bad, p, 1, 1, 2, -1, null) == E_UNSUPPORTED, bad
        assert lbwd(p, 32, p, p, bad, p, p, p, 1, 1, 2, -1, null) == E_UNSUPPORTED, bad


def test_cpu_tensors_are_refused_with_and_without_gradients():
    from dkt_stereo_amd import _ffi
    from dkt_stereo_amd.submodule import context_upsample
    from dkt_stereo_amd.upsample import context_upsample_logits
    disp, nine = torch.zeros(1, 1, 2, 3), torch.zeros(1, 9, 8, 12)
    for d, n in ((disp, nine), (disp.clone().requires_grad_(True), nine.clone().requires_grad_(True))):
        with pytest.raises(_ffi.DktError):
            context_upsample(d, n)
        with pytest.raises(_ffi.DktError):
            context_upsample_logits(d, n)
