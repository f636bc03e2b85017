"""Host-side checks of the PCVNet backward entries (no device needed): the two symbols, the header's declarations against
_ffi.SIGNATURES, every argument error before any device call, that no workspace entry exists (the sum over levels runs inside
one thread, in ascending order: there are no per-level partials to size), and the Python block's refusals."""
import ctypes

import pytest
import torch

import _abi_header as H

NAMES = ("dkt_pcv_lookup_bwd", "dkt_pcv_pool_bwd")
E_NULL, E_SHAPE, E_LEVELS = -1, -2, -3


def test_header_declares_what_ffi_mirrors():
    from dkt_stereo_amd import _ffi
    declared = H.functions()
    lib = _ffi.lib()
    for n in NAMES:
        restype, argtypes = declared[n]
        assert restype is ctypes.c_int and n not in _ffi.RESTYPES
        assert _ffi.SIGNATURES[n] == argtypes, n
        assert hasattr(lib, n)
    # lookup_bwd: two pointer tables, five device pointers, eight sizes, device, stream
    assert len(_ffi.SIGNATURES["dkt_pcv_lookup_bwd"]) == 17 and len(_ffi.SIGNATURES["dkt_pcv_pool_bwd"]) == 11
    assert not [n for n in declared if n.startswith("dkt_pcv") and ("ws" in n or "workspace" in n)]


def test_entries_refuse_bad_arguments_before_any_device_call():
    from dkt_stereo_amd import _ffi
    lib = _ffi.lib()
    look, pool = (getattr(lib, n) for n in NAMES)
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    none = ctypes.cast(null, _ffi._pp)

    def table(n, hole=None):
        arr = (ctypes.c_void_p * 8)()
        for i in range(n):
            arr[i] = None if i == hole else p.value
        return ctypes.cast(arr, _ffi._pp)

    # lookup_bwd(pyr, coords, sigma, grad_out, grad_pyr, gcoords, gsigma, B, G, H, W1, W2, L, S, factor, device, stream)
    def LK(pyr=None, coords=p, sigma=p, gout=p, gpyr=None, gc=p, gs=p, dims=(1, 1, 1, 2), W2=8, L=2, S=3, f=2):
        pyr = table(L if 0 < L <= 8 else 1) if pyr is None else pyr
        gpyr = table(L if 0 < L <= 8 else 1) if gpyr is None else gpyr
        return look(pyr, coords, sigma, gout, gpyr, gc, gs, *dims, W2, L, S, f, -1, null)
    assert LK(pyr=none) == E_NULL and LK(coords=null) == E_NULL and LK(sigma=null) == E_NULL and LK(gout=null) == E_NULL
    assert LK(gpyr=none, gc=null, gs=null) == E_NULL                            # no result asked for
    assert LK(pyr=table(2, hole=1)) == E_NULL and LK(gpyr=table(2, hole=0)) == E_NULL
    for dims in ((0, 1, 1, 2), (1, 0, 1, 2), (1, 1, -1, 2), (1, 1, 1, 0), (65536, 1, 1, 2)):
        assert LK(dims=dims) == E_SHAPE, dims
    assert LK(W2=0) == E_SHAPE
    for S in (0, -1, 2, 4):
        assert LK(S=S) == E_SHAPE, S
    for f in (1, 0, -2):
        assert LK(f=f) == E_SHAPE, f
    for L in (0, -1, 9):
        assert LK(L=L) == E_LEVELS, L
    assert LK(W2=8, L=3, f=4) == E_LEVELS                                       # widths 8, 2, 0
    assert LK(W2=7, L=2, f=4) == E_LEVELS                                       # widths 7, 1: the sampler divides by W - 1
    assert LK(W2=1, L=1) == E_LEVELS

    # pool_bwd(grad_pyr, grad_vol, B, H, W1, W2, L, factor, divisor, device, stream)
    def PL(gpyr=None, gvol=p, dims=(1, 1, 2), W2=8, L=2, f=2, divisor=2.0):
        gpyr = table(L if 0 < L <= 8 else 1) if gpyr is None else gpyr
        return pool(gpyr, gvol, *dims, W2, L, f, divisor, -1, null)
    assert PL(gpyr=none) == E_NULL and PL(gvol=null) == E_NULL and PL(gpyr=table(2, hole=1)) == E_NULL
    for dims in ((0, 1, 2), (1, 0, 2), (1, 1, -3)):
        assert PL(dims=dims) == E_SHAPE, dims
    assert PL(W2=0) == E_SHAPE and PL(f=1) == E_SHAPE
    for divisor in (0.0, -1.0, float("nan")):
        assert PL(divisor=divisor) == E_SHAPE, divisor
    for L in (0, 9):
        assert PL(L=L) == E_LEVELS, L
    assert PL(W2=7, L=2, f=4) == E_LEVELS and PL(W2=8, L=3, f=4) == E_LEVELS


def test_python_block_refuses_cpu_tensors_under_autograd():
    """Today's message for CPU tensors is kept, with grad or without: there is no CPU path."""
    from dkt_stereo_amd import _ffi
    from dkt_stereo_amd.pcvnet_corr import CorrBlock1D
    f1, f2 = torch.zeros(1, 4, 2, 8), torch.zeros(1, 4, 2, 8)
    for a, b in ((f1, f2), (f1.clone().requires_grad_(True), f2)):
        with pytest.raises(_ffi.DktError):
            CorrBlock1D(a, b, sample_num=3, num_levels=2, downsample=3)
    with pytest.raises(_ffi.DktError):
        CorrBlock1D.corr(f1.clone().requires_grad_(True), f2)
    with pytest.raises(_ffi.DktError):                                          # widths 8, 2, 0 under autograd
        CorrBlock1D(f1.clone().requires_grad_(True), f2, sample_num=3, num_levels=3, downsample=2)
    with pytest.raises(ValueError):
        CorrBlock1D(f1, f2, sample_num=4, num_levels=2, downsample=3)
