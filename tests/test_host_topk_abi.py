"""Host-side checks of the top-k regression entries (no device needed): the two symbols, the header's declarations against
_ffi.SIGNATURES, every argument error before any device call, and the Python entry's refusals (CPU tensors, k, D)."""
import ctypes

import pytest
import torch

NAMES = ("dkt_topk_regress_fwd", "dkt_topk_regress_bwd")
E_NULL, E_SHAPE, E_ALIGN, E_UNSUPPORTED = -1, -2, -6, -7


def test_entries_refuse_bad_arguments_before_any_device_call():
    from dkt_stereo_amd import _ffi
    lib = _ffi.lib()
    fwd, bwd = (getattr(lib, n) for n in NAMES)
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    p, off = ctypes.c_void_p(base), ctypes.c_void_p(base + 2)
    big = 1 << 40

    # fwd(cost, cost_bstride, samples, samples_bstride, out, idx, B, D, h, w, k, device, stream) at B = 1, D = 4, h = 1, w = 2
    def F(cost=p, cbs=8, samples=null, sbs=0, out=p, idx=null, dims=(1, 4, 1, 2), k=2):
        return fwd(cost, cbs, samples, sbs, out, idx, *dims, k, -1, null)
    assert F(cost=null) == E_NULL and F(out=null) == E_NULL
    for dims in ((0, 4, 1, 2), (1, 0, 1, 2), (1, 4, -1, 2), (1, 4, 1, 0)):
        assert F(dims=dims) == E_SHAPE, dims
    for k in (0, -1, 5, 9):                                                      # k < 1, k > D (9 > 8 as well: the shape comes first)
        assert F(k=k) == E_SHAPE, k
    assert F(cbs=7) == E_SHAPE                                                   # batch strides shorter than an image
    assert F(samples=p, sbs=7) == E_SHAPE
    assert F(cbs=big, dims=(1, 16, 1, 2), k=9) == E_UNSUPPORTED                  # k beyond the registers
    assert F(cbs=big, dims=(1, 257, 1, 2)) == E_UNSUPPORTED                      # a plane index beyond a byte
    assert F(cbs=big, dims=(65536, 4, 1, 2)) == E_UNSUPPORTED                    # B beyond the grid
    assert F(cbs=big, dims=(1, 4, 1 << 16, 1 << 15)) == E_UNSUPPORTED            # h * w = 2^31
    assert F(cost=off) == E_ALIGN and F(out=off) == E_ALIGN and F(samples=off, sbs=8) == E_ALIGN
    assert F(idx=ctypes.c_void_p(base + 1), k=0) == E_SHAPE                      # (idx is bytes: no alignment of its own to miss)

    # bwd(gout, gout_bstride, cost, cost_bstride, samples, samples_bstride, idx, gcost, gsamples, B, D, h, w, k, device, stream)
    def G(gout=p, gbs=2, cost=p, cbs=8, samples=null, sbs=0, idx=p, gcost=p, gsamples=null, dims=(1, 4, 1, 2), k=2):
        return bwd(gout, gbs, cost, cbs, samples, sbs, idx, gcost, gsamples, *dims, k, -1, null)
    assert G(gout=null) == E_NULL and G(cost=null) == E_NULL and G(idx=null) == E_NULL
    assert G(gcost=null) == E_NULL                                               # no gradient asked for
    assert G(gsamples=p) == E_NULL                                               # gsamples without samples
    for dims in ((0, 4, 1, 2), (1, 0, 1, 2), (1, 4, -1, 2), (1, 4, 1, 0)):
        assert G(dims=dims) == E_SHAPE, dims
    for k in (0, 5):
        assert G(k=k) == E_SHAPE, k
    assert G(cbs=7) == E_SHAPE and G(gbs=1) == E_SHAPE and G(samples=p, sbs=7) == E_SHAPE
    assert G(cbs=big, dims=(1, 16, 1, 2), k=9) == E_UNSUPPORTED
    assert G(cbs=big, dims=(1, 257, 1, 2)) == E_UNSUPPORTED
    assert G(cbs=big, dims=(65536, 4, 1, 2)) == E_UNSUPPORTED
    assert G(cbs=big, gbs=big, dims=(1, 4, 1 << 16, 1 << 15)) == E_UNSUPPORTED
    for bad in ("gout", "cost", "gcost"):
        assert G(**{bad: off}) == E_ALIGN, bad
    assert G(samples=off, sbs=8) == E_ALIGN
    assert G(samples=p, sbs=8, gcost=null, gsamples=off) == E_ALIGN


def test_python_entry_refuses_cpu_tensors_bad_k_and_large_d():
    from dkt_stereo_amd import _ffi, submodule, topk
    assert submodule.regression_topk is topk.regression_topk
    cost = torch.zeros(1, 4, 2, 3)
    for c, s in ((cost, None), (cost, torch.zeros_like(cost)), (cost.clone().requires_grad_(True), None),
                 (cost, torch.zeros_like(cost).requires_grad_(True))):
        with pytest.raises(_ffi.DktError):
            topk.regression_topk(c, s, 2)
    with pytest.raises(_ffi.DktError):
        topk.cgi_disparity_head(cost[:, None], torch.zeros(1, 9, 8, 12))
    for k in (0, -1, 5, 2.5):                                                    # D = 4
        with pytest.raises(_ffi.DktError):
            topk.regression_topk(cost, None, k)
    with pytest.raises(_ffi.DktError):
        topk.regression_topk(torch.zeros(1, 16, 2, 3), None, 9)                  # k <= D but beyond 8
    with pytest.raises(_ffi.DktError):
        topk.regression_topk(torch.zeros(1, 257, 1, 1), None, 2)
