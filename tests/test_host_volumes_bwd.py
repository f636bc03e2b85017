"""Host-side argument validation of the cost-volume backward entries (include/dktstereo.h): negative DKT_E_* codes
before any launch, so no device is needed."""
import ctypes

DKT_E_NULL, DKT_E_SHAPE, DKT_E_GROUPS = -1, -2, -5


def test_volume_bwd_argument_errors_before_launch():
    from dkt_stereo_amd import _ffi
    lib = _ffi.lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # dkt_gwc_volume_bwd(grad_vol, bstride, ref, tgt, grad_ref, grad_tgt, B, C, H, W, D, G, device, stream)
    assert lib.dkt_gwc_volume_bwd(null, 64, p, p, p, p, 1, 8, 1, 4, 2, 4, -1, null) == DKT_E_NULL
    assert lib.dkt_gwc_volume_bwd(p, 64, null, p, p, p, 1, 8, 1, 4, 2, 4, -1, null) == DKT_E_NULL
    assert lib.dkt_gwc_volume_bwd(p, 64, p, p, null, null, 1, 8, 1, 4, 2, 4, -1, null) == DKT_E_NULL
    assert lib.dkt_gwc_volume_bwd(p, 64, p, p, p, null, 1, 6, 1, 4, 2, 4, -1, null) == DKT_E_GROUPS     # 6 % 4
    assert lib.dkt_gwc_volume_bwd(p, 64, p, p, null, p, 1, 8, 1, 4, 0, 4, -1, null) == DKT_E_SHAPE      # D < 1
    assert lib.dkt_gwc_volume_bwd(p, 31, p, p, p, p, 1, 8, 1, 4, 2, 4, -1, null) == DKT_E_SHAPE        # bstride < G*D*H*W
    # dkt_concat_volume_bwd(grad_vol, bstride, grad_ref, grad_tgt, B, C, H, W, D, ref_masked, device, stream)
    assert lib.dkt_concat_volume_bwd(null, 64, p, p, 1, 2, 1, 4, 2, 1, -1, null) == DKT_E_NULL
    assert lib.dkt_concat_volume_bwd(p, 64, null, null, 1, 2, 1, 4, 2, 1, -1, null) == DKT_E_NULL
    assert lib.dkt_concat_volume_bwd(p, 64, p, p, 1, 2, 1, 4, 0, 0, -1, null) == DKT_E_SHAPE          # D < 1
    assert lib.dkt_concat_volume_bwd(p, 31, p, p, 1, 2, 1, 4, 2, 1, -1, null) == DKT_E_SHAPE          # bstride too small
    # dkt_gwc_concat_volume_bwd(grad_vol, bstride, ref, tgt, grad_ref, grad_tgt, B, C, G, grad_cat_ref, grad_cat_tgt,
    #                           Cc, ref_masked, H, W, D, device, stream)
    assert lib.dkt_gwc_concat_volume_bwd(null, 64, p, p, p, p, 1, 8, 4, p, p, 2, 1, 1, 4, 2, -1, null) == DKT_E_NULL
    assert lib.dkt_gwc_concat_volume_bwd(p, 64, p, p, null, null, 1, 8, 4, null, null, 2, 1, 1, 4, 2, -1, null) == DKT_E_NULL
    assert lib.dkt_gwc_concat_volume_bwd(p, 64, p, p, p, p, 1, 6, 4, p, p, 2, 1, 1, 4, 2, -1, null) == DKT_E_GROUPS
    assert lib.dkt_gwc_concat_volume_bwd(p, 64, p, p, p, p, 1, 8, 4, p, p, 2, 1, 1, 4, 0, -1, null) == DKT_E_SHAPE
    assert lib.dkt_gwc_concat_volume_bwd(p, 63, p, p, p, p, 1, 8, 4, p, p, 2, 1, 1, 4, 2, -1, null) == DKT_E_SHAPE
