"""The C ABI of the NeRF-supervised loss without a device: the symbols, the header against _ffi, every argument error before
any device call, the workspace table, and the Python entry points' refusals."""
import ctypes

import pytest
import torch

import _abi_header
from dkt_stereo_amd import _ffi, loss, ns_loss as N

NULL, SHAPE, ALIGN, UNSUPPORTED = -1, -2, -6, -7


def test_header_declares_the_three_entries():
    """(their signatures, the struct and the constants against _ffi: test_host_abi_mirror.py)"""
    declared = sorted(n for n in _abi_header.functions() if n.startswith("dkt_ns_"))
    assert declared == ["dkt_ns_loss", "dkt_ns_loss_bwd", "dkt_ns_loss_workspace"]


class _Host:
    """A descriptor over host buffers: valid for every check, never launched (each call below fails a check first)."""

    def __init__(self, B=2, H=5, W=6, n=2):
        self.buf = (ctypes.c_double * 4096)()
        p = ctypes.addressof(self.buf)
        d = _ffi.NsLossDesc()
        for i in range(n):
            d.pred[i], d.pred_bstride[i], d.weight[i] = p, H * W, 1.0
        d.n = n
        for k in range(3):
            d.im[k], d.im_bstride[k] = p, 3 * H * W
        d.conf, d.conf_bstride, d.target, d.target_bstride = p, H * W, p, H * W
        d.valid = d.state = d.loss = d.rec = p
        d.conf_threshold, d.max_flow, d.alpha_disp, d.alpha_photo = 0.5, 512.0, 1.0, 0.1
        d.B, d.H, d.W = B, H, W
        self.d, self.p = d, p
        g = _ffi.NsLossGrad()
        for i in range(n):
            g.grad[i] = p
        g.grad_loss = p
        self.g = g

    def fwd(self, ws=True):
        return _ffi.lib().dkt_ns_loss(self.d, self.p if ws is True else ws, -1, None)

    def bwd(self):
        return _ffi.lib().dkt_ns_loss_bwd(self.d, self.g, -1, None)


def _both(h, code):
    assert h.fwd() == code and h.bwd() == code


def test_argument_errors_before_any_device_call():
    lib = _ffi.lib()
    assert lib.dkt_ns_loss(None, None, -1, None) == NULL and lib.dkt_ns_loss_bwd(None, None, -1, None) == NULL
    assert _Host().fwd(ws=None) == NULL
    assert _Host().fwd(ws=_Host().p + 4) == ALIGN
    for field in ("conf", "loss", "rec", "valid", "state"):
        h = _Host()
        setattr(h.d, field, None)
        _both(h, NULL)
    h = _Host()
    h.d.pred[1] = None
    _both(h, NULL)
    h = _Host()
    h.d.im[2] = None
    _both(h, NULL)
    h = _Host()
    h.d.target = None                      # without a target the mask comes in through valid_in
    _both(h, NULL)
    h = _Host()
    h.g.grad[1] = None
    assert h.bwd() == NULL
    h = _Host()
    h.g.grad_loss = None
    assert h.bwd() == NULL
    for field, value in (("B", 0), ("H", 0), ("W", -1), ("H", 3), ("W", 3), ("n", 0), ("n", _ffi.NS_MAX_PRED + 1)):
        h = _Host()
        setattr(h.d, field, value)
        _both(h, SHAPE)
    h = _Host()
    h.d.pred_bstride[0] = 5 * 6 - 1        # a batch stride shorter than an image
    _both(h, SHAPE)
    h = _Host()
    h.d.im_bstride[1] = 3 * 5 * 6 - 1
    _both(h, SHAPE)
    h = _Host()
    h.d.conf_bstride = 1
    _both(h, SHAPE)
    h = _Host()
    h.d.pred[0] = h.p + 2
    _both(h, ALIGN)
    h = _Host()
    h.d.rec = h.p + 4
    _both(h, ALIGN)
    h = _Host()
    h.g.grad[0] = h.p + 1
    assert h.bwd() == ALIGN
    h = _Host(B=40000)
    _both(h, UNSUPPORTED)                  # B * n > 65535


def test_workspace_table_does_not_depend_on_n():
    lib = _ffi.lib()
    assert _ffi.SIGNATURES["dkt_ns_loss_workspace"] == [ctypes.c_int] * 3          # (B, H, W): no n
    per_block = 8 * (8 + 4 * _ffi.NS_MAX_PRED)                                      # 2112 bytes of fp64 partials per 16 x 16 tile
    assert per_block == 2112
    table = {(1, 4, 4): 2112 + 64, (1, 5, 9): 2112 + 184, (2, 17, 53): 2 * 2 * 4 * 2112 + 7208, (1, 16, 16): 2112 + 1024,
             (1, 17, 16): 2 * 2112 + 1088, (2, 480, 896): 2 * 30 * 56 * 2112 + 3440640}
    for (B, H, W), nbytes in table.items():
        assert lib.dkt_ns_loss_workspace(B, H, W) == nbytes, (B, H, W)
    assert lib.dkt_ns_loss_workspace(0, 8, 8) == SHAPE and lib.dkt_ns_loss_workspace(1, 3, 8) == SHAPE
    assert lib.dkt_ns_loss_workspace(1, 8, 3) == SHAPE


def test_python_refusals():
    p = [torch.zeros(1, 1, 5, 6), torch.zeros(1, 1, 5, 6)]
    t, im = torch.zeros(1, 5, 6), torch.zeros(1, 3, 5, 6)
    with pytest.raises(_ffi.DktError):
        N.ns_loss(p, t, t, im, im, im)
    with pytest.raises(_ffi.DktError):
        N.trinocular_loss(p[0], im, im, im, t, torch.ones(1, 1, 5, 6))
    with pytest.raises(_ffi.DktError):
        N.photometric_planes(p[0], im, im, im)
    with pytest.raises(TypeError):
        N.ns_loss(p, t, t, im, im, im, trinocular_loss=False)
    assert "ns_loss" not in loss.__losses__ and N.ns_loss not in loss.__losses__.values()
