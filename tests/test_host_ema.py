"""ema.ema_update_ without a device: the ABI's argument errors (negative DKT_E_* before any launch) and the torch fallback,
which must compute exactly the reference's expression (tools/ft_dkt.py:179-181)."""
import ctypes
import math

import torch
import torch.nn as nn

DKT_OK, DKT_E_NULL, DKT_E_SHAPE, DKT_E_UNSUPPORTED = 0, -1, -2, -7


def test_ema_update_argument_errors_before_launch():
    from dkt_stereo_amd import _ffi
    lib = _ffi.lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_long * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # dkt_ema_update(t, s, n, count, decay, one_minus_decay, absmax, device, stream)
    assert lib.dkt_ema_update(p, p, p, -1, 0.5, 0.5, null, -1, null) == DKT_E_SHAPE
    assert lib.dkt_ema_update(null, p, p, 2, 0.5, 0.5, null, -1, null) == DKT_E_NULL
    assert lib.dkt_ema_update(p, null, p, 2, 0.5, 0.5, null, -1, null) == DKT_E_NULL
    assert lib.dkt_ema_update(p, p, null, 2, 0.5, 0.5, null, -1, null) == DKT_E_NULL
    assert lib.dkt_ema_update(p, p, p, 2, math.nan, 0.5, null, -1, null) == DKT_E_UNSUPPORTED
    assert lib.dkt_ema_update(p, p, p, 2, 0.5, math.inf, null, -1, null) == DKT_E_UNSUPPORTED
    assert lib.dkt_ema_update(null, null, null, 0, 0.5, 0.5, null, -1, null) == DKT_OK        # nothing to do


def _net(seed, dtype=torch.float32):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Conv2d(3, 8, 3), nn.BatchNorm2d(8), nn.Conv2d(8, 5, 1), nn.Linear(7, 1)).to(dtype)


def test_fallback_equals_reference_expression():
    from dkt_stereo_amd.ema import ema_update_
    for dtype in (torch.float32, torch.float64):
        for decay in (0.9999, 0.99999, 0.5):
            teacher, student, want = _net(1, dtype), _net(2, dtype), _net(1, dtype)
            for t in teacher.parameters():
                t.requires_grad = False
            for t_params, s_params in zip(want.parameters(), student.parameters()):        # tools/ft_dkt.py:179-181
                t_params.data = (decay * t_params.data + (1 - decay) * s_params.data)
                t_params.requires_grad = False
            info = ema_update_(nn.DataParallel(teacher), nn.DataParallel(student), decay)
            assert info["kernel"] == 0 and info["fallback"] == len(list(teacher.parameters()))
            for a, b in zip(teacher.parameters(), want.parameters()):
                assert torch.equal(a, b) and not a.requires_grad
            for a, b in zip(teacher.buffers(), want.buffers()):            # buffers are not parameters: untouched
                assert torch.equal(a, b)
