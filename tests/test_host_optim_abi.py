"""dkt_adamw_step / dkt_adamw_workspace and optim.AdamW without a device: the symbols, the header's declarations against
_ffi.SIGNATURES, the argument errors (negative DKT_E_* before any device call), the workspace size, and the refusal of
parameters the kernel cannot take."""
import ctypes
import math

import pytest
import torch

DKT_OK, DKT_E_NULL, DKT_E_SHAPE, DKT_E_UNSUPPORTED = 0, -1, -2, -7


def _call(lib, **kw):
    """dkt_adamw_step with valid host-side arguments except those given (tables are never dereferenced on the host)."""
    buf = (ctypes.c_long * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    a = dict(p=p, g=p, m=p, v=p, n=p, count=2, total=8, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2, max_norm=1.0,
             inv_scale=1.0, grad_scale=null, found_inf=null, step=p, record=p, absmax=null, workspace=p, grid=0)
    a.update(kw)
    return lib.dkt_adamw_step(a["p"], a["g"], a["m"], a["v"], a["n"], a["count"], a["total"], a["lr"], a["beta1"], a["beta2"],
                              a["eps"], a["wd"], a["max_norm"], a["inv_scale"], a["grad_scale"], a["found_inf"], a["step"],
                              a["record"], a["absmax"], a["workspace"], a["grid"], -1, null)


def test_argument_errors_before_launch():
    from dkt_stereo_amd import _ffi
    lib = _ffi.lib()
    null = ctypes.c_void_p(0)
    assert _call(lib, count=-1) == DKT_E_SHAPE
    assert _call(lib, total=-1) == DKT_E_SHAPE
    for table in ("p", "g", "m", "v", "n", "step", "record", "workspace"):
        assert _call(lib, **{table: null}) == DKT_E_NULL, table
    for name in ("lr", "beta1", "beta2", "eps", "wd", "inv_scale"):
        for bad in (math.nan, math.inf):
            assert _call(lib, **{name: bad}) == DKT_E_UNSUPPORTED, (name, bad)
    assert _call(lib, max_norm=math.nan) == DKT_E_UNSUPPORTED
    assert _call(lib, max_norm=math.inf, p=null) == DKT_E_NULL        # +inf is clip_grad_norm_'s "report the norm only": taken
    for name in ("lr", "eps", "wd", "beta1", "beta2"):
        assert _call(lib, **{name: -1e-3}) == DKT_E_UNSUPPORTED, name
    assert _call(lib, beta1=1.0) == DKT_E_UNSUPPORTED
    assert _call(lib, beta2=1.0) == DKT_E_UNSUPPORTED
    assert _call(lib, count=0, p=null, g=null, m=null, v=null, n=null, step=null, record=null, workspace=null) == DKT_OK
    assert _call(lib, count=0, lr=math.nan) == DKT_E_UNSUPPORTED          # (hyper-parameters are checked first)


@pytest.mark.parametrize("count,total", [(0, 0), (1, 1), (3, 2048), (3, 2049), (218, 11116130), (10, 2 ** 31 + 5)])
def test_workspace_size(count, total):
    """64 bytes of flags, then one double per tile of 2048 elements of the flat range."""
    from dkt_stereo_amd import _ffi, optim
    want = 64 + 8 * ((total + 2047) // 2048)
    assert _ffi.lib().dkt_adamw_workspace(count, total) == want
    assert optim.workspace_bytes(count, total) == want


def test_workspace_refuses_negative():
    from dkt_stereo_amd import _ffi
    lib = _ffi.lib()
    assert lib.dkt_adamw_workspace(-1, 4) < 0 and lib.dkt_adamw_workspace(1, -4) < 0


def test_cpu_parameters_are_refused():
    from dkt_stereo_amd import _ffi, optim
    with pytest.raises(_ffi.DktError):
        optim.AdamW([torch.nn.Parameter(torch.zeros(4))], lr=1e-3)
    with pytest.raises(_ffi.DktError):
        optim.AdamW(torch.nn.Linear(3, 2).parameters())


def test_supports_amp_scaling():
    from dkt_stereo_amd import optim
    assert optim.AdamW._step_supports_amp_scaling is True
    assert issubclass(optim.AdamW, torch.optim.Optimizer)
