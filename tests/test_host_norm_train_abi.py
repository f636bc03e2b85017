"""Host-side checks of the instance-norm training entries (no device needed): their argument errors before any launch,
the header's declarations against _ffi.SIGNATURES, the nodes' refusal of CPU tensors, and the CPU encoder under autograd,
which stays on torch whatever extractor.TRAIN_NORM_NODES says."""
import ctypes

import pytest
import torch

import _abi_header
import _encoder_ref as er
import _norm_train_ref as R

NAMES = ("dkt_instance_norm_bwd_workspace", "dkt_instance_norm_bwd", "dkt_instance_norm_add_relu_bwd")


def test_entries_refuse_bad_arguments_before_launch():
    from dkt_stereo_amd import _ffi
    lib = _ffi.lib()
    ws, bwd, join = (getattr(lib, n) for n in NAMES)
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert ws(0, 16) == -2 and ws(2, 0) == -2 and ws(-1, 16) == -2
    assert ws(2, 16) == 2 * 1 * 2 * 8                                   # one slice per plane
    assert ws(2, 96 * 97) == 2 * R.split(2, 96 * 97) * 2 * 8 == 2 * 3 * 2 * 8
    assert ws(256, 480 * 896) == 256 * 8 * 2 * 8
    assert ws(1, 1 << 30) == R.SPLIT_MAX * 2 * 8
    good = [p, p, p, 1, p, p, 2, 8, -1, null]
    for i in (0, 1, 2, 4, 5):                                           # gy, x, mean_invstd, gx, workspace
        args = list(good)
        args[i] = null
        assert bwd(*args) == -1, i
    assert bwd(p, p, p, 1, p, p, 0, 8, -1, null) == -2                  # planes = 0
    assert bwd(p, p, p, 0, p, p, 2, 0, -1, null) == -2                  # HW = 0
    assert bwd(p, p, p, 0, p, p, -3, 8, -1, null) == -2
    assert bwd(p, p, p, 1, p, p, 65536, 8, -1, null) == -2              # planes beyond the grid
    assert join(null, p, p, p, p, p, p, 2, 8, -1, null) == -1           # gout
    assert join(p, null, p, p, p, p, p, 2, 8, -1, null) == -1           # out
    assert join(p, p, p, p, null, null, p, 2, 8, -1, null) == -1        # neither gradient wanted
    assert join(p, p, null, p, p, p, p, 2, 8, -1, null) == -1           # gc needs c ...
    assert join(p, p, p, null, p, p, p, 2, 8, -1, null) == -1           # ... the statistics ...
    assert join(p, p, p, p, null, p, null, 2, 8, -1, null) == -1        # ... and the workspace
    assert join(p, p, p, p, p, p, p, 0, 8, -1, null) == -2
    assert join(p, p, p, p, p, p, p, 2, 0, -1, null) == -2
    assert join(p, p, null, null, p, null, null, 2, -1, -1, null) == -2     # (the ga-only form is checked alike)
    assert join(p, p, p, p, p, p, p, 65536, 8, -1, null) == -2
    assert all(v == 0.0 for v in buf)                                   # nothing was written


def test_header_cites_the_reference():
    hdr = _abi_header.raw()
    doc = hdr[:hdr.index("long dkt_instance_norm_bwd_workspace")]
    assert "core/extractor.py:21-33" in doc[-1800:] and "core/extractor.py:52-60" in doc[-1800:]


def test_nodes_refuse_cpu_and_other_dtypes():
    from dkt_stereo_amd import _ffi, norm_train
    x = torch.randn(1, 2, 4, 4, requires_grad=True)
    with pytest.raises(_ffi.DktError):
        norm_train.instance_norm(x, 1e-5, True)
    with pytest.raises(_ffi.DktError):
        norm_train.instance_norm_add_relu(x, x, 1e-5)
    with pytest.raises(_ffi.DktError):
        norm_train.instance_norm(x.double(), 1e-5, False)


@pytest.mark.parametrize("handle", [True, False])
def test_cpu_encoder_under_autograd_stays_on_torch(handle, monkeypatch):
    from dkt_stereo_amd import extractor
    monkeypatch.setattr(extractor, "TRAIN_NORM_NODES", handle)
    fnet = er.make_basic("instance", 2, 128, 7).train()
    x = er.images(3, 2, 37, 53)[0]
    seen = []
    inner_act, inner_join = extractor.norm_act, extractor.norm_add_relu

    def spy_act(norm, t, relu):
        y = inner_act(norm, t, relu)
        seen.append(type(y.grad_fn).__name__)
        return y

    def spy_join(norm, a, c, c_stats=None):
        y = inner_join(norm, a, c, c_stats)
        seen.append(type(y.grad_fn).__name__)
        return y

    monkeypatch.setattr(extractor, "norm_act", spy_act)
    monkeypatch.setattr(extractor, "norm_add_relu", spy_join)
    y = fnet(x)
    assert len(seen) >= 13 and not any(n in ("_InstanceNormFnBackward", "_InstanceNormAddReluFnBackward") for n in seen), seen
    (want,) = er.flatten(er.basic(er.cast_sd(er.prefixed(fnet, "fnet"), torch.float32), x, "instance", 2))
    assert float((y.detach() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    with torch.no_grad():
        assert torch.equal(fnet(x), y.detach())
    (g,) = torch.autograd.grad(y.square().sum(), [fnet.conv1.weight])
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0
