"""Host-side checks of the mixture-update entries and their Python front (no device needed): the two symbols, the header's
declarations against _ffi.SIGNATURES, every argument error before any device call, the Python refusals, the CPU path, and
the state-dict keys of ParametersUpdater against a reference-shaped module."""
import ctypes
import types

import pytest
import torch
import torch.nn as nn

import _abi_header as H
import _pcv_update_ref as R

NAMES = ("dkt_pcv_update_fwd", "dkt_pcv_update_bwd")
E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -7


def test_header_declares_what_ffi_mirrors():
    from dkt_stereo_amd import _ffi
    declared = H.functions()
    lib = _ffi.lib()
    for n in NAMES:
        restype, argtypes = declared[n]
        assert restype is ctypes.c_int and n not in _ffi.RESTYPES
        assert _ffi.SIGNATURES[n] == argtypes, n
        assert hasattr(lib, n)
    # fwd: four inputs, three results, disp, code; bwd: four inputs, code, four upstream gradients, four results;
    # then N, M, H, W, five constants, device, stream
    assert len(_ffi.SIGNATURES["dkt_pcv_update_fwd"]) == 9 + 4 + 5 + 2
    assert len(_ffi.SIGNATURES["dkt_pcv_update_bwd"]) == 13 + 4 + 5 + 2
    assert not [n for n in declared if n.startswith("dkt_pcv_update") and ("ws" in n or "workspace" in n)]


def test_entries_refuse_bad_arguments_before_any_device_call():
    from dkt_stereo_amd import _ffi
    lib = _ffi.lib()
    fwd, bwd = (getattr(lib, n) for n in NAMES)
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    consts = (0.5, 1e-3, 1.0, 1.0, 1.0)

    # fwd(delta, mu, sigma, w, mu_out, w_out, sigma_out, disp, code, N, M, H, W, consts, device, stream)
    def FW(ptrs=(p,) * 9, dims=(1, 2, 1, 2)):
        return fwd(*ptrs, *dims, *consts, -1, null)
    for i in range(7):                                                          # the four inputs and the three results
        assert FW(ptrs=tuple(null if j == i else p for j in range(9))) == E_NULL, i
    for dims in ((0, 2, 1, 2), (1, 0, 1, 2), (1, 2, -1, 2), (1, 2, 1, 0)):
        assert FW(dims=dims) == E_SHAPE, dims
        assert FW(ptrs=(null,) * 9, dims=dims) == E_NULL                        # a null pointer is reported first
    for dims in ((1, 9, 1, 2), (65536, 2, 1, 2), (1, 2, 46341, 46341)):
        assert FW(dims=dims) == E_UNSUPPORTED, dims

    # bwd(delta, mu, sigma, w, code, gmu_out, gw_out, gsigma_out, gdisp, gdelta, gmu, gsigma, gw, N, M, H, W, consts, ...)
    def BW(ptrs=(p,) * 13, dims=(1, 2, 1, 2)):
        return bwd(*ptrs, *dims, *consts, -1, null)
    for i in range(5):                                                          # the four inputs and the decision bytes
        assert BW(ptrs=tuple(null if j == i else p for j in range(13))) == E_NULL, i
    assert BW(ptrs=(p,) * 5 + (null,) * 4 + (p,) * 4) == E_NULL                 # no upstream gradient at all
    assert BW(ptrs=(p,) * 9 + (null,) * 4) == E_NULL                            # no result asked for
    for dims in ((0, 2, 1, 2), (1, 0, 1, 2), (1, 2, -1, 2), (1, 2, 1, 0)):
        assert BW(dims=dims) == E_SHAPE, dims
    for dims in ((1, 9, 1, 2), (65536, 2, 1, 2), (1, 2, 46341, 46341)):
        assert BW(dims=dims) == E_UNSUPPORTED, dims
    # every single upstream gradient and every single result is a valid request: the refusal above is "not all four" only
    for i in range(5, 13):
        keep = tuple(p if (j < 5 or j == i or (i < 9) != (j < 9)) else null for j in range(13))
        assert BW(ptrs=keep, dims=(0, 2, 1, 2)) == E_SHAPE, i                  # past the null checks, stopped at the shape


def test_python_refusals():
    from dkt_stereo_amd import _ffi
    from dkt_stereo_amd.pcvnet_update import mixture_upsample, parameters_update
    z = torch.zeros(1, 2, 3, 4)
    with pytest.raises(_ffi.DktError):
        parameters_update(z, z, z, torch.zeros(1, 2, 3, 5))
    with pytest.raises(_ffi.DktError):
        parameters_update(z[0], z[0], z[0], z[0])
    nine = torch.zeros(1, 9, 3, 4)
    with pytest.raises(_ffi.DktError):
        parameters_update(nine, nine, nine, nine)
    with pytest.raises(_ffi.DktError):
        parameters_update(z, z, z, z, gammas=(1, 1))
    for factor in (3, 6, 0, -2):
        with pytest.raises(_ffi.DktError):
            mixture_upsample(z[:, :1], z, z, z, torch.zeros(1, 9 * factor * factor, 3, 4), factor)
    with pytest.raises(_ffi.DktError):                                          # the up-sampling node itself has no CPU path
        mixture_upsample(z[:, :1], z, z, z, torch.zeros(1, 36, 3, 4), 2)


@pytest.mark.parametrize("name", ("base", "m3"))
def test_cpu_tensors_take_the_restatement(name):
    from dkt_stereo_amd.pcvnet_update import parameters_update
    a = R.reference(name)["a"]
    ins = [torch.from_numpy(a[k]).requires_grad_(True) for k in ("delta", "mu", "sigma", "w")]
    got = parameters_update(*ins)
    want = R.restated(*[t.detach() for t in ins])
    assert len(got) == 4 and all(torch.equal(g, w) for g, w in zip(got, want))
    assert parameters_update(*ins, regress=False)[3] is None
    sum(g.sum() for g in got).backward()
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in ins)
    damped = parameters_update(*ins, gammas=(0.25, 0.5, 0.25), sigma0=0.75)
    want = R.restated(*[t.detach() for t in ins], sigma0=0.75, gammas=(0.25, 0.5, 0.25))
    assert all(torch.equal(g, w) for g, w in zip(damped, want))


def test_module_has_the_references_keys_and_signature():
    """State-dict keys against a module built as meta_arch/pcvnet/update.py:76-86 builds it (FlowHead: conv1, conv2, a
    parameterless ReLU), the constants as attributes read per call, and forward's two forms on the CPU."""
    from dkt_stereo_amd.pcvnet_update import ParametersUpdater

    class Head(nn.Module):
        def __init__(self, i, h, o):
            super().__init__()
            self.conv1, self.conv2, self.relu = nn.Conv2d(i, h, 3, padding=1), nn.Conv2d(h, o, 3, padding=1), nn.ReLU(inplace=True)

    class Shaped(nn.Module):
        def __init__(self, args, i, h):
            super().__init__()
            self.head = Head(i, h, args.gauss_num)

    args = types.SimpleNamespace(gauss_num=4)
    m = ParametersUpdater(args, 8, 8)
    want = Shaped(args, 8, 8).state_dict()
    assert list(m.state_dict()) == list(want) == ["head.conv1.weight", "head.conv1.bias", "head.conv2.weight", "head.conv2.bias"]
    assert all(m.state_dict()[k].shape == v.shape for k, v in want.items())
    assert (m.sigma0, m.eps, m.gamma1, m.gamma2, m.gamma3) == (0.5, 1e-3, 1, 1, 1) and m.args is args
    a = R.reference("base")["a"]
    hidden = torch.from_numpy(R._synth.normal((1, 8, 6, 10), 1, "hidden"))
    st = [torch.from_numpy(a[k]) for k in ("mu", "sigma", "w")]
    with torch.no_grad():
        three = m(hidden, *st)
        four = m(hidden, *st, regress=True)
        delta = m.head.conv2(torch.relu(m.head.conv1(hidden)))
        want = R.restated(delta, *st)
        assert len(three) == 3 and len(four) == 4
        assert all(torch.equal(x, y) for x, y in zip(four, want)) and all(torch.equal(x, y) for x, y in zip(three, want))
        m.gamma1 = 0.5                                                          # read per call
        assert not torch.equal(m(hidden, *st)[2], three[2])
