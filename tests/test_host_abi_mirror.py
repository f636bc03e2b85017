"""The whole of _ffi against include/dktstereo.h (no device needed, but for the two cases marked gpu): every entry's argtypes
and restype, every ctypes.Structure, every mirrored constant, under the one rule _abi_header.py states -- no entry is left
out, and the only exceptions are _abi_header.DEVICE_TABLES.  Then _ffi.call and _ffi.size, the two helpers every native
call of the package goes through, on calls the library refuses before any device work."""
import ctypes
import inspect
import re

import pytest
import torch

import _abi_header as H
from dkt_stereo_amd import _ffi

UNLISTED = {"dkt_version", "dkt_strerror"}          # bound by _ffi.lib() itself, not through SIGNATURES


def test_header_was_read():
    """A parser that silently finds nothing would let everything below pass."""
    assert len(H.functions()) >= 110 + len(UNLISTED) and len(H.structs()) >= 11
    assert H.defines()["DKT_ABI_VERSION"] == 1 and H.defines()["DKT_E_NULL"] == -1


def test_abi_exports_every_declared_symbol():
    lib = _ffi.lib()
    for n in H.functions():
        assert hasattr(lib, n), n
    assert set(_ffi.SIGNATURES) | UNLISTED == set(H.functions())
    assert lib.dkt_version() == 1
    assert lib.dkt_strerror(0) == b"ok"
    assert b"null" in lib.dkt_strerror(-1)


def test_every_signature_matches_the_header():
    lib = _ffi.lib()
    declared = H.functions()
    for name, argtypes in _ffi.SIGNATURES.items():
        restype, want = declared[name]
        assert argtypes == want, name
        assert _ffi.RESTYPES.get(name, ctypes.c_int) is restype, name
    assert set(_ffi.RESTYPES) == {n for n in _ffi.SIGNATURES if declared[n][0] is not ctypes.c_int}
    for name in UNLISTED:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == declared[name], name
    assert set(H.DEVICE_TABLES) <= {(n, i) for n, (_, a) in declared.items() for i in range(len(a))}


def test_every_struct_has_its_mirror():
    declared, mirrors = H.structs(), H.mirrors()
    assert set(mirrors) == set(declared)
    for name, cls in mirrors.items():
        assert H.mirror_fields(cls) == declared[name], name


def test_mirrored_constants_equal_the_header():
    """Every `#: DKT_X[, DKT_Y ...] of include/dktstereo.h` line of _ffi.py against the assignment under it."""
    found = re.findall(r"^#: (DKT_\w+(?:, DKT_\w+)*) of include/dktstereo\.h\n(\w+(?:, \w+)*) = ", inspect.getsource(_ffi), flags=re.M)
    pairs = [(c, p) for cs, ps in found for c, p in zip(cs.split(", "), ps.split(", "))]
    assert all(len(cs.split(", ")) == len(ps.split(", ")) for cs, ps in found)
    assert {p for _, p in pairs} >= {"STATUS_MAX_JOBS", "FANDE_MAX_B", "FANDE_MAX_JOBS", "FANDE_WS_DOUBLES_PER_IMAGE", "LOSS_MAX_PRED",
                                     "LOSS_RAFT", "LOSS_GWC", "LOSS_REC", "NS_MAX_PRED", "NS_REC", "E_UNSUPPORTED"}
    for c, p in pairs:
        assert getattr(_ffi, p) == H.defines()[c], (c, p)


def test_size_returns_an_int_and_raises_the_library_s_error():
    with _ffi.launch_log() as names:
        n = _ffi.size("dkt_conv_grad_prepass_ws_floats", 2, 3, 5000)
        with pytest.raises(_ffi.DktError) as e:
            _ffi.size("dkt_conv_grad_prepass_ws_floats", 0, 1, 1)
    assert n == 24 and type(n) is int                   # (the value: test_host_conv_grad_abi.py)
    assert "dkt_conv_grad_prepass_ws_floats" in str(e.value) and _ffi.lib().dkt_strerror(-2).decode() in str(e.value)
    assert names == []                                  # a size query is no launch


@pytest.mark.gpu
def test_call_raises_on_an_unlisted_code_and_logs_nothing():
    t = torch.zeros(1, device="cuda")
    with _ffi.launch_log() as names:
        with pytest.raises(_ffi.DktError) as e:
            _ffi.call("dkt_pool_w", t, None, None, 1, 4)
        with pytest.raises(_ffi.DktError):
            _ffi.call("dkt_pool_w", t, None, None, 1, 4, ok=(_ffi.E_UNSUPPORTED,), log="other")
    assert str(e.value) == "dkt_pool_w failed: %s (rc=-1)" % _ffi.lib().dkt_strerror(-1).decode()
    assert names == []


@pytest.mark.gpu
def test_call_returns_a_code_listed_in_ok_and_logs_nothing():
    t = torch.zeros(64, device="cuda")
    p = t.data_ptr()
    with _ffi.launch_log() as names:
        # one group's target row > 160 KB of LDS: refused before any device work (test_layout.py has it with device -1)
        rc = _ffi.call("dkt_gwc_volume", t, p, p, p, 1, 8192, 1, 16, 2, 1, 32, ok=(_ffi.E_UNSUPPORTED,))
        with pytest.raises(_ffi.DktError):
            _ffi.call("dkt_gwc_volume", t, p, p, p, 1, 8192, 1, 16, 2, 1, 32)
    assert rc == _ffi.E_UNSUPPORTED == -7 and names == []
