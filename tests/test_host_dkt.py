"""F&E and the sequence losses without a device: the C ABI's argument errors (negative DKT_E_* before any launch), DktError
for CPU tensors (the library has no CPU path), the loss table and the fixture's shape."""
import ctypes
import os

import numpy as np
import pytest
import torch

DKT_OK, DKT_E_NULL, DKT_E_SHAPE, DKT_E_UNSUPPORTED = 0, -1, -2, -7
HERE = os.path.dirname(os.path.abspath(__file__))
FAKE = 0x1000          # a non-null pointer the calls below reject before they could use it


def _job(**kw):
    from dkt_stereo_amd import _ffi
    j = _ffi.FandeJob()
    j.src = j.tgt = j.valid = j.out = j.out_valid = FAKE
    j.tau, j.filter, j.ensemble = 3.0, 1, 1
    for k, v in kw.items():
        setattr(j, k, v)
    return j


def test_fande_argument_errors_before_launch():
    from dkt_stereo_amd import _ffi
    L = _ffi.lib()
    null = ctypes.c_void_p(0)
    ws = ctypes.c_void_p(FAKE)
    one = (_ffi.FandeJob * 1)(_job())
    # dkt_fande(jobs, njobs, B, H, W, ws, device, stream)
    assert L.dkt_fande(None, 1, 1, 4, 4, ws, -1, null) == DKT_E_NULL
    assert L.dkt_fande(one, 1, 1, 4, 4, null, -1, null) == DKT_E_NULL
    for njobs, B, H, W in ((0, 1, 4, 4), (3, 1, 4, 4), (1, 0, 4, 4), (1, 1, 0, 4), (1, 1, 4, -1)):
        assert L.dkt_fande(one, njobs, B, H, W, ws, -1, null) == DKT_E_SHAPE, (njobs, B, H, W)
    assert L.dkt_fande(one, 1, _ffi.FANDE_MAX_B + 1, 4, 4, ws, -1, null) == DKT_E_UNSUPPORTED
    assert L.dkt_fande((_ffi.FandeJob * 1)(_job(filter=3)), 1, 1, 4, 4, ws, -1, null) == DKT_E_UNSUPPORTED
    for field in ("src", "tgt", "out", "out_valid"):
        assert L.dkt_fande((_ffi.FandeJob * 1)(_job(**{field: 0})), 1, 1, 4, 4, ws, -1, null) == DKT_E_NULL, field
    # a null out_valid is fine when nothing is filtered -- checked on the second job of a pair that fails on its filter mode
    two = (_ffi.FandeJob * 2)(_job(filter=0, out_valid=0), _job(filter=-1))
    assert L.dkt_fande(two, 2, 1, 4, 4, ws, -1, null) == DKT_E_UNSUPPORTED


def _desc(**kw):
    from dkt_stereo_amd import _ffi
    d = _ffi.SeqLossDesc()
    d.n, d.n_loss, d.kind, d.ntargets = 3, 3, _ffi.LOSS_RAFT, 2
    for i in range(3):
        d.pred[i] = FAKE
    for k in range(2):
        d.gt[k] = d.valid[k] = d.mask[k] = d.loss[k] = FAKE
    d.rec, d.B, d.H, d.W, d.max_flow = FAKE, 2, 8, 8, 700.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_seq_loss_argument_errors_before_launch():
    from dkt_stereo_amd import _ffi
    L = _ffi.lib()
    null = ctypes.c_void_p(0)
    ws = ctypes.c_void_p(FAKE)
    assert L.dkt_seq_loss(None, ws, -1, null) == DKT_E_NULL
    assert L.dkt_seq_loss(_desc(), null, -1, null) == DKT_E_NULL
    for kw in (dict(n=0), dict(n=_ffi.LOSS_MAX_PRED + 1), dict(n_loss=0), dict(n_loss=4), dict(ntargets=0), dict(ntargets=3),
               dict(B=0), dict(H=0), dict(W=-2)):
        assert L.dkt_seq_loss(_desc(**kw), ws, -1, null) == DKT_E_SHAPE, kw
    assert L.dkt_seq_loss(_desc(kind=2), ws, -1, null) == DKT_E_UNSUPPORTED
    d = _desc()
    d.pred[2] = 0
    assert L.dkt_seq_loss(d, ws, -1, null) == DKT_E_NULL
    for field in ("gt", "valid", "mask", "loss"):
        d = _desc()
        getattr(d, field)[1] = 0
        assert L.dkt_seq_loss(d, ws, -1, null) == DKT_E_NULL, field
    d = _desc(ntargets=1)
    d.gt[1] = 0                         # the second target's pointers are not needed with one target: fails on rec instead
    d.rec = 0
    assert L.dkt_seq_loss(d, ws, -1, null) == DKT_E_NULL
    # the backward: the same checks, then its own table
    g = _ffi.SeqLossGrad()
    assert L.dkt_seq_loss_bwd(_desc(kind=5), g, -1, null) == DKT_E_UNSUPPORTED
    assert L.dkt_seq_loss_bwd(_desc(), None, -1, null) == DKT_E_NULL
    assert L.dkt_seq_loss_bwd(_desc(), g, -1, null) == DKT_E_NULL                    # grad[0] null
    for i in range(3):
        g.grad[i] = FAKE
    assert L.dkt_seq_loss_bwd(_desc(), g, -1, null) == DKT_E_NULL                    # grad_loss null
    # the workspace size: (targets * (n + 5) + 3 flag words) per block of 1024 pixels
    assert L.dkt_seq_loss_ws_doubles(2, 16, 2, 480, 896) == (2 * 21 + 3) * 2 * 420
    assert L.dkt_seq_loss_ws_doubles(1, 1, 1, 1, 1) == 9
    assert L.dkt_seq_loss_ws_doubles(1, _ffi.LOSS_MAX_PRED + 1, 1, 8, 8) == DKT_E_SHAPE
    assert L.dkt_seq_loss_ws_doubles(3, 4, 1, 8, 8) == DKT_E_SHAPE
    assert _ffi.LOSS_MAX_PRED >= 64


def test_cpu_tensors_raise():
    from types import SimpleNamespace
    from dkt_stereo_amd import _ffi
    from dkt_stereo_amd.fande import FandE_Ensemble, FandE_Filter, fande_targets
    from dkt_stereo_amd.loss import dkt_loss_pair, loss_gwcnet, sequence_loss_raft
    d = torch.zeros(2, 1, 4, 6)
    v = torch.ones(2, 1, 4, 6)
    with pytest.raises(_ffi.DktError):
        FandE_Filter(d, d, v, withprob=True)
    with pytest.raises(_ffi.DktError):
        FandE_Ensemble(d, d, v, clamp=1.0)
    with pytest.raises(_ffi.DktError):
        fande_targets(d, v[:, 0], d, d, 3.0, 3.0, False)
    res = {"disp_preds": [d.clone().requires_grad_(True) for _ in range(3)]}
    with pytest.raises(_ffi.DktError):
        sequence_loss_raft(res, d, v[:, 0])
    with pytest.raises(_ffi.DktError):
        loss_gwcnet(res, d, v[:, 0], args=SimpleNamespace(maxdisp=192))
    with pytest.raises(_ffi.DktError):
        dkt_loss_pair("sequence_loss_raft", res, d, v[:, 0], d, v[:, 0])
    with pytest.raises(_ffi.DktError):
        dkt_loss_pair("sequence_loss_pcvnet", res, d, v[:, 0], d, v[:, 0])


def test_losses_table():
    from dkt_stereo_amd.loss import __losses__, loss_gwcnet, sequence_loss_raft
    assert __losses__ == {"sequence_loss_raft": sequence_loss_raft, "loss_gwcnet": loss_gwcnet}


def test_dkt_fixture_is_small_and_complete():
    path = os.path.join(HERE, "golden", "dkt.npz")
    assert os.path.getsize(path) <= 1 << 20
    z = np.load(path)
    cases = {k.rsplit("/", 1)[0] for k in z.files}
    assert sum(c.startswith("fande/filter_") for c in cases) == 12
    assert sum(c.startswith("fande/ensemble_") for c in cases) == 12
    assert sum(c.startswith("fande/fused_") for c in cases) == 3
    assert {"loss/raft_n16_g0.8", "loss/raft_empty", "loss/raft_nan_first", "loss/raft_nan_inf", "loss/gwc_n3"} <= cases
    assert all(z[k].dtype != object for k in z.files)
