"""Host-side checks of the update operator's training nodes (no device needed): the six ABI entries refuse bad arguments
before any launch, the TRAIN_NODES handle, and the torch expression sequence that CPU tensors keep taking."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import _synth


def test_entries_refuse_bad_arguments_before_launch():
    from dkt_stereo_amd import _ffi
    lib = _ffi.lib()
    names = ["dkt_gru_gate_zr_train", "dkt_gru_gate_out_train", "dkt_gru_gate_out_bwd", "dkt_gru_gate_zr_bwd",
             "dkt_pool2x_bwd", "dkt_interp_bilinear_bwd"]
    assert set(names) <= set(_ffi.SIGNATURES) and all(hasattr(lib, n) for n in names)
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 256)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    zr, out, obwd, zbwd = (getattr(lib, n) for n in names[:4])
    pool, interp = lib.dkt_pool2x_bwd, lib.dkt_interp_bilinear_bwd
    tail = (1, 2, 4, -1, null)                                       # B, Ch, HW, device = -1, stream
    # dkt_gru_gate_zr_train(azr, cz, bs, cr, bs, h, bs, z, r, rh, bs, ...): every pointer is required
    good = [p, p, 8, p, 8, p, 8, p, p, p, 8]
    for k in (0, 1, 3, 5, 7, 8, 9):
        assert zr(*[null if i == k else a for i, a in enumerate(good)], *tail) == -1, k
    for bad in ((0, 2, 4), (1, 0, 4), (1, 2, 0), (-1, 2, 4)):
        assert zr(*good, *bad, -1, null) == -2, bad
    # dkt_gru_gate_out_train(aq, cq, bs, z, h, bs, q, hout, bs, ...)
    good = [p, p, 8, p, p, 8, p, p, 8]
    for k in (0, 1, 3, 4, 6, 7):
        assert out(*[null if i == k else a for i, a in enumerate(good)], *tail) == -1, k
    assert out(*good, 1, 0, 4, -1, null) == -2
    # dkt_gru_gate_out_bwd(gout, bs, z, q, h, bs, gaq, gz, gh, ...): inputs required, any output may be null, not all
    good = [p, 8, p, p, p, 8, p, p, p]
    for k in (0, 2, 3, 4):
        assert obwd(*[null if i == k else a for i, a in enumerate(good)], *tail) == -1, k
    assert obwd(p, 8, p, p, p, 8, null, null, null, *tail) == -1
    assert obwd(p, 8, p, p, p, 8, null, p, null, 1, 2, 0, -1, null) == -2           # a null output alone is no error
    assert obwd(*good, 0, 2, 4, -1, null) == -2
    # dkt_gru_gate_zr_bwd(gz, grh, bs, z, r, h, bs, gazr, gh, ...)
    good = [p, p, 8, p, p, p, 8, p, p]
    for k in (0, 1, 3, 4, 5):
        assert zbwd(*[null if i == k else a for i, a in enumerate(good)], *tail) == -1, k
    assert zbwd(p, p, 8, p, p, p, 8, null, null, *tail) == -1
    assert zbwd(p, p, 8, p, p, p, 8, null, p, 1, 0, 4, -1, null) == -2
    assert zbwd(*good, 1, 2, -3, -1, null) == -2
    # the resamplers
    assert pool(null, p, 1, 2, 2, -1, null) == -1 and pool(p, null, 1, 2, 2, -1, null) == -1
    for bad in ((0, 2, 2), (1, 0, 2), (1, 2, 0)):
        assert pool(p, p, *bad, -1, null) == -2, bad
    assert pool(p, p, 1, 65536, 65536, -1, null) == -7              # a plane beyond int indices
    assert interp(null, p, 1, 2, 2, 4, 4, -1, null) == -1 and interp(p, null, 1, 2, 2, 4, 4, -1, null) == -1
    for bad in ((0, 2, 2, 4, 4), (1, 0, 2, 4, 4), (1, 2, 0, 4, 4), (1, 2, 2, 0, 4), (1, 2, 2, 4, 0)):
        assert interp(p, p, *bad, -1, null) == -2, bad
    assert interp(p, p, 1, 2, 2, 4, (1 << 22) + 1, -1, null) == -7
    assert all(v == 0.0 for v in buf)                               # nothing was written


def test_train_nodes_handle():
    from dkt_stereo_amd.update import BasicMultiUpdateBlock, BasicMultiUpdateBlockIGEV
    assert BasicMultiUpdateBlock.TRAIN_NODES is True
    assert BasicMultiUpdateBlockIGEV.TRAIN_NODES is True            # inherited
    assert "TRAIN_NODES" not in vars(BasicMultiUpdateBlockIGEV)


def test_nodes_refuse_cpu_tensors():
    """The nodes themselves have no host path: a CPU tensor is an error, not a fallback."""
    from dkt_stereo_amd import _ffi, gru_train
    x = torch.zeros(1, 2, 4, 4)
    with pytest.raises(_ffi.DktError):
        gru_train.pool2x(x)
    with pytest.raises(_ffi.DktError):
        gru_train.gate_out(x, x, x, x)


@pytest.mark.parametrize("igev", [False, True])
def test_cpu_tensors_keep_the_torch_sequence(igev):
    """The update block under autograd on CPU tensors (TRAIN_NODES on): torch nodes only, values and gradients as the
    oracle's, to the tolerances of the GPU test of the same name (1e-5 values, 5e-5 gradients)."""
    from oracle import torch_oracle as to
    from dkt_stereo_amd.update import BasicMultiUpdateBlock, BasicMultiUpdateBlockIGEV
    cfg = dict(corr_levels=2 if igev else 4, corr_radius=4, n_downsample=2, n_gru_layers=3, hidden_dims=[128, 128, 128],
               slow_fast_gru=False)
    blk = (BasicMultiUpdateBlockIGEV if igev else BasicMultiUpdateBlock)(SimpleNamespace(**cfg), hidden_dims=cfg["hidden_dims"])
    sd = _synth.torch_state_dict(_synth.shapes_of(blk), 21)
    blk.load_state_dict(sd)
    H, W = 8, 12
    torch.manual_seed(9)
    net0 = [torch.tanh(torch.randn(1, 128, H >> i, W >> i)) for i in range(3)]
    inp = [[0.5 * torch.randn(1, 128, H >> i, W >> i) for _ in range(3)] for i in range(3)]
    corr0 = torch.randn(1, 162 if igev else 36, H, W)
    aux = torch.randn(1, 1 if igev else 2, H, W)
    net_t = [t.clone().requires_grad_(True) for t in net0]
    corr_t = corr0.clone().requires_grad_(True)
    net, mask, delta = blk(list(net_t), inp, corr_t, **(dict(disp=aux) if igev else dict(flow=aux)))
    loss = sum(n.sum() for n in net) + mask.sum() + delta.sum()
    seen = _graph_names(loss)
    assert {"SigmoidBackward0", "TanhBackward0", "AvgPool2DBackward0", "UpsampleBilinear2DBackward0"} <= seen
    assert not any(n.startswith(("_GateZrFn", "_GateOutFn", "_Pool2xFn", "_InterpFn")) for n in seen)
    got = torch.autograd.grad(loss, net_t + [corr_t])
    sdd = {("ub." + k): v.double() for k, v in sd.items()}
    net_c = [t.double().requires_grad_(True) for t in net0]
    corr_c = corr0.double().requires_grad_(True)
    o_net, o_mask, o_delta = to.update_block(sdd, "ub", 3, list(net_c), [[t.double() for t in s] for s in inp], corr_c,
                                             aux.double(), igev=igev)
    want = torch.autograd.grad(sum(n.sum() for n in o_net) + o_mask.sum() + o_delta.sum(), net_c + [corr_c])
    rel = lambda a, b: float((a.detach().double() - b.detach()).abs().max() / b.detach().abs().max())
    for a, b in zip(list(net) + [mask, delta], list(o_net) + [o_mask, o_delta]):
        assert rel(a, b) <= 1e-5
    for a, b in zip(got, want):
        assert rel(a, b) <= 5e-5


def _graph_names(t):
    seen, todo, names = set(), [t.grad_fn], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        todo.extend(f for f, _ in fn.next_functions)
    return names
