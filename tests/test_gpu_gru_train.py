"""The update operator's training nodes (-m gpu): gru_train.gate_zr / gate_out / pool2x / interp and their wiring into
BasicMultiUpdateBlock under autograd (TRAIN_NODES).

Forward: bit-identical to the inference kernels on the same tensors.  Backward: every gradient against the float64 truth of
_gru_ref.py under its bound,

    |got - exact| <= 2 c u mag + 2^-126,  u = 2^-24,

with c mag per output as derived there and the device budgets E_SIGMA / E_T of the sigmoid and tanh;
test_host_gru_ref.py shows that the reference's own fp32 arithmetic meets the same bound with its own budget.  Every
comparison is over all elements.  Each case prints the kernels' worst error in units of u * mag (run with -s)."""
import functools
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _cases
import _gru_ref as R
import _synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 9.0
LAYOUTS = ["dense", "slice", "misaligned"]
NODES = ("_GateZrFnBackward", "_GateOutFnBackward", "_Pool2xFnBackward", "_InterpFnBackward")
TORCH_NODES = ("SigmoidBackward", "TanhBackward", "AvgPool2DBackward", "UpsampleBilinear2DBackward")


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=2)
def _gate_ref(name):
    """Inputs and the float64 truth with the device budget, once per case (the layouts of a case run back to back)."""
    i = R.gate_inputs(R.GATE_CASES[name])
    return i, R.closed_gates(i, R.E_SIGMA, R.E_T)


class Wide:
    """A (B, C, H, W) tensor as a channel slice [2, 2 + C) of a (B, C + 3, H, W) buffer filled with a canary; `misaligned`
    starts the buffer one float past a 16-byte boundary.  `dense`: a plain contiguous tensor."""

    def __init__(self, t, how):
        self.how = how
        if how == "dense":
            self.buf, self.view = None, t.contiguous()
            return
        B, C, H, W = t.shape
        n = B * (C + 3) * H * W
        flat = torch.full((n + 4,), CANARY, device=t.device)
        off = (-flat.data_ptr() // 4) % 4 + (1 if how == "misaligned" else 0)          # floats to the wanted alignment
        self.buf = flat[off:off + n].view(B, C + 3, H, W)
        self.flat, self.C = flat, C
        self.view = self.buf[:, 2:2 + C]
        self.view.copy_(t)
        self.want = flat.clone()
        assert self.buf.data_ptr() % 16 == (4 if how == "misaligned" else 0)

    def untouched(self):
        """Nothing but (possibly) the slice itself has changed since construction."""
        if self.buf is None:
            return True
        now = self.flat.clone()
        keep = torch.ones_like(self.buf, dtype=torch.bool)
        keep[:, 2:2 + self.C] = False
        off = (self.buf.data_ptr() - self.flat.data_ptr()) // 4
        outside = torch.ones_like(self.flat, dtype=torch.bool)
        outside[off:off + keep.numel()] = keep.reshape(-1)
        return bool((now[outside] == self.want[outside]).all())


def _ffi():
    from dkt_stereo_amd import _ffi
    return _ffi


def _worst_line(name, got, truth, cmag, mag, keys):
    line = []
    for k, t in zip(keys, got):
        in_u, of_bound = R.worst(t, truth[k], cmag[k], mag[k])
        line.append("%s %.2f (%.3f)" % (k, in_u, of_bound))
        assert of_bound <= 1.0, (name, k, in_u, of_bound)
    return ", ".join(line)


# ---- gates: forward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", LAYOUTS)
@pytest.mark.parametrize("name", list(R.GATE_CASES))
def test_gate_forward_bits(name, how):
    """The two training entries against dkt_gru_gate_zr / dkt_gru_gate_out on the same tensors: z, rh, h' bit-identical, r
    and q the planes they are made of; strided operands and outputs, canaries untouched."""
    f = _ffi()
    L = f.lib()
    i, (truth, cmag, mag) = _gate_ref(name)
    B, Ch, H, W = i["h"].shape
    HW = H * W
    azr, aq, z_in = G(i["azr"]), G(i["aq"]), G(i["z"])
    cz, cr, cq, h = (Wide(G(i[k]), how) for k in ("cz", "cr", "cq", "h"))
    dev, st = f.device_of(azr), f.stream_of(azr)
    new = lambda: torch.full((B, Ch, H, W), CANARY, device=DEV)
    outs = {k: Wide(new(), how) for k in ("rh_t", "rh_i", "ho_t", "ho_i")}
    z_t, z_i, r, q = new(), new(), new(), new()
    bs = lambda w: w.view.stride(0)
    p = lambda w: w.view.data_ptr()
    f.check(L.dkt_gru_gate_zr_train(azr.data_ptr(), p(cz), bs(cz), p(cr), bs(cr), p(h), bs(h), z_t.data_ptr(), r.data_ptr(),
                                    p(outs["rh_t"]), bs(outs["rh_t"]), B, Ch, HW, dev, st), "dkt_gru_gate_zr_train")
    f.check(L.dkt_gru_gate_zr(azr.data_ptr(), p(cz), bs(cz), p(cr), bs(cr), p(h), bs(h), z_i.data_ptr(),
                              p(outs["rh_i"]), bs(outs["rh_i"]), B, Ch, HW, dev, st), "dkt_gru_gate_zr")
    f.check(L.dkt_gru_gate_out_train(aq.data_ptr(), p(cq), bs(cq), z_in.data_ptr(), p(h), bs(h), q.data_ptr(),
                                     p(outs["ho_t"]), bs(outs["ho_t"]), B, Ch, HW, dev, st), "dkt_gru_gate_out_train")
    f.check(L.dkt_gru_gate_out(aq.data_ptr(), p(cq), bs(cq), z_in.data_ptr(), p(h), bs(h),
                               p(outs["ho_i"]), bs(outs["ho_i"]), B, Ch, HW, dev, st), "dkt_gru_gate_out")
    torch.cuda.synchronize()
    assert R.same(z_t, z_i) and R.same(outs["rh_t"].view, outs["rh_i"].view) and R.same(outs["ho_t"].view, outs["ho_i"].view)
    hv = h.view
    assert R.same(r * hv, outs["rh_t"].view)                                     # r is the plane rh was made of
    assert R.same((1 - z_in) * hv + z_in * q, outs["ho_t"].view)                 # and q the one h' was
    assert all(w.untouched() for w in (cz, cr, cq, h, *outs.values()))
    print("%-8s %-10s " % (name, how) + _worst_line(name, (z_t, outs["rh_t"].view, outs["ho_t"].view), truth, cmag, mag,
                                                    ("z", "rh", "hout")))


# ---- gates: backward ---------------------------------------------------------------------------------------------------
def _planes(i):
    """z, r, q as the training entries write them (dense operands)."""
    f = _ffi()
    L = f.lib()
    B, Ch, H, W = i["h"].shape
    azr, cz, cr, h, aq, cq, zi = (G(i[k]) for k in ("azr", "cz", "cr", "h", "aq", "cq", "z"))
    z, r, rh, q, out = (torch.empty_like(h) for _ in range(5))
    n, dev, st = Ch * H * W, f.device_of(h), f.stream_of(h)
    f.check(L.dkt_gru_gate_zr_train(azr.data_ptr(), cz.data_ptr(), n, cr.data_ptr(), n, h.data_ptr(), n, z.data_ptr(),
                                    r.data_ptr(), rh.data_ptr(), n, B, Ch, H * W, dev, st), "dkt_gru_gate_zr_train")
    f.check(L.dkt_gru_gate_out_train(aq.data_ptr(), cq.data_ptr(), n, zi.data_ptr(), h.data_ptr(), n, q.data_ptr(),
                                     out.data_ptr(), n, B, Ch, H * W, dev, st), "dkt_gru_gate_out_train")
    return z, r, q


def _run_gate_zr(i, how, need=(True, True, True, True)):
    """(z, rh, [gazr, gcz, gcr, gh] with None where not needed, the Wide operands) through the node."""
    from dkt_stereo_amd import gru_train
    azr = G(i["azr"]).requires_grad_(need[0])
    ws = [Wide(G(i[k]), how) for k in ("cz", "cr", "h")]
    cz, cr, h = (w.view.detach().requires_grad_(n) for w, n in zip(ws, need[1:]))
    grh = Wide(G(i["grh"]), how)
    z, rh = gru_train.gate_zr(azr, cz, cr, h)
    assert type(z.grad_fn).__name__ == NODES[0]
    torch.autograd.backward([z, rh], [G(i["gz"]), grh.view])
    return z.detach(), rh.detach(), [azr.grad, cz.grad, cr.grad, h.grad], ws + [grh]


def _run_gate_out(i, how, need=(True, True, True, True)):
    from dkt_stereo_amd import gru_train
    aq, z = G(i["aq"]).requires_grad_(need[0]), G(i["z"]).requires_grad_(need[2])
    ws = [Wide(G(i[k]), how) for k in ("cq", "h")]
    cq, h = (w.view.detach().requires_grad_(n) for w, n in zip(ws, (need[1], need[3])))
    g = Wide(G(i["gout"]), how)
    out = gru_train.gate_out(aq, cq, z, h)
    assert type(out.grad_fn).__name__ == NODES[1]
    out.backward(g.view)
    return out.detach(), [aq.grad, cq.grad, z.grad, h.grad], ws + [g]


@pytest.mark.parametrize("how", LAYOUTS)
@pytest.mark.parametrize("name", list(R.GATE_CASES))
def test_gate_backward(name, how):
    """Every gradient of both nodes under the bound, the gradients of cz, cr, cq the halves of gazr and gaq, operands and
    upstream gradients dense, batch-strided and misaligned; a second run bit-identical."""
    i, (truth, cmag, mag) = _gate_ref(name)
    Ch = i["h"].shape[1]
    z, rh, (gazr, gcz, gcr, gh), ws = _run_gate_zr(i, how)
    assert R.same(gcz, gazr[:, :Ch]) and R.same(gcr, gazr[:, Ch:])
    line = _worst_line(name, (z, rh, gazr, gh), truth, cmag, mag, ("z", "rh", "gazr", "gh_zr"))
    out, (gaq, gcq, gz, gh2), ws2 = _run_gate_out(i, how)
    assert R.same(gcq, gaq)
    line += ", " + _worst_line(name, (out, gaq, gz, gh2), truth, cmag, mag, ("hout", "gaq", "gz", "gh_out"))
    assert all(w.untouched() for w in ws + ws2)
    print("%-8s %-10s " % (name, how) + line)
    again = _run_gate_zr(i, how)[2] + _run_gate_out(i, how)[1]
    assert all(R.same(a, b) for a, b in zip([gazr, gcz, gcr, gh, gaq, gcq, gz, gh2], again))
    if R.GATE_CASES[name]["scale"] == "sat":
        # exact gates give exact zeros, and nothing overflows
        zc, r, q = (t.cpu() for t in _planes(i))
        assert all(bool(torch.isfinite(t).all()) for t in (gazr, gh, gaq, gz, gh2))
        edge_z, edge_r = (zc == 0) | (zc == 1), (r == 0) | (r == 1)
        assert bool(edge_z.any()) and bool(edge_r.any())
        assert bool((gazr[:, :Ch].cpu()[edge_z] == 0).all()) and bool((gazr[:, Ch:].cpu()[edge_r] == 0).all())
        zi = torch.from_numpy(i["z"])
        assert bool((q.abs() == 1).any()) and bool((zi == 0).any()) and bool((zi == 1).any())
        assert bool((gaq.cpu()[(q.abs() == 1) | (zi == 0)] == 0).all())
        assert bool((gh2.cpu()[zi == 1] == 0).all())


SUBSETS = [s for s in itertools.product([False, True], repeat=4) if any(s) and not all(s)]


@pytest.mark.parametrize("name,how", [("odd_s4", "dense"), ("mid_s4", "slice")])
def test_gate_needs_input_grad_subsets(name, how):
    """Each of the 14 proper subsets of the four inputs of either node: the wanted gradients are bit-identical to the ones
    computed beside all the others (which test_gate_backward holds to the bound), the others are None."""
    i, _ = _gate_ref(name)
    full_zr, full_out = _run_gate_zr(i, how)[2], _run_gate_out(i, how)[1]
    for need in SUBSETS:
        for got, full in ((_run_gate_zr(i, how, need)[2], full_zr), (_run_gate_out(i, how, need)[1], full_out)):
            for n, a, b in zip(need, got, full):
                assert (a is None) == (not n), need
                assert a is None or R.same(a, b), need


# ---- resamplers --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", R.POOL_CASES)
def test_pool2x_node(hw):
    from dkt_stereo_amd import gru_train, update
    H, W = hw
    x, gy = R.pool_inputs(H, W)
    a = G(x).requires_grad_(True)
    y = gru_train.pool2x(a)
    assert type(y.grad_fn).__name__ == NODES[2]
    with torch.no_grad():
        assert R.same(y, update.pool2x(G(x)))
    y.backward(G(gy))
    gx, cmag, mag = R.closed_pool(gy, H, W)
    in_u, of_bound = R.worst(a.grad, gx, cmag, mag)
    print("pool2x %s: %.2f u*mag (%.3f of the bound)" % (hw, in_u, of_bound))
    assert of_bound <= 1.0
    b = G(x).requires_grad_(True)
    gru_train.pool2x(b).backward(G(gy))
    assert R.same(a.grad, b.grad)


@pytest.mark.parametrize("case", R.INTERP_CASES)
def test_interp_node(case):
    from dkt_stereo_amd import gru_train, update
    H, W, Ho, Wo, planes = case
    x, gy = R.interp_inputs(H, W, Ho, Wo, planes)
    a = G(x).requires_grad_(True)
    y = gru_train.interp(a, (Ho, Wo))
    assert type(y.grad_fn).__name__ == NODES[3]
    with torch.no_grad():
        assert R.same(y, update.interp(G(x), torch.empty(1, 1, Ho, Wo)))
    y.backward(G(gy))
    gx, cmag, mag = R.closed_interp(gy, H, W)
    in_u, of_bound = R.worst(a.grad, gx, cmag, mag)
    print("interp %s: %.2f u*mag (%.3f of the bound)" % (case, in_u, of_bound))
    assert of_bound <= 1.0
    b = G(x).requires_grad_(True)                                                # determinism: a second run, the same bits
    gru_train.interp(b, (Ho, Wo)).backward(G(gy))
    assert R.same(a.grad, b.grad)


def test_resamplers_take_non_contiguous_upstream():
    """A transposed-storage upstream gradient and a batch of planes (N > 1) give the contiguous result."""
    from dkt_stereo_amd import gru_train
    x = torch.randn(2, 3, 7, 10, device=DEV)
    for fn, shape in ((gru_train.pool2x, (2, 3, 4, 5)), (lambda t: gru_train.interp(t, (13, 17)), (2, 3, 13, 17))):
        g = torch.randn(shape, device=DEV)
        a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        fn(a).backward(g)
        fn(b).backward(g.transpose(2, 3).contiguous().transpose(2, 3))
        assert R.same(a.grad, b.grad)


# ---- the whole operator ------------------------------------------------------------------------------------------------
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


def _block(igev):
    from dkt_stereo_amd.update import BasicMultiUpdateBlock, BasicMultiUpdateBlockIGEV
    cfg = dict(corr_levels=2 if igev else 4, corr_radius=4, n_downsample=2, n_gru_layers=3, hidden_dims=[128, 128, 128],
               slow_fast_gru=False)
    blk = (BasicMultiUpdateBlockIGEV if igev else BasicMultiUpdateBlock)(SimpleNamespace(**cfg), hidden_dims=cfg["hidden_dims"])
    sd = _synth.torch_state_dict(_synth.shapes_of(blk), 21)
    blk.load_state_dict(sd)
    return blk.to(DEV), sd


def _block_inputs(igev, H=16, W=24):
    torch.manual_seed(8)
    net0 = [torch.tanh(torch.randn(1, 128, H >> i, W >> i)) for i in range(3)]
    inp = [[0.5 * torch.randn(1, 128, H >> i, W >> i) for _ in range(3)] for i in range(3)]
    corr0 = torch.randn(1, 162 if igev else 36, H, W)
    aux = torch.randn(1, 1 if igev else 2, H, W)
    wts = [torch.randn(1, 128, H >> i, W >> i) for i in range(3)]
    wd = torch.randn(1, 1 if igev else 2, H, W)
    wm = torch.randn(1, 32 if igev else 144, H, W)
    return net0, inp, corr0, aux, wts, wd, wm


@pytest.fixture
def train_nodes():
    """Sets BasicMultiUpdateBlock.TRAIN_NODES for a test and restores it."""
    from dkt_stereo_amd.update import BasicMultiUpdateBlock
    before = BasicMultiUpdateBlock.TRAIN_NODES

    def put(v):
        BasicMultiUpdateBlock.TRAIN_NODES = v
    yield put
    BasicMultiUpdateBlock.TRAIN_NODES = before


@pytest.mark.parametrize("nodes", [True, False])
@pytest.mark.parametrize("igev", [False, True])
def test_wiring_and_oracle(igev, nodes, train_nodes):
    """BasicMultiUpdateBlock(...) under autograd at 16 x 24, three layers: with TRAIN_NODES the graph holds the four nodes
    and none of torch's sigmoid / tanh / pooling / bilinear backward nodes, without it the reverse; both match the float64
    oracle to the tolerances of test_update_block_autograd_matches_oracle (1e-5 values, 5e-5 gradients)."""
    from oracle import torch_oracle as to
    train_nodes(nodes)
    blk, sd = _block(igev)
    net0, inp, corr0, aux, wts, wd, wm = _block_inputs(igev)
    names = ["encoder.convc1.weight", ("gru04" if igev else "gru08") + ".convz.weight",
             ("gru08" if igev else "gru16") + ".convq.weight", ("gru16" if igev else "gru32") + ".convr.bias"]

    def loss_of(net, mask, delta, dev):
        t = lambda a: a.to(dev)
        return sum((n * t(w)).sum() for n, w in zip(net, wts)) + (delta * t(wd)).sum() + (mask * t(wm)).sum()

    net_g = [t.to(DEV).requires_grad_(True) for t in net0]
    corr_g = corr0.to(DEV).requires_grad_(True)
    kw = dict(disp=aux.to(DEV)) if igev else dict(flow=aux.to(DEV))
    net, mask, delta = blk(list(net_g), [[t.to(DEV) for t in s] for s in inp], corr_g, **kw)
    loss = loss_of(net, mask, delta, DEV)
    seen = _graph_names(loss)
    ours = {n for n in seen if n.startswith(NODES)}
    theirs = {n for n in seen if n.startswith(TORCH_NODES)}
    if nodes:
        assert {n.rstrip("0123456789") for n in ours} == set(NODES) and not theirs, (ours, theirs)
    else:
        assert {n.rstrip("0123456789") for n in theirs} == set(TORCH_NODES) and not ours, (ours, theirs)
    params = dict(blk.named_parameters())
    got = torch.autograd.grad(loss, net_g + [corr_g] + [params[n] for n in names])
    sdd = {("ub." + k): v.double().requires_grad_(True) for k, v in sd.items()}
    net_c = [t.double().requires_grad_(True) for t in net0]
    corr_c = corr0.double().requires_grad_(True)
    o_net, o_mask, o_delta = to.update_block(sdd, "ub", 3, list(net_c), [[t.double() for t in s] for s in inp], corr_c,
                                             aux.double(), igev=igev)
    want = torch.autograd.grad(loss_of(o_net, o_mask, o_delta, "cpu"), net_c + [corr_c] + [sdd["ub." + n] for n in names])
    rel = lambda a, b: float((a.detach().double().cpu() - b.detach()).abs().max() / b.detach().abs().max())
    for a, b in zip(list(net) + [mask, delta], list(o_net) + [o_mask, o_delta]):
        assert rel(a, b) <= 1e-5
    for name, a, b in zip(["net0", "net1", "net2", "corr"] + names, got, want):
        assert rel(a, b) <= 5e-5, (name, rel(a, b))


def test_stack_backward_is_deterministic():
    """Two runs of the whole _stack_autograd backward: the gradients of the hidden states and the correlation features are
    bit-identical (the weight gradients are the vendor library's and are not compared)."""
    blk, _ = _block(False)
    net0, inp, corr0, aux, wts, _, _ = _block_inputs(False)
    inp = [[t.to(DEV) for t in s] for s in inp]

    def run():
        net_g = [t.to(DEV).requires_grad_(True) for t in net0]
        corr_g = corr0.to(DEV).requires_grad_(True)
        net = blk._stack_autograd(net_g, inp, (blk.gru08, blk.gru16, blk.gru32), aux.to(DEV), corr_g, (True, True, True))
        assert set(NODES) <= {n.rstrip("0123456789") for n in _graph_names(sum(n.sum() for n in net))}
        return torch.autograd.grad(sum((n * w.to(DEV)).sum() for n, w in zip(net, wts)), net_g + [corr_g])

    first, second = run(), run()
    assert all(R.same(a, b) for a, b in zip(first, second))
    assert all(float(a.abs().max()) > 0 for a in first)


def test_raft_training_step_through_the_nodes():
    """RAFTStereo.forward(test_mode=False), 2 iterations at 64 x 128: finite predictions, the last within 1e-4 of the
    test_mode result, and backward() fills every trainable update-block parameter's .grad with finite values.  (The
    encoders are frozen: their trainable layers go layer by layer through torch.)"""
    from dkt_stereo_amd.raft_stereo import RAFTStereo, make_args
    model = RAFTStereo(make_args())
    model.load_state_dict(_synth.torch_state_dict(_synth.shapes_of(model), _cases.E2E_WEIGHT_SEED), strict=True)
    model.to(DEV).eval()
    for n, p in model.named_parameters():
        if n.startswith(("fnet.", "cnet.")):
            p.requires_grad_(False)
    i1, i2 = (G(a) for a in _synth.image_pair(5, 1, 64, 128, 12))
    with torch.no_grad():
        _, want = model(i1, i2, iters=2, test_mode=True)
    preds = model(i1, i2, iters=2, test_mode=False)["disp_preds"]
    assert len(preds) == 2 and all(bool(torch.isfinite(p).all()) for p in preds)
    assert float((preds[-1].detach() - want).abs().max()) <= 1e-4
    assert set(NODES) <= {n.rstrip("0123456789") for n in _graph_names(preds[-1])}
    sum(p.sum() for p in preds).backward()
    ub = [(n, p) for n, p in model.named_parameters() if n.startswith("update_block.") and p.requires_grad]
    assert len(ub) > 20
    for n, p in ub:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
