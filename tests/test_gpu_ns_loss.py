"""ns_loss.hip on the device against the float64 truth of _ns_loss_ref.py: the per-pixel planes inside their bounds, the
decisions by the decision rule, loss and gradients against truth(decisions=the device's), the reference's exceptions and
NaNs, in-place reads of views, bit-identical repeats, the sum of the parts, the memory the node takes and its one host read."""
import math
import warnings

import pytest
import torch

import _ns_loss_ref as R
from dkt_stereo_amd import _ffi, ns_loss as N

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = sorted(R.CASES)
PHOTO = [n for n in NAMES if R.params(R.CASES[n])["alpha_photometric"] != 0.0]
UP = 1.7


def on_device(name, n=None):
    """(args of ns_loss on the device, the leaves whose .grad the backward fills)."""
    c = R.CASES[name]
    a = {k: torch.from_numpy(v).to(DEV) for k, v in R.inputs(c).items()}
    leaves, preds = [], []
    for p in a["preds"][:n]:
        if c.get("views"):
            two = torch.stack([p[:, 0], p[:, 0] + 100.0], 1).requires_grad_(True)      # (B, 2, H, W); the loss reads [:, :1]
            leaves.append(two)
            preds.append(two[:, :1])
        else:
            leaves.append(p.clone().requires_grad_(True))
            preds.append(leaves[-1])
    return (preds, a["target"], a["conf"], a["im0"], a["im1"], a["im2"]), leaves


def run_device(name):
    args, leaves = on_device(name)
    loss, metrics, valid, am, third = N.ns_loss_decisions(*args, **R.params(R.CASES[name]))
    (UP * loss).backward()
    grads = [(l.grad[:, :1] if R.CASES[name].get("views") else l.grad).cpu() for l in leaves]
    return dict(loss=float(loss), metrics=metrics, valid=valid.cpu(), automask=None if am is None else am.cpu(),
                third=None if third is None else third.cpu(), grads=grads, leaves=leaves)


@pytest.mark.parametrize("name", PHOTO)
def test_planes_inside_bounds(name):
    a = {k: torch.from_numpy(v).to(DEV) for k, v in R.inputs(R.CASES[name]).items()}
    got = dict(zip(("p12", "p23", "loss_2"), N.photometric_planes(a["preds"][0], a["im0"], a["im1"], a["im2"])))
    t, b = R.reference(name)["truth"]["per"][0], R.plane_bounds(name, 0)
    for k, v in got.items():
        w = R.worst(v, t[k], b[k])
        print("%s %s: worst err / bound %.3f" % (name, k, w))
        assert w <= 1.0, k


@pytest.mark.parametrize("name", NAMES)
def test_loss_and_gradients_under_the_device_decisions(name):
    d = run_device(name)
    ref = R.reference(name)
    assert torch.equal(d["valid"], ref["truth"]["valid"])
    dec = None
    if d["automask"] is not None:
        dec = []
        for i in range(R.CASES[name]["n"]):
            md, t = R.may_differ(name, i), ref["truth"]["per"][i]
            for k in ("automask", "third"):
                diff = d[k][i] != t[k]
                assert not bool((diff & ~md[k]).any()), (i, k, int((diff & ~md[k]).sum()))
                assert float(md[k].double().mean()) <= R.MAY_DIFFER
            dec.append(dict(automask=d["automask"][i], third=d["third"][i]))
    t = R.run(name, torch.float64, decisions=dec)
    y = R.run(name, torch.float32, decisions=dec)
    if math.isnan(t["loss"]):
        assert math.isnan(d["loss"])
    else:
        lb = R.loss_bound(y["loss"], t["loss"])
        print("%s loss: err / bound %.3f" % (name, abs(d["loss"] - t["loss"]) / lb))
        assert abs(d["loss"] - t["loss"]) <= lb
    for i, (g, gy, gt) in enumerate(zip(d["grads"], y["grads"], t["grads"])):
        w = R.worst(g, gt, R.grad_bound(gy, gt))
        print("%s grad %d: worst err / bound %.3f" % (name, i, w))
        assert w <= 1.0, i
    for k, v in y["metrics"].items():
        assert (math.isnan(v) and math.isnan(d["metrics"][k])) or abs(d["metrics"][k] - v) <= 2e-6 * max(1.0, abs(v)), k
    if R.CASES[name].get("views"):
        for l in d["leaves"]:
            assert not bool(l.grad[:, 1:].any())                    # the channel the loss never saw


def test_reference_exceptions():
    args, _ = on_device("h5w9")
    preds, rest = args[0], args[1:]
    with pytest.raises(ZeroDivisionError):
        N.ns_loss(preds[:1], *rest)
    with pytest.raises(TypeError):
        N.ns_loss(preds, *rest, trinocular_loss=False)
    bad = [preds[0], preds[1].detach().clone()]
    bad[1][0, 0, 1, 2] = float("nan")
    with pytest.raises(AssertionError):
        N.ns_loss(bad, *rest)
    bad[0] = bad[1].clone()
    bad[0][0, 0, 1, 2] = float("-inf")
    with pytest.raises(AssertionError):
        N.ns_loss(bad[:1], *rest)                                   # :155 comes before the division of :157
    with pytest.raises(AttributeError):
        N.trinocular_loss(preds[0], rest[2], rest[3], rest[4], rest[1])
    with pytest.raises(_ffi.DktError):
        N.ns_loss(preds, rest[0], rest[1].clone().requires_grad_(True), *rest[2:])


def test_views_are_read_in_place_and_match_contiguous_inputs():
    from dkt_stereo_amd.loss import _plane
    args, leaves = on_device("views")
    for p in args[0]:
        assert not p.is_contiguous() and _plane(p).data_ptr() == p.data_ptr()
    loss, _, _ = N.ns_loss(*args)
    loss.backward()
    flat = [p.detach().contiguous().requires_grad_(True) for p in args[0]]
    loss2, _, _ = N.ns_loss(flat, *args[1:])
    loss2.backward()
    assert R.same(loss, loss2)
    for l, f in zip(leaves, flat):
        assert R.same(l.grad[:, :1], f.grad)
    im = [torch.stack([t, t + 1.0], 1)[:, 0] for t in args[3:]]           # batch-strided images
    assert all(not t.is_contiguous() for t in im)
    assert R.same(N.ns_loss([p.detach() for p in args[0]], args[1], args[2], *im)[0], loss)


def test_two_runs_are_bit_identical():
    a, b = run_device("seams"), run_device("seams")
    assert a["loss"] == b["loss"] and torch.equal(a["automask"], b["automask"])
    for x, y in zip(a["grads"], b["grads"]):
        assert R.same(x, y)


def test_sum_of_parts():
    name = "b2"
    args, _ = on_device(name)
    preds, target, conf, im0, im1, im2 = args
    loss, _, valid = N.ns_loss(*args)
    cf = conf * (target < 0).float()
    w = R.weights(len(preds))
    disp = photo = 0.0
    for i, p in enumerate(preds):
        disp = disp + w[i] * ((p[:, 0] - target).abs() * cf)[valid].mean()
        photo = photo + w[i] * N.trinocular_loss(p, im0, im1, im2, 1 - cf, valid[:, None])
    total = 1.0 * disp + 0.1 * photo
    assert abs(float(total) - float(loss)) <= 4 * R.EPS * abs(float(loss))


def test_memory_is_outputs_byte_planes_and_workspace():
    c = R.CASES["odd"]
    B, H, W, n = c["B"], c["H"], c["W"], 16
    a = {k: torch.from_numpy(v).to(DEV) for k, v in R.inputs(c).items()}
    preds = [(a["preds"][i % 2] + 0.01 * i).requires_grad_(True) for i in range(n)]
    up = torch.tensor(UP, device=DEV)
    N.ns_loss(preds, a["target"], a["conf"], a["im0"], a["im1"], a["im2"])[0].backward()           # warm: library, caches
    for p in preds:
        p.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss, _, _ = N.ns_loss(preds, a["target"], a["conf"], a["im0"], a["im1"], a["im2"])
    loss.backward(up)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    r512 = lambda nbytes: (nbytes + 511) // 512 * 512
    ws = _ffi.lib().dkt_ns_loss_workspace(B, H, W)
    allowed = (r512(4) + r512(B * H * W) + r512(8 * _ffi.NS_REC)          # loss, valid, the record
               + r512(n * B * H * W)                                     # automask and branch, one byte per prediction
               + r512(ws)
               + n * r512(4 * B * H * W) + 2 * r512(4))                  # the gradients, the upstream scalar and its product
    print("ns_loss n=16 2x17x53: peak grew %d bytes, allowed %d (workspace %d)" % (grew, allowed, ws))
    assert grew <= allowed


class _Syncs:
    """Counts torch's synchronising calls inside the block (as test_gpu_optim.py counts them)."""

    def __enter__(self):
        torch.cuda.synchronize()
        self.cm = warnings.catch_warnings(record=True)
        self.rec = self.cm.__enter__()
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        return self

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode(0)
        self.msgs = [str(r.message) for r in self.rec if "called a synchronizing" in str(r.message)]
        self.n = len(self.msgs)
        return self.cm.__exit__(*exc)


def test_one_host_read_per_call():
    args, _ = on_device("b2")
    N.ns_loss(*args)[0].backward()
    args, _ = on_device("b2")
    with _Syncs() as s:
        loss, _, _ = N.ns_loss(*args)
        loss.backward()
    assert s.n == 1, s.msgs
