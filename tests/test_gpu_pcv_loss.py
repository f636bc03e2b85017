"""PCVNet's sequence loss on the device (-m gpu): dkt_pcv_loss / dkt_pcv_loss_bwd through the raw entries, through
pcvnet_loss.sequence_loss_pcvnet and pcv_loss_pair, against the float64 truth of _pcv_loss_ref.py under its bounds, and EQUAL
to torch's fp32 restatement on the mask, the counts, the twelve fractions and the sign pattern of every gradient
(test_host_pcv_loss_ref.py shows torch's own fp32 autograd inside the bounds and every mutant outside); the reference's
exceptions, its list rebinding and the repeated call; exact zeros off the mask; repeats to the bit; CHECK_MIXTURE_FINITE;
only the required gradients; the launches and the one host read; and three iterations of _pcv_update_ref's PCVNet loop
ending in this loss against their float64 restatement.  Each case prints the kernels' share of the bounds (run with -s).

Before this feature every test here failed at the import of dkt_stereo_amd.pcvnet_loss or at the missing symbols.

Figures (MI355X), the largest error / bound over all cases: see DESIGN 3.26."""
import types
import warnings

import numpy as np
import pytest
import torch

import _pcv_loss_ref as R
from dkt_stereo_amd import _ffi, pcvnet_loss as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYOUTS = ("plain", "views", "5d")


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _args(a):
    return types.SimpleNamespace(gauss_num=a["M"])


def _lay(v, layout, M, leaf):
    """(the tensor the loss sees, the leaf that collects its gradient, how to read the gradient back as the plain layout)."""
    t = G(v)
    if layout == "views":
        base = torch.cat((t, t + 1.0), dim=1)
        if leaf:
            base.requires_grad_(True)
        return base[:, :1], base, lambda g: g[:, :1]
    if layout == "5d" and t.shape[0] % M == 0 and M > 0:
        t = t.reshape(t.shape[0] // M, M, 1, t.shape[2], t.shape[3]).contiguous()
    if leaf:
        t.requires_grad_(True)
    return t, t, lambda g: g


def on_device(name, layout="plain", requires=None, a=None):
    """results, targets [(gt, valid)], and the leaves dict(refine, disp [n], mu [n]) as (leaf, reader) pairs."""
    a = R.inputs(name) if a is None else a
    M, n = a["M"], len(a["mu"])
    want = (lambda key, i: True) if requires is None else (lambda key, i: (key, i) in requires)
    mixl = layout if layout in ("views", "5d") else "plain"
    pixl = "views" if layout == "views" else "plain"
    refine, rl, rr = _lay(a["refine"], pixl, 0, want("refine", 0))
    leaves = dict(refine=(rl, rr), disp=[], mu=[])
    disps, mus, ws, sigmas = [], [], [], []
    for i in range(n):
        t, l, r = _lay(a["disp"][i], pixl, 0, want("disp", i))
        disps.append(t)
        leaves["disp"].append((l, r))
        t, l, r = _lay(a["mu"][i], mixl, M, want("mu", i))
        mus.append(t)
        leaves["mu"].append((l, r))
        ws.append(_lay(a["w"][i], mixl, M, False)[0])
        sigmas.append(_lay(a["sigma"][i], mixl, M, False)[0])
    res = {"output_list": (refine, disps, mus, ws, sigmas)}
    if layout == "views":
        targets = [(torch.cat((G(g), G(g)), 1)[:, :1], torch.stack((G(v), G(v)), 1)[:, 0]) for g, v in zip(a["gt"], a["valid"])]
    else:
        targets = [(G(g), G(v)) for g, v in zip(a["gt"], a["valid"])]
    return a, res, targets, leaves


def _grads(leaves, shape_of):
    """The leaves' gradients in the plain layout (zeros where a leaf received none), for _pcv_loss_ref.compare."""
    def read(pair, like):
        leaf, reader = pair
        if leaf.grad is None:
            return torch.zeros(like.shape)
        return reader(leaf.grad).detach().cpu().reshape(like.shape)
    return dict(grefine=read(leaves["refine"], shape_of["refine"]),
                gdisp=[read(p, v) for p, v in zip(leaves["disp"], shape_of["disp"])],
                gmu=[read(p, v) for p, v in zip(leaves["mu"], shape_of["mu"])])


def run_sequence(name, layout="plain", k=0, backward=True):
    a, res, targets, leaves = on_device(name, layout)
    loss, metrics, mask = P.sequence_loss_pcvnet(res, *targets[k], args=_args(a))
    got = dict(targets=[dict(loss=loss, metrics=metrics, mask=mask.cpu(), raises=None)], res=res, leaves=leaves)
    if backward and torch.is_tensor(loss):
        (loss * R.UPSTREAM[0]).backward()
        got.update(_grads(leaves, a))
    return got


def _single(a, k=0):
    return dict(a, gt=a["gt"][k:k + 1], valid=a["valid"][k:k + 1])


@pytest.fixture(scope="module")
def refs():
    """truth and fp32 yardstick of a case restricted to its first target, computed once per case and shared."""
    cache = {}

    def get(name, pair=False):
        key = (name, pair)
        if key not in cache:
            a = R.inputs(name)
            a = a if pair else _single(a)
            cache[key] = dict(a=a, truth=R.truth(a), fp32=R.torch_run(a, torch.float32))
        return cache[key]
    return get


def hold(label, got, ref):
    """Bounds, equalities and the exact zeros off every mask."""
    t, y = ref["truth"], ref["fp32"]
    assert R.exact_facts(got) == R.exact_facts(y), label
    for k, (g, tk) in enumerate(zip(got["targets"], t["targets"])):
        if tk["loss"] is None:
            assert type(g["loss"]) is int and g["loss"] == 0 and g["metrics"] == R.EMPTY_METRICS, label
        else:
            assert sorted(g["metrics"]) == sorted(R.METRIC_KEYS) and all(type(v) is float for v in g["metrics"].values())
            assert g["loss"].dim() == 0 and g["loss"].dtype == torch.float32 and g["mask"].dtype == torch.bool
    for what, ratio in R.compare(got, t).items():
        print("%-28s %-10s %.4f of the bound" % (label, what, ratio))
        assert ratio <= 1.0, (label, what, ratio)
    if "gdisp" in got:
        off = ~torch.stack([tk["mask"] for tk in t["targets"] if tk["loss"] is not None]).any(0)
        B, _, H, W = off.shape
        assert float(got["grefine"][off].abs().max()) == 0.0 if off.any() else True
        for g in got["gdisp"]:
            assert not off.any() or float(g[off].abs().max()) == 0.0, label
        for g in got["gmu"]:
            g = g.reshape(B, -1, H, W)
            assert not off.any() or float(g[off.expand_as(g)].abs().max()) == 0.0, label


# ---- the raw entries --------------------------------------------------------------------------------------------------------

def _raw(a, backward=True, check=True, want=None):
    """dkt_pcv_loss and dkt_pcv_loss_bwd on contiguous tensors, min(n, 7) predictions: got (torch_run's layout) and rec."""
    M, n, K = a["M"], min(len(a["mu"]), _ffi.PCV_LOSS_MAX_PRED), len(a["gt"])
    B, _, H, W = a["refine"].shape
    keep = dict(refine=G(a["refine"]), disp=[G(v) for v in a["disp"][:n]], mu=[G(v) for v in a["mu"][:n]],
                w=[G(v) for v in a["w"][:n]], sigma=[G(v) for v in a["sigma"][:n]], gt=[G(v) for v in a["gt"]],
                valid=[G(v) for v in a["valid"]])
    d = _ffi.PcvLossDesc()
    for i in range(n):
        d.disp[i], d.disp_bstride[i] = keep["disp"][i].data_ptr(), H * W
        d.mu[i], d.mu_bstride[i], d.mu_gstride[i] = keep["mu"][i].data_ptr(), M * H * W, H * W
        if check:
            d.w[i], d.w_bstride[i], d.w_gstride[i] = keep["w"][i].data_ptr(), M * H * W, H * W
            d.sigma[i], d.sigma_bstride[i], d.sigma_gstride[i] = keep["sigma"][i].data_ptr(), M * H * W, H * W
    n_loss = min(n, 6)
    for i in range(n_loss):
        d.weight[i] = R.I_WEIGHTS[i]
    d.refine, d.refine_bstride, d.refine_weight = keep["refine"].data_ptr(), H * W, 1.4
    d.n, d.n_loss, d.M, d.ntargets, d.max_disp = n, n_loss, M, K, 512.0
    losses = [torch.full((), 7.0, device=DEV) for _ in range(K)]
    masks = [torch.full((B, 1, H, W), True, device=DEV) for _ in range(K)]
    rec = torch.full((_ffi.PCV_LOSS_REC,), -1.0, device=DEV, dtype=torch.float64)
    for k in range(K):
        d.gt[k], d.gt_bstride[k] = keep["gt"][k].data_ptr(), H * W
        d.valid[k], d.valid_bstride[k] = keep["valid"][k].data_ptr(), H * W
        d.mask[k], d.loss[k] = masks[k].data_ptr(), losses[k].data_ptr()
    d.rec, d.B, d.H, d.W = rec.data_ptr(), B, H, W
    ws = torch.empty(_ffi.size("dkt_pcv_loss_partial_doubles", K, B, H, W), device=DEV, dtype=torch.float64)
    _ffi.call("dkt_pcv_loss", ws, d, ws.data_ptr())
    r = rec.cpu().tolist()
    got = dict(targets=[], rec=r, raw_losses=[float(l) for l in losses])
    for k in range(K):
        m = dict(zip(R.METRIC_KEYS, r[16 * k + 1:16 * k + 15]))
        got["targets"].append(dict(loss=float(losses[k]), metrics=m, mask=masks[k].cpu(), raises=None, N=r[16 * k]))
    if backward:
        g = _ffi.PcvLossGrad()
        ups = [torch.tensor(R.UPSTREAM[k], device=DEV) for k in range(K)]
        nan = lambda shape: torch.full(shape, float("nan"), device=DEV)                                # noqa: E731
        wanted = (lambda key, i: True) if want is None else (lambda key, i: (key, i) in want)
        out = dict(grefine=nan((B, 1, H, W)) if wanted("refine", 0) else None,
                   gdisp=[nan((B, 1, H, W)) if wanted("disp", i) else None for i in range(n)],
                   gmu=[nan((B * M, 1, H, W)) if wanted("mu", i) else None for i in range(n)])
        g.grefine = _ffi.ptr(out["grefine"])
        for i in range(n):
            g.gdisp[i], g.gmu[i] = _ffi.ptr(out["gdisp"][i]), _ffi.ptr(out["gmu"][i])
        for k in range(K):
            g.grad_loss[k] = ups[k].data_ptr() if r[16 * k] > 0 else None        # an empty target: no upstream, as the node passes it
        _ffi.call("dkt_pcv_loss_bwd", ws, d, g)
        got.update(grefine=None if out["grefine"] is None else out["grefine"].cpu(),
                   gdisp=[None if t is None else t.cpu() for t in out["gdisp"]],
                   gmu=[None if t is None else t.cpu() for t in out["gmu"]])
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("name", list(R.CASES))
def test_entries(name, refs):
    """Every case through the C entries: the record's N, metrics and flag word, the device scalars, the masks, the gradients
    (buffers pre-filled with NaN: every element is stored).  The raising cases are data here: their flag word and, where the
    sequence is too long or too short, the values of what was computed."""
    ref = refs(name, pair=True)
    a, t = ref["a"], ref["truth"]
    got = _raw(a)
    assert int(got["rec"][32]) == R.expected_flags(a), name
    assert got["rec"][15] == 0.0 and all(v == 0.0 for v in got["rec"][33:])
    for g, tk in zip(got["targets"], t["targets"]):
        assert g["N"] == tk["N"] and torch.equal(g["mask"], tk["mask"]), name
    n = len(a["mu"])
    if name in R.RAISING or any(tk["loss"] is None for tk in t["targets"]):
        for k, tk in enumerate(t["targets"]):
            if tk["loss"] is None:
                assert np.isnan(got["raw_losses"][k])                  # the mean of an empty set, as torch's is
        live = [k for k, tk in enumerate(t["targets"]) if tk["loss"] is not None]
        if name in R.RAISING or not live:
            return
        # (the case "pair": the first target's numbers beside an empty second one)
        sub = dict(targets=[got["targets"][k] for k in live], grefine=got["grefine"], gdisp=got["gdisp"], gmu=got["gmu"])
        ref1 = refs(name)
        assert live == [0]
        hold("entries " + name, _as_returned(sub), ref1)
        return
    assert n <= 6
    hold("entries " + name, _as_returned(got), ref)


def _as_returned(got):
    """A raw run in the form the Python entry returns it (loss as a 0-dim tensor, float metrics)."""
    out = dict(got)
    out["targets"] = [dict(g, loss=torch.tensor(g["loss"], dtype=torch.float32)) for g in got["targets"]]
    return out


def test_entries_skip_null_gradients_and_absent_upstream():
    a = R.inputs("pair2")
    full = _raw(a)
    part = _raw(a, want={("disp", 2), ("mu", 4)})
    assert part["grefine"] is None and torch.equal(part["gdisp"][2], full["gdisp"][2]) and torch.equal(part["gmu"][4], full["gmu"][4])
    assert sum(t is not None for t in part["gdisp"] + part["gmu"]) == 2


# ---- the Python entries -----------------------------------------------------------------------------------------------------

class _backward_launches:
    """The backward entry's calls inside the block, from whichever thread: autograd runs the backward on a thread of its own,
    which _ffi.launch_log (thread-local) does not see, so the entry itself is counted (as test_gpu_pcv_update.py counts its own)."""

    def __enter__(self):
        self.lib, self.calls = _ffi.lib(), []
        self.real = self.lib.dkt_pcv_loss_bwd

        def counted(*args):
            self.calls.append("dkt_pcv_loss_bwd")
            return self.real(*args)
        self.lib.dkt_pcv_loss_bwd = counted
        return self.calls

    def __exit__(self, *exc):
        self.lib.dkt_pcv_loss_bwd = self.real
        return False


@pytest.mark.parametrize("name", R.VALUE_CASES)
def test_sequence_loss(name, refs):
    got = run_sequence(name)
    hold("sequence " + name, got, refs(name))
    a = R.inputs(name)
    _, _, mu_preds, w_preds, sigma_preds = got["res"]["output_list"]
    empty = refs(name)["truth"]["targets"][0]["loss"] is None
    for lst in (mu_preds, w_preds, sigma_preds):                       # loss.py:35-38; untouched on the empty mask (:20-27)
        assert all(t.dim() == (4 if empty else 5) for t in lst), name
        if not empty:
            assert all(tuple(t.shape[:3]) == (a["refine"].shape[0], a["M"], 1) for t in lst)


@pytest.mark.parametrize("name", list(R.RAISING))
def test_exceptions_and_what_they_leave_behind(name):
    a, res, targets, _ = on_device(name)
    with pytest.raises(AssertionError if R.RAISING[name] == "AssertionError" else IndexError):
        P.sequence_loss_pcvnet(res, *targets[0], args=_args(a))
    n = len(a["mu"])
    flags = R.expected_flags(a)
    first = next((i for i in range(n) if (flags >> i) & 1), min(n, 7))
    for lst in res["output_list"][2:]:
        assert [t.dim() for t in lst] == [5] * first + [4] * (n - first), name


def test_nan_refine_goes_into_the_loss(refs):
    got = run_sequence("nan_refine")
    assert torch.isnan(got["targets"][0]["loss"]) and np.isnan(got["targets"][0]["metrics"]["epe_final"])
    assert np.isfinite(got["targets"][0]["metrics"]["epe"])


@pytest.mark.parametrize("layout", LAYOUTS[1:])
def test_layouts_are_read_in_place(layout, refs):
    """`[:, :1]` views of two-channel tensors (targets included) and the (B,M,1,H,W) layout: the same bits as the plain
    layout, and nothing lands in the channel the view leaves out."""
    plain, got = run_sequence("strided"), run_sequence("strided", layout)
    hold("%s strided" % layout, got, refs("strided"))
    assert torch.equal(plain["targets"][0]["loss"], got["targets"][0]["loss"]) and plain["targets"][0]["metrics"] == got["targets"][0]["metrics"]
    for key in ("gdisp", "gmu"):
        assert all(torch.equal(x, y) for x, y in zip(plain[key], got[key]))
    assert torch.equal(plain["grefine"], got["grefine"])
    if layout == "views":
        for leaf, _ in [got["leaves"]["refine"]] + got["leaves"]["disp"] + got["leaves"]["mu"]:
            assert float(leaf.grad[:, 1:].abs().max()) == 0.0


def test_mixture_upsample_views_are_read_in_place(refs):
    """mixture_upsample's N = 1 results are views into one (1, 3G, H, W) tensor: split(G, dim=1) then reshape(G,1,H,W)."""
    a = R.inputs("n4")
    M, n = a["M"], len(a["mu"])
    _, res, targets, leaves = on_device("n4")
    stacks = []
    for i in range(n):
        st = torch.cat([G(a[key][i]).reshape(1, M, *a[key][i].shape[2:]) for key in ("mu", "sigma", "w")], dim=1).requires_grad_(True)
        mu, sigma, w = (t.reshape(M, 1, *t.shape[2:]) for t in st.split(M, dim=1))
        assert mu.data_ptr() == st.data_ptr() and w._base is not None
        res["output_list"][2][i], res["output_list"][4][i], res["output_list"][3][i] = mu, sigma, w
        stacks.append(st)
    loss, metrics, mask = P.sequence_loss_pcvnet(res, *targets[0], args=_args(a))
    (loss * R.UPSTREAM[0]).backward()
    got = dict(targets=[dict(loss=loss, metrics=metrics, mask=mask.cpu(), raises=None)])
    for i in range(n):
        leaves["mu"][i] = (stacks[i], lambda g, M=M: g[:, :M])
        assert float(stacks[i].grad[:, M:].abs().max()) == 0.0
    got.update(_grads(leaves, a))
    hold("split n4", got, refs("n4"))


@pytest.mark.parametrize("name", ("pair", "pair2", "ord"))
def test_pair(name, refs):
    """pcv_loss_pair against the two calls: each part what its own call returns (to the bit), the gradients of the sum
    against the truth of both targets."""
    a = R.inputs(name)
    if len(a["gt"]) == 1:
        a = dict(a, gt=a["gt"] * 2, valid=[a["valid"][0], np.roll(a["valid"][0], 3, axis=-1)])
    ref = dict(a=a, truth=R.truth(a), fp32=R.torch_run(a, torch.float32))
    _, res, targets, leaves = on_device(name, a=a)
    with _ffi.launch_log() as names, _backward_launches() as back:
        l0, m0, v0, l1, v1 = P.pcv_loss_pair(res, *targets[0], *targets[1], args=_args(a))
        total = sum(l * R.UPSTREAM[k] for k, l in enumerate((l0, l1)) if torch.is_tensor(l))
        total.backward()
    assert names == ["dkt_pcv_loss"] and back == ["dkt_pcv_loss_bwd"]       # one forward entry (two launches), one backward launch
    got = dict(targets=[dict(loss=l0, metrics=m0, mask=v0.cpu(), raises=None)])
    singles = []
    for k in range(2):
        _, res_k, targets_k, _ = on_device(name, a=a)
        singles.append(P.sequence_loss_pcvnet(res_k, *targets_k[k], args=_args(a)))
    got["targets"].append(dict(loss=l1, metrics=singles[1][1], mask=v1.cpu(), raises=None))
    got.update(_grads(leaves, a))
    hold("pair " + name, got, ref)
    for (l, m, v), (pl, pm, pv) in zip(singles, ((l0, m0, v0), (l1, None, v1))):
        assert torch.equal(v, pv) and (pm is None or m == pm)
        assert (l == pl) if type(l) is int else torch.equal(l, pl)
    assert all(t.dim() == 5 for t in res["output_list"][2])


def test_repeated_call_and_bit_identical_repeats():
    """The first call leaves the lists 5-D (views of the same storage); the second call on the same results works (the
    reference raises ValueError there) and returns the same bits, forward and backward."""
    a, res, targets, leaves = on_device("vec")
    before = [t.data_ptr() for t in res["output_list"][2]]
    runs = []
    for _ in range(2):
        loss, metrics, mask = P.sequence_loss_pcvnet(res, *targets[0], args=_args(a))
        for lst in leaves["disp"] + leaves["mu"] + [leaves["refine"]]:
            lst[0].grad = None
        (loss * R.UPSTREAM[0]).backward()
        runs.append((loss.detach().clone(), metrics, mask.clone(), _grads(leaves, a)))
        assert all(t.dim() == 5 for t in res["output_list"][2]) and [t.data_ptr() for t in res["output_list"][2]] == before
    (l0, m0, k0, g0), (l1, m1, k1, g1) = runs
    assert torch.equal(l0, l1) and m0 == m1 and torch.equal(k0, k1) and torch.equal(g0["grefine"], g1["grefine"])
    assert all(torch.equal(x, y) for key in ("gdisp", "gmu") for x, y in zip(g0[key], g1[key]))
    x, y = _raw(_single(a)), _raw(_single(a))
    assert x["rec"] == y["rec"] and x["raw_losses"] == y["raw_losses"] and torch.equal(x["grefine"], y["grefine"])
    assert all(torch.equal(p, q) for key in ("gdisp", "gmu") for p, q in zip(x[key], y[key]))


def test_check_mixture_finite_switch(refs, monkeypatch):
    """False: w and sigma are not read -- the same numbers, no assertion on a NaN sigma; a NaN mu still asserts."""
    on = run_sequence("ord")
    monkeypatch.setattr(P, "CHECK_MIXTURE_FINITE", False)
    off = run_sequence("ord")
    hold("unchecked ord", off, refs("ord"))
    assert torch.equal(on["targets"][0]["loss"], off["targets"][0]["loss"]) and on["targets"][0]["metrics"] == off["targets"][0]["metrics"]
    assert all(torch.equal(x, y) for key in ("gdisp", "gmu") for x, y in zip(on[key], off[key]))
    for name in ("nan_sigma", "inf_w_offmask"):
        a, res, targets, _ = on_device(name)
        loss, _, _ = P.sequence_loss_pcvnet(res, *targets[0], args=_args(a))
        assert bool(torch.isfinite(loss))
    a, res, targets, _ = on_device("nan_mu")
    with pytest.raises(AssertionError):
        P.sequence_loss_pcvnet(res, *targets[0], args=_args(a))
    got = _raw(_single(R.inputs("nan_sigma")), backward=False, check=False)
    assert got["rec"][32] == 0.0


def test_backward_allocates_only_the_required_gradients():
    name, need = "vec", {("disp", 2), ("mu", 4)}
    a, res, targets, leaves = on_device(name, requires=need)
    loss, _, _ = P.sequence_loss_pcvnet(res, *targets[0], args=_args(a))
    up = torch.tensor(R.UPSTREAM[0], device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss.backward(up)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    B, _, H, W = a["refine"].shape
    r512 = lambda nbytes: (nbytes + 511) // 512 * 512                                                  # noqa: E731
    allowed = r512(4 * B * H * W) + r512(4 * B * a["M"] * H * W) + 4 * 512         # the two gradients; scalars of the upstream product
    print("pcv_loss backward, 2 of 13 gradients required: peak grew %d bytes, allowed %d" % (grew, allowed))
    assert grew <= allowed
    for key in ("disp", "mu"):
        for i, (leaf, _) in enumerate(leaves[key]):
            assert (leaf.grad is not None) == ((key, i) in need), (key, i)
    assert leaves["refine"][0].grad is None
    full = run_sequence(name)
    assert torch.equal(leaves["disp"][2][0].grad.cpu(), full["gdisp"][2]) and torch.equal(leaves["mu"][4][0].grad.cpu(), full["gmu"][4])
    # nothing required: no launch at all
    a, res, targets, _ = on_device(name, requires=set())
    with _ffi.launch_log() as names:
        loss, _, _ = P.sequence_loss_pcvnet(res, *targets[0], args=_args(a))
    assert names == ["dkt_pcv_loss"] and not loss.requires_grad


class _Syncs:
    """Counts torch's synchronising calls inside the block (as test_gpu_ns_loss.py counts them)."""

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
    for pair in (False, True):
        for _ in range(2):                      # (the first round warms the library and the allocator)
            a, res, targets, _ = on_device("pair2")
            with _Syncs() as s:
                if pair:
                    l0, _, _, l1, _ = P.pcv_loss_pair(res, *targets[0], *targets[1], args=_args(a))
                    (l0 + l1).backward()
                else:
                    loss, _, _ = P.sequence_loss_pcvnet(res, *targets[0], args=_args(a))
                    loss.backward()
        assert s.n == 1, s.msgs


# ---- the loop -------------------------------------------------------------------------------------------------------------------

def test_three_iteration_loop_ending_in_the_loss():
    """model.py:120-174 (refinement aside) as test_gpu_pcv_update.py runs it -- CorrBlock1D, the real ParametersUpdater,
    mixture_upsample -- with its four up-sampled results per iteration handed to sequence_loss_pcvnet (the last iteration
    standing twice, its disparity standing for disp_refine: _pcv_loss_ref.loop_results).  The target comes from the float64
    loop's own predictions and keeps every compared plane LOOP_MARGIN away from it, so every sign and branch is settled.
    Against the float64 restatement of the same loop and loss: the loss, and the gradients of both maps and of the head's four
    parameters, in the unit of test_gpu_pcv_update.py's loop:
        err <= 8 max(|fp32 CPU restatement - truth|, n u max|truth|),  n = L G S = 20."""
    import _pcv_train_ref as PT
    import _pcv_update_ref as U
    from dkt_stereo_amd.pcvnet_corr import CorrBlock1D
    from dkt_stereo_amd.pcvnet_update import ParametersUpdater, mixture_upsample
    c, a = U.LOOP, U.loop_inputs()
    head = [k for k in a if k.startswith("head.")]
    leaves_of = ("fmap1", "fmap2") + tuple(head)
    M = c["G"]
    target = {}

    def run(dtype, device, device_path):
        t = {k: torch.from_numpy(v).to(device=device, dtype=dtype) for k, v in a.items()}
        if device_path:
            m = ParametersUpdater(types.SimpleNamespace(gauss_num=M), c["hidden"], c["hidden"]).to(DEV)
            m.load_state_dict({k: torch.from_numpy(a[k]) for k in head})
            m.gamma1, m.gamma2, m.gamma3 = c["gammas"]
            params = dict(m.named_parameters())
            leaves = [t["fmap1"].requires_grad_(True), t["fmap2"].requires_grad_(True)] + [params[k] for k in head]
            block = lambda p, q: CorrBlock1D(p, q, sample_num=c["S"], num_levels=c["L"], downsample=c["downsample"])  # noqa: E731
            updater = lambda h, mu, s, w, watch=None: m(h, mu, s, w, regress=True)  # noqa: E731
            ups = mixture_upsample
        else:
            leaves = [t[k].requires_grad_(True) for k in leaves_of]
            block = lambda p, q: PT.TorchBlock(p, q, c["S"], c["L"], c["downsample"])  # noqa: E731
            updater, ups = U.restated_updater(t), U.upsample4
        _, preds = U.loop(block, updater, ups, t)
        if not target:
            target["gt"], target["valid"] = R.loop_target(preds, M)
        res = R.loop_results(preds)
        gt = torch.from_numpy(target["gt"]).to(device=device, dtype=dtype)
        valid = torch.from_numpy(target["valid"]).to(device=device, dtype=dtype)
        if device_path:
            loss, metrics, mask = P.sequence_loss_pcvnet(res, gt, valid, args=types.SimpleNamespace(gauss_num=M))
        else:
            refine, disps, mus, ws, sigmas = res["output_list"]
            loss, metrics, mask = R.restated(refine, disps, mus, ws, sigmas, gt, valid, M)
        loss.backward()
        return [loss.detach().reshape(1)] + [l.grad for l in leaves], mask.cpu(), metrics

    truth, mask64, metrics64 = run(torch.float64, "cpu", False)
    yard, mask32, _ = run(torch.float32, "cpu", False)
    got, mask, metrics = run(torch.float32, DEV, True)
    assert torch.equal(mask, mask64) and torch.equal(mask32, mask64) and int(mask64.sum()) > 0.5 * mask64.numel()
    for k in R.COUNT_KEYS:
        assert metrics[k] == float(np.float32(metrics64[k])), k
    n = c["L"] * c["G"] * c["S"]
    labels = ["loss"] + ["g" + k for k in leaves_of]
    assert len(labels) == len(got) == len(truth)
    for label, g, t, y in zip(labels, got, truth, yard):
        assert float(t.abs().max()) > 0.0, label
        err = (g.double().cpu().reshape(t.shape) - t).abs()
        env = 8.0 * torch.maximum((y.double() - t).abs(), torch.full_like(t, n * R.U * float(t.abs().max())))
        ratio = float((err / env).max())
        print("loop %-20s %.4f of the envelope" % (label, ratio))
        assert bool(torch.isfinite(err).all()) and ratio <= 1.0, (label, ratio)
