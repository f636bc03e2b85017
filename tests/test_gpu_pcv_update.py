"""PCVNet's mixture-parameter update on the device (-m gpu): dkt_pcv_update_fwd / dkt_pcv_update_bwd through the raw entries,
through the autograd node of pcvnet_update.parameters_update and through the ParametersUpdater module, against the float64
truth of _pcv_update_ref.py evaluated on the device's own decision bytes, under its per-element bounds; the bytes against the
truth's wherever a decision is not open (test_host_pcv_update_ref.py shows torch's own fp32 autograd inside the bounds and
every mutant outside); the forward without grad against the node's, subsets of results and repeated runs to the bit; one
forward and one backward launch; mixture_upsample against the four reference-shaped calls; and three iterations of
meta_arch/pcvnet/model.py:120-174 on pcvnet_corr.CorrBlock1D, the real ParametersUpdater and mixture_upsample against their
float64 restatement.  Each case prints the kernels' share of the bounds (run with -s).

Before this feature every test here failed at the import of dkt_stereo_amd.pcvnet_update or at the missing symbols."""
import types

import numpy as np
import pytest
import torch

import _pcv_train_ref as PT
import _pcv_update_ref as R
import _upsample_ref as UP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INS = ("delta", "mu", "sigma", "w")
UPS = ("gmu_out", "gw_out", "gsigma_out", "gdisp")
CONSTS = (0.5, 1e-3, 1.0, 1.0, 1.0)


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _raw_fwd(name, disp=True, code=True):
    """dict(mu, w, sigma, disp, code) through the C entry, every output poisoned first."""
    from dkt_stereo_amd import _ffi
    a, c = R.reference(name)["a"], R.CASES[name]
    ins = [G(a[k]) for k in INS]
    outs = [torch.full_like(ins[0], float("nan")) for _ in range(3)]
    dsp = torch.full((c["N"], 1, c["H"], c["W"]), float("nan"), device=DEV) if disp else None
    cd = torch.full(ins[0].shape, 255, dtype=torch.uint8, device=DEV) if code else None
    with _ffi.launch_log() as names:
        _ffi.call("dkt_pcv_update_fwd", ins[0], *[t.data_ptr() for t in ins], *[t.data_ptr() for t in outs], _ffi.ptr(dsp),
                  _ffi.ptr(cd), c["N"], c["M"], c["H"], c["W"], *CONSTS)
    assert names == ["dkt_pcv_update_fwd"]
    return dict(mu=outs[0], w=outs[1], sigma=outs[2], disp=dsp, code=cd)


def _raw_bwd(name, code, upstream=UPS, want=R.GRADS):
    from dkt_stereo_amd import _ffi
    a, c = R.reference(name)["a"], R.CASES[name]
    ins = [G(a[k]) for k in INS]
    ups = [G(a[k]) if k in upstream else None for k in UPS]
    res = [torch.full_like(ins[0], float("nan")) if k in want else None for k in R.GRADS]
    with _ffi.launch_log() as names:
        _ffi.call("dkt_pcv_update_bwd", ins[0], *[t.data_ptr() for t in ins], code.data_ptr(), *[_ffi.ptr(t) for t in ups],
                  *[_ffi.ptr(t) for t in res], c["N"], c["M"], c["H"], c["W"], *CONSTS)
    assert names == ["dkt_pcv_update_bwd"]
    return dict(zip(R.GRADS, res))


def _truth_for(name, code, upstream=UPS):
    return R.truth_on(name, code.cpu().numpy().tobytes(), tuple(upstream))


def _same(a, b):
    return UP.same(a, b)


def _hold(label, name, got, t, keys):
    for k in keys:
        ratio = R.worst(got[k], t["value"][k], t["bound"][k])
        print("%-12s %-6s %-7s %.4f of the bound" % (name, label, k, ratio))
        assert ratio <= 1.0, (name, label, k, ratio)


def _check_code(name, code):
    """The decision rule: the truth's byte wherever no decision of the element is open; at most MAY_DIFFER open; the bytes
    that are exact by construction (the planted zeros of "edge", every w~ of M = 1) are "inside"."""
    t = R.reference(name)["truth"]
    same, share = R.code_agrees(code.cpu(), t)
    print("%-12s code: open %.4f of the elements" % (name, share))
    assert int(code.max()) <= 242 and same and share <= R.MAY_DIFFER, (name, share)
    exact = R.exact_wt(name)
    if exact is not None:
        exact = torch.from_numpy(exact)
        assert bool((R.unpack(code.cpu().numpy())["wt"][exact] == 1).all()), name
        if name == "edge":
            assert bool((R.unpack(code.cpu().numpy())["dw"][exact] == 2).all())


@pytest.mark.parametrize("name", list(R.CASES))
def test_entries(name):
    """The two entries on given inputs under the bounds, the bytes under the decision rule; without disp and code the three
    results have the same bits; fewer gradients asked for have the same bits; a second run repeats the first to the bit; at
    the NaN pixel of "zero" the device has NaN where the truth has, and nowhere else."""
    got = _raw_fwd(name)
    _check_code(name, got["code"])
    t = _truth_for(name, got["code"])
    _hold("raw", name, got, t, R.RESULTS)
    for k in R.RESULTS:
        assert torch.equal(torch.isnan(got[k]).cpu(), torch.isnan(t["value"][k])), (name, k)
    bare = _raw_fwd(name, disp=False, code=False)
    again = _raw_fwd(name)
    for k in ("mu", "w", "sigma"):
        assert _same(got[k], bare[k]) and _same(got[k], again[k]), (name, k)
    assert _same(got["disp"], again["disp"]) and torch.equal(got["code"], again["code"])

    grads = _raw_bwd(name, got["code"])
    _hold("raw", name, grads, t, R.GRADS)
    for k in R.GRADS:
        assert torch.equal(torch.isnan(grads[k]).cpu(), torch.isnan(t["value"][k])), (name, k)
    again = _raw_bwd(name, got["code"])
    for k in R.GRADS:
        assert _same(grads[k], again[k]), (name, k)
        alone = _raw_bwd(name, got["code"], want=(k,))
        assert _same(grads[k], alone[k]) and all(alone[j] is None for j in R.GRADS if j != k), (name, k)


@pytest.mark.parametrize("up", UPS)
def test_single_upstream_gradients(up):
    """Each upstream gradient alone (the other three null) against the truth with the others zero."""
    name = "base"
    code = _raw_fwd(name)["code"]
    t = _truth_for(name, code, upstream=(up,))
    _hold(up, name, _raw_bwd(name, code, upstream=(up,)), t, R.GRADS)
    if up == "gsigma_out":                                  # sigma' does not see mu: an exact zero, not a small number
        assert float(t["value"]["gmu"].abs().max()) == 0.0


class _backward_launches:
    """The names of the backward entry's calls inside the block, from whichever thread: autograd runs the backward on a thread
    of its own, which _ffi.launch_log (thread-local) does not see, so the entry itself is counted (as test_gpu_soft_argmin.py
    counts its own)."""

    def __enter__(self):
        from dkt_stereo_amd import _ffi
        self.lib, self.calls = _ffi.lib(), []
        self.real = self.lib.dkt_pcv_update_bwd

        def counted(*args):
            self.calls.append("dkt_pcv_update_bwd")
            return self.real(*args)
        self.lib.dkt_pcv_update_bwd = counted
        return self.calls

    def __exit__(self, *exc):
        self.lib.dkt_pcv_update_bwd = self.real
        return False


def _node(name, requires=INS, strided=False, regress=True, upstream=UPS):
    """The public function under autograd: results, gradients of sum(result * upstream) and the launches of each pass (the
    forward's through _ffi.launch_log, the backward's through _backward_launches)."""
    from dkt_stereo_amd import _ffi
    from dkt_stereo_amd.pcvnet_update import parameters_update
    a = R.reference(name)["a"]
    leaves = {}
    for k in INS:
        t = G(a[k])
        if strided:                                         # every second column of a tensor twice as wide
            wide = torch.full(t.shape[:-1] + (2 * t.shape[-1],), 3.25, device=DEV)
            wide[..., ::2] = t
            t = wide
        leaves[k] = t.requires_grad_(k in requires)
    view = lambda t: t[..., ::2] if strided else t  # noqa: E731
    with _ffi.launch_log() as fwd:
        outs = parameters_update(*[view(leaves[k]) for k in INS], regress=regress)
    loss = 0.0
    for o, k in zip(outs, UPS):
        if k in upstream and o is not None:
            g = G(a[k])
            if strided:
                g = g.transpose(2, 3).contiguous().transpose(2, 3)
            loss = loss + (o * g).sum()
    with _backward_launches() as bwd, _ffi.launch_log() as stray:
        loss.backward()
    assert stray == []
    got = dict(zip(R.RESULTS, outs))
    for k, n in zip(INS, R.GRADS):
        g = leaves[k].grad
        got[n] = None if g is None else view(g)
    return got, fwd, bwd


@pytest.mark.parametrize("name", list(R.CASES))
def test_node(name):
    """One forward and one backward launch; the node's results are the raw entries' to the bit, and the forward under no_grad
    and with nothing requiring grad is the node's."""
    from dkt_stereo_amd import _ffi
    from dkt_stereo_amd.pcvnet_update import parameters_update
    got, fwd, bwd = _node(name)
    assert fwd == ["dkt_pcv_update_fwd"] and bwd == ["dkt_pcv_update_bwd"], (fwd, bwd)
    raw = _raw_fwd(name)
    grads = _raw_bwd(name, raw["code"])
    for k in R.RESULTS:
        assert _same(got[k], raw[k]), (name, k)
    for k in R.GRADS:
        assert _same(got[k], grads[k]), (name, k)
    ins = [G(R.reference(name)["a"][k]) for k in INS]
    with _ffi.launch_log() as names:
        plain = parameters_update(*ins)
        with torch.no_grad():
            quiet = parameters_update(*[t.clone().requires_grad_(True) for t in ins])
    assert names == ["dkt_pcv_update_fwd"] * 2
    for k, p, q in zip(R.RESULTS, plain, quiet):
        assert _same(got[k], p) and _same(got[k], q) and not p.requires_grad and not q.requires_grad, (name, k)


def test_node_layouts_and_subsets():
    """Non-contiguous inputs and upstream gradients; only the gradients that are required exist; regress=False returns no
    disp and the same three results; a lone upstream gradient reaches the entry alone."""
    name = "base"
    full, _, _ = _node(name)
    strided, fwd, bwd = _node(name, strided=True)
    assert fwd == ["dkt_pcv_update_fwd"] and bwd == ["dkt_pcv_update_bwd"]
    for k in R.RESULTS + R.GRADS:
        assert _same(full[k], strided[k]), k
    for k, n in zip(INS, R.GRADS):
        one, _, bwd = _node(name, requires=(k,))
        assert bwd == ["dkt_pcv_update_bwd"] and _same(one[n], full[n]), k
        assert all(one[m] is None for m in R.GRADS if m != n), k
    three, _, _ = _node(name, regress=False)
    assert three["disp"] is None
    code = _raw_fwd(name)["code"]
    t = _truth_for(name, code, upstream=UPS[:3])
    _hold("no disp", name, three, t, R.GRADS)
    for k in ("mu", "w", "sigma"):
        assert _same(three[k], full[k]), k
    for up in UPS:
        lone, _, bwd = _node(name, upstream=(up,))
        assert bwd == ["dkt_pcv_update_bwd"]
        _hold(up, name, lone, _truth_for(name, code, upstream=(up,)), R.GRADS)


def test_constants_reach_the_kernel():
    """sigma0 and the gammas as arguments (fp32 numbers, so the truth means the same operator)."""
    from dkt_stereo_amd.pcvnet_update import parameters_update
    a = R.reference("base")["a"]
    consts = dict(sigma0=0.75, gammas=(0.25, 0.5, 2.0))
    leaves = [G(a[k]).requires_grad_(True) for k in INS]
    outs = parameters_update(*leaves, **consts)
    sum((o * G(a[k])).sum() for o, k in zip(outs, UPS)).backward()
    t = R.truth(a, consts)
    code = _device_code("base", consts)
    dev = R.truth(a, consts, decisions=code)
    same, share = R.code_agrees(code, t)
    assert same and share <= R.MAY_DIFFER
    got = dict(zip(R.RESULTS, outs))
    got.update({n: l.grad for n, l in zip(R.GRADS, leaves)})
    _hold("consts", "base", got, dev, R.RESULTS + R.GRADS)


def _device_code(name, consts):
    from dkt_stereo_amd import _ffi
    a, c = R.reference(name)["a"], R.CASES[name]
    ins = [G(a[k]) for k in INS]
    outs = [torch.empty_like(ins[0]) for _ in range(3)]
    cd = torch.empty(ins[0].shape, dtype=torch.uint8, device=DEV)
    _ffi.call("dkt_pcv_update_fwd", ins[0], *[t.data_ptr() for t in ins], *[t.data_ptr() for t in outs], None, cd.data_ptr(),
              c["N"], c["M"], c["H"], c["W"], consts["sigma0"], 1e-3, *consts["gammas"])
    return cd.cpu().numpy()


# ---- the module -----------------------------------------------------------------------------------------------------------------

def _module(G_, hidden, weights=None):
    from dkt_stereo_amd.pcvnet_update import ParametersUpdater
    m = ParametersUpdater(types.SimpleNamespace(gauss_num=G_), hidden, hidden).to(DEV)
    if weights is not None:
        m.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    return m


def test_module_is_head_then_node():
    """forward(hidden_state, mu, sigma, w) = parameters_update(head(hidden_state), ...): three results as the reference
    returns them, four with regress=True, the constants read per call."""
    from dkt_stereo_amd.pcvnet_update import parameters_update
    a = R.reference("base")["a"]
    m = _module(4, 8)
    hidden = G(R._synth.normal((1, 8, 6, 10), 2, "hidden"))
    st = [G(a[k]) for k in ("mu", "sigma", "w")]
    with torch.no_grad():
        delta = m.head(hidden)
        three, four = m(hidden, *st), m(hidden, *st, regress=True)
        want = parameters_update(delta, *st)
        assert len(three) == 3 and len(four) == 4
        assert all(_same(x, y) for x, y in zip(four, want)) and all(_same(x, y) for x, y in zip(three, want))
        m.gamma1, m.sigma0 = 0.5, 0.75
        damped = parameters_update(delta, *st, sigma0=0.75, gammas=(0.5, 1, 1))
        assert all(_same(x, y) for x, y in zip(m(hidden, *st, regress=True), damped))


# ---- the up-samplings -----------------------------------------------------------------------------------------------------------

UPC = dict(seed=751, N=2, G=4, H=7, W=13, f=4)


def _up_inputs():
    c = UPC
    shp = (c["N"], c["G"], c["H"], c["W"])
    one = (c["N"], 1, c["H"], c["W"])
    fine = lambda ch: (c["N"] * ch, 1, c["f"] * c["H"], c["f"] * c["W"])  # noqa: E731
    S = R._synth
    return dict(disp=S.normal(one, c["seed"], "disp", scale=5.0), mu=S.normal(shp, c["seed"], "mu", scale=5.0),
                sigma=S.uniform(shp, 0.5, 4.0, c["seed"], "sigma"), w=S.uniform(shp, 0.0, 1.0, c["seed"], "w"),
                mask=S.normal((c["N"], 9 * c["f"] ** 2, c["H"], c["W"]), c["seed"], "mask", scale=2.0),
                g_disp=S.normal((c["N"], 1, c["f"] * c["H"], c["f"] * c["W"]), c["seed"], "g_disp"),
                g_mu=S.normal(fine(c["G"]), c["seed"], "g_mu"), g_sigma=S.normal(fine(c["G"]), c["seed"], "g_sigma"),
                g_w=S.normal(fine(c["G"]), c["seed"], "g_w"))


def test_mixture_upsample():
    """Against the four reference-shaped calls (model.py:165-174) in float64, every result and gradient within the bound of
    _upsample_ref (one call of D channels is D calls of one: the bound of each is that of its own call); w_up has the bits of
    the unscaled call (factor 1 on w is what scale=False means; the node multiplies by the factor, a power of two, what
    mixture_upsample divided out); the mask's gradient is the disp call's alone; no repeated mask: the peak stays below the
    reference form's, which holds G copies of the mask for three of its calls."""
    from dkt_stereo_amd.pcvnet_update import mixture_upsample
    from dkt_stereo_amd.upsample import convex_upsample
    c, a = UPC, _up_inputs()
    f, Gn = c["f"], c["G"]
    names = ("disp", "mu", "sigma", "w", "mask")

    def run(fn, dtype, device):
        t = {k: torch.from_numpy(a[k]).to(device=device, dtype=dtype) for k in a}
        leaves = [t[k].requires_grad_(True) for k in names]
        ups = fn(*leaves, f)
        sum((u * t[g]).sum() for u, g in zip(ups, ("g_disp", "g_mu", "g_sigma", "g_w"))).backward()
        return [u.detach() for u in ups] + [l.grad for l in leaves]

    truth = run(R.upsample4, torch.float64, "cpu")
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    got = run(mixture_upsample, torch.float32, DEV)
    peak_node = torch.cuda.max_memory_allocated() - base
    labels = ("disp_up", "mu_up", "sigma_up", "w_up", "gdisp", "gmu", "gsigma", "gw", "gmask")

    # the bounds of _upsample_ref, per call: (flow, gout, factor-scaled?) of the call that produced each result
    mask64 = torch.from_numpy(a["mask"]).double()
    rep = lambda x: x.reshape(c["N"] * Gn, 1, c["H"], c["W"])  # noqa: E731
    calls = dict(disp=(a["disp"], a["mask"], a["g_disp"]))
    for k in ("mu", "sigma", "w"):
        calls[k] = (rep(torch.from_numpy(a[k])).numpy() / (f if k == "w" else 1),
                    mask64.repeat(1, Gn, 1, 1).reshape(c["N"] * Gn, -1, c["H"], c["W"]).float().numpy(), a["g_" + k])
    worst = {}
    for i, k in enumerate(("disp", "mu", "sigma", "w")):
        flow, mask, gout = (torch.from_numpy(np.ascontiguousarray(x)) for x in calls[k])
        mags = UP.magnitudes(flow, mask, gout, f, 1)
        cs = UP.constants(mags, f, 1)
        out_t = truth[i].reshape(mags["out"].shape)
        gin_t = truth[4 + i].reshape(mags["gflow"].shape)
        gin_scale = (1.0 / f) if k == "w" else 1.0                  # the gradient of w passes the exact 1/f once more
        worst[labels[i]] = UP.worst(got[i].reshape(out_t.shape), out_t, mags["out"], cs["out"])[1]
        worst[labels[4 + i]] = UP.worst(got[4 + i].reshape(gin_t.shape) / gin_scale, gin_t / gin_scale, mags["gflow"], cs["gflow"])[1]
        if k == "disp":
            worst["gmask"] = UP.worst(got[8], truth[8], mags["gmask"], cs["gmask"])[1]
    for k, v in worst.items():
        print("mixture_upsample %-8s %.4f of the bound" % (k, v))
        assert v <= 1.0, (k, v)

    # the unscaled call: scale=False is `unfold(x)` without the factor, i.e. the node at flow = w / f exactly
    fine = lambda x: x.reshape(-1, 1, x.shape[2], x.shape[3])  # noqa: E731
    four = run(lambda d, m, s, w, k, ff: (convex_upsample(d, k, ff), fine(convex_upsample(m, k.detach(), ff)),
                                         fine(convex_upsample(s, k.detach(), ff)),
                                         fine(convex_upsample(w * (1.0 / ff), k.detach(), ff))), torch.float32, DEV)
    assert _same(got[3].reshape(four[3].shape), four[3])
    assert _same(got[1].reshape(four[1].shape), four[1]) and _same(got[2].reshape(four[2].shape), four[2])
    only_disp = run(lambda d, m, s, w, k, ff: (convex_upsample(d, k, ff),), torch.float32, DEV)
    assert _same(got[8], only_disp[-1])                                        # the mask's gradient is the disp call's alone

    def reference_form(d, m, s, w, k, ff):
        N, Gn_, H, W = m.shape
        r = lambda: k.repeat(1, Gn_, 1, 1).reshape(N * Gn_, -1, H, W).detach()  # noqa: E731
        return (convex_upsample(d, k, ff), convex_upsample(m.reshape(-1, 1, H, W), r(), ff),
                convex_upsample(s.reshape(-1, 1, H, W), r(), ff), convex_upsample(w.reshape(-1, 1, H, W) * (1.0 / ff), r(), ff))
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ref_form = run(reference_form, torch.float32, DEV)
    peak_ref = torch.cuda.max_memory_allocated() - base
    print("mixture_upsample peak %d bytes, reference form %d" % (peak_node, peak_ref))
    assert peak_node < peak_ref
    for x, y in zip(got[:4], ref_form[:4]):
        assert _same(x, y)


# ---- the loop -------------------------------------------------------------------------------------------------------------------

def test_three_iteration_loop():
    """model.py:120-174 (refinement aside) on CorrBlock1D, the real ParametersUpdater (head 8 -> 8 -> G, this library's
    convolutions under autograd) and mixture_upsample: coords detached every iteration, mu / w / sigma detached into the
    updater, sigma handed to the next lookup with its graph.  Against the float64 restatement of the same loop, every
    prediction and the gradients of both maps and of the head's four parameters:
        err <= 8 max(|fp32 CPU restatement - truth|, n u max|truth|),  n = L G S = 20
    -- the unit of test_gpu_pcv_train.py's loop.  The taps stay 1e-4 off the integers and every decision's margin above eight
    times the yardstick's own distance (test_host_pcv_update_ref.py), so no floor and no decision is in question."""
    from dkt_stereo_amd.pcvnet_corr import CorrBlock1D
    from dkt_stereo_amd.pcvnet_update import mixture_upsample
    c, a = R.LOOP, R.loop_inputs()
    head = [k for k in a if k.startswith("head.")]
    leaves_of = ("fmap1", "fmap2") + tuple(head)

    def run(dtype, device, device_path):
        t = {k: torch.from_numpy(v).to(device=device, dtype=dtype) for k, v in a.items()}
        if device_path:
            m = _module(c["G"], c["hidden"], {k: a[k] for k in head})
            m.gamma1, m.gamma2, m.gamma3 = c["gammas"]
            params = dict(m.named_parameters())
            leaves = [t["fmap1"].requires_grad_(True), t["fmap2"].requires_grad_(True)] + [params[k] for k in head]
            block = lambda p, q: CorrBlock1D(p, q, sample_num=c["S"], num_levels=c["L"], downsample=c["downsample"])  # noqa: E731
            updater = lambda h, mu, s, w, watch=None: m(h, mu, s, w, regress=True)  # noqa: E731
            ups = mixture_upsample
        else:
            leaves = [t[k].requires_grad_(True) for k in leaves_of]
            block = lambda p, q: PT.TorchBlock(p, q, c["S"], c["L"], c["downsample"])  # noqa: E731
            updater, ups = R.restated_updater(t), R.upsample4
        loss, preds = R.loop(block, updater, ups, t)
        loss.backward()
        return [p.detach() for p in preds] + [l.grad for l in leaves]

    truth = run(torch.float64, "cpu", False)
    yard = run(torch.float32, "cpu", False)
    got = run(torch.float32, DEV, True)
    n = c["L"] * c["G"] * c["S"]
    labels = ["%s %d" % (k, i) for i in range(c["iters"]) for k in ("disp_up", "mu_up", "sigma_up", "w_up")]
    labels += ["g" + k for k in leaves_of]
    assert len(labels) == len(got) == len(truth)
    for label, g, t, y in zip(labels, got, truth, yard):
        assert float(t.abs().max()) > 0.0, label
        err = (g.double().cpu().reshape(t.shape) - t).abs()
        env = 8.0 * torch.maximum((y.double() - t).abs(), torch.full_like(t, n * R.U * float(t.abs().max())))
        ratio = float((err / env).max())
        print("loop %-20s %.4f of the envelope" % (label, ratio))
        assert bool(torch.isfinite(err).all()) and ratio <= 1.0, (label, ratio)
