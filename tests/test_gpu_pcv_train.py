"""PCVNet's correlation block under autograd on the device (-m gpu): dkt_pcv_lookup_bwd / dkt_pcv_pool_bwd through the raw
entries and through the two autograd nodes of pcvnet_corr.CorrBlock1D, against the float64 truth of _pcv_train_ref.py evaluated
on the host-restated fp32 floors, under its per-element bounds (test_host_pcv_train_ref.py shows torch's own fp32 autograd
inside them and every mutant outside); the forward under autograd against the no_grad forward and repeated runs, to the bit;
gradients only for what requires grad; the refusals; and a three-iteration loop shaped like meta_arch/pcvnet/model.py:120-142
against its float64 restatement.  Each case prints the kernels' share of the bounds (run with -s).

Before this feature every test here raised DktError at the first lookup ("the HIP path is inference-only")."""
import numpy as np
import pytest
import torch

import _pcv_train_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INPUTS = ("fmap1", "fmap2", "coords", "sigma", "gout")
KEYS = ("out", "gf1", "gf2", "gcoords", "gsigma")


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _inputs(name):
    ref = R.reference(name)
    return {k: ref[k] for k in INPUTS}


def _levels32(name):
    ref, c = R.reference(name), R.CASES[name]
    pyr = R.pyramid(torch.from_numpy(ref["fmap1"]).double(), torch.from_numpy(ref["fmap2"]).double(), c["L"], R.factor_of(c))
    return [p.float().numpy() for p in pyr]


def _raw_lookup_bwd(name, levels, want=("glevels", "gcoords", "gsigma")):
    """dict(glevels, gcoords, gsigma) through the C entry on given level values; the two small outputs poisoned first."""
    from dkt_stereo_amd import _ffi
    ref, c = R.reference(name), R.CASES[name]
    lv = [G(l) for l in levels]
    coords, sigma, gout = G(ref["coords"]), G(ref["sigma"]), G(ref["gout"])
    B, Gn, H, W = coords.shape
    glv = [torch.zeros_like(l) for l in lv] if "glevels" in want else None
    gc = torch.full_like(coords, float("nan")) if "gcoords" in want else None
    gs = torch.full_like(coords, float("nan")) if "gsigma" in want else None
    with _ffi.launch_log() as names:
        _ffi.call("dkt_pcv_lookup_bwd", gout, _ffi.ptr_array(lv), coords.data_ptr(), sigma.data_ptr(), gout.data_ptr(),
                  None if glv is None else _ffi.ptr_array(glv), _ffi.ptr(gc), _ffi.ptr(gs),
                  B, Gn, H, W, c["W"], c["L"], c["S"], R.factor_of(c))
    assert names == ["dkt_pcv_lookup_bwd"]
    return dict(glevels=glv, gcoords=gc, gsigma=gs)


def _raw_pool_bwd(name):
    from dkt_stereo_amd import _ffi
    c = R.CASES[name]
    gl = [G(g) for g in R.level_grads(c)]
    gvol = torch.full((gl[0].shape[0], c["W"]), float("nan"), device=DEV)
    _ffi.call("dkt_pcv_pool_bwd", gvol, _ffi.ptr_array(gl), gvol.data_ptr(), c["B"], c["H"], c["W"], c["W"], c["L"],
              R.factor_of(c), R.divisor_of(c["C"]))
    return gvol


@pytest.mark.parametrize("name", list(R.CASES))
def test_entries(name):
    """The two entries on given inputs: level gradients, gcoords, gsigma and the folded pool chain under the bounds; asking
    for fewer results gives the same bits for those; a second run repeats the first to the bit."""
    ref, c = R.reference(name), R.CASES[name]
    lv = _levels32(name)
    t = R.truth(_inputs(name), c, floors=ref["floors"], levels=lv)
    got = _raw_lookup_bwd(name, lv)
    for k in ("gcoords", "gsigma"):
        ratio = R.worst(got[k], t[k], t["bound"][k])
        print("%-8s raw  %-8s %.4f of the bound" % (name, k, ratio))
        assert ratio <= 1.0, (name, k, ratio)
    for i in range(c["L"]):
        ratio = R.worst(got["glevels"][i], t["glevels"][i], t["bound"]["glevels"][i])
        print("%-8s raw  glevel %d %.4f of the bound" % (name, i, ratio))
        assert ratio <= 1.0, (name, i, ratio)
    again = _raw_lookup_bwd(name, lv)
    sigma_only = _raw_lookup_bwd(name, lv, want=("gsigma",))
    levels_only = _raw_lookup_bwd(name, lv, want=("glevels",))
    assert torch.equal(got["gcoords"], again["gcoords"]) and torch.equal(got["gsigma"], again["gsigma"])
    assert torch.equal(got["gsigma"], sigma_only["gsigma"]) and sigma_only["gcoords"] is None and sigma_only["glevels"] is None
    for a, b, d in zip(got["glevels"], again["glevels"], levels_only["glevels"]):
        assert torch.equal(a, b) and torch.equal(a, d)
    if c["S"] == 1:
        assert float(got["gsigma"].abs().max()) == 0.0

    gt = [torch.from_numpy(g) for g in R.level_grads(c)]
    div = R.divisor_of(c["C"])
    want = R.pool_bwd_closed(gt, R.factor_of(c), div)
    bound = R.pool_bwd_bound(gt, [torch.zeros_like(g, dtype=torch.float64) for g in gt], R.factor_of(c), div)
    gvol = _raw_pool_bwd(name)
    ratio = R.worst(gvol, want, bound)
    print("%-8s raw  gvol     %.4f of the bound" % (name, ratio))
    assert ratio <= 1.0, (name, ratio)
    assert torch.equal(gvol, _raw_pool_bwd(name))


def _leaves(name, requires=("fmap1", "fmap2", "coords", "sigma")):
    """The four inputs on the device as leaves; for the strided case coords and sigma are every second column of tensors
    twice as wide, the columns in between holding other data."""
    ref, c = R.reference(name), R.CASES[name]
    out = {}
    for k in ("fmap1", "fmap2", "coords", "sigma"):
        t = G(ref[k])
        if c["kind"] == "strided" and k in ("coords", "sigma"):
            wide = torch.full(t.shape[:-1] + (2 * t.shape[-1],), 7.25, device=DEV)
            wide[..., ::2] = t
            t = wide.requires_grad_(k in requires)[..., ::2]
            assert not t.is_contiguous()
            out[k + "_leaf"] = wide
        else:
            t.requires_grad_(k in requires)
        out[k] = t
    return out


def _grad_of(leaves, k):
    if k + "_leaf" in leaves:
        g = leaves[k + "_leaf"].grad
        return None if g is None else g[..., ::2]
    return leaves[k].grad


def _node(name, requires=("fmap1", "fmap2", "coords", "sigma")):
    from dkt_stereo_amd.pcvnet_corr import CorrBlock1D
    ref, c = R.reference(name), R.CASES[name]
    lf = _leaves(name, requires)
    blk = CorrBlock1D(lf["fmap1"], lf["fmap2"], sample_num=c["S"], num_levels=c["L"], downsample=c["downsample"])
    out = blk(lf["coords"], lf["sigma"])
    out.backward(G(ref["gout"]))
    res = dict(out=out.detach(), gf1=lf["fmap1"].grad, gf2=lf["fmap2"].grad, gcoords=_grad_of(lf, "coords"),
               gsigma=_grad_of(lf, "sigma"))
    return res, blk, out


@pytest.mark.parametrize("name", list(R.CASES))
def test_nodes(name):
    """The block from its four inputs, all leaves: one node for the pyramid, one for the lookup; out and the four gradients
    under the bounds; the forward equals the no_grad forward to the bit; a second run repeats every bit."""
    from dkt_stereo_amd.pcvnet_corr import CorrBlock1D
    ref, c = R.reference(name), R.CASES[name]
    truth = ref["truth"]
    got, blk, out = _node(name)
    assert type(out.grad_fn).__name__ == "_LookupFnBackward"
    assert all(type(p.grad_fn).__name__ == "_PyramidFnBackward" for p in blk.corr_pyramid)
    assert len({id(p.grad_fn) for p in blk.corr_pyramid}) == 1
    for k in KEYS:
        ratio = R.worst(got[k], truth[k], truth["bound"][k])
        print("%-8s node %-8s %.4f of the bound" % (name, k, ratio))
        assert ratio <= 1.0, (name, k, ratio)
    if c["S"] == 1:
        assert float(got["gsigma"].abs().max()) == 0.0
    with torch.no_grad():
        lf = _leaves(name)
        quiet_blk = CorrBlock1D(lf["fmap1"], lf["fmap2"], sample_num=c["S"], num_levels=c["L"], downsample=c["downsample"])
        quiet = quiet_blk(lf["coords"], lf["sigma"])
    assert quiet.grad_fn is None and all(p.grad_fn is None for p in quiet_blk.corr_pyramid)
    assert torch.equal(quiet, got["out"])
    for p, q in zip(blk.corr_pyramid, quiet_blk.corr_pyramid):
        assert torch.equal(p.detach(), q)
    again, _, _ = _node(name)
    for k in KEYS:
        assert torch.equal(got[k], again[k]), (name, k)


def test_sigma_alone():
    """Only sigma requires grad (the state of the reference's loop at its first lookup of frozen features): the lookup is a
    node, the pyramid is not, and the backward is one launch that fills gsigma only."""
    from dkt_stereo_amd import _ffi
    from dkt_stereo_amd.pcvnet_corr import CorrBlock1D
    name = "ds2"
    ref, c = R.reference(name), R.CASES[name]
    lf = _leaves(name, requires=("sigma",))
    blk = CorrBlock1D(lf["fmap1"], lf["fmap2"], sample_num=c["S"], num_levels=c["L"], downsample=c["downsample"])
    assert all(p.grad_fn is None and not p.requires_grad for p in blk.corr_pyramid)
    out = blk(lf["coords"], lf["sigma"])
    assert type(out.grad_fn).__name__ == "_LookupFnBackward"
    # the node's backward called in this thread (autograd's own runs on a device thread the launch log does not see):
    # one launch, and nothing but gsigma comes back
    from dkt_stereo_amd.pcvnet_corr import _LookupFn
    with _ffi.launch_log() as names:
        direct = _LookupFn.backward(out.grad_fn, G(ref["gout"]))
    assert names == ["dkt_pcv_lookup_bwd"]
    assert [i for i, g in enumerate(direct) if g is not None] == [1]
    out.backward(G(ref["gout"]))
    assert torch.equal(direct[1], lf["sigma"].grad)
    assert lf["fmap1"].grad is None and lf["fmap2"].grad is None and lf["coords"].grad is None
    full, _, _ = _node(name)
    assert torch.equal(lf["sigma"].grad, full["gsigma"])
    assert R.worst(lf["sigma"].grad, ref["truth"]["gsigma"], ref["truth"]["bound"]["gsigma"]) <= 1.0


def test_feature_maps_alone():
    """Only the maps require grad (RAFT's situation): both nodes run, neither gcoords nor gsigma exists."""
    from dkt_stereo_amd import _ffi
    name = "odd"
    ref = R.reference(name)
    lf = _leaves(name, requires=("fmap1", "fmap2"))
    from dkt_stereo_amd.pcvnet_corr import CorrBlock1D
    c = R.CASES[name]
    blk = CorrBlock1D(lf["fmap1"], lf["fmap2"], sample_num=c["S"], num_levels=c["L"], downsample=c["downsample"])
    out = blk(lf["coords"], lf["sigma"])
    from dkt_stereo_amd.pcvnet_corr import _LookupFn
    with _ffi.launch_log() as names:
        direct = _LookupFn.backward(out.grad_fn, G(ref["gout"]))
    assert names == ["dkt_pcv_lookup_bwd"]
    assert [i for i, g in enumerate(direct) if g is not None] == [5 + i for i in range(c["L"])]
    out.backward(G(ref["gout"]))
    assert lf["coords"].grad is None and lf["sigma"].grad is None
    full, _, _ = _node(name)
    for k, leaf in (("gf1", "fmap1"), ("gf2", "fmap2")):
        assert torch.equal(lf[leaf].grad, full[k])
        assert R.worst(lf[leaf].grad, ref["truth"][k], ref["truth"]["bound"][k]) <= 1.0
    # fmap2 alone: the product for fmap1 is not formed
    lf = _leaves(name, requires=("fmap2",))
    blk = CorrBlock1D(lf["fmap1"], lf["fmap2"], sample_num=c["S"], num_levels=c["L"], downsample=c["downsample"])
    blk(lf["coords"], lf["sigma"]).backward(G(ref["gout"]))
    assert lf["fmap1"].grad is None and torch.equal(lf["fmap2"].grad, full["gf2"])


def test_corr_is_differentiable_and_refusals():
    from dkt_stereo_amd import _ffi
    from dkt_stereo_amd.pcvnet_corr import CorrBlock1D
    ref, c = R.reference("l1"), R.CASES["l1"]
    f1, f2 = G(ref["fmap1"]).requires_grad_(True), G(ref["fmap2"]).requires_grad_(True)
    vol = CorrBlock1D.corr(f1, f2)
    assert vol.requires_grad and vol.shape == (c["B"], c["H"], c["W"], 1, c["W"])
    gv = torch.from_numpy(R.level_grads(c)[0])
    vol.backward(G(gv.numpy()).view(vol.shape))
    want1, want2 = R.products(gv.double() / R.divisor_of(c["C"]), torch.from_numpy(ref["fmap1"]).double(),
                              torch.from_numpy(ref["fmap2"]).double())
    p1, p2 = R.products(gv.double().abs() / R.divisor_of(c["C"]), torch.from_numpy(ref["fmap1"]).double().abs(),
                        torch.from_numpy(ref["fmap2"]).double().abs())
    assert R.worst(f1.grad, want1, 2.0 * R.U * (c["W"] + 2.0) * p1 + R.TINY) <= 1.0
    assert R.worst(f2.grad, want2, 2.0 * R.U * (c["W"] + 2.0) * p2 + R.TINY) <= 1.0
    # a last level of width 1: the reference divides by zero; refused under autograd, unchanged without
    a, b = torch.zeros(1, 4, 2, 7, device=DEV), torch.zeros(1, 4, 2, 7, device=DEV)
    co, sg = torch.zeros(1, 1, 2, 7, device=DEV), torch.ones(1, 1, 2, 7, device=DEV)
    with pytest.raises(_ffi.DktError):
        CorrBlock1D(a.clone().requires_grad_(True), b, sample_num=3, num_levels=2, downsample=2)
    blk = CorrBlock1D(a, b, sample_num=3, num_levels=2, downsample=2)                  # widths 7, 1
    with pytest.raises(_ffi.DktError):
        blk(co, sg.clone().requires_grad_(True))
    with torch.no_grad():
        assert blk(co, sg.clone().requires_grad_(True)).shape == (1, 6, 2, 7)
    assert blk(co, sg).grad_fn is None
    with pytest.raises(ValueError):
        blk(co, sg[:, :, :1])


def test_three_iteration_loop():
    """model.py:120-142 with a stand-in head: coords detached every iteration, sigma the previous iteration's head output with
    its graph, so the loss reaches the head through the NEXT lookup's gsigma.  Against the float64 restatement of the same loop
    (TorchBlock), every lookup and the gradients of both maps and of the sigma head's weights:
        err <= 8 max(|fp32 CPU restatement - truth|, n u max|truth|),  n = L G S = 20
    -- the project's envelope rule; the floor is the first-order size of the shortest reduction every result passes through
    (the head's projection sums n products; every other sum of the loop is longer).  The taps of this case stay 1e-4 away from
    the integers (test_host_pcv_train_ref.py), so no floor is in question.  A backward that stopped at the maps would leave
    the head's gradient without its later-iteration terms."""
    from dkt_stereo_amd.pcvnet_corr import CorrBlock1D
    c, a = R.LOOP, R.loop_inputs()
    names = ("fmap1", "fmap2", "coords", "sigma", "head_sigma", "head_mu", "gouts", "gsig")

    def run(block, dtype, device):
        t = {k: torch.from_numpy(a[k]).to(device=device, dtype=dtype) for k in names}
        leaves = [t[k].requires_grad_(True) for k in ("fmap1", "fmap2", "head_sigma")]
        loss, outs = R.loop(block, t["fmap1"], t["fmap2"], t["coords"], t["sigma"], t["head_sigma"], t["head_mu"], t["gouts"],
                            t["gsig"], c["iters"])
        loss.backward()
        return [o.detach() for o in outs] + [l.grad for l in leaves]

    restated = lambda p, q: R.TorchBlock(p, q, c["S"], c["L"], c["downsample"])  # noqa: E731
    truth = run(restated, torch.float64, "cpu")
    yard = run(restated, torch.float32, "cpu")
    got = run(lambda p, q: CorrBlock1D(p, q, sample_num=c["S"], num_levels=c["L"], downsample=c["downsample"]),
              torch.float32, DEV)
    n = c["L"] * c["G"] * c["S"]
    labels = ["lookup %d" % i for i in range(c["iters"])] + ["gfmap1", "gfmap2", "ghead_sigma"]
    assert float(truth[-1].abs().max()) > 0.0
    for label, g, t, y in zip(labels, got, truth, yard):
        err = (g.double().cpu() - t).abs()
        env = 8.0 * torch.maximum((y.double() - t).abs(), torch.full_like(t, n * R.U * float(t.abs().max())))
        ratio = float((err / env).max())
        print("loop %-12s %.4f of the envelope" % (label, ratio))
        assert bool(torch.isfinite(err).all()) and ratio <= 1.0, (label, ratio)
