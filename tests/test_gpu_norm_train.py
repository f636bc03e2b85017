"""The instance-norm training nodes (-m gpu): dkt_instance_norm_bwd / dkt_instance_norm_add_relu_bwd behind
norm_train.instance_norm / instance_norm_add_relu, and their wiring into the encoders (extractor.TRAIN_NORM_NODES).

Forward: bit-identical to the inference kernels on the same input.  Backward: against the float64 closed form under the
bound derived in _norm_train_ref.py,

    |gx - truth| <= 8 U r (|g| + |mean g| + |yh| |mean(g yh)|) + r (e_y |mean(g yh)| + |yh| mean(|g| e_y)),  U = 2^-24,

with the masks of the forward under test; ga = gout [out > 0] exactly.  test_host_norm_train_ref.py shows that the CPU
emulation of the kernels' arithmetic meets the bound and that a wrong backward misses it by three orders of magnitude.
Each case prints the kernel's worst error as a fraction of the bound (run with -s)."""
import ctypes

import pytest
import torch

import _norm_train_ref as R
import _synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NORM_NODE, JOIN_NODE = "_InstanceNormFnBackward", "_InstanceNormAddReluFnBackward"
#: weight draws of test_encoder_wiring, tried in order (see its docstring)
WIRING_SEEDS = tuple(range(5, 17))


def G(t):
    return t.contiguous().to(DEV)


def _call(fn, what, *args):
    from dkt_stereo_amd import _ffi
    _ffi.check(fn(*args), what)


def _ws(x):
    from dkt_stereo_amd import _ffi
    n, c, h, w = x.shape
    return torch.empty(_ffi.lib().dkt_instance_norm_workspace(n * c, h * w), device=x.device, dtype=torch.uint8)


def _inference_norm(x, relu):
    """dkt_instance_norm itself on the same tensor."""
    from dkt_stereo_amd import _ffi
    n, c, h, w = x.shape
    y, ws = torch.empty_like(x), _ws(x)
    _call(_ffi.lib().dkt_instance_norm, "dkt_instance_norm", x.data_ptr(), y.data_ptr(), ws.data_ptr(), n * c, h * w, R.EPS,
          int(relu), _ffi.device_of(x), _ffi.stream_of(x))
    return y


def _inference_join(a, c):
    """dkt_instance_norm_stats + dkt_instance_norm_add_relu on the same tensors."""
    from dkt_stereo_amd import _ffi
    n, ch, h, w = c.shape
    y, ws = torch.empty_like(c), _ws(c)
    L, dev, st = _ffi.lib(), _ffi.device_of(c), _ffi.stream_of(c)
    _call(L.dkt_instance_norm_stats, "dkt_instance_norm_stats", c.data_ptr(), ws.data_ptr(), n * ch, h * w, dev, st)
    _call(L.dkt_instance_norm_add_relu, "dkt_instance_norm_add_relu", a.data_ptr(), c.data_ptr(), y.data_ptr(), ws.data_ptr(),
          n * ch, h * w, R.EPS, dev, st)
    return y


def _upstream(g, how):
    """The upstream gradient contiguous, as a channel slice of a wider buffer, or as a transposed view."""
    if how == "slice":
        buf = torch.full((g.shape[0], g.shape[1] + 3) + tuple(g.shape[2:]), 9.0, device=g.device)
        buf[:, 2:2 + g.shape[1]] = g
        return buf[:, 2:2 + g.shape[1]]
    if how == "transposed":
        return g.transpose(2, 3).contiguous().transpose(2, 3)
    return g


def _run_norm(x, gy, relu, up="contiguous"):
    from dkt_stereo_amd.norm_train import instance_norm
    xd = G(x).requires_grad_(True)
    y = instance_norm(xd, R.EPS, relu)
    assert type(y.grad_fn).__name__ == NORM_NODE
    y.backward(_upstream(G(gy), up))
    return y.detach(), xd.grad


def _run_join(a, c, gout, need="both", up="contiguous"):
    from dkt_stereo_amd.norm_train import instance_norm_add_relu
    ad = G(a).requires_grad_(need in ("both", "a"))
    cd = G(c).requires_grad_(need in ("both", "c"))
    out = instance_norm_add_relu(ad, cd, R.EPS)
    assert type(out.grad_fn).__name__ == JOIN_NODE
    out.backward(_upstream(G(gout), up))
    return out.detach(), ad.grad, cd.grad


def _check_norm(name, relu, up="contiguous"):
    x, gy, _ = R.inputs(R.CASES[name])
    y, gx = _run_norm(x, gy, relu, up)
    assert torch.equal(y, _inference_norm(G(x), relu)), name                      # forward: the same bits
    mask = (y > 0).cpu() if relu else None
    exact, bound, _, _ = R.truth_and_bound(gy, x, mask)
    ratio = R.worst(gx, exact, bound)
    print("%-14s norm%s %-10s %.3f of the bound" % (name, "+relu" if relu else "     ", up, ratio))
    assert ratio <= 1.0, (name, relu, up, ratio)
    return y, gx


def _check_join(name, need="both", up="contiguous"):
    c, gout, a = R.inputs(R.CASES[name])
    out, ga, gc = _run_join(a, c, gout, need, up)
    assert torch.equal(out, _inference_join(G(a), G(c))), name
    assert (ga is None) == (need == "c") and (gc is None) == (need == "a"), name
    if ga is not None:
        assert torch.equal(ga, G(gout) * (out > 0)), name                         # exact
    if gc is not None:
        mask = ((out > 0) & (_inference_norm(G(c), True) > 0)).cpu()
        exact, bound, _, _ = R.truth_and_bound(gout, c, mask)
        ratio = R.worst(gc, exact, bound)
        print("%-14s join %-4s %-10s %.3f of the bound" % (name, need, up, ratio))
        assert ratio <= 1.0, (name, need, up, ratio)
    return out, ga, gc


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("name", list(R.CASES))
def test_norm_fixed_cases(name, relu):
    """Forward bits, the gradient under the bound, a second run bit-identical."""
    first = _check_norm(name, relu)
    x, gy, _ = R.inputs(R.CASES[name])
    assert all(R.same(p, q) for p, q in zip(first, _run_norm(x, gy, relu))), name
    if name == "constant" and relu:
        assert float(first[1].abs().max()) == 0.0


@pytest.mark.parametrize("name", list(R.CASES))
def test_join_fixed_cases(name):
    first = _check_join(name)
    c, gout, a = R.inputs(R.CASES[name])
    assert all(R.same(p, q) for p, q in zip(first, _run_join(a, c, gout))), name
    frac = float((first[0] > 0).float().mean())
    if name not in R.DEGENERATE and first[0].numel() > 100:
        assert 0.3 <= frac <= 0.7, (name, frac)                                   # roughly half of the join is cut off


@pytest.mark.parametrize("name", ["odd", "slices_partial", "aligned"])
@pytest.mark.parametrize("need", ["a", "c"])
def test_join_needs_input_grad_subsets(name, need):
    """One gradient alone (for `a`: the single launch without sums) is bit-identical to the same gradient beside the other."""
    _, ga, gc = _check_join(name, need=need)
    c, gout, a = R.inputs(R.CASES[name])
    _, ba, bc = _run_join(a, c, gout)
    assert R.same(ga, ba) if need == "a" else R.same(gc, bc)


@pytest.mark.parametrize("name", ["odd", "slices_partial", "aligned"])
@pytest.mark.parametrize("up", ["slice", "transposed"])
def test_non_contiguous_upstream(name, up):
    x, gy, a = R.inputs(R.CASES[name])
    got = _check_norm(name, True, up=up)
    assert all(R.same(p, q) for p, q in zip(got, _run_norm(x, gy, True)))
    got = _check_join(name, up=up)
    assert all(R.same(p, q) for p, q in zip(got, _run_join(a, x, gy)))


def test_split_rule_and_workspace():
    """The sums launch of the slice cases takes more than one block per plane, by the rule the emulation mirrors."""
    from dkt_stereo_amd import _ffi
    for name, c in R.CASES.items():
        n, ch, h, w = c["shape"]
        nbytes = _ffi.lib().dkt_instance_norm_bwd_workspace(n * ch, h * w)
        assert nbytes == n * ch * R.split(n * ch, h * w) * 16, name
        assert (nbytes > n * ch * 16) == (name in R.SPLIT_CASES), name


def test_abi_names_and_argument_errors():
    """The entries are exported and refuse bad arguments before any launch."""
    from dkt_stereo_amd import _ffi
    lib = _ffi.lib()
    bwd, join = lib.dkt_instance_norm_bwd, lib.dkt_instance_norm_add_relu_bwd
    assert {"dkt_instance_norm_bwd", "dkt_instance_norm_add_relu_bwd", "dkt_instance_norm_bwd_workspace"} <= set(_ffi.SIGNATURES)
    null = ctypes.c_void_p(0)
    buf = torch.zeros(4096, device=DEV)
    p = ctypes.c_void_p(buf.data_ptr())
    assert bwd(null, p, p, 1, p, p, 2, 8, -1, null) == -1
    assert bwd(p, null, p, 1, p, p, 2, 8, -1, null) == -1
    assert bwd(p, p, null, 1, p, p, 2, 8, -1, null) == -1
    assert bwd(p, p, p, 1, null, p, 2, 8, -1, null) == -1
    assert bwd(p, p, p, 1, p, null, 2, 8, -1, null) == -1
    assert bwd(p, p, p, 1, p, p, 0, 8, -1, null) == -2
    assert bwd(p, p, p, 1, p, p, 2, 0, -1, null) == -2
    assert bwd(p, p, p, 1, p, p, 65536, 8, -1, null) == -2
    assert join(null, p, p, p, p, p, p, 2, 8, -1, null) == -1
    assert join(p, null, p, p, p, p, p, 2, 8, -1, null) == -1
    assert join(p, p, p, p, null, null, p, 2, 8, -1, null) == -1        # neither gradient wanted
    assert join(p, p, null, p, null, p, p, 2, 8, -1, null) == -1        # gc needs c, the statistics and the workspace
    assert join(p, p, p, null, null, p, p, 2, 8, -1, null) == -1
    assert join(p, p, p, p, null, p, null, 2, 8, -1, null) == -1
    assert join(p, p, p, p, p, p, p, 0, 8, -1, null) == -2
    assert join(p, p, p, p, p, p, p, 2, 0, -1, null) == -2
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0                                # nothing ran


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max())


def test_encoder_wiring(monkeypatch):
    """BasicEncoder(norm_fn='instance', downsample=2) at 2 x 3 x 32 x 64, every parameter trainable: with the handle on
    every norm, join and projection norm is a node; output and parameter gradients agree with the handle-off (torch) run.

    The encoder is piecewise linear in its parameters, and the gradient jumps where a pre-ReLU value changes sign.  Two
    fp32 evaluations that put ONE of the ~2 million activations on different sides of 0 differ by 1e-2 in these
    gradients (on the CPU, torch's own fp32 against its fp64 run: 1.7e-6, 1.1e-2 and 9.4e-2 at three weight draws; on
    the device the two arms were 8.7e-3 apart on conv1.weight at seed 5), so the gradients are compared at the first of
    WIRING_SEEDS at which both forwards took the same ReLU masks -- a property of the forwards alone, which are held to
    the inference kernels bit for bit above.  The node types and the forward are checked at every draw on the way."""
    from dkt_stereo_amd import extractor
    x = G(torch.from_numpy(_synth.uniform((2, 3, 32, 64), -1.0, 1.0, 21, "image")))
    wl = G(torch.from_numpy(_synth.normal((2, 128, 8, 16), 21, "loss")))
    seen, masks = [], []
    inner_act, inner_join = extractor.norm_act, extractor.norm_add_relu

    nested = []

    def spy_act(norm, t, relu):
        y = inner_act(norm, t, relu)
        if not nested:                                  # (the torch join calls norm_act itself: a mask, not a layer)
            seen.append((type(y.grad_fn).__name__, bool(relu)))
        if relu:
            masks.append((y > 0).detach())
        return y

    def spy_join(norm, a, c, c_stats=None):
        nested.append(1)
        try:
            y = inner_join(norm, a, c, c_stats)
        finally:
            nested.pop()
        if type(y.grad_fn).__name__ == JOIN_NODE:       # the node's inner ReLU mask: the inference kernel's, bit for bit
            masks.append(_inference_norm(c.detach().contiguous(), True) > 0)
        seen.append((type(y.grad_fn).__name__, None))
        masks.append((y > 0).detach())
        return y

    monkeypatch.setattr(extractor, "norm_act", spy_act)
    monkeypatch.setattr(extractor, "norm_add_relu", spy_join)
    for seed in WIRING_SEEDS:
        torch.manual_seed(seed)
        fnet = extractor.BasicEncoder(output_dim=128, norm_fn="instance", downsample=2).to(DEV).train()
        params = list(fnet.parameters())
        assert all(p.requires_grad for p in params)
        runs = {}
        for handle in (True, False):
            monkeypatch.setattr(extractor, "TRAIN_NORM_NODES", handle)
            del seen[:], masks[:]
            y = fnet(x)
            runs[handle] = (y.detach(), torch.autograd.grad((y * wl).sum(), params), list(seen), list(masks))
        # the stem, 6 x norm1, 2 x norm3 (relu=False), 6 joins
        names = runs[True][2]
        assert sorted(names) == sorted([(NORM_NODE, True)] * 7 + [(NORM_NODE, False)] * 2 + [(JOIN_NODE, None)] * 6), names
        assert not any(n in (NORM_NODE, JOIN_NODE) for n, _ in runs[False][2]), runs[False][2]
        err = _rel(runs[True][0], runs[False][0])
        assert [m.shape for m in runs[True][3]] == [m.shape for m in runs[False][3]] and len(runs[True][3]) == 19
        flips = sum(int((p != q).sum()) for p, q in zip(runs[True][3], runs[False][3]))
        print("seed %d: fnet forward, nodes against torch %.2e, activations of different sign %d" % (seed, err, flips))
        assert err <= 1e-5, (seed, err)
        if flips == 0:
            break
    else:
        raise AssertionError("no draw of WIRING_SEEDS at which the two forwards take the same ReLU masks")
    # A bias in front of an affine-free instance norm has a gradient of exactly 0 (the norm removes the plane's mean):
    # what either run returns for it is rounding residue, and a ratio of two residues says nothing.  Those differences
    # are held to the same 5e-4 of the scale of the layer's weight gradient (sums of the same upstream gradient against
    # inputs of order 1); every other parameter, conv2.bias included, to 5e-4 of its own gradient.
    named = dict(zip((n for n, _ in fnet.named_parameters()), zip(runs[True][1], runs[False][1])))
    errs = {}
    for n, (a, b) in named.items():
        if n.endswith(".bias") and n != "conv2.bias":
            scale = float(named[n[:-4] + "weight"][1].abs().max())
            errs[n] = float((a.double() - b.double()).abs().max()) / scale
        else:
            errs[n] = _rel(a, b)
        print("  %-28s %.2e" % (n, errs[n]))
    assert max(errs.values()) <= 5e-4, {n: e for n, e in errs.items() if e > 5e-4}
    with torch.no_grad():                                               # without autograd nothing changes: the inference kernels
        monkeypatch.setattr(extractor, "TRAIN_NORM_NODES", True)
        on = fnet(x)
        monkeypatch.setattr(extractor, "TRAIN_NORM_NODES", False)
        assert torch.equal(on, fnet(x)) and on.grad_fn is None


def test_untouched_paths(monkeypatch):
    """Inputs that do not require grad and disabled autograd keep the inference launches; other norms stay on torch."""
    from dkt_stereo_amd import _ffi, extractor
    monkeypatch.setattr(extractor, "TRAIN_NORM_NODES", True)
    norm = torch.nn.InstanceNorm2d(4)
    x, _, a = (G(t) for t in R.inputs(R.CASES["odd_mean"]))
    with _ffi.launch_log() as names:
        y = extractor.norm_act(norm, x, True)
        z = extractor.norm_add_relu(norm, a, x)
        with torch.no_grad():
            extractor.norm_act(norm, x.clone().requires_grad_(True), True)
    assert names == ["dkt_instance_norm", "dkt_instance_norm_stats", "dkt_instance_norm_add_relu", "dkt_instance_norm"]
    assert y.grad_fn is None and z.grad_fn is None
    affine = torch.nn.InstanceNorm2d(4, affine=True).to(DEV)
    assert type(extractor.norm_act(affine, x.clone().requires_grad_(True), True).grad_fn).__name__ == "ReluBackward0"
    # one operand of the join requires grad: still the node
    z = extractor.norm_add_relu(norm, a.clone().requires_grad_(True), x)
    assert type(z.grad_fn).__name__ == JOIN_NODE


def test_raft_training_step_through_the_nodes(monkeypatch):
    """One RAFTStereo step with test_mode=False at 64 x 128, 2 iterations, the feature encoder trainable: finite
    predictions, finite and non-zero fnet gradients."""
    import _cases
    from dkt_stereo_amd import extractor
    from dkt_stereo_amd.raft_stereo import RAFTStereo, make_args
    monkeypatch.setattr(extractor, "TRAIN_NORM_NODES", True)
    model = RAFTStereo(make_args())
    model.load_state_dict(_synth.torch_state_dict(_synth.shapes_of(model), _cases.E2E_WEIGHT_SEED), strict=True)
    model.to(DEV).eval()
    for n, p in model.named_parameters():
        p.requires_grad_(n.startswith("fnet."))
    i1, i2 = (G(torch.from_numpy(t)) for t in _synth.image_pair(5, 1, 64, 128, 12))
    preds = model(i1, i2, iters=2, test_mode=False)["disp_preds"]
    assert len(preds) == 2 and all(bool(torch.isfinite(p).all()) for p in preds)
    fparams = [p for n, p in model.named_parameters() if n.startswith("fnet.")]
    grads = torch.autograd.grad(sum(p.abs().mean() for p in preds), fparams)
    assert all(bool(torch.isfinite(g).all()) for g in grads)
    assert float(grads[0].abs().max()) > 0.0
    node = preds[-1].grad_fn
    found, stack, visited = set(), [node], set()
    while stack:                                                        # the graph behind the predictions holds the nodes
        f = stack.pop()
        if f is None or f in visited:
            continue
        visited.add(f)
        found.add(type(f).__name__)
        stack.extend(nf for nf, _ in f.next_functions)
    assert NORM_NODE in found and JOIN_NODE in found
