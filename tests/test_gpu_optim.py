"""optim.AdamW / dkt_adamw_step on the device against the fp64 truth of one step (tests/_optim_ref.py: cases, bounds and
their derivation), the GradScaler contract, torch's state-dict layout, OneCycleLR, and the refresh that keeps a training
RAFT-Stereo warm across optimizer steps.  Every comparison is of a single step from a stated fp32 state."""
import copy
import ctypes
import gc
import warnings

import pytest
import torch
import torch.nn as nn

import _encoder_ref as E
import _optim_ref as O
import _raft_train_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
#: warm against fresh predictions: test_gpu_ema.py's BOUND, the contract bound of test_calibration_stress_twenty_pairs (max-abs
#: of the up-sampled disparity between two valid split-fp16 scalings of the same weights)
WARM_BOUND = 1e-3


@pytest.fixture(autouse=True)
def _collect():
    gc.collect()
    yield


def G(ts):
    return [t.clone().to(DEV) for t in ts]


class _Syncs:
    """Counts torch's synchronising calls inside the block (as test_gpu_ema.py::test_one_sync_per_update counts them)."""

    def __enter__(self):
        torch.cuda.synchronize()
        self.cm = warnings.catch_warnings(record=True)
        self.rec = self.cm.__enter__()
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        return self

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode(0)
        hits = [r for r in self.rec if "called a synchronizing" in str(r.message)]
        self.msgs = [str(r.message) for r in hits]
        self.where = ["%s:%d" % (r.filename.rsplit("/", 1)[-1], r.lineno) for r in hits]
        self.n = len(self.msgs)
        return self.cm.__exit__(*exc)


def _raw(name, grid=0, poison_fix=None, **override):
    """One dkt_adamw_step of a case through the raw entry: dict(p, m, v, step, total_norm, clip, skipped, absmax)."""
    from dkt_stereo_amd import optim
    p, g, m, v, c = O.state(name)
    dp, dg, dm, dv = G(p), G(g), G(m), G(v)
    step = torch.tensor(float(c["step"]), device=DEV)
    record = torch.zeros(4, device=DEV)
    ws = torch.zeros(optim.workspace_bytes(len(p), sum(O.SIZES)), device=DEV, dtype=torch.uint8)
    absmax = torch.full((len(p),), -1.0, device=DEV)
    kw = dict(lr=c["lr"], betas=O.BETAS, eps=c["eps"], weight_decay=c["wd"], max_norm=c["max_norm"],
              inv_scale=c.get("inv_scale", 1.0), absmax=absmax, grid=grid)
    kw.update(override)
    optim.adamw_kernel(dp, dg, dm, dv, step, record, ws, **kw)
    out = _result(dp, dm, dv, step, record, absmax)
    if poison_fix is not None:                     # the following finite step, from the state the skipped one left
        last = max(k for k, n in enumerate(O.SIZES) if n)
        dg[last][-1] = poison_fix
        optim.adamw_kernel(dp, dg, dm, dv, step, record, ws, **kw)
        out["next"] = _result(dp, dm, dv, step, record, absmax)
        out["next_g"] = [t.cpu() for t in dg]
    assert not bool(ws[:8].any())                  # the flag and the ticket are left cleared
    return out


def _result(dp, dm, dv, step, record, absmax):
    rec = record.cpu().tolist()
    return dict(p=[t.cpu() for t in dp], m=[t.cpu() for t in dm], v=[t.cpu() for t in dv], step=int(step.item()),
                total_norm=rec[0], clip=rec[1], skipped=int(rec[2]), absmax=absmax.cpu())


def _check(name, got, through):
    p, g, m, v, c = O.state(name)
    t = O.truth(p, g, m, v, c)
    plain = c["max_norm"] is None and c.get("inv_scale", 1.0) == 1.0
    if plain:
        assert got["total_norm"] == -1.0 and got["clip"] == 1.0       # the single launch takes no norm
    res = dict(got, total_norm=None if plain or t["skipped"] else got["total_norm"])
    x = O.excess(res, t, p, m, v, c["step"])
    print("%s through %s: %.3g of the bound; total_norm %.9g (truth %.9g), clip %.9g (truth %.9g), skipped %d" %
          (name, through, x, got["total_norm"], t["total_norm"], got["clip"], t["clip"], got["skipped"]))
    assert x <= 1.0
    assert got["skipped"] == t["skipped"]
    if not t["skipped"] and not plain:
        assert abs(got["clip"] - t["clip"]) <= 6 * O.EPS32 * t["clip"]        # (the docstring's count; exactly 1 when clamped)
        if t["clip"] == 1.0:
            assert got["clip"] == 1.0
    if got.get("absmax") is not None:
        want = torch.tensor([float(q.abs().max()) if q.numel() else 0.0 for q in got["p"]])
        assert torch.equal(got["absmax"], want)


# ---- the kernel against the truth ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(O.CASES))
def test_kernel_vs_truth_raw_entry(name):
    _check(name, _raw(name), "dkt_adamw_step")


def _optimizer(name, module=None):
    """optim.AdamW over a case's tensors, its state loaded from torch's state-dict layout; (opt, params, case)."""
    from dkt_stereo_amd import optim
    p, g, m, v, c = O.state(name)
    ps = [nn.Parameter(t) for t in G(p)]
    for q, gk in zip(ps, G(g)):
        q.grad = gk
    opt = optim.AdamW(ps, max_norm=c["max_norm"], module=module, **O.hyper(c))
    sd = opt.state_dict()
    sd["state"] = {i: dict(step=torch.tensor(float(c["step"])), exp_avg=mk.clone(), exp_avg_sq=vk.clone())
                   for i, (mk, vk) in enumerate(zip(m, v))}
    opt.load_state_dict(sd)
    if c.get("inv_scale", 1.0) != 1.0:             # what GradScaler.step leaves on the optimizer
        opt.grad_scale = torch.tensor(1.0 / c["inv_scale"], device=DEV)
        opt.found_inf = torch.zeros((), device=DEV)
    return opt, ps, c


@pytest.mark.parametrize("name", sorted(O.CASES))
def test_optimizer_step_vs_truth(name):
    opt, ps, c = _optimizer(name)
    grads = [q.grad.clone() for q in ps]
    versions = [q._version for q in ps]
    with _Syncs() as s:
        total_norm, clip, skipped = opt.step()
    assert s.n == 0, s.msgs
    assert [q._version for q in ps] == [v + 1 for v in versions]     # one bump each: whatever is keyed on them goes stale
    for q, g0 in zip(ps, grads):                                      # .grad is not rewritten
        assert torch.equal(q.grad.view(torch.int32), g0.view(torch.int32))
    st = [opt.state[q] for q in ps]
    got = dict(p=[q.detach().cpu() for q in ps], m=[s_["exp_avg"].cpu() for s_ in st], v=[s_["exp_avg_sq"].cpu() for s_ in st],
               step=int(st[0]["step"].item()), total_norm=float(total_norm), clip=float(clip), skipped=int(skipped))
    _check(name, got, "optim.AdamW.step")


@pytest.mark.parametrize("name", ["clip", "scale", "plain1000", "inf"])
def test_deterministic_and_grid_independent(name):
    a = _raw(name)
    for grid in (0, 1, 3, 4096):
        b = _raw(name, grid=grid)
        for key in "pmv":
            for x, y in zip(a[key], b[key]):
                assert torch.equal(x, y), (grid, key)
        assert torch.equal(a["absmax"], b["absmax"])
        assert (a["step"], a["skipped"]) == (b["step"], b["skipped"])
        if name != "inf":
            assert (a["total_norm"], a["clip"]) == (b["total_norm"], b["clip"])


def test_infinite_max_norm_reports_the_norm_only():
    """max_norm = inf is clip_grad_norm_'s 'tell me the norm': the three launches run, clip is 1 and the update is the
    unclipped one bit for bit."""
    name = "plain1000"
    p, g, m, v, c = O.state(name)
    a, b = _raw(name), _raw(name, max_norm=float("inf"))
    for key in "pmv":
        for x, y in zip(a[key], b[key]):
            assert torch.equal(x, y)
    t = O.truth(p, g, m, v, c)
    assert b["clip"] == 1.0 and b["skipped"] == 0 and b["step"] == a["step"]
    assert abs(b["total_norm"] - t["total_norm"]) <= O.norm_tol(t)


@pytest.mark.parametrize("name", O.POISONED)
def test_skip_then_first_step(name):
    p, g, m, v, c = O.state(name)
    got = _raw(name, poison_fix=0.5 * c["sigma"])
    assert got["skipped"] == 1 and got["step"] == c["step"]
    for key, ref in (("p", p), ("m", m), ("v", v)):
        for a, b in zip(got[key], ref):
            assert torch.equal(a, b)
    nxt = got["next"]
    t = O.truth(p, got["next_g"], m, v, c)
    x = O.excess(nxt, t, p, m, v, c["step"])
    print("%s: the finite step after the skipped one at %.3g of the bound, step %d" % (name, x, nxt["step"]))
    assert nxt["skipped"] == 0 and nxt["step"] == c["step"] + 1 and x <= 1.0


# ---- GradScaler ---------------------------------------------------------------------------------------------------------------
def _two_layer(seed):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(37, 64), nn.ReLU(), nn.Linear(64, 5)).to(DEV)


@pytest.mark.parametrize("overflow", [False, True])
def test_grad_scaler_contract(overflow):
    from dkt_stereo_amd import optim
    hy = dict(lr=2e-4, weight_decay=1e-5, eps=1e-8)
    mine, ref = _two_layer(3), _two_layer(3)
    torch.manual_seed(4)
    x = torch.randn(16, 37, device=DEV)
    opt, topt = optim.AdamW(mine.parameters(), max_norm=1.0, **hy), torch.optim.AdamW(ref.parameters(), **hy)
    sc, tsc = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16), torch.amp.GradScaler("cuda", init_scale=2.0 ** 16)
    p0 = [q.detach().cpu().clone() for q in mine.parameters()]

    sc.scale(mine(x).square().mean() * 30).backward()
    if overflow:
        next(mine.parameters()).grad[0, 0] = float("inf")
    g = [q.grad.detach().cpu().clone() for q in mine.parameters()]
    with _Syncs() as s:
        sc.step(opt)
    sc.update()
    print("scaler.step(optim.AdamW): %d synchronising call(s)" % s.n)
    assert s.n == 0, s.msgs

    tsc.scale(ref(x).square().mean() * 30).backward()              # the reference sequence, tools/ft_dkt.py:242-248
    if overflow:
        next(ref.parameters()).grad[0, 0] = float("inf")
    tsc.unscale_(topt)
    torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0)
    tsc.step(topt)
    tsc.update()

    assert float(sc.get_scale()) == float(tsc.get_scale()) == (2.0 ** 15 if overflow else 2.0 ** 16)
    c = dict(lr=hy["lr"], wd=hy["weight_decay"], eps=hy["eps"], step=0, max_norm=1.0, inv_scale=2.0 ** -16)
    zeros = [torch.zeros_like(q) for q in p0]
    t = O.truth(p0, g, zeros, zeros, c)
    got = [q.detach().cpu() for q in mine.parameters()]
    if overflow:
        assert t["skipped"] == 1 and float(opt._record[2]) == 1.0 and int(opt._step_t.item()) == 0
        for a, b, r in zip(got, p0, ref.parameters()):
            assert torch.equal(a, b) and torch.equal(r.detach().cpu(), b)
        return
    tol = O.bounds(p0, t)[0]
    for a, w, r, tl in zip(got, t["p"], ref.parameters(), tol):
        assert bool(((a.double() - w).abs() <= tl).all())                               # against the truth
        assert bool(((a.double() - r.detach().cpu().double()).abs() <= tl).all())       # against the reference sequence
    print("total_norm %.6g, clip %.6g (truth %.6g, %.6g)" % (float(opt._record[0]), float(opt._record[1]), t["total_norm"], t["clip"]))


def test_scaler_unscaled_first():
    """The caller ran scaler.unscale_ itself: grad_scale arrives as None, found_inf comes from the scaler."""
    from dkt_stereo_amd import optim
    mine = _two_layer(5)
    x = torch.randn(8, 37, device=DEV)
    opt = optim.AdamW(mine.parameters(), lr=1e-3, max_norm=1.0)
    sc = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10)
    p0 = [q.detach().cpu().clone() for q in mine.parameters()]
    sc.scale(mine(x).square().mean()).backward()
    sc.unscale_(opt)
    g = [q.grad.detach().cpu().clone() for q in mine.parameters()]
    sc.step(opt)
    sc.update()
    c = dict(lr=1e-3, wd=1e-2, eps=1e-8, step=0, max_norm=1.0)
    zeros = [torch.zeros_like(q) for q in p0]
    t = O.truth(p0, g, zeros, zeros, c)
    for a, w, tl in zip(mine.parameters(), t["p"], O.bounds(p0, t)[0]):
        assert bool(((a.detach().cpu().double() - w).abs() <= tl).all())
    assert int(opt._step_t.item()) == 1


# ---- state dict, scheduler ----------------------------------------------------------------------------------------------------
SMALL = [7, 4097, 33]


def _small(seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=gen) * (k + 1) for k, n in enumerate(SMALL)]


def _grads(seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=gen) * 0.02 for n in SMALL]


def _snapshot(opt, ps):
    return ([q.detach().cpu().clone() for q in ps], [opt.state[q]["exp_avg"].cpu().clone() for q in ps],
            [opt.state[q]["exp_avg_sq"].cpu().clone() for q in ps])


def test_state_dict_round_trip_with_torch():
    from dkt_stereo_amd import optim
    hy = dict(lr=1e-2, weight_decay=1e-1, eps=1e-8)
    ps = [nn.Parameter(t) for t in G(_small(1))]
    opt = optim.AdamW(ps, max_norm=1.0, **hy)
    for i in range(3):
        for q, gk in zip(ps, G(_grads(10 + i))):
            q.grad = gk
        opt.step()
    p3, m3, v3 = _snapshot(opt, ps)
    g4 = _grads(13)
    t = O.truth(p3, g4, m3, v3, dict(lr=hy["lr"], wd=hy["weight_decay"], eps=hy["eps"], step=3, max_norm=1.0))
    tol = O.bounds(p3, t)[0]

    tps = [nn.Parameter(t_.clone()) for t_ in G(p3)]                  # ours -> torch
    topt = torch.optim.AdamW(tps, **hy)
    topt.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert all(float(topt.state[q]["step"]) == 3 for q in tps)
    ops = [nn.Parameter(t_.clone()) for t_ in G(p3)]                  # torch -> ours
    opt2 = optim.AdamW(ops, max_norm=1.0, **hy)
    opt2.load_state_dict(copy.deepcopy(topt.state_dict()))
    assert all(float(opt2.state[q]["step"]) == 3 for q in ops) and float(opt.state[ps[0]]["step"]) == 3
    for q, mk, vk in zip(ops, m3, v3):
        assert torch.equal(opt2.state[q]["exp_avg"].cpu(), mk) and torch.equal(opt2.state[q]["exp_avg_sq"].cpu(), vk)

    for params in (tps, ops, ps):
        for q, gk in zip(params, G(g4)):
            q.grad = gk
    torch.nn.utils.clip_grad_norm_(tps, 1.0)
    topt.step()
    opt2.step()
    opt.step()
    for side, params in (("torch", tps), ("loaded", ops), ("original", ps)):
        for a, w, tl in zip(params, t["p"], tol):
            assert bool(((a.detach().cpu().double() - w).abs() <= tl).all()), side
    assert float(topt.state[tps[0]]["step"]) == 4 and float(opt2.state[ops[0]]["step"]) == 4
    for a, b in zip(ops, ps):
        assert torch.equal(a, b)                                      # the loaded optimizer continues bit for bit


def test_one_cycle_lr_drives_the_kernel():
    from dkt_stereo_amd import optim
    ps = [nn.Parameter(t) for t in G(_small(2))]
    opt = optim.AdamW(ps, lr=2e-4, weight_decay=1e-5, eps=1e-8, max_norm=1.0)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, 2e-4, 110, pct_start=0.01, cycle_momentum=False, anneal_strategy="linear")
    seen = []
    for i in range(10):
        lr = sched.get_last_lr()[0]
        for q, gk in zip(ps, G(_grads(20 + i))):
            q.grad = gk
        if i == 0:
            p0, m0, v0 = [q.detach().cpu().clone() for q in ps], [torch.zeros(n) for n in SMALL], [torch.zeros(n) for n in SMALL]
        else:
            p0, m0, v0 = _snapshot(opt, ps)
        opt.step()
        sched.step()
        assert opt.last_lr == lr
        seen.append(lr)
        t = O.truth(p0, _grads(20 + i), m0, v0, dict(lr=lr, wd=1e-5, eps=1e-8, step=i, max_norm=1.0))
        tp, tm, tv = O.bounds(p0, t)
        for a, w, tl in zip(ps, t["p"], tp):
            assert bool(((a.detach().cpu().double() - w).abs() <= tl).all()), i
        for q, w, tl in zip(ps, t["m"], tm):
            assert bool(((opt.state[q]["exp_avg"].cpu().double() - w).abs() <= tl).all()), i
    dummy = torch.optim.AdamW([nn.Parameter(torch.zeros(1))], lr=2e-4)          # the same schedule on torch's optimizer
    ref = torch.optim.lr_scheduler.OneCycleLR(dummy, 2e-4, 110, pct_start=0.01, cycle_momentum=False, anneal_strategy="linear")
    want = []
    for _ in range(10):
        want.append(ref.get_last_lr()[0])
        dummy.step()
        ref.step()
    assert seen == want and len(set(seen)) == 10
    assert int(opt._step_t.item()) == 10


def test_added_param_group_is_stepped():
    """A group added after construction (larger than everything before it: the workspace grows) takes the same step."""
    from dkt_stereo_amd import optim
    hy = dict(lr=1e-2, weight_decay=1e-1, eps=1e-8)
    small, big = _small(3), [torch.randn(3 * 2048 + 5, generator=torch.Generator().manual_seed(4))]
    ps = [nn.Parameter(t) for t in G(small)]
    opt = optim.AdamW(ps, max_norm=1.0, **hy)
    more = [nn.Parameter(t) for t in G(big)]
    opt.add_param_group(dict(params=more))
    g = _grads(30) + [torch.randn(3 * 2048 + 5, generator=torch.Generator().manual_seed(5)) * 0.02]
    for q, gk in zip(ps + more, G(g)):
        q.grad = gk
    opt.step()
    p0 = small + big
    zeros = [torch.zeros_like(t) for t in p0]
    t = O.truth(p0, g, zeros, zeros, dict(lr=hy["lr"], wd=hy["weight_decay"], eps=hy["eps"], step=0, max_norm=1.0))
    for a, w, tl in zip(ps + more, t["p"], O.bounds(p0, t)[0]):
        assert bool(((a.detach().cpu().double() - w).abs() <= tl).all())


def test_refusals():
    from dkt_stereo_amd import _ffi, optim
    with pytest.raises(_ffi.DktError):
        optim.AdamW([nn.Parameter(torch.zeros(4, device=DEV, dtype=torch.float64))])
    with pytest.raises(_ffi.DktError):
        optim.AdamW([nn.Parameter(torch.zeros(4, 6, device=DEV).t())])
    q = nn.Parameter(torch.zeros(4, 3, device=DEV))
    opt = optim.AdamW([q])
    with pytest.raises(_ffi.DktError):                                 # parameters added later meet the same checks
        opt.add_param_group(dict(params=[nn.Parameter(torch.zeros(4))]))
    q.grad = torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.tensor([1.0]), (4, 3)).to(DEV)
    with pytest.raises(_ffi.DktError):
        opt.step()


# ---- the warm student ---------------------------------------------------------------------------------------------------------
def _nodes_on(mp):
    from dkt_stereo_amd import conv, extractor
    from dkt_stereo_amd.update import BasicMultiUpdateBlock
    mp.setattr(extractor, "TRAIN_NORM_NODES", True)
    mp.setattr(extractor, "TRAIN_CONV_NODES", True)
    mp.setattr(BasicMultiUpdateBlock, "TRAIN_NODES", True)
    mp.setattr(conv, "GRAD_PREPASS", True)
    mp.setattr(conv, "GRAD_WEIGHT_HIP", True)


def _student(seed=0):
    model = E.make_raft({}, 100 + seed).to(DEV)
    model.train()
    model.freeze_bn()
    _, i1, i2, ws = R.model_and_inputs((), seed)
    return model, i1.to(DEV), i2.to(DEV), ws


def _fwd_bwd(model, i1, i2, ws):
    preds, grads, _ = R.model_step(model, i1, i2, ws, R.MaskSpy())
    for n, p in model.named_parameters():
        p.grad = grads.get(n)
    return preds


class _ColdPacks:
    """Counts conv.pack_scale calls: each is a cold pack of conv._packed_weights / stem7_packed, after a host read of max|w|."""

    def __init__(self, mp):
        from dkt_stereo_amd import conv
        self.n = 0
        inner = conv.pack_scale

        def counted(wmax):
            self.n += 1
            return inner(wmax)
        mp.setattr(conv, "pack_scale", counted)


def _current(key, w):
    return key.tensors[0] == (w.data_ptr(), w._version)


def _packed_layers(model):
    return [(n, m) for n, m in model.named_modules() if m.__dict__.get("_dkt_packed") or m.__dict__.get("_dkt_stem7")]


def _holders(model):
    """Everything that may hold a cache, breadth first, as ema._refresh walks it: the modules, the derived layers cached
    below them (folded, merged, z|r, views, scaled) and the input-gradient layers of conv._grad_layer.  [(holder, owner)]:
    `owner` is the layer an input-gradient layer derives from, else None."""
    todo, out, seen = [(m, None) for m in model.modules()], [], set()
    while todo:
        h, owner = todo.pop(0)
        if id(h) in seen:
            continue
        seen.add(id(h))
        out.append((h, owner))
        d = h.__dict__
        for name in ("_dkt_folded", "_dkt_merged", "_zr_cache", "_dkt_view", "_dkt_scaled"):
            todo += [(e, None) for lst in (d.get(name) or {}).values() for e in lst]
        todo += [(e.value, h) for lst in (d.get("_dkt_grad") or {}).values() for e in lst if _current(e.key, h.weight)]
    return out


def _check_packs_cold_equal(model):
    """Every current split-fp16 image below `model` == a cold dkt_conv2d_pack_weights / dkt_conv2d_stem7_pack of its holder's
    current weight at the image's scale, bit for bit (the check of test_gpu_ema.py, restated for the caches a training
    step fills), on every holder of _holders; and every current input-gradient layer's weight == its owner's weight
    transposed over (Cout, Cin) and rotated by 180 degrees.  Returns (images checked, of them on derived layers, of them
    on input-gradient layers)."""
    from dkt_stereo_amd import _ffi
    L = _ffi.lib()
    modules = {id(m) for m in model.modules()}
    n = derived = grad = 0
    for h, owner in _holders(model):
        w = getattr(h, "weight", None)
        if w is None or not torch.is_tensor(w):
            continue
        if owner is not None:
            assert torch.equal(w, owner.weight.detach().float().transpose(0, 1).flip(2, 3))
        wc = w.detach().float().contiguous()
        for p in (p for lst in h.__dict__.get("_dkt_packed", {}).values() for p in lst):
            if not _current(p.key, w):
                continue
            chs = p.src_channels
            ch = (ctypes.c_int * len(chs))(*chs)
            hi, lo = torch.empty_like(p.hi), torch.empty_like(p.lo)
            assert L.dkt_conv2d_pack_weights(wc.data_ptr(), ch, len(chs), int(w.shape[0]), int(w.shape[2]), int(w.shape[3]),
                                             1.0 / p.inv_scale, hi.data_ptr(), lo.data_ptr(), _ffi.device_of(w),
                                             _ffi.stream_of(w)) == 0
            assert torch.equal(hi, p.hi) and torch.equal(lo, p.lo)
            if p.bias is not None:
                assert torch.equal(p.bias, h.bias.detach().float())
            n += 1
            grad += owner is not None
            derived += owner is None and id(h) not in modules
        for pk in (p for lst in h.__dict__.get("_dkt_stem7", {}).values() for p in lst):
            if not _current(pk.key, w):
                continue
            hi, lo = torch.empty_like(pk.hi), torch.empty_like(pk.lo)
            assert L.dkt_conv2d_stem7_pack(wc.data_ptr(), int(w.shape[0]), int(w.shape[1]), 1.0 / pk.inv_scale, hi.data_ptr(),
                                           lo.data_ptr(), _ffi.device_of(w), _ffi.stream_of(w)) == 0
            assert torch.equal(hi, pk.hi) and torch.equal(lo, pk.lo)
            n += 1
    return n, derived, grad


def _fresh_like(model):
    fresh = E.make_raft({}, 100).to(DEV)
    fresh.load_state_dict(model.state_dict())
    fresh.train()
    fresh.freeze_bn()
    return fresh


def _loop(mp, ours):
    """Two warm-up steps, a third under the sync counter, then the following forward and backward under it."""
    from dkt_stereo_amd import optim
    model, i1, i2, ws = _student()
    hy = dict(lr=2e-4, weight_decay=1e-5, eps=1e-8)
    opt = optim.AdamW(model.parameters(), max_norm=1.0, module=model, **hy) if ours else torch.optim.AdamW(model.parameters(), **hy)

    def step():
        if not ours:
            torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
    for _ in range(2):
        _fwd_bwd(model, i1, i2, ws)
        step()
    _fwd_bwd(model, i1, i2, ws)
    with _Syncs() as s_step:
        step()
    cold = _ColdPacks(mp)
    with _Syncs() as s_fwd:
        preds = _fwd_bwd(model, i1, i2, ws)
    return dict(model=model, opt=opt, step_syncs=s_step, fwd_syncs=s_fwd, cold=cold.n, preds=preds, inputs=(i1, i2, ws))


def test_student_stays_warm(monkeypatch):
    with monkeypatch.context() as mp:
        _nodes_on(mp)
        a = _loop(mp, ours=True)
    with monkeypatch.context() as mp:
        _nodes_on(mp)
        b = _loop(mp, ours=False)
        layers = len(_packed_layers(b["model"]))
        print("optim.AdamW(module=model): step %d synchronising call(s); next forward + backward %d cold pack(s), %d synchronising "
              "call(s) in all.  torch.optim.AdamW: next forward + backward %d cold pack(s) over %d packed layers, %d synchronising "
              "call(s) in all" % (a["step_syncs"].n, a["cold"], a["fwd_syncs"].n, b["cold"], layers, b["fwd_syncs"].n))
        info = a["opt"].last_refresh
        assert a["step_syncs"].n <= 1, a["step_syncs"].msgs
        assert info["warm"] and info["repacked"] > 0 and info["unknown"] == [], info
        assert a["cold"] == 0
        assert b["cold"] >= layers > 0                                 # the control: one host read per packed layer
        assert b["fwd_syncs"].n - a["fwd_syncs"].n >= b["cold"]
        n, derived, grad = _check_packs_cold_equal(a["model"])
        print("%d current images equal cold packs bit for bit: %d on derived layers, %d on input-gradient layers; %d repacked; "
              "synchronising calls of the warm forward + backward at %s" % (n, derived, grad, info["repacked"], a["fwd_syncs"].where))
        assert n == info["repacked"] and derived > 0 and grad > 0      # every image the refresh rewrote was compared
        # the forward AND the backward after the step against a fresh model of the same state dict: the predictions under
        # WARM_BOUND, the gradients -- which the refreshed input-gradient layers carry -- under R.G_BOUND (max|d| / max|want|
        # per parameter, the rule and the bound test_gpu_raft_train.py holds the nodes to)
        model = a["model"]
        fresh = _fresh_like(model)
        i1, i2, ws = a["inputs"]
        want = _fwd_bwd(fresh, i1, i2, ws)
        d = max(float((x.detach() - y.detach()).abs().max()) for x, y in zip(a["preds"], want))
        errs = R.grad_error({k: q.grad for k, q in model.named_parameters()}, {k: q.grad for k, q in fresh.named_parameters()})
        k, e = R.worst(errs)
        print("warm student against a fresh model of the same state dict: predictions max|d| %.3g; %d gradients, worst %.3g at %s"
              % (d, len(errs), e, k))
        assert d <= WARM_BOUND
        assert e <= R.G_BOUND


def test_overflow_with_module_changes_nothing(monkeypatch):
    """module= together with an inf gradient: the step is skipped on the device, the one host read carries the skipped bit,
    no parameter, moment or count changes, the refresh rewrites the same images (still equal to cold packs) and the next
    forward and backward pack nothing."""
    from dkt_stereo_amd import optim
    with monkeypatch.context() as mp:
        _nodes_on(mp)
        model, i1, i2, ws = _student()
        opt = optim.AdamW(model.parameters(), lr=2e-4, weight_decay=1e-5, max_norm=1.0, module=model)
        _fwd_bwd(model, i1, i2, ws)
        opt.step()
        _fwd_bwd(model, i1, i2, ws)
        victim = next(p for p in model.parameters() if p.grad is not None)
        victim.grad.view(-1)[0] = float("inf")
        before = {k: q.detach().clone() for k, q in model.named_parameters()}
        moments = [(st["exp_avg"].clone(), st["exp_avg_sq"].clone()) for st in opt.state.values()]
        with _Syncs() as s:
            _, _, skipped = opt.step()
        info = opt.last_refresh
        print("overflow with module=: %d synchronising call(s), %s" % (s.n, info))
        assert s.n <= 1, s.msgs
        assert info["skipped"] is True and info["warm"] and info["repacked"] > 0 and info["unknown"] == []
        assert float(skipped) == 1.0 and int(opt._step_t.item()) == 1
        for k, q in model.named_parameters():
            assert torch.equal(q.detach(), before[k]), k
        for st, (m0, v0) in zip(opt.state.values(), moments):
            assert torch.equal(st["exp_avg"], m0) and torch.equal(st["exp_avg_sq"], v0)
        n, derived, grad = _check_packs_cold_equal(model)
        assert n == info["repacked"] and grad > 0
        cold = _ColdPacks(mp)
        _fwd_bwd(model, i1, i2, ws)
        assert cold.n == 0


def test_window_exit_goes_cold(monkeypatch):
    """One layer's weights shrink to a tenth in one step (decoupled decay with lr * weight_decay = 0.9, the Adam term 1e-4 of
    max|w|): its image leaves [2^11, 2^14) at its scale, is dropped, and the next forward packs it cold."""
    from dkt_stereo_amd import optim
    with monkeypatch.context() as mp:
        _nodes_on(mp)
        model, i1, i2, ws = _student()
        _fwd_bwd(model, i1, i2, ws)
        name, layer = [(n, m) for n, m in _packed_layers(model) if m.__dict__.get("_dkt_packed")][-1]
        wmax = float(layer.weight.detach().abs().max())
        for p in model.parameters():
            if p is not layer.weight:
                p.grad = None
        lr = 1e-4 * wmax
        opt = optim.AdamW(model.parameters(), lr=lr, weight_decay=0.9 / lr, max_norm=None, module=model)
        opt.step()
        info = opt.last_refresh
        print("window exit at %s: max|w| %.3g -> %.3g, %s" % (name, wmax, float(layer.weight.detach().abs().max()), info))
        assert not info["warm"] and info["kernel"] == 1
        assert not any(_current(p.key, layer.weight) for lst in layer.__dict__.get("_dkt_packed", {}).values() for p in lst)
        cold = _ColdPacks(mp)
        fresh = _fresh_like(model)
        got = model(i1, i2, iters=R.ITERS, test_mode=False)["disp_preds"]
        n_cold = cold.n
        want = fresh(i1, i2, iters=R.ITERS, test_mode=False)["disp_preds"]
        assert n_cold >= 1
        assert any(_current(p.key, layer.weight) for lst in layer.__dict__["_dkt_packed"].values() for p in lst)
        d = max(float((x.detach() - y.detach()).abs().max()) for x, y in zip(got, want))
        print("after the window exit: %d cold pack(s), max|d| against a fresh model %.3g" % (n_cold, d))
        assert d <= WARM_BOUND
