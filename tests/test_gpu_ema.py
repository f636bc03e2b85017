"""ema.ema_update_ on the device: dkt_ema_update against torch's evaluation of tools/ft_dkt.py:179-181, and the refresh of
a warm RAFTStereo teacher (packed images rewritten in place, captured loop kept) against fresh models holding the same
weights.  The bound is the contract bound of test_calibration_stress_twenty_pairs (1e-3 max-abs at 256x512, 12 iterations):
random-init GRU dynamics are not contractive."""
import ctypes
import gc
import warnings

import numpy as np
import pytest
import torch

import _synth
from test_gpu_parity import DEV, G, _raft, maxabs

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _collect():
    gc.collect()             # the models of the previous test (captured states are cyclic) go before this one captures
    yield
H, W, ITERS = 256, 512, 12
BOUND = 1e-3


def _student(teacher, seed, rel=0.01):
    """A copy of the teacher's weights with a relative perturbation (the student of one DKT step)."""
    student, _ = _raft(mixed_precision=teacher.args.mixed_precision)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for s, t in zip(student.parameters(), teacher.parameters()):
            noise = torch.randn(t.shape, generator=gen).to(t.device)
            s.copy_(t + rel * noise * t.abs().mean().clamp_min(1e-3))
    return student


def _fresh_like(model):
    fresh, _ = _raft(mixed_precision=model.args.mixed_precision)
    fresh.load_state_dict(model.state_dict())
    return fresh


def _graphs(model):
    """Identity of the model's loop state and of every graph its loop has captured."""
    st = model._graph_state
    lp = st.get("c8")
    ids = [id(st), id(lp)]
    for d in (lp.graph, lp.graph_n, lp.graph_last):
        ids += [id(g) for g in (d.values() if isinstance(d, dict) else [d])]
    return tuple(ids)


class _Captures:
    """Counts graph captures (CUDAGraph.capture_end) while installed."""

    def __init__(self, monkeypatch):
        self.n = 0
        end = torch.cuda.CUDAGraph.capture_end

        def counted(g, *a, **k):
            self.n += 1
            return end(g, *a, **k)
        monkeypatch.setattr(torch.cuda.CUDAGraph, "capture_end", counted)


def _holders(model):
    """Modules and the derived layers cached below them (folded, merged, views), breadth first."""
    todo, out, seen = list(model.modules()), [], set()
    while todo:
        h = todo.pop(0)
        if id(h) in seen:
            continue
        seen.add(id(h))
        out.append(h)
        d = h.__dict__
        for name in ("_dkt_folded", "_dkt_merged", "_zr_cache", "_dkt_view", "_dkt_scaled"):
            todo += [e for lst in (d.get(name) or {}).values() for e in lst]
    return out


def _current(key, w):
    return key.tensors[0] == (w.data_ptr(), w._version)


def _check_packs_cold_equal(model):
    """Every current packed image == a cold pack of the current weights at the same scale (same pack kernels); every current
    copied weight (head, k-major) == the current weights."""
    from dkt_stereo_amd import _ffi
    from dkt_stereo_amd import conv_c8 as c8
    L = _ffi.lib()
    n = 0
    for h in _holders(model):
        w = getattr(h, "weight", None)
        for lst in h.__dict__.get("_dkt_packed_c8", {}).values():
            for p in lst:
                if not _current(p.key, w):
                    continue
                wc = w.detach().float()
                if p.scales is not None:
                    wc = wc * c8._in_scale_vector(p.scales, w.device).view(1, -1, 1, 1)
                img = torch.zeros_like(p.img)
                c8._repack_raw(wc, p.src_channels, p.inv_scale, img)
                assert torch.equal(img, p.img)
                n += 1
        for lst in h.__dict__.get("_dkt_gru_c8", {}).values():
            for p in lst:
                if not _current(p.key, h.convz.weight):
                    continue
                wzr, wq2, ch = c8._gru_images(h, p.x_channels, p.hs, p.xs)
                a, b = torch.zeros_like(p.wzr), torch.zeros_like(p.wq)
                c8._repack_raw(wzr, [ch] + list(p.x_channels), p.inv_zr, a)
                c8._repack_raw(wq2, list(p.x_channels) + [ch], p.inv_q, b)
                assert torch.equal(a, p.wzr) and torch.equal(b, p.wq)
                assert torch.equal(p.bz, h.convz.bias) and torch.equal(p.bq, h.convq.bias)
                n += 1
        for p in (p for lst in h.__dict__.get("_dkt_packed", {}).values() for p in lst):
            if not _current(p.key, w):
                continue
            chs = p.src_channels
            ch = (ctypes.c_int * len(chs))(*chs)
            hi, lo = torch.empty_like(p.hi), torch.empty_like(p.lo)
            wc = w.detach().float().contiguous()
            assert L.dkt_conv2d_pack_weights(wc.data_ptr(), ch, len(chs), int(w.shape[0]), int(w.shape[2]), int(w.shape[3]),
                                             1.0 / p.inv_scale, hi.data_ptr(), lo.data_ptr(), _ffi.device_of(w),
                                             _ffi.stream_of(w)) == 0
            assert torch.equal(hi, p.hi) and torch.equal(lo, p.lo)
            if p.bias is not None:
                assert torch.equal(p.bias, h.bias.detach().float())
            n += 1
        for e in (e for lst in h.__dict__.get("_dkt_head_w", {}).values() for e in lst):
            if _current(e.key, w):
                assert torch.equal(e.value[:, :, :9], w.detach().float().reshape(w.shape[0], w.shape[1], 9))
                n += 1
        for e in (e for lst in h.__dict__.get("_dkt_wt", {}).values() for e in lst):
            if _current(e.key, w):
                assert torch.equal(e.value, w.detach().reshape(w.shape[0], -1).t())
                n += 1
        for pk in (p for lst in h.__dict__.get("_dkt_stem7", {}).values() for p in lst):
            if not _current(pk.key, w):
                continue
            hi, lo = torch.empty_like(pk.hi), torch.empty_like(pk.lo)
            wc = w.detach().float().contiguous()
            assert L.dkt_conv2d_stem7_pack(wc.data_ptr(), int(w.shape[0]), int(w.shape[1]), 1.0 / pk.inv_scale, hi.data_ptr(),
                                           lo.data_ptr(), _ffi.device_of(w), _ffi.stream_of(w)) == 0
            assert torch.equal(hi, pk.hi) and torch.equal(lo, pk.lo)
            n += 1
    return n


def _pair(seed=12):
    return [G(t) for t in _synth.image_pair(seed, 1, H, W, 12)]


def _warm(mp, n=6, **attrs):
    """A teacher past its first captures: the loop alternates between unit kinds, so a few forwards capture them all."""
    teacher, _ = _raft(mixed_precision=mp)
    for k, v in attrs.items():
        setattr(teacher, k, v)
    pair = _pair()
    for _ in range(n):
        teacher(*pair, iters=ITERS, test_mode=True)
    return teacher, pair


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_ema_kernel_bit_identical_to_torch():
    from dkt_stereo_amd.ema import ema_kernel
    torch.manual_seed(0)
    sizes = [1, 0, 7, 1023, 2048, 4097, 3 * 2048 + 5, 100003, 0, 33]
    for decay in (0.9999, 0.99999, 0.5):
        ts = [torch.randn(n, device=DEV) * (k + 1) for k, n in enumerate(sizes)]
        ss = [torch.randn(n, device=DEV) for n in sizes]
        want = [(decay * t + (1 - decay) * s) for t, s in zip(ts, ss)]
        absmax = torch.full((len(sizes),), -1.0, device=DEV)
        ema_kernel(ts, ss, decay, absmax)
        for t, w in zip(ts, want):
            assert np.array_equal(t.cpu().numpy(), w.cpu().numpy())
        amax = [float(w.abs().amax()) if w.numel() else 0.0 for w in want]
        assert np.array_equal(absmax.cpu().numpy(), np.asarray(amax, np.float32))
        ema_kernel([ts[3]], [ss[3]], decay)                                  # absmax is optional
        assert torch.equal(ts[3], decay * want[3] + (1 - decay) * ss[3])


# ---- the refresh of a warm teacher --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mp", [False, True])
@torch.no_grad()
def test_warm_refresh_keeps_loop_and_matches_fresh(mp, monkeypatch):
    from dkt_stereo_amd.ema import ema_update_
    teacher, pair = _warm(mp)
    lp = teacher._graph_state["c8"]
    cap = _Captures(monkeypatch)
    teacher(*pair, iters=ITERS, test_mode=True)
    assert cap.n == 0                                      # (warm: a forward without an update captures nothing)
    calib, graphs = lp.calibrations, _graphs(teacher)
    student = _student(teacher, 1)
    info = ema_update_(teacher, student, 0.99)
    assert info["warm"] and info["fallback"] == 0 and info["repacked"] > 0, info
    _, got = teacher(*pair, iters=ITERS, test_mode=True)
    assert lp.calibrations == calib and _graphs(teacher) == graphs and cap.n == 0
    n = _check_packs_cold_equal(teacher)
    assert n > 0
    _, want = _fresh_like(teacher)(*pair, iters=ITERS, test_mode=True)
    d = maxabs(got, want)
    print("warm refresh mixed_precision=%s: %d packs checked, %d repacked, flow_up max|d| vs fresh %.3g" % (mp, n, info["repacked"], d))
    assert d <= BOUND


@torch.no_grad()
def test_twenty_updates_large_drift():
    from dkt_stereo_amd.ema import ema_update_
    teacher, pair = _warm(False)
    lp = teacher._graph_state["c8"]
    student = _student(teacher, 2, rel=0.05)
    rec0, cold, dist = lp.recalibrations, 0, []
    for step in range(20):
        info = ema_update_(teacher, student, 0.9)
        cold += not info["warm"]
        _, got = teacher(*pair, iters=ITERS, test_mode=True)
        if teacher._graph_state["c8"] is lp:
            _check_packs_cold_equal(teacher)
        else:                                  # (a pack left its window: the loop was rebuilt cold)
            lp = teacher._graph_state["c8"]
        _, want = _fresh_like(teacher)(*pair, iters=ITERS, test_mode=True)
        dist.append(maxabs(got, want))
    print("twenty updates at decay 0.9: %d cold steps, %d rescales of the last loop, worst max|d| %.3g" %
          (cold, lp.recalibrations - rec0 if cold == 0 else lp.recalibrations, max(dist)))
    assert max(dist) <= BOUND


@torch.no_grad()
def test_window_exit_goes_cold():
    from dkt_stereo_amd.ema import ema_update_
    teacher, pair = _warm(False)
    st = teacher._graph_state
    student = _fresh_like(teacher)
    with torch.no_grad():
        for p in student.update_block.parameters():
            p.mul_(16.0)
    info = ema_update_(teacher, student, 0.0)
    assert not info["warm"]
    for h in _holders(teacher.update_block):                 # every pack of the scaled layers was dropped, none is current
        for name in ("_dkt_packed_c8", "_dkt_packed", "_dkt_stem7"):
            for lst in h.__dict__.get(name, {}).values():
                assert not any(_current(p.key, h.weight) for p in lst), name
        for lst in h.__dict__.get("_dkt_gru_c8", {}).values():
            assert not any(_current(p.key, h.convz.weight) for p in lst)
    _, got = teacher(*pair, iters=ITERS, test_mode=True)
    assert teacher._graph_state is not st
    _, want = _fresh_like(teacher)(*pair, iters=ITERS, test_mode=True)
    assert torch.equal(got, want)


@torch.no_grad()
def test_graphed_encoders_never_replay_old_weights():
    from dkt_stereo_amd.ema import ema_update_
    teacher, pair = _warm(False, graph_encoders=True)
    info = ema_update_(teacher, _student(teacher, 3), 0.99)
    assert info["warm"]
    _, got = teacher(*pair, iters=ITERS, test_mode=True)
    _, want = _fresh_like(teacher)(*pair, iters=ITERS, test_mode=True)
    d = maxabs(got, want)
    print("graphed encoders after ema_update_: max|d| vs fresh %.3g" % d)
    assert d <= BOUND


@pytest.mark.parametrize("table,left_out", [("PACK_HOOKS", "_dkt_packed_c8"), ("DERIVED_HOOKS", "_dkt_folded")])
@torch.no_grad()
def test_cache_left_out_goes_cold(table, left_out, monkeypatch):
    from dkt_stereo_amd import ema
    teacher, pair = _warm(False, graph_encoders=True)
    st = teacher._graph_state
    monkeypatch.delitem(getattr(ema, table), left_out)
    info = ema.ema_update_(teacher, _student(teacher, 4), 0.99)
    assert not info["warm"] and left_out in info["unknown"]
    _, got = teacher(*pair, iters=ITERS, test_mode=True)
    assert teacher._graph_state is not st                    # the loop was rebuilt, not replayed on old weights
    _, want = _fresh_like(teacher)(*pair, iters=ITERS, test_mode=True)
    d = maxabs(got, want)
    print("%s left out of the refresh: max|d| vs fresh %.3g" % (left_out, d))
    assert d <= BOUND


@torch.no_grad()
def test_one_sync_per_update():
    from dkt_stereo_amd.ema import ema_update_
    teacher, pair = _warm(True)
    student = _student(teacher, 5)
    ema_update_(teacher, student, 0.9999)             # first call: builds the kernel's pointer tables
    teacher(*pair, iters=ITERS, test_mode=True)
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            info = ema_update_(teacher, student, 0.9999)
        finally:
            torch.cuda.set_sync_debug_mode(0)
    syncs = [r for r in rec if "called a synchronizing" in str(r.message)]
    print("ema_update_ on a warm mixed-precision teacher: %d synchronising call(s), %d images repacked" % (len(syncs), info["repacked"]))
    assert info["warm"]
    assert len(syncs) <= 1, [str(r.message) for r in syncs]
