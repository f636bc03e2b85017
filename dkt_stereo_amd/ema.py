"""The EMA teacher's update of tools/ft_dkt.py:179-181, keeping the teacher's derived weights and captured loop warm.

The reference rewrites every parameter of ``model_T_EMA`` before each step::

    for t_params, s_params in zip(model_T_EMA.parameters(), model.parameters()):
        t_params.data = (ema_decay * t_params.data + (1 - ema_decay) * s_params.data)
        t_params.requires_grad = False

Every weight derivative of this library (packed images, folded / merged layers, the captured loop's key) is keyed on
``(data_ptr, _version)``, so each EMA-teacher forward after that loop is a cold start.  ``ema_update_(teacher, student,
decay)`` computes the same values in place (``dkt_ema_update``, one launch for all parameters), bumps every parameter's
version counter, and then rewrites every cache entry that was current before the update into its existing buffers with
its existing scales and re-keys it.  Whatever is not rewritten -- a cache this module does not know, an entry whose
weights left their scale window -- keeps its old key and is rebuilt cold on next use: never stale.

Window: a cold pack scales max|w| into [2^12, 2^13).  A refreshed pack keeps its scale while the new max|w|
times that scale lies in [2^11, 2^14): the hi part stays finite (2^14 is far below fp16's 65504) and the residual keeps
at least all but one of the bits a cold pack gives it.  The check runs on the device; the flags of all packs are read with
one host synchronisation per call.
"""

import torch
import torch.nn as nn

from . import _ffi
from ._flat_tables import flat_tables
# (importing the modules that fill the caches registers their refreshers)
from . import conv, conv_c8, corr, extractor, update      # noqa: F401
from .wcache import DERIVED_HOOKS, NOT_WEIGHTS, PACK_HOOKS

#: scaled max|w| window of a refreshed pack: [2^WINDOW_LO, 2^WINDOW_HI)
WINDOW_LO, WINDOW_HI = 11, 14


class _Refresh:
    """State of one ema_update_ call: old -> new version of every tensor written, the window flags of the repacked images."""

    def __init__(self):
        self.vmap = {}            # data_ptr -> (version before, version after)
        self.gone = set()         # data_ptrs of parameters the fallback replaced
        self.amaxes, self.invs, self.drops = [], [], []   # per repacked image: max|w| (device), its 1 / scale, its drop()
        self.unknown = []         # caches no hook refreshed
        self.absmax = None
        self.index = {}           # data_ptr -> (position in absmax, numel) of the kernel's parameters
        self.repacked = 0

    def current(self, key):
        """True when `key` names at least one written tensor and every one at the version it had before this update."""
        seen = False
        for t in key.tensors:
            if t is None:
                continue
            if t[0] in self.gone:
                return False
            ver = self.vmap.get(t[0])
            if ver is not None:
                if ver[0] != t[1]:
                    return False
                seen = True
        return seen

    def rekey(self, key):
        """`key` with every written tensor it names at its pre-update version moved to the new one."""
        def moved(t):
            ver = None if t is None else self.vmap.get(t[0])
            return (t[0], ver[1]) if ver is not None and ver[0] == t[1] else t
        return key._replace(tensors=tuple(moved(t) for t in key.tensors))

    def each(self, cache):
        """(entry, drop) of every current entry of one holder's cache; drop() takes the entry out of the cache."""
        def dropper(slot, e):
            def drop():
                cache[slot] = [q for q in cache.get(slot, ()) if q is not e]
            return drop
        for slot, lst in list(cache.items()):
            for e in list(lst):
                if self.current(e.key):
                    yield e, dropper(slot, e)

    def write(self, t, fn):
        old = t._version
        fn()
        self.vmap[t.data_ptr()] = (old, t._version)

    def amax(self, w):
        """max|w| on the device: the kernel's own output when `w` is one of the updated parameters, else a reduction."""
        hit = self.index.get(w.data_ptr())
        if hit is not None and hit[1] == w.numel() and w.dtype == torch.float32:
            return self.absmax[hit[0]]
        return w.detach().float().abs().amax()

    def window(self, amax, inv_scale, drop):
        if torch.is_tensor(inv_scale):         # (a pack's scale is a host number; float() of a device tensor would be a host read)
            raise TypeError("_Refresh.window: inv_scale is a Python number")
        self.amaxes.append(amax)
        self.invs.append(float(inv_scale))
        self.drops.append(drop)
        self.repacked += 1

    def flags(self):
        """Whether each repacked image's max|w| * scale lies in the window: one bool tensor per device, in a handful of
        launches for all images (the scales travel through pinned memory, without blocking), with the positions it covers."""
        by_dev = {}
        for i, a in enumerate(self.amaxes):
            by_dev.setdefault(a.device, []).append(i)
        out = []
        for dev, idx in by_dev.items():
            inv = torch.tensor([self.invs[i] for i in idx], dtype=torch.float32)
            inv = inv.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else inv
            s = torch.stack([self.amaxes[i].reshape(()).float() for i in idx]) / inv
            out.append((idx, (s >= 2.0 ** WINDOW_LO) & (s < 2.0 ** WINDOW_HI)))
        return out


def ema_kernel(ts, ss, decay, absmax=None):
    """t <- decay * t + (1 - decay) * s for lists of same-device, dense fp32 CUDA tensors, one launch (dkt_ema_update).
    `absmax`: optional (len(ts),) fp32 tensor receiving max|t_new| per tensor."""
    if not ts:
        return
    dev = ts[0].device
    _, ptr, _ = flat_tables(dev, ts, ss)
    _ffi.call("dkt_ema_update", ts[0], ptr[0], ptr[1], ptr[2], len(ts), float(decay), float(1 - decay),
              None if absmax is None else absmax.data_ptr())


def _kernel_ok(t, s):
    return (t.is_cuda and s.is_cuda and t.device == s.device and t.dtype == torch.float32 and s.dtype == torch.float32
            and t.shape == s.shape and t.is_contiguous() and s.is_contiguous())


def _unwrap(m):
    return m.module if isinstance(m, (nn.DataParallel, nn.parallel.DistributedDataParallel)) else m


def _refresh(teacher, R, extra=()):
    """Rewrites every current weight derivative below `teacher` in place; returns True when the captured states may be
    re-keyed (nothing unknown, every scale window held -- read with the call's one host synchronisation).  Derived layers
    carry caches of their own (a folded layer's merged heads, a layer view's head weights, every pack): they are visited
    after the layers they derive from, breadth first.  `extra`: 0-d bool device tensors of the caller, read in the same
    host read and left in R.extra."""
    todo, seen, holders = list(teacher.modules()), set(), []
    while todo:
        h = todo.pop(0)
        if id(h) in seen:
            continue
        seen.add(id(h))
        holders.append(h)
        for name, val in list(h.__dict__.items()):
            if not (name.startswith("_dkt_") or name == "_zr_cache") or val is None or (isinstance(val, dict) and not val):
                continue
            hook = DERIVED_HOOKS.get(name)
            if hook is not None:
                todo.extend(hook(h, val, R))
            elif name not in PACK_HOOKS and name not in NOT_WEIGHTS:
                R.unknown.append((h, name))
    for h in holders:
        for name, hook in PACK_HOOKS.items():
            cache = h.__dict__.get(name)
            if cache:
                hook(h, cache, R)
    ok = not R.unknown
    R.extra = []
    if R.amaxes or extra:
        groups = R.flags()
        parts = [f for _, f in groups] + ([torch.stack(list(extra))] if extra else [])
        if len({t.device for t in parts}) > 1:             # (parameters across devices: one read per device)
            parts = [t.cpu() for t in parts]
        flat = torch.cat(parts).cpu()                      # the one host read of the call
        bits = flat.tolist()
        order = [i for idx, _ in groups for i in idx]
        R.extra = bits[len(order):]
        for i, good in zip(order, bits):
            if not good:
                R.drops[i]()
                ok = False
    return ok


def refresh_written(module, tensors, R, extra=()):
    """After a kernel has written the parameters `tensors` of `module` in place (R.absmax / R.index: its max|w| per tensor):
    bumps their version counters once, rewrites every weight derivative that was current before the write into its existing
    buffers at its existing scale and, when nothing was unknown and every scale window held, re-keys the captured states.
    One host read (see _refresh).  Returns whether everything stayed warm.  ema_update_ and optim.AdamW.step() share it."""
    olds = [t._version for t in tensors]
    if tensors:
        torch.autograd.graph.increment_version(tensors)
    for t, old in zip(tensors, olds):
        R.vmap[t.data_ptr()] = (old, t._version)
    ok = _refresh(module, R, extra) if tensors else False
    if ok:
        for m in module.modules():
            rekey = getattr(m, "_ema_rekey", None)
            if rekey is not None:
                rekey(R)
    return ok


def ema_update_(teacher, student, decay):
    """In place: for every (t, s) of zip(teacher.parameters(), student.parameters()), t = decay * t + (1 - decay) * s, with
    the result bit-identical to the reference's expression, then the teacher's weight derivatives and captured loop are
    refreshed so that its next forward stays warm.  `teacher` / `student`: modules or nn.DataParallel wrappers.  Parameters
    the kernel cannot take (CPU, not fp32, mismatched shapes or devices) are updated by the reference's own expression;
    their derivatives go cold.  Returns a dict of counts (parameters by kernel / by fallback, repacked images, whether the
    captured states were kept)."""
    tm, sm = _unwrap(teacher), _unwrap(student)
    decay = float(decay)
    R = _Refresh()
    by_dev, fallback = {}, []
    with torch.no_grad():
        for t, s in zip(tm.parameters(), sm.parameters()):
            if _kernel_ok(t, s):
                by_dev.setdefault(t.device, ([], []))
                by_dev[t.device][0].append(t)
                by_dev[t.device][1].append(s)
            else:
                fallback.append((t, s))
        for t, s in fallback:
            R.gone.add(t.data_ptr())
            t.data = (decay * t.data + (1 - decay) * s.data)
            t.requires_grad = False
        kernel = [t for ts, _ in by_dev.values() for t in ts]
        for dev, (ts, ss) in by_dev.items():
            absmax = torch.empty(len(ts), device=dev, dtype=torch.float32)
            ema_kernel(ts, ss, decay, absmax)
            if len(by_dev) == 1:                           # (amax by reduction when the parameters span devices)
                R.absmax = absmax
                R.index = {t.data_ptr(): (i, t.numel()) for i, t in enumerate(ts)}
        for t in kernel:
            t.requires_grad = False
        ok = refresh_written(tm, kernel, R)
    return dict(kernel=len(kernel), fallback=len(fallback), repacked=R.repacked, warm=ok,
                unknown=[name for _, name in R.unknown])


def reference_update_(teacher, student, decay):
    """tools/ft_dkt.py:179-181 verbatim (the fallback and the yardstick of the tests and tools/bench_ema_teacher.py)."""
    for t_params, s_params in zip(_unwrap(teacher).parameters(), _unwrap(student).parameters()):
        t_params.data = (decay * t_params.data + (1 - decay) * s_params.data)
        t_params.requires_grad = False
