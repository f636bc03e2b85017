"""The optimizer step of tools/ft_dkt.py:243-246 on the device: unscale, clip_grad_norm_, AdamW (:58), skip on overflow.

The reference runs, between backward() and the next forward::

    scaler.unscale_(optimizer)
    torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
    scaler.step(optimizer)          # AdamW(lr, weight_decay=1e-5, eps=1e-8)

``AdamW(model.parameters(), ..., max_norm=1.0, module=model)`` does the three in ``dkt_adamw_step``: a pass over the
gradients (sum of squares per fixed tile in fp64, an integer flag for inf / nan), a one-block finalise (total norm, clip
coefficient, the skip decision, the device-resident step counter) and the update, which skips itself on overflow.  Nothing is
read on the host: ``step()`` returns the device record ``(total_norm, clip, skipped)``.  ``.grad`` is NOT rewritten (a stated
difference from ``unscale_`` / ``clip_grad_norm_``): the unscaled, clipped gradient exists in registers only.

GradScaler: the class sets ``_step_supports_amp_scaling``; ``GradScaler.step`` then hands it the attributes ``grad_scale``
(the scale, a device tensor; None when the caller ran ``unscale_`` itself) and ``found_inf`` (a device tensor) and calls
``step()`` without reading ``found_inf`` on the host.

``module=``: every weight derivative of this library is keyed on ``(data_ptr, _version)``, so an optimizer step makes every
convolution of the student cold, at one host read of max|w| per layer in the next forward.  With ``module=model`` the step
bumps the version counters once and then rewrites every current derivative in place at its existing scale, with max|w| taken
from the update kernel -- the refresh ``ema.ema_update_`` gives the teacher, one host read for all window flags.  On a
skipped step the parameters are unchanged; the refresh still runs (the skip is known on the device only) and rewrites the
same images.  Without ``module=`` the version counters are bumped all the same and the model goes cold, as after any
optimizer's step.

Param groups with equal hyper-parameters are folded into one call; groups that differ are refused (the clip coefficient and
the step counter belong to the whole parameter list).  State is torch's layout: ``state[p] = {"step", "exp_avg",
"exp_avg_sq"}``; every ``step`` entry is the one device counter, and ``state_dict()`` writes it out per parameter as torch
does, so state dicts load into ``torch.optim.AdamW`` and back.  One counter is a difference from torch where parameters do
not step together: a parameter that receives its first gradient later (or arrives through ``add_param_group``) starts with
zero moments but takes the bias corrections of the shared count, where torch would start its own count at 1; and
``load_state_dict`` refuses a state whose parameters are at different steps.
"""
import math

import torch

from . import _ffi
from ._flat_tables import flat_tables

_HYPER = ("lr", "betas", "eps", "weight_decay")


def workspace_bytes(count, total):
    return _ffi.size("dkt_adamw_workspace", int(count), int(total))


def adamw_kernel(ps, gs, ms, vs, step, record, workspace, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None,
                 inv_scale=1.0, grad_scale=None, found_inf=None, absmax=None, grid=0):
    """One dkt_adamw_step over lists of same-device, dense fp32 CUDA tensors (include/dktstereo.h).  `step`: 0-d fp32 device
    counter; `record`: 4 fp32; `workspace`: zero-initialised uint8 tensor of workspace_bytes(count, total) bytes, reused."""
    if not ps:
        return
    dev = ps[0].device
    _, ptr, total = flat_tables(dev, ps, gs, ms, vs)
    if workspace.numel() < workspace_bytes(len(ps), total):
        raise _ffi.DktError("dkt_adamw_step workspace too small")
    opt = lambda t: None if t is None else t.data_ptr()
    _ffi.call("dkt_adamw_step", ps[0], ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], len(ps), total, float(lr), float(betas[0]),
              float(betas[1]), float(eps), float(weight_decay), -1.0 if max_norm is None else float(max_norm),
              float(inv_scale), opt(grad_scale), opt(found_inf), step.data_ptr(), record.data_ptr(),
              opt(absmax), workspace.data_ptr(), int(grid))


def _require(p):
    if not p.is_cuda:
        raise _ffi.DktError("optim.AdamW updates parameters on a HIP device only (got a %s tensor); there is no CPU path" % p.device)
    if p.dtype != torch.float32:
        raise _ffi.DktError("optim.AdamW parameters are float32 (got %s)" % p.dtype)
    if p.is_sparse or not p.is_contiguous():
        raise _ffi.DktError("optim.AdamW parameters are dense and contiguous")


class AdamW(torch.optim.Optimizer):
    """torch.optim.AdamW(params, lr, betas, eps, weight_decay) with the gradient clipping of clip_grad_norm_(params,
    max_norm) and the GradScaler's unscale and overflow skip inside the step (module docstring)."""

    _step_supports_amp_scaling = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None, module=None):
        if torch.is_tensor(lr):
            raise ValueError("lr is a Python number (it is passed to the kernel by value on every call)")
        if not 0.0 <= lr or not math.isfinite(lr):
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not 0.0 <= eps or not math.isfinite(eps):
            raise ValueError("Invalid epsilon value: %r" % (eps,))
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameters: %r" % (betas,))
        if not 0.0 <= weight_decay or not math.isfinite(weight_decay):
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        if max_norm is not None and (math.isnan(max_norm) or max_norm < 0):       # (inf: the norm is taken, nothing is clipped)
            raise ValueError("Invalid max_norm: %r" % (max_norm,))
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.max_norm = max_norm
        self.module = module
        self.last_refresh = None
        dev = self.param_groups[0]["params"][0].device
        self._step_t = torch.zeros((), device=dev, dtype=torch.float32)
        self._record = torch.zeros(4, device=dev, dtype=torch.float32)
        self._workspace = self._absmax = None            # sized by step() for the parameters it finds
        self.last_lr = None

    def add_param_group(self, param_group):
        """torch's, then the checks of the constructor for the new parameters (the constructor itself comes through here)."""
        super().add_param_group(param_group)
        ps = [p for g in self.param_groups for p in g["params"]]
        for p in self.param_groups[-1]["params"]:
            _require(p)
        if len({p.device for p in ps}) > 1:
            raise _ffi.DktError("optim.AdamW takes the parameters of one device (got %s)" % sorted({str(p.device) for p in ps}))

    # -- state -------------------------------------------------------------------------------------------------------------------
    def _hyper(self):
        g0 = self.param_groups[0]
        for g in self.param_groups[1:]:
            if any(g[k] != g0[k] for k in _HYPER):
                raise _ffi.DktError("optim.AdamW folds param groups into one call: their lr, betas, eps and weight_decay must "
                                    "agree (the clip coefficient and the step counter belong to the whole list)")
        if g0.get("amsgrad") or g0.get("maximize"):
            raise _ffi.DktError("optim.AdamW has no amsgrad / maximize variant")
        return g0

    def state_dict(self):
        """torch's layout, every parameter with a `step` tensor of its own on the host (one host read of the counter)."""
        sd = super().state_dict()
        step = self._step_t.detach().cpu()
        sd["state"] = {k: dict(v, step=step.clone()) if "step" in v else dict(v) for k, v in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        steps = {float(st["step"]) for st in self.state.values() if "step" in st}
        if len(steps) > 1:
            raise _ffi.DktError("optim.AdamW keeps one step counter: the loaded parameters are at steps %s" % sorted(steps))
        self._step_t.fill_(steps.pop() if steps else 0.0)
        for p, st in self.state.items():
            if "step" in st:
                st["step"] = self._step_t
                for k in ("exp_avg", "exp_avg_sq"):
                    st[k] = st[k].to(device=p.device, dtype=torch.float32).contiguous().clone()

    # -- the step ----------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        """One step; returns the device record as three 0-d tensors (total_norm, clip, skipped), unread.  total_norm is -1
        when neither clipping nor a loss scale asked for the pass over the gradients."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        g0 = self._hyper()
        ps, gs, ms, vs = [], [], [], []
        for group in self.param_groups:
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse or g.layout != torch.strided or not g.is_contiguous() or g.dtype != torch.float32 \
                        or g.device != p.device or g.shape != p.shape:
                    raise _ffi.DktError("optim.AdamW takes dense, contiguous fp32 gradients laid out as their parameters")
                st = self.state[p]
                if not st:
                    st["step"] = self._step_t
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                ps.append(p)
                gs.append(g)
                ms.append(st["exp_avg"])
                vs.append(st["exp_avg_sq"])
        self.last_refresh = None
        if not ps:
            return loss if closure is not None else tuple(self._record[:3].unbind())
        need = workspace_bytes(len(ps), sum(p.numel() for p in ps))
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.zeros(need, device=ps[0].device, dtype=torch.uint8)
        if self._absmax is None or self._absmax.numel() < len(ps):
            self._absmax = torch.zeros(len(ps), device=ps[0].device, dtype=torch.float32)
        grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        for name, t in (("grad_scale", grad_scale), ("found_inf", found_inf)):
            if t is not None and (not t.is_cuda or t.device != ps[0].device or t.dtype != torch.float32 or t.numel() != 1):
                raise _ffi.DktError("optim.AdamW: %s is one fp32 value on the parameters' device" % name)
        absmax = self._absmax if self.module is not None else None
        self.last_lr = float(g0["lr"])
        adamw_kernel(ps, gs, ms, vs, self._step_t, self._record, self._workspace, self.last_lr, g0["betas"], g0["eps"],
                     g0["weight_decay"], self.max_norm, 1.0, grad_scale, found_inf, absmax)
        if self.module is not None:
            self.last_refresh = self._refresh(ps, absmax)
        else:
            torch.autograd.graph.increment_version(ps)       # (written behind autograd's back: everything keyed on them is stale)
        return loss if closure is not None else tuple(self._record[:3].unbind())

    def _refresh(self, ps, absmax):
        from . import ema
        R = ema._Refresh()
        R.absmax = absmax
        R.index = {p.data_ptr(): (i, p.numel()) for i, p in enumerate(ps)}
        ok = ema.refresh_written(ema._unwrap(self.module), ps, R, extra=[self._record[2] != 0])
        return dict(kernel=len(ps), repacked=R.repacked, warm=ok, unknown=[name for _, name in R.unknown],
                    skipped=bool(R.extra[0]) if R.extra else None)
