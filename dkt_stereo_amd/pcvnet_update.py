"""PCVNet's mixture-parameter update and its up-samplings on the HIP kernels of libdktstereo.so
(``meta_arch/pcvnet/update.py:76-108``, ``meta_arch/pcvnet/model.py:154-174``):

    updater = ParametersUpdater(args, input_dim=128, hidden_dim=256)        # state-dict keys head.conv1.weight, ...
    mu, w, sigma, disp = updater(net[0], mu, sigma, w, regress=True)         # disp = sum_j w mu (model.py:154)
    disp_up, mu_up, sigma_up, w_up = mixture_upsample(disp, mu, sigma, w, up_mask, 2 ** args.n_downsample)

``parameters_update`` is everything of ``ParametersUpdater.forward`` after the conv head, with the disparity regression, as
one launch (dkt_pcv_update_fwd) and under autograd one node whose backward is one launch (dkt_pcv_update_bwd).  The node
saves its four inputs and one byte per element, the five clip decisions; the backward recomputes the rest.  Under
``no_grad``, or with nothing requiring grad, the same forward launch runs without the byte.  CPU tensors take the torch
restatement (host tests); there is no other fall-back.

``mixture_upsample`` runs the four ``convex_upsample`` calls of model.py:165-174 as two ``upsample.convex_upsample`` nodes:
one for ``disp`` with the mask's gradient, one for ``cat(mu, sigma, w / factor)`` on the detached mask.  The node broadcasts
one mask over its channels, so ``up_mask.repeat(1, G, 1, 1)`` is never built.  ``w`` is up-sampled unscaled in the reference
(``scale=False``); ``factor`` is a power of two, so dividing ``w`` by it and letting the kernel multiply it back is exact and
``w_up`` has the bits of the unscaled call.
"""
import torch
import torch.nn as nn

from . import _ffi
from .conv import conv2d_autograd
from .update import FlowHead
from .upsample import convex_upsample

MAX_GAUSSIANS = 8


def parameters_update_torch(delta, mu, sigma, w, sigma0=0.5, eps=1e-3, gammas=(1, 1, 1), regress=True):
    """update.py:89-107 and model.py:154 restated operation for operation, in the dtype and on the device of the tensors."""
    M = delta.shape[1]
    g1, g2, g3 = gammas
    delta_sigma = 0.5 * (((1 - M * w) * sigma ** 2 - sigma0 ** 2 - delta ** 2) / (M * sigma ** 3) + w * sigma / (sigma0 ** 2))
    delta_mu = -0.5 * delta * (1 / (M * sigma ** 2) + w / (sigma0 ** 2))
    beta = 0.5 * (-1 / (M * w + eps) + torch.log(sigma0 * M * w / sigma + eps) + (sigma ** 2 + delta ** 2) / (2 * sigma0 ** 2) + 0.5)
    delta_w = beta - torch.sum(beta, dim=1, keepdim=True) / M
    delta_sigma = torch.clip(delta_sigma * g1, min=-3, max=3)
    delta_mu = torch.clip(delta_mu * g2, min=-128, max=128)
    delta_w = torch.clip(delta_w * g3, min=-1 / (M * 4), max=1 / (M * 4))
    sigma = torch.clip(sigma - delta_sigma, min=0.1, max=16)
    mu = mu - delta_mu
    w = torch.clip(w - delta_w, min=0, max=1)
    w = w / torch.sum(w, dim=1, keepdim=True)
    return mu, w, sigma, (torch.sum(w * mu, dim=1, keepdim=True) if regress else None)


def _forward(delta, mu, sigma, w, consts, regress, with_code):
    N, M, H, W = delta.shape
    mu_out, w_out, sigma_out = torch.empty_like(mu), torch.empty_like(w), torch.empty_like(sigma)
    disp = torch.empty((N, 1, H, W), device=delta.device, dtype=torch.float32) if regress else None
    code = torch.empty((N, M, H, W), device=delta.device, dtype=torch.uint8) if with_code else None
    _ffi.call("dkt_pcv_update_fwd", delta, delta.data_ptr(), mu.data_ptr(), sigma.data_ptr(), w.data_ptr(),
              mu_out.data_ptr(), w_out.data_ptr(), sigma_out.data_ptr(), _ffi.ptr(disp), _ffi.ptr(code), N, M, H, W, *consts)
    return mu_out, w_out, sigma_out, disp, code


class _UpdateFn(torch.autograd.Function):
    """(delta, mu, sigma, w) -> (mu', w', sigma', disp | None).  Saves the inputs and the decision bytes; the backward is
    one dkt_pcv_update_bwd, given only the upstream gradients that exist and asked only for what requires grad."""

    @staticmethod
    def forward(ctx, delta, mu, sigma, w, consts, regress):
        mu_out, w_out, sigma_out, disp, code = _forward(delta, mu, sigma, w, consts, regress, True)
        ctx.save_for_backward(delta, mu, sigma, w, code)
        ctx.consts = consts
        ctx.set_materialize_grads(False)
        return mu_out, w_out, sigma_out, disp

    @staticmethod
    def backward(ctx, gmu_out, gw_out, gsigma_out, gdisp=None):
        delta, mu, sigma, w, code = ctx.saved_tensors
        N, M, H, W = delta.shape
        ups = [None if g is None else g.float().contiguous() for g in (gmu_out, gw_out, gsigma_out, gdisp)]
        need = ctx.needs_input_grad[:4]
        if all(g is None for g in ups) or not any(need):
            return (None,) * 6
        res = [torch.empty_like(delta) if n else None for n in need]          # gdelta, gmu, gsigma, gw
        _ffi.call("dkt_pcv_update_bwd", delta, delta.data_ptr(), mu.data_ptr(), sigma.data_ptr(), w.data_ptr(), code.data_ptr(),
                  *[_ffi.ptr(g) for g in ups], *[_ffi.ptr(r) for r in res], N, M, H, W, *ctx.consts)
        return tuple(res) + (None, None)


def parameters_update(delta, mu, sigma, w, *, sigma0=0.5, eps=1e-3, gammas=(1, 1, 1), regress=True):
    """delta, mu, sigma, w (N, M, H, W), M = gauss_num in 1..8 -> (mu, w, sigma, disp | None): update.py:92-107, and with
    ``regress`` model.py:154's disp (N, 1, H, W).  Differentiable with respect to the four tensors.  Non-fp32 inputs are cast
    and copies made here, outside the node: autograd undoes them."""
    shape = tuple(delta.shape)
    if len(shape) != 4 or any(tuple(t.shape) != shape for t in (mu, sigma, w)):
        raise _ffi.DktError("parameters_update: delta %s, mu %s, sigma %s, w %s must be four (N, M, H, W) tensors of one shape"
                            % (shape, tuple(mu.shape), tuple(sigma.shape), tuple(w.shape)))
    if not 1 <= shape[1] <= MAX_GAUSSIANS:
        raise _ffi.DktError("parameters_update: %d gaussians outside 1..%d" % (shape[1], MAX_GAUSSIANS))
    gammas = tuple(float(g) for g in gammas)
    if len(gammas) != 3:
        raise _ffi.DktError("parameters_update: gammas must be three numbers")
    if not delta.is_cuda:
        return parameters_update_torch(delta, mu, sigma, w, sigma0, eps, gammas, regress)
    ts = [t.float().contiguous() for t in (delta, mu, sigma, w)]
    _ffi.require_gpu(*ts)
    consts = (float(sigma0), float(eps)) + gammas
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        return _UpdateFn.apply(*ts, consts, bool(regress))
    return _forward(*ts, consts, bool(regress), False)[:4]


class ParametersUpdater(nn.Module):
    """meta_arch/pcvnet/update.py:76-108: the conv head (this library's convolutions) and parameters_update."""

    def __init__(self, args, input_dim, hidden_dim):
        super().__init__()
        self.args = args
        self.head = FlowHead(input_dim, hidden_dim, args.gauss_num)
        self.sigma0 = 0.5
        self.eps = 1e-3
        self.gamma1 = 1
        self.gamma2 = 1
        self.gamma3 = 1

    def _delta(self, hidden_state):
        head = self.head
        if not hidden_state.is_cuda or (torch.is_grad_enabled() and (
                hidden_state.requires_grad or any(p.requires_grad for p in head.parameters()))):
            return conv2d_autograd(conv2d_autograd(hidden_state, head.conv1, relu=True), head.conv2)
        return head(hidden_state)

    def forward(self, hidden_state, mu, sigma, w, regress=False):
        """-> (mu, w, sigma) as the reference returns them; ``regress=True`` appends disp = sum_j w mu."""
        out = parameters_update(self._delta(hidden_state), mu, sigma, w, sigma0=self.sigma0, eps=self.eps,
                                gammas=(self.gamma1, self.gamma2, self.gamma3), regress=regress)
        return out if regress else out[:3]


def mixture_upsample(disp, mu, sigma, w, up_mask, factor):
    """model.py:165-174.  disp (N,1,H,W), mu / sigma / w (N,G,H,W), up_mask (N, 9 factor^2, H, W) ->
    disp_up (N,1,fH,fW) and mu_up, sigma_up, w_up (N G, 1, fH, fW).  The mask receives disp's gradient only, as in the
    reference (the other three calls detach it)."""
    factor = int(factor)
    if factor < 1 or factor & (factor - 1):
        raise _ffi.DktError("mixture_upsample: factor %d is not a power of two (2 ** n_downsample); pre-dividing w by it "
                            "would round" % factor)
    N, G, H, W = mu.shape
    disp_up = convex_upsample(disp.float(), up_mask.float(), factor)
    stack = torch.cat((mu.float(), sigma.float(), w.float() * (1.0 / factor)), dim=1)
    up = convex_upsample(stack, up_mask.detach().float(), factor)
    mu_up, sigma_up, w_up = (t.reshape(N * G, 1, factor * H, factor * W) for t in up.split(G, dim=1))
    return disp_up, mu_up, sigma_up, w_up
