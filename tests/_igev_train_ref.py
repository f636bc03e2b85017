"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

The fp64 truth of IGEV-Stereo's training loop (test_host_igev_train_ref.py, test_gpu_igev_train.py): igev_stereo.py:199-217
with test_mode=False from the point where this library's operators take over, at quarter resolution 16 x 24, B = 1, two
iterations.

The model of a draw: BasicMultiUpdateBlockIGEV with seeded weights, hidden states and context inputs built as in
test_gpu_gru_train.py, a seeded geometry volume (1, 8, 12, 16, 24) and feature pair (1, 16, 16, 24), a seeded initial
disparity, and a stand-in for the up-sampling head spx_2_gru / spx_gru (which needs the timm feature network): two
ConvTranspose2d(k=4, s=2, p=1), 32 -> 32 -> 9, no activation between them.

train_forward() restates the loop on state dicts, in their dtype, from oracle/torch_oracle.py (geo_pyramids,
update_block(..., igev=True)); geo_lookup is restated because the oracle's ends in .float() and builds its taps in fp32.  Per
iteration: disp.detach(), lookup, the optional slow-fast calls, the update block, disp + delta, the head, then
_context_upsample_ref.sequence_logits (igev_stereo.py:145-146).

loss(preds, ws) = sum_i mean(pred_i * w_i), grad_error (max|got - want| / max|want| per parameter) and G_BOUND = 5e-5 are
those of _raft_train_ref.py.  The gradient is discontinuous where a ReLU input changes sign, and fp32 puts a few
activations on the other side of 0 from fp64; so the node arm is compared with the truth at the first draw of DRAWS at
which the torch arm -- the same driver and the same update block with the reference's expression sequence for the
up-sampling, hence the same low-resolution states bit for bit -- is itself within G_BOUND of the truth on every parameter.
test_host_igev_train_ref.py shows on the CPU how many of the draws an fp32 restatement is within G_BOUND at."""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import _context_upsample_ref as CR
import _synth
from _raft_train_ref import G_BOUND, grad_error, loss, loss_weights, worst  # noqa: F401
from oracle import torch_oracle as to

DRAWS = range(10)
H, W, ITERS = 16, 24, 2
GEO_C, GEO_D, FEAT_C, LEVELS, RADIUS = 8, 12, 16, 2, 4
VARIANTS = [dict(), dict(slow_fast_gru=True), dict(n_gru_layers=2)]


def key(overrides):
    return tuple(sorted(overrides.items()))


def config(case=()):
    cfg = dict(corr_levels=LEVELS, corr_radius=RADIUS, n_downsample=2, n_gru_layers=3, hidden_dims=[128, 128, 128],
               slow_fast_gru=False)
    cfg.update(dict(case))
    return cfg


class Head(torch.nn.Module):
    """The stand-in for spx_2_gru (which also takes the stem features: ignored here) and spx_gru."""

    def __init__(self):
        super().__init__()
        self.up1 = torch.nn.ConvTranspose2d(32, 32, 4, 2, 1)
        self.up2 = torch.nn.ConvTranspose2d(32, 9, 4, 2, 1)

    def spx_2_gru(self, mask_feat_4, stem_2x=None):
        return self.up1(mask_feat_4)

    def spx_gru(self, x):
        return self.up2(x)


def make_block(case, seed):
    """BasicMultiUpdateBlockIGEV on the CPU with the weights of draw `seed`."""
    from dkt_stereo_amd.update import BasicMultiUpdateBlockIGEV
    cfg = config(case)
    blk = BasicMultiUpdateBlockIGEV(SimpleNamespace(**cfg), hidden_dims=cfg["hidden_dims"])
    blk.load_state_dict(_synth.torch_state_dict(_synth.shapes_of(blk), 21 + seed))
    return blk.eval()


def make_head(seed):
    head = Head()
    g = torch.Generator().manual_seed(9000 + seed)
    with torch.no_grad():
        for p in head.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.1 if p.dim() > 1 else 0.5))
    return head.eval()


@functools.lru_cache(maxsize=None)
def inputs(case, seed):
    """dict(net, inp, m1, m2, geo, disp, coords, ws) of a draw: float32 CPU tensors (ws: float64)."""
    n = config(case)["n_gru_layers"]
    g = torch.Generator().manual_seed(8000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    net = [torch.tanh(rn(1, 128, H >> i, W >> i)) for i in range(n)]
    inp = [[0.5 * rn(1, 128, H >> i, W >> i) for _ in range(3)] for i in range(n)]
    m1, m2 = rn(1, FEAT_C, H, W), rn(1, FEAT_C, H, W)
    geo = rn(1, GEO_C, GEO_D, H, W)
    disp = 8.0 * torch.rand(1, 1, H, W, generator=g)
    coords = torch.arange(W).float().reshape(1, 1, W, 1).repeat(1, H, 1, 1)
    return dict(net=net, inp=inp, m1=m1, m2=m2, geo=geo, disp=disp, coords=coords, ws=loss_weights(seed, ITERS, 1, 4 * H, 4 * W))


def state_dict(blk, head, dtype):
    sd = {"update_block." + k: v.detach().to(dtype) for k, v in blk.state_dict().items()}
    sd.update({"head." + k: v.detach().to(dtype) for k, v in head.state_dict().items()})
    return sd


def param_names(blk, head):
    return ["update_block." + n for n, _ in blk.named_parameters()] + ["head." + n for n, _ in head.named_parameters()]


def geo_lookup(geo_pyr, init_pyr, disp, coords, radius):
    """to.geo_lookup in the dtype of its operands (taps included, no .float() at the end)."""
    b, _, h, w = disp.shape
    dx = torch.linspace(-radius, radius, 2 * radius + 1, dtype=disp.dtype).view(1, 1, 2 * radius + 1, 1)
    dn = disp.reshape(b * h * w, 1, 1, 1)
    cn = coords.reshape(b * h * w, 1, 1, 1)
    outs = []
    for i in range(len(geo_pyr)):
        g = to._sample_rows(geo_pyr[i], dx + dn / 2 ** i).view(b, h, w, -1)
        c0 = to._sample_rows(init_pyr[i], cn / 2 ** i - dn / 2 ** i + dx).view(b, h, w, -1)
        outs += [g, c0]
    return torch.cat(outs, dim=-1).permute(0, 3, 1, 2).contiguous()


def head_logits(sd, mask_feat_4):
    x = F.conv_transpose2d(mask_feat_4, sd["head.up1.weight"], sd["head.up1.bias"], stride=2, padding=1)
    return F.conv_transpose2d(x, sd["head.up2.weight"], sd["head.up2.bias"], stride=2, padding=1)


def train_forward(sd, cfg, x, iters=ITERS):
    """(preds, per-iteration low-resolution disparities, final hidden states) of the loop in the dtype of `sd`."""
    dtype = sd["head.up1.weight"].dtype
    n, slow_fast = cfg["n_gru_layers"], cfg.get("slow_fast_gru", False)
    t = lambda a: a.to(dtype)  # noqa: E731
    gp, ip = to.geo_pyramids(t(x["m1"]), t(x["m2"]), t(x["geo"]), cfg["corr_levels"])
    coords, disp = t(x["coords"]), t(x["disp"])
    net, inp = [t(a) for a in x["net"]], [[t(a) for a in s] for s in x["inp"]]
    ub = lambda net, **kw: to.update_block(sd, "update_block", n, list(net), inp, igev=True, **kw)  # noqa: E731
    preds, disps, held = [], [], []
    for _ in range(iters):
        disp = disp.detach()
        feat = geo_lookup(gp, ip, disp, coords, cfg["corr_radius"])
        if n == 3 and slow_fast:
            net = ub(net, it_coarse=True, it_mid=False, it_fine=False, update=False)
        if n >= 2 and slow_fast:
            net = ub(net, it_coarse=(n == 3), it_mid=True, it_fine=False, update=False)
        net, mask, delta = ub(net, corr=feat, flow=disp, it_coarse=(n == 3), it_mid=(n >= 2))
        disp = disp + delta
        preds.append(CR.sequence_logits(disp, head_logits(sd, mask)).unsqueeze(1))
        disps.append(disp.detach())
        held += [feat, mask, delta, disp] + list(net)
    for a in held + preds:
        assert a.dtype == dtype, "an intermediate left %s for %s" % (dtype, a.dtype)
    return preds, disps, net


def grads(case, seed, dtype):
    """({name: gradient or None} of the loss of draw `seed` in `dtype` on the CPU, predictions)."""
    blk, head = make_block(case, seed), make_head(seed)
    names = param_names(blk, head)
    sd = state_dict(blk, head, dtype)
    for k in names:
        sd[k] = sd[k].clone().requires_grad_(True)
    x = inputs(case, seed)
    preds, _, _ = train_forward(sd, config(case), x)
    got = torch.autograd.grad(loss(preds, x["ws"]), [sd[k] for k in names], allow_unused=True)
    return dict(zip(names, got)), [p.detach() for p in preds]


@functools.lru_cache(maxsize=None)
def truth(case, seed):
    return grads(case, seed, torch.float64)


@functools.lru_cache(maxsize=None)
def fp32(case, seed):
    return grads(case, seed, torch.float32)
