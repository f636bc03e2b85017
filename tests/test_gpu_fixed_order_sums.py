"""The loss scalars of the fixed-order fp64 sums (csrc/wave_reduce.h) against their CPU restatement, bit for bit.

test_losses_are_deterministic compares two runs of the same code, and the loss tests' reference data has a narrow dynamic
range where fp64 adds are exact in any order; here the terms span 2^-30 .. 2^9 with 24 bits each and the totals are
steered onto a rounding boundary of the fp32 result (tests/_fixed_order_ref.py), so another association of the same
terms -- the blocks in another order, a lane added out of turn -- changes the loss bits
(tests/test_host_fixed_order_ref.py checks that this holds for every case below).

Shapes.  Sequence losses, one block per 1024 pixels: B=1, 5x7 is one partly filled tile, fewer than 64 partials for the
finalize; B=3, 176x1025, n=3 is 531 partials (one unrolled pass of 512, then the tail), the last tile of each image partly
filled.  ns_loss, one block per 16x16 pixels: B=1, 40x56 is 12 blocks with ragged tiles; B=2, 272x256 is 544 blocks."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _fixed_order_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEQ = [(kind,) + c for kind in ("raft", "gwc") for c in R.SEQ_CASES[kind]]
IDS = lambda c: "-".join(str(v) for v in c[:-1]) if isinstance(c, tuple) else None


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(x):
    return int(torch.as_tensor(x).detach().cpu().reshape(1).view(torch.int32)) if torch.is_tensor(x) else int(np.float32(x).view(np.int32))


@functools.lru_cache(maxsize=None)
def _seq(case):
    kind, B, H, W, n, skips = case
    gts, preds, _ = R.draw(kind, B, H, W, n, 2, skips)
    return gts, preds, R.seq_loss(kind, preds, gts)


@pytest.mark.parametrize("case", SEQ, ids=IDS)
def test_single_target_loss_bits(case):
    from dkt_stereo_amd.loss import loss_gwcnet, sequence_loss_raft
    gts, preds, want = _seq(case)
    res = {"disp_preds": [G(p[:, None]) for p in preds]}
    gt, valid = G(gts[0][:, None]), torch.ones(gts[0].shape, device=DEV)
    if case[0] == "raft":
        loss, _, mask = sequence_loss_raft(res, gt, valid)
    else:
        loss, _, mask = loss_gwcnet(res, gt, valid, args=SimpleNamespace(maxdisp=192))
    assert bool(mask.all())
    assert bits(loss) == bits(want[0]), (case, bits(loss), bits(want[0]))


@pytest.mark.parametrize("case", SEQ, ids=IDS)
def test_loss_pair_bits(case):
    from dkt_stereo_amd.loss import dkt_loss_pair
    gts, preds, want = _seq(case)
    res = {"disp_preds": [G(p[:, None]) for p in preds]}
    valid = torch.ones(gts[0].shape, device=DEV)
    name = "sequence_loss_raft" if case[0] == "raft" else "loss_gwcnet"
    l_gt, _, v_gt, l_pl, v_pl = dkt_loss_pair(name, res, G(gts[0][:, None]), valid, G(gts[1][:, None]), valid,
                                              args=SimpleNamespace(maxdisp=192))
    assert bool(v_gt.all()) and bool(v_pl.all())
    assert (bits(l_gt), bits(l_pl)) == (bits(want[0]), bits(want[1])), case


@pytest.mark.parametrize("case", R.NS_CASES, ids=IDS)
def test_ns_loss_disparity_bits(case):
    from dkt_stereo_amd.ns_loss import ns_loss
    B, H, W, n, skips = case
    (t,), preds, conf = R.draw("ns", B, H, W, n, 1, skips)
    want = R.ns_disp_loss(preds, t, conf)
    ims = [torch.rand(B, 3, H, W, device=DEV, generator=torch.Generator(DEV).manual_seed(k)) for k in range(3)]
    loss, _, valid = ns_loss([G(p[:, None]) for p in preds], G(t), G(conf), *ims, alpha_photometric=0.0)
    assert bool(valid.all())
    assert bits(loss) == bits(want), (case, bits(loss), bits(want))
