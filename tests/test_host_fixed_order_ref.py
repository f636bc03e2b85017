"""The CPU restatement of the fixed-order sums (tests/_fixed_order_ref.py) on the inputs of test_gpu_fixed_order_sums.py:
it is a sum of the right terms (math.fsum truth), and on these inputs another association of the same terms changes the
bits of the LOSS.  The second is a condition on the inputs, not a measurement: the loss is an fp32 scalar and resolves an
fp64 rounding difference only where the total sits on a rounding boundary, which is where _fixed_order_ref.steer puts it
(the loss tests' own data has a narrow dynamic range, where every order gives the exact sum).

Two mutants.  One addition after the other in place of the butterfly must show in every case.  The blocks in another
order must show in every case whose partials fill more than one row of the column sum (more than 64 blocks), where a
lane adds several partials in turn; with fewer, every lane holds one partial and the order enters only through the
pairing of the butterfly, which the first mutant covers (and a one-block case has nothing to permute), so the block
order is pinned by the large cases."""
import math

import numpy as np
import pytest

import _fixed_order_ref as R

SEQ = [(kind,) + c for kind in ("raft", "gwc") for c in R.SEQ_CASES[kind]]
IDS = lambda c: "-".join(str(v) for v in c[:-1]) if isinstance(c, tuple) else None


def _shows(loss, nblk, pick=lambda o: o):
    """(the permuted block order changes the loss bits or is not required to, the sequential sum changes them)"""
    mine, perm = pick(loss()).view(np.int32), np.random.default_rng(0).permutation(nblk)
    return (nblk <= 64 or pick(loss(perm=perm)).view(np.int32) != mine,
            pick(loss(sequential=True)).view(np.int32) != mine)


@pytest.mark.parametrize("case", SEQ, ids=IDS)
def test_seq_loss_order_shows(case):
    kind, B, H, W, n, skips = case
    gts, preds, _ = R.draw(kind, B, H, W, n, 2, skips)
    loss = lambda **m: R.seq_loss(kind, preds, gts, **m)
    for k in range(2):              # either target alone (sequence_loss_raft / loss_gwcnet take the first only)
        assert _shows(loss, B * -(-H * W // 1024), lambda o: o[k]) == (True, True), k
    for g in gts:
        for p in preds:
            x = R.loss_term(kind, p, g).astype(np.float64)
            truth = math.fsum(x.ravel().tolist())
            assert abs(R.column_sum(R.seq_partials(x.reshape(B, -1))) - truth) <= 1e-12 * truth


@pytest.mark.parametrize("case", R.NS_CASES, ids=IDS)
def test_ns_loss_order_shows(case):
    B, H, W, n, skips = case
    (t,), preds, conf = R.draw("ns", B, H, W, n, 1, skips)
    loss = lambda **m: R.ns_disp_loss(preds, t, conf, **m)
    assert _shows(loss, B * -(-H // 16) * -(-W // 16)) == (True, True)
    for p in preds:
        x = (np.abs(p - t) * conf).astype(np.float64)
        truth = math.fsum(x.ravel().tolist())
        assert abs(R.column_sum(R.ns_partials(x)) - truth) <= 1e-12 * truth


def test_butterfly_lane0_equals_down_tree():
    """Lane 0 of the __shfl_down tree has the butterfly's partners at every step (csrc/wave_reduce.h)."""
    v = 2.0 ** np.random.default_rng(3).uniform(-40, 40, (256, 64))
    d = v.copy()
    for sh in (32, 16, 8, 4, 2, 1):
        d[:, :64 - sh] = d[:, :64 - sh] + d[:, sh:]
    assert np.array_equal(d[:, 0], R.butterfly(v))
