"""The on-the-fly correlation lookup (-m gpu): dkt_corr1d_lookup_otf behind corr.PytorchAlternateCorrBlock1D on every path
a block can take -- the staged window with one or two rows, an empty window, a window of exactly 64 columns, the general
gather for irregular lanes, differing rows and wide spans -- at channel counts that leave waves and half-waves empty, at
radius 0 / 1 / 8 and at levels narrower than the window.

Every case of _otf_ref.CASES is compared with the float64 truth of _otf_ref.alt64 over ALL elements under

    |got - truth| <= 2 c u mag + 2^-126,  u = 2^-24,  c = n(C) + lv + 9

(derived in _otf_ref.py; test_host_otf_ref.py shows that both oracles meet it with their own counts, that every mutant of
the truth breaks it, and that each case reaches the paths it names), with the NaN rule, exact zeros wherever the truth's
magnitude is zero, and a second call returning the same bits.  Each case prints the kernel's worst error in units of
u * mag and as a fraction of the bound, overall and per path (run with -s)."""
import numpy as np
import pytest
import torch

import _otf_ref as R
from _gru_ref import same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 9.0
PAD = 64


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(c, f1, f2, co):
    """Two results of the same call, on the host.  raw: through the C ABI into the middle of a canary-filled buffer."""
    from dkt_stereo_amd import _ffi
    from dkt_stereo_amd.corr import PytorchAlternateCorrBlock1D
    blk = PytorchAlternateCorrBlock1D(G(f1), G(f2), num_levels=c["L"], radius=c["r"])
    cd = G(co)
    if not c.get("raw"):
        return blk(cd).cpu(), blk(cd).cpu()
    shape = (c["B"], c["L"] * (2 * c["r"] + 1), c["H"], c["W1"])
    n = int(np.prod(shape))
    outs = []
    for _ in range(2):
        flat = torch.full((n + 2 * PAD,), CANARY, device=DEV)
        out = flat[PAD:PAD + n]
        _ffi.call("dkt_corr1d_lookup_otf", cd, blk.fmap1.data_ptr(), _ffi.ptr_array(blk._f2pyr), cd.data_ptr(),
                  out.data_ptr(), c["B"], c["C"], c["H"], c["W1"], c["W2"], c["L"], c["r"])
        flat = flat.cpu()
        assert bool((flat[:PAD] == CANARY).all()) and bool((flat[PAD + n:] == CANARY).all()), "canaries overwritten"
        outs.append(flat[PAD:PAD + n].view(shape).clone())
    return outs


def _per_path(c, paths, got, truth, cmag, mag):
    """{label: (worst u * mag, worst fraction of the bound)} over the elements of the blocks with that label."""
    K = 2 * c["r"] + 1
    lab = np.repeat(paths["label"], R.SEG, axis=2)[:, :, :c["W1"]]          # (B, H, W1, L)
    lab = np.repeat(np.transpose(lab, (0, 3, 1, 2)), K, axis=1)              # (B, L*K, H, W1)
    out = {}
    for l in sorted(set(lab.reshape(-1))):
        m = torch.from_numpy(lab == l)
        nan = torch.full_like(truth, float("nan"))
        out[l] = R.worst(torch.where(m, got.double(), nan), torch.where(m, truth, nan), cmag, mag)
    return out


@pytest.mark.parametrize("name", list(R.CASES))
@torch.no_grad()
def test_otf_case(name, c_oracle):
    c = R.CASES[name]
    f1, f2, co = R.case_inputs(name)
    truth, mag, cmag = R.case_truth(name)
    y_c = c_oracle.corr1d_lookup_alt(f1, f2, co, c["L"], c["r"])
    got, again = _run(c, f1, f2, co)
    in_u, of_bound = R.worst(got, truth, cmag, mag)
    paths = _per_path(c, R.case_paths(name), got, truth, cmag, mag)
    print("otf %-16s u*mag %.2f (of the bound %.3f); %s" % (
        name, in_u, of_bound, ", ".join("%s %.2f (%.3f)" % ((l,) + v) for l, v in paths.items())))
    ok, msg = R.nan_rule(got, truth, y_c)
    assert ok, (name, msg)
    assert bool(torch.isnan(got).any()) == bool(c.get("nans", False)), name
    assert of_bound <= 1.0, (name, in_u, of_bound)
    zero = (mag == 0) & ~torch.isnan(truth)
    assert bool((got[zero] == 0).all()), (name, "a number where every contributing value is padding")
    if c.get("zeros"):
        assert bool(zero.any()), name
    assert same(got, again), name
