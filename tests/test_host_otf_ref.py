"""The reference module of the on-the-fly correlation lookup (_otf_ref.py) checked on the CPU: every fixed case reaches the
kernel paths it was written for (by the model of the kernel's dispatch), no earlier input of the suite reaches an empty
window, both oracles meet the bound with their own operation counts, every mutant of the truth breaks the kernel's bound, the
restatement is torch's float64 arithmetic, and the entry point refuses bad arguments before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import _otf_ref as R
from oracle import torch_oracle as to

T = torch.from_numpy


# ---- the cases reach their paths ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_case_reaches_its_paths(name):
    c = R.CASES[name]
    p = R.case_paths(name)
    lab = p["label"]
    found = sorted(set(lab.reshape(-1)))
    print("%-16s %s" % (name, ", ".join("%s x%d" % (l, int((lab == l).sum())) for l in found)))
    assert set(found) <= set(R.LABELS)
    for l in c["must"]:
        assert l in found, (name, l, found)
    if c["only"] is not None:
        assert set(found) <= set(c["only"]), (name, found)
    for lv, n in c.get("empty", {}).items():
        here = lab[..., lv] == "window_empty"
        assert here.all() if n == "all" else int(here.sum()) == n, (name, lv, int(here.sum()))
    if "ncol" in c:
        assert (p["ncol"] == c["ncol"]).all(), (name, p["ncol"])
    if c.get("outside"):
        win = np.isin(lab, R.WINDOW) & p["outside"]
        assert win[0].any() and win[1].any(), name             # clipped on the left (item 0) and on the right (item 1)
    if c.get("one_live"):
        assert (p["live"] == 1).any(), name
    if c.get("far"):
        assert (np.isin(lab, R.WINDOW) & p["far"]).any(), name
    if "all_levels" in c:
        for lv in range(c["L"]):
            assert set(lab[..., lv].reshape(-1)) <= set(c["all_levels"]), (name, lv)


def test_specific_paths():
    """What the case table promises beyond labels."""
    assert (R.case_paths("half_row")["label"] == "window_two_rows").all()
    # rows -1 and >= H: every element of row 0 of item 0 and all of item 1 is an exact zero of the truth
    truth, mag, _ = R.case_truth("row_outside")
    assert bool((mag[0, :, 0] == 0).all()) and bool((mag[1] == 0).all()) and bool((mag[0, :, 1:] > 0).any())
    # the empty windows are zeros of the truth
    for name in ("empty_left", "empty_right"):
        c = R.CASES[name]
        truth, mag, _ = R.case_truth(name)
        lab = R.case_paths(name)["label"]
        K = 2 * c["r"] + 1
        for b, h, s, lv in zip(*np.nonzero(lab == "window_empty")):
            blk = mag[b, lv * K:(lv + 1) * K, h, s * R.SEG:(s + 1) * R.SEG]
            assert bool((blk == 0).all()) and bool((truth[b, lv * K:(lv + 1) * K, h, s * R.SEG:(s + 1) * R.SEG] == 0).all())
    # the channel counts leave waves and half-waves empty as described
    assert [R.chain(c) for c in (1, 3, 17, 48, 72, 132, 256)] == [1, 1, 5, 12, 16, 17, 32]


def test_existing_inputs_have_no_empty_window():
    """Why the empty_* cases exist: nothing the suite ran through the kernel before them has a block without a column."""
    seen = set()
    for name, (co, H, W1, W2, L, r) in R.existing_inputs().items():
        lab = R.block_paths(co, H, W1, W2, L, r)["label"]
        assert not (lab == "window_empty").any(), name
        seen |= set(lab.reshape(-1))
    assert "window_one_row" in seen and "general_rows" in seen and "general_wide" in seen


# ---- the oracles meet the bound -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_oracles_meet_the_bound(name, c_oracle):
    c = R.CASES[name]
    f1, f2, co = R.case_inputs(name)
    truth, mag, _ = R.case_truth(name)
    y_c = T(c_oracle.corr1d_lookup_alt(f1, f2, co, c["L"], c["r"]))
    # (the torch restatement, like the reference, pools once more after its last level and cannot run a level of width 1)
    y_t = to.corr1d_lookup_alt(T(f1), T(f2), T(co), c["L"], c["r"]) if c.get("torch", True) else y_c
    assert bool(torch.equal(torch.isnan(truth), torch.isnan(y_c))), name          # one NaN pattern
    assert bool(torch.isnan(truth).any()) == bool(c.get("nans", False)), name
    line = []
    for who, y, c_of in (("C", y_c, R.c_c_oracle), ("torch", y_t, R.c_torch))[:2 if c.get("torch", True) else 1]:
        in_u, of_bound = R.worst(y, truth, R.cmag_of(mag, c_of, c["C"], c["L"], c["r"]), mag)
        line.append("%s %.2f (%.3f)" % (who, in_u, of_bound))
        assert of_bound <= 1.0, (name, who, in_u, of_bound)
        ok, msg = R.nan_rule(y, truth, y_c)
        assert ok, (name, who, msg)
    print("%-16s u*mag (of its bound): %s" % (name, ", ".join(line)))
    if c.get("zeros"):
        z = (mag == 0) & ~torch.isnan(truth)
        assert bool(z.any()) and bool((y_c[z] == 0).all()) and bool((y_t[z] == 0).all())


# ---- the bound discriminates --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutants_break_the_kernel_bound(mutant):
    """Each mutant of the truth, rounded to fp32, exceeds the KERNEL's bound on some case (where the unmutated fp32 oracles
    pass, test_oracles_meet_the_bound)."""
    hit = []
    for name, c in R.CASES.items():
        f1, f2, co = R.case_inputs(name)
        truth, mag, cmag = R.case_truth(name)
        wrong = R.alt64(f1, f2, co, c["L"], c["r"], mutant=mutant)[0]
        wrong = torch.where(torch.isnan(truth), truth, wrong).float()
        if R.worst(wrong, truth, cmag, mag)[1] > 1.0:
            hit.append(name)
    print("%-13s caught on %s" % (mutant, ", ".join(hit)))
    assert hit, mutant


# ---- the restatement itself ---------------------------------------------------------------------------------------------
FAR_FROM_INTEGRAL = ("chan_17", "chan_gather_72", "half_row", "clipped_edges", "ragged_33", "radius_1", "span_64")


@pytest.mark.parametrize("name", FAR_FROM_INTEGRAL)
def test_truth_is_float64_torch(name):
    """With the coordinate round trip in float64 too, alt64 is corr1d_lookup_alt on float64 tensors: to 1e-12 of the
    magnitude plus the half ulp of the fp32 cast that ends the oracle.  (Coordinates far from integral: both agree on
    every floor.)"""
    c = R.CASES[name]
    f1, f2, co = R.case_inputs(name)
    mine, mag = R.alt64(f1, f2, co, c["L"], c["r"], positions="fp64")
    want = to.corr1d_lookup_alt(T(f1).double(), T(f2).double(), T(co).double(), c["L"], c["r"]).double()
    assert bool(((mine - want).abs() <= 1e-12 * mag + R.U * mine.abs() + R.FLOOR).all()), name
    # and the fp32 positions move it by what their rounding allows: the round trip's three roundings move a position by
    # <= 3 u |ix| <= 3 u 160 = 2.9e-5 of a column on each axis, hence a weight by as much
    truth = R.case_truth(name)[0]
    far = (mine - truth).abs().max() / mag.max()
    print("%-16s fp32 vs fp64 positions: %.2e of max mag" % (name, float(far)))
    assert float(far) < 1e-4


# ---- the entry point's refusals -----------------------------------------------------------------------------------------
def test_abi_refusals_before_launch():
    """dkt_corr1d_lookup_otf validates on the host (device -1: nothing is launched)."""
    from dkt_stereo_amd import _ffi
    lib = _ffi.lib()
    null = ctypes.c_void_p(0)
    nullpp = ctypes.cast(null, ctypes.POINTER(ctypes.c_void_p))
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    arr = (ctypes.c_void_p * 8)(*([p.value] * 8))
    pp = ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p))
    hole = (ctypes.c_void_p * 8)(p.value, None, p.value, p.value, p.value, p.value, p.value, p.value)
    holepp = ctypes.cast(hole, ctypes.POINTER(ctypes.c_void_p))
    f = lib.dkt_corr1d_lookup_otf
    E_NULL, E_SHAPE, E_LEVELS, E_RADIUS = -1, -2, -3, -4
    assert f(null, pp, p, p, 1, 4, 2, 8, 8, 1, 4, -1, null) == E_NULL
    assert f(p, nullpp, p, p, 1, 4, 2, 8, 8, 1, 4, -1, null) == E_NULL
    assert f(p, pp, null, p, 1, 4, 2, 8, 8, 1, 4, -1, null) == E_NULL
    assert f(p, pp, p, null, 1, 4, 2, 8, 8, 1, 4, -1, null) == E_NULL
    assert f(p, holepp, p, p, 1, 4, 2, 8, 8, 2, 4, -1, null) == E_NULL           # level 1 of 2 is null
    assert f(p, holepp, p, p, 1, 4, 2, 8, 8, 1, 4, -1, null) != E_NULL           # ... and is not looked at with one level
    for B in (0, -1, 65536):
        assert f(p, pp, p, p, B, 4, 2, 8, 8, 1, 4, -1, null) == E_SHAPE
    for dims in ((0, 2, 8, 8), (4, 0, 8, 8), (4, 2, 0, 8), (4, 2, 8, 0)):
        assert f(p, pp, p, p, 1, *dims, 1, 4, -1, null) == E_SHAPE
    assert f(p, pp, p, p, 1, 4, 2, 8, 8, 0, 4, -1, null) == E_LEVELS
    assert f(p, pp, p, p, 1, 4, 2, 8, 8, 9, 4, -1, null) == E_LEVELS
    assert f(p, pp, p, p, 1, 4, 2, 8, 8, 5, 4, -1, null) == E_LEVELS            # 8 >> 4 == 0
    assert f(p, pp, p, p, 1, 4, 2, 8, 8, 1, -1, -1, null) == E_RADIUS
    assert f(p, pp, p, p, 1, 4, 2, 8, 8, 1, 9, -1, null) == E_RADIUS


# ---- the Python wrapper's shape checks ----------------------------------------------------------------------------------
def test_block_refuses_mismatched_shapes(monkeypatch):
    """PytorchAlternateCorrBlock1D raises ValueError before any launch when the feature maps disagree in (B, C, H) or the
    coordinates are not (B, 2, H, W1): the kernel would read out of range.  _ffi.call is stubbed to record launches."""
    from dkt_stereo_amd import _ffi, corr
    launched = []
    monkeypatch.setattr(_ffi, "require_gpu", lambda *t: None)
    monkeypatch.setattr(_ffi, "call", lambda name, *a, **k: launched.append(name) or 0)
    f1 = torch.zeros(2, 4, 3, 16)
    for bad in ((1, 4, 3, 16), (2, 5, 3, 16), (2, 4, 2, 16)):
        with pytest.raises(ValueError):
            corr.PytorchAlternateCorrBlock1D(f1, torch.zeros(*bad), num_levels=2, radius=1)
    assert launched == []
    blk = corr.PytorchAlternateCorrBlock1D(f1, torch.zeros(2, 4, 3, 24), num_levels=2, radius=1)     # W2 may differ
    assert launched == ["dkt_pool_w"]
    for bad in ((2, 2, 3, 15), (2, 1, 3, 16), (1, 2, 3, 16), (2, 2, 4, 16), (2, 3, 16), (2, 2, 3, 24)):
        with pytest.raises(ValueError):
            blk(torch.zeros(*bad))
    assert launched == ["dkt_pool_w"]
    assert tuple(blk(torch.zeros(2, 2, 3, 16)).shape) == (2, 6, 3, 16)
    assert launched == ["dkt_pool_w", "dkt_corr1d_lookup_otf"]
