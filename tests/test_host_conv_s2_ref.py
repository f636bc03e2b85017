"""_conv_s2_ref.py checked on the CPU: the emulation of each stride-2 backward kernel and torch's own fp32 gradients meet every
bound at every magnitude of the upstream gradient; the device scale is necessary (unit scale misses GX_BOUND at 2^-40); the
mutants a kernel of this shape can turn into -- a dropped parity, a dropped tap, a lost last odd row or column, a lost slice --
miss the bounds on the seven non-degenerate cases; the restated plan covers every output row exactly once.

The two 1x1 cases have no odd taps (the odd rows and columns of gx are zero, the odd rows and columns of x are never read),
so the odd-row / odd-column mutants cannot show there: for them the test asserts the exact zeros instead.
Every figure is printed (run with -s)."""
import pytest
import torch

import _conv_s2_ref as S


def _io(case, m):
    x, w, b, gy, y = S.inputs(case)
    return x, w, S.masked(case, m)


@pytest.mark.parametrize("case", S.CASES, ids=S.CASE_IDS)
def test_emulation_and_torch_meet_the_bounds(case):
    B, H, W, k, cin, cout = case
    for m in S.KS:
        x, w, gp = _io(case, m)
        gx, gw, bound = S.truth_gx(gp, w, (H, W)), S.truth_gw(x, gp, k), S.b_bound(x, gp, k)
        for name, got_gx, got_gw in (("torch fp32", S.torch32_gx(gp, w, (H, W)), S.torch32_gw(x, gp, k)),
                                     ("emulation", S.emulate_gx(gp, w, (H, W)), S.emulate_gw(case, x, gp))):
            e_gx, e_a = S.gx_error(got_gx, gx), S.a_error(got_gw, gw)
            ok_b, r_b = S.b_ratio(got_gw, gw, bound)
            print("case %s m=%d %s: gx %.2e  gw (a) %.2e  (b) ratio %.3f" % (case, m, name, e_gx, e_a, r_b))
            assert e_gx <= S.GX_BOUND and e_a <= S.A_BOUND and ok_b, (case, m, name)


@pytest.mark.parametrize("case", S.NONDEGENERATE, ids=S.CASE_IDS[3:])
def test_unit_scale_misses_at_a_small_gradient(case):
    B, H, W, k, cin, cout = case
    x, w, gp = _io(case, -40)
    err = S.gx_error(S.emulate_gx(gp, w, (H, W), e=0), S.truth_gx(gp, w, (H, W)))
    print("case %s: unit-scale emulation at 2^-40, gx error %.2e" % (case, err))
    assert err > S.GX_BOUND


@pytest.mark.parametrize("case", S.NONDEGENERATE, ids=S.CASE_IDS[3:])
def test_mutants_miss_the_bounds(case):
    B, H, W, k, cin, cout = case
    x, w, gp = _io(case, 0)
    gx, gw, bound = S.truth_gx(gp, w, (H, W)), S.truth_gw(x, gp, k), S.b_bound(x, gp, k)
    parity = (1, 1) if k == 3 else (0, 0)
    tap = (0, 0)
    gx_mutants = {"dropped parity": dict(drop_parity=parity), "dropped tap": dict(drop_tap=tap)}
    gw_mutants = {"dropped tap": dict(drop_tap=tap), "lost slice": dict(drop_slice=B * S.plan(case)[1] - 1)}
    if k == 3:
        for what in ("row", "col"):
            gx_mutants["lost last odd " + what] = dict(lose_odd=what)
            gw_mutants["lost last odd " + what] = dict(lose_odd=what)
    else:
        good = S.emulate_gx(gp, w, (H, W))
        assert not good[:, :, 1::2].any() and not good[:, :, :, 1::2].any() and good[:, :, ::2, ::2].any()
        assert not gx[:, :, 1::2].any() and not gx[:, :, :, 1::2].any()
    for name, kw in gx_mutants.items():
        err = S.gx_error(S.emulate_gx(gp, w, (H, W), **kw), gx)
        print("case %s gx %s: error %.2e" % (case, name, err))
        assert err > S.GX_BOUND, (case, name)
    for name, kw in gw_mutants.items():
        got = S.emulate_gw(case, x, gp, **kw)
        ok_b, r_b = S.b_ratio(got, gw, bound)
        print("case %s gw %s: (a) %.2e  (b) ratio %.3g" % (case, name, S.a_error(got, gw), r_b))
        assert not ok_b, (case, name)
    # zeroing the last column of g' (a kernel that loses the column tile's tail)
    cut = gp.clone()
    cut[:, :, :, -1] = 0
    err = S.gx_error(S.emulate_gx(cut, w, (H, W)), gx)
    print("case %s gx without the last column of g': error %.2e" % (case, err))
    assert err > S.GX_BOUND


@pytest.mark.parametrize("case", S.CASES + [(2, 320, 720, 3, 64, 96), (2, 160, 360, 1, 96, 128), (8, 80, 180, 3, 128, 128)],
                         ids=lambda c: "x".join(str(v) for v in c))
def test_plan_covers_every_output_row_once(case):
    rows, bands, n_co, n_ci = S.plan(case)
    Ho, Wo = S.out_size(case[1], case[2])
    seen = torch.zeros(Ho, dtype=torch.int32)
    for r0, r1 in S.bands_of(case):
        assert 0 <= r0 < r1 <= Ho and r0 % S.TILE_ROWS == 0
        seen[r0:r1] += 1
    assert bool((seen == 1).all())
    assert rows % S.TILE_ROWS == 0 and n_co == -(-case[5] // S.BLOCK) and n_ci == -(-case[4] // S.BLOCK)


def test_cases_keep_bound_b_discriminating():
    for case in S.CASES:
        Ho, Wo = S.out_size(case[1], case[2])
        assert case[0] * Ho * Wo <= 1105, case
