"""The plan-regime cases of the conv backward kernels checked on the CPU (no device): PLAN_CASES of _conv_wgrad_ref.py and
_conv_s2_ref.py, PREPASS_PLAN_CASES of _conv_grad_ref.py and the seeded small shapes of _conv_wgrad_ref.drawn_cases -- what
test_gpu_conv_grad_plans.py runs on the device.

  * every regime the cases are there for is met, asserted from the restated plan: a change of the plan's constants fails
    here instead of leaving the device test at "one item per block" without a word;
  * on every case the references (the emulation of the kernel's arithmetic, torch's own fp32) meet A_BOUND and bound (b);
  * a kernel that loses one 2 x 32 tile of g', one slice, or every item past the first 256 misses A_BOUND on every walked
    case -- the bounds see what a walked plan can lose;
  * emulate_gb (the pre-pass's summation order restated) is inside gb_bound and has the sum's exact properties.

Every figure is printed (run with -s).  Largest seen on the plan cases: references (a) 3.1e-6 of the 5e-6 allowed, (b)
ratio 0.09; a lost tile (a) 3.5e-2 or more, a lost slice 0.12 or more, the lost late items 0.26 or more.  On the drawn
cases: (a) 1.7e-6, (b) ratio 0.30, the stride-2 gx 6.1e-7."""
import pytest
import torch

import _conv_grad_ref as R
import _conv_s2_ref as S
import _conv_wgrad_ref as WR

STRIDES = {1: (WR.PLAN_CASES, WR.WALKED, WR.MIXED, WR.regime_of), 2: (S.PLAN_CASES, S.WALKED, S.MIXED, S.regime_of)}
ALL = [(s, c) for s in (1, 2) for c in STRIDES[s][0]]
_id = lambda v: "s%d-%s" % (v[0], "x".join(str(n) for n in v[1]))


def _operands(stride, case):
    """x, g' (masked by the random saved output), the grid's rows."""
    x, _, _, gy, y = WR.drawn_inputs(case, stride)
    return x, R.mask(gy, y), (case[1] if stride == 1 else S.out_size(case[1], case[2])[0])


def _refs(stride, case, x, gp):
    k = case[3]
    if stride == 1:
        return WR.truth(x, gp, k), WR.b_bound(x, gp, k), {"emulation": WR.emulate(x, gp, k), "torch fp32": WR._cw(x, gp, k)}
    return S.truth_gw(x, gp, k), S.b_bound(x, gp, k), {"emulation": S.emulate_gw(case, x, gp), "torch fp32": S.torch32_gw(x, gp, k)}


# --------------------------------------------------------------------------------------------------------- the regimes
@pytest.mark.parametrize("stride", [1, 2])
def test_every_required_regime_is_met(stride):
    cases, walked, mixed, regime_of = STRIDES[stride]
    regs = {c: regime_of(c) for c in cases}
    for c in walked:
        assert regs[c]["items"] > WR.CUS, (c, regs[c]["items"])
    for c in cases:
        if c not in walked:
            assert regs[c]["items"] <= WR.CUS
    # T = 2048 walked, with k = 3 and with k = 1
    for k in (3, 1):
        assert any(regs[c]["T"] == 2048 and c[3] == k for c in walked), k
    # T = 1024: one column tile, a shorter last band, items of odd and of even tile count in one launch
    m = regs[mixed]
    assert mixed in walked and m["T"] == 1024 and m["tiles_w"] == 1
    assert m["tiles"][-1] < m["tiles"][0] and {t & 1 for t in m["tiles"]} == {0, 1}
    if stride == 1:
        # ... and on the part the plan is named after (256 blocks) a block starts a later item at an odd tile count: the
        # stride-1 kernel's buffer parity is then the opposite of a first item's
        assert WR.odd_start(m), "no item starts at an odd running tile count"
    # T = 512 walked
    assert any(regs[c]["T"] == 512 for c in walked)
    if stride == 1:
        # a block takes a third item somewhere: the running tile count is carried twice
        assert any(regs[c]["items"] > 2 * WR.CUS for c in walked)
    # the finishing kernel strides, at a tiny image
    assert any(c[4] * c[5] * c[3] ** 2 > WR.FINISH_STRIDE and regs[c]["items"] <= 32 and regs[c]["slices"] == 1 for c in cases)
    # channel tails on both sides in one walked case; odd W (stride 2: and odd H) in one walked case
    assert any(c[4] % WR.BLOCK and c[5] % WR.BLOCK for c in walked)
    assert any(c[2] % 2 == 1 and (stride == 1 or c[1] % 2 == 1) for c in walked)
    # a walked case leaves the 16-byte path open (W, and at stride 2 Wo, multiples of 4)
    assert any(c[2] % 4 == 0 and (stride == 1 or S.out_size(c[1], c[2])[1] % 4 == 0) for c in walked)
    # more than one slice per weight and more than one band everywhere it is walked
    for c in walked:
        assert regs[c]["slices"] > c[0] > 1


def test_the_fixed_cases_never_leave_one_item_per_block():
    """Why PLAN_CASES exist: every fixed case has at most 24 items and stops at T = 512."""
    for c in WR.CASES:
        assert WR.regime_of(c)["items"] <= 24 and WR.regime_of(c)["T"] == 512
    for c in S.CASES:
        assert S.regime_of(c)["items"] <= 24 and S.regime_of(c)["T"] == 512


def test_operands_stay_small():
    for stride, case in ALL:
        B, H, W, k, cin, cout = case
        Ho, Wo = (H, W) if stride == 1 else S.out_size(H, W)
        assert 4 * B * cin * H * W < 150e6 and 4 * B * cout * Ho * Wo < 150e6, case


def test_prepass_regimes():
    regs = {c: R.prepass_regime(c) for c in R.PREPASS_PLAN_CASES}
    assert any(r["nseg"] >= 2 and r["last"] < 1024 for r in regs.values())
    assert any(r["nseg"] >= 2 and r["last"] == R.PRE_SEG for r in regs.values())
    assert any(r["items"] > R.PRE_BLOCKS for r in regs.values())
    assert any(c[1] > 2 * R.PRE_THREADS and r["per_thread"] == 3 for c, r in regs.items())
    assert any(not r["vec"] for r in regs.values()) and any(r["vec"] for r in regs.values())
    for c in R.CASES:                                       # the fixed cases: one segment, at most 256 items and channels
        assert c[1] * c[2] <= R.PRE_SEG and c[0] * c[5] <= 256
    # the three places the maximum is planted in (test_gpu_conv_grad_plans.py) are what they are called
    case = R.PREPASS_PLAN_CASES[0]
    B, C, H, W = case
    assert R.item_of(case, B - 1, C - 1, H * W - 1) >= R.PRE_BLOCKS and C - 1 >= 2 * R.PRE_THREADS


# ------------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("sc", ALL, ids=_id)
def test_references_meet_the_bounds_and_mutants_miss(sc):
    stride, case = sc
    x, gp, rows = _operands(stride, case)
    exact, bound, refs = _refs(stride, case, x, gp)
    for name, got in refs.items():
        ea = WR.a_error(got, exact)
        ok, rb = WR.b_ratio(got, exact, bound)
        print("s%d %s %s: (a) %.2e  (b) ratio %.2e" % (stride, case, name, ea, rb))
        assert ea <= WR.A_BOUND, (case, name, ea)
        assert ok, (case, name, rb)
    if case not in STRIDES[stride][1]:
        return
    reg = STRIDES[stride][3](case)
    for name, lost in WR.mutants(x, gp, case[3], stride, reg, rows).items():
        ea = WR.a_error(refs["emulation"] - lost, exact)
        print("s%d %s without %s: (a) %.2e" % (stride, case, name, ea))
        assert ea > WR.A_BOUND, (case, name, ea)


@pytest.mark.parametrize("stride", [1, 2])
def test_references_meet_the_bounds_on_the_drawn_cases(stride):
    cases = WR.drawn_cases(stride)
    assert len(cases) == 40 and cases == WR.drawn_cases(stride)
    assert {c[3] for c in cases} == {1, 3} and any(c[2] % 4 for c in cases) and any(c[2] % 4 == 0 for c in cases)
    worst = [0.0, 0.0, 0.0]
    for case in cases:
        B, H, W, k, cin, cout = case
        x, w, _, gy, y = WR.drawn_inputs(case, stride)
        gp = R.mask(gy, y)
        exact, bound, refs = _refs(stride, case, x, gp)
        for name, got in refs.items():
            ea = WR.a_error(got, exact)
            ok, rb = WR.b_ratio(got, exact, bound)
            worst[0], worst[1] = max(worst[0], ea), max(worst[1], rb)
            assert ea <= WR.A_BOUND and ok, (case, name, ea, rb)
        if stride == 2:
            gx = S.truth_gx(gp, w, (H, W))
            for got in (S.emulate_gx(gp, w, (H, W)), S.torch32_gx(gp, w, (H, W))):
                e = S.gx_error(got, gx)
                worst[2] = max(worst[2], e)
                assert e <= S.GX_BOUND, (case, e)
    print("stride %d, 40 drawn cases: gw (a) %.2e  (b) ratio %.2e  gx %.2e" % (stride, *worst))


# --------------------------------------------------------------------------------------------------------- emulate_gb
@pytest.mark.parametrize("case", R.PREPASS_PLAN_CASES, ids=R.PREPASS_PLAN_IDS)
def test_emulate_gb_is_inside_the_bound(case):
    gy, y = R.prepass_inputs(case)
    for gp in (gy, R.mask(gy, y), gy * 2.0 ** -20):
        d = (R.emulate_gb(gp).double() - gp.double().sum(dim=(0, 2, 3))).abs()
        bound = R.gb_bound(gp)
        print("case %s: emulate_gb |d|/bound %.2e" % (case, float((d / bound).max())))
        assert bool((d <= bound).all())
    # a power-of-two multiple goes through every addition unchanged
    assert torch.equal(R.emulate_gb(gy * 2.0 ** -20), R.emulate_gb(gy) * 2.0 ** -20)


def test_emulate_gb_exact_properties():
    """What holds for the sum in any order: zero gradient -> zeros; one non-zero element -> that element, wherever it sits
    (the last element of a partial segment, an item past the launch's width, a channel of the finish's third round)."""
    shapes = [(c[0], c[5], c[1], c[2]) for c in R.CASES] + R.PREPASS_PLAN_CASES
    for B, C, H, W in shapes:
        z = torch.zeros(B, C, H, W)
        assert torch.equal(R.emulate_gb(z), torch.zeros(C))
        for b, c, e in ((0, 0, 0), (B - 1, C - 1, H * W - 1), (B // 2, C // 2, (H * W) // 2)):
            g = z.clone()
            g.view(B, C, -1)[b, c, e] = -1.7
            want = torch.zeros(C)
            want[c] = -1.7
            assert torch.equal(R.emulate_gb(g), want), (B, C, H, W, b, c, e)
    # ... and the order is NOT that of a plain sum: the restatement is about the order
    gy = R.prepass_inputs(R.PREPASS_PLAN_CASES[0])[0]
    assert not torch.equal(R.emulate_gb(gy), gy.sum(dim=(0, 2, 3)))
