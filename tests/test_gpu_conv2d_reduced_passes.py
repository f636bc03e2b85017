"""conv2d_f16s_kernel at one and two passes (the backends "f16" and "f16x2", what args.mixed_precision runs) against the fp64
convolution of exactly the operands those pass counts are defined to multiply (tests/_conv2d_ref.py), on every row of
CONV_TILE_TABLE in every variant the reduced-pass translation units instantiate, and at three passes wherever no other file
asserts the tile.  The checks, inside conv.use_backend(...) -- every launch is held to 1, and to 2 and 3 either directly or,
for the pair launches of the gate epilogues, by being bit for bit (4) a lone launch that is:

  1. layer_tile(...) answers the tile the case is named after: a tuning that moves a threshold fails here, loudly, and does
     not quietly test another kernel;
  2. max|got - conv_ref| <= 3e-6 max(1, max|ref|), the project's split-fp16 bound: products of fp16 operands are exact in
     fp32, only the accumulation is left (gate epilogues: 1e-5, the bound of test_gpu_conv2d_epilogue_bodies.py -- hardware
     exp / rcp; the device-scaled form: 3e-6 max(magnitude, max|ref|), the gradient's own scale);
  3. at one and two passes max|got - exact| >= 1e-5 max|exact|: the reduced arithmetic did run;
  4. placement, bit for bit: the batch with its items rotated by one, the batch against one item at a time, a layer alone
     against the first and the second problem of a pair launch.  Two launches agree bit for bit when they accumulate in the
     same order, i.e. on tiles of the same chunk size CK (chunk, tap, 16-channel step is the order of the main loop; the
     64 x 8 tile alone has CK = 1): a single item or a pair partner that layer_tile sends to a tile of the other chunk size
     is compared with the reference instead.

All inputs are randn * 1.5 + 0.3 in 40 channels (ragged over the 16- and the 32-channel chunk: more than one chunk, a
partial last one; the 64 x 8 row, whose 16-channel chunks come from sources padded to 32, also at 56), widths are ragged (250 = 7 column tiles + 26).  tests/test_host_conv2d_ref.py proves without a device
that every channel configuration here is discriminating: the one-pass model, the two-pass model, the exact convolution and
a model that skips one (tap, 16-channel chunk) lie >= 3e-5 of max|y| apart, ten times the bound.

Every comparison prints `RP <group> <case> p<passes> err/bound <ratio> off <distance to the exact convolution>` before it
asserts.  Largest err/bound per group over all pass counts, measured on an MI355X (bound: 1), and the smallest distance of a
reduced-pass result to the exact convolution (check 3 asks >= 1e-5):
  plain          0.232  (64x8_cin56, an item alone on the 64 x 4 tile, three passes)     1.85e-4
  1x1            0.093  (stride2_subsampled, three passes)                               2.18e-4
  stride 2       0.200  (96_p3)                                                          1.88e-4
  in-norm        0.241  (64x8_cin56, three passes)                                       1.90e-4
  device-scaled  0.221  (64x8_cin56, three passes; unit and 2^-18 magnitudes alike)      1.85e-4
  pair           0.190  (64x8 as the first problem, three passes)                        1.90e-4
  epilogues      0.243  (stats_64x8_cin56; residual <= 0.21; gates 0.179 of their 1e-5)  1.40e-4, gates 7.9e-5
  range          0.147  (128x2_exp-4)                                                    2.00e-4
One and two passes sit where three do (0.21 at most): what is left is the fp32 accumulation, as the bound supposes.  The
same bound added to test_gpu_conv.py::test_conv_vs_fp64 measures 0.44 at most (k3_cat3: 384 input channels).  No case came
near the bound and no kernel had to be changed.

Value-only mutants this file was run against once each on an MI355X (built aside, never kept): failing cases of the 223 here,
and what the convolution tests of the suite before this file noticed (104 cases: test_gpu_conv.py without the bound this
change adds to test_conv_vs_fp64, test_gpu_conv2d_epilogues.py, test_gpu_conv2d_epilogue_bodies.py,
test_gpu_random.py::test_conv_random, test_gpu_round6.py):
  1 the two-pass step skips its w_lo*x_hi MFMAs          every two-pass case here (68 of 68), no other; there: nothing
  2 conv_run sends passes == 1 to the two-pass units     every one-pass case here (68 of 68), no other; there: nothing
  3 the weight packer writes w_hi at scale / 2           every case here, three passes included; there 77 of 104 (gross: the
                                                         one-pass result halves, w_lo loses its low bits)
  4 CK == 1, PASSES < 3: a tile's last 16-channel        16 here: every one- and two-pass case of the 64 x 8 row at 56 and 64
    chunk adds nothing                                   channels (plain, in-norm, device-scaled at both magnitudes, residual,
                                                         statistics) and the pair launch whose 24-channel partner rides on that
                                                         tile; the 40-channel cases cannot see it (their last chunk is padding):
                                                         the 56-channel cases were added for it.  There: only the end-to-end
                                                         tests (test_reduced_pass_backends_report_their_deviation,
                                                         test_mixed_precision_flag: 7.5 px), no operator test
  5 in-norm staging applies the ReLU before the          all 18 in-norm cases here, three passes included; there 13 (the in-norm
    normalisation: (relu(x) - mean) / std                operator tests and the end-to-end fixtures).  The ReLU moved in front of
                                                         the multiplication by 1/std alone is no mutant: 1/std > 0, bit-identical
Mutants 1 and 2 are what the bounds of 1e-3 / 3e-3 could not see; the bound added to test_conv_vs_fp64 catches both as well (7
of its cases each).
"""
import collections

import pytest
import torch

import _conv2d_ref as cr
from test_host_conv2d_tile import DSCALE, NORM, PAIR, SINGLE, layer_tile, table_rows

DEV = "cuda:0"
gpu = pytest.mark.gpu
BACKEND = {1: "f16", 2: "f16x2", 3: "f16x3"}

# ---- the rows of CONV_TILE_TABLE: (WM, WN, NF, MF, ST, CK) -------------------------------------------------------------------
R32, R64X8, R64X4, R96 = (1, 4, 1, 1, 1, 2), (1, 4, 2, 2, 1, 1), (1, 4, 1, 2, 1, 2), (1, 4, 1, 3, 1, 2)
R128X2, R128X4, R4X96 = (2, 2, 1, 2, 1, 2), (2, 2, 2, 2, 1, 2), (4, 1, 2, 3, 1, 2)
R256X1, R8W, R256X2 = (4, 1, 1, 2, 1, 2), (4, 2, 2, 2, 1, 2), (4, 1, 2, 2, 1, 2)
S96, S128X4, S128X2, S256X1 = (1, 4, 1, 3, 2, 1), (2, 2, 2, 2, 2, 1), (2, 2, 1, 2, 2, 2), (4, 1, 1, 2, 2, 2)
P123, P12, P3 = (1, 2, 3), (1, 2), (3,)

#: group: what the docstring's table is keyed on; srcs: the channels of the cat operands; tile: (WM, WN, NF, MF, ST, CK) as
#: the kernel RUNS (a 1x1 stride-2 layer reports ST = 1); epi: ConvArgs.epi; o: what the group's test needs beyond that
Case = collections.namedtuple("Case", "group name B srcs H W cout ks stride form passes tile epi o")


def _c(group, name, shape, cout, tile, ks=3, stride=1, form=SINGLE, passes=P123, epi=0, srcs=None, **o):
    B, cin, H, W = shape
    return Case(group, name, B, tuple(srcs or (cin,)), H, W, cout, ks, stride, form, passes, tile, epi, o)


def want_tile(c):
    return (0, c.ks) + tuple(c.tile)


#: the 3x3 stride-1 rows; (4, 64, 126, 250) -> 64 has >= 192 eight-row tiles: at one and two passes it must stay on the generic
#: kernel (the weights-stationary kernel is three-pass only and has its own tests).  The 64 x 8 row stages 16-channel chunks of
#: sources padded to 32 channels: 40 channels leave its last chunk all padding, so every variant of that row also runs at 56
#: channels (a partial last chunk) -- mutant 4 of the docstring is invisible without them
PLAIN = [
    _c("plain", "32x4", (1, 40, 13, 45), 24, R32),
    _c("plain", "64x8", (4, 40, 126, 250), 64, R64X8),
    _c("plain", "64x8_cin64", (4, 64, 126, 250), 64, R64X8, passes=P12),
    _c("plain", "64x8_cin56", (4, 56, 126, 250), 64, R64X8),
    _c("plain", "64x4", (2, 40, 13, 45), 48, R64X4),
    _c("plain", "96", (2, 40, 50, 250), 80, R96),
    _c("plain", "128x2", (1, 40, 21, 70), 112, R128X2),
    _c("plain", "128x4", (2, 40, 50, 250), 112, R128X4),
    _c("plain", "4x96", (2, 40, 63, 250), 300, R4X96),
    _c("plain", "256x1", (1, 40, 21, 70), 200, R256X1),
    _c("plain", "8wave", (2, 40, 62, 250), 200, R8W),
    _c("plain", "256x2", (1, 40, 59, 250), 200, R256X2),
    _c("plain", "256x2_two_blocks", (1, 40, 30, 250), 400, R256X2),
]
#: stride 2: (2, 40, 129, 500) gives 2 * 8 * 33 = 528 two-row tiles, more than the 512 resident blocks -- reached at reduced
#: passes only, three passes take the P3 rows from 512 four-row tiles on ((2, 40, 129, 999): 2 * 16 * 17 = 544)
STRIDE2 = [
    _c("stride2", "128x2_few", (1, 40, 47, 81), 96, S128X2, stride=2),
    _c("stride2", "128x2_528_tiles", (2, 40, 129, 500), 96, S128X2, stride=2),
    _c("stride2", "256x1_few", (1, 40, 47, 81), 200, S256X1, stride=2),
    _c("stride2", "256x1_many", (2, 40, 129, 500), 200, S256X1, stride=2),
    _c("stride2", "96_p3", (2, 40, 129, 999), 96, S96, stride=2, passes=P3),
    _c("stride2", "128x4_p3", (2, 40, 129, 999), 112, S128X4, stride=2, passes=P3),
]
K1 = [
    _c("1x1", "32x4", (1, 40, 13, 45), 24, R32, ks=1),
    _c("1x1", "64x4", (2, 40, 50, 250), 64, R64X4, ks=1),
    _c("1x1", "128x2", (1, 40, 21, 70), 112, R128X2, ks=1),
    _c("1x1", "128x4", (2, 40, 50, 250), 112, R128X4, ks=1),
    _c("1x1", "256x1", (1, 40, 21, 70), 200, R256X1, ks=1),
    _c("1x1", "256x2", (2, 40, 62, 250), 200, R256X2, ks=1),
    _c("1x1", "stride2_subsampled", (2, 40, 99, 499), 96, R128X4, ks=1, stride=2),
]
#: the NRM column of the table
NORMED = [
    _c("in-norm", "64x8", (4, 40, 126, 250), 64, R64X8, form=NORM),
    _c("in-norm", "64x8_cin56", (4, 56, 126, 250), 64, R64X8, form=NORM),
    _c("in-norm", "64x4", (2, 40, 13, 45), 48, R64X4, form=NORM),
    _c("in-norm", "96", (2, 40, 50, 250), 80, R96, form=NORM),
    _c("in-norm", "128x2", (1, 40, 21, 70), 112, R128X2, form=NORM),
    _c("in-norm", "128x4", (2, 40, 50, 250), 112, R128X4, form=NORM),
]
#: the DSC column: every stride-1 row, at the plain cases' shapes
DSCALED = [_c("device-scaled", c.name, (c.B, c.srcs[0], c.H, c.W), c.cout, c.tile, form=DSCALE)
           for c in PLAIN if c.name not in ("64x8_cin64", "256x2_two_blocks")]
#: the PAIR column; partner: a layer of the same width class, another input width (24 channels) and another size.  Two cases
#: where the pair form changes the tile: 80 channels (no 96-channel wave tile in a pair launch), 300 (no four waves of 96)
PARTNER_SHAPE = (1, 24, 11, 37)
PAIRED = [
    _c("pair", "32x4", (1, 40, 13, 45), 24, R32, form=PAIR, partner=20),
    _c("pair", "64x8", (4, 40, 126, 250), 64, R64X8, form=PAIR, partner=40),
    _c("pair", "64x4", (2, 40, 13, 45), 48, R64X4, form=PAIR, partner=56),
    _c("pair", "128x2", (1, 40, 21, 70), 112, R128X2, form=PAIR, partner=100),
    _c("pair", "128x4", (2, 40, 50, 250), 112, R128X4, form=PAIR, partner=72),
    _c("pair", "256x1", (1, 40, 21, 70), 200, R256X1, form=PAIR, partner=136),
    _c("pair", "8wave", (2, 40, 62, 250), 200, R8W, form=PAIR, partner=136),
    _c("pair", "256x2", (1, 40, 59, 250), 200, R256X2, form=PAIR, partner=136),
    _c("pair", "80_to_128x4", (2, 40, 50, 250), 80, R128X4, form=PAIR, partner=128),
    _c("pair", "300_to_8wave", (2, 40, 63, 250), 300, R8W, form=PAIR, partner=260),
]
#: the residual join (both relu settings) and the output statistics on the 64 x 8 and 128 x 4 rows
EPILOGUES = [
    _c("epilogues", "residual_64x8", (4, 40, 126, 250), 64, R64X8, epi=3),
    _c("epilogues", "residual_64x8_cin56", (4, 56, 126, 250), 64, R64X8, epi=3),
    _c("epilogues", "residual_128x4", (2, 40, 50, 250), 112, R128X4, epi=3),
    _c("epilogues", "stats_64x8", (4, 40, 126, 250), 64, R64X8, stats=True),
    _c("epilogues", "stats_64x8_cin56", (4, 56, 126, 250), 64, R64X8, stats=True),
    _c("epilogues", "stats_128x4", (2, 40, 50, 250), 112, R128X4, stats=True),
]
#: the ConvGRU of core/update.py:23-32, 128 hidden + 256 / 64 input channels at 24 x 60 and 20 x 45 (the shapes of _gates()
#: in test_gpu_conv2d_epilogue_bodies.py): the merged z|r convolution (epi 1) and the q convolution (epi 2)
GATES = [
    _c("epilogues", "gate_zr_a", (1, 384, 24, 60), 256, R256X1, epi=1, srcs=(128, 256)),
    _c("epilogues", "gate_zr_b", (1, 192, 20, 45), 256, R256X1, epi=1, srcs=(128, 64)),
    _c("epilogues", "gate_zr_pair", (1, 384, 24, 60), 256, R256X1, epi=1, srcs=(128, 256), form=PAIR),
    _c("epilogues", "gate_q_a", (1, 384, 24, 60), 128, R128X2, epi=2, srcs=(128, 256)),
    _c("epilogues", "gate_q_b", (1, 192, 20, 45), 128, R128X2, epi=2, srcs=(128, 64)),
    _c("epilogues", "gate_q_pair", (1, 384, 24, 60), 128, R128X2, epi=2, srcs=(128, 256), form=PAIR),
]
#: range control: layer.dkt_in_exp = -4 with inputs x 16, = 6 with inputs x 2^-6 (bias-free layers: the result is then the
#: unscaled one times the exact power of two)
RANGED = [
    _c("range", "32x4_exp-4", (1, 40, 13, 45), 24, R32, in_exp=-4),
    _c("range", "128x2_exp-4", (1, 40, 21, 70), 112, R128X2, in_exp=-4),
    _c("range", "64x4_exp6", (2, 40, 13, 45), 48, R64X4, in_exp=6),
    _c("range", "256x1_exp6", (1, 40, 21, 70), 200, R256X1, in_exp=6),
]
ALL_CASES = PLAIN + STRIDE2 + K1 + NORMED + DSCALED + PAIRED + EPILOGUES + GATES + RANGED


def _each(cases):
    """(case, passes) for every pass count of every case, a case's pass counts next to each other (they share its data)."""
    return [pytest.param(c, p, id="%s-p%d" % (c.name, p)) for c in cases for p in c.passes]


# ---- no device: the case list against the selection and the table ----------------------------------------------------------
def make_layer(c, device, bias=True, seed=None):
    torch.manual_seed(1000 + sum(c.srcs) + c.cout + 7 * c.ks if seed is None else seed)
    return torch.nn.Conv2d(sum(c.srcs), c.cout, c.ks, stride=c.stride, padding=c.ks // 2, bias=bias).to(device)


def make_partner(c, device):
    """The second layer of a pair case and its input shape."""
    B, cin, H, W = PARTNER_SHAPE
    torch.manual_seed(2000 + c.cout)
    return torch.nn.Conv2d(cin, c.o["partner"], c.ks, padding=c.ks // 2).to(device), PARTNER_SHAPE


def _shape(c):
    return (c.B, sum(c.srcs), c.H, c.W)


def _tile(c, passes, form=None, shape=None, layer=None):
    layer = make_layer(c, "cpu") if layer is None else layer
    return layer_tile(shape or _shape(c), layer, form=c.form if form is None else form, passes=passes, epilogue=c.epi,
                      src_channels=c.srcs)


@pytest.mark.parametrize("c", ALL_CASES, ids=["%s-%s" % (c.group, c.name) for c in ALL_CASES])
def test_case_tiles_are_what_the_selection_answers(c):
    """What every GPU case asserts before it launches, asked without a device."""
    for p in c.passes:
        assert _tile(c, p) == want_tile(c), p
    if c.form == PAIR and "partner" in c.o:
        from dkt_stereo_amd import conv
        assert conv.pair_eligible(make_layer(c, "cpu"), make_partner(c, "cpu")[0])


def test_every_row_and_variant_of_the_shape_table_has_a_case():
    """Every row of CONV_TILE_TABLE, in every variant its flags instantiate at the reduced pass counts (3x3; K1: 1x1; NRM:
    in-norm; DSC: device scales; PAIR: the first of a pair launch) and at three passes for the P3 rows, is the tile of a case
    here -- cases that all compare values with the reference.  A row added to the table arrives with its cases."""
    have = set()
    for c in ALL_CASES:
        for p in c.passes:
            have.add((tuple(c.tile), c.ks, c.form, p))
    for row in table_rows():
        shape, (k1, nrm, dsc, pair, p3) = row[:6], row[6:]
        need = [(3, SINGLE)] + [(1, SINGLE)] * k1 + [(3, NORM)] * nrm + [(3, DSCALE)] * dsc + [(3, PAIR)] * pair
        for ks, form in need:
            for p in (P3 if p3 else P12):
                assert (shape, ks, form, p) in have, (shape, ks, form, p)
        if p3:
            assert not any(h[0] == shape and h[3] != 3 for h in have), shape
    assert {h[0] for h in have} == {r[:6] for r in table_rows()}


# ---- shared data of a case: built once, shared by its pass counts -----------------------------------------------------------
#: ONE slot: the inputs and fp64 references of the large cases are hundreds of MB each, and pytest runs a case's pass counts
#: next to each other (_each), so the slot is rebuilt once per case.  Any other order (-k, a random-order plugin, several
#: workers) only rebuilds more often; nothing depends on what an earlier test left here (test_range_exponent restores
#: layer.dkt_in_exp before it returns).
_DATA = {}


def _data(key, build):
    if _DATA.get("key") != key:
        _DATA.clear()
        _DATA.update(key=key, val=build())
    return _DATA["val"]


def _input(shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, device=DEV, generator=g) * 1.5 + 0.3) * scale, g


def _judge(c, tag, passes, got, ref, exact=None, bound=cr.BOUND, floor=1.0):
    """Checks 2 and 3 of the docstring; prints before it asserts."""
    assert got.shape == ref.shape and got.dtype == torch.float32
    r = cr.ratio(got, ref, bound, floor)
    off = cr.distance(got, exact) if exact is not None and passes < 3 else float("nan")
    print("RP %s %s%s p%d err/bound %.3f off %.2e" % (c.group, c.name, tag, passes, r, off))
    assert r <= 1.0, (c.name, tag, passes, r)
    if exact is not None and passes < 3:
        assert off >= cr.OFF, (c.name, tag, passes, off)


def _same_order(tile_a, tile_b):
    """Two launches accumulate in the same order: tiles of the generic kernel with the same chunk size CK."""
    return isinstance(tile_a, tuple) and isinstance(tile_b, tuple) and tile_a[0] == tile_b[0] == 0 and tile_a[7] == tile_b[7]


def _placement(c, passes, layer, x, got, run, ref, form=None):
    """Check 4 for a batched launch: run(x_sub, b0, b1) -> the result of items [b0, b1) launched on their own."""
    B = x.shape[0]
    if B > 1:                                        # the same tile, every item under another batch index
        rolled = run(x.roll(1, 0), None)
        assert torch.equal(rolled.roll(-1, 0), got), "rolled batch"
    one = _tile(c, passes, form=form, shape=(1,) + tuple(x.shape[1:]), layer=layer)
    for b in range(B):
        item = run(x[b:b + 1], b)
        if _same_order(one, want_tile(c)):
            assert torch.equal(item[0], got[b]), b
        else:
            _judge(c, "[item %d on %s]" % (b, "x".join(str(v) for v in one[2:])), passes, item, ref[b:b + 1])


# ---- plain launches: 3x3, 1x1, stride 2 -------------------------------------------------------------------------------------
def _build_plain(c):
    layer = make_layer(c, DEV)
    x, _ = _input(_shape(c), 11 + c.cout)
    relu = c.cout % 16 == 0                           # (half of the cases with the ReLU)
    return dict(layer=layer, x=x, relu=relu, exact=cr.conv_ref(x, layer, 3, relu=relu))


@gpu
@torch.no_grad()
@pytest.mark.parametrize("c,passes", _each(PLAIN + STRIDE2 + K1))
def test_plain_launch(c, passes):
    from dkt_stereo_amd import conv
    d = _data((c.group, c.name), lambda: _build_plain(c))
    layer, x, relu = d["layer"], d["x"], d["relu"]
    with conv.use_backend(BACKEND[passes]):
        assert conv.hip_eligible(layer) and not conv.few_eligible(layer) and not conv.direct_eligible(layer)
        assert _tile(c, passes, layer=layer) == want_tile(c)
        ref = cr.conv_ref(x, layer, passes, relu=relu)
        got = conv.conv2d(x, layer, relu=relu)
        _judge(c, "", passes, got, ref, d["exact"])
        _placement(c, passes, layer, x, got, lambda xx, b: conv.conv2d(xx, layer, relu=relu), ref)


# ---- range control ----------------------------------------------------------------------------------------------------------
@gpu
@torch.no_grad()
@pytest.mark.parametrize("c,passes", _each(RANGED))
def test_range_exponent(c, passes):
    from dkt_stereo_amd import conv
    e = c.o["in_exp"]

    def build():
        layer = make_layer(c, DEV, bias=False)
        x, _ = _input(_shape(c), 17 + c.cout)
        return dict(layer=layer, x=x, xs=x * 2.0 ** -e)
    d = _data((c.group, c.name), build)
    layer, x, xs = d["layer"], d["x"], d["xs"]
    with conv.use_backend(BACKEND[passes]):
        assert _tile(c, passes, layer=layer) == want_tile(c)
        layer.dkt_in_exp = 0
        plain = conv.conv2d(x, layer)
        try:
            layer.dkt_in_exp = e
            got = conv.conv2d(xs, layer)
            _judge(c, "", passes, got, cr.conv_ref(xs, layer, passes, in_exp=e), cr.conv_ref(xs, layer, 3))
        finally:
            layer.dkt_in_exp = 0
        assert torch.equal(got, plain * 2.0 ** -e)        # the same fp16 operands, the exact power of two in the epilogue


# ---- the input's instance norm in the staging -------------------------------------------------------------------------------
def _check_stats(c, out, st, ref):
    """The statistics conv2d_stats leaves behind, as test_many_tiles_conv2d_stats checks them."""
    from dkt_stereo_amd import extractor
    norm = torch.nn.InstanceNorm2d(c.cout)
    got = extractor.instance_norm_params(norm, out, stats=st).view(-1, 2).double()
    mean, invstd, var = cr.stats_ref(out, norm.eps)
    assert float((got[:, 0] - mean).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))
    assert float(((got[:, 1] - invstd) / invstd).abs().max()) <= cr.stats_tolerance(mean, var, out.shape[2] * out.shape[3])


@gpu
@torch.no_grad()
@pytest.mark.parametrize("c,passes", _each(NORMED))
def test_in_norm_launch(c, passes):
    from dkt_stereo_amd import conv, extractor

    def build():
        layer = make_layer(c, DEV)
        x, _ = _input(_shape(c), 23 + c.cout)
        params = extractor.instance_norm_params(torch.nn.InstanceNorm2d(x.shape[1]), x)
        xn = cr.norm_operand(x, params)
        return dict(layer=layer, x=x, params=params, xn=xn, exact=cr.conv_ref(xn, layer, 3))
    d = _data((c.group, c.name), build)
    layer, x, params, xn = d["layer"], d["x"], d["params"], d["xn"]
    B, cin = x.shape[:2]
    with conv.use_backend(BACKEND[passes]):
        assert conv.fused_eligible(layer, True) and conv.stats_eligible(layer)
        assert _tile(c, passes, layer=layer) == want_tile(c)
        ref = cr.conv_ref(xn, layer, passes)
        got = conv.conv2d_fused(x, layer, in_norm=params)
        _judge(c, "", passes, got, ref, d["exact"])
        # "bit-identical to the separate passes" (conv2d_fused): the plain launch on the separately normalised tensor
        if _same_order(_tile(c, passes, form=SINGLE, layer=layer), want_tile(c)):
            assert torch.equal(got, conv.conv2d(xn, layer))
        out, st = conv.conv2d_stats(x, layer, in_norm=params)
        assert torch.equal(out, got)
        _check_stats(c, out, st, ref)
        item = lambda b: params.view(B, cin, 2)[b].reshape(cin, 2).contiguous()  # noqa: E731

        def run(xx, b):
            if b is None:                               # the rolled batch: its parameters roll along
                return conv.conv2d_fused(xx, layer, in_norm=params.view(B, cin, 2).roll(1, 0).reshape(B * cin, 2).contiguous())
            return conv.conv2d_fused(xx, layer, in_norm=item(b))
        _placement(c, passes, layer, x, got, run, ref)
        one, _ = conv.conv2d_stats(x[:1], layer, in_norm=item(0))
        assert torch.equal(one, run(x[:1], 0))


# ---- the device-scaled form -------------------------------------------------------------------------------------------------
@gpu
@torch.no_grad()
@pytest.mark.parametrize("c,passes", _each(DSCALED))                            # (varies fastest: a case's pass counts stay together)
@pytest.mark.parametrize("magnitude", [1.0, 2.0 ** -18], ids=["unit", "tiny"])
def test_device_scaled_launch(c, passes, magnitude):
    from dkt_stereo_amd import conv

    def build():
        layer = make_layer(c, DEV)
        x, _ = _input(_shape(c), 29 + c.cout, magnitude)
        g, _, scale = conv.conv_grad_prepass(x, want_bias=False)
        assert g.data_ptr() == x.data_ptr()
        return dict(layer=layer, x=x, scale=scale, exact=cr.conv_ref(x, layer, 3, bias=False))
    d = _data((c.group, c.name, magnitude), build)
    layer, x, scale = d["layer"], d["x"], d["scale"]
    with conv.use_backend(BACKEND[passes]):
        assert _tile(c, passes, layer=layer) == want_tile(c)
        s = scale.tolist()
        assert s[0] * s[1] == 1.0 and s[0] > 0
        ref = cr.conv_ref(x, layer, passes, bias=False, act=cr.dscale_act(scale))
        got = conv.conv2d_dscale(x, layer, scale)
        _judge(c, "[%s]" % ("unit" if magnitude == 1.0 else "tiny"), passes, got, ref, d["exact"], floor=magnitude)
        _placement(c, passes, layer, x, got, lambda xx, b: conv.conv2d_dscale(xx, layer, scale), ref)


# ---- pair launches ----------------------------------------------------------------------------------------------------------
@gpu
@torch.no_grad()
@pytest.mark.parametrize("c,passes", _each(PAIRED))
def test_pair_launch(c, passes):
    from dkt_stereo_amd import conv

    def build():
        layer = make_layer(c, DEV)
        x, _ = _input(_shape(c), 31 + c.cout)
        other, oshape = make_partner(c, DEV)
        ox, _ = _input(oshape, 37 + c.cout)
        return dict(layer=layer, x=x, other=other, ox=ox, exact=cr.conv_ref(x, layer, 3), oexact=cr.conv_ref(ox, other, 3, relu=True))
    d = _data((c.group, c.name), build)
    layer, x, other, ox = d["layer"], d["x"], d["other"], d["ox"]
    with conv.use_backend(BACKEND[passes]):
        assert conv.pair_eligible(layer, other)
        first_tile = _tile(c, passes, layer=layer)
        assert first_tile == want_tile(c)
        alone_tile = _tile(c, passes, form=SINGLE, layer=layer)
        o_first_tile = layer_tile(ox.shape, other, form=PAIR, passes=passes)
        o_alone_tile = layer_tile(ox.shape, other, form=SINGLE, passes=passes)
        ref, oref = cr.conv_ref(x, layer, passes), cr.conv_ref(ox, other, passes, relu=True)
        first, o_second = conv.conv2d_pair((x, layer, False), (ox, other, True))          # both on first_tile
        o_first, second = conv.conv2d_pair((ox, other, True), (x, layer, False))          # both on o_first_tile
        _judge(c, "[first]", passes, first, ref, d["exact"])
        _judge(c, "[second]", passes, second, ref, d["exact"])
        _judge(c, "[partner first]", passes, o_first, oref, d["oexact"])
        _judge(c, "[partner second]", passes, o_second, oref, d["oexact"])
        checked = 0
        if not conv.few_eligible(layer):
            alone = conv.conv2d(x, layer)
            for got, t in ((first, first_tile), (second, o_first_tile)):
                if _same_order(t, alone_tile):
                    assert torch.equal(got, alone)
                    checked += 1
        if _same_order(first_tile, o_first_tile):
            assert torch.equal(first, second) and torch.equal(o_first, o_second)
            checked += 1
        o_alone = conv.conv2d(ox, other, relu=True)
        for got, t in ((o_first, o_first_tile), (o_second, first_tile)):
            if _same_order(t, o_alone_tile):
                assert torch.equal(got, o_alone)
                checked += 1
        assert checked >= 2                               # (every case keeps bit-for-bit comparisons)


# ---- residual join and output statistics ------------------------------------------------------------------------------------
@gpu
@torch.no_grad()
@pytest.mark.parametrize("c,passes", _each(EPILOGUES))
def test_residual_and_statistics_epilogues(c, passes):
    from dkt_stereo_amd import conv

    def build():
        layer = make_layer(c, DEV)
        x, g = _input(_shape(c), 41 + c.cout)
        res = torch.randn((c.B, c.cout, c.H, c.W), device=DEV, generator=g)
        return dict(layer=layer, x=x, res=res, exact=cr.conv_ref(x, layer, 3))
    d = _data((c.group, c.name), build)
    layer, x, res = d["layer"], d["x"], d["res"]
    with conv.use_backend(BACKEND[passes]):
        assert conv.fused_eligible(layer) and conv.stats_eligible(layer)
        assert _tile(c, passes, layer=layer) == want_tile(c)
        v = cr.conv_ref(x, layer, passes)
        if c.o.get("stats"):
            for relu in (False, True):
                ref = v.clamp_min(0) if relu else v
                out, st = conv.conv2d_stats(x, layer, relu=relu)
                _judge(c, "[relu %d]" % relu, passes, out, ref, d["exact"].clamp_min(0) if relu else d["exact"])
                assert torch.equal(out, conv.conv2d(x, layer, relu=relu))
                _check_stats(c, out, st, ref)
            _placement(c, passes, layer, x, out, lambda xx, b: conv.conv2d_stats(xx, layer, relu=True)[0], ref)
            return
        for relu in (False, True):
            ref = cr.residual_ref(v, res, relu)
            got = conv.conv2d_fused(x, layer, relu=relu, residual=res)
            _judge(c, "[relu %d]" % relu, passes, got, ref, cr.residual_ref(d["exact"], res, relu))

            def run(xx, b):
                r = res.roll(1, 0) if b is None else res[b:b + 1]
                return conv.conv2d_fused(xx, layer, relu=relu, residual=r)
            _placement(c, passes, layer, x, got, run, ref)


# ---- gate epilogues ---------------------------------------------------------------------------------------------------------
def _gate_data():
    def build():
        g = torch.Generator(device=DEV).manual_seed(51)
        rnd = lambda *s: torch.randn(s, device=DEV, generator=g)  # noqa: E731
        out = {}
        for key in "ab":
            zr_c = next(c for c in GATES if c.name == "gate_zr_" + key)
            q_c = next(c for c in GATES if c.name == "gate_q_" + key)
            cx, H, W = zr_c.srcs[1], zr_c.H, zr_c.W
            out[key] = dict(zr=make_layer(zr_c, DEV, seed=52), q=make_layer(q_c, DEV, seed=53), h=torch.tanh(rnd(1, 128, H, W)),
                            x=rnd(1, cx, H, W), cz=rnd(1, 128, H, W), cr=rnd(1, 128, H, W), cq=rnd(1, 128, H, W), zr_c=zr_c, q_c=q_c)
        return out
    return _data(("gates",), build)


def _gate_case(name):
    return next(c for c in GATES if c.name == name)


@gpu
@torch.no_grad()
@pytest.mark.parametrize("passes", P123)
def test_gate_zr_alone_and_in_a_pair(passes):
    from dkt_stereo_amd import conv
    G = _gate_data()
    pair_c = _gate_case("gate_zr_pair")
    with conv.use_backend(BACKEND[passes]):
        arg = lambda d: ([d["h"], d["x"]], d["zr"], d["cz"], d["cr"], d["h"])  # noqa: E731
        alone = {}
        for key, d in G.items():
            c = d["zr_c"]
            assert conv.hip_eligible(d["zr"])
            assert _tile(c, passes, layer=d["zr"]) == want_tile(c)
            z, rh = conv.conv2d_gate_zr(*arg(d))
            want = cr.gate_zr_ref(cr.conv_ref([d["h"], d["x"]], d["zr"], passes), d["cz"], d["cr"], d["h"])
            exact = cr.gate_zr_ref(cr.conv_ref([d["h"], d["x"]], d["zr"], 3), d["cz"], d["cr"], d["h"])
            _judge(c, "[z]", passes, z, want[0], exact[0], bound=cr.GATE_BOUND)
            _judge(c, "[rh]", passes, rh, want[1], exact[1], bound=cr.GATE_BOUND)
            alone[key] = (z, rh)
        a, b = G["a"], G["b"]
        assert conv.pair_eligible(a["zr"], b["zr"])
        assert _tile(pair_c, passes, layer=a["zr"]) == want_tile(pair_c) == want_tile(b["zr_c"])      # either order: one tile
        assert _tile(b["zr_c"], passes, form=PAIR, layer=b["zr"]) == want_tile(pair_c)
        (z1, rh1), (zb2, rhb2) = conv.conv2d_gate_zr_pair(arg(a), arg(b))
        (zb1, rhb1), (z2, rh2) = conv.conv2d_gate_zr_pair(arg(b), arg(a))
        for got in ((z1, rh1), (z2, rh2)):
            assert torch.equal(got[0], alone["a"][0]) and torch.equal(got[1], alone["a"][1])
        for got in ((zb1, rhb1), (zb2, rhb2)):
            assert torch.equal(got[0], alone["b"][0]) and torch.equal(got[1], alone["b"][1])


@gpu
@torch.no_grad()
@pytest.mark.parametrize("passes", P123)
def test_gate_q_alone_in_a_pair_and_in_place(passes):
    """The q gate is fed the z and r*h of the reference, so the launch is judged on its own."""
    from dkt_stereo_amd import conv
    G = _gate_data()
    pair_c = _gate_case("gate_q_pair")
    with conv.use_backend(BACKEND[passes]):
        outs = {}
        for key, d in G.items():
            c = d["q_c"]
            assert conv.hip_eligible(d["q"])
            assert _tile(c, passes, layer=d["q"]) == want_tile(c)
            z64, rh64 = cr.gate_zr_ref(cr.conv_ref([d["h"], d["x"]], d["zr"], passes), d["cz"], d["cr"], d["h"])
            z, rh = z64.float(), rh64.float()
            want = cr.gate_out_ref(cr.conv_ref([rh, d["x"]], d["q"], passes), d["cq"], z, d["h"])
            exact = cr.gate_out_ref(cr.conv_ref([rh, d["x"]], d["q"], 3), d["cq"], z, d["h"])
            got = conv.conv2d_gate_out([rh, d["x"]], d["q"], d["cq"], z, d["h"])
            _judge(c, "", passes, got, want, exact, bound=cr.GATE_BOUND)
            h2 = d["h"].clone()                          # the state updated in place: out aliases h
            same = conv.conv2d_gate_out([rh, d["x"]], d["q"], d["cq"], z, h2, out=h2)
            assert same.data_ptr() == h2.data_ptr() and torch.equal(h2, got)
            outs[key] = (z, rh, got)
        a, b = G["a"], G["b"]
        assert conv.pair_eligible(a["q"], b["q"])
        assert _tile(pair_c, passes, layer=a["q"]) == want_tile(pair_c) == want_tile(b["q_c"])
        assert _tile(b["q_c"], passes, form=PAIR, layer=b["q"]) == want_tile(pair_c)
        arg = lambda k, out: ([outs[k][1], G[k]["x"]], G[k]["q"], G[k]["cq"], outs[k][0], out if out is not None else G[k]["h"], out)  # noqa: E731
        first, o_second = conv.conv2d_gate_out_pair(arg("a", None), arg("b", None))
        ha, hb = a["h"].clone(), b["h"].clone()
        o_first, second = conv.conv2d_gate_out_pair(arg("b", hb), arg("a", ha))       # both in place
        assert torch.equal(first, outs["a"][2]) and torch.equal(second, outs["a"][2]) and second.data_ptr() == ha.data_ptr()
        assert torch.equal(o_first, outs["b"][2]) and torch.equal(o_second, outs["b"][2])
