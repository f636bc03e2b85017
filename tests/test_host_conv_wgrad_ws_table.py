"""The workspace sizes of both weight-gradient convolutions against recorded numbers (no device needed): the two entries share
one slice plan (csrc/conv_wgrad_common.h) and both references share one restatement of it (_conv_wgrad_ref.grid_plan), so a
mistake common to the plan and its restatement shows only here.  The table holds what dkt_conv2d_wgrad_ws_floats and
dkt_conv2d_wgrad_s2_ws_floats returned when each file still had a plan of its own (commit cb1f252).

Every fixed case of the two references has fewer than 256 work items at every slice size, so their rows see the plan's lower
limit (512 pixels) but neither where it starts (2048) nor where it stops halving (256 items); the training-recipe shapes
below them do, on both grids, and a plan that took rows for columns would change their rows.  Those rows pin SIZES only.  The
arithmetic at a plan that stops at 2048 or 1024 pixels, or has more items than blocks, is held on the device by
test_gpu_conv_grad_plans.py on PLAN_CASES of the two references (test_host_conv_grad_plans.py asserts their regimes); their
rows, recorded from the library before those tests existed (commit 7d30439), close the table."""
import _conv_s2_ref as S
import _conv_wgrad_ref as WR

#: (B, H, W, k, Cin, Cout): (dkt_conv2d_wgrad_ws_floats, dkt_conv2d_wgrad_s2_ws_floats) at cb1f252
TABLE = {
    (1, 1, 1, 1, 1, 1): (1, 1),
    (2, 24, 40, 3, 48, 40): (69120, 34560),
    (1, 33, 37, 1, 36, 64): (6912, 2304),
    (1, 20, 28, 3, 64, 2): (2304, 1152),
    (1, 16, 24, 3, 384, 256): (884736, 884736),
    (2, 9, 35, 3, 33, 5): (2970, 2970),
    (1, 5, 70, 3, 8, 40): (2880, 2880),
    (3, 7, 9, 1, 130, 3): (1170, 1170),
    (1, 1, 1, 3, 1, 1): (9, 9),
    (1, 2, 3, 3, 3, 2): (54, 54),
    (2, 24, 40, 3, 64, 96): (221184, 110592),
    (1, 33, 37, 3, 36, 40): (38880, 12960),
    (1, 18, 70, 3, 8, 40): (8640, 2880),
    (1, 34, 130, 3, 5, 70): (53550, 9450),
    (1, 33, 37, 1, 96, 128): (36864, 12288),
    (1, 16, 24, 3, 128, 128): (147456, 147456),
    # the update operator's and the encoders' layers at the training recipe's sizes
    (2, 120, 224, 3, 384, 256): (26542080, 14155776),
    (2, 60, 112, 3, 384, 128): (13271040, 3538944),
    (2, 30, 56, 1, 36, 64): (18432, 4608),
    (2, 320, 720, 3, 64, 96): (17694720, 8847360),
    (2, 160, 360, 1, 96, 128): (983040, 983040),
    (2, 80, 180, 3, 128, 128): (11796480, 2949120),
    (2, 240, 448, 3, 384, 256): (106168320, 26542080),
    # PLAN_CASES of _conv_wgrad_ref.py, then of _conv_s2_ref.py (at 7d30439)
    (2, 42, 256, 3, 260, 257): (7216560, 7216560),
    (3, 88, 256, 1, 200, 250): (1650000, 900000),
    (3, 146, 24, 3, 257, 257): (7133292, 3566646),
    (2, 64, 255, 3, 130, 70): (5241600, 1310400),
    (1, 6, 8, 3, 384, 320): (1105920, 1105920),
    (2, 83, 512, 3, 260, 257): (25257960, 7216560),
    (3, 79, 512, 1, 70, 520): (2184000, 546000),
    (3, 291, 48, 3, 257, 257): (12483261, 7133292),
    (2, 127, 511, 3, 130, 70): (5241600, 5241600),
    (1, 12, 16, 3, 384, 320): (1105920, 1105920),
}


def test_the_table_covers_both_references_cases():
    assert set(WR.CASES) | set(S.CASES) | set(WR.PLAN_CASES) | set(S.PLAN_CASES) <= set(TABLE)


def test_workspace_sizes_are_the_recorded_ones():
    from dkt_stereo_amd import _ffi
    lib = _ffi.lib()
    for (B, H, W, k, cin, cout), want in TABLE.items():
        got = (lib.dkt_conv2d_wgrad_ws_floats(B, cin, cout, H, W, k), lib.dkt_conv2d_wgrad_s2_ws_floats(B, cin, cout, H, W, k))
        assert got == want, (B, H, W, k, cin, cout)
