// conv_tile.h -- the ONE place that decides which kernel and tile shape a dkt_conv2d_f16s_desc / _pair call runs on.  Plain C++ (no HIP,
// no kernel argument block): conv2d.hip asks conv_tile_select() before every launch and generates the launch of each shape
// from CONV_TILE_TABLE; dkt_conv2d_f16s_tile() gives the tests the same answer.  A tile shape is tuned here and nowhere else.
// Wave tile = 32*MF output channels x NF rows x 32 columns; WM x WN waves along (channels, rows); ST the stride; activations
// are staged in chunks of 16*CK channels.  Wide layers put all four waves on the channel axis (one block = up to 256
// channels: each patch is staged once); narrow layers put them on rows; images too small to give every CU a block with
// 4-row wave tiles use 2-row wave tiles.
#pragma once
#include <cstdlib>
#include "../../include/dktstereo.h"

#ifndef CONV_FEW_TILES
#define CONV_FEW_TILES 200   // fewer tiles than this: half-height tile shapes
#endif

// Every shape conv2d_f16s_kernel is instantiated for, per pass count.  K1: also for 1x1 filters (every row exists for 3x3);
// NRM: with the input's instance norm folded into the staging; DSC: with the device-resident scales; PAIR: may carry a second
// problem; P3: three passes only.  Stride-2 rows are 3x3 only: a 1x1 stride-2 layer runs a stride-1 row on a sub-sampled source.
//        WM WN NF MF ST CK   K1 NRM DSC PAIR P3
#define CONV_TILE_TABLE(X)                                                                               \
    X(1, 4, 1, 1, 1, 2,    1, 0, 1, 1, 0) /*  32 co x 4 rows */                                          \
    X(1, 4, 2, 2, 1, 1,    0, 1, 1, 1, 0) /*  64 co x 8 rows, 16-channel chunks */                       \
    X(1, 4, 1, 2, 1, 2,    1, 1, 1, 1, 0) /*  64 co x 4 rows */                                          \
    X(1, 4, 1, 3, 1, 2,    0, 1, 1, 0, 0) /*  96 co x 4 rows */                                          \
    X(2, 2, 1, 2, 1, 2,    1, 1, 1, 1, 0) /* 128 co x 2 rows */                                          \
    X(2, 2, 2, 2, 1, 2,    1, 1, 1, 1, 0) /* 128 co x 4 rows */                                          \
    X(4, 1, 2, 3, 1, 2,    0, 0, 1, 0, 0) /* 384 co x 2 rows */                                          \
    X(4, 1, 1, 2, 1, 2,    1, 0, 1, 1, 0) /* 256 co x 1 row */                                           \
    X(4, 2, 2, 2, 1, 2,    0, 0, 1, 1, 0) /* 256 co x 4 rows, 8 waves */                                 \
    X(4, 1, 2, 2, 1, 2,    1, 0, 1, 1, 0) /* 256 co x 2 rows */                                          \
    X(1, 4, 1, 3, 2, 1,    0, 0, 0, 0, 1) /* stride 2:  96 co x 4 rows, 16-channel chunks */             \
    X(2, 2, 2, 2, 2, 1,    0, 0, 0, 0, 1) /* stride 2: 128 co x 4 rows, 16-channel chunks */             \
    X(2, 2, 1, 2, 2, 2,    0, 0, 0, 0, 0) /* stride 2: 128 co x 2 rows */                                \
    X(4, 1, 1, 2, 2, 2,    0, 0, 0, 0, 0) /* stride 2: 256 co x 1 row */

enum { CONV_FORM_SINGLE = 0, CONV_FORM_PAIR = 1, CONV_FORM_NORM = 2, CONV_FORM_DSCALE = 3 };
enum { CONV_KERNEL_GENERIC = 0, CONV_KERNEL_WS = 1 };       // conv2d_f16s_kernel / conv_ws.h's weights-stationary kernel

// (what dkt_conv2d_f16s_tile reports, in this order; KS and ST as the kernel RUNS: a 1x1 stride-2 layer reports ST = 1)
struct ConvTile { int kernel, KS, WM, WN, NF, MF, ST, CK; };
// (H, W the INPUT size; form: one problem, the first of a pair launch, in-norm input, device-resident scales)
struct ConvTileQuery { int KS, stride, passes, Cout, nsrc; const int *src_channels; int epilogue, B, H, W, form; };

// What every form asks of a call's integers (conv_fill checks pointers, scales and the options of the descriptor).
static inline int conv_query_check(int stride, int epilogue, int nsrc, int B, int H, int W, int Cout, int KH, int KW, int passes) {
    if (stride != 1 && (stride != 2 || epilogue)) return DKT_E_UNSUPPORTED;
    if (nsrc < 1 || nsrc > DKT_CONV_MAX_SRC || B <= 0 || H <= 0 || W <= 0 || Cout <= 0 || B > 65535) return DKT_E_SHAPE;
    if (KH != KW || (KH != 1 && KH != 3)) return DKT_E_UNSUPPORTED;
    if (passes < 1 || passes > 3) return DKT_E_UNSUPPORTED;
    return DKT_OK;
}

// both problems of a pair launch run one kernel instantiation: they must fall in the same class of the ladder below
static inline int conv_width_class(int Cout) { return Cout <= 32 ? 0 : Cout <= 64 ? 1 : Cout <= 128 ? 2 : 3; }

// The kernel and tile shape of a call, or the error code the call returns.
static inline int conv_tile_select(const ConvTileQuery &q, ConvTile *t) {
    if (!q.src_channels) return DKT_E_NULL;
    const int rc = conv_query_check(q.stride, q.epilogue, q.nsrc, q.B, q.H, q.W, q.Cout, q.KS, q.KS, q.passes);
    if (rc != DKT_OK) return rc;
    if (q.form < CONV_FORM_SINGLE || q.form > CONV_FORM_DSCALE) return DKT_E_UNSUPPORTED;
    const bool pair = q.form == CONV_FORM_PAIR, norm = q.form == CONV_FORM_NORM, dsc = q.form == CONV_FORM_DSCALE;
    const int Cout = q.Cout;
    int KS = q.KS, ST = q.stride, H = q.H, W = q.W;
    if (ST == 2) {
        if (q.form != CONV_FORM_SINGLE) return DKT_E_UNSUPPORTED;
        H = (H - 1) / 2 + 1;           // the ladders count OUTPUT tiles
        W = (W - 1) / 2 + 1;
        // 1x1, stride 2 = the 1x1 stride-1 layer on the even pixels of the even rows: the tiled stride-2 form stages the
        // odd rows and columns it never uses -- three quarters of its requests
        if (KS == 1) ST = 1;
    }
    // the in-norm form: the second 3x3 layer of the feature encoder's residual blocks (core/extractor.py:46-50; 64, 96 and
    // 128 channels), one source, no gate epilogue -- the NRM rows of the table
    if (norm && (KS != 3 || q.nsrc != 1 || Cout <= 32 || Cout > 128 || q.epilogue == 1 || q.epilogue == 2)) return DKT_E_UNSUPPORTED;
    if (dsc && q.epilogue) return DKT_E_UNSUPPORTED;
    const long tiles_w = (W + 31) / 32, few = CONV_FEW_TILES;
    const long tiles4 = tiles_w * ((H + 3) / 4) * q.B;            // blocks if a block covers 4 rows
    const long rows2 = tiles_w * ((H + 1) / 2) * q.B;             // ... 2 rows
    const long nco = (Cout + 255) / 256;
    auto shape = [&](int WM, int WN, int NF, int MF, int CK, int kernel = CONV_KERNEL_GENERIC) {
        *t = ConvTile{kernel, KS, WM, WN, NF, MF, ST, CK};
        return (int)DKT_OK;
    };
    if (ST == 2) {
        // Stride-2 layers (the encoders' down-sampling convolutions, core/extractor.py:16,34,136-138): 2-row output tiles keep
        // the (2*TR+1) x 65 input patch at 52 KB per LDS stage.
        // 128 co x 4 rows with 16-channel chunks (9 x 65 patch, 56 KB per stage, one block per CU): twice the MFMAs per weight
        // fragment of the 2-row form -- 64->96 @736x1248 281 -> 243 us, two images 518 -> 422; 96->128 @368x624 x 2: 174 -> 138
        // (up to 96 channels: the 96-channel wave tile, as for stride 1 -- 243 -> 223 us, two images 422 -> 395)
        if (q.passes == 3 && Cout <= 128 && tiles4 >= 512) return Cout <= 96 ? shape(1, 4, 1, 3, 1) : shape(2, 2, 2, 2, 1);
        return Cout <= 128 ? shape(2, 2, 1, 2, 2) : shape(4, 1, 1, 2, 2);
    }
    // 64 -> 64, 3x3, three passes, one 64-channel source, epilogues 0 / 3, plain or in-norm input: images with at least 192
    // tiles of 8 x 32 pixels take the weights-stationary kernel -- measured 22 against 30 us at 230 tiles (184 x 312), equal
    // at 128, 35 against 45-48 at 512.  (Its buffer descriptors span 32 output planes with byte offsets in 32 bits.)
    if (KS == 3 && q.passes == 3 && !pair && !dsc && q.nsrc == 1 && q.src_channels[0] == 64 && Cout == 64 &&
        (q.epilogue == 0 || q.epilogue == 3) && q.B <= 64 && (long)H * W * 128 <= 0x7fffffffL &&
        tiles_w * ((H + 7) / 8) * q.B >= 192) {
        // DKT_CONV_WS=0 keeps the streaming kernel; read per call: the tests compare both kernels in one process
        const char *e = getenv("DKT_CONV_WS");
        if (!(e && e[0] == '0')) return shape(1, 4, 2, 2, 1, CONV_KERNEL_WS);
    }
    // 4-row blocks keep the LDS stage at 65 KB, i.e. two blocks per CU; the 8-row forms (one block per CU) measured 15-35 %
    // slower on every encoder layer.  Small images (the 1/8 and 1/16 GRUs: 115 and 69 tiles of the default shape for 256 CUs)
    // take half-height tiles so that twice as many CUs work.
    // the flow / disparity heads (2 and 1 output channels): a 32-channel wave tile halves the padded MFMA work
    if (Cout <= 32) return shape(1, 4, 1, 1, 2);
    // 64 co x 8 rows with 16-channel chunks (33 KB LDS stage: still two blocks per CU): twice the MFMAs per weight fragment of
    // the 4-row form (64->64 @368x624: 90 -> 78 us; not for images that give fewer 8-row tiles than resident blocks: @184x312
    // 29 -> 32 us), i.e. from one full wave of blocks on
    if (Cout <= 64) return KS == 3 && tiles4 / 2 >= 512 ? shape(1, 4, 2, 2, 1) : shape(1, 4, 1, 2, 2);
    if (Cout <= 128) {
        // 65 .. 96 channels: a 96-channel wave tile (three 32-channel blocks per wave, four waves on rows) instead of padding a
        // quarter of the 128-channel tile's MFMAs and weight fragments: 96->96 @368x624 205 -> 181 us, two images 357 -> 330
        if (KS == 3 && Cout <= 96 && !pair && tiles4 >= few) return shape(1, 4, 1, 3, 2);
        return tiles4 < few ? shape(2, 2, 1, 2, 2) : shape(2, 2, 2, 2, 2);
    }
    // 257 .. 384 channels (the context encoder's 128 -> 3 x 128 projection, raft_stereo.py:103-106) on large images: four
    // waves of 96 channels each and two rows -- the patch is staged once and no channel block is padding, where the 256-channel
    // tile runs a second, half-empty block: 253 -> 213 us @184x312 (slower below ~500 tiles: 65 -> 70 us @92x156)
    if (KS == 3 && Cout > 256 && Cout <= 384 && !pair && rows2 >= 512) return shape(4, 1, 2, 3, 2);
    if (rows2 * nco < few) return shape(4, 1, 1, 2, 2);
    // wide layers on large images: ONE block of 8 waves per CU, 256 co x 4 rows (WM x WN = 4 x 2): the two waves of a SIMD
    // share their weight fragments through L1 and the patch halo shrinks (6 rows staged per 4 instead of 4 per 2).  Measured
    // 384->256 @184x312: 326 -> 315 us; 128->256: 113 -> 109.
    if (KS == 3 && tiles4 * nco >= 256) return shape(4, 2, 2, 2, 2);
    // otherwise 256 co x 2 rows per block, two blocks per CU (384->256 @184x312: 324 us against 374 for one 4-row block per CU)
    return shape(4, 1, 2, 2, 2);
}
