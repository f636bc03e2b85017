// conv_wgrad_common.h -- the contract of the weight-gradient convolutions (conv_wgrad.hip: stride 1, conv_wgrad_s2.hip:
// stride 2), told once.  Each kernel file describes only how it stages its operands.
//   gw[co][ci][ky][kx] = sum_{b,oy,ox} g'[b,co,oy,ox] * x[b,ci,s*oy+ky-p,s*ox+kx-p]          K in {1, 3}, p = K/2, s in {1, 2}
//
// GEMM view   D[co][(ci, tap)] = sum_{pixel} G[co][pixel] * X[ci][pixel'(tap)]:  the reduction index is the pixel of g', the
// contiguous axis of both operands in NCHW, so neither is transposed on the way into LDS.  Its rows x cols -- H x W at
// stride 1, Ho x Wo at stride 2 -- is the REDUCTION GRID every rule below is stated on.  Both operands are split into fp16
// hi / lo while they are staged (g' * scale[0] from the pre-pass, x * x_scale: wgrad_split8); the products are
// g_hi*x_hi + g_lo*x_hi + g_hi*x_lo on v_mfma_f32_32x32x16_f16 with fp32 accumulation, as in conv2d.hip.
//
// Work item = (slice, 64 output channels, 64 input channels), a block walks items blockIdx.x, + gridDim.x, ...; a slice is
// (batch element, band of grid rows) and the item walks its band in pixel tiles of 2 rows x 32 columns.  The band height
// is a function of the shape alone (wgrad_plan).
//
// Split-K without float atomics: every item stores its partial tile to ws[slice][Cout][Cin][K][K]; the one finishing kernel
// (conv_wgrad.hip, launched through wgrad_finish) adds a weight's slices in ascending order and un-scales by
// scale[1] / x_scale (powers of two: wgrad_x_scale_ok).  Bit-identical from run to run, for every grid size, and for the
// 16-byte and the 4-byte load path alike (they stage the same values).  The workspace, B * bands weight images, grows with
// every size only at a fixed band height: a shape that crosses the plan's 256 work items gets shorter bands and more of them.
//
// Device code is shared here only where sharing leaves the instruction stream of every kernel unchanged:
// the stride-1 file keeps its own row load and both keep their own item decode and partial-tile store.
#pragma once
#include "dkt_common.h"
#include <cmath>

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

#define WG_TH 2               // grid rows of a pixel tile
#define WG_TW 32              // grid columns of a pixel tile
#define WG_CB 64              // channels of a block tile, on both sides
#define WG_GP 72              // fp16 per staged g' channel: 2 x 32 pixels + 8 pad (pitch 144 B = 16 * 9)
#define WG_T0 2048            // grid pixels per slice the plan starts from ...
#define WG_TMIN 512           // ... and does not go below
#define WG_ITEMS 256          // work items the plan asks for before it stops halving

// The by-value kernel argument, in two runs of fields: the stride-2 kernel has Ho, Wo between them, and a base struct that
// ends at W would be padded to 8 bytes and move every later kernarg offset.
#define WGRAD_ARGS_OPERANDS                                                                                                   \
    const float *x, *g, *scale;                                                                                               \
    float x_scale;                                                                                                            \
    float *ws;                                                                                                                \
    long x_bs, g_bs;                                                                                                          \
    int B, Cin, Cout, H, W;
#define WGRAD_ARGS_SLICES                                                                                                     \
    int rows_band, bands;     /* slice = b * bands + band; bands of grid rows */                                              \
    int n_co, n_ci, tiles_w;                                                                                                  \
    long items;               /* item = (slice * n_co + co block) * n_ci + ci block */

__device__ __forceinline__ void wgrad_split8(const float (&v)[8], float s, f16x8 &hi, f16x8 &lo) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float t = __fmul_rn(v[j], s);
        const _Float16 h = (_Float16)t;
        hi[j] = h;
        lo[j] = (_Float16)__fsub_rn(t, (float)h);
    }
}

struct WgradPlan {
    int rows_band, bands, n_co, n_ci;
};

// The slice rule on the reduction grid: bands of (T / cols rounded down to whole pixel tiles, at least one) rows, T = 2048
// pixels halved down to 512 while the problem has fewer than 256 work items.  A function of the shape alone.
static inline WgradPlan wgrad_plan(int B, int Cin, int Cout, int rows, int cols) {
    WgradPlan p;
    p.n_co = (Cout + WG_CB - 1) / WG_CB;
    p.n_ci = (Cin + WG_CB - 1) / WG_CB;
    for (long T = WG_T0;; T >>= 1) {
        const long r = (T / cols) & ~(long)(WG_TH - 1);
        p.rows_band = (int)(r < WG_TH ? WG_TH : r);
        p.bands = (rows + p.rows_band - 1) / p.rows_band;
        if ((long)p.n_co * p.n_ci * B * p.bands >= WG_ITEMS || T <= WG_TMIN) break;
    }
    return p;
}

static inline bool wgrad_shape_ok(int B, int Cin, int Cout, int H, int W, int K) {
    return B > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0 && (K == 1 || K == 3);
}

// a positive power of two whose reciprocal is finite
static inline bool wgrad_x_scale_ok(float x_scale) {
    int e = 0;
    return x_scale > 0.0f && std::isfinite(x_scale) && std::frexp(x_scale, &e) == 0.5f && std::isfinite(1.0f / x_scale);
}

// floats of ws[slice][Cout][Cin][K][K] (the *_ws_floats entries)
static inline long wgrad_ws_floats(int B, int Cin, int Cout, int rows, int cols, int K) {
    return (long)B * wgrad_plan(B, Cin, Cout, rows, cols).bands * Cout * Cin * K * K;
}

// every field but the stride-2 kernel's Ho, Wo; cols = columns of the reduction grid
template <class Args>
static inline void wgrad_fill_args(Args &a, const float *x, long x_bstride, const float *g, long g_bstride,
                                   const float *scale, float x_scale, float *ws, int B, int Cin, int Cout, int H, int W,
                                   const WgradPlan &p, int cols) {
    a.x = x; a.g = g; a.scale = scale; a.x_scale = x_scale; a.ws = ws;
    a.x_bs = x_bstride; a.g_bs = g_bstride;
    a.B = B; a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W;
    a.rows_band = p.rows_band; a.bands = p.bands; a.n_co = p.n_co; a.n_ci = p.n_ci;
    a.tiles_w = (cols + WG_TW - 1) / WG_TW;
    a.items = (long)B * p.bands * p.n_co * p.n_ci;
}

// blocks of the main launch: one per CU (either kernel's LDS fills a CU), at most one per item
static inline unsigned wgrad_blocks(long items, int device) {
    int dev = device, cus = 0;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    return (unsigned)(items < cus ? items : cus);
}

// conv_wgrad_finish_kernel on `st` (conv_wgrad.hip): gw[e] = (sum over the nslices images of ws, ascending) * scale[1] /
// x_scale for the E weights; returns the launch status
__attribute__((visibility("hidden"))) int wgrad_finish(const float *ws, const float *scale, float x_scale, float *gw, long E,
                                                       int nslices, hipStream_t st);
