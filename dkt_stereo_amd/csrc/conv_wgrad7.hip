// conv_wgrad7.hip -- the weight gradient of a 7x7, stride-1, padding-3 convolution with 1..4 input channels: the stem layers
// (dkt_stereo_amd/conv.py: _Conv2dGradFn.backward with GRAD_WEIGHT7_HIP).
// Reference: torch autograd through [relu](conv2d(x, w, b)) of core/extractor.py:140, :217 (conv1, 3 -> 64), core/update.py:73
// (convf1, 2 -> 64) and meta_arch/igev_stereo/update.py:80 (convd1, 1 -> 64), under training.
// The contract -- hi / lo split, three products, slice plan (wgrad_plan on the H x W grid, n_ci = 1), split-K workspace and
// the finishing kernel -- is in conv_wgrad_common.h.  This file is the staging scheme of a problem whose output is tiny
// (Cout x Cin*49 weights) and whose reduction streams g' once.
//
// GEMM view   D[co][n] = sum_{pixel} G[co][pixel] * X[n][pixel + tap(n)],  n = (ci * 7 + kx) * 7 + ky  < Cin * 49,
// padded to NF = ceil(Cin * 49 / 32) fragments of 32 columns (2, 4, 5, 7 for Cin = 1..4; the columns past Cin * 49 read a
// valid address and are never stored).
//
// Block = 8 waves on one CU, as in conv_wgrad.hip: waves 4..7 stage, waves 0..3 multiply.  Multiplying wave (wco, wn) owns
// the output channels 32 wco .. of the item's 64 and the column fragments wn * NFW .., NFW = ceil(NF / 2): at most 4
// accumulators (64 registers), no scratch.  An item = (slice, 64 output channels) walks its band in pixel tiles of 2 rows x
// 32 columns through two LDS buffers:
//   sg[buffer][hi|lo][co 64][2 x 32 pixels]                       pitch 144 B = 16 * 9
//   sx[buffer][hi|lo][ci * 7 + kx][2 + 6 rows][32 columns | 8]    row pitch 80 B = 16 * 5, image pitch 816 B = 16 * 51
// sx holds SEVEN column-shifted images of the patch, image kx at column c = x[.., tw0 + c + kx - 3], so the B fragment of
// every tap is one aligned ds_read_b128 with no register shifts: lane (column n, half h) reads the 8 pixels 8h.. of a k-step
// (16 pixels of one row) at image n / 7, patch row (tile row + ky).  With ky fastest in n, the 16 lanes the LDS serves
// together differ by 5 ky + 51 (n / 7) sixteen-byte slots: distinct mod 16 but for one 2-way pair in a channel count's last
// fragment (enumerated over the four lane groups of ds_read_b128 for Cin = 1..4).
// A staging thread owns 8 columns of one (channel, patch row): it loads the 16 floats around them (four float4, or one
// by one), splits them once and writes the seven shifted copies, 14 ds_write_b128.
// Zero-fill: g' beyond W, beyond the band's last row and beyond Cout; x outside the image.
#include "conv_wgrad_common.h"

#define W7_K 7
#define W7_XR (WG_TH + W7_K - 1)   // patch rows
#define W7_ROW 40                  // fp16 per staged row of a shifted image: 32 + 8 pad
#define W7_IMG 408                 // fp16 per shifted image: 8 rows of 40 + 88 pad (816 B = 16 * 51)
#define W7_MAXCIN 4

struct Wgrad7Args {
    WGRAD_ARGS_OPERANDS
    WGRAD_ARGS_SLICES
};

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The staging waves' loop body is ONE basic block: every load is unconditional (an element outside reads the batch element's
// first floats, always there, and is zeroed when the tile is converted, not when it is loaded), every thread stores, and an
// odd tile count is rounded up by a tile nobody multiplies.  With a branch between the loads of tile t + 1 and the conversion
// of tile t the compiler waits for ALL outstanding loads (s_waitcnt vmcnt(0)) and the prefetch hides nothing; so it waits for
// tile t's alone.
// N consecutive floats from base[off] on, element j fetched where keep(j); V = 4: whole aligned float4s (off % 4 == 0, and
// W % 4 == 0 puts a float4 inside or outside), V = 1: one by one.
template <int V, int N, class Keep>
__device__ __forceinline__ void wgrad7_fetch(const float *base, long off, Keep keep, float (&v)[N]) {
    if (V == 4) {
#pragma unroll
        for (int q = 0; q < N / 4; ++q) {
            const f32x4 t = *(const f32x4 *)(base + (keep(4 * q) ? off + 4 * q : 0L));
#pragma unroll
            for (int e = 0; e < 4; ++e) v[4 * q + e] = t[e];
        }
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = base[keep(j) ? off + j : 0L];
    }
}

template <int V, int N, class Keep>
__device__ __forceinline__ void wgrad7_zero_outside(Keep keep, const float (&v)[N], float (&z)[N]) {
#pragma unroll
    for (int j = 0; j < N; ++j) z[j] = keep(V == 4 ? j & ~3 : j) ? v[j] : 0.0f;
}

template <int CIN, int V>
__global__ __launch_bounds__(512, 1) void conv_wgrad7_kernel(Wgrad7Args a) {
    constexpr int TAPS = W7_K * W7_K, COLS = CIN * TAPS;
    constexpr int NF = (COLS + 31) / 32, NFW = (NF + 1) / 2;   // column fragments, and those of one multiplying wave
    constexpr int GU = WG_CB * WG_TH * 4 / 256;                // 8-pixel units of g' per loader thread
    constexpr int SGN = WG_CB * WG_GP, SXN = W7_K * CIN * W7_IMG;        // fp16 per plane
    __shared__ __attribute__((aligned(16))) _Float16 sg[2][2][SGN];      // [buffer][hi | lo]
    __shared__ __attribute__((aligned(16))) _Float16 sx[2][2][SXN];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool loader = wave >= 4;                             // waves 4..7 stage, waves 0..3 multiply: one of each per SIMD
    const int lt = tid & 255;                                  // thread index inside its role
    const int wco = wave & 1, wn = (wave >> 1) & 1;
    const int r = lane & 31, h = lane >> 5;
    const long HW = (long)a.H * a.W;
    const long E = (long)a.Cout * COLS;
    const float gs = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a.scale[0])));
    const float xs = a.x_scale;

    for (long item = blockIdx.x; item < a.items; item += gridDim.x) {
        const int cob = (int)(item % a.n_co);
        const int slice = (int)(item / a.n_co);
        const int band = slice % a.bands, b = slice / a.bands;
        const int r0 = band * a.rows_band;
        const int r1 = min(a.H, r0 + a.rows_band);
        const int ntiles = ((r1 - r0 + WG_TH - 1) / WG_TH) * a.tiles_w;
        // Both roles pass one barrier per tile of an EVEN count: tile t lives in buffer t & 1 and every item starts at buffer 0.
        // Buffer t & 1 was last read for tile t - 2 (of the item before, for t < 2), which the multiplying waves finished
        // before the barrier of tile t - 1.
        const int ntp = ntiles + (ntiles & 1);
        if (loader) {
            // ---- the staging waves: the loads of tile t + 1 are issued before tile t is converted and written
            const float *gb = a.g + (long)b * a.g_bs;
            const float *xb = a.x + (long)b * a.x_bs;
            // x: one thread per (channel, patch row, 8-column group); the threads past Cin * 32 stage channel Cin - 1 again
            const int xgrp = lt & 3, xpr = (lt >> 2) & (W7_XR - 1), xch = min(lt >> 5, CIN - 1);
            // where unit i of g' / the x unit of a tile lies: row usable, first column, offset in the batch element
            auto gpos = [&](int tile, int i, bool &ok, int &c0, long &off) {
                const int u = lt + 256 * i;
                const int grp = u & 3, row = (u >> 2) & (WG_TH - 1), ch = u >> 3;
                const int co = cob * WG_CB + ch, ih = r0 + (tile / a.tiles_w) * WG_TH + row;
                ok = co < a.Cout && ih < r1;
                c0 = (tile % a.tiles_w) * WG_TW + grp * 8;
                off = (long)co * HW + (long)ih * a.W + c0;
            };
            // 16 floats from column tw0 + 8 grp - 4 on, of which 1 .. 14 are used
            auto xpos = [&](int tile, bool &ok, int &c0, long &off) {
                const int ih = r0 + (tile / a.tiles_w) * WG_TH - W7_K / 2 + xpr;
                ok = ih >= 0 && ih < a.H;
                c0 = (tile % a.tiles_w) * WG_TW + xgrp * 8 - 4;
                off = (long)xch * HW + (long)ih * a.W + c0;
            };
            float gv[2][GU][8], xv[2][16];
            auto load = [&](int tile, float (&g8)[GU][8], float (&x16)[16]) {
                bool ok;
                int c0;
                long off;
#pragma unroll
                for (int i = 0; i < GU; ++i) {
                    gpos(tile, i, ok, c0, off);
                    wgrad7_fetch<V>(gb, off, [&](int j) { return ok && c0 + j < a.W; }, g8[i]);
                }
                xpos(tile, ok, c0, off);
                wgrad7_fetch<V>(xb, off, [&](int j) { return ok && c0 + j >= 0 && c0 + j < a.W; }, x16);
            };
            auto store = [&](int buf, int tile, const float (&g8)[GU][8], const float (&x16)[16]) {
                bool ok;
                int c0;
                long off;
#pragma unroll
                for (int i = 0; i < GU; ++i) {
                    const int u = lt + 256 * i;
                    const int grp = u & 3, row = (u >> 2) & (WG_TH - 1), ch = u >> 3;
                    float z[8];
                    gpos(tile, i, ok, c0, off);
                    wgrad7_zero_outside<V>([&](int j) { return ok && c0 + j < a.W; }, g8[i], z);
                    f16x8 hi, lo;
                    wgrad_split8(z, gs, hi, lo);
                    const int o = ch * WG_GP + row * WG_TW + grp * 8;
                    *(f16x8 *)&sg[buf][0][o] = hi;
                    *(f16x8 *)&sg[buf][1][o] = lo;
                }
                float z[16], v0[8], v1[8];
                // (elements 0 and 15 are loaded and never used: kept alive up to here, or their registers serve as temporaries
                // while the load is in flight and every such write waits for it)
                asm volatile("" ::"v"(x16[0]), "v"(x16[15]));
                xpos(tile, ok, c0, off);
                wgrad7_zero_outside<V>([&](int j) { return ok && c0 + j >= 0 && c0 + j < a.W; }, x16, z);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    v0[j] = z[j];
                    v1[j] = z[8 + j];
                }
                f16x8 h0, l0, h1, l1;
                wgrad_split8(v0, xs, h0, l0);
                wgrad_split8(v1, xs, h1, l1);
                _Float16 *dst = &sx[buf][0][xch * W7_K * W7_IMG + xpr * W7_ROW + xgrp * 8];
#pragma unroll
                for (int kx = 0; kx < W7_K; ++kx) {
                    // image kx, column 8 grp + m = x column tw0 + 8 grp + m + kx - 3 = element m + kx + 1 of the 16
                    f16x8 hi, lo;
#pragma unroll
                    for (int m = 0; m < 8; ++m) {
                        const int j = m + kx + 1;
                        hi[m] = j < 8 ? h0[j & 7] : h1[j & 7];
                        lo[m] = j < 8 ? l0[j & 7] : l1[j & 7];
                    }
                    *(f16x8 *)(dst + kx * W7_IMG) = hi;
                    *(f16x8 *)(dst + SXN + kx * W7_IMG) = lo;
                }
            };
            // (a tile index past the last stands for the last again: loads the cache serves, a buffer nobody reads)
            const int last = ntiles - 1;
            // (the scheduling barriers keep the conversion of a tile from being moved above the loads of the next, where its
            // wait for the tile's own loads would delay their issue)
            load(0, gv[0], xv[0]);
            for (int t = 0; t < ntp; t += 2) {
                load(min(t + 1, last), gv[1], xv[1]);
                __builtin_amdgcn_sched_barrier(0);
                store(0, t, gv[0], xv[0]);
                __syncthreads();                               // tile t is staged
                load(min(t + 2, last), gv[0], xv[0]);
                __builtin_amdgcn_sched_barrier(0);
                store(1, min(t + 1, last), gv[1], xv[1]);
                __syncthreads();                               // tile t + 1 is staged
            }
        } else {
            // column n of fragment j: image n / 7 = ci * 7 + kx, first patch row ky = n % 7; weight ci * 49 + ky * 7 + kx
            int boff[NFW], widx[NFW];
#pragma unroll
            for (int j = 0; j < NFW; ++j) {
                const int n = (wn * NFW + j) * 32 + r;
                const int nc = min(n, COLS - 1);
                const int ky = nc % W7_K, img = nc / W7_K;
                boff[j] = img * W7_IMG + ky * W7_ROW + 8 * h;
                widx[j] = n < COLS ? (img / W7_K) * TAPS + ky * W7_K + img % W7_K : -1;
            }
            f32x16 acc[NFW];
#pragma unroll
            for (int j = 0; j < NFW; ++j)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[j][i] = 0.0f;
            for (int tile = 0; tile < ntp; ++tile) {
                const int buf = tile & 1;
                const _Float16 *pg = &sg[buf][0][(wco * 32 + r) * WG_GP + 8 * h];
                const _Float16 *px = &sx[buf][0][0];
                __syncthreads();                               // tile `tile` is staged
                if (tile < ntiles) {
                    // ---- 4 k-steps of 16 pixels: (row, 16-column half)
#pragma unroll
                    for (int st = 0; st < WG_TH * 2; ++st) {
                        const int row = st >> 1, cb = (st & 1) * 16;
                        const f16x8 ahi = *(const f16x8 *)(pg + row * WG_TW + cb);
                        const f16x8 alo = *(const f16x8 *)(pg + SGN + row * WG_TW + cb);
#pragma unroll
                        for (int j = 0; j < NFW; ++j) {
                            // (for odd NF the second group's last fragment is all padding: multiplied like the rest, on a
                            // SIMD of its own, so that the k-steps stay one basic block; never stored)
                            const _Float16 *q = px + boff[j] + row * W7_ROW + cb;
                            const f16x8 bhi = *(const f16x8 *)q;
                            const f16x8 blo = *(const f16x8 *)(q + SXN);
                            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, bhi, acc[j], 0, 0, 0);
                            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, bhi, acc[j], 0, 0, 0);
                            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, blo, acc[j], 0, 0, 0);
                        }
                    }
                }
            }
            // ---- the partial tile: D[row = co][col = n], col = lane & 31, row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5)
            float *wp = a.ws + (long)slice * E;
#pragma unroll
            for (int j = 0; j < NFW; ++j) {
                if (widx[j] >= 0) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int co = cob * WG_CB + wco * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                        if (co < a.Cout) wp[(long)co * COLS + widx[j]] = acc[j][i];
                    }
                }
            }
        }
    }
}

static inline bool wgrad7_shape_ok(int B, int Cin, int Cout, int H, int W) {
    return B > 0 && Cin > 0 && Cin <= W7_MAXCIN && Cout > 0 && H > 0 && W > 0;
}

template <int CIN>
static void wgrad7_launch(const Wgrad7Args &a, bool vec, unsigned blocks, hipStream_t st) {
    if (vec) hipLaunchKernelGGL((conv_wgrad7_kernel<CIN, 4>), dim3(blocks), dim3(512), 0, st, a);
    else hipLaunchKernelGGL((conv_wgrad7_kernel<CIN, 1>), dim3(blocks), dim3(512), 0, st, a);
}

extern "C" long dkt_conv2d_wgrad7_ws_floats(int B, int Cin, int Cout, int H, int W) {
    if (!wgrad7_shape_ok(B, Cin, Cout, H, W)) return DKT_E_SHAPE;
    return wgrad_ws_floats(B, Cin, Cout, H, W, W7_K);
}

extern "C" int dkt_conv2d_wgrad7(const float *x, long x_bstride, const float *g, long g_bstride, const float *scale,
                                 float x_scale, float *gw, float *ws, int B, int Cin, int Cout, int H, int W, int device,
                                 void *stream) {
    if (!x || !g || !scale || !gw || !ws) return DKT_E_NULL;
    if (!wgrad7_shape_ok(B, Cin, Cout, H, W)) return DKT_E_SHAPE;
    const long HW = (long)H * W;
    if (x_bstride < (long)Cin * HW || g_bstride < (long)Cout * HW) return DKT_E_SHAPE;
    if (!wgrad_x_scale_ok(x_scale)) return DKT_E_SHAPE;
    DKT_ENTER(device);
    const WgradPlan p = wgrad_plan(B, Cin, Cout, H, W);        // n_ci = 1: an item is (slice, 64 output channels)
    Wgrad7Args a;
    wgrad_fill_args(a, x, x_bstride, g, g_bstride, scale, x_scale, ws, B, Cin, Cout, H, W, p, W);
    const bool vec = (W % 4 == 0) && (x_bstride % 4 == 0) && (g_bstride % 4 == 0) &&
                     ((uintptr_t)x % 16 == 0) && ((uintptr_t)g % 16 == 0);
    const unsigned blocks = wgrad_blocks(a.items, device);     // one block of 8 waves per CU
    hipStream_t st = (hipStream_t)stream;
    switch (Cin) {
    case 1: wgrad7_launch<1>(a, vec, blocks, st); break;
    case 2: wgrad7_launch<2>(a, vec, blocks, st); break;
    case 3: wgrad7_launch<3>(a, vec, blocks, st); break;
    default: wgrad7_launch<4>(a, vec, blocks, st); break;
    }
    const int rc = dkt_launch_status();
    if (rc != DKT_OK) return rc;
    return wgrad_finish(ws, scale, x_scale, gw, (long)Cout * Cin * W7_K * W7_K, B * p.bands, st);
}
