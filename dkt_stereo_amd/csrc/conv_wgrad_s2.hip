// conv_wgrad_s2.hip -- the weight gradient of a stride-2, padding K/2 convolution, K in {1, 3} (dkt_stereo_amd/conv.py:
// _Conv2dGradFn.backward for the encoders' down-sampling layers).
// Reference: torch autograd through conv2d(x, w, b, stride=2) (core/extractor.py:6-60, :122-175 under training).
// The contract -- GEMM view, hi / lo split, slice plan, split-K workspace and its finishing kernel -- is in
// conv_wgrad_common.h; the reduction grid is the Ho x Wo of g'.  This file is the stride-2 staging scheme.
//
// Stride 2 breaks the unit pixel stride the stride-1 kernel's aligned reads rest on, so x is DE-INTERLEAVED while it is
// staged: a row of x becomes an even plane E[c] = x[2c] and an odd plane O[c] = x[2c + 1], and for 8 consecutive ox
//   kx = 1 reads E at ox        kx = 2 reads O at ox        kx = 0 reads O at ox - 1
// -- the first two are aligned ds_read_b128, the third is the aligned block to the left plus four v_alignbit_b32, as in
// conv_wgrad.hip; its halo (x[2 tw0 - 1]) is one fp16 in the last slot of the 8-column pad between the planes.  Rows need
// no planes: a tile of 2 output rows stages the 5 input rows 2 oy0 - 1 .. 2 oy0 + 3 and (row, ky) picks row 2 row + ky.
//   sg[hi|lo][co 64][2 x 32 pixels]                  pitch 144 B = 16 * 9
//   sx[hi|lo][ci 64][5 rows][E 32 | 8 pad | O 32]    pitch 720 B = 16 * 45 (K = 1: 2 rows + 8, 304 B = 16 * 19)
// 108 KiB: one block of 4 waves per CU, 2 x 2 fragments of 32 x 32 with all K*K taps in accumulators (144 registers; the
// block has the CU's registers to itself, so nothing spills).  Every wave stages and multiplies: the global loads of tile
// t + 1 are issued before the MFMAs of tile t and consumed after them.
// Zero-fill: g' beyond Wo, beyond the band's last row and beyond Cout; x outside the image and beyond Cin.
#include "conv_wgrad_common.h"

#define W2_XROW 72            // fp16 per staged x row: E 32 | 8 pad | O 32

struct WgradS2Args {
    WGRAD_ARGS_OPERANDS
    int Ho, Wo;
    WGRAD_ARGS_SLICES
};

// (conv_wgrad.hip keeps a load of its own: with this template its instruction stream changes)
// N consecutive floats of a row from column iw on; zero from column W on (V = 4: W % 4 == 0, a float4 is inside or outside)
template <int V, int N>
__device__ __forceinline__ void w2_load(const float *row, int iw, int W, bool ok, float (&v)[N]) {
    if (V == 4) {
#pragma unroll
        for (int q = 0; q < N / 4; ++q) {
            const float4 t = ok && iw + 4 * q < W ? *(const float4 *)(row + iw + 4 * q) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = ok && iw + j < W ? row[iw + j] : 0.0f;
    }
}

template <int KS, int V>
__global__ __launch_bounds__(256, 1) void conv_wgrad_s2_kernel(WgradS2Args a) {
    constexpr int TAPS = KS * KS;
    constexpr int XR = KS == 3 ? 2 * WG_TH + 1 : WG_TH;         // staged x rows
    constexpr int XP = XR * W2_XROW + (KS == 3 ? 0 : 8);        // fp16 per staged x channel: 16 * odd bytes
    constexpr int GU = WG_CB * WG_TH * 4 / 256;                 // 8-pixel units of g' per thread
    constexpr int XU = WG_CB * XR * 4 / 256;                    // 16-column units of x per thread
    constexpr int HN = WG_CB * XR;                              // halo elements (K = 3)
    constexpr int HU = (HN + 255) / 256;
    constexpr int SGN = WG_CB * WG_GP, SXN = WG_CB * XP;        // fp16 per plane
    __shared__ __attribute__((aligned(16))) _Float16 sg[2][SGN];           // [hi | lo]
    __shared__ __attribute__((aligned(16))) _Float16 sx[2][SXN];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wco = wave & 1, wci = wave >> 1;
    const int r = lane & 31, h = lane >> 5;
    const long HW = (long)a.H * a.W, HoWo = (long)a.Ho * a.Wo;
    const long E = (long)a.Cout * a.Cin * TAPS;
    const float gs = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a.scale[0])));
    const float xs = a.x_scale;

    for (long item = blockIdx.x; item < a.items; item += gridDim.x) {
        const int cib = (int)(item % a.n_ci);
        const long t1 = item / a.n_ci;
        const int cob = (int)(t1 % a.n_co);
        const int slice = (int)(t1 / a.n_co);
        const int band = slice % a.bands, b = slice / a.bands;
        const int r0 = band * a.rows_band;
        const int r1 = min(a.Ho, r0 + a.rows_band);
        const int ntiles = ((r1 - r0 + WG_TH - 1) / WG_TH) * a.tiles_w;
        const float *gb = a.g + (long)b * a.g_bs;
        const float *xb = a.x + (long)b * a.x_bs;
        float gv[GU][8], xv[XU][16], hv[HU];

        auto load = [&](int tile) {
            const int th0 = r0 + (tile / a.tiles_w) * WG_TH;
            const int tw0 = (tile % a.tiles_w) * WG_TW;
#pragma unroll
            for (int i = 0; i < GU; ++i) {
                const int u = tid + 256 * i;
                const int grp = u & 3, row = (u >> 2) & (WG_TH - 1), ch = u >> 3;
                const int co = cob * WG_CB + ch, oy = th0 + row;
                const bool ok = co < a.Cout && oy < r1;
                w2_load<V, 8>(gb + (ok ? (long)co * HoWo + (long)oy * a.Wo : 0L), tw0 + grp * 8, a.Wo, ok, gv[i]);
            }
#pragma unroll
            for (int i = 0; i < XU; ++i) {
                const int u = tid + 256 * i;
                const int grp = u & 3, xr = (u >> 2) % XR, ch = (u >> 2) / XR;
                const int ci = cib * WG_CB + ch, ih = KS == 3 ? 2 * th0 - 1 + xr : 2 * (th0 + xr);
                const bool ok = ci < a.Cin && ih >= 0 && ih < a.H;
                w2_load<V, 16>(xb + (ok ? (long)ci * HW + (long)ih * a.W : 0L), 2 * tw0 + grp * 16, a.W, ok, xv[i]);
            }
            if constexpr (KS == 3) {
#pragma unroll
                for (int i = 0; i < HU; ++i) {
                    const int u = tid + 256 * i;
                    const int xr = u % XR, ch = u / XR;
                    const int ci = cib * WG_CB + ch, ih = 2 * th0 - 1 + xr, iw = 2 * tw0 - 1;
                    const bool ok = u < HN && ci < a.Cin && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
                    hv[i] = ok ? xb[(long)ci * HW + (long)ih * a.W + iw] : 0.0f;
                }
            }
        };
        auto store = [&]() {
#pragma unroll
            for (int i = 0; i < GU; ++i) {
                const int u = tid + 256 * i;
                const int grp = u & 3, row = (u >> 2) & (WG_TH - 1), ch = u >> 3;
                f16x8 hi, lo;
                wgrad_split8(gv[i], gs, hi, lo);
                const int o = ch * WG_GP + row * WG_TW + grp * 8;
                *(f16x8 *)&sg[0][o] = hi;
                *(f16x8 *)&sg[1][o] = lo;
            }
#pragma unroll
            for (int i = 0; i < XU; ++i) {
                const int u = tid + 256 * i;
                const int grp = u & 3, xr = (u >> 2) % XR, ch = (u >> 2) / XR;
                float ev[8], ov[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    ev[j] = xv[i][2 * j];
                    ov[j] = xv[i][2 * j + 1];
                }
                f16x8 hi, lo;
                const int o = ch * XP + xr * W2_XROW + grp * 8;
                wgrad_split8(ev, xs, hi, lo);
                *(f16x8 *)&sx[0][o] = hi;
                *(f16x8 *)&sx[1][o] = lo;
                if constexpr (KS == 3) {
                    wgrad_split8(ov, xs, hi, lo);
                    *(f16x8 *)&sx[0][o + 40] = hi;
                    *(f16x8 *)&sx[1][o + 40] = lo;
                }
            }
            if constexpr (KS == 3) {
#pragma unroll
                for (int i = 0; i < HU; ++i) {
                    const int u = tid + 256 * i;
                    const int xr = u % XR, ch = u / XR;
                    if (u < HN) {
                        const float t = __fmul_rn(hv[i], xs);
                        const _Float16 hh = (_Float16)t;
                        const int o = ch * XP + xr * W2_XROW + 39;
                        sx[0][o] = hh;
                        sx[1][o] = (_Float16)__fsub_rn(t, (float)hh);
                    }
                }
            }
        };

        f32x16 acc[TAPS];
#pragma unroll
        for (int t = 0; t < TAPS; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;

        load(0);
        for (int tile = 0; tile < ntiles; ++tile) {
            store();
            __syncthreads();                                   // tile `tile` is staged
            if (tile + 1 < ntiles) load(tile + 1);             // in flight under the MFMAs below
            const _Float16 *pg = &sg[0][(wco * 32 + r) * WG_GP + 8 * h];
            const _Float16 *px = &sx[0][(wci * 32 + r) * XP + 8 * h];
            // ---- 4 k-steps of 16 output pixels: (row, 16-column half)
#pragma unroll
            for (int st = 0; st < WG_TH * 2; ++st) {
                const int row = st >> 1, cb = (st & 1) * 16;
                const f16x8 ahi = *(const f16x8 *)(pg + row * WG_TW + cb);
                const f16x8 alo = *(const f16x8 *)(pg + SGN + row * WG_TW + cb);
#pragma unroll
                for (int ky = 0; ky < KS; ++ky) {
                    const _Float16 *q = px + (KS == 3 ? 2 * row + ky : row) * W2_XROW + cb;
                    f16x8 bhi[KS], blo[KS];
                    if constexpr (KS == 3) {
#pragma unroll
                        for (int pl = 0; pl < 2; ++pl) {
                            const _Float16 *qq = q + pl * SXN;
                            // E at qq, the odd plane's block at qq + 40, the block to its left at qq + 32
                            const u32x4 Ev = *(const u32x4 *)qq, L = *(const u32x4 *)(qq + 32), C = *(const u32x4 *)(qq + 40);
                            u32x4 m;
                            m[0] = __builtin_amdgcn_alignbit(C[0], L[3], 16);      // O[ox - 1 .. ox + 6]
                            m[1] = __builtin_amdgcn_alignbit(C[1], C[0], 16);
                            m[2] = __builtin_amdgcn_alignbit(C[2], C[1], 16);
                            m[3] = __builtin_amdgcn_alignbit(C[3], C[2], 16);
                            f16x8 *dst = pl ? blo : bhi;
                            dst[0] = __builtin_bit_cast(f16x8, m);
                            dst[1] = __builtin_bit_cast(f16x8, Ev);
                            dst[2] = __builtin_bit_cast(f16x8, C);
                        }
                    } else {
                        bhi[0] = *(const f16x8 *)q;
                        blo[0] = *(const f16x8 *)(q + SXN);
                    }
#pragma unroll
                    for (int kx = 0; kx < KS; ++kx) {
                        const int tap = ky * KS + kx;
                        acc[tap] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, bhi[kx], acc[tap], 0, 0, 0);
                        acc[tap] = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, bhi[kx], acc[tap], 0, 0, 0);
                        acc[tap] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, blo[kx], acc[tap], 0, 0, 0);
                    }
                }
            }
            __syncthreads();                                   // the tile has been read
        }
        // ---- the partial tile: D[row = co][col = ci], col = lane & 31, row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5)
        const int ci = cib * WG_CB + wci * 32 + r;
        float *wp = a.ws + (long)slice * E;
        if (ci < a.Cin) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int co = cob * WG_CB + wco * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                if (co < a.Cout) {
                    float *p = wp + ((long)co * a.Cin + ci) * TAPS;
#pragma unroll
                    for (int t = 0; t < TAPS; ++t) p[t] = acc[t][i];
                }
            }
        }
    }
}

extern "C" long dkt_conv2d_wgrad_s2_ws_floats(int B, int Cin, int Cout, int H, int W, int K) {
    if (!wgrad_shape_ok(B, Cin, Cout, H, W, K)) return DKT_E_SHAPE;
    return wgrad_ws_floats(B, Cin, Cout, (H - 1) / 2 + 1, (W - 1) / 2 + 1, K);
}

extern "C" int dkt_conv2d_wgrad_s2(const float *x, long x_bstride, const float *g, long g_bstride, const float *scale,
                                   float x_scale, float *gw, float *ws, int B, int Cin, int Cout, int H, int W, int K,
                                   int device, void *stream) {
    if (!x || !g || !scale || !gw || !ws) return DKT_E_NULL;
    if (!wgrad_shape_ok(B, Cin, Cout, H, W, K)) return DKT_E_SHAPE;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    if (x_bstride < (long)Cin * H * W || g_bstride < (long)Cout * Ho * Wo) return DKT_E_SHAPE;
    if (!wgrad_x_scale_ok(x_scale)) return DKT_E_SHAPE;
    DKT_ENTER(device);
    const WgradPlan p = wgrad_plan(B, Cin, Cout, Ho, Wo);
    WgradS2Args a;
    wgrad_fill_args(a, x, x_bstride, g, g_bstride, scale, x_scale, ws, B, Cin, Cout, H, W, p, Wo);
    a.Ho = Ho; a.Wo = Wo;
    const bool vec = (W % 4 == 0) && (Wo % 4 == 0) && (x_bstride % 4 == 0) && (g_bstride % 4 == 0) &&
                     ((uintptr_t)x % 16 == 0) && ((uintptr_t)g % 16 == 0);
    const unsigned blocks = wgrad_blocks(a.items, device);     // one block per CU (108 KiB of LDS)
    hipStream_t st = (hipStream_t)stream;
    if (K == 3) {
        if (vec) hipLaunchKernelGGL((conv_wgrad_s2_kernel<3, 4>), dim3(blocks), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((conv_wgrad_s2_kernel<3, 1>), dim3(blocks), dim3(256), 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((conv_wgrad_s2_kernel<1, 4>), dim3(blocks), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((conv_wgrad_s2_kernel<1, 1>), dim3(blocks), dim3(256), 0, st, a);
    }
    const int rc = dkt_launch_status();
    if (rc != DKT_OK) return rc;
    return wgrad_finish(ws, scale, x_scale, gw, (long)Cout * Cin * K * K, B * p.bands, st);
}
