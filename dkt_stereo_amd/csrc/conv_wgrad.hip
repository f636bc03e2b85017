// conv_wgrad.hip -- the weight gradient of a stride-1 "same" convolution (dkt_stereo_amd/conv.py: _Conv2dGradFn.backward).
// Reference: torch autograd through [relu](conv2d(x, w, b)) (core/update.py:9-10, 19-21, 72-76, 111-113 under training).
// The contract -- GEMM view, hi / lo split, slice plan, split-K workspace and its finishing kernel, which lives here for
// both strides -- is in conv_wgrad_common.h; the reduction grid is H x W.  This file is the stride-1 staging scheme.
//
// Block = 8 waves on one CU: waves 0..3 multiply -- each owns one 32 x 32 fragment with all K*K taps in accumulators (144
// registers for 3x3) -- and waves 4..7 stage, one of each kind per SIMD.  The item walks its band through two LDS buffers
// (136 KiB):
//   sg[buffer][hi|lo][co 64][2 x 32 pixels]                     pitch 144 B = 16 * 9
//   sx[buffer][hi|lo][ci 64][2 + 2p rows][8 | 32 | 8 columns]   pitch 400 B = 16 * 25 (208 B = 16 * 13 for 1x1)
// The staging waves hold two tiles in registers: the global loads of tile t + 1 are issued before tile t is split and
// written, so their latency runs under that conversion and under the MFMAs of tile t - 1; one barrier per tile hands a
// buffer over.  (The first form of this kernel staged and multiplied in the same four waves, two blocks per CU: its 144
// accumulators left the staging addresses in scratch, every reload waited behind the tile's global loads, and the z|r layer
// at 120 x 224 took 810 us against the 618 us of this form.  This form is not free of scratch either: with 512 threads a
// wave has 256 registers for both roles, and the 3x3 kernels compile to 256 VGPRs with 132 spilled, 532 B of scratch; the
// 1x1 kernels to 130 / 132 VGPRs and none.  A compile-time fact -- what the spill costs on the device is not measured,
// DESIGN 3.14.)
// A k-step is 16 pixels of one row; lane l (channel l & 31, half h = l >> 5) reads the 8 pixels 8h.. of the step as ONE
// aligned ds_read_b128: the 16 lanes the LDS serves together differ in the channel alone, and a channel pitch of 16 * odd
// bytes spreads 16 channels over the 64 banks -- conflict-free.  The kx = +-1 taps are built in registers: the aligned block
// to the left (right) of the centre one is read as well and the shifted fragment is four v_alignbit_b32 of neighbouring
// dwords -- per k-step 2 + 18 reads for 27 MFMAs, under the 2-per-MFMA budget.  The column halo is one fp16 per row in the
// last (first) slot of the left (right) 8-column pad; the rest of the pads is never used arithmetically.
// Zero-fill: g' beyond W, beyond the band's last row and beyond Cout; x outside the image and beyond Cin.
#include "conv_wgrad_common.h"

#define WG_XROW 48            // fp16 per staged x row: 8 pad | 32 | 8 pad

struct WgradArgs {
    WGRAD_ARGS_OPERANDS
    WGRAD_ARGS_SLICES
};

// 8 consecutive floats of a row from column iw on; zero from column W on (V = 4: W % 4 == 0, a float4 is inside or outside)
template <int V>
__device__ __forceinline__ void wgrad_load8(const float *row, int iw, int W, bool ok, float (&v)[8]) {
    if (V == 4) {
        const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const float4 a = ok && iw < W ? *(const float4 *)(row + iw) : z;
        const float4 b = ok && iw + 4 < W ? *(const float4 *)(row + iw + 4) : z;
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = ok && iw + j < W ? row[iw + j] : 0.0f;
    }
}

// 8-pixel unit u of the staged x patch: (channel, patch row, 8-column group)
template <int KS, int V>
__device__ __forceinline__ void wgrad_load_x(const WgradArgs &a, const float *xb, int u, int cib, int th0, int tw0, long HW,
                                             float (&v)[8]) {
    constexpr int XR = WG_TH + 2 * (KS / 2);
    const int grp = u & 3, row = (u >> 2) % XR, ch = (u >> 2) / XR;
    const int ci = cib * WG_CB + ch, ih = th0 - KS / 2 + row;
    const bool ok = ci < a.Cin && ih >= 0 && ih < a.H;
    wgrad_load8<V>(xb + (ok ? (long)ci * HW + (long)ih * a.W : 0L), tw0 + grp * 8, a.W, ok, v);
}

template <int KS>
__device__ __forceinline__ void wgrad_store_x(_Float16 *sx, int u, float xs, const float (&v)[8]) {
    constexpr int XR = WG_TH + 2 * (KS / 2), XP = XR * WG_XROW + 8;
    const int grp = u & 3, row = (u >> 2) % XR, ch = (u >> 2) / XR;
    f16x8 hi, lo;
    wgrad_split8(v, xs, hi, lo);
    const int o = ch * XP + row * WG_XROW + 8 + grp * 8;
    *(f16x8 *)&sx[o] = hi;
    *(f16x8 *)&sx[WG_CB * XP + o] = lo;
}

template <int KS, int V>
__global__ __launch_bounds__(512, 1) void conv_wgrad_kernel(WgradArgs a) {
    constexpr int P = KS / 2, TAPS = KS * KS, XR = WG_TH + 2 * P;
    constexpr int XP = XR * WG_XROW + 8;                       // fp16 per staged x channel
    constexpr int GU = WG_CB * WG_TH * 4 / 256;                // 8-pixel units of g' per loader thread
    constexpr int XU = WG_CB * XR * 4 / 256;                   // ... of x
    constexpr int SGN = WG_CB * WG_GP, SXN = WG_CB * XP;       // fp16 per plane
    __shared__ __attribute__((aligned(16))) _Float16 sg[2][2][SGN];      // [buffer][hi | lo]
    __shared__ __attribute__((aligned(16))) _Float16 sx[2][2][SXN];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool loader = wave >= 4;                             // waves 4..7 stage, waves 0..3 multiply: one of each per SIMD
    const int lt = tid & 255;                                  // thread index inside its role
    const int wco = wave & 1, wci = (wave >> 1) & 1;
    const int r = lane & 31, h = lane >> 5;
    const long HW = (long)a.H * a.W;
    const long E = (long)a.Cout * a.Cin * TAPS;
    // wave-uniform device scale of g' (a power of two)
    const float gs = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a.scale[0])));
    const float xs = a.x_scale;
    int tc = 0;                                                // tiles so far: a tile's buffer is its running index & 1

    for (long item = blockIdx.x; item < a.items; item += gridDim.x) {
        const int cib = (int)(item % a.n_ci);
        const long t1 = item / a.n_ci;
        const int cob = (int)(t1 % a.n_co);
        const int slice = (int)(t1 / a.n_co);
        const int band = slice % a.bands, b = slice / a.bands;
        const int r0 = band * a.rows_band;
        const int r1 = min(a.H, r0 + a.rows_band);
        const int ntiles = ((r1 - r0 + WG_TH - 1) / WG_TH) * a.tiles_w;
        if (loader) {
            // ---- the staging waves: the loads of tile t + 1 are issued before tile t is converted and written, so their
            // latency runs under that conversion and under the other waves' MFMAs; one barrier per tile hands a buffer over.
            // Buffer (tc + t) & 1 was last read for tile t - 2, which the multiplying waves finished before the barrier of
            // tile t - 1.
            const float *gb = a.g + (long)b * a.g_bs;
            const float *xb = a.x + (long)b * a.x_bs;
            float gv[2][GU][8], xv[2][XU][8], hv[2][2];
            auto load = [&](int tile, float (&g8)[GU][8], float (&x8)[XU][8], float (&h1)[2]) {
                const int th0 = r0 + (tile / a.tiles_w) * WG_TH;
                const int tw0 = (tile % a.tiles_w) * WG_TW;
#pragma unroll
                for (int i = 0; i < GU; ++i) {
                    const int u = lt + 256 * i;
                    const int grp = u & 3, row = (u >> 2) & (WG_TH - 1), ch = u >> 3;
                    const int co = cob * WG_CB + ch, ih = th0 + row;
                    const bool ok = co < a.Cout && ih < r1;
                    wgrad_load8<V>(gb + (ok ? (long)co * HW + (long)ih * a.W : 0L), tw0 + grp * 8, a.W, ok, g8[i]);
                }
#pragma unroll
                for (int i = 0; i < XU; ++i) wgrad_load_x<KS, V>(a, xb, lt + 256 * i, cib, th0, tw0, HW, x8[i]);
                if (KS == 3) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int u = lt + 256 * i;
                        const int side = u & 1, row = (u >> 1) & 3, ch = u >> 3;
                        const int ci = cib * WG_CB + ch, ih = th0 - P + row, iw = side ? tw0 + WG_TW : tw0 - 1;
                        const bool ok = ci < a.Cin && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
                        h1[i] = ok ? xb[(long)ci * HW + (long)ih * a.W + iw] : 0.0f;
                    }
                }
            };
            auto store = [&](int buf, const float (&g8)[GU][8], const float (&x8)[XU][8], const float (&h1)[2]) {
#pragma unroll
                for (int i = 0; i < GU; ++i) {
                    const int u = lt + 256 * i;
                    const int grp = u & 3, row = (u >> 2) & (WG_TH - 1), ch = u >> 3;
                    f16x8 hi, lo;
                    wgrad_split8(g8[i], gs, hi, lo);
                    const int o = ch * WG_GP + row * WG_TW + grp * 8;
                    *(f16x8 *)&sg[buf][0][o] = hi;
                    *(f16x8 *)&sg[buf][1][o] = lo;
                }
#pragma unroll
                for (int i = 0; i < XU; ++i) wgrad_store_x<KS>(&sx[buf][0][0], lt + 256 * i, xs, x8[i]);
                if (KS == 3) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int u = lt + 256 * i;
                        const int side = u & 1, row = (u >> 1) & 3, ch = u >> 3;
                        const float t = __fmul_rn(h1[i], xs);
                        const _Float16 hh = (_Float16)t;
                        const int o = ch * XP + row * WG_XROW + (side ? 8 + WG_TW : 7);
                        sx[buf][0][o] = hh;
                        sx[buf][1][o] = (_Float16)__fsub_rn(t, (float)hh);
                    }
                }
            };
            load(0, gv[0], xv[0], hv[0]);
            for (int t = 0; t < ntiles; t += 2) {
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const int tt = t + p;
                    if (tt < ntiles) {
                        if (tt + 1 < ntiles) load(tt + 1, gv[p ^ 1], xv[p ^ 1], hv[p ^ 1]);
                        store((tc + tt) & 1, gv[p], xv[p], hv[p]);
                        __syncthreads();                       // tile tt is staged
                    }
                }
            }
        } else {
            f32x16 acc[TAPS];
#pragma unroll
            for (int t = 0; t < TAPS; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
            for (int tile = 0; tile < ntiles; ++tile) {
                const int buf = (tc + tile) & 1;
                const _Float16 *pg = &sg[buf][0][(wco * 32 + r) * WG_GP + 8 * h];
                const _Float16 *px = &sx[buf][0][(wci * 32 + r) * XP + 8 * h];
                __syncthreads();                               // tile `tile` is staged
                // ---- 4 k-steps of 16 pixels: (row, 16-column half)
#pragma unroll
                for (int st = 0; st < WG_TH * 2; ++st) {
                    const int row = st >> 1, cb = (st & 1) * 16;
                    const f16x8 ahi = *(const f16x8 *)(pg + row * WG_TW + cb);
                    const f16x8 alo = *(const f16x8 *)(pg + SGN + row * WG_TW + cb);
#pragma unroll
                    for (int ky = 0; ky < KS; ++ky) {
                        const _Float16 *q = px + (row + ky) * WG_XROW + cb;  // blocks: left at q, centre at q + 8, right at q + 16
                        f16x8 bhi[KS], blo[KS];
                        if (KS == 3) {
#pragma unroll
                            for (int pl = 0; pl < 2; ++pl) {
                                const _Float16 *qq = q + pl * SXN;
                                const u32x4 L = *(const u32x4 *)qq, C = *(const u32x4 *)(qq + 8), R = *(const u32x4 *)(qq + 16);
                                u32x4 m, n;
                                m[0] = __builtin_amdgcn_alignbit(C[0], L[3], 16);      // columns -1 .. 6 of the centre block
                                m[1] = __builtin_amdgcn_alignbit(C[1], C[0], 16);
                                m[2] = __builtin_amdgcn_alignbit(C[2], C[1], 16);
                                m[3] = __builtin_amdgcn_alignbit(C[3], C[2], 16);
                                n[0] = m[1];                                            // columns 1 .. 8
                                n[1] = m[2];
                                n[2] = m[3];
                                n[3] = __builtin_amdgcn_alignbit(R[0], C[3], 16);
                                f16x8 *dst = pl ? blo : bhi;
                                dst[0] = __builtin_bit_cast(f16x8, m);
                                dst[1] = __builtin_bit_cast(f16x8, C);
                                dst[2] = __builtin_bit_cast(f16x8, n);
                            }
                        } else {
                            bhi[0] = *(const f16x8 *)(q + 8);
                            blo[0] = *(const f16x8 *)(q + SXN + 8);
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
        tc += ntiles;
    }
}

struct WgradFinishArgs {
    const float *ws, *scale;
    float inv_x_scale;
    float *gw;
    long E;
    int nslices;
};

// One thread per weight: its slices in ascending order, then the un-scaling (a power of two).
__global__ __launch_bounds__(256) void conv_wgrad_finish_kernel(WgradFinishArgs a) {
    const float un = __fmul_rn(a.scale[1], a.inv_x_scale);
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < a.E; e += (long)gridDim.x * 256) {
        float s = 0.0f;
#pragma unroll 4
        for (int k = 0; k < a.nslices; ++k) s = __fadd_rn(s, a.ws[(long)k * a.E + e]);
        a.gw[e] = __fmul_rn(s, un);
    }
}

int wgrad_finish(const float *ws, const float *scale, float x_scale, float *gw, long E, int nslices, hipStream_t st) {
    WgradFinishArgs f;
    f.ws = ws; f.scale = scale; f.inv_x_scale = 1.0f / x_scale; f.gw = gw;
    f.E = E;
    f.nslices = nslices;
    const long fb = (E + 255) / 256;
    hipLaunchKernelGGL(conv_wgrad_finish_kernel, dim3((unsigned)(fb < 4096 ? fb : 4096)), dim3(256), 0, st, f);
    return dkt_launch_status();
}

extern "C" long dkt_conv2d_wgrad_ws_floats(int B, int Cin, int Cout, int H, int W, int K) {
    if (!wgrad_shape_ok(B, Cin, Cout, H, W, K)) return DKT_E_SHAPE;
    return wgrad_ws_floats(B, Cin, Cout, H, W, K);
}

extern "C" int dkt_conv2d_wgrad(const float *x, long x_bstride, const float *g, long g_bstride, const float *scale,
                                float x_scale, float *gw, float *ws, int B, int Cin, int Cout, int H, int W, int K,
                                int device, void *stream) {
    if (!x || !g || !scale || !gw || !ws) return DKT_E_NULL;
    if (!wgrad_shape_ok(B, Cin, Cout, H, W, K)) return DKT_E_SHAPE;
    const long HW = (long)H * W;
    if (x_bstride < (long)Cin * HW || g_bstride < (long)Cout * HW) return DKT_E_SHAPE;
    if (!wgrad_x_scale_ok(x_scale)) return DKT_E_SHAPE;
    DKT_ENTER(device);
    const WgradPlan p = wgrad_plan(B, Cin, Cout, H, W);
    WgradArgs a;
    wgrad_fill_args(a, x, x_bstride, g, g_bstride, scale, x_scale, ws, B, Cin, Cout, H, W, p, W);
    const bool vec = (W % 4 == 0) && (x_bstride % 4 == 0) && (g_bstride % 4 == 0) &&
                     ((uintptr_t)x % 16 == 0) && ((uintptr_t)g % 16 == 0);
    const unsigned blocks = wgrad_blocks(a.items, device);     // one block of 8 waves per CU (136 KiB of LDS)
    hipStream_t st = (hipStream_t)stream;
    if (K == 3) {
        if (vec) hipLaunchKernelGGL((conv_wgrad_kernel<3, 4>), dim3(blocks), dim3(512), 0, st, a);
        else hipLaunchKernelGGL((conv_wgrad_kernel<3, 1>), dim3(blocks), dim3(512), 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((conv_wgrad_kernel<1, 4>), dim3(blocks), dim3(512), 0, st, a);
        else hipLaunchKernelGGL((conv_wgrad_kernel<1, 1>), dim3(blocks), dim3(512), 0, st, a);
    }
    const int rc = dkt_launch_status();
    if (rc != DKT_OK) return rc;
    return wgrad_finish(ws, scale, x_scale, gw, (long)Cout * Cin * K * K, B * p.bands, st);
}
