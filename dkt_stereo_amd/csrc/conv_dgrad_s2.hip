// conv_dgrad_s2.hip -- the input gradient of a stride-2, padding K/2 convolution, K in {1, 3} (dkt_stereo_amd/conv.py:
// _Conv2dGradFn.backward for the encoders' down-sampling layers).
// Reference: torch autograd through conv2d(x, w, b, stride=2) (core/extractor.py:6-60, :122-175 under training):
//   gx[b,ci,y,x] = sum_{co,ky,kx} g'[b,co,oy,ox] * w[co,ci,ky,kx]     with y = 2 oy + ky - p, x = 2 ox + kx - p, p = K/2
//
// Decomposition by output parity (K = 3).  On the Ho x Wo grid of g', pixel (i, j) owns the four outputs (2i + py, 2j + px):
//   (even, even)  w[1][1] g'(i, j)
//   (even, odd)   w[1][0] g'(i, j+1) + w[1][2] g'(i, j)
//   (odd, even)   w[0][1] g'(i+1, j) + w[2][1] g'(i, j)
//   (odd, odd)    w[0][0] g'(i+1, j+1) + w[0][2] g'(i+1, j) + w[2][0] g'(i, j+1) + w[2][2] g'(i, j)
// nine (parity, tap) products per pixel of g' -- the useful work: no zero-inserted copy of g' exists anywhere, nothing is
// scattered and nothing is cleared beforehand.  K = 1: (even, even) = w g'(i, j); the kernel stores the zeros of the other
// three parities itself.  Every element of gx is stored exactly once, by one lane: no atomics, the same bits every run.
//
// GEMM view   D[ci][pixel] = sum_{co} Wt[tap][co][ci] * G[co][pixel (+ neighbour)]:
//   A = the weight of the input gradient (transposed over (Cout, Cin), rotated by 180 degrees) in the pack layout of
//       dkt_conv2d_pack_weights, [tap][co/16][ci pad 64][16] fp16 hi / lo: a fragment is one 16-byte load per lane;
//   B = g' * scale[0] (the device pair of dkt_conv_grad_prepass), split into fp16 hi / lo while it is staged as a
//       (4 + 1) x (32 + 1) pixel patch of 32 channels, [pixel][channel], pitch 80 B (conflict-free ds_read_b128);
//   D = four parity accumulators per 32 output channels, pixels along lanes: the two column parities of a lane are one
//       float2, a wave's store of one row is 256 dense bytes.
// w_hi*g_hi + w_lo*g_hi + w_hi*g_lo on v_mfma_f32_32x32x16_f16, fp32 accumulation, un-scaled by scale[1] * w_inv_scale:
// every factor outside the fp16 operands is a power of two, so g' * 2^m gives gx * 2^m bit for bit.
// Block = 4 waves; tile = 4 rows x 32 columns of g' (8 x 64 of gx) x 64 output channels; wave w owns row w of the tile.
#include "dkt_common.h"
#include <cmath>

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define DG_TR 4               // rows of g' per tile, one per wave
#define DG_TW 32              // columns of g' per tile
#define DG_KC 32              // channels of g' per staged chunk
#define DG_PP 40              // fp16 per staged pixel: 32 channels + 8 pad
#define DG_OC 64              // output channels per block

struct DgradS2Args {
    const float *g, *scale;
    const _Float16 *whi, *wlo;
    float w_inv_scale;
    float *gx;
    long g_bs, gx_bs;
    int Cin, Cout;            // channels of gx / of g'
    int CoPad, nch16;         // the pack's padded output-channel count (Cin to 64) and its 16-channel reduction steps
    int H, W, Ho, Wo, tiles_w;
};

__device__ __forceinline__ f32x16 dg_mfma3(f32x16 acc, f16x8 ahi, f16x8 alo, f16x8 bhi, f16x8 blo) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, bhi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, bhi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, blo, acc, 0, 0, 0);
    return acc;
}

// the two column parities (x0, x0 + 1) of one output row; V = 2: W is even, row starts are 8-byte aligned
template <int V>
__device__ __forceinline__ void dg_store2(float *row, int x0, int W, float a, float b) {
    if (V == 2) {
        if (x0 + 1 < W) *(float2 *)(row + x0) = make_float2(a, b);
    } else {
        if (x0 < W) row[x0] = a;
        if (x0 + 1 < W) row[x0 + 1] = b;
    }
}

template <int KS, int V>
__global__ __launch_bounds__(256) void conv_dgrad_s2_kernel(DgradS2Args a) {
    constexpr int PR = KS == 3 ? DG_TR + 1 : DG_TR;            // patch rows
    constexpr int PC = KS == 3 ? DG_TW + 1 : DG_TW;            // patch columns
    constexpr int NPX = PR * PC;
    constexpr int NE = NPX * DG_KC;                            // staged elements per chunk
    constexpr int NL = (NE + 255) / 256;                       // ... per thread
    constexpr int NPAR = KS == 3 ? 4 : 1;                      // parities with products
    __shared__ __attribute__((aligned(16))) _Float16 sp[2][NPX * DG_PP];     // [hi | lo][pixel][channel]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int i0 = ((int)blockIdx.x / a.tiles_w) * DG_TR, j0 = ((int)blockIdx.x % a.tiles_w) * DG_TW;
    const int ocb = blockIdx.y, b = blockIdx.z;
    const long HoWo = (long)a.Ho * a.Wo, HW = (long)a.H * a.W;
    const float gs = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a.scale[0])));
    const float *gb = a.g + (long)b * a.g_bs;

    f32x16 acc[NPAR][2];
#pragma unroll
    for (int p = 0; p < NPAR; ++p)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[p][m][i] = 0.0f;

    const int nchunks = a.nch16 >> 1;
    for (int cc = 0; cc < nchunks; ++cc) {
        // ---- stage 32 channels of the patch: every load first, then the split
        float v[NL];
#pragma unroll
        for (int n = 0; n < NL; ++n) {
            const int e = tid + 256 * n;
            const int col = e % PC, t = e / PC;
            const int row = t % PR, ch = t / PR;
            const int c = cc * DG_KC + ch, oy = i0 + row, ox = j0 + col;
            const bool ok = e < NE && c < a.Cout && oy < a.Ho && ox < a.Wo;
            v[n] = ok ? gb[(long)c * HoWo + (long)oy * a.Wo + ox] : 0.0f;
        }
        if (cc > 0) __syncthreads();                           // the previous chunk has been read
#pragma unroll
        for (int n = 0; n < NL; ++n) {
            const int e = tid + 256 * n;
            const int col = e % PC, t = e / PC;
            const int row = t % PR, ch = t / PR;
            if (e < NE) {
                const float s = __fmul_rn(v[n], gs);
                const _Float16 hi = (_Float16)s;
                const int o = (row * PC + col) * DG_PP + ch;
                sp[0][o] = hi;
                sp[1][o] = (_Float16)__fsub_rn(s, (float)hi);
            }
        }
        __syncthreads();
        // ---- two reduction steps of 16 channels
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int o00 = ((wave * PC) + r) * DG_PP + ks * 16 + 8 * h;
            const f16x8 b00h = *(const f16x8 *)&sp[0][o00], b00l = *(const f16x8 *)&sp[1][o00];
            const long wbase = ((long)(cc * 2 + ks) * a.CoPad + ocb * DG_OC + r) * 16 + 8 * h;
            const long wtap = (long)a.nch16 * a.CoPad * 16;    // elements per tap
            if constexpr (KS == 3) {
                const int o01 = o00 + DG_PP, o10 = o00 + PC * DG_PP, o11 = o10 + DG_PP;
                const f16x8 b01h = *(const f16x8 *)&sp[0][o01], b01l = *(const f16x8 *)&sp[1][o01];
                const f16x8 b10h = *(const f16x8 *)&sp[0][o10], b10l = *(const f16x8 *)&sp[1][o10];
                const f16x8 b11h = *(const f16x8 *)&sp[0][o11], b11l = *(const f16x8 *)&sp[1][o11];
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    // w[ky][kx] sits at tap (2 - ky) * 3 + (2 - kx) of the rotated pack
#define DG_W(ky, kx, name)                                                                                   \
    const f16x8 name##h = *(const f16x8 *)(a.whi + wbase + ((2 - (ky)) * 3 + (2 - (kx))) * wtap + m * 32 * 16); \
    const f16x8 name##l = *(const f16x8 *)(a.wlo + wbase + ((2 - (ky)) * 3 + (2 - (kx))) * wtap + m * 32 * 16);
                    DG_W(1, 1, w11) DG_W(1, 0, w10) DG_W(1, 2, w12) DG_W(0, 1, w01) DG_W(2, 1, w21)
                    DG_W(0, 0, w00) DG_W(0, 2, w02) DG_W(2, 0, w20) DG_W(2, 2, w22)
#undef DG_W
                    acc[0][m] = dg_mfma3(acc[0][m], w11h, w11l, b00h, b00l);
                    acc[1][m] = dg_mfma3(acc[1][m], w10h, w10l, b01h, b01l);
                    acc[1][m] = dg_mfma3(acc[1][m], w12h, w12l, b00h, b00l);
                    acc[2][m] = dg_mfma3(acc[2][m], w01h, w01l, b10h, b10l);
                    acc[2][m] = dg_mfma3(acc[2][m], w21h, w21l, b00h, b00l);
                    acc[3][m] = dg_mfma3(acc[3][m], w00h, w00l, b11h, b11l);
                    acc[3][m] = dg_mfma3(acc[3][m], w02h, w02l, b10h, b10l);
                    acc[3][m] = dg_mfma3(acc[3][m], w20h, w20l, b01h, b01l);
                    acc[3][m] = dg_mfma3(acc[3][m], w22h, w22l, b00h, b00l);
                }
            } else {
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const f16x8 wh = *(const f16x8 *)(a.whi + wbase + m * 32 * 16);
                    const f16x8 wl = *(const f16x8 *)(a.wlo + wbase + m * 32 * 16);
                    acc[0][m] = dg_mfma3(acc[0][m], wh, wl, b00h, b00l);
                }
            }
        }
    }
    // ---- D[row = channel][col = pixel]: col = lane & 31, row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5)
    const float un = __fmul_rn(a.scale[1], a.w_inv_scale);
    const int y0 = 2 * (i0 + wave), x0 = 2 * (j0 + r);
    float *ob = a.gx + (long)b * a.gx_bs;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int oc = ocb * DG_OC + m * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            if (oc < a.Cin) {
                float *p = ob + (long)oc * HW;
                if constexpr (KS == 3) {
                    if (y0 < a.H)
                        dg_store2<V>(p + (long)y0 * a.W, x0, a.W, __fmul_rn(acc[0][m][i], un), __fmul_rn(acc[1][m][i], un));
                    if (y0 + 1 < a.H)
                        dg_store2<V>(p + (long)(y0 + 1) * a.W, x0, a.W, __fmul_rn(acc[2][m][i], un),
                                     __fmul_rn(acc[3][m][i], un));
                } else {
                    if (y0 < a.H) dg_store2<V>(p + (long)y0 * a.W, x0, a.W, __fmul_rn(acc[0][m][i], un), 0.0f);
                    if (y0 + 1 < a.H) dg_store2<V>(p + (long)(y0 + 1) * a.W, x0, a.W, 0.0f, 0.0f);
                }
            }
        }
    }
}

extern "C" int dkt_conv2d_dgrad_s2(const float *g, long g_bstride, const void *w_hi, const void *w_lo, float w_inv_scale,
                                   const float *scale, float *gx, long gx_bstride, int B, int Cin, int Cout, int H, int W,
                                   int K, int device, void *stream) {
    if (!g || !w_hi || !w_lo || !scale || !gx) return DKT_E_NULL;
    if (B < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1 || (K != 1 && K != 3)) return DKT_E_SHAPE;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    if (g_bstride < (long)Cout * Ho * Wo || gx_bstride < (long)Cin * H * W) return DKT_E_SHAPE;
    if (!(w_inv_scale > 0.0f) || !std::isfinite(w_inv_scale)) return DKT_E_SHAPE;
    if (B > 65535 || (Cin + DG_OC - 1) / DG_OC > 65535) return DKT_E_SHAPE;
    DKT_ENTER(device);
    DgradS2Args a;
    a.g = g; a.scale = scale; a.whi = (const _Float16 *)w_hi; a.wlo = (const _Float16 *)w_lo;
    a.w_inv_scale = w_inv_scale; a.gx = gx; a.g_bs = g_bstride; a.gx_bs = gx_bstride;
    a.Cin = Cin; a.Cout = Cout;
    a.CoPad = (Cin + 63) & ~63;
    a.nch16 = ((Cout + 31) & ~31) / 16;
    a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo;
    a.tiles_w = (Wo + DG_TW - 1) / DG_TW;
    const long tiles = (long)a.tiles_w * ((Ho + DG_TR - 1) / DG_TR);
    const dim3 grid((unsigned)tiles, (unsigned)((Cin + DG_OC - 1) / DG_OC), (unsigned)B);
    const bool vec = (W % 2 == 0) && (gx_bstride % 2 == 0) && ((uintptr_t)gx % 8 == 0);
    hipStream_t st = (hipStream_t)stream;
    if (K == 3) {
        if (vec) hipLaunchKernelGGL((conv_dgrad_s2_kernel<3, 2>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((conv_dgrad_s2_kernel<3, 1>), grid, dim3(256), 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((conv_dgrad_s2_kernel<1, 2>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((conv_dgrad_s2_kernel<1, 1>), grid, dim3(256), 0, st, a);
    }
    return dkt_launch_status();
}
