// conv2d.hip -- implicit-GEMM 2-D convolution for the update operator on gfx950.
//
// The ConvGRU / motion-encoder / head convolutions are ~98 % of a RAFT-Stereo
// iteration (core/update.py:19-21, 72-76, 9-10, 111-113).  fp32 MFMA peaks at
// 157 TFLOP/s on MI355X, 1/16 of the fp16 rate, so this kernel evaluates the
// fp32 convolution on the fp16 matrix cores with SPLIT operands:
//     w*s = w_hi + w_lo,  x = x_hi + x_lo   (each part fp16, s a power of two)
//     w*x*s ~= w_hi*x_hi + w_lo*x_hi + w_hi*x_lo      (fp32 accumulation)
// which keeps ~22 significant bits per operand (fp32 has 24) at three
// v_mfma_f32_32x32x16_f16 per product block: 833 TFLOP/s-equivalent peak, 5.3x
// the fp32 pipe.  PASSES = 3 is that form (measured 1.5e-6 relative to an fp64
// convolution, the vendor fp32 path measures 0.9e-6); PASSES = 2 drops
// w_hi*x_lo (activations rounded to fp16, weights still split); PASSES = 1 is
// plain fp16.
//
// GEMM view   D[co][px] = sum_{tap, ci} Wp[tap][ci][co] * X[ci][px + off(tap)]
//   A = weights, pre-packed once per layer to [tap][ci/16][co][16] fp16 so a
//       fragment (lane l: A[co = l&31][k = 8*(l>>5)..+7]) is one coalesced
//       16-byte load per lane straight from L2 -- no LDS for weights; loads run
//       two (tap, k16) steps ahead of the MFMAs that consume them;
//   B = activations: NCHW fp32 in HBM (possibly several tensors = the
//       reference's torch.cat operands, read in place), staged per 32-channel
//       chunk as a (rows+halo) x (32+halo) pixel patch in LDS, converted to
//       fp16 hi/lo and transposed to [pixel][channel] (pitch 80 B: conflict-
//       free ds_read_b128 for the fragment lane l: B[k = 8*(l>>5)..+7][px = l&31]);
//       each staged patch is reused by all taps and ALL output channels of the
//       block (a block spans up to 256 output channels, so a patch is staged once);
//   D accumulators keep pixels along lanes (C/D map col = l&31), so output
//       stores are 128-byte NCHW rows.
// Block = 4 waves inside a 256-VGPR budget (two blocks per CU).  Wave tile = 32*MF output
// channels (MF = 2; 1 for the 1-2 channel heads) x NF rows x 32 columns; WM x WN waves along (channels, rows).  Blocks are
// persistent (a stream of tiles per block); LDS is double buffered: the fp32 loads of
// chunk c+1 -- of this tile or the block's next one -- are in flight under the MFMAs of
// chunk c; one barrier per chunk.  Which instantiation a call runs on -- the tile shape by layer width and image size, the
// stride-2 shapes, the weights-stationary kernel of conv_ws.h -- is decided in conv_tile.h and nowhere else.
#include "dkt_common.h"
#include "conv_tile.h"
#include <cstdlib>
#include <cstring>
#include <type_traits>

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define CONV_MAX_SRC 4
// scheduling tunables (swept with tools/build_conv_variant.sh + tools/conv_ablation.py)
#ifndef CONV_AR
#define CONV_AR 3
#endif
#ifndef CONV_MIN_BLOCKS
#define CONV_MIN_BLOCKS 2    // blocks per CU the register budget is capped for (256 VGPRs)
#endif
#ifndef CONV_AR_NF1
#define CONV_AR_NF1 3
#endif
#ifndef CONV_SGB_MFMA
#define CONV_SGB_MFMA 1
#endif
#ifndef CONV_SGB_MEM
#define CONV_SGB_MEM 1
#endif
#ifndef CONV_SGB_VALU
#define CONV_SGB_VALU 3
#endif

struct ConvArgs {
    const float *src[CONV_MAX_SRC];
    long src_bs[CONV_MAX_SRC];
    int src_ch[CONV_MAX_SRC];
    int nsrc;
    const _Float16 *whi;
    const _Float16 *wlo;
    const float *bias;
    float out_scale;  // 1 / (weight scale * in_scale)
    float in_scale;   // power of two applied to the activations before the fp16 split (range control)
    float *out;
    long out_bs;
    int H, W, Cout, CoutPad, nch16, tiles_w;
    int Ho, Wo;                        // output size (== H, W for stride 1)
    int tiles_xy, n_co, total_tiles;   // persistent tile stream: id = (b*n_co + co block)*tiles_xy + xy
    int relu;
    // fused ConvGRU gate epilogues (core/update.py:27-31), epi = 0 none;
    //   1: merged z|r convolution, Cout = 2*Ch:  co <  Ch: z  = sigmoid(v + cz)        -> out  (z)
    //                                            co >= Ch: rh = sigmoid(v + cr) * h    -> out2 (r*h)
    //   2: q convolution, Cout = Ch:             h' = (1 - z)*h + z*tanh(v + cq)        -> out  (may alias h)
    int epi;
    const float *e_c0;   // cz (epi 1) / cq (epi 2)
    const float *e_c1;   // cr (epi 1) / z  (epi 2)
    const float *e_h;    // h
    long e_c0_bs, e_c1_bs, e_h_bs;
    float *out2;
    long out2_bs;
    //   3: residual join (core/extractor.py:60 with the preceding norm folded into the weights):
    //      out = relu(e_c0 + [relu](v))
    // Instance-norm of the INPUT folded into the staging (kernel instantiations with NRM = 1; one source):
    // (mean, 1/std) per (batch, channel) plane; the kernel convolves relu((x - mean) * invstd).
    // Kernel instantiations with DSC = 1 (never together with NRM) find the device-resident scales in this slot instead, so
    // that the argument block keeps its layout: in_norm[0] replaces in_scale, out_scale is multiplied by in_norm[1] -- the
    // pair dkt_conv_grad_prepass writes, read by the kernel, never by the host.
    const float *in_norm;
    // Instance-norm statistics of the OUTPUT accumulated in the epilogue (epi 0): every wave writes the sums and sums of
    // squares of its channels over its rows x 32 columns to stats_ws[((b * entries + e) * Cout + co) * 2 + {0, 1}], entry
    // e = (tile index in the image) * WN + wave row; conv_stats_reduce (norm.hip) folds them into the fp64 partial-sum
    // workspace the instance-norm kernels read (the statistics pass over the 235 MB activation disappears).
    float *stats_ws;
    double *stats_part;
    long stats_hw;       // filled by launch_conv: plane size of the output
    // Sub-sampled sources (a 1x1 stride-2 projection run as a 1x1 stride-1 layer on every second pixel of every second row:
    // the tiled stride-2 form stages the odd rows and columns it never uses -- three quarters of its requests): H, W are the
    // OUTPUT size, src_px the pixel stride in the source, src_w / src_hw its row pitch and plane size.  Plain layers: 1, W, H*W.
    int src_px, src_w;
    long src_hw;
};
// norm.hip: folds stats_ws into stats_part, then recomputes from `out` the planes whose fp32 sums are ill-conditioned
int conv_stats_reduce(const float *ws, double *part, int B, int C, long entries, long HW, const float *out, long out_bs,
                      hipStream_t st);

// Gate non-linearities for the fused epilogues.  The epilogue runs on the VALU after the
// MFMA loop with nothing to overlap it, so it uses the hardware transcendentals
// (v_exp_f32 / v_rcp_f32, ~1 ulp each: absolute error <= 3e-7 on (0,1) / (-1,1)) rather than
// the ~45-instruction correctly-rounded forms the streaming gate kernels afford
// (measured: precise forms cost +7.7 ms per pair, these -x ms).
__device__ __forceinline__ float conv_sigmoid(float x) {
    return __frcp_rn(1.0f + __expf(-x));
}
__device__ __forceinline__ float conv_tanh(float x) {
    const float xc = x < -15.0f ? -15.0f : (x > 15.0f ? 15.0f : x);      // NaN passes through
    const float t = __expf(2.0f * xc);
    return (t - 1.0f) * __frcp_rn(t + 1.0f);
}

__device__ __forceinline__ unsigned pack_h2(_Float16 a, _Float16 b) {
    union { _Float16 h[2]; unsigned u; } v;
    v.h[0] = a;
    v.h[1] = b;
    return v.u;
}

struct ConvArgsPair {
    ConvArgs p[2];
};

// A wave-uniform value pinned to scalar registers: what comes out cannot be recomputed (or re-loaded from the argument
// segment) from what went in.  (readfirstlane first: a uniform value the compiler computed on the vector ALU -- the
// quotients of decode() -- is in a vector register.)  The epilogue reads its arguments through these, once per tile.
__device__ __forceinline__ unsigned conv_hold(unsigned x) {
    x = __builtin_amdgcn_readfirstlane(x);
    asm volatile("" : "+s"(x));
    return x;
}
__device__ __forceinline__ int conv_hold(int x) { return (int)conv_hold((unsigned)x); }
__device__ __forceinline__ float conv_hold(float x) { return __uint_as_float(conv_hold(__float_as_uint(x))); }
template <class T>
__device__ __forceinline__ T *conv_hold(T *p) {
    // (every pointer of the argument structure is a global one; rebuilt from two integers it would be a flat one)
    const unsigned long long v = (unsigned long long)p;
    return (T *)(__attribute__((address_space(1))) T *)(((unsigned long long)conv_hold((unsigned)(v >> 32)) << 32) | conv_hold((unsigned)v));
}
// Four pointers in ONE statement: the scalar loads they are formed from are issued back to back behind one wait (a
// statement per pointer is a load, a wait and the statement, pointer after pointer).
template <class T0, class T1, class T2, class T3>
__device__ __forceinline__ void conv_hold4(T0 *&p0, T1 *&p1, T2 *&p2, T3 *&p3) {
    const unsigned long long v0 = (unsigned long long)p0, v1 = (unsigned long long)p1, v2 = (unsigned long long)p2, v3 = (unsigned long long)p3;
    unsigned l0 = __builtin_amdgcn_readfirstlane((unsigned)v0), h0 = __builtin_amdgcn_readfirstlane((unsigned)(v0 >> 32));
    unsigned l1 = __builtin_amdgcn_readfirstlane((unsigned)v1), h1 = __builtin_amdgcn_readfirstlane((unsigned)(v1 >> 32));
    unsigned l2 = __builtin_amdgcn_readfirstlane((unsigned)v2), h2 = __builtin_amdgcn_readfirstlane((unsigned)(v2 >> 32));
    unsigned l3 = __builtin_amdgcn_readfirstlane((unsigned)v3), h3 = __builtin_amdgcn_readfirstlane((unsigned)(v3 >> 32));
    asm volatile("" : "+s"(l0), "+s"(h0), "+s"(l1), "+s"(h1), "+s"(l2), "+s"(h2), "+s"(l3), "+s"(h3));
    p0 = (T0 *)(__attribute__((address_space(1))) T0 *)(((unsigned long long)h0 << 32) | l0);
    p1 = (T1 *)(__attribute__((address_space(1))) T1 *)(((unsigned long long)h1 << 32) | l1);
    p2 = (T2 *)(__attribute__((address_space(1))) T2 *)(((unsigned long long)h2 << 32) | l2);
    p3 = (T3 *)(__attribute__((address_space(1))) T3 *)(((unsigned long long)h3 << 32) | l3);
}
// The same for an address formed per access, without `volatile` (a volatile statement is a fence for the memory operations
// around it: the loads of an operand batch would go out one by one); this one only cannot be folded into the lane offset
// that is added to it, so the access keeps the form scalar base + 32-bit lane offset.
template <class T>
__device__ __forceinline__ T *conv_base(T *p) {
    unsigned long long v = (unsigned long long)p;
    unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    asm("" : "+s"(lo), "+s"(hi));
    return (T *)(__attribute__((address_space(1))) T *)(((unsigned long long)hi << 32) | lo);
}
template <int V>
struct ConvTag {
    static constexpr int value = V;
};

// DSC = 1: in_scale / out_scale come from device memory -- the input gradient of a convolution, whose
// range only the device knows (conv_grad.hip; the pair sits in ConvArgs::in_norm).  Instantiated for the tile shapes of the stride-1 selection alone, in
// translation units of their own; with DSC = 0 the flag compiles to nothing (the code of every other instantiation is the
// code it had without the flag).
template <int KS, int WM, int WN, int NF, int PASSES, int MF = 2, int ST = 1, int CK = 2, int NRM = 0, int DSC = 0>
__global__ __launch_bounds__(64 * WM * WN, (WM * WN > 4 ? 1 : CONV_MIN_BLOCKS)) void conv2d_f16s_kernel(ConvArgsPair ap, int nb0) {
    static_assert(!(DSC && (NRM || ST != 1)), "the device scales share the argument slot of in_norm; stride 1 only");
    // Two independent convolutions may share one launch (dkt_conv2d_f16s_pair): blocks [0, nb0) stream
    // the tiles of problem 0, the others those of problem 1 -- a small layer (the coarsest GRU: 36
    // tiles) then rides in the tile-quantisation slack of a large one (the finest GRU: 460 tiles on
    // 256 resident blocks) instead of occupying the device for a launch of its own.  The selection
    // is block-uniform: every a.field below is a scalar load from the chosen argument block.
    const bool second = (int)blockIdx.x >= nb0;
    const ConvArgs &a = ap.p[second ? 1 : 0];      // uniform index into the kernel-argument segment: scalar loads
    const int blk_first = second ? nb0 : 0;
    const int blk_count = second ? (int)gridDim.x - nb0 : nb0;
    // DSC: the scales come from device memory (wave-uniform: pinned into SGPRs); both factors are powers of two
    const float dsc_in = DSC ? __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a.in_norm[0]))) : 0.0f;
    const float dsc_out = DSC ? __fmul_rn(a.out_scale, __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a.in_norm[1])))) : 0.0f;
    constexpr int HALO = KS / 2;
    constexpr int TR = NF * WN;              // output rows per block
    // ST = 2: stride-2 convolution (the encoders' down-sampling layers).  Tiles are OUTPUT tiles;
    // the input patch is (TR-1)*ST + KS rows x 31*ST + KS columns, and the fragment of tap
    // (dy,dx) reads patch pixel (ST*row + dy, ST*col + dx): a lane stride of ST*80 B, still
    // conflict-free for ds_read_b128 (8 consecutive lanes hit 8 disjoint 4-bank groups).
    constexpr int PR = (TR - 1) * ST + KS;   // patch rows
    constexpr int PC = 31 * ST + KS;         // patch cols
    constexpr int NPP = PR * PC;             // patch pixels
    // CK = k16 steps per tap and chunk: a chunk is 16*CK input channels.  CK = 1 halves the LDS
    // stage, which lets the 64-channel layers use 8-row tiles (NF = 2) at two blocks per CU.
    constexpr int PITCH = 8 * CK + 4;        // 32-bit words per pixel: 8*CK (16*CK fp16) + 4 pad
    constexpr int PLANE = NPP * PITCH;       // words per (hi or lo) plane
    constexpr int NPLANES = PASSES == 3 ? 2 : 1;   // x_lo is only needed for the w_hi*x_lo pass
    constexpr int STAGE = PLANE * NPLANES;
    constexpr int NSTEP = KS * KS * CK;      // (tap, 16-channel group) steps per chunk
    // weight-fragment ring (prefetch distance AR-1 steps).  A step of an NF=1 tile is only
    // 6 MFMAs (~80 ns): its ring is deeper so that the L2 latency of the weights stays covered.
    constexpr int AR_WANT = NF == 1 ? CONV_AR_NF1 : CONV_AR;
    constexpr int AR = (NSTEP % AR_WANT == 0) ? AR_WANT : 2;
    extern __shared__ __attribute__((aligned(16))) unsigned lds[];   // 2 * STAGE words (+ 8 dummy)

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM;
    const long HW = (long)a.H * a.W;
    const long SHW = a.src_hw;              // plane size of the sources (== HW unless they are sub-sampled)
    // Persistent block: tiles t = (block index within its problem), + (blocks of that problem), ...; the (tile, chunk)
    // pairs of a block form ONE software-pipelined stream, so that only the block's first
    // chunk is staged with its global-load latency exposed (for a 64->64 layer -- two chunks
    // per tile -- prologue + epilogue used to be 52 of 113 us).
    // tile id = (b * n_co + co block) * tiles_xy + spatial tile.
    auto decode = [&](int t, int &th0, int &tw0, int &tco, int &tb) {
        const int xy = t % a.tiles_xy, r = t / a.tiles_xy;
        tw0 = (xy % a.tiles_w) * 32;
        th0 = (xy / a.tiles_w) * TR;
        tco = (r % a.n_co) * (32 * MF * WM);
        tb = r / a.n_co;
    };
    int h0, w0, co_blk, b;            // tile being computed
    int tile = (int)blockIdx.x - blk_first;
    decode(tile, h0, w0, co_blk, b);

    // ---- staging.  Wave w stages channels 8w..8w+7 of every 32-channel chunk; its lanes walk
    // the patch pixels (pp = lane + 64*it).  The channel is wave-uniform, so a channel plane's
    // base address lives in SGPRs and the per-lane part of the address -- the pixel's byte
    // offset in a plane -- is computed once per TILE (SIT registers), not per chunk: staging
    // costs ~7 VALU instructions per value (select, clamp, 2 cvt + sub + cvt for the hi/lo
    // split, half a pack) instead of ~30.  (PMC on a 64->64 layer before this form: 18 VALU
    // instructions per MFMA, VALU port 50 % busy, MFMA pipe 22 %.)  Each lane writes its
    // pixel's 8 channels as one ds_write_b128 per plane.  Both halves take a SLICE range
    // (slice = pixel slot x channel pair) so that they can be spread over the MFMA steps of the
    // previous chunk.
    constexpr int SG = 2 * CK;                // waves along channels (8 channels each)
    constexpr int PG = WM * WN / SG;          // waves along pixels
    constexpr int SIT = (NPP + 64 * PG - 1) / (64 * PG);   // pixel slots per lane
    constexpr int NSL = SIT * 4;              // slices per chunk
    const int swave = __builtin_amdgcn_readfirstlane(wave) % SG;     // channel group this wave stages
    const int spgrp = __builtin_amdgcn_readfirstlane(wave) / SG;     // pixel group
    unsigned spix[SIT];                       // byte offset of the slot's pixel inside a channel plane
    bool sok[SIT];                            // the slot's pixel lies inside the image
    float sreg[SIT][8];
    unsigned shw[SIT][4], slw[SIT][4];        // converted (hi, lo) fp16 pairs awaiting the LDS write
    const float *sbase = nullptr;             // plane of the first channel this wave stages (wave-uniform)
    int snch = 0;                             // valid channels from there on (<= 0: all padding)
    float nmean[NRM ? 8 : 1], ninv[NRM ? 8 : 1];   // NRM: (mean, 1/std) of the 8 planes this wave stages (wave-uniform)
    auto stage_tile = [&](int th0, int tw0) {
#pragma unroll
        for (int it = 0; it < SIT; ++it) {
            const int pp = lane + 64 * (it * PG + spgrp);
            const int pr = pp / PC, pc = pp - pr * PC;
            const int ih = th0 * ST - HALO + pr, iw = tw0 * ST - HALO + pc;
            sok[it] = pp < NPP && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
            spix[it] = sok[it] ? (unsigned)((ih * a.src_w + iw) * a.src_px) * 4u : 0u;
        }
    };
    auto stage_select = [&](int tb, int chunk) {
        int s = 0, c0 = chunk * 16 * CK;
        while (s + 1 < a.nsrc && c0 >= ((a.src_ch[s] + 31) & ~31)) {
            c0 -= (a.src_ch[s] + 31) & ~31;
            ++s;
        }
        const int cb = c0 + 8 * swave;
        snch = a.src_ch[s] - cb;
        sbase = a.src[s] + (long)tb * a.src_bs[s] + (long)(snch > 0 ? cb : 0) * SHW;
        if (NRM) {
            const float *np = a.in_norm + 2 * ((long)tb * a.src_ch[0] + (snch > 0 ? cb : 0));
#pragma unroll
            for (int j = 0; j < (NRM ? 8 : 1); ++j) {
                const int jc = min(j, max(snch, 1) - 1);
                // wave-uniform values: pinned into SGPRs (the loads themselves are vector loads -- the compiler
                // cannot prove the buffer is not written by this kernel -- and would otherwise hold 16 VGPRs)
                nmean[j] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(np[2 * jc])));
                ninv[j] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(np[2 * jc + 1])));
            }
        }
    };
    auto stage_load = [&](int k0, int k1) {
#pragma unroll
        for (int k = k0; k < k1; ++k) {
            if (k >= NSL) break;
            const int it = k >> 2, q = k & 3;
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                // unconditional load from a clamped (valid) plane; padding channels and pixels
                // outside the image are zeroed when the value is converted (stage_store) -- a
                // select here would tie an s_waitcnt vmcnt(0) to every load
                const int j = 2 * q + jj;
                const int jc = min(j, max(snch, 1) - 1);                     // wave-uniform
                const char *pj = (const char *)(sbase + (long)jc * SHW);
                sreg[it][j] = *(const float *)(pj + spix[it]);
            }
        }
    };
    auto stage_store = [&](unsigned *buf, int k0, int k1) {
#pragma unroll
        for (int k = k0; k < k1; ++k) {
            if (k >= NSL) break;
            const int it = k >> 2, q = k & 3;
            float u0 = sreg[it][2 * q], u1 = sreg[it][2 * q + 1];
            if (NRM) {     // the arithmetic of instnorm_apply_kernel (norm.hip), so that the fusion is bit-identical
                u0 = dkt_relu(__fmul_rn(__fsub_rn(u0, nmean[(2 * q) % (NRM ? 8 : 1)]), ninv[(2 * q) % (NRM ? 8 : 1)]));
                u1 = dkt_relu(__fmul_rn(__fsub_rn(u1, nmean[(2 * q + 1) % (NRM ? 8 : 1)]), ninv[(2 * q + 1) % (NRM ? 8 : 1)]));
            }
            const float v0 = (2 * q < snch && sok[it]) ? u0 : 0.0f;
            const float v1 = (2 * q + 1 < snch && sok[it]) ? u1 : 0.0f;
            // range: |x * in_scale| must stay below 65520 (the fp16 hi part); beyond that -- and for
            // NaN / Inf inputs -- the result is non-finite, never a silently saturated value
            const float x0 = v0 * (DSC ? dsc_in : a.in_scale);
            const float x1 = v1 * (DSC ? dsc_in : a.in_scale);
            const _Float16 h0_ = (_Float16)x0, h1_ = (_Float16)x1;
            shw[it][q] = pack_h2(h0_, h1_);
            if (NPLANES == 2) slw[it][q] = pack_h2((_Float16)(x0 - (float)h0_), (_Float16)(x1 - (float)h1_));
            if (q == 3) {
                const int pp = lane + 64 * (it * PG + spgrp);
                unsigned *dst = pp < NPP ? buf + pp * PITCH + 4 * swave : lds + 2 * STAGE;   // surplus lanes -> dummy
                *(uint4 *)dst = make_uint4(shw[it][0], shw[it][1], shw[it][2], shw[it][3]);
                if (NPLANES == 2)
                    *(uint4 *)(dst + (pp < NPP ? PLANE : 4)) = make_uint4(slw[it][0], slw[it][1], slw[it][2], slw[it][3]);
            }
        }
    };

    f32x16 acc[MF][NF];
    auto zero_acc = [&]() {
#pragma unroll
        for (int m = 0; m < MF; ++m)
#pragma unroll
            for (int n = 0; n < NF; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.0f;
    };
    zero_acc();

    const int li = lane & 31, kg = lane >> 5;
    // weight fragment base (halves): ((tap*nch16 + ch16)*CoutPad + co)*16 + kg*8; waves past
    // the (64-padded) channel count idle on clamped weights
    auto wlane_of = [&](int tco) {
        const int cw = tco + wm * 32 * MF;
        return ((long)((cw < a.CoutPad ? cw : 0) + li)) * 16 + kg * 8;
    };
    long wl_cur = wlane_of(co_blk), wl_nxt = wl_cur;   // weight bases of the computed / the following tile
    const long wstep = (long)a.CoutPad * 16;           // one 16-channel slab
    const int nchunks = a.nch16 / CK;

    f16x8 Ahi[AR][MF], Alo[AR][MF];
    f16x8 Bhi[2][NF], Blo[2][NF];
    auto loadA = [&](int slot, long wlane, int chunk, int step) {
        const int tap = step / CK, kh = step % CK;
        const long wbase = ((long)tap * a.nch16 + (chunk * CK + kh)) * wstep + wlane;
#pragma unroll
        for (int m = 0; m < MF; ++m) {
            Ahi[slot][m] = *(const f16x8 *)(a.whi + wbase + m * 32 * 16);
            if (PASSES >= 2) Alo[slot][m] = *(const f16x8 *)(a.wlo + wbase + m * 32 * 16);
        }
    };
    auto loadB = [&](int slot, const unsigned *buf, int step) {
        const int tap = step / CK, kh = step % CK;
        const int dy = tap / KS, dx = tap % KS;
#pragma unroll
        for (int n = 0; n < NF; ++n) {
            const int pp = ((wn * NF + n) * ST + dy) * PC + li * ST + dx;
            const unsigned *pb = buf + pp * PITCH + kh * 8 + kg * 4;
            Bhi[slot][n] = *(const f16x8 *)pb;
            if (NPLANES == 2) Blo[slot][n] = *(const f16x8 *)(pb + PLANE);
        }
    };
    // Pass-major order: every accumulator is touched once per pass, so two MFMAs on the
    // same accumulator are 2*NF issues apart.  (Pass-minor order interleaves two
    // dependent chains one MFMA apart: measured 41 % issue-stall, MFMA pipe 46 % busy.)
    auto mma = [&](int as, int bs) {
#pragma unroll
        for (int n = 0; n < NF; ++n)
#pragma unroll
            for (int m = 0; m < MF; ++m)
                acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ahi[as][m], Bhi[bs][n], acc[m][n], 0, 0, 0);
        if (PASSES >= 2) {
#pragma unroll
            for (int n = 0; n < NF; ++n)
#pragma unroll
                for (int m = 0; m < MF; ++m)
                    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Alo[as][m], Bhi[bs][n], acc[m][n], 0, 0, 0);
        }
        if (PASSES == 3) {
#pragma unroll
            for (int n = 0; n < NF; ++n)
#pragma unroll
                for (int m = 0; m < MF; ++m)
                    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ahi[as][m], Blo[bs][n], acc[m][n], 0, 0, 0);
        }
    };

    // One wave per SIMD issues in order, so MFMA time and everything else ADD unless the
    // other instructions sit between MFMAs in program order (measured on the 384->256
    // layer: MFMAs alone 237 us, data movement alone 122 us, serial form 392 us).  Each
    // (tap, k16) step therefore carries, besides its 8*NF*PASSES MFMAs: the weight loads of
    // step s+AR-1, the LDS fragment reads of step s+1 and one slice of the NEXT chunk's
    // staging (fp32 loads in the first half of the steps, convert + LDS writes in the
    // second half); a sched_group_barrier pattern asks for ~1 memory op + 3 VALU per MFMA.
    // Idle waves (co >= CoutPad) run the same stream on clamped weights and store nothing:
    // a wave-uniform branch here would split the scheduling region.
    // ARGUMENTS: `a` lives in the kernel-argument segment, so every `a.field` is a scalar load, and with the scalar registers
    // this kernel has left the compiler re-issued that load (and drained lgkmcnt for it) at each use: once per stored value.
    // Behind the tile's last MFMA nothing of this wave hides those round trips, so the epilogue reads what it needs ONCE per
    // tile into locals that conv_hold() makes opaque, decides the wave-uniform switches once (one dispatch to bodies
    // specialised at compile time: kind, z or r half, statistics, FAST) and addresses every tensor as wave-uniform base + one
    // lane offset per row.  FAST = the wave's 32 MF channels all exist (no channel guard) and its 32 MF planes span less than
    // 2^31 bytes (the lane offset fits 32 bits: scalar base + 32-bit vector offset, the base of each value advanced on the
    // scalar ALU); every other tile keeps the per-value guard and 64-bit lane offsets.
    auto epilogue = [&]() __attribute__((always_inline)) {
        // ---- epilogue: un-scale, bias, optional ReLU, NCHW stores (128-byte rows) ----
        const int co_w = conv_hold(co_blk + wm * 32 * MF);         // this wave's first output channel
        // (ONE statement holds the batch: its scalar loads are issued back to back behind one wait; a statement per field
        // would be a load, a wait and the statement, field after field)
        auto sgpr = [](auto x) { return __builtin_amdgcn_readfirstlane((unsigned)x); };    // (a no-op on what is scalar already)
        unsigned epi_u = sgpr(a.epi), Cout_u = sgpr(a.Cout), relu_f = sgpr(a.relu), oh_ = sgpr(a.Ho), ow_ = sgpr(a.Wo), ih_ = sgpr(a.H), iw_ = sgpr(a.W);
        unsigned want_stats = sgpr(!DSC && a.stats_ws != nullptr ? 1 : 0), CoutPad_u = sgpr(a.CoutPad);
        unsigned osc_u = sgpr(__float_as_uint(DSC ? dsc_out : a.out_scale));
        unsigned bias_lo = sgpr((unsigned long long)a.bias), bias_hi = sgpr((unsigned long long)a.bias >> 32);
        asm volatile("" : "+s"(epi_u), "+s"(Cout_u), "+s"(relu_f), "+s"(oh_), "+s"(ow_), "+s"(ih_), "+s"(iw_), "+s"(want_stats),
                          "+s"(CoutPad_u), "+s"(osc_u), "+s"(bias_lo), "+s"(bias_hi));
        const float osc = __uint_as_float(osc_u);
        const int epi = (int)epi_u, Cout = (int)Cout_u;
        if (co_w >= (int)CoutPad_u) return;                        // idle wave
        const float *const bias_p = (const float *)(__attribute__((address_space(1))) const float *)(((unsigned long long)bias_hi << 32) | bias_lo);
        // the plane of the epilogue's tensors: the output's (kind 0; == H x W at stride 1), H x W for the gate kinds
        const int PH = (int)(epi == 0 ? oh_ : ih_), PW = (int)(epi == 0 ? ow_ : iw_);
        const int plane = conv_hold(PH * PW);
        const int bi = conv_hold(b), row0 = conv_hold(h0 + wn * NF);
        const int ow = w0 + li;
        const bool relu = relu_f != 0;
        // this lane's 32 output channels: co = co_lane + m*32 + (r&3) + 8*(r>>2); their biases
        // are fetched as one batch of independent loads (clamped index, no per-element branch)
        const int co_lane = co_w + 4 * kg;
        float bv[MF][16];
        if (bias_p) {
#pragma unroll
            for (int m = 0; m < MF; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = co_lane + m * 32 + (r & 3) + 8 * (r >> 2);
                    bv[m][r] = bias_p[co < Cout ? co : Cout - 1];
                }
        } else {
#pragma unroll
            for (int m = 0; m < MF; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) bv[m][r] = 0.0f;
        }
        // The biases land HERE, once, and reach the stores below as values no load is pending on.  Left to the compiler, every
        // use of a bias behind a guarded store got a drained wait of its own (it cannot count the stores a masked block issued):
        // in the plain epilogue each of a row's 16 MF stores was waited on before the next one was issued.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int m = 0; m < MF; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(bv[m][r]));
        const bool all_co = co_w + 32 * MF <= Cout;              // wave-uniform: no channel guard needed
        const bool fast = all_co && (long)plane * (32 * MF * 4) < (1L << 31);
        // the value (m, n, r) of this lane: un-scaled, biased, ReLU as a select on the held flag.  The statistics recompute
        // their values from the accumulators with a scale of their own (the same number, opaque): were the two passes to share
        // the values, 16 MF NF of them would be kept beside the accumulators across the row masks (measured: the 1x1 forms went
        // from 159 to 233 registers, three blocks per CU to two).
        auto value = [&](int m, int n, int r, float scale) {
            const float v = acc[m][n][r] * scale + bv[m][r];
            return (relu && v < 0.0f) ? 0.0f : v;
        };
        // address of channel dco (relative to the wave's first) of a tensor whose plane of the wave's first channel is p;
        // the lane adds loff bytes: its channel half, row and column
        auto at = [&](auto kFast, const float *p, int dco, auto loff) __attribute__((always_inline)) -> float * {
            return (float *)(conv_base((const char *)p + (long)dco * plane * 4) + loff);
        };
        // ---- kind 0: plain stores
        auto body_plain = [&](auto kFast) __attribute__((always_inline)) {
            constexpr bool FAST = decltype(kFast)::value != 0;
            using OT = std::conditional_t<FAST, unsigned, long>;
            float *const ob = conv_hold(a.out + (long)bi * a.out_bs + (long)co_w * plane);
            const OT kgo = (OT)(4 * kg) * (OT)plane;
#pragma unroll
            for (int n = 0; n < NF; ++n) {
                const int oh = row0 + n;
                if (oh >= PH || ow >= PW) continue;
                const OT loff = (kgo + (OT)oh * (OT)PW + (OT)ow) * 4;
#pragma unroll
                for (int m = 0; m < MF; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int dco = m * 32 + (r & 3) + 8 * (r >> 2);
                        const float v = value(m, n, r, osc);
                        if (FAST || co_lane + dco < Cout) *at(kFast, ob, dco, loff) = v;
                        if (!FAST && (r & 3) == 3) __builtin_amdgcn_sched_barrier(0);     // (no row's worth of 64-bit addresses formed ahead)
                    }
            }
        };
        // ---- kind 0: the statistics of the values just stored
        auto body_stats = [&]() __attribute__((always_inline)) {
            const float osc_s = conv_hold(osc);
            const long e = (long)((h0 / (NF * WN)) * a.tiles_w + w0 / 32) * WN + wn;
            // (the statistics rows of this wave's first channel; a lane adds the channel it ends up holding)
            float *const sws = conv_hold(a.stats_ws + (((long)bi * a.tiles_xy * WN + e) * Cout + co_w) * 2);
            // sums / sums of squares of the values just stored: per lane over its NF pixels, then a reduce-scatter over the
            // 32 pixel lanes of the half-wave (31 exchanges per statistic instead of 160): lane li ends with value index li.
            // Channel blocks go in groups of two (32 values per lane) and, for an odd MF, a last single one (16 values: the
            // first exchange only adds, lane li & 15 ends with value li & 15).
            auto stats_group = [&](const int m0, const int nm) {
                float s1[32], s2[32];
#pragma unroll
                for (int i = 0; i < 32; ++i) s1[i] = s2[i] = 0.0f;
#pragma unroll
                for (int n = 0; n < NF; ++n) {
                    const bool ok = row0 + n < PH && ow < PW;
#pragma unroll
                    for (int mm = 0; mm < nm; ++mm)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float v = ok ? value(m0 + mm, n, r, osc_s) : 0.0f;
                            s1[mm * 16 + r] = __fadd_rn(s1[mm * 16 + r], v);
                            s2[mm * 16 + r] = __fadd_rn(s2[mm * 16 + r], __fmul_rn(v, v));
                        }
                }
                if (nm == 1) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        s1[i] = __fadd_rn(s1[i], __shfl_xor(s1[i], 16, 32));
                        s2[i] = __fadd_rn(s2[i], __shfl_xor(s2[i], 16, 32));
                    }
                }
#pragma unroll
                for (int d = 16; d >= 1; d >>= 1) {
                    if (nm == 1 && d == 16) continue;
                    const bool up = (li & d) != 0;
#pragma unroll
                    for (int j = 0; j < d; ++j) {
                        const float k1 = up ? s1[j + d] : s1[j], g1 = up ? s1[j] : s1[j + d];
                        const float k2 = up ? s2[j + d] : s2[j], g2 = up ? s2[j] : s2[j + d];
                        s1[j] = __fadd_rn(k1, __shfl_xor(g1, d, 32));
                        s2[j] = __fadd_rn(k2, __shfl_xor(g2, d, 32));
                    }
                }
                const int vi = nm == 1 ? (li & 15) : li;                 // value index this lane holds
                const int dco = (m0 + (vi >> 4)) * 32 + (vi & 3) + 8 * ((vi & 15) >> 2);
                const int co = co_lane + dco;
                if (co < Cout && (nm == 2 || li < 16)) {
                    float *p = sws + (4 * kg + dco) * 2;
                    p[0] = s1[0];
                    p[1] = s2[0];
                }
            };
#pragma unroll
            for (int m0 = 0; m0 + 1 < MF; m0 += 2) stats_group(m0, 2);
            if (MF & 1) stats_group(MF - 1, 1);
        };
        // ---- fused GRU gates (gru_gates.hip arithmetic with hardware exp/rcp) ----
        // EPI: kind 1 (merged z|r), 2 (q), 3 (residual join); RPART (kind 1): this wave owns r channels
        auto body_gate = [&](auto kEpi, auto kRpart, auto kFast) __attribute__((always_inline)) {
            constexpr int EPI = decltype(kEpi)::value;
            constexpr bool RPART = decltype(kRpart)::value != 0, FAST = decltype(kFast)::value != 0;
            constexpr bool LOAD_H = EPI == 2 || RPART, LOAD_Z = EPI == 2;
            using OT = std::conditional_t<FAST, unsigned, long>;
            const int Ch = EPI == 1 ? Cout / 2 : Cout;
            const long cb = (long)(co_w - (RPART ? Ch : 0)) * plane;      // the wave's first channel inside the Ch-wide gate tensors
            const float *pc = (RPART ? a.e_c1 + (long)bi * a.e_c1_bs : a.e_c0 + (long)bi * a.e_c0_bs) + cb;
            const float *pz = LOAD_Z ? a.e_c1 + (long)bi * a.e_c1_bs + cb : pc;
            const float *ph = LOAD_H ? a.e_h + (long)bi * a.e_h_bs + cb : pc;
            float *po = (RPART ? a.out2 + (long)bi * a.out2_bs : a.out + (long)bi * a.out_bs) + cb;
            conv_hold4(pc, pz, ph, po);
            const OT kgo = (OT)(4 * kg) * (OT)plane;
#pragma unroll
            for (int n = 0; n < NF; ++n) {
                const int oh = row0 + n;
                if (oh >= PH || ow >= PW) continue;
                const OT loff = (kgo + (OT)oh * (OT)PW + (OT)ow) * 4;
#pragma unroll
                for (int mh = 0; mh < 2 * MF; ++mh) {
                    // the gate operands of 8 channels are fetched as one batch BEFORE any store (hout
                    // may alias h, so the compiler cannot hoist the loads over stores itself); batches
                    // of 8 rather than 16 keep the kernel inside the 256-VGPR budget of two blocks/CU
                    const int m = mh >> 1, r0 = (mh & 1) * 8;
                    float gc[8], gh[8], gz[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int r = r0 + i;
                        const int dco = m * 32 + (r & 3) + 8 * (r >> 2);
                        if constexpr (FAST) {
                            gc[i] = *at(kFast, pc, dco, loff);
                            gh[i] = LOAD_H ? *at(kFast, ph, dco, loff) : 0.0f;
                            gz[i] = LOAD_Z ? *at(kFast, pz, dco, loff) : 0.0f;
                        } else {
                            // (a channel past the last one reads the lane's first channel: a valid address, the value unused)
                            const long o = (co_lane + dco < Cout ? (long)conv_base((const char *)nullptr + (long)dco * plane * 4) : 0L) + loff;
                            gc[i] = *(const float *)((const char *)pc + o);
                            gh[i] = LOAD_H ? *(const float *)((const char *)ph + o) : 0.0f;
                            gz[i] = LOAD_Z ? *(const float *)((const char *)pz + o) : 0.0f;
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int r = r0 + i;
                        const int dco = m * 32 + (r & 3) + 8 * (r >> 2);
                        if (!(FAST || co_lane + dco < Cout)) continue;
                        float *const o = at(kFast, po, dco, loff);
                        const float v = acc[m][n][r] * osc + bv[m][r];
                        if constexpr (EPI == 1) {
                            const float g = conv_sigmoid(__fadd_rn(v, gc[i]));
                            *o = RPART ? __fmul_rn(g, gh[i]) : g;
                        } else if constexpr (EPI == 3) {
                            *o = dkt_relu(__fadd_rn(gc[i], (relu && v < 0.0f) ? 0.0f : v));
                        } else {
                            const float q = conv_tanh(__fadd_rn(v, gc[i]));
                            *o = __fadd_rn(__fmul_rn(__fsub_rn(1.0f, gz[i]), gh[i]), __fmul_rn(gz[i], q));
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);           // one operand batch at a time (see above: the register budget)
                }
            }
        };
        // ---- one dispatch per tile.  What no host path launches is not instantiated: the gate kinds need stride 1 and host
        // scales (conv_fill refuses them at stride 2 and beside `dscale`), kinds 1 and 2 no input norm (conv_tile_select),
        // and conv_fill refuses statistics beside `dscale`.
        if (epi == 0) {
            const bool stats = want_stats != 0;
            if (fast) body_plain(ConvTag<1>{});
            else body_plain(ConvTag<0>{});
            if constexpr (!DSC) {
                if (stats) body_stats();
            }
            return;
        }
        if constexpr (ST == 1 && !DSC) {
            if (epi == 3) {
                if (fast) body_gate(ConvTag<3>{}, ConvTag<0>{}, ConvTag<1>{});
                else body_gate(ConvTag<3>{}, ConvTag<0>{}, ConvTag<0>{});
                return;
            }
            if constexpr (!NRM) {
                if (epi == 2) {
                    if (fast) body_gate(ConvTag<2>{}, ConvTag<0>{}, ConvTag<1>{});
                    else body_gate(ConvTag<2>{}, ConvTag<0>{}, ConvTag<0>{});
                } else if (co_w >= Cout / 2) {                  // kind 1, the r half
                    if (fast) body_gate(ConvTag<1>{}, ConvTag<1>{}, ConvTag<1>{});
                    else body_gate(ConvTag<1>{}, ConvTag<1>{}, ConvTag<0>{});
                } else {
                    if (fast) body_gate(ConvTag<1>{}, ConvTag<0>{}, ConvTag<1>{});
                    else body_gate(ConvTag<1>{}, ConvTag<0>{}, ConvTag<0>{});
                }
            }
        }
    };

    constexpr int HALF = NSTEP / 2;
    constexpr int PER = (NSL + HALF - 1) / HALF;
    constexpr int NMMA = MF * NF * PASSES;
    stage_tile(h0, w0);
    stage_select(b, 0);
    stage_load(0, NSL);
    stage_store(lds, 0, NSL);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < AR - 1; ++s) loadA(s, wl_cur, 0, s);
    loadB(0, lds, 0);
    int g = 0;                               // chunks consumed by this block: LDS buffer parity
    for (;;) {
        const int tn = tile + blk_count;
        const bool have_next = tn < a.total_tiles;
        int nh0 = h0, nw0 = w0, nco = co_blk, nb = b;
        if (have_next) decode(tn, nh0, nw0, nco, nb);
        wl_nxt = wlane_of(nco);
        for (int c = 0; c < nchunks; ++c, ++g) {
            const bool in_tile = c + 1 < nchunks;
            const bool more = in_tile || have_next;
            const unsigned *cur = lds + (g & 1) * STAGE;
            unsigned *nxt = lds + ((g + 1) & 1) * STAGE;
            // what this chunk's steps stage and prefetch: the tile's next chunk, else the next
            // tile's first chunk, else (the block's very last chunk) itself again, harmlessly,
            // into the idle buffer
            const int c_f = in_tile ? c + 1 : (have_next ? 0 : c);
            const long wl_f = in_tile ? wl_cur : wl_nxt;
            if (in_tile || !have_next) stage_select(b, c_f);
            else {
                stage_select(nb, 0);
                stage_tile(nh0, nw0);
            }
#pragma unroll
            for (int s = 0; s < NSTEP; ++s) {
                // weights for step s+AR-1 (possibly the following chunk's first steps)
                const int sa = s + AR - 1;
                if (sa < NSTEP) loadA(sa % AR, wl_cur, c, sa);
                else loadA(sa % AR, wl_f, c_f, sa - NSTEP);
                if (s + 1 < NSTEP) loadB((s + 1) & 1, cur, s + 1);
                if (s < HALF) stage_load(s * PER, (s + 1) * PER);
                else stage_store(nxt, (s - HALF) * PER, (s - HALF + 1) * PER);
                mma(s % AR, s & 1);
#pragma unroll
                for (int i = 0; i < NMMA / CONV_SGB_MFMA; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, CONV_SGB_MFMA, 0);   // MFMA
                    __builtin_amdgcn_sched_group_barrier(0x320, CONV_SGB_MEM, 0);    // VMEM read / DS read / DS write
                    __builtin_amdgcn_sched_group_barrier(0x002, CONV_SGB_VALU, 0);   // VALU
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();
            if (more) loadB(0, nxt, 0);      // step 0 always uses B slot 0
        }
        epilogue();
        if (!have_next) break;
        tile = tn; h0 = nh0; w0 = nw0; co_blk = nco; b = nb;
        wl_cur = wl_nxt;
        zero_acc();
    }
}

// ---------------------------------------------------------------------------
// Weight pre-pack: (Cout, Cin, KH, KW) fp32 -> hi/lo fp16, [tap][ci16][coPad][16],
// with the input-channel axis re-chunked to match the per-source 32-channel
// padding of the activation operands.  One thread per packed element.
// ---------------------------------------------------------------------------
#if !defined(CONV_TU_PASSES) || CONV_TU_PASSES == 0
struct PackArgs {
    const float *w;
    _Float16 *whi, *wlo;
    int Cout, Cin, taps, CoutPad, nch16;
    int src_ch[CONV_MAX_SRC];
    int nsrc;
    float scale;
};

__global__ __launch_bounds__(256) void conv2d_pack_kernel(PackArgs a) {
    const long total = (long)a.taps * a.nch16 * a.CoutPad * 16;
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= total) return;
    const int k = (int)(i % 16);
    const int co = (int)((i / 16) % a.CoutPad);
    const int c16 = (int)((i / (16L * a.CoutPad)) % a.nch16);
    const int tap = (int)(i / (16L * a.CoutPad * a.nch16));
    // padded channel index -> (source, channel in source) -> original input channel
    int pc = c16 * 16 + k, s = 0, cbase = 0;
    while (s + 1 < a.nsrc && pc >= ((a.src_ch[s] + 31) & ~31)) {
        pc -= (a.src_ch[s] + 31) & ~31;
        cbase += a.src_ch[s];
        ++s;
    }
    float v = 0.0f;
    if (co < a.Cout && pc < a.src_ch[s]) v = a.w[((long)co * a.Cin + cbase + pc) * a.taps + tap] * a.scale;
    const _Float16 hi = (_Float16)v;
    a.whi[i] = hi;
    a.wlo[i] = (_Float16)(v - (float)hi);
}

// output channels are owned 64 per wave; the packed image is padded to that granule
#endif  // CONV_TU_PASSES == 0

static int conv_cout_pad(int Cout) { return (Cout + 63) & ~63; }

static int conv_padded_channels(const int *src_ch, int nsrc) {
    int t = 0;
    for (int s = 0; s < nsrc; ++s) t += (src_ch[s] + 31) & ~31;
    return t;
}

#if !defined(CONV_TU_PASSES) || CONV_TU_PASSES == 0
extern "C" long dkt_conv2d_packed_elems(const int *src_channels, int nsrc, int Cout, int KH, int KW) {
    if (!src_channels || nsrc < 1 || nsrc > CONV_MAX_SRC || Cout <= 0 || KH <= 0 || KW <= 0) return DKT_E_SHAPE;
    return (long)KH * KW * (conv_padded_channels(src_channels, nsrc) / 16) * conv_cout_pad(Cout) * 16;
}

extern "C" int dkt_conv2d_pack_weights(const float *w, const int *src_channels, int nsrc,
                                       int Cout, int KH, int KW, float scale,
                                       void *w_hi, void *w_lo, int device, void *stream) {
    if (!w || !src_channels || !w_hi || !w_lo) return DKT_E_NULL;
    if (nsrc < 1 || nsrc > CONV_MAX_SRC || Cout <= 0 || KH <= 0 || KW != KH || !(scale > 0.0f)) return DKT_E_SHAPE;
    PackArgs a;
    a.w = w;
    a.whi = (_Float16 *)w_hi;
    a.wlo = (_Float16 *)w_lo;
    a.Cout = Cout;
    a.Cin = 0;
    for (int s = 0; s < CONV_MAX_SRC; ++s) {
        a.src_ch[s] = s < nsrc ? src_channels[s] : 0;
        if (s < nsrc && src_channels[s] <= 0) return DKT_E_SHAPE;
        a.Cin += a.src_ch[s];
    }
    a.nsrc = nsrc;
    a.taps = KH * KW;
    a.CoutPad = conv_cout_pad(Cout);
    a.nch16 = conv_padded_channels(src_channels, nsrc) / 16;
    a.scale = scale;
    DKT_ENTER(device);
    const long total = (long)a.taps * a.nch16 * a.CoutPad * 16;
    hipLaunchKernelGGL(conv2d_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, a);
    return dkt_launch_status();
}

#endif  // CONV_TU_PASSES == 0 (weight packer)

// Resident blocks the device holds of one instantiation (occupancy x CUs), cached per device.
static int conv_slots(const void *kern, size_t lds, int dev, int threads) {
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, lds) != hipSuccess || per_cu < 1) per_cu = 1;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    return per_cu * cus;
}

// A second, independent convolution that shares the launch (see the kernel's head comment).
struct ConvSecond {
    ConvArgs a;
    int B;
};

template <int KS, int WM, int WN, int NF, int PASSES, int MF = 2, int ST = 1, int CK = 2, int NRM = 0, int DSC = 0>
static int launch_conv(ConvArgs a, int B, hipStream_t st, const ConvSecond *sec = nullptr) {
    constexpr int NPP = ((NF * WN - 1) * ST + KS) * (31 * ST + KS);
    constexpr int STAGE = NPP * (8 * CK + 4) * (PASSES == 3 ? 2 : 1);
    const size_t lds = ((size_t)2 * STAGE + 8) * sizeof(unsigned);   // + dummy words for surplus staging lanes
    auto kern = conv2d_f16s_kernel<KS, WM, WN, NF, PASSES, MF, ST, CK, NRM, DSC>;
    // once per device and instantiation (and never inside a stream capture after warm-up)
    static int slots[64] = {0};                        // benign race: worst case computed twice
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (!slots[dev & 63]) {
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return (int)e;
        }
        slots[dev & 63] = conv_slots((const void *)kern, lds, dev, 64 * WM * WN);
    }
    const int tiles_h = (a.Ho + NF * WN - 1) / (NF * WN);
    a.tiles_xy = a.tiles_w * tiles_h;
    a.n_co = (a.Cout + 32 * MF * WM - 1) / (32 * MF * WM);
    const long total = (long)a.tiles_xy * a.n_co * B;
    if (total > 0x7fffffffL) return DKT_E_SHAPE;
    a.total_tiles = (int)total;
    const long cap = slots[dev & 63];
    if (!sec) {
        const long nblk = total > cap ? cap : total;       // blocks stream their tiles (cross-tile pipelining)
        ConvArgsPair ap;
        ap.p[0] = a;
        ap.p[1] = a;
        hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(64 * WM * WN), lds, st, ap, (int)nblk);
        int rc = dkt_launch_status();
        if (rc == DKT_OK && a.stats_ws)
            rc = conv_stats_reduce(a.stats_ws, a.stats_part, B, a.Cout, (long)a.tiles_xy * WN, (long)a.Ho * a.Wo, a.out, a.out_bs, st);
        return rc;
    }
    if (a.stats_ws || sec->a.stats_ws) return DKT_E_UNSUPPORTED;
    // ---- two problems: resident blocks are split in proportion to the work (tiles x chunks)
    ConvArgs b = sec->a;
    b.tiles_xy = b.tiles_w * ((b.Ho + NF * WN - 1) / (NF * WN));
    b.n_co = (b.Cout + 32 * MF * WM - 1) / (32 * MF * WM);
    const long total1 = (long)b.tiles_xy * b.n_co * sec->B;
    if (total1 > 0x7fffffffL) return DKT_E_SHAPE;
    b.total_tiles = (int)total1;
    long nb0 = total, nb1 = total1;
    if (total + total1 > cap) {
        const double w0 = (double)total * a.nch16, w1 = (double)total1 * b.nch16;
        nb1 = (long)(cap * w1 / (w0 + w1) + 0.5);
        nb1 = nb1 < 1 ? 1 : (nb1 > total1 ? total1 : nb1);
        nb0 = cap - nb1;
        if (nb0 > total) nb0 = total;
        if (nb0 < 1) nb0 = 1;
    }
    ConvArgsPair ap;
    ap.p[0] = a;
    ap.p[1] = b;
    hipLaunchKernelGGL(kern, dim3((unsigned)(nb0 + nb1)), dim3(64 * WM * WN), lds, st, ap, (int)nb0);
    return dkt_launch_status();
}

#if !defined(CONV_TU_PASSES) || CONV_TU_PASSES == 3
#include "conv_ws.h"      // weights-stationary kernel of the 64 -> 64 layers (three-pass form only)
#define CONV_HAVE_WS 1
#endif

// The launch of a tile conv_tile_select() chose, for one (filter size, pass count, NRM, DSC): the rows of CONV_TILE_TABLE
// that exist for it, and only those, are instantiated.
template <int KS, int PASSES, int NRM, int DSC>
static int launch_conv_tile(const ConvTile &t, const ConvArgs &a, int B, hipStream_t st, const ConvSecond *sec) {
#define CONV_TILE_CASE(WM_, WN_, NF_, MF_, ST_, CK_, K1_, NRM_, DSC_, PAIR_, P3_)                                            \
    if constexpr ((KS == 3 || (K1_)) && (!NRM || (NRM_)) && (!DSC || (DSC_)) && (PASSES == 3 || !(P3_))) {                  \
        if (t.WM == WM_ && t.WN == WN_ && t.NF == NF_ && t.MF == MF_ && t.ST == ST_ && t.CK == CK_ && (!sec || (PAIR_)))    \
            return launch_conv<KS, WM_, WN_, NF_, PASSES, MF_, ST_, CK_, NRM, DSC>(a, B, st, sec);                          \
    }
    CONV_TILE_TABLE(CONV_TILE_CASE)
#undef CONV_TILE_CASE
    return DKT_E_UNSUPPORTED;
}

// The kernel instantiations are split by number of MFMA passes so that the build can compile them as parallel translation
// units (dkt_stereo_amd/build.py: -DCONV_TU_PASSES=1|2|3, =4|5|6 the device-scaled instantiations of 1|2|3 passes, each
// unit one specialisation of conv2d_launch_passes; =0 holds the tile selection, the ABI and the weight packer).  Compiled
// without the macro this file is one complete translation unit.
template <int PASSES, int DSC>
int conv2d_launch_passes(const ConvTile &t, const ConvArgs &a, int B, hipStream_t st, const ConvSecond *sec);
#if !defined(CONV_TU_PASSES) || CONV_TU_PASSES != 0
template <int PASSES, int DSC>
int conv2d_launch_passes(const ConvTile &t, const ConvArgs &a, int B, hipStream_t st, const ConvSecond *sec) {
#ifdef CONV_HAVE_WS
    if constexpr (PASSES == 3 && !DSC) {
        if (t.kernel == CONV_KERNEL_WS) return launch_conv_ws(a, B, st);
    }
#endif
    if (t.KS == 1) return launch_conv_tile<1, PASSES, 0, DSC>(t, a, B, st, sec);
    if constexpr (!DSC) {
        if (a.in_norm) return launch_conv_tile<3, PASSES, 1, 0>(t, a, B, st, sec);
    }
    return launch_conv_tile<3, PASSES, 0, DSC>(t, a, B, st, sec);
}
#endif
#if defined(CONV_TU_PASSES) && CONV_TU_PASSES != 0
template int conv2d_launch_passes<(CONV_TU_PASSES - 1) % 3 + 1, (CONV_TU_PASSES > 3)>(const ConvTile &, const ConvArgs &, int, hipStream_t,
                                                                                     const ConvSecond *);
#endif

#if !defined(CONV_TU_PASSES) || CONV_TU_PASSES == 0
// The one validator of the launch entries: checks a descriptor and fills its kernel argument block.
static int conv_fill(ConvArgs &a, const dkt_conv_desc *d, int passes) {
    if (!d) return DKT_E_NULL;
    if (d->epilogue < 0 || d->epilogue > 3) return DKT_E_UNSUPPORTED;
    if (d->epilogue == 1) {
        if (!d->e0 || !d->e1 || !d->h || !d->out2) return DKT_E_NULL;
        if (d->Cout % 128 != 0) return DKT_E_UNSUPPORTED;          // Ch multiple of 64: z and r never share a wave
    } else if (d->epilogue == 2) {
        if (!d->e0 || !d->e1 || !d->h) return DKT_E_NULL;
    } else if (d->epilogue == 3) {
        if (!d->e0) return DKT_E_NULL;
    }
    if (d->stride != 0 && d->stride != 1 && d->stride != 2) return DKT_E_UNSUPPORTED;
    const int stride = d->stride == 2 ? 2 : 1;
    // device-resident scales: the plain stride-1 layer alone (the pair sits in the slot of in_norm)
    if (d->dscale && (d->bias || d->relu || d->epilogue || d->in_norm || d->stats_ws || d->stats_part || stride == 2))
        return DKT_E_UNSUPPORTED;
    if (!d->w_hi || !d->w_lo || !d->out) return DKT_E_NULL;
    const int rc = conv_query_check(stride, d->epilogue, d->nsrc, d->B, d->H, d->W, d->Cout, d->KH, d->KW, passes);
    if (rc != DKT_OK) return rc;
    if (!(d->in_scale > 0.0f) || !(d->out_scale > 0.0f)) return DKT_E_SHAPE;
    for (int s = 0; s < CONV_MAX_SRC; ++s) {
        a.src[s] = s < d->nsrc ? d->src[s] : nullptr;
        a.src_bs[s] = s < d->nsrc ? d->src_bstride[s] : 0;
        a.src_ch[s] = s < d->nsrc ? d->src_channels[s] : 0;
        if (s < d->nsrc && (!d->src[s] || d->src_channels[s] <= 0)) return DKT_E_NULL;
    }
    a.nsrc = d->nsrc;
    a.whi = (const _Float16 *)d->w_hi;
    a.wlo = (const _Float16 *)d->w_lo;
    a.bias = d->bias;
    a.out_scale = d->out_scale;
    a.in_scale = d->in_scale;
    a.out = d->out;
    a.out_bs = d->out_bstride;
    a.H = d->H; a.W = d->W; a.Cout = d->Cout;
    // "same"-style padding KH/2 (what every layer on the path uses): output = floor((H - 1) / stride) + 1
    a.Ho = (d->H - 1) / stride + 1;
    a.Wo = (d->W - 1) / stride + 1;
    a.CoutPad = conv_cout_pad(d->Cout);
    a.nch16 = conv_padded_channels(d->src_channels, d->nsrc) / 16;
    a.tiles_w = (a.Wo + 31) / 32;
    a.tiles_xy = a.n_co = a.total_tiles = 0;       // set by launch_conv (they depend on the tile shape)
    a.relu = d->relu ? 1 : 0;
    a.epi = d->epilogue;
    a.e_c0 = a.e_c1 = a.e_h = nullptr;
    a.e_c0_bs = a.e_c1_bs = a.e_h_bs = 0;
    a.out2 = nullptr;
    a.out2_bs = 0;
    if (d->epilogue) {
        a.e_c0 = d->e0; a.e_c1 = d->e1; a.e_h = d->h;
        a.e_c0_bs = d->e0_bstride; a.e_c1_bs = d->e1_bstride; a.e_h_bs = d->h_bstride;
        a.out2 = d->out2; a.out2_bs = d->out2_bstride;
    }
    a.stats_ws = nullptr;
    a.stats_part = nullptr;
    a.stats_hw = 0;
    a.src_px = 1; a.src_w = d->W; a.src_hw = (long)d->H * d->W;
    if (d->stats_ws || d->stats_part) {
        if (!d->stats_ws || !d->stats_part) return DKT_E_NULL;
        if (d->epilogue != 0) return DKT_E_UNSUPPORTED;
        a.stats_ws = d->stats_ws;
        a.stats_part = (double *)d->stats_part;
    }
    // DSC: in_scale = dscale[0], out_scale = w_inv_scale * dscale[1], both read by the kernel; else (mean, 1/std) of the
    // in-norm form (what it supports: conv_tile_select) or nothing
    a.in_norm = d->dscale ? d->dscale : d->in_norm;
    return DKT_OK;
}

// One filled argument block (or two: sec) to its launch: the tile is chosen before the device is entered.
static int conv_run(ConvArgs &a, int B, int KH, int stride, int passes, int form, int device, void *stream,
                    const ConvSecond *sec = nullptr) {
    ConvTile t;
    const int rc = conv_tile_select({KH, stride, passes, a.Cout, a.nsrc, a.src_ch, a.epi, B, a.H, a.W, form}, &t);
    if (rc != DKT_OK) return rc;
    DKT_ENTER(device);
    if (stride == 2 && t.ST == 1) {       // the sub-sampled source of a 1x1 stride-2 layer (see ConvArgs::src_px)
        a.src_px = 2; a.src_w = a.W; a.src_hw = (long)a.H * a.W;
        a.H = a.Ho; a.W = a.Wo;
    }
    const hipStream_t st = (hipStream_t)stream;
    const bool dsc = form == CONV_FORM_DSCALE;
    if (passes == 3) return dsc ? conv2d_launch_passes<3, 1>(t, a, B, st, sec) : conv2d_launch_passes<3, 0>(t, a, B, st, sec);
    if (passes == 2) return dsc ? conv2d_launch_passes<2, 1>(t, a, B, st, sec) : conv2d_launch_passes<2, 0>(t, a, B, st, sec);
    return dsc ? conv2d_launch_passes<1, 1>(t, a, B, st, sec) : conv2d_launch_passes<1, 0>(t, a, B, st, sec);
}

extern "C" long dkt_conv2d_stats_ws_floats(int B, int Cout, int Ho, int Wo) {
    if (B <= 0 || Cout <= 0 || Ho <= 0 || Wo <= 0) return DKT_E_SHAPE;
    // One entry per (tile, wave row): tiles_w * ceil(Ho / TR) * WN per image with TR = WN * NF rows per tile, TR in {1, 2, 4, 8}
    // over the tile shapes -- waves whose rows lie past Ho write (zero) entries too, so the bound is Ho rounded UP to 8 rows per
    // 32-column strip (`Ho` entries were 9 short at Ho = 33 on the 4-row shapes)
    return (long)B * ((Wo + 31) / 32) * ((Ho + 7) / 8 * 8) * Cout * 2;
}

extern "C" int dkt_conv2d_f16s_tile(int KS, int stride, int passes, int Cout, const int *src_channels, int nsrc, int epilogue,
                                    int B, int H, int W, int form, int *tile) {
    if (!tile) return DKT_E_NULL;
    ConvTile t;
    const int rc = conv_tile_select({KS, stride, passes, Cout, nsrc, src_channels, epilogue, B, H, W, form}, &t);
    if (rc == DKT_OK) memcpy(tile, &t, sizeof t);        // eight integers, in the order of the struct
    return rc;
}

extern "C" int dkt_conv2d_f16s_desc(const dkt_conv_desc *p, int passes, int device, void *stream) {
    ConvArgs a;
    const int rc = conv_fill(a, p, passes);
    if (rc != DKT_OK) return rc;
    const int form = p->dscale ? CONV_FORM_DSCALE : p->in_norm ? CONV_FORM_NORM : CONV_FORM_SINGLE;
    return conv_run(a, p->B, p->KH, p->stride == 2 ? 2 : 1, passes, form, device, stream);
}

extern "C" int dkt_conv2d_f16s_pair(const dkt_conv_desc *p0, const dkt_conv_desc *p1, int passes, int device, void *stream) {
    ConvArgs a;
    ConvSecond sec;
    int rc = conv_fill(a, p0, passes);
    if (rc != DKT_OK) return rc;
    rc = conv_fill(sec.a, p1, passes);
    if (rc != DKT_OK) return rc;
    if (p0->in_norm || p1->in_norm || p0->dscale || p1->dscale || p0->stride == 2 || p1->stride == 2) return DKT_E_UNSUPPORTED;
    sec.B = p1->B;
    // both problems run one kernel instantiation: same filter size and the same output-width class
    if (p0->KH != p1->KH || conv_width_class(p0->Cout) != conv_width_class(p1->Cout)) return DKT_E_UNSUPPORTED;
    return conv_run(a, p0->B, p0->KH, 1, passes, CONV_FORM_PAIR, device, stream, &sec);
}
#endif  // CONV_TU_PASSES == 0 (ABI entry points)
