// conv_grad.hip -- the pre-pass of a convolution's backward (dkt_stereo_amd/conv.py: _Conv2dFn.backward).
// Reference: torch autograd through relu(conv2d(x, w, b)) (core/update.py:9-10, 19-21, 72-76, 111-113 under training):
//   g' = gy * (y > 0)            the gradient behind the ReLU
//   gb = g'.sum((0, 2, 3))       the bias gradient
// and, for this library's split-fp16 input-gradient convolution, the RANGE of g':  a power of two 2^e that puts max|g'| in
// [2^12, 2^13) -- the window the weights are packed in -- so that the convolution keeps ~22 bits of a gradient of any
// magnitude (dkt_conv2d_f16s_desc with `dscale` reads {2^e, 2^-e} from device memory; the host reads nothing back).
//
//   dkt_conv_grad_prepass   one streaming pass over gy [and y], then a one-block finish
//
// Shape of the gate kernels (gru_gates.h): float4 accesses when HW, the batch strides and the pointers allow it, 4-byte ones otherwise, a
// grid-stride loop over at most 2048 blocks of 256; every load of an item is issued before its first use.
// The order of every sum is a function of the shape alone: a (batch, channel) plane is cut into segments of PRE_SEG elements,
// a segment is one work item of one block (thread t owns the elements 4t..4t+3 of every 1024, added in ascending order; the 64
// lanes of a wave fold in a butterfly, the four waves as (w0 + w1) + (w2 + w3)), and the finish adds a channel's items in
// ascending (batch, segment).  No float atomics: the bias gradient is bit-identical from run to run, for every grid size and
// for the 16-byte and the 4-byte path alike.  The maximum is taken on the bit patterns of |g'| (an unsigned maximum orders
// finite < Inf < NaN), so a non-finite gradient is seen as such.
#include "dkt_common.h"
#include "wave_reduce.h"

#define PRE_SEG 4096          // elements per work item: 4 x float4 per thread
#define PRE_K (PRE_SEG / 1024)

struct PrepassArgs {
    const float *gy, *y;
    float *gmask;             // dense (B, C, HW); written only with y
    float *ws;                // [item][2]: partial sum, bits of the partial max|g'|
    long gy_bs, y_bs;
    long HW;
    int B, C;
    long nseg;                // segments per plane
    long items;               // C * B * nseg; item = (c * B + b) * nseg + s
};

template <int V, int MASK>
__global__ __launch_bounds__(256) void conv_grad_prepass_kernel(PrepassArgs a) {
    __shared__ float wsum[4];
    __shared__ unsigned wmax[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long item = blockIdx.x; item < a.items; item += gridDim.x) {
        const long s = item % a.nseg, cb = item / a.nseg;
        const long b = cb % a.B, c = cb / a.B;
        const long e0 = s * PRE_SEG;
        const long left = a.HW - e0;
        const int len = left < PRE_SEG ? (int)left : PRE_SEG;
        const float *pg = a.gy + b * a.gy_bs + c * a.HW + e0;
        const float *py = MASK ? a.y + b * a.y_bs + c * a.HW + e0 : nullptr;
        float *po = MASK ? a.gmask + (b * a.C + c) * a.HW + e0 : nullptr;
        float g[PRE_K][4], yv[PRE_K][4];
#pragma unroll
        for (int k = 0; k < PRE_K; ++k) {
            const int off = (k * 256 + tid) * 4;
            if (V == 4) {
                // HW % 4 == 0: a float4 is inside the segment or outside it as a whole
                const bool ok = off < len;
                const float4 t = ok ? *(const float4 *)(pg + off) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                g[k][0] = t.x; g[k][1] = t.y; g[k][2] = t.z; g[k][3] = t.w;
                if (MASK) {
                    const float4 u = ok ? *(const float4 *)(py + off) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    yv[k][0] = u.x; yv[k][1] = u.y; yv[k][2] = u.z; yv[k][3] = u.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool ok = off + j < len;
                    g[k][j] = ok ? pg[off + j] : 0.0f;
                    if (MASK) yv[k][j] = ok ? py[off + j] : 0.0f;
                }
            }
        }
        float sum = 0.0f;
        unsigned amax = 0u;
#pragma unroll
        for (int k = 0; k < PRE_K; ++k) {
            const int off = (k * 256 + tid) * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (MASK) g[k][j] = yv[k][j] > 0.0f ? g[k][j] : 0.0f;        // elements past the segment: y = 0 -> 0
                sum = __fadd_rn(sum, g[k][j]);
                const unsigned bits = __float_as_uint(g[k][j]) & 0x7fffffffu;
                amax = bits > amax ? bits : amax;
            }
            if (MASK) {
                if (V == 4) {
                    if (off < len) *(float4 *)(po + off) = make_float4(g[k][0], g[k][1], g[k][2], g[k][3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (off + j < len) po[off + j] = g[k][j];
                }
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) sum = __fadd_rn(sum, __shfl_xor(sum, d, 64));
        amax = wave_max(amax);
        if (lane == 0) {
            wsum[wave] = sum;
            wmax[wave] = amax;
        }
        __syncthreads();
        if (tid == 0) {
            const unsigned m01 = wmax[0] > wmax[1] ? wmax[0] : wmax[1], m23 = wmax[2] > wmax[3] ? wmax[2] : wmax[3];
            a.ws[2 * item] = __fadd_rn(__fadd_rn(wsum[0], wsum[1]), __fadd_rn(wsum[2], wsum[3]));
            a.ws[2 * item + 1] = __uint_as_float(m01 > m23 ? m01 : m23);
        }
        __syncthreads();                                    // wsum / wmax are reused by the block's next item
    }
}

struct PrepassFinishArgs {
    const float *ws;
    float *gb;                // may be null
    float *scale;             // {2^e, 2^-e}
    int C;
    long per_c;               // items per channel: B * nseg
};

// One block.  Thread t owns the channels t, t + 256, ...: their items in ascending order; then the maximum over everything.
__global__ __launch_bounds__(256) void conv_grad_prepass_finish_kernel(PrepassFinishArgs a) {
    __shared__ unsigned wmax[4];
    const int tid = threadIdx.x;
    unsigned amax = 0u;
    for (int c = tid; c < a.C; c += 256) {
        const float *p = a.ws + 2 * (long)c * a.per_c;
        float s = 0.0f;
#pragma unroll 4
        for (long i = 0; i < a.per_c; ++i) {
            s = __fadd_rn(s, p[2 * i]);
            const unsigned bits = __float_as_uint(p[2 * i + 1]);
            amax = bits > amax ? bits : amax;
        }
        if (a.gb) a.gb[c] = s;
    }
    amax = block_max<4>(amax, wmax);
    if (tid == 0) {
        // e = 12 - floor(log2(amax)): amax * 2^e in [2^12, 2^13); clamped to +-DKT_CONV_GRAD_MAX_EXP (a subnormal amax lands
        // on the clamp); amax == 0, Inf or NaN: e = 0 -- a non-finite gradient then reaches the convolution unscaled and
        // comes out non-finite, as the format's contract says
        int e = 0;
        if (amax != 0u && amax < 0x7f800000u) {
            e = 12 - ((int)(amax >> 23) - 127);
            e = e > DKT_CONV_GRAD_MAX_EXP ? DKT_CONV_GRAD_MAX_EXP : (e < -DKT_CONV_GRAD_MAX_EXP ? -DKT_CONV_GRAD_MAX_EXP : e);
        }
        a.scale[0] = __uint_as_float((unsigned)(127 + e) << 23);
        a.scale[1] = __uint_as_float((unsigned)(127 - e) << 23);
    }
}

static long prepass_nseg(long HW) { return (HW + PRE_SEG - 1) / PRE_SEG; }

extern "C" long dkt_conv_grad_prepass_ws_floats(int B, int C, long HW) {
    if (B <= 0 || C <= 0 || HW <= 0) return DKT_E_SHAPE;
    return 2L * B * C * prepass_nseg(HW);
}

extern "C" int dkt_conv_grad_prepass(const float *gy, long gy_bstride, const float *y, long y_bstride,
                                     float *gmask, float *gb, float *scale, float *ws,
                                     int B, int C, long HW, int device, void *stream) {
    if (!gy || !scale || !ws || (y && !gmask)) return DKT_E_NULL;
    if (B <= 0 || C <= 0 || HW <= 0) return DKT_E_SHAPE;
    if (gy_bstride < (long)C * HW || (y && y_bstride < (long)C * HW)) return DKT_E_SHAPE;
    DKT_ENTER(device);
    PrepassArgs a;
    a.gy = gy; a.y = y; a.gmask = y ? gmask : nullptr; a.ws = ws;
    a.gy_bs = gy_bstride; a.y_bs = y_bstride;
    a.HW = HW; a.B = B; a.C = C;
    a.nseg = prepass_nseg(HW);
    a.items = (long)B * C * a.nseg;
    const bool vec = (HW % 4 == 0) && (gy_bstride % 4 == 0) && dkt_aligned16(gy) &&
                     (!y || ((y_bstride % 4 == 0) && dkt_aligned16(y) && dkt_aligned16(gmask)));
    const unsigned blocks = (unsigned)(a.items < 2048 ? a.items : 2048);
    hipStream_t st = (hipStream_t)stream;
    if (y) {
        if (vec) hipLaunchKernelGGL((conv_grad_prepass_kernel<4, 1>), dim3(blocks), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((conv_grad_prepass_kernel<1, 1>), dim3(blocks), dim3(256), 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((conv_grad_prepass_kernel<4, 0>), dim3(blocks), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((conv_grad_prepass_kernel<1, 0>), dim3(blocks), dim3(256), 0, st, a);
    }
    int rc = dkt_launch_status();
    if (rc != DKT_OK) return rc;
    PrepassFinishArgs f;
    f.ws = ws; f.gb = gb; f.scale = scale; f.C = C;
    f.per_c = (long)B * a.nseg;
    hipLaunchKernelGGL(conv_grad_prepass_finish_kernel, dim3(1), dim3(256), 0, st, f);
    return dkt_launch_status();
}
