// context_upsample_train.hip -- IGEV-Stereo's context up-sampling on the training path (IGEVStereo.forward with
// test_mode=False, meta_arch/igev_stereo/igev_stereo.py:199-225: once per refinement iteration and once for init_disp):
//   dkt_context_upsample_bwd          the gradient of context_upsample (meta_arch/igev_stereo/submodule.py:242-254, torch
//                                     autograd through those lines) with respect to disp_low and up_weights; the forward is
//                                     dkt_context_upsample (upsample.hip) unchanged
//   dkt_context_upsample_logits_fwd   upsample_disp's tail (igev_stereo.py:145-147) in one pass: the softmax over the nine
//   dkt_context_upsample_logits_bwd   planes, the factor on disp and context_upsample; the backward recomputes the softmax
//                                     (nothing but disp and the logits is saved)
//
// Fine pixel (Y, X) over coarse pixel (y, x) = (Y/4, X/4); nb_k = disp[b,0,y+k/3-1,x+k%3-1] (0 outside), g = gout[b,Y,X]:
//   weights form   out = sum_k w_k nb_k;   gweights_k = g nb_k;   C_k(y,x) = sum_{i,j<4} w_k g at (4y+i, 4x+j)
//                  gdisp[b,0,y,x] = sum_k C_k(y-k/3+1, x-k%3+1)  (terms outside the image absent)
//   logits form    p_k = softmax_k(logits), v_k = scale nb_k (exact: scale is a power of two);  out = sum_k p_k v_k
//                  a_k = g v_k, s = sum_k p_k a_k, glogits_k = p_k (a_k - s);  C_k = sum_{i,j} p_k g;  gdisp = scale sum_k C_k
//
// HBM-bound: the nine-plane tensor (9 * 16 floats per coarse pixel) is read once and its gradient written once.  A block
// is four waves over 64 consecutive coarse pixels of one image (flattened y*w + x); wave i owns fine row i, and a thread
// moves the four pixels of its coarse pixel in that row -- of each plane, of gout and of the result -- as one 16-byte
// access, so a wave's access is 1 KB of one row of one plane, and all ten (or nineteen) loads of a thread are in flight
// together.  (One thread per coarse pixel walking its four rows leaves the recipe shape with 840 waves for 1024 SIMDs, each
// waiting four times for its own loads: the logits form took 17.4 us forward and 26.5 us backward there, against 11.8 and 20.9 with this mapping.)
//
// Deterministic, no atomics, one owner per element.  C_k: thread (i, y, x) adds the four products of its row in ascending
// j, the four row sums meet in LDS and one thread adds them in ascending i; the result goes to a workspace of 9 floats per
// coarse pixel (1/16 of the nine-plane tensor).  A second launch owns one gdisp element per thread and adds its (up to 9)
// in-image C terms in ascending k.  (Two launches rather than a tile with a halo, for the reasons of upsample_train.hip.)
// Plain scalar fp32 (no packed math: DESIGN 3.4).
#include <math.h>

#include "dkt_common.h"

// nb_k of one coarse pixel, in two steps: the loads, unconditional (clamped index) so that all nine are in flight together
// with the plane loads that follow, and the finish (the zero padding as a select, the factor).  As ups_taps_load /
// ups_taps_finish of upsample_train.hip: the empty asm makes each loaded value count as used where it stands.
__device__ __forceinline__ void cxu_taps_load(const float *__restrict__ dp, int y, int x, int h, int w, float (&v)[9]) {
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] = dp[(long)min(max(y + k / 3 - 1, 0), h - 1) * w + min(max(x + k % 3 - 1, 0), w - 1)];
}

__device__ __forceinline__ void cxu_taps_finish(float (&v)[9], int y, int x, int h, int w, float scale) {
#pragma unroll
    for (int k = 0; k < 9; ++k) asm volatile("" : "+v"(v[k]));
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
        v[k] = (yy >= 0 && yy < h && xx >= 0 && xx < w) ? __fmul_rn(scale, v[k]) : 0.0f;
    }
}

__device__ __forceinline__ void cxu_load4(const float *__restrict__ p, float (&v)[4]) {
    const float4 t = *reinterpret_cast<const float4 *>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
}

__device__ __forceinline__ void cxu_store4(float *__restrict__ p, const float (&v)[4]) {
    *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
}

// The softmax of convex_upsample_kernel (upsample.hip) in place, the same bits: max, expf(fl(m - max)), the sum in
// ascending k, nine IEEE divisions.  The divisions are written out as in ups_softmax (upsample_train.hip, where the
// equivalence with a / b is argued): the steps that depend on the divisor alone are done once for the nine quotients, and
// a numerator below 2^-100 other than 0 (a spread of the logits beyond 69) sends the pixel to the plain division.
__device__ __forceinline__ void cxu_softmax(float (&m)[9]) {
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < 9; ++k) mx = fmaxf(mx, m[k]);
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        m[k] = expf(__fsub_rn(m[k], mx));
        sum = __fadd_rn(sum, m[k]);
    }
    const float r0 = __builtin_amdgcn_rcpf(sum);
    const float r = __fmaf_rn(__fmaf_rn(-sum, r0, 1.0f), r0, r0);
    bool tiny = false;
#pragma unroll
    for (int k = 0; k < 9; ++k) tiny |= m[k] < 0x1p-100f && m[k] != 0.0f;
    if (__builtin_expect(tiny, 0)) {
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = __fdiv_rn(m[k], sum);
        return;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float a = m[k];
        float q = __fmul_rn(a, r);
        q = __fmaf_rn(__fmaf_rn(-sum, q, a), r, q);
        m[k] = __fmaf_rn(__fmaf_rn(-sum, q, a), r, q);
    }
}

// The row sums of C meet here: red[i][k][lane] -> ws[b, k, p], added in ascending i by one thread per (k, lane).  Every
// thread of the block comes here (no early return in front of it).
__device__ __forceinline__ void cxu_reduce_rows(float (&red)[4][9][64], const float (&r)[9], int i, int lane, float *__restrict__ ws,
                                                int b, long hw) {
#pragma unroll
    for (int k = 0; k < 9; ++k) red[i][k][lane] = r[k];
    __syncthreads();
    for (int e = threadIdx.x; e < 9 * 64; e += 256) {
        const int k = e >> 6, l = e & 63;
        const long pp = blockIdx.x * 64L + l;
        if (pp >= hw) continue;
        float s = red[0][k][l];
#pragma unroll
        for (int q = 1; q < 4; ++q) s = __fadd_rn(s, red[q][k][l]);
        ws[((long)b * 9 + k) * hw + pp] = s;
    }
}

// block (256): wave i = fine row i of 64 consecutive coarse pixels p = y*w + x of image blockIdx.y.  gweights and ws may be
// null (uniform: launch arguments), not both
__global__ __launch_bounds__(256) void cxu_weights_bwd_kernel(const float *__restrict__ gout, long gbs, const float *__restrict__ disp,
                                                              const float *__restrict__ wts, float *__restrict__ gweights,
                                                              float *__restrict__ ws, int h, int w) {
    __shared__ float red[4][9][64];
    const long hw = (long)h * w;
    const int lane = threadIdx.x & 63, i = threadIdx.x >> 6, b = blockIdx.y;
    const long p = blockIdx.x * 64L + lane;                                 // h * w < 2^31 - 256 (cxu_check)
    float r[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = 0.0f;
    if (p < hw) {
        const int y = (int)(p / w), x = (int)(p - (long)y * w);
        const long W4 = 4L * w, plane = 16 * hw;
        const long fine = (4L * y + i) * W4 + 4L * x;                       // (4y + i, 4x) inside a fine plane
        const long at = (long)b * 9 * plane + fine;
        float nb[9], g[4];
        if (gweights) cxu_taps_load(disp + b * hw, y, x, h, w, nb);
        cxu_load4(gout + b * gbs + fine, g);
        if (ws) {
            float q[9][4];
#pragma unroll
            for (int k = 0; k < 9; ++k) cxu_load4(wts + at + k * plane, q[k]);
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                r[k] = __fmul_rn(q[k][0], g[0]);
#pragma unroll
                for (int j = 1; j < 4; ++j) r[k] = __fadd_rn(r[k], __fmul_rn(q[k][j], g[j]));
            }
        }
        if (gweights) {
            cxu_taps_finish(nb, y, x, h, w, 1.0f);
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                float t[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) t[j] = __fmul_rn(g[j], nb[k]);
                cxu_store4(gweights + at + k * plane, t);
            }
        }
    }
    if (!ws) return;                                                        // uniform
    cxu_reduce_rows(red, r, i, lane, ws, b, hw);
}

// the same mapping
__global__ __launch_bounds__(256) void cxu_logits_fwd_kernel(const float *__restrict__ disp, const float *__restrict__ logits,
                                                             float scale, float *__restrict__ out, int h, int w) {
    const long hw = (long)h * w;
    const int lane = threadIdx.x & 63, i = threadIdx.x >> 6, b = blockIdx.y;
    const long p = blockIdx.x * 64L + lane;
    if (p >= hw) return;
    const int y = (int)(p / w), x = (int)(p - (long)y * w);
    const long W4 = 4L * w, plane = 16 * hw;
    const long fine = (4L * y + i) * W4 + 4L * x;
    float v[9], q[9][4], o[4];
    cxu_taps_load(disp + b * hw, y, x, h, w, v);
#pragma unroll
    for (int k = 0; k < 9; ++k) cxu_load4(logits + ((long)b * 9 + k) * plane + fine, q[k]);
    cxu_taps_finish(v, y, x, h, w, scale);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float m[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = q[k][j];
        cxu_softmax(m);
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < 9; ++k) acc = __fadd_rn(acc, __fmul_rn(m[k], v[k]));
        o[j] = acc;
    }
    cxu_store4(out + b * plane + fine, o);
}

// the same mapping; glogits and ws may be null (uniform), not both
__global__ __launch_bounds__(256) void cxu_logits_bwd_kernel(const float *__restrict__ gout, long gbs, const float *__restrict__ disp,
                                                             const float *__restrict__ logits, float scale,
                                                             float *__restrict__ glogits, float *__restrict__ ws, int h, int w) {
    __shared__ float red[4][9][64];
    const long hw = (long)h * w;
    const int lane = threadIdx.x & 63, i = threadIdx.x >> 6, b = blockIdx.y;
    const long p = blockIdx.x * 64L + lane;
    float r[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = 0.0f;
    if (p < hw) {
        const int y = (int)(p / w), x = (int)(p - (long)y * w);
        const long W4 = 4L * w, plane = 16 * hw;
        const long fine = (4L * y + i) * W4 + 4L * x;
        const long at = (long)b * 9 * plane + fine;
        float v[9], g[4], q[9][4];
        cxu_taps_load(disp + b * hw, y, x, h, w, v);
        cxu_load4(gout + b * gbs + fine, g);
#pragma unroll
        for (int k = 0; k < 9; ++k) cxu_load4(logits + at + k * plane, q[k]);
        cxu_taps_finish(v, y, x, h, w, scale);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float m[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) m[k] = q[k][j];
            cxu_softmax(m);
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const float t = __fmul_rn(m[k], g[j]);
                r[k] = j == 0 ? t : __fadd_rn(r[k], t);
            }
            float a[9], s = 0.0f;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                a[k] = __fmul_rn(g[j], v[k]);
                s = __fadd_rn(s, __fmul_rn(m[k], a[k]));
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) q[k][j] = __fmul_rn(m[k], __fsub_rn(a[k], s));
        }
        if (glogits) {
#pragma unroll
            for (int k = 0; k < 9; ++k) cxu_store4(glogits + at + k * plane, q[k]);
        }
    }
    if (!ws) return;                                                        // uniform
    cxu_reduce_rows(red, r, i, lane, ws, b, hw);
}

// thread = one gdisp element of image blockIdx.y
__global__ __launch_bounds__(256) void cxu_gdisp_kernel(const float *__restrict__ ws, float *__restrict__ gdisp, int h, int w,
                                                        float scale) {
    const long hw = (long)h * w;
    const long p = blockIdx.x * 256L + threadIdx.x;
    if (p >= hw) return;
    const int b = blockIdx.y, y = (int)(p / w), x = (int)(p - (long)y * w);
    const float *cp = ws + (long)b * 9 * hw;
    float t[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {                                           // clamped loads, the padding a select
        const int yy = y - k / 3 + 1, xx = x - k % 3 + 1;
        t[k] = cp[k * hw + (long)min(max(yy, 0), h - 1) * w + min(max(xx, 0), w - 1)];
    }
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int yy = y - k / 3 + 1, xx = x - k % 3 + 1;
        if (yy >= 0 && yy < h && xx >= 0 && xx < w) s = __fadd_rn(s, t[k]);
    }
    gdisp[b * hw + p] = __fmul_rn(scale, s);
}

static int cxu_check(int B, int h, int w) {
    if (B <= 0 || h <= 0 || w <= 0) return DKT_E_SHAPE;
    if (B > 65535 || (long)h * w > 0x7fffffffL - 256) return DKT_E_UNSUPPORTED;       // (grid.y; coarse pixel indices)
    return DKT_OK;
}

static bool cxu_aligned(const void *p) {
    return (uintptr_t)p % 16 == 0;
}

// a finite positive power of two: scale * disp is exact
static bool cxu_scale_ok(float scale) {
    int e;
    return isfinite(scale) && scale > 0.0f && frexpf(scale, &e) == 0.5f;
}

// blocks of 64 coarse pixels (the four-wave kernels) or of 256 (cxu_gdisp_kernel)
static dim3 cxu_grid(int B, int h, int w, int per = 64) {
    return dim3((unsigned)(((long)h * w + per - 1) / per), (unsigned)B);
}

extern "C" int dkt_context_upsample_bwd(const float *gout, long gout_bstride, const float *disp_low, const float *up_weights,
                                        float *gdisp, float *gweights, float *ws, int B, int h, int w, int device, void *stream) {
    if (!gout || !disp_low || !up_weights || (!gdisp && !gweights) || (gdisp && !ws)) return DKT_E_NULL;
    const int rc = cxu_check(B, h, w);
    if (rc != DKT_OK) return rc;
    if (gout_bstride < 16L * h * w) return DKT_E_SHAPE;
    if (!cxu_aligned(gout) || !cxu_aligned(up_weights) || !cxu_aligned(gweights) || gout_bstride % 4 != 0) return DKT_E_ALIGN;
    DKT_ENTER(device);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cxu_weights_bwd_kernel, cxu_grid(B, h, w), dim3(256), 0, st, gout, gout_bstride, disp_low, up_weights,
                       gweights, gdisp ? ws : nullptr, h, w);
    if (gdisp) hipLaunchKernelGGL(cxu_gdisp_kernel, cxu_grid(B, h, w, 256), dim3(256), 0, st, ws, gdisp, h, w, 1.0f);
    return dkt_launch_status();
}

extern "C" int dkt_context_upsample_logits_fwd(const float *disp_low, const float *logits, float scale, float *out, int B, int h,
                                               int w, int device, void *stream) {
    if (!disp_low || !logits || !out) return DKT_E_NULL;
    const int rc = cxu_check(B, h, w);
    if (rc != DKT_OK) return rc;
    if (!cxu_scale_ok(scale)) return DKT_E_UNSUPPORTED;
    if (!cxu_aligned(out) || !cxu_aligned(logits)) return DKT_E_ALIGN;
    DKT_ENTER(device);
    hipLaunchKernelGGL(cxu_logits_fwd_kernel, cxu_grid(B, h, w), dim3(256), 0, (hipStream_t)stream, disp_low, logits, scale, out,
                       h, w);
    return dkt_launch_status();
}

extern "C" int dkt_context_upsample_logits_bwd(const float *gout, long gout_bstride, const float *disp_low, const float *logits,
                                               float scale, float *gdisp, float *glogits, float *ws, int B, int h, int w,
                                               int device, void *stream) {
    if (!gout || !disp_low || !logits || (!gdisp && !glogits) || (gdisp && !ws)) return DKT_E_NULL;
    const int rc = cxu_check(B, h, w);
    if (rc != DKT_OK) return rc;
    if (gout_bstride < 16L * h * w) return DKT_E_SHAPE;
    if (!cxu_scale_ok(scale)) return DKT_E_UNSUPPORTED;
    if (!cxu_aligned(gout) || !cxu_aligned(logits) || !cxu_aligned(glogits) || gout_bstride % 4 != 0) return DKT_E_ALIGN;
    DKT_ENTER(device);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cxu_logits_bwd_kernel, cxu_grid(B, h, w), dim3(256), 0, st, gout, gout_bstride, disp_low, logits, scale,
                       glogits, gdisp ? ws : nullptr, h, w);
    if (gdisp) hipLaunchKernelGGL(cxu_gdisp_kernel, cxu_grid(B, h, w, 256), dim3(256), 0, st, ws, gdisp, h, w, scale);
    return dkt_launch_status();
}
