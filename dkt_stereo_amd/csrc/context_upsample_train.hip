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
// This is the nine-tap core of ups9.h at one channel and f = 4 (softmax, taps, row accesses, the meeting of the row sums,
// the second launch), shared with upsample_train.hip; here are the three kernels that read the nine planes at full resolution.
// Plain scalar fp32 (no packed math: DESIGN 3.4).
#include <math.h>

#include "ups9.h"

// block (256): wave i = fine row i of 64 consecutive coarse pixels p = y*w + x of image blockIdx.y.  gweights and ws may be
// null (uniform: launch arguments), not both
__global__ __launch_bounds__(256) void cxu_weights_bwd_kernel(const float *__restrict__ gout, long gbs, const float *__restrict__ disp,
                                                              const float *__restrict__ wts, float *__restrict__ gweights,
                                                              float *__restrict__ ws, int h, int w) {
    __shared__ float red[4][9][64];
    const long hw = (long)h * w;
    const int lane = threadIdx.x & 63, i = threadIdx.x >> 6, b = blockIdx.y;
    const long p = blockIdx.x * 64L + lane;                                 // h * w < 2^31 - 256 (ups9_check)
    const int ch[1] = {0};
    const bool on[1] = {true};
    float r[1][9];
#pragma unroll
    for (int k = 0; k < 9; ++k) r[0][k] = 0.0f;
    if (p < hw) {
        const int y = (int)(p / w), x = (int)(p - (long)y * w);
        const long W4 = 4L * w, plane = 16 * hw;
        const long fine = (4L * y + i) * W4 + 4L * x;                       // (4y + i, 4x) inside a fine plane
        const long at = (long)b * 9 * plane + fine;
        float nb[1][9], g[4];
        if (gweights) ups9_taps_load<1>(disp + b * hw, hw, ch, y, x, h, w, nb);
        ups9_load_row<4>(gout + b * gbs + fine, g);
        if (ws) {
            float q[9][4];
#pragma unroll
            for (int k = 0; k < 9; ++k) ups9_load_row<4>(wts + at + k * plane, q[k]);
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                r[0][k] = __fmul_rn(q[k][0], g[0]);
#pragma unroll
                for (int j = 1; j < 4; ++j) r[0][k] = __fadd_rn(r[0][k], __fmul_rn(q[k][j], g[j]));
            }
        }
        if (gweights) {
            ups9_taps_finish<1>(nb, on, y, x, h, w, 1.0f);
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                float t[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) t[j] = __fmul_rn(g[j], nb[0][k]);
                ups9_store_row<4>(gweights + at + k * plane, t);
            }
        }
    }
    if (!ws) return;                                                        // uniform
    ups9_reduce_rows<4, 1>(red, r, i, lane, ws, b, 1, 0, hw);               // every thread comes here: no return above but that one
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
    const int ch[1] = {0};
    const bool on[1] = {true};
    float v[1][9], q[9][4], o[4];
    ups9_taps_load<1>(disp + b * hw, hw, ch, y, x, h, w, v);
#pragma unroll
    for (int k = 0; k < 9; ++k) ups9_load_row<4>(logits + ((long)b * 9 + k) * plane + fine, q[k]);
    ups9_taps_finish<1>(v, on, y, x, h, w, scale);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float m[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = q[k][j];
        ups9_softmax(m);
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < 9; ++k) acc = __fadd_rn(acc, __fmul_rn(m[k], v[0][k]));
        o[j] = acc;
    }
    ups9_store_row<4>(out + b * plane + fine, o);
}

// the same mapping; glogits and ws may be null (uniform), not both
__global__ __launch_bounds__(256) void cxu_logits_bwd_kernel(const float *__restrict__ gout, long gbs, const float *__restrict__ disp,
                                                             const float *__restrict__ logits, float scale,
                                                             float *__restrict__ glogits, float *__restrict__ ws, int h, int w) {
    __shared__ float red[4][9][64];
    const long hw = (long)h * w;
    const int lane = threadIdx.x & 63, i = threadIdx.x >> 6, b = blockIdx.y;
    const long p = blockIdx.x * 64L + lane;
    const int ch[1] = {0};
    const bool on[1] = {true};
    float r[1][9];
#pragma unroll
    for (int k = 0; k < 9; ++k) r[0][k] = 0.0f;
    if (p < hw) {
        const int y = (int)(p / w), x = (int)(p - (long)y * w);
        const long W4 = 4L * w, plane = 16 * hw;
        const long fine = (4L * y + i) * W4 + 4L * x;
        const long at = (long)b * 9 * plane + fine;
        float v[1][9], g[4], q[9][4];
        ups9_taps_load<1>(disp + b * hw, hw, ch, y, x, h, w, v);
        ups9_load_row<4>(gout + b * gbs + fine, g);
#pragma unroll
        for (int k = 0; k < 9; ++k) ups9_load_row<4>(logits + at + k * plane, q[k]);
        ups9_taps_finish<1>(v, on, y, x, h, w, scale);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float m[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) m[k] = q[k][j];
            ups9_softmax(m);
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const float t = __fmul_rn(m[k], g[j]);
                r[0][k] = j == 0 ? t : __fadd_rn(r[0][k], t);
            }
            float a[9], s = 0.0f;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                a[k] = __fmul_rn(g[j], v[0][k]);
                s = __fadd_rn(s, __fmul_rn(m[k], a[k]));
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) q[k][j] = __fmul_rn(m[k], __fsub_rn(a[k], s));
        }
        if (glogits) {
#pragma unroll
            for (int k = 0; k < 9; ++k) ups9_store_row<4>(glogits + at + k * plane, q[k]);
        }
    }
    if (!ws) return;                                                        // uniform
    ups9_reduce_rows<4, 1>(red, r, i, lane, ws, b, 1, 0, hw);               // every thread comes here: no return above but that one
}

// a finite positive power of two: scale * disp is exact
static bool cxu_scale_ok(float scale) {
    int e;
    return isfinite(scale) && scale > 0.0f && frexpf(scale, &e) == 0.5f;
}

extern "C" int dkt_context_upsample_bwd(const float *gout, long gout_bstride, const float *disp_low, const float *up_weights,
                                        float *gdisp, float *gweights, float *ws, int B, int h, int w, int device, void *stream) {
    if (!gout || !disp_low || !up_weights || (!gdisp && !gweights) || (gdisp && !ws)) return DKT_E_NULL;
    const int rc = ups9_check(B, h, w);
    if (rc != DKT_OK) return rc;
    if (gout_bstride < 16L * h * w) return DKT_E_SHAPE;
    if (!ups9_aligned(gout) || !ups9_aligned(up_weights) || !ups9_aligned(gweights) || gout_bstride % 4 != 0) return DKT_E_ALIGN;
    DKT_ENTER(device);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cxu_weights_bwd_kernel, ups9_grid(B, h, w), dim3(256), 0, st, gout, gout_bstride, disp_low, up_weights,
                       gweights, gdisp ? ws : nullptr, h, w);
    if (gdisp) ups9_gather(ws, gdisp, B, 1, 1, h, w, 1.0f, st);
    return dkt_launch_status();
}

extern "C" int dkt_context_upsample_logits_fwd(const float *disp_low, const float *logits, float scale, float *out, int B, int h,
                                               int w, int device, void *stream) {
    if (!disp_low || !logits || !out) return DKT_E_NULL;
    const int rc = ups9_check(B, h, w);
    if (rc != DKT_OK) return rc;
    if (!cxu_scale_ok(scale)) return DKT_E_UNSUPPORTED;
    if (!ups9_aligned(out) || !ups9_aligned(logits)) return DKT_E_ALIGN;
    DKT_ENTER(device);
    hipLaunchKernelGGL(cxu_logits_fwd_kernel, ups9_grid(B, h, w), dim3(256), 0, (hipStream_t)stream, disp_low, logits, scale, out,
                       h, w);
    return dkt_launch_status();
}

extern "C" int dkt_context_upsample_logits_bwd(const float *gout, long gout_bstride, const float *disp_low, const float *logits,
                                               float scale, float *gdisp, float *glogits, float *ws, int B, int h, int w,
                                               int device, void *stream) {
    if (!gout || !disp_low || !logits || (!gdisp && !glogits) || (gdisp && !ws)) return DKT_E_NULL;
    const int rc = ups9_check(B, h, w);
    if (rc != DKT_OK) return rc;
    if (gout_bstride < 16L * h * w) return DKT_E_SHAPE;
    if (!cxu_scale_ok(scale)) return DKT_E_UNSUPPORTED;
    if (!ups9_aligned(gout) || !ups9_aligned(logits) || !ups9_aligned(glogits) || gout_bstride % 4 != 0) return DKT_E_ALIGN;
    DKT_ENTER(device);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cxu_logits_bwd_kernel, ups9_grid(B, h, w), dim3(256), 0, st, gout, gout_bstride, disp_low, logits, scale,
                       glogits, gdisp ? ws : nullptr, h, w);
    if (gdisp) ups9_gather(ws, gdisp, B, 1, 1, h, w, scale, st);
    return dkt_launch_status();
}
