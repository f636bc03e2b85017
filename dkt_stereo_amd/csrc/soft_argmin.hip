// soft_argmin.hip -- the disparity head of GwcNet (GWCNet.forward, meta_arch/gwcnet/gwc_main.py:246-276: F.interpolate
// x4 trilinear, F.softmax over the 192 planes, disparity_regression of gwcnet/submodules.py:18-22) and, at factor 1,
// IGEV's initial disparity (igev_stereo.py:175-176) as one operator, forward and backward:
//   dkt_soft_argmin_fwd            out[b,0,Y,X] = out_scale * sum_d d softmax_d(up(cost))[b,d,Y,X], one launch
//   dkt_soft_argmin_bwd            its gradient with respect to cost, the softmax recomputed from cost (nothing else saved)
//   dkt_soft_argmin_bwd_workspace  the bytes of scratch the backward wants
// The up-sampled volume (B, f Dc, f h, f w) never exists: a thread owns one output pixel and streams over the coarse depth.
//
// up() is torch's trilinear align_corners=False at exactly 1/f per axis.  At f = 4 fine index o = 4q + j lies between coarse
// i0 = q - 1 (j < 2) or q (j >= 2) and i0 + 1, at lambda = .625, .875, .125, .375; indices clamp to the axis.  (torch also
// clamps the source coordinate to 0, which makes lambda 0 where i0 would be -1: the two taps are then the same element, and
// a + lambda (b - a) is a for every lambda.  The same holds at the far end, so only the indices are clamped here.)
//
// Depth.  With v_k the H/W blend of coarse plane k at the thread's pixel (v_-1 = v_0, v_Dc = v_Dc-1), slot k = 0..Dc lies
// between a = v_k-1 and b = v_k and holds the fine logits d = 4k - 2 + j, j < 4, z_d = a + (.125 + .25 j)(b - a); d outside
// [0, D) is absent.  The softmax is shifted by the maximum of the FINE logits seen so far (online rescale per slot): the
// coarse maximum is no valid shift, a fine logit can lie .125 (spread) below every coarse value next to it.
//   m, s = sum_d exp(z_d - m), t = sum_d d exp(z_d - m) in ascending d;  E = t / s;  out = out_scale E.
// At f = 1 a "slot" is four consecutive planes of the thread's column, read from global memory as they are.
//
// Forward, f = 4: a block of 256 threads owns a 32 x 8 tile of output pixels (a wave: two rows of 32) and stages the
// (Dc, 4, 10) coarse footprint of the tile in LDS with clamped indices (<= 10 KB); per slot a thread reads four LDS values.
//
// Backward.  g' = out_scale gout, p_d = exp(z_d - m) / s, u_d = g' p_d (d - E) is the gradient of z_d.  A first pass is the
// forward's (the same m, s, E bits); a second one forms u_d per slot and gives (1 - lambda) u_d to a, lambda u_d to b, so
// the gradient of v_k is complete one slot later.  It goes to the workspace ws (B, Dc, f h, f w), a quarter of the
// up-sampled volume; a second launch owns one element of gcost per thread and gathers the at most 8 x 8 output pixels whose
// blend reads it, rows ascending, within a row columns ascending.  At f = 1 u_d is gcost: one launch, no workspace.
// Deterministic: one owner per element, fixed orders, no atomics.  Plain scalar fp32 (no packed math: DESIGN 3.4); the
// build's -ffp-contract=off keeps every product and sum rounded as written.
#include <math.h>

#include "dkt_common.h"

#define SA_TW 32                        // the tile of output pixels
#define SA_TH 8
#define SA_CW (SA_TW / 4 + 2)           // its coarse footprint at f = 4
#define SA_CH (SA_TH / 4 + 2)
#define SA_CELLS (SA_CW * SA_CH)
#define SA_MAX_D 256
#define SA_MAX_DC4 (SA_MAX_D / 4)

struct SaStat {
    float m, s, t;                      // running maximum, sum of exp(z - m), sum of d exp(z - m)
};

// lambda of phase j = o & 3 of a fine index at f = 4: .625, .875, .125, .375
__device__ __forceinline__ float sa_lambda(int j) {
    return 0.125f + 0.25f * (float)((j + 2) & 3);
}

// four fine logits d0 .. d0 + 3 (those outside [0, D) absent) join the running softmax; the first call of a column holds a
// logit inside the range, so m is finite afterwards (expf(-inf) = 0 makes the first rescale a multiplication of 0 by 0)
__device__ __forceinline__ void sa_push(SaStat &a, const float (&z)[4], int d0, int D) {
    float zz[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) zz[j] = (unsigned)(d0 + j) < (unsigned)D ? z[j] : -INFINITY;
    const float mn = fmaxf(a.m, fmaxf(fmaxf(zz[0], zz[1]), fmaxf(zz[2], zz[3])));
    const float r = expf(a.m - mn);
    float s = a.s * r, t = a.t * r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float e = expf(zz[j] - mn);
        s = s + e;
        t = t + (float)(d0 + j) * e;
    }
    a.m = mn, a.s = s, a.t = t;
}

// the four fine logits of the slot between a and b
__device__ __forceinline__ void sa_slot(float a, float b, float (&z)[4]) {
    const float diff = b - a;
#pragma unroll
    for (int j = 0; j < 4; ++j) z[j] = a + (0.125f + 0.25f * (float)j) * diff;
}

// f = 4: what a thread of the tile reads of the staged footprint -- the four cells around its pixel and the two lambdas
struct SaTaps {
    int c00, c01, c10, c11;
    float lx, ly;
};

__device__ __forceinline__ SaTaps sa_taps(int tx, int ty) {
    const int jx = tx & 3, jy = ty & 3;                     // the tile's origin is a multiple of 4
    const int c = (tx >> 2) + (jx >= 2), r = (ty >> 2) + (jy >= 2);   // footprint cell of (i0y, i0x): the footprint starts one coarse cell before the tile
    SaTaps t;
    t.c00 = r * SA_CW + c, t.c01 = t.c00 + 1, t.c10 = t.c00 + SA_CW, t.c11 = t.c10 + 1;
    t.lx = sa_lambda(jx), t.ly = sa_lambda(jy);
    return t;
}

__device__ __forceinline__ float sa_blend(const float *__restrict__ plane, const SaTaps &t) {
    const float top = plane[t.c00] + t.lx * (plane[t.c01] - plane[t.c00]);
    const float bot = plane[t.c10] + t.lx * (plane[t.c11] - plane[t.c10]);
    return top + t.ly * (bot - top);
}

// the (Dc, SA_CH, SA_CW) footprint of tile (blockIdx.y, blockIdx.x) of one image, indices clamped to the image; Dc <= 64
__device__ __forceinline__ void sa_stage(float *__restrict__ tile, const float *__restrict__ img, int Dc, int h, int w) {
    const long hw = (long)h * w;
    const int y0 = blockIdx.y * (SA_TH / 4) - 1, x0 = blockIdx.x * (SA_TW / 4) - 1;
    for (int e = threadIdx.x; e < Dc * SA_CELLS; e += 256) {
        const int k = e / SA_CELLS, c = e - k * SA_CELLS, r = c / SA_CW, cc = c - r * SA_CW;
        const int y = min(max(y0 + r, 0), h - 1), x = min(max(x0 + cc, 0), w - 1);
        tile[e] = img[k * hw + (long)y * w + x];
    }
}

// m, s, t of the thread's column.  F = 4: from the staged footprint; F = 1: col points at plane 0 of the pixel, planes hw apart
template <int F>
__device__ __forceinline__ SaStat sa_column(const float *__restrict__ tile, const SaTaps &tp, const float *__restrict__ col,
                                            long hw, int Dc) {
    SaStat st = {-INFINITY, 0.0f, 0.0f};
    float z[4];
    if constexpr (F == 4) {
        float a = sa_blend(tile, tp);
        for (int k = 0; k <= Dc; ++k) {
            const float b = sa_blend(tile + min(k, Dc - 1) * SA_CELLS, tp);
            sa_slot(a, b, z);
            sa_push(st, z, 4 * k - 2, 4 * Dc);
            a = b;
        }
    } else {
        for (int k = 0; k < Dc; k += 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] = col[min(k + j, Dc - 1) * hw];
            sa_push(st, z, k, Dc);
        }
    }
    return st;
}

// block (256) = the 32 x 8 tile (blockIdx.y, blockIdx.x) of the output of image blockIdx.z
template <int F>
__global__ __launch_bounds__(256) void sa_fwd_kernel(const float *__restrict__ cost, long cbs, float out_scale,
                                                     float *__restrict__ out, int Dc, int h, int w) {
    float *tile = nullptr;
    const int H = F * h, W = F * w, b = blockIdx.z;
    const int tx = threadIdx.x & (SA_TW - 1), ty = threadIdx.x / SA_TW;
    const int X = blockIdx.x * SA_TW + tx, Y = blockIdx.y * SA_TH + ty;
    const float *img = cost + b * cbs;
    SaTaps tp = {};
    if constexpr (F == 4) {
        __shared__ float staged[SA_MAX_DC4 * SA_CELLS];
        tile = staged;
        sa_stage(tile, img, Dc, h, w);
        tp = sa_taps(tx, ty);
        __syncthreads();
    }
    if (X >= W || Y >= H) return;                           // after the block's only barrier
    const long hw = (long)h * w, pix = (long)Y * W + X;
    const SaStat st = sa_column<F>(tile, tp, img + pix, hw, Dc);
    out[(long)b * H * W + pix] = out_scale * (st.t / st.s);
}

// the same mapping.  F = 4: dst is ws (B, Dc, H, W), the gradient of the blended v_k of every output pixel; F = 1: dst is gcost
template <int F>
__global__ __launch_bounds__(256) void sa_bwd_kernel(const float *__restrict__ gout, long gbs, const float *__restrict__ cost,
                                                     long cbs, float out_scale, float *__restrict__ dst, int Dc, int h, int w) {
    float *tile = nullptr;
    const int H = F * h, W = F * w, b = blockIdx.z;
    const int tx = threadIdx.x & (SA_TW - 1), ty = threadIdx.x / SA_TW;
    const int X = blockIdx.x * SA_TW + tx, Y = blockIdx.y * SA_TH + ty;
    const float *img = cost + b * cbs;
    SaTaps tp = {};
    if constexpr (F == 4) {
        __shared__ float staged[SA_MAX_DC4 * SA_CELLS];
        tile = staged;
        sa_stage(tile, img, Dc, h, w);
        tp = sa_taps(tx, ty);
        __syncthreads();
    }
    if (X >= W || Y >= H) return;
    const long hw = (long)h * w, HW = (long)H * W, pix = (long)Y * W + X;
    const float *col = img + pix;
    const SaStat st = sa_column<F>(tile, tp, col, hw, Dc);
    const float E = st.t / st.s, rs = 1.0f / st.s, m = st.m;
    const float gs = out_scale * gout[b * gbs + pix];
    float *o = dst + (long)b * Dc * HW + pix;               // plane k of the pixel at o[k * HW]
    if constexpr (F == 4) {
        const int D = 4 * Dc;
        float a = sa_blend(tile, tp), carry = 0.0f;
        for (int k = 0; k <= Dc; ++k) {
            const float bb = sa_blend(tile + min(k, Dc - 1) * SA_CELLS, tp);
            float z[4], ga = 0.0f, gb = 0.0f;
            sa_slot(a, bb, z);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int d = 4 * k - 2 + j;
                const float lam = 0.125f + 0.25f * (float)j;
                if ((unsigned)d >= (unsigned)D) continue;    // absent (uniform: slots 0 and Dc only)
                const float u = gs * ((expf(z[j] - m) * rs) * ((float)d - E));
                ga = ga + (1.0f - lam) * u;
                gb = gb + lam * u;
            }
            if (k == 0) {
                carry = ga + gb;                            // a is v_0 itself
            } else if (k < Dc) {
                o[(k - 1) * HW] = carry + ga;
                carry = gb;
            } else {
                o[(Dc - 1) * HW] = carry + (ga + gb);       // b is v_Dc-1 itself
            }
            a = bb;
        }
    } else {
        for (int k = 0; k < Dc; ++k) {
            const float p = expf(col[k * hw] - m) * rs;
            o[k * HW] = gs * (p * ((float)k - E));
        }
    }
}

// the weight of coarse index c (axis length n) in the blend of fine index o at f = 4
__device__ __forceinline__ float sa_weight(int o, int c, int n) {
    const int j = o & 3, i = (o >> 2) - (j < 2);
    const float lam = sa_lambda(j);
    return (max(i, 0) == c ? 1.0f - lam : 0.0f) + (min(i + 1, n - 1) == c ? lam : 0.0f);
}

// f = 4, the second launch.  thread = one element (y, x) of plane (blockIdx.z, blockIdx.y) = (b, k) of gcost: the output
// pixels 4y - 2 .. 4y + 5 by 4x - 2 .. 4x + 5 that lie in the image, each times its two weights
__global__ __launch_bounds__(256) void sa_gather_kernel(const float *__restrict__ ws, float *__restrict__ gcost, int h, int w) {
    const int Dc = gridDim.y, k = blockIdx.y, b = blockIdx.z;
    const int p = blockIdx.x * 256 + threadIdx.x;           // h * w < 2^31 - 256 (sa_check)
    if (p >= h * w) return;
    const int y = p / w, x = p - y * w, H = 4 * h, W = 4 * w;
    const float *src = ws + ((long)b * Dc + k) * ((long)H * W);
    float wx[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) wx[i] = sa_weight(4 * x - 2 + i, x, w);
    float s = 0.0f;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int Y = 4 * y - 2 + r;
        if (Y < 0 || Y >= H) continue;
        const float *row = src + (long)Y * W;
        float q = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int X = 4 * x - 2 + i;
            if (X >= 0 && X < W) q = q + wx[i] * row[X];
        }
        s = s + sa_weight(Y, y, h) * q;
    }
    gcost[((long)b * Dc + k) * ((long)h * w) + p] = s;
}

// ---- host side
// sign, the batch stride, then the limits: the factor, the depth (the staged footprint), grid.z, grid.y and the int pixel index
static int sa_check(long cost_bstride, int B, int Dc, int h, int w, int factor) {
    if (B <= 0 || Dc <= 0 || h <= 0 || w <= 0) return DKT_E_SHAPE;
    if (cost_bstride < (long)Dc * h * w) return DKT_E_SHAPE;
    if (factor != 1 && factor != 4) return DKT_E_UNSUPPORTED;
    if ((long)factor * Dc > SA_MAX_D || B > 65535) return DKT_E_UNSUPPORTED;
    const long H = (long)factor * h, W = (long)factor * w;
    if (H * W > 0x7fffffffL - 256 || (H + SA_TH - 1) / SA_TH > 65535) return DKT_E_UNSUPPORTED;
    return DKT_OK;
}

static bool sa_aligned(const void *p) {
    return (uintptr_t)p % sizeof(float) == 0;
}

static dim3 sa_grid(int B, int h, int w, int factor) {
    return dim3((unsigned)((factor * w + SA_TW - 1) / SA_TW), (unsigned)((factor * h + SA_TH - 1) / SA_TH), (unsigned)B);
}

extern "C" long dkt_soft_argmin_bwd_workspace(int B, int Dc, int h, int w, int factor) {
    const int rc = sa_check((long)Dc * h * w, B, Dc, h, w, factor);
    if (rc != DKT_OK) return rc;
    return factor == 1 ? 0L : (long)sizeof(float) * B * Dc * 16L * h * w;
}

extern "C" int dkt_soft_argmin_fwd(const float *cost, long cost_bstride, float out_scale, float *out, int B, int Dc, int h, int w,
                                   int factor, int device, void *stream) {
    if (!cost || !out) return DKT_E_NULL;
    const int rc = sa_check(cost_bstride, B, Dc, h, w, factor);
    if (rc != DKT_OK) return rc;
    if (!sa_aligned(cost) || !sa_aligned(out)) return DKT_E_ALIGN;
    DKT_ENTER(device);
    hipStream_t st = (hipStream_t)stream;
    if (factor == 4)
        hipLaunchKernelGGL(sa_fwd_kernel<4>, sa_grid(B, h, w, 4), dim3(256), 0, st, cost, cost_bstride, out_scale, out, Dc, h, w);
    else
        hipLaunchKernelGGL(sa_fwd_kernel<1>, sa_grid(B, h, w, 1), dim3(256), 0, st, cost, cost_bstride, out_scale, out, Dc, h, w);
    return dkt_launch_status();
}

extern "C" int dkt_soft_argmin_bwd(const float *gout, long gout_bstride, const float *cost, long cost_bstride, float out_scale,
                                   float *gcost, void *ws, int B, int Dc, int h, int w, int factor, int device, void *stream) {
    if (!gout || !cost || !gcost) return DKT_E_NULL;
    const int rc = sa_check(cost_bstride, B, Dc, h, w, factor);
    if (rc != DKT_OK) return rc;
    if (gout_bstride < (long)factor * h * factor * w) return DKT_E_SHAPE;
    if (factor == 4 && !ws) return DKT_E_NULL;              // (after the sizes: only then is it known that the call needs it)
    if (!sa_aligned(gout) || !sa_aligned(cost) || !sa_aligned(gcost) || !sa_aligned(ws)) return DKT_E_ALIGN;
    DKT_ENTER(device);
    hipStream_t st = (hipStream_t)stream;
    if (factor == 4) {
        hipLaunchKernelGGL(sa_bwd_kernel<4>, sa_grid(B, h, w, 4), dim3(256), 0, st, gout, gout_bstride, cost, cost_bstride, out_scale,
                           (float *)ws, Dc, h, w);
        hipLaunchKernelGGL(sa_gather_kernel, dim3((unsigned)(((long)h * w + 255) / 256), (unsigned)Dc, (unsigned)B), dim3(256), 0, st,
                           (const float *)ws, gcost, h, w);
    } else {
        hipLaunchKernelGGL(sa_bwd_kernel<1>, sa_grid(B, h, w, 1), dim3(256), 0, st, gout, gout_bstride, cost, cost_bstride, out_scale,
                           gcost, Dc, h, w);
    }
    return dkt_launch_status();
}
