// topk_regress.hip -- CGI-Stereo's disparity head, regression_topk(cost, disparity_samples, k) of meta_arch/cgi/submodule.py:220-228
// (called with k = 2 at meta_arch/cgi/CGI_Stereo.py:256-259: a full descending sort of every pixel's column, two gathers, a
// softmax over the k kept values, a product and a sum), forward and backward:
//   dkt_topk_regress_fwd   out[b,0,y,x] = sum_i s_i p_i over the k largest planes of the pixel's column, one launch
//   dkt_topk_regress_bwd   its gradient with respect to cost and to the samples, from the k saved plane indices, one launch
// The sorted volume, its int64 indices and the (B, D, h, w) tensor of repeated arange never exist.
//
// Selection.  A thread owns one pixel and streams its D planes in ascending d (a wave reads 64 consecutive floats of a
// plane), TK_BATCH loads issued together ahead of their compares.  It keeps the K best (value, plane) pairs in registers,
// best first.  x ranks above y when x > y, or when x is NaN and y is not (torch's sort puts NaN above every number); a plane
// that does not rank above a kept one stays behind it, so equal values (and NaNs among themselves) keep ascending plane
// order: the selection of cost.sort(dim=1, descending=True, stable=True).  A slot that holds nothing yet (plane -1) is below
// everything, -inf included; K <= D fills every slot.  The insertion is a fixed network of K compares and selects on
// named registers (K is a template parameter, every loop over the slots unrolled): nothing is indexed dynamically.
//
// Regression.  c_0 >= c_1 >= ... are the kept values, c_0 their maximum:  e_i = exp(c_i - c_0),  S = e_0 + e_1 + ... in that
// order,  p_i = e_i / S,  pred = s_0 p_0 + s_1 p_1 + ... in that order,  s_i = samples[b, d_i, y, x] or, when the samples
// pointer is null, float(d_i).  A NaN in the column is kept first and makes every e_i, hence pred, NaN; no other pixel reads it.
// With an index buffer the planes d_0 .. d_K-1 are stored as bytes, (B, K, h, w): D <= 256.
//
// Backward.  The owner of a pixel reads its K bytes, gathers the K costs (and samples), recomputes p_i and pred with the
// forward's arithmetic, and writes all D planes of gcost once: g p_i (s_i - pred) on plane d_i, zero on the others; gsamples
// likewise with g p_i.  One owner per element, no atomics, no memset: deterministic, and an unwritten output cannot exist.
// Plain scalar fp32 (no packed math: DESIGN 3.4); the build's -ffp-contract=off keeps every product and sum rounded as written.
#include <math.h>

#include "dkt_common.h"

#define TK_MAX_K 8
#define TK_MAX_D 256
#define TK_THREADS 64                   // one wave per block: at B = 1, 136 x 240 that is 510 blocks over 256 CUs, two per CU
#define TK_BATCH 24                     // planes loaded together ahead of their compares (measured: DESIGN 3.23)

// x (not yet kept) ranks above the kept value v of plane d
__device__ __forceinline__ bool tk_above(float x, float v, int d) {
    return d < 0 || x > v || (x != x && v == v);
}

// (x, plane dx) joins the K kept pairs, best first
template <int K>
__device__ __forceinline__ void tk_insert(float (&v)[K], int (&d)[K], float x, int dx) {
    bool above[K];
#pragma unroll
    for (int j = 0; j < K; ++j) above[j] = tk_above(x, v[j], d[j]);
#pragma unroll
    for (int j = K - 1; j > 0; --j) {    // descending: slot j - 1 still holds what it held
        v[j] = above[j] ? (above[j - 1] ? v[j - 1] : x) : v[j];
        d[j] = above[j] ? (above[j - 1] ? d[j - 1] : dx) : d[j];
    }
    v[0] = above[0] ? x : v[0];
    d[0] = above[0] ? dx : d[0];
}

// p_i and pred from the kept costs c (best first) and their samples s
template <int K>
__device__ __forceinline__ float tk_regress(const float (&c)[K], const float (&s)[K], float (&p)[K]) {
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        p[i] = expf(c[i] - c[0]);
        sum = i ? sum + p[i] : p[i];
    }
    float pred = 0.0f;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        p[i] = p[i] / sum;
        pred = i ? pred + s[i] * p[i] : s[i] * p[i];
    }
    return pred;
}

// thread = pixel blockIdx.x * TK_THREADS + threadIdx.x of image blockIdx.y
template <int K>
__global__ __launch_bounds__(TK_THREADS) void tk_fwd_kernel(const float *__restrict__ cost, long cbs, const float *__restrict__ samples,
                                                            long sbs, float *__restrict__ out, unsigned char *__restrict__ idx, int D,
                                                            int hw) {
    const int pix = blockIdx.x * TK_THREADS + threadIdx.x, b = blockIdx.y;   // hw < 2^31 - TK_THREADS (tk_check)
    if (pix >= hw) return;
    const float *col = cost + b * cbs + pix;                                 // plane d of the pixel at col[d * hw]
    float v[K];
    int d[K];
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] = -INFINITY, d[j] = -1;
    for (int d0 = 0; d0 < D; d0 += TK_BATCH) {
        float x[TK_BATCH];
#pragma unroll
        for (int j = 0; j < TK_BATCH; ++j) x[j] = col[(long)min(d0 + j, D - 1) * hw];
#pragma unroll
        for (int j = 0; j < TK_BATCH; ++j)
            if (d0 + j < D) tk_insert<K>(v, d, x[j], d0 + j);                // (uniform: the last batch only)
    }
    float s[K], p[K];
#pragma unroll
    for (int i = 0; i < K; ++i) s[i] = samples ? samples[b * sbs + (long)d[i] * hw + pix] : (float)d[i];
    out[(long)b * hw + pix] = tk_regress<K>(v, s, p);
    if (idx) {
#pragma unroll
        for (int i = 0; i < K; ++i) idx[((long)b * K + i) * hw + pix] = (unsigned char)d[i];
    }
}

// the same mapping; gcost and gsamples (B, D, h, w) contiguous, either may be null
template <int K>
__global__ __launch_bounds__(TK_THREADS) void tk_bwd_kernel(const float *__restrict__ gout, long gbs, const float *__restrict__ cost, long cbs,
                                                            const float *__restrict__ samples, long sbs,
                                                            const unsigned char *__restrict__ idx, float *__restrict__ gcost,
                                                            float *__restrict__ gsamples, int D, int hw) {
    const int pix = blockIdx.x * TK_THREADS + threadIdx.x, b = blockIdx.y;
    if (pix >= hw) return;
    int d[K];
    float c[K], s[K], p[K];
#pragma unroll
    for (int i = 0; i < K; ++i) d[i] = min((int)idx[((long)b * K + i) * hw + pix], D - 1);   // (a byte the forward wrote is < D)
#pragma unroll
    for (int i = 0; i < K; ++i) {
        c[i] = cost[b * cbs + (long)d[i] * hw + pix];
        s[i] = samples ? samples[b * sbs + (long)d[i] * hw + pix] : (float)d[i];
    }
    const float pred = tk_regress<K>(c, s, p);
    const float g = gout[b * gbs + pix];
    float gc[K], gs[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        gs[i] = g * p[i];
        gc[i] = gs[i] * (s[i] - pred);
    }
    const long o = (long)b * D * hw + pix;                                   // plane k of the pixel at o + k * hw
    if (gcost) {
        for (int k = 0; k < D; ++k) {
            float val = 0.0f;
#pragma unroll
            for (int i = 0; i < K; ++i) val = d[i] == k ? gc[i] : val;
            gcost[o + (long)k * hw] = val;
        }
    }
    if (gsamples) {
        for (int k = 0; k < D; ++k) {
            float val = 0.0f;
#pragma unroll
            for (int i = 0; i < K; ++i) val = d[i] == k ? gs[i] : val;
            gsamples[o + (long)k * hw] = val;
        }
    }
}

// ---- host side
// sign and k against D, the batch stride, then the limits: k (the registers), D (a byte per index), grid.y and the int pixel index
static int tk_check(long cost_bstride, int B, int D, int h, int w, int k) {
    if (B <= 0 || D <= 0 || h <= 0 || w <= 0 || k < 1 || k > D) return DKT_E_SHAPE;
    if (cost_bstride < (long)D * h * w) return DKT_E_SHAPE;
    if (k > TK_MAX_K || D > TK_MAX_D || B > 65535) return DKT_E_UNSUPPORTED;
    if ((long)h * w > 0x7fffffffL - 256) return DKT_E_UNSUPPORTED;
    return DKT_OK;
}

static bool tk_aligned(const void *p) {
    return (uintptr_t)p % sizeof(float) == 0;
}

static dim3 tk_grid(int B, int h, int w) {
    return dim3((unsigned)(((long)h * w + TK_THREADS - 1) / TK_THREADS), (unsigned)B);
}

#define TK_DISPATCH(K, LAUNCH)  \
    switch (K) {                \
    case 1: LAUNCH(1); break;   \
    case 2: LAUNCH(2); break;   \
    case 3: LAUNCH(3); break;   \
    case 4: LAUNCH(4); break;   \
    case 5: LAUNCH(5); break;   \
    case 6: LAUNCH(6); break;   \
    case 7: LAUNCH(7); break;   \
    default: LAUNCH(8); break;  \
    }

extern "C" int dkt_topk_regress_fwd(const float *cost, long cost_bstride, const float *samples, long samples_bstride, float *out,
                                    unsigned char *idx, int B, int D, int h, int w, int k, int device, void *stream) {
    if (!cost || !out) return DKT_E_NULL;
    const int rc = tk_check(cost_bstride, B, D, h, w, k);
    if (rc != DKT_OK) return rc;
    if (samples && samples_bstride < (long)D * h * w) return DKT_E_SHAPE;
    if (!tk_aligned(cost) || !tk_aligned(samples) || !tk_aligned(out)) return DKT_E_ALIGN;
    DKT_ENTER(device);
    hipStream_t st = (hipStream_t)stream;
#define TK_FWD(K) \
    hipLaunchKernelGGL(tk_fwd_kernel<K>, tk_grid(B, h, w), dim3(TK_THREADS), 0, st, cost, cost_bstride, samples, samples_bstride, out, idx, D, h * w)
    TK_DISPATCH(k, TK_FWD)
#undef TK_FWD
    return dkt_launch_status();
}

extern "C" int dkt_topk_regress_bwd(const float *gout, long gout_bstride, const float *cost, long cost_bstride, const float *samples,
                                    long samples_bstride, const unsigned char *idx, float *gcost, float *gsamples, int B, int D, int h,
                                    int w, int k, int device, void *stream) {
    if (!gout || !cost || !idx || (!gcost && !gsamples) || (gsamples && !samples)) return DKT_E_NULL;
    const int rc = tk_check(cost_bstride, B, D, h, w, k);
    if (rc != DKT_OK) return rc;
    if (gout_bstride < (long)h * w || (samples && samples_bstride < (long)D * h * w)) return DKT_E_SHAPE;
    if (!tk_aligned(gout) || !tk_aligned(cost) || !tk_aligned(samples) || !tk_aligned(gcost) || !tk_aligned(gsamples)) return DKT_E_ALIGN;
    DKT_ENTER(device);
    hipStream_t st = (hipStream_t)stream;
#define TK_BWD(K)                                                                                                                     \
    hipLaunchKernelGGL(tk_bwd_kernel<K>, tk_grid(B, h, w), dim3(TK_THREADS), 0, st, gout, gout_bstride, cost, cost_bstride, samples, \
                       samples_bstride, idx, gcost, gsamples, D, h * w)
    TK_DISPATCH(k, TK_BWD)
#undef TK_BWD
    return dkt_launch_status();
}
