// norm_train.hip -- the feature encoder's instance norms on the training path (BasicEncoder(norm_fn='instance') under
// autograd, core/extractor.py:21-60, :140-146): the gradients of
//   dkt_instance_norm            y   = [relu]((x - mean) * invstd)                  -> dkt_instance_norm_bwd
//   dkt_instance_norm_add_relu   out = relu(a + relu((c - mean_c) * invstd_c))      -> dkt_instance_norm_add_relu_bwd
// torch runs them as a batch-norm backward, a threshold backward and (the join) an add and a second threshold backward,
// each a pass over the activation of its own.
//
// With yh = (x - mean) * invstd recomputed from the saved (mean, 1/std) floats of dkt_instance_norm_finalize -- the
// forward's own pre-ReLU value, bit for bit, so the ReLU mask is the forward's -- and g the masked upstream gradient
// (gy * [yh > 0] for the norm with ReLU; gout * [out > 0] * [yh > 0] for the join):
//   gx = invstd * (g - mean(g) - yh * mean(g * yh))          ga = gout * [out > 0]
// Two launches, both HBM-bound streaming passes (float4 when the plane bases and HW allow, blockIdx.y = plane, no
// per-thread division):
//   sums    per-plane sum(g) and sum(g * yh) in fp64 (the product of two floats is exact in fp64), `split` blocks per
//           plane in the manner of norm.hip's statistics pass so that a few large planes still fill the device; every
//           block writes its partial pair to the workspace;
//   apply   every block adds its plane's partials in slice order (no atomics: the same bits on every run), rounds the
//           two means to fp32 once and writes the gradient with plain fp32 arithmetic:
//           fl(invstd * fl(fl(g - m1) - fl(yh * m2))).
// The join without a gradient for c (gc == NULL) needs no sums: one launch writes ga.
// Plain scalar fp32 (no packed math: DESIGN 3.4).
#include "dkt_common.h"
#include "norm_split.h"
#include "wave_reduce.h"

enum { INB_NORM = 0, INB_NORM_RELU = 1, INB_JOIN = 2 };

// yh and the masked upstream gradient of one element (o: the join's output, unused otherwise)
template <int MODE>
__device__ __forceinline__ void inb_elem(float gy, float x, float o, float mean, float invstd, float &g, float &yh) {
    yh = __fmul_rn(__fsub_rn(x, mean), invstd);
    if (MODE == INB_NORM) g = gy;
    else if (MODE == INB_NORM_RELU) g = yh > 0.0f ? gy : 0.0f;
    else g = (o > 0.0f && yh > 0.0f) ? gy : 0.0f;
}

__device__ __forceinline__ float inb_grad(float g, float yh, float m1, float m2, float invstd) {
    return __fmul_rn(invstd, __fsub_rn(__fsub_rn(g, m1), __fmul_rn(yh, m2)));
}

// slice blockIdx.x of plane blockIdx.y: part[(plane * S + s) * 2 + {0, 1}] = (sum g, sum g * yh) of the slice
template <int MODE>
__global__ __launch_bounds__(256) void inb_sums_kernel(const float *__restrict__ gy, const float *__restrict__ x,
                                                       const float *__restrict__ o, const float *__restrict__ mi,
                                                       double *__restrict__ part, long HW, int S) {
    const int plane = blockIdx.y, s = blockIdx.x;
    const float mean = mi[2 * plane], invstd = mi[2 * plane + 1];
    const float *pg = gy + (long)plane * HW, *px = x + (long)plane * HW;
    const float *po = MODE == INB_JOIN ? o + (long)plane * HW : px;
    const long per = ((HW + S - 1) / S + 3) & ~3L;
    const long lo = (long)s * per;
    long hi = lo + per;
    if (hi > HW) hi = HW;
    double sg = 0.0, sgy = 0.0;
    float g, yh;
    if ((((uintptr_t)pg | (uintptr_t)px | (uintptr_t)po) & 15) == 0 && (HW & 3) == 0) {
#pragma unroll 2
        for (long i = lo + 4L * threadIdx.x; i + 3 < hi; i += 1024) {
            const float4 vg = *(const float4 *)(pg + i), vx = *(const float4 *)(px + i);
            const float4 vo = MODE == INB_JOIN ? *(const float4 *)(po + i) : vx;
            inb_elem<MODE>(vg.x, vx.x, vo.x, mean, invstd, g, yh); sg += (double)g; sgy += (double)g * (double)yh;
            inb_elem<MODE>(vg.y, vx.y, vo.y, mean, invstd, g, yh); sg += (double)g; sgy += (double)g * (double)yh;
            inb_elem<MODE>(vg.z, vx.z, vo.z, mean, invstd, g, yh); sg += (double)g; sgy += (double)g * (double)yh;
            inb_elem<MODE>(vg.w, vx.w, vo.w, mean, invstd, g, yh); sg += (double)g; sgy += (double)g * (double)yh;
        }
    } else {
        for (long i = lo + threadIdx.x; i < hi; i += 256) {
            inb_elem<MODE>(pg[i], px[i], po[i], mean, invstd, g, yh);
            sg += (double)g;
            sgy += (double)g * (double)yh;
        }
    }
    __shared__ double red[2][4];
    sg = block_sum<4>(sg, red[0]);
    sgy = block_sum<4>(sgy, red[1]);
    if (threadIdx.x == 0) {
        part[((long)plane * S + s) * 2] = sg;
        part[((long)plane * S + s) * 2 + 1] = sgy;
    }
}

// the plane's two means from its S partials, added in slice order and rounded to fp32 once
__device__ __forceinline__ void inb_means(const double *__restrict__ part, int plane, int S, long HW, float &m1, float &m2) {
    double sg = 0.0, sgy = 0.0;
    for (int s = 0; s < S; ++s) {
        sg += part[((long)plane * S + s) * 2];
        sgy += part[((long)plane * S + s) * 2 + 1];
    }
    m1 = (float)(sg / (double)HW);
    m2 = (float)(sgy / (double)HW);
}

template <int MODE>
__global__ __launch_bounds__(256) void inb_apply_kernel(const float *__restrict__ gy, const float *__restrict__ x,
                                                        const float *__restrict__ mi, const double *__restrict__ part,
                                                        float *__restrict__ gx, long HW, int S, int blocks_per_plane) {
    const int plane = blockIdx.y;
    const float mean = mi[2 * plane], invstd = mi[2 * plane + 1];
    float m1, m2;
    inb_means(part, plane, S, HW, m1, m2);
    const float *pg = gy + (long)plane * HW, *px = x + (long)plane * HW;
    float *q = gx + (long)plane * HW;
    float g, yh;
    if ((((uintptr_t)pg | (uintptr_t)px | (uintptr_t)q) & 15) == 0 && (HW & 3) == 0) {
        const long stride = (long)blocks_per_plane * 1024;
#pragma unroll 2
        for (long i = blockIdx.x * 1024L + 4L * threadIdx.x; i + 3 < HW; i += stride) {
            const float4 vg = *(const float4 *)(pg + i), vx = *(const float4 *)(px + i);
            float4 r;
            inb_elem<MODE>(vg.x, vx.x, 0.0f, mean, invstd, g, yh); r.x = inb_grad(g, yh, m1, m2, invstd);
            inb_elem<MODE>(vg.y, vx.y, 0.0f, mean, invstd, g, yh); r.y = inb_grad(g, yh, m1, m2, invstd);
            inb_elem<MODE>(vg.z, vx.z, 0.0f, mean, invstd, g, yh); r.z = inb_grad(g, yh, m1, m2, invstd);
            inb_elem<MODE>(vg.w, vx.w, 0.0f, mean, invstd, g, yh); r.w = inb_grad(g, yh, m1, m2, invstd);
            *(float4 *)(q + i) = r;
        }
    } else {
        for (long i = blockIdx.x * 256L + threadIdx.x; i < HW; i += (long)blocks_per_plane * 256) {
            inb_elem<MODE>(pg[i], px[i], 0.0f, mean, invstd, g, yh);
            q[i] = inb_grad(g, yh, m1, m2, invstd);
        }
    }
}

// GA: ga = gout * [out > 0] is written; GC: gc is written (c, mi and part are read only then)
template <bool GA, bool GC>
__global__ __launch_bounds__(256) void inb_join_apply_kernel(const float *__restrict__ gout, const float *__restrict__ out,
                                                             const float *__restrict__ c, const float *__restrict__ mi,
                                                             const double *__restrict__ part, float *__restrict__ ga,
                                                             float *__restrict__ gc, long HW, int S, int blocks_per_plane) {
    const int plane = blockIdx.y;
    float mean = 0.0f, invstd = 1.0f, m1 = 0.0f, m2 = 0.0f;
    if (GC) {
        mean = mi[2 * plane], invstd = mi[2 * plane + 1];
        inb_means(part, plane, S, HW, m1, m2);
    }
    const float *pg = gout + (long)plane * HW, *po = out + (long)plane * HW;
    const float *pc = GC ? c + (long)plane * HW : po;
    float *qa = GA ? ga + (long)plane * HW : nullptr, *qc = GC ? gc + (long)plane * HW : nullptr;
    float g, yh;
    if ((((uintptr_t)pg | (uintptr_t)po | (uintptr_t)pc | (uintptr_t)qa | (uintptr_t)qc) & 15) == 0 && (HW & 3) == 0) {
        const long stride = (long)blocks_per_plane * 1024;
#pragma unroll 2
        for (long i = blockIdx.x * 1024L + 4L * threadIdx.x; i + 3 < HW; i += stride) {
            const float4 vg = *(const float4 *)(pg + i), vo = *(const float4 *)(po + i);
            if (GA) {
                float4 r;
                r.x = vo.x > 0.0f ? vg.x : 0.0f; r.y = vo.y > 0.0f ? vg.y : 0.0f;
                r.z = vo.z > 0.0f ? vg.z : 0.0f; r.w = vo.w > 0.0f ? vg.w : 0.0f;
                *(float4 *)(qa + i) = r;
            }
            if (GC) {
                const float4 vc = *(const float4 *)(pc + i);
                float4 r;
                inb_elem<INB_JOIN>(vg.x, vc.x, vo.x, mean, invstd, g, yh); r.x = inb_grad(g, yh, m1, m2, invstd);
                inb_elem<INB_JOIN>(vg.y, vc.y, vo.y, mean, invstd, g, yh); r.y = inb_grad(g, yh, m1, m2, invstd);
                inb_elem<INB_JOIN>(vg.z, vc.z, vo.z, mean, invstd, g, yh); r.z = inb_grad(g, yh, m1, m2, invstd);
                inb_elem<INB_JOIN>(vg.w, vc.w, vo.w, mean, invstd, g, yh); r.w = inb_grad(g, yh, m1, m2, invstd);
                *(float4 *)(qc + i) = r;
            }
        }
    } else {
        for (long i = blockIdx.x * 256L + threadIdx.x; i < HW; i += (long)blocks_per_plane * 256) {
            const float vg = pg[i], vo = po[i];
            if (GA) qa[i] = vo > 0.0f ? vg : 0.0f;
            if (GC) {
                inb_elem<INB_JOIN>(vg, pc[i], vo, mean, invstd, g, yh);
                qc[i] = inb_grad(g, yh, m1, m2, invstd);
            }
        }
    }
}

extern "C" long dkt_instance_norm_bwd_workspace(int planes, long HW) {
    if (planes <= 0 || HW <= 0) return DKT_E_SHAPE;
    return (long)planes * norm_split(planes, HW) * 2 * (long)sizeof(double);
}

extern "C" int dkt_instance_norm_bwd(const float *gy, const float *x, const float *mean_invstd, int relu, float *gx,
                                     void *workspace, int planes, long HW, int device, void *stream) {
    if (!gy || !x || !mean_invstd || !gx || !workspace) return DKT_E_NULL;
    if (planes <= 0 || HW <= 0 || planes > 65535) return DKT_E_SHAPE;
    DKT_ENTER(device);
    hipStream_t st = (hipStream_t)stream;
    const int S = norm_split(planes, HW);
    const dim3 grid((unsigned)S, (unsigned)planes);
    double *part = (double *)workspace;
    if (relu) {
        hipLaunchKernelGGL(inb_sums_kernel<INB_NORM_RELU>, grid, dim3(256), 0, st, gy, x, (const float *)nullptr, mean_invstd,
                           part, HW, S);
        hipLaunchKernelGGL(inb_apply_kernel<INB_NORM_RELU>, grid, dim3(256), 0, st, gy, x, mean_invstd, (const double *)part,
                           gx, HW, S, S);
    } else {
        hipLaunchKernelGGL(inb_sums_kernel<INB_NORM>, grid, dim3(256), 0, st, gy, x, (const float *)nullptr, mean_invstd,
                           part, HW, S);
        hipLaunchKernelGGL(inb_apply_kernel<INB_NORM>, grid, dim3(256), 0, st, gy, x, mean_invstd, (const double *)part, gx,
                           HW, S, S);
    }
    return dkt_launch_status();
}

extern "C" int dkt_instance_norm_add_relu_bwd(const float *gout, const float *out, const float *c, const float *mean_invstd,
                                              float *ga, float *gc, void *workspace, int planes, long HW, int device,
                                              void *stream) {
    if (!gout || !out || (!ga && !gc)) return DKT_E_NULL;
    if (gc && (!c || !mean_invstd || !workspace)) return DKT_E_NULL;
    if (planes <= 0 || HW <= 0 || planes > 65535) return DKT_E_SHAPE;
    DKT_ENTER(device);
    hipStream_t st = (hipStream_t)stream;
    const int S = norm_split(planes, HW);
    const dim3 grid((unsigned)S, (unsigned)planes);
    double *part = (double *)workspace;
    if (!gc) {                                      // only `a` needs a gradient: no sums, one launch
        hipLaunchKernelGGL((inb_join_apply_kernel<true, false>), grid, dim3(256), 0, st, gout, out, c, mean_invstd,
                           (const double *)part, ga, gc, HW, S, S);
        return dkt_launch_status();
    }
    hipLaunchKernelGGL(inb_sums_kernel<INB_JOIN>, grid, dim3(256), 0, st, gout, c, out, mean_invstd, part, HW, S);
    if (ga)
        hipLaunchKernelGGL((inb_join_apply_kernel<true, true>), grid, dim3(256), 0, st, gout, out, c, mean_invstd,
                           (const double *)part, ga, gc, HW, S, S);
    else
        hipLaunchKernelGGL((inb_join_apply_kernel<false, true>), grid, dim3(256), 0, st, gout, out, c, mean_invstd,
                           (const double *)part, ga, gc, HW, S, S);
    return dkt_launch_status();
}
