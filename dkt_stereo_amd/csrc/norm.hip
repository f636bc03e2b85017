// norm.hip -- streaming helpers around the convolutions (HBM-bound, float4, grid-stride):
//   dkt_instance_norm   InstanceNorm2d(affine=False) [+ ReLU], two launches
//   dkt_add_relu        relu(a + b), the residual join of core/extractor.py:60
// torch runs instance norm as collect_statistics (100 us) + transform_input (224 us) + a
// separate ReLU (28 us) on a 235 MB activation; here it is one statistics pass (fp64
// partial sums, several blocks per plane so that 128 planes still fill 256 CUs) and one
// normalise(+ReLU) pass.
#include "dkt_common.h"
#include "norm_split.h"
#include "wave_reduce.h"

__global__ __launch_bounds__(256) void instnorm_stats_kernel(const float *__restrict__ x,
                                                             double *__restrict__ part, long HW, int S) {
    const int plane = blockIdx.y, s = blockIdx.x;
    const float *p = x + (long)plane * HW;
    const long per = ((HW + S - 1) / S + 3) & ~3L;
    const long lo = (long)s * per;
    long hi = lo + per;
    if (hi > HW) hi = HW;
    double sum = 0.0, sq = 0.0;
    if (((uintptr_t)p & 15) == 0 && (HW & 3) == 0) {
        for (long i = lo + 4L * threadIdx.x; i + 3 < hi; i += 1024) {
            const float4 v = *(const float4 *)(p + i);
            sum += (double)v.x + (double)v.y + (double)v.z + (double)v.w;
            sq += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
        }
    } else {
        for (long i = lo + threadIdx.x; i < hi; i += 256) {
            const float v = p[i];
            sum += v;
            sq += (double)v * v;
        }
    }
    __shared__ double red[2][4];
    sum = block_sum<4>(sum, red[0]);
    sq = block_sum<4>(sq, red[1]);
    if (threadIdx.x == 0) {
        part[((long)plane * S + s) * 2] = sum;
        part[((long)plane * S + s) * 2 + 1] = sq;
    }
}

__global__ __launch_bounds__(256) void instnorm_apply_kernel(const float *__restrict__ x, float *__restrict__ y,
                                                             const double *__restrict__ part, long HW, int S,
                                                             float eps, int relu, int blocks_per_plane) {
    const int plane = blockIdx.y;
    double sum = 0.0, sq = 0.0;
    for (int s = 0; s < S; ++s) {
        sum += part[((long)plane * S + s) * 2];
        sq += part[((long)plane * S + s) * 2 + 1];
    }
    const double mean_d = sum / (double)HW;
    double var_d = sq / (double)HW - mean_d * mean_d;      // biased variance, as instance_norm uses
    if (var_d < 0.0) var_d = 0.0;
    const float mean = (float)mean_d;
    const float invstd = 1.0f / sqrtf((float)var_d + eps);
    const float *p = x + (long)plane * HW;
    float *q = y + (long)plane * HW;
    const long stride = (long)blocks_per_plane * 1024;
    if (((uintptr_t)p & 15) == 0 && ((uintptr_t)q & 15) == 0 && (HW & 3) == 0) {
        for (long i = blockIdx.x * 1024L + 4L * threadIdx.x; i + 3 < HW; i += stride) {
            float4 v = *(const float4 *)(p + i);
            v.x = (v.x - mean) * invstd; v.y = (v.y - mean) * invstd;
            v.z = (v.z - mean) * invstd; v.w = (v.w - mean) * invstd;
            if (relu) {
                v.x = dkt_relu(v.x); v.y = dkt_relu(v.y); v.z = dkt_relu(v.z); v.w = dkt_relu(v.w);
            }
            *(float4 *)(q + i) = v;
        }
    } else {
        for (long i = blockIdx.x * 256L + threadIdx.x; i < HW; i += (long)blocks_per_plane * 256) {
            float v = (p[i] - mean) * invstd;
            q[i] = relu ? dkt_relu(v) : v;
        }
    }
}

extern "C" long dkt_instance_norm_workspace(int planes, long HW) {
    if (planes <= 0 || HW <= 0) return DKT_E_SHAPE;
    return (long)planes * NORM_SPLIT_MAX * 2 * (long)sizeof(double);
}

// Statistics accumulated by a convolution's epilogue (conv2d.hip, ConvArgs.stats_ws: per (batch, entry, channel) fp32 sums
// and sums of squares) folded into the partial-sum workspace the kernels above read, part[(plane * S + s) * 2 + {0, 1}]:
// one block per plane writes the plane's fp64 totals to partial 0 and zeroes the other S - 1.
// The epilogue's sums are fp32, and E[x^2] - mean^2 cancels when a plane's mean is much larger than its spread: 1/std is off
// by ~5e-7 at mean / sigma = 10, 3e-5 at 100, 2e-3 at 1000, and the variance of a small plane at 10^4 goes negative.  A plane
// with mean^2 > CONV_STATS_TRUST * var (or a negative / NaN variance) is therefore recomputed by the same block from the
// stored output with fp64 squares, the arithmetic of instnorm_stats_kernel: a full read of that plane, only for such planes.
#define CONV_STATS_TRUST 16.0
__global__ __launch_bounds__(256) void conv_stats_reduce_kernel(const float *__restrict__ ws, double *__restrict__ part,
                                                                int C, long E, int S, const float *__restrict__ out,
                                                                long out_bs, long HW) {
    const int plane = blockIdx.x;
    const int b = plane / C, c = plane - b * C;
    __shared__ double red[2][4];
    double sum = 0.0, sq = 0.0;
    for (long e = threadIdx.x; e < E; e += 256) {
        const float2 v = *(const float2 *)(ws + (((long)b * E + e) * C + c) * 2);
        sum += (double)v.x;
        sq += (double)v.y;
    }
    sum = block_sum<4>(sum, red[0]);
    sq = block_sum<4>(sq, red[1]);
    const double mean = sum / (double)HW, var = sq / (double)HW - mean * mean;
    if (!(mean * mean <= CONV_STATS_TRUST * var)) {         // block-uniform (also true for a NaN or a negative variance)
        const float *p = out + (long)b * out_bs + (long)c * HW;
        sum = sq = 0.0;
        if (((uintptr_t)p & 15) == 0 && (HW & 3) == 0) {
            for (long i = 4L * threadIdx.x; i < HW; i += 1024) {
                const float4 v = *(const float4 *)(p + i);
                sum += (double)v.x + (double)v.y + (double)v.z + (double)v.w;
                sq += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
            }
        } else {
            for (long i = threadIdx.x; i < HW; i += 256) {
                const double v = p[i];
                sum += v;
                sq += v * v;
            }
        }
        sum = block_sum<4>(sum, red[0]);
        sq = block_sum<4>(sq, red[1]);
    }
    for (int s = threadIdx.x; s < S; s += 256) {
        part[((long)plane * S + s) * 2] = s ? 0.0 : sum;
        part[((long)plane * S + s) * 2 + 1] = s ? 0.0 : sq;
    }
}

int conv_stats_reduce(const float *ws, double *part, int B, int C, long entries, long HW, const float *out, long out_bs,
                      hipStream_t st) {
    const long planes = (long)B * C;
    if (planes <= 0 || planes > 65535 || entries <= 0) return DKT_E_SHAPE;
    const int S = norm_split((int)planes, HW);
    hipLaunchKernelGGL(conv_stats_reduce_kernel, dim3((unsigned)planes), dim3(256), 0, st, ws, part, C, entries, S, out,
                       out_bs, HW);
    return dkt_launch_status();
}

extern "C" int dkt_instance_norm_stats(const float *x, void *workspace, int planes, long HW, int device, void *stream) {
    if (!x || !workspace) return DKT_E_NULL;
    if (planes <= 0 || HW <= 0 || planes > 65535) return DKT_E_SHAPE;
    DKT_ENTER(device);
    const int S = norm_split(planes, HW);
    hipLaunchKernelGGL(instnorm_stats_kernel, dim3((unsigned)S, (unsigned)planes), dim3(256), 0, (hipStream_t)stream,
                       x, (double *)workspace, HW, S);
    return dkt_launch_status();
}

extern "C" int dkt_instance_norm(const float *x, float *y, void *workspace, int planes, long HW,
                                 float eps, int relu, int device, void *stream) {
    if (!x || !y || !workspace) return DKT_E_NULL;
    if (planes <= 0 || HW <= 0 || planes > 65535) return DKT_E_SHAPE;
    int rc = dkt_instance_norm_stats(x, workspace, planes, HW, device, stream);
    if (rc) return rc;
    DKT_ENTER(device);
    const int S = norm_split(planes, HW);
    hipLaunchKernelGGL(instnorm_apply_kernel, dim3((unsigned)S, (unsigned)planes), dim3(256), 0, (hipStream_t)stream,
                       x, y, (const double *)workspace, HW, S, eps, relu ? 1 : 0, S);
    return dkt_launch_status();
}

// (mean, 1/std) per plane as two floats -- the form the convolution kernel's staging takes
// (dkt_conv_desc.in_norm): the normalise(+ReLU) pass between two layers disappears.  Same
// arithmetic as instnorm_apply_kernel's prologue.
__global__ __launch_bounds__(256) void instnorm_finalize_kernel(const double *__restrict__ part, float *__restrict__ out,
                                                                int planes, long HW, int S, float eps) {
    const int plane = blockIdx.x * 256 + threadIdx.x;
    if (plane >= planes) return;
    double sum = 0.0, sq = 0.0;
    for (int s = 0; s < S; ++s) {
        sum += part[((long)plane * S + s) * 2];
        sq += part[((long)plane * S + s) * 2 + 1];
    }
    const double mean_d = sum / (double)HW;
    double var_d = sq / (double)HW - mean_d * mean_d;
    if (var_d < 0.0) var_d = 0.0;
    out[2 * plane] = (float)mean_d;
    out[2 * plane + 1] = 1.0f / sqrtf((float)var_d + eps);
}

extern "C" int dkt_instance_norm_finalize(const void *workspace, int planes, long HW, float eps, float *mean_invstd,
                                          int device, void *stream) {
    if (!workspace || !mean_invstd) return DKT_E_NULL;
    if (planes <= 0 || HW <= 0 || planes > 65535) return DKT_E_SHAPE;
    DKT_ENTER(device);
    const int S = norm_split(planes, HW);
    hipLaunchKernelGGL(instnorm_finalize_kernel, dim3((unsigned)((planes + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const double *)workspace, mean_invstd, planes, HW, S, eps);
    return dkt_launch_status();
}

// The tail of a residual block with instance norm (core/extractor.py:52-60) in one pass:
//   y = relu(a + relu((c - mean_c) * invstd_c)),  statistics of c from dkt_instance_norm_stats.
// Replaces the normalise(+ReLU) pass over c and the separate add+ReLU pass.
__global__ __launch_bounds__(256) void instnorm_add_relu_kernel(const float *__restrict__ a, const float *__restrict__ c,
                                                                float *__restrict__ y, const double *__restrict__ part,
                                                                long HW, int S, float eps, int blocks_per_plane,
                                                                const float *__restrict__ a_norm, int a_relu) {
    const int plane = blockIdx.y;
    double sum = 0.0, sq = 0.0;
    for (int s = 0; s < S; ++s) {
        sum += part[((long)plane * S + s) * 2];
        sq += part[((long)plane * S + s) * 2 + 1];
    }
    const double mean_d = sum / (double)HW;
    double var_d = sq / (double)HW - mean_d * mean_d;
    if (var_d < 0.0) var_d = 0.0;
    const float mean = (float)mean_d;
    const float invstd = 1.0f / sqrtf((float)var_d + eps);
    // the residual operand may itself be a not-yet-normalised tensor: a' = [relu]((a - mean_a) * invstd_a)
    const bool an = a_norm != nullptr;
    const float am = an ? a_norm[2 * plane] : 0.0f, ai = an ? a_norm[2 * plane + 1] : 1.0f;
    auto res = [&](float u) {
        if (!an) return u;
        const float t = (u - am) * ai;
        return a_relu ? dkt_relu(t) : t;
    };
    const float *pa = a + (long)plane * HW, *pc = c + (long)plane * HW;
    float *q = y + (long)plane * HW;
    const long stride = (long)blocks_per_plane * 1024;
    if ((((uintptr_t)pa | (uintptr_t)pc | (uintptr_t)q) & 15) == 0 && (HW & 3) == 0) {
        for (long i = blockIdx.x * 1024L + 4L * threadIdx.x; i + 3 < HW; i += stride) {
            const float4 u = *(const float4 *)(pa + i);
            float4 v = *(const float4 *)(pc + i);
            v.x = dkt_relu(res(u.x) + dkt_relu((v.x - mean) * invstd));
            v.y = dkt_relu(res(u.y) + dkt_relu((v.y - mean) * invstd));
            v.z = dkt_relu(res(u.z) + dkt_relu((v.z - mean) * invstd));
            v.w = dkt_relu(res(u.w) + dkt_relu((v.w - mean) * invstd));
            *(float4 *)(q + i) = v;
        }
    } else {
        for (long i = blockIdx.x * 256L + threadIdx.x; i < HW; i += (long)blocks_per_plane * 256)
            q[i] = dkt_relu(res(pa[i]) + dkt_relu((pc[i] - mean) * invstd));
    }
}

static int instnorm_add_relu_impl(const float *a, const float *a_norm, int a_relu, const float *c, float *y,
                                  const void *workspace, int planes, long HW, float eps, int device, void *stream) {
    if (!a || !c || !y || !workspace) return DKT_E_NULL;
    if (planes <= 0 || HW <= 0 || planes > 65535) return DKT_E_SHAPE;
    DKT_ENTER(device);
    const int S = norm_split(planes, HW);
    hipLaunchKernelGGL(instnorm_add_relu_kernel, dim3((unsigned)S, (unsigned)planes), dim3(256), 0, (hipStream_t)stream,
                       a, c, y, (const double *)workspace, HW, S, eps, S, a_norm, a_relu ? 1 : 0);
    return dkt_launch_status();
}

extern "C" int dkt_instance_norm_add_relu(const float *a, const float *c, float *y, const void *workspace,
                                          int planes, long HW, float eps, int device, void *stream) {
    return instnorm_add_relu_impl(a, nullptr, 0, c, y, workspace, planes, HW, eps, device, stream);
}

extern "C" int dkt_instance_norm_add_relu_lazy(const float *a, const float *a_mean_invstd, int a_relu, const float *c,
                                               float *y, const void *workspace, int planes, long HW, float eps,
                                               int device, void *stream) {
    if (!a_mean_invstd) return DKT_E_NULL;
    return instnorm_add_relu_impl(a, a_mean_invstd, a_relu, c, y, workspace, planes, HW, eps, device, stream);
}

__global__ __launch_bounds__(256) void add_relu_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                       float *__restrict__ y, long n4, long n) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const float4 u = ((const float4 *)a)[i], v = ((const float4 *)b)[i];
        float4 o;
        o.x = dkt_relu(u.x + v.x); o.y = dkt_relu(u.y + v.y);
        o.z = dkt_relu(u.z + v.z); o.w = dkt_relu(u.w + v.w);
        ((float4 *)y)[i] = o;
    }
    for (long i = n4 * 4 + blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        y[i] = dkt_relu(a[i] + b[i]);
}

extern "C" int dkt_add_relu(const float *a, const float *b, float *y, long n, int device, void *stream) {
    if (!a || !b || !y) return DKT_E_NULL;
    if (n <= 0) return DKT_E_SHAPE;
    DKT_ENTER(device);
    const bool al = ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)y)) & 15) == 0;
    const long n4 = al ? n / 4 : 0;
    long blocks = ((al ? n4 : n) + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(add_relu_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, b, y, n4, n);
    return dkt_launch_status();
}
