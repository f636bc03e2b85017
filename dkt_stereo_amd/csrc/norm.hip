// norm.hip -- streaming helpers around the convolutions (HBM-bound, float4, grid-stride):
//   dkt_instance_norm   InstanceNorm2d(affine=False) [+ ReLU], two launches
//   dkt_add_relu        relu(a + b), the residual join of core/extractor.py:60
//   dkt_pool2x          avg_pool2d(x, 3, stride=2, padding=1)          core/update.py:87-88
//   dkt_interp2x        bilinear resize, align_corners=True             core/update.py:93-95
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

// avg_pool2d(x, 3, stride=2, padding=1), count_include_pad=True (divide by 9 always).
// Sum order: rows top to bottom, columns left to right (ATen's loop order), then * (1/9)?
// ATen divides the sum by the pool size: sum / 9.
// grid.y = output row of a plane (plane * Ho + oy), threads along ox: no per-thread division; the nine loads are
// unconditional (clamped index, zero selected afterwards -- s + 0.0f is s) and in flight together.
__global__ __launch_bounds__(256) void pool2x_kernel(const float *__restrict__ x, float *__restrict__ y,
                                                     int H, int W, int Ho, int Wo, long planes) {
    const int ox = blockIdx.x * 256 + threadIdx.x;
    if (ox >= Wo) return;
    constexpr int RB = 4;                                  // output rows per step: 36 loads in flight per thread
    const long nrows = planes * Ho;
    for (long row0 = (long)blockIdx.y * RB; row0 < nrows; row0 += (long)gridDim.y * RB) {
        float v[RB][9];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const long row = min(row0 + r, nrows - 1);
            const long pl = row / Ho;                      // block-uniform
            const int oy = (int)(row - pl * Ho);
            const float *p = x + pl * H * W;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const int iy = 2 * oy - 1 + dy;
                const bool yok = iy >= 0 && iy < H;
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int ix = 2 * ox - 1 + dx;
                    const bool ok = yok && ix >= 0 && ix < W;
                    const float t = p[(long)(yok ? iy : 0) * W + (ix >= 0 && ix < W ? ix : 0)];
                    v[r][dy * 3 + dx] = ok ? t : 0.0f;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            if (row0 + r >= nrows) break;
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < 9; ++k) s = __fadd_rn(s, v[r][k]);
            y[(row0 + r) * Wo + ox] = __fdiv_rn(s, 9.0f);
        }
    }
}

extern "C" int dkt_pool2x(const float *x, float *y, long planes, int H, int W, int device, void *stream) {
    if (!x || !y) return DKT_E_NULL;
    if (planes <= 0 || H <= 0 || W <= 0) return DKT_E_SHAPE;
    DKT_ENTER(device);
    const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    // (an LDS-staged form like interp_lds_kernel measured 11.7 us against 12.2 us: 36.7 MB in a launch this short is
    // already at ~3.1 TB/s -- not kept)
    long rows = (planes * Ho + 3) / 4;                     // 4 output rows per block step
    if (rows > 65535) rows = 65535;
    hipLaunchKernelGGL(pool2x_kernel, dim3((unsigned)((Wo + 255) / 256), (unsigned)rows), dim3(256), 0, (hipStream_t)stream,
                       x, y, H, W, Ho, Wo, planes);
    return dkt_launch_status();
}

// F.interpolate(x, (Ho,Wo), mode='bilinear', align_corners=True): ATen's
//   src = dst * (in-1)/(out-1);  i0 = (int)src;  l1 = src - i0;  l0 = 1 - l1
//   out = l0y*(l0x*v00 + l1x*v01) + l1y*(l0x*v10 + l1x*v11)
// One thread = 4 adjacent outputs of one row (float4 store when Wo % 4 == 0); the row weights
// and the two source-row pointers are shared by the four.
// grid.y = output row of a plane, threads along quads of ox: no per-thread division.
__global__ __launch_bounds__(128) void interp_kernel(const float *__restrict__ x, float *__restrict__ y,
                                                     int H, int W, int Ho, int Wo, float sy, float sx, long planes) {
    const int Wq = (Wo + 3) / 4;
    const int oq = blockIdx.x * 128 + threadIdx.x;
    if (oq >= Wq) return;
    const bool vec = (Wo & 3) == 0 && (((uintptr_t)y) & 15) == 0;
    // the four columns' source indices and weights do not depend on the row
    int x0[4], x1[4];
    float lx0[4], lx1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ox = min(4 * oq + k, Wo - 1);
        const float fx = __fmul_rn(sx, (float)ox);
        x0[k] = (int)fx;
        x1[k] = x0[k] + (x0[k] < W - 1 ? 1 : 0);
        lx1[k] = __fsub_rn(fx, (float)x0[k]);
        lx0[k] = __fsub_rn(1.0f, lx1[k]);
    }
    constexpr int RB = 4;                                  // output rows per step: 16 loads per row in flight together
    const long nrows = planes * Ho;
    for (long row0 = (long)blockIdx.y * RB; row0 < nrows; row0 += (long)gridDim.y * RB) {
        float a0[RB][4], a1[RB][4], b0[RB][4], b1[RB][4], ly0[RB], ly1[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const long row = min(row0 + r, nrows - 1);
            const long pl = row / Ho;                      // block-uniform
            const int oy = (int)(row - pl * Ho);
            const float *p = x + pl * H * W;
            const float fy = __fmul_rn(sy, (float)oy);
            const int y0 = (int)fy;
            const int y1 = y0 + (y0 < H - 1 ? 1 : 0);
            ly1[r] = __fsub_rn(fy, (float)y0);
            ly0[r] = __fsub_rn(1.0f, ly1[r]);
            const float *r0 = p + (long)y0 * W, *r1 = p + (long)y1 * W;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                a0[r][k] = r0[x0[k]]; a1[r][k] = r0[x1[k]];
                b0[r][k] = r1[x0[k]]; b1[r][k] = r1[x1[k]];
            }
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const long row = row0 + r;
            if (row >= nrows) break;
            float o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float top = __fadd_rn(__fmul_rn(lx0[k], a0[r][k]), __fmul_rn(lx1[k], a1[r][k]));
                const float bot = __fadd_rn(__fmul_rn(lx0[k], b0[r][k]), __fmul_rn(lx1[k], b1[r][k]));
                o[k] = __fadd_rn(__fmul_rn(ly0[r], top), __fmul_rn(ly1[r], bot));
            }
            float *q = y + row * (long)Wo + 4 * oq;
            if (vec) {
                *(float4 *)q = make_float4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (4 * oq + k < Wo) q[k] = o[k];
            }
        }
    }
}

// LDS-staged form for up-sampling (the loop's 1/8 -> 1/4 and 1/16 -> 1/8 resizes): a block produces INTERP_RB
// consecutive output rows of one plane; the <= INTERP_SR source rows they blend are copied to LDS once with 16-byte
// loads (the gather form above issues 16 scalar loads per output quad: 23 us for a 29 MB result), and every
// (row, output quad) item reads its 2 x 2 x 4 taps from there.  Same arithmetic, same order: bit-identical.
#define INTERP_RB 8
#define INTERP_SR 8
#define INTERP_MAXW 640
__global__ __launch_bounds__(256) void interp_lds_kernel(const float *__restrict__ x, float *__restrict__ y,
                                                         int H, int W, int Ho, int Wo, float sy, float sx) {
    __shared__ __attribute__((aligned(16))) float rows[INTERP_SR * INTERP_MAXW];
    const int rb_per_plane = (Ho + INTERP_RB - 1) / INTERP_RB;
    const long pl = blockIdx.x / rb_per_plane;
    const int oy0 = (int)(blockIdx.x - pl * rb_per_plane) * INTERP_RB;
    const int nr = min(INTERP_RB, Ho - oy0);
    const float *p = x + pl * (long)H * W;
    const int ylo = (int)__fmul_rn(sy, (float)oy0);
    const int ylast = (int)__fmul_rn(sy, (float)(oy0 + nr - 1));
    const int yhi = ylast + (ylast < H - 1 ? 1 : 0);
    const int ns = yhi - ylo + 1;                          // <= INTERP_SR (checked by the host for this scale)
    const int W4 = W >> 2;
    for (int i = threadIdx.x; i < ns * W4; i += 256) {
        const int r = i / W4, q = i - r * W4;
        *(float4 *)(rows + r * INTERP_MAXW + 4 * q) = *(const float4 *)(p + (long)(ylo + r) * W + 4 * q);
    }
    __syncthreads();
    const int Wq = Wo >> 2;
    for (int item = threadIdx.x; item < nr * Wq; item += 256) {
        const int r = item / Wq, oq = item - r * Wq;
        const int oy = oy0 + r;
        const float fy = __fmul_rn(sy, (float)oy);
        const int y0 = (int)fy;
        const int y1 = y0 + (y0 < H - 1 ? 1 : 0);
        const float ly1 = __fsub_rn(fy, (float)y0), ly0 = __fsub_rn(1.0f, ly1);
        const float *r0 = rows + (y0 - ylo) * INTERP_MAXW, *r1 = rows + (y1 - ylo) * INTERP_MAXW;
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ox = 4 * oq + k;
            const float fx = __fmul_rn(sx, (float)ox);
            const int x0 = (int)fx;
            const int x1 = x0 + (x0 < W - 1 ? 1 : 0);
            const float lx1 = __fsub_rn(fx, (float)x0), lx0 = __fsub_rn(1.0f, lx1);
            const float top = __fadd_rn(__fmul_rn(lx0, r0[x0]), __fmul_rn(lx1, r0[x1]));
            const float bot = __fadd_rn(__fmul_rn(lx0, r1[x0]), __fmul_rn(lx1, r1[x1]));
            o[k] = __fadd_rn(__fmul_rn(ly0, top), __fmul_rn(ly1, bot));
        }
        *(float4 *)(y + (pl * Ho + oy) * (long)Wo + 4 * oq) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

extern "C" int dkt_interp_bilinear(const float *x, float *y, long planes, int H, int W, int Ho, int Wo,
                                   int device, void *stream) {
    if (!x || !y) return DKT_E_NULL;
    if (planes <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return DKT_E_SHAPE;
    DKT_ENTER(device);
    const float sy = Ho > 1 ? (float)(H - 1) / (float)(Ho - 1) : 0.0f;
    const float sx = Wo > 1 ? (float)(W - 1) / (float)(Wo - 1) : 0.0f;
    // up-sampling with 16-byte aligned rows: the LDS-staged form.  INTERP_RB output rows blend at most
    // floor((INTERP_RB - 1) * sy) + 3 source rows.
    const long nblk = planes * ((Ho + INTERP_RB - 1) / INTERP_RB);
    if (W % 4 == 0 && Wo % 4 == 0 && W <= INTERP_MAXW && sy <= 1.0f && sx <= 1.0f
        && (int)((INTERP_RB - 1) * sy) + 3 <= INTERP_SR && nblk <= 0x7fffffffL
        && ((((uintptr_t)x) | ((uintptr_t)y)) & 15) == 0) {
        hipLaunchKernelGGL(interp_lds_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, x, y, H, W, Ho, Wo, sy, sx);
        return dkt_launch_status();
    }
    long rows = (planes * Ho + 3) / 4;                     // 4 output rows per block step
    if (rows > 65535) rows = 65535;
    const int Wq = (Wo + 3) / 4;
    hipLaunchKernelGGL(interp_kernel, dim3((unsigned)((Wq + 127) / 128), (unsigned)rows), dim3(128), 0, (hipStream_t)stream,
                       x, y, H, W, Ho, Wo, sy, sx, planes);
    return dkt_launch_status();
}
