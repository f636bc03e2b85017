// ups9.h -- the nine-tap core of the training-path up-samplers, defined once: RAFT's convex up-sampling
// (upsample_train.hip) and IGEV's context up-sampling (context_upsample_train.hip) are the same
// operator on two layouts of the nine planes.  Shared here: the softmax with its bit contract, the 3 x 3 neighbour taps of
// the coarse map, the f-float row accesses, the meeting of the per-row sums of C in LDS, the launch that gathers C into the
// coarse gradient, and the host checks.  The kernels that read the nine planes stay in their own files.
// Plain scalar fp32 (no packed math: DESIGN 3.4).
#pragma once
#include "dkt_common.h"

// The softmax of convex_upsample_kernel (upsample.hip) in place, the same bits: max, expf(fl(m - max)), the sum in
// ascending k, nine IEEE divisions.  The divisions are the compiler's own sequence for a / b (reciprocal estimate, one
// Newton step on it, the quotient and two fused corrections) written out, so that the steps that depend on the divisor
// alone are done once for the nine quotients.  The compiler's sequence differs from this one only by v_div_scale /
// v_div_fixup, which leave the operands and the result as they are unless the divisor or the quotient is near the ends of
// the exponent range: here 1 <= sum <= 9 (the largest logit contributes exactly 1), so that happens only for a numerator
// below 2^-103, and every numerator below 2^-100 other than 0 takes the plain division.
__device__ __forceinline__ void ups9_softmax(float (&m)[9]) {
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
    if (__builtin_expect(tiny, 0)) {                                        // a spread of the logits beyond 69
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

// The taps ff * map[d, h + k/3 - 1, w + k%3 - 1] (0 outside) of one coarse pixel for the channels d[0..NC) of one image
// (fn: its first plane, HW floats per plane), in two steps: the loads, unconditional (clamped index) so that all 9 * NC
// are in flight together with the plane loads the caller issues next, and the finish (zero padding as a select, the
// factor; channels that are not `on` give 0).  (Left to itself the compiler sinks each load under its bounds test: one
// branch and one full wait per tap.  The empty asm of the finish makes each loaded value count as used where it stands.)
template <int NC>
__device__ __forceinline__ void ups9_taps_load(const float *__restrict__ fn, long HW, const int (&d)[NC], int h, int w, int H,
                                               int W, float (&x)[NC][9]) {
#pragma unroll
    for (int dd = 0; dd < NC; ++dd)
#pragma unroll
        for (int k = 0; k < 9; ++k)
            x[dd][k] = fn[d[dd] * HW + (long)min(max(h + k / 3 - 1, 0), H - 1) * W + min(max(w + k % 3 - 1, 0), W - 1)];
}

template <int NC>
__device__ __forceinline__ void ups9_taps_finish(float (&x)[NC][9], const bool (&on)[NC], int h, int w, int H, int W, float ff) {
#pragma unroll
    for (int dd = 0; dd < NC; ++dd)
#pragma unroll
        for (int k = 0; k < 9; ++k) asm volatile("" : "+v"(x[dd][k]));
#pragma unroll
    for (int dd = 0; dd < NC; ++dd)
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int hh = h + k / 3 - 1, ww = w + k % 3 - 1;
            x[dd][k] = (on[dd] && hh >= 0 && hh < H && ww >= 0 && ww < W) ? __fmul_rn(ff, x[dd][k]) : 0.0f;
        }
}

// F contiguous floats as one access of min(4 F, 16) bytes (two of 16 for F = 8)
template <int F>
__device__ __forceinline__ void ups9_load_row(const float *__restrict__ p, float (&v)[F]) {
    if constexpr (F == 1) {
        v[0] = p[0];
    } else if constexpr (F == 2) {
        const float2 t = *reinterpret_cast<const float2 *>(p);
        v[0] = t.x, v[1] = t.y;
    } else {
#pragma unroll
        for (int q = 0; q < F / 4; ++q) {
            const float4 t = reinterpret_cast<const float4 *>(p)[q];
            v[4 * q] = t.x, v[4 * q + 1] = t.y, v[4 * q + 2] = t.z, v[4 * q + 3] = t.w;
        }
    }
}

template <int F>
__device__ __forceinline__ void ups9_store_row(float *__restrict__ p, const float (&v)[F]) {
    if constexpr (F == 1) {
        p[0] = v[0];
    } else if constexpr (F == 2) {
        *reinterpret_cast<float2 *>(p) = make_float2(v[0], v[1]);
    } else {
#pragma unroll
        for (int q = 0; q < F / 4; ++q)
            reinterpret_cast<float4 *>(p)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    }
}

// The row sums of C meet here, in a block of F waves over 64 coarse pixels of image n (wave i = fine row i):
// red[i][dd * 9 + k][lane] <- c[dd][k], and one thread per (dd, k, lane) adds them in ascending i into
// ws[((n * Dout + d0 + dd) * 9 + k) * HW + pixel].  Every thread of the block has to come here.
template <int F, int NC>
__device__ __forceinline__ void ups9_reduce_rows(float (&red)[F][NC * 9][64], const float (&c)[NC][9], int i, int lane,
                                                 float *ws, int n, int Dout, int d0, long HW) {
#pragma unroll
    for (int dd = 0; dd < NC; ++dd)
#pragma unroll
        for (int k = 0; k < 9; ++k) red[i][dd * 9 + k][lane] = c[dd][k];
    __syncthreads();
    for (int e = threadIdx.x; e < NC * 9 * 64; e += 64 * F) {
        const int q = e >> 6, l = e & 63, dd = NC == 1 ? 0 : q / 9, k = q - dd * 9;
        const int pp = blockIdx.x * 64 + l;                                 // H * W < 2^31 - 256 (ups9_check)
        if (d0 + dd >= Dout || pp >= HW) continue;
        float s = red[0][q][l];
#pragma unroll
        for (int r = 1; r < F; ++r) s = __fadd_rn(s, red[r][q][l]);
        ws[(((long)n * Dout + d0 + dd) * 9 + k) * HW + pp] = s;
    }
}

// The second launch.  thread = one element of plane (blockIdx.z, blockIdx.y) = (n, d) of the coarse gradient: its (up to
// 9) in-image terms of C in ascending k, times ff; channels d >= Dout get an exact 0.  static: each unit that launches it
// carries its own copy.
static __global__ __launch_bounds__(256) void ups9_gather_kernel(const float *__restrict__ ws, float *__restrict__ gflow, int Dout,
                                                                 int H, int W, float ff) {
    const int HW = H * W, D = gridDim.y, d = blockIdx.y, n = blockIdx.z;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int y = p / W, x = p - y * W;
    float s = 0.0f;
    if (d < Dout) {                                                         // uniform
        const float *cp = ws + ((long)n * Dout + d) * 9 * HW;
        float t[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {                                       // clamped loads, the padding a select
            const int hh = y - k / 3 + 1, ww = x - k % 3 + 1;
            t[k] = cp[(long)k * HW + min(max(hh, 0), H - 1) * W + min(max(ww, 0), W - 1)];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int hh = y - k / 3 + 1, ww = x - k % 3 + 1;
            if (hh >= 0 && hh < H && ww >= 0 && ww < W) s = __fadd_rn(s, t[k]);
        }
        s = __fmul_rn(ff, s);
    }
    gflow[((long)n * D + d) * HW + p] = s;
}

// ---- host side: what every entry checks.  Each entry keeps its own order of checks (the return codes are pinned).
// sign, then the limits of grid.y / grid.z and of the int pixel indices
static int ups9_check(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return DKT_E_SHAPE;
    if (N > 65535 || (long)H * W > 0x7fffffffL - 256) return DKT_E_UNSUPPORTED;
    return DKT_OK;
}

static bool ups9_aligned(const void *p, size_t bytes = 16) {
    return (uintptr_t)p % bytes == 0;
}

// blocks of 64 coarse pixels of one image (the F-wave kernels)
static dim3 ups9_grid(int N, int H, int W) {
    return dim3((unsigned)(((long)H * W + 63) / 64), (unsigned)N);
}

// C (N, Dout, 9, H, W) -> g (N, D, H, W), blocks of 256 elements of one plane
static void ups9_gather(const float *ws, float *g, int N, int D, int Dout, int H, int W, float ff, hipStream_t st) {
    hipLaunchKernelGGL(ups9_gather_kernel, dim3((unsigned)(((long)H * W + 255) / 256), (unsigned)D, (unsigned)N), dim3(256), 0, st,
                       ws, g, Dout, H, W, ff);
}
