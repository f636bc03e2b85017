// resample.h -- the arithmetic of the update block's two resamplers (core/update.py:87-95), one definition for the fp32
// kernels and their gradients (resample.hip) and for the C8S kernels (resample_c8.hip), so that all of them compile the
// same operations in the same order.  Each helper is one stage -- taps, loads, blend -- so that a kernel may batch the
// loads of several outputs ahead of their arithmetic.
#pragma once
#include "dkt_common.h"

// F.interpolate(x, (Ho, Wo), mode='bilinear', align_corners=True), ATen's arithmetic per axis:
//   src = dst * (in-1)/(out-1);  i0 = (int)src;  l1 = src - i0;  l0 = 1 - l1
struct DktLerp {
    int i0, i1;      // source indices, i1 == i0 at the last one
    float l0, l1;    // their weights
};

// output o of an axis with N source elements, s = (N - 1) / (No - 1) rounded once on the host (0 when No == 1)
__device__ __forceinline__ DktLerp dkt_lerp(int o, float s, int N) {
    DktLerp t;
    const float f = __fmul_rn(s, (float)o);
    t.i0 = (int)f;
    t.i1 = t.i0 + (t.i0 < N - 1 ? 1 : 0);
    t.l1 = __fsub_rn(f, (float)t.i0);
    t.l0 = __fsub_rn(1.0f, t.l1);
    return t;
}

//   out = l0y*(l0x*v00 + l1x*v01) + l1y*(l0x*v10 + l1x*v11),  v<row tap><column tap>
__device__ __forceinline__ float dkt_lerp_blend(const DktLerp &ty, const DktLerp &tx, float v00, float v01, float v10,
                                                float v11) {
    const float top = __fadd_rn(__fmul_rn(tx.l0, v00), __fmul_rn(tx.l1, v01));
    const float bot = __fadd_rn(__fmul_rn(tx.l0, v10), __fmul_rn(tx.l1, v11));
    return __fadd_rn(__fmul_rn(ty.l0, top), __fmul_rn(ty.l1, bot));
}

// avg_pool2d(x, 3, stride=2, padding=1), count_include_pad=True, of output (oy, ox) of the H x W plane p.
// The nine loads are unconditional (clamped index, zero selected afterwards -- s + 0.0f is s) and in flight together.
__device__ __forceinline__ void dkt_pool9_load(const float *p, int H, int W, int oy, int ox, float (&t)[9]) {
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int iy = 2 * oy - 1 + dy;
        const bool yok = iy >= 0 && iy < H;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int ix = 2 * ox - 1 + dx;
            const bool ok = yok && ix >= 0 && ix < W;
            const float u = p[(long)(yok ? iy : 0) * W + (ix >= 0 && ix < W ? ix : 0)];
            t[dy * 3 + dx] = ok ? u : 0.0f;
        }
    }
}

// Sum order: rows top to bottom, columns left to right (ATen's loop order); ATen divides the sum by the pool size: sum / 9.
__device__ __forceinline__ float dkt_pool9_avg(const float (&t)[9]) {
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) s = __fadd_rn(s, t[k]);
    return __fdiv_rn(s, 9.0f);
}
