// dkt_ema_update: the EMA teacher's parameter update of tools/ft_dkt.py:179-181,
//     t_params.data = ema_decay * t_params.data + (1 - ema_decay) * s_params.data
// for every parameter of the model in ONE launch: the walk over the list of tensors, its tiles and the per-tensor absmax
// are flat_walk.h's; this file holds the element arithmetic.
//
// Arithmetic: fl(fl(decay * t) + fl(one_minus_decay * s)) in fp32 with two separate roundings (the library builds with
// -ffp-contract=off), which is what torch's elementwise kernels compute for the reference expression: the Python scalars
// become fp32 operands, 1 - ema_decay having been formed in double by Python.
//
// absmax (optional): max |t_new| per tensor.  Memory traffic: 12 B per parameter (read t and s, write t) plus the tiny tables.
#include "dkt_common.h"
#include "flat_walk.h"

#include <math.h>

#define EMA_THREADS 256
#define EMA_ITEMS 8

__device__ __forceinline__ float ema_blend(float t, float s, float decay, float omd) {
    const float a = decay * t;
    const float b = omd * s;
    return a + b;
}

__global__ __launch_bounds__(EMA_THREADS) void ema_update_kernel(float *const *__restrict__ tp, const float *const *__restrict__ sp,
                                                               const long *__restrict__ off, int count, float decay, float omd,
                                                               unsigned *__restrict__ absmax) {
    __shared__ unsigned red[EMA_THREADS / 64];
    const int tid = threadIdx.x;
    flat_walk<EMA_THREADS, EMA_ITEMS>(
        off, count, absmax, red,
        [&](int k, long base, long end) {
            float *__restrict__ t = tp[k] - off[k];
            const float *__restrict__ s = sp[k] - off[k];
            float a[EMA_ITEMS], b[EMA_ITEMS];
#pragma unroll
            for (int j = 0; j < EMA_ITEMS; ++j) {
                const long e = base + j * EMA_THREADS + tid;
                a[j] = e < end ? t[e] : 0.f;
                b[j] = e < end ? s[e] : 0.f;
            }
            unsigned m = 0;
#pragma unroll
            for (int j = 0; j < EMA_ITEMS; ++j) {
                const long e = base + j * EMA_THREADS + tid;
                if (e < end) {
                    const float v = ema_blend(a[j], b[j], decay, omd);
                    t[e] = v;
                    const unsigned u = __float_as_uint(fabsf(v));
                    m = u > m ? u : m;
                }
            }
            return m;
        },
        [&](int k, long i, int) {
            const float v = ema_blend(tp[k][i], sp[k][i], decay, omd);
            tp[k][i] = v;
            return __float_as_uint(fabsf(v));
        },
        [](long) {});
}

extern "C" int dkt_ema_update(float *const *t, const float *const *s, const long *n, int count, float decay,
                              float one_minus_decay, float *absmax, int device, void *stream) {
    if (count < 0) return DKT_E_SHAPE;
    if (!isfinite(decay) || !isfinite(one_minus_decay)) return DKT_E_UNSUPPORTED;
    if (count == 0) return DKT_OK;
    if (!t || !s || !n) return DKT_E_NULL;
    DKT_ENTER(device);
    if (absmax) {
        const hipError_t e = hipMemsetAsync(absmax, 0, (size_t)count * sizeof(float), (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    // (the total lives in the device table: the grid is not capped by the tile count)
    hipLaunchKernelGGL(ema_update_kernel, dim3((unsigned)flat_walk_blocks(-1)), dim3(EMA_THREADS), 0, (hipStream_t)stream,
                       t, s, n, count, decay, one_minus_decay, (unsigned *)absmax);
    return dkt_launch_status();
}
