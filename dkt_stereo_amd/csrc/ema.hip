// dkt_ema_update: the EMA teacher's parameter update of tools/ft_dkt.py:179-181,
//     t_params.data = ema_decay * t_params.data + (1 - ema_decay) * s_params.data
// for every parameter of the model in ONE launch.  The parameters are a list of tensors of arbitrary sizes; a device
// table of exclusive prefix offsets flattens them, and the grid strides over tiles of that flat range.  A tile that lies
// inside one tensor (all but the few that straddle a boundary) reads its two base pointers once and keeps eight loads of
// each operand in flight per thread; a straddling tile walks the boundary element by element.
//
// Arithmetic: fl(fl(decay * t) + fl(one_minus_decay * s)) in fp32 with two separate roundings (the library builds with
// -ffp-contract=off), which is what torch's elementwise kernels compute for the reference expression: the Python scalars
// become fp32 operands, 1 - ema_decay having been formed in double by Python.
//
// absmax (optional): max |t_new| per tensor, an integer atomic max on the bit patterns of non-negative floats -- max is
// order-independent, so the result does not depend on the schedule.  Memory traffic: 12 B per parameter (read t and s,
// write t) plus the tiny tables.
#include "dkt_common.h"

#include <math.h>

#define EMA_THREADS 256
#define EMA_ITEMS 8
#define EMA_TILE (EMA_THREADS * EMA_ITEMS)

// the tensor holding flat element e: the largest k with off[k] <= e (empty tensors have off[k] == off[k+1] and are skipped)
__device__ __forceinline__ int ema_tensor_of(const long *__restrict__ off, int count, long e) {
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= e) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ float ema_blend(float t, float s, float decay, float omd) {
    const float a = decay * t;
    const float b = omd * s;
    return a + b;
}

__global__ __launch_bounds__(EMA_THREADS) void ema_update_kernel(float *const *__restrict__ tp, const float *const *__restrict__ sp,
                                                               const long *__restrict__ off, int count, float decay, float omd,
                                                               unsigned *__restrict__ absmax) {
    __shared__ unsigned red[EMA_THREADS / 64];
    const long total = off[count];
    const long tiles = (total + EMA_TILE - 1) / EMA_TILE;
    const int tid = threadIdx.x;
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long base = tile * EMA_TILE;
        const long end = base + EMA_TILE < total ? base + EMA_TILE : total;
        int k = ema_tensor_of(off, count, base);
        const long o = off[k];
        if (off[k + 1] >= end) {
            // the whole tile is inside tensor k
            float *__restrict__ t = tp[k] - o;
            const float *__restrict__ s = sp[k] - o;
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
            if (absmax) {
                for (int sh = 32; sh > 0; sh >>= 1) {
                    const unsigned x = (unsigned)__shfl_xor((int)m, sh, 64);
                    m = x > m ? x : m;
                }
                if ((tid & 63) == 0) red[tid >> 6] = m;
                __syncthreads();
                if (tid == 0) {
                    for (int w = 1; w < EMA_THREADS / 64; ++w) m = red[w] > m ? red[w] : m;
                    atomicMax(absmax + k, m);
                }
                __syncthreads();            // (red is reused by the next tile)
            }
        } else {
            // a tile across tensor boundaries: each thread walks its elements in increasing order
            unsigned m = 0;
            for (int j = 0; j < EMA_ITEMS; ++j) {
                const long e = base + j * EMA_THREADS + tid;
                if (e >= end) break;
                while (e >= off[k + 1]) {
                    if (absmax && m) atomicMax(absmax + k, m);
                    m = 0;
                    ++k;
                }
                const long i = e - off[k];
                const float v = ema_blend(tp[k][i], sp[k][i], decay, omd);
                tp[k][i] = v;
                const unsigned u = __float_as_uint(fabsf(v));
                m = u > m ? u : m;
            }
            if (absmax && m) atomicMax(absmax + k, m);
        }
    }
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
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
        cus = 256;
    // 8 blocks of 4 waves per CU: 32 waves, the CU's full occupancy; the grid strides over the tiles of the flat range
    hipLaunchKernelGGL(ema_update_kernel, dim3((unsigned)(cus * 8)), dim3(EMA_THREADS), 0, (hipStream_t)stream,
                       t, s, n, count, decay, one_minus_decay, (unsigned *)absmax);
    return dkt_launch_status();
}
