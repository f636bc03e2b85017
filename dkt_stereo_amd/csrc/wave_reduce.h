// wave_reduce.h -- the fixed-order reductions of the training kernels (device only).
//
// The library's contract is "no float atomics, bit-identical from run to run and for every grid size", so every fp64 sum
// has ONE association, written here once:
//   wave_sum    xor-butterfly over the 64 lanes, offsets 32, 16, ... 1: every lane ends with the same bits.  A lane's sum
//               is (own + partner) at every step.  Lane 0 of the __shfl_down tree has the same partners at every step
//               (lane l < offset reads lane l + offset == l ^ offset, and the values it reads were formed by lanes
//               below 2 * offset in the same way), so a site that reads lane 0 only gets the same bits from either form.
//   block_sum   one LDS slot per wave, then the waves in index order starting FROM slot 0 (s = red[0]; s += red[1]; ...).
//               Starting from red[0] instead of 0.0 differs only for a total of -0.0; every site that uses block_sum
//               was written this way.
//   column_sum  the finalize kernels' "one wave per quantity": lane l adds p[l], p[l + 64], ... in order, eight loads in
//               flight (the unrolled pass adds in the same order as one at a time), then wave_sum.
// Maxima of unsigned bit patterns and ORs are order-independent; they live here so that no kernel file writes a
// 64-lane shuffle loop of its own.  tests/_fixed_order_ref.py restates the three sums on the CPU.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) v += __shfl_xor(v, sh, 64);
    return v;
}

__device__ __forceinline__ unsigned long long wave_or(unsigned long long v) {
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, sh, 64);
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), sh, 64);
        v |= ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) {
        const unsigned u = (unsigned)__shfl_xor((int)v, sh, 64);
        v = u > v ? u : v;
    }
    return v;
}

// Sum over a block of WAVES waves, returned to every thread.  `red`: WAVES doubles of LDS; the trailing barrier lets
// every reader finish, so the same `red` serves any number of calls.
template <int WAVES>
__device__ __forceinline__ double block_sum(double v, double *red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s += red[w];
    __syncthreads();
    return s;
}

// Maximum over a block of WAVES waves, returned to every thread; `red` as in block_sum.
template <int WAVES>
__device__ __forceinline__ unsigned block_max(unsigned v, unsigned *red) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned m = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) m = red[w] > m ? red[w] : m;
    __syncthreads();
    return m;
}

// One wave sums p[0 .. n): lane l takes l, l + 64, ... in increasing order, then the butterfly.  Valid in every lane.
__device__ __forceinline__ double column_sum(const double *__restrict__ p, int n) {
    double s = 0.0;
    int i = threadIdx.x & 63;
    for (; i + 7 * 64 < n; i += 8 * 64) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[i + u * 64];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; i < n; i += 64) s += p[i];
    return wave_sum(s);
}
