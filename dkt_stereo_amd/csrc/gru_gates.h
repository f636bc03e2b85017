// gru_gates.h -- the ConvGRU gate arithmetic and the one streaming walk every gate kernel of gru_gates.hip runs on: one
// definition each, so the inference and the training kernels compile the same operations in the same order.
// Reference: core/update.py:27-31 (== meta_arch/igev_stereo/update.py:37-40).
#pragma once
#include <initializer_list>

#include "dkt_common.h"

__device__ __forceinline__ float dkt_sigmoid(float x) {
    return __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-x)));
}

// q = tanh(aq + cq) (core/update.py:30)
__device__ __forceinline__ float dkt_gru_q(float aq, float cq) {
    return tanhf(__fadd_rn(aq, cq));
}

// (1-z)*h + z*q, two rounded products and a rounded sum (core/update.py:31)
__device__ __forceinline__ float dkt_gru_blend(float z, float h, float q) {
    return __fadd_rn(__fmul_rn(__fsub_rn(1.0f, z), h), __fmul_rn(z, q));
}

// streaming launches: at most 2048 blocks of 256, the kernels grid-stride over the rest
static inline unsigned dkt_gate_blocks(long total) {
    long blocks = (total + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    return (unsigned)blocks;
}

// ---- lanes: a functor states its formula once on GateVec<V>; V == 4 is one 16-byte access per operand -----------------
template <int V>
struct GateVec {
    float v[V];
};

template <int V>
__device__ __forceinline__ GateVec<V> gate_load(const float *p) {
    GateVec<V> r;
    if constexpr (V == 4) {
        const float4 t = *(const float4 *)p;
        r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
    } else {
        r.v[0] = p[0];
    }
    return r;
}

template <int V>
__device__ __forceinline__ void gate_store(float *p, const GateVec<V> &a) {
    if constexpr (V == 4) *(float4 *)p = make_float4(a.v[0], a.v[1], a.v[2], a.v[3]);
    else p[0] = a.v[0];
}

// f, a scalar __device__ function, applied to each lane
template <int V, class F, class... A>
__device__ __forceinline__ GateVec<V> gate_map(F f, const A &...a) {
    GateVec<V> r;
#pragma unroll
    for (int k = 0; k < V; ++k) r.v[k] = f(a.v[k]...);
    return r;
}

// ---- the walk: item i of B * CHW / V is V adjacent elements at offset e of batch b ------------------------------------
// CHW is the functor's own member (every functor addresses with it): a second copy among the kernel arguments costs
// every kernel one more scalar load, issued behind the early-exit test of its prologue.
template <int V, class Op>
__global__ __launch_bounds__(256) void gate_walk_kernel(Op op, long total) {
    const long per_b = op.CHW / V;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const long b = i / per_b;
        const long e = (i - b * per_b) * V;
        op.template item<V>(b, e);
    }
}

// `pointers`: every pointer op touches (a null optional output counts as aligned); `strides`: every batch stride.
// float4 items when CHW, the strides and the pointers all allow it, scalar items otherwise.
template <class Op>
static inline int gate_launch(const Op &op, int B, std::initializer_list<const void *> pointers,
                              std::initializer_list<long> strides, void *stream) {
    const long CHW = op.CHW;
    bool vec = CHW % 4 == 0;
    for (long s : strides) vec = vec && s % 4 == 0;
    for (const void *p : pointers) vec = vec && dkt_aligned16(p);
    const long total = (long)B * CHW / (vec ? 4 : 1);
    const dim3 grid(dkt_gate_blocks(total));
    if (vec) hipLaunchKernelGGL((gate_walk_kernel<4, Op>), grid, dim3(256), 0, (hipStream_t)stream, op, total);
    else hipLaunchKernelGGL((gate_walk_kernel<1, Op>), grid, dim3(256), 0, (hipStream_t)stream, op, total);
    return dkt_launch_status();
}
