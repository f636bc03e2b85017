// gru_gates.h -- the ConvGRU gate arithmetic shared by the inference gates (gru_gates.hip) and the training gates
// (gru_gates_train.hip): one definition, so both compile the same operations in the same order.
// Reference: core/update.py:27-31 (== meta_arch/igev_stereo/update.py:37-40).
#pragma once
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

__device__ __forceinline__ float dkt_gru_out(float aq, float cq, float z, float h) {
    return dkt_gru_blend(z, h, dkt_gru_q(aq, cq));
}

static inline bool dkt_aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

// streaming launches: at most 2048 blocks of 256, the kernels grid-stride over the rest
static inline unsigned dkt_gate_blocks(long total) {
    long blocks = (total + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    return (unsigned)blocks;
}
