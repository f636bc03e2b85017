// pcv_update.hip -- PCVNet's mixture-parameter update (ParametersUpdater.forward after its conv head,
// meta_arch/pcvnet/update.py:92-107) with the disparity regression of meta_arch/pcvnet/model.py:154, and what autograd
// derives for the two: one launch each.  Per pixel, j over the M gaussians (sigma0, eps, gamma1..3 are arguments):
//   ds_raw = 0.5 (((1 - M w) s^2 - sigma0^2 - d^2) / (M s^3) + w s / sigma0^2)
//   dm_raw = -0.5 d (1 / (M s^2) + w / sigma0^2)
//   beta   = 0.5 (-1 / (M w + eps) + log(sigma0 M w / s + eps) + (s^2 + d^2) / (2 sigma0^2) + 0.5),  dw_raw = beta - (sum_j beta) / M
//   ds = clip(gamma1 ds_raw, +-3)   dm = clip(gamma2 dm_raw, +-128)   dw = clip(gamma3 dw_raw, +-1/(4M))
//   s' = clip(s - ds, 0.1, 16)      mu' = mu - dm      w~ = clip(w - dw, 0, 1)      w' = w~ / sum_j w~      disp = sum_j w' mu'
// One thread owns one pixel (four adjacent ones where 16-byte accesses are possible: the rule of gate_launch) and walks its
// gaussians in ascending j, so both sums stay in registers and lanes run along pixels: every plane moves in contiguous
// segments.  No LDS, no atomics, no workspace; the same bits every run.  The five three-state clip decisions of an element
// (below / inside / above) are one base-3 byte, `code`: the backward recomputes beta, dm_raw, w~ and w' from the four inputs
// through the functions of the first section and replays the decisions from the byte, never from a second comparison, and
// passes a gradient where the value was inside or on the edge (torch.clamp's backward).  w~ all zero gives 0/0: NaN at that
// pixel as in the reference, nothing elsewhere.  -ffp-contract=off: every expression below is evaluated as written.
#include "gru_gates.h"

#define PCV_MAX_M 8

struct PcvConst {
    float M, s0M, s0sq, two_s0sq, eps, g1, g2, g3, wlim;
};

static inline PcvConst pcv_const(int M, float sigma0, float eps, float g1, float g2, float g3) {
    PcvConst k;
    k.M = (float)M;
    k.s0M = sigma0 * (float)M;
    k.s0sq = sigma0 * sigma0;
    k.two_s0sq = 2.0f * k.s0sq;
    k.eps = eps;
    k.g1 = g1; k.g2 = g2; k.g3 = g3;
    k.wlim = (float)(1.0 / (4.0 * M));          // 1 / (M * 4) of update.py:100, rounded once
    return k;
}

// ---- the arithmetic, written once: the forward and the backward's recomputation call the same functions ----------------------
__device__ __forceinline__ float pcv_mw_eps(const PcvConst &k, float w) { return k.M * w + k.eps; }

__device__ __forceinline__ float pcv_log_arg(const PcvConst &k, float s, float w) { return __fdiv_rn(k.s0M * w, s) + k.eps; }

__device__ __forceinline__ float pcv_ds_raw(const PcvConst &k, float d, float s, float w) {
    const float s2 = s * s;
    const float num = (1.0f - k.M * w) * s2 - k.s0sq - d * d;
    return 0.5f * (__fdiv_rn(num, k.M * (s2 * s)) + __fdiv_rn(w * s, k.s0sq));
}

__device__ __forceinline__ float pcv_dm_raw(const PcvConst &k, float d, float s, float w) {
    return (-0.5f * d) * (__fdiv_rn(1.0f, k.M * (s * s)) + __fdiv_rn(w, k.s0sq));
}

__device__ __forceinline__ float pcv_beta(const PcvConst &k, float d, float s, float w) {
    const float t = __fdiv_rn(-1.0f, pcv_mw_eps(k, w)) + logf(pcv_log_arg(k, s, w));
    return 0.5f * (t + __fdiv_rn(s * s + d * d, k.two_s0sq) + 0.5f);
}

// a clip and its decision (0 below, 1 inside or on an edge, 2 above; a NaN stays a NaN, inside): DECIDE compares, the
// backward replays st
template <bool DECIDE>
__device__ __forceinline__ float pcv_clip(float x, float lo, float hi, unsigned &st) {
    if (DECIDE) st = x < lo ? 0u : (x > hi ? 2u : 1u);
    return st == 0u ? lo : (st == 2u ? hi : x);
}

// code = (((st_ds 3 + st_dm) 3 + st_dw) 3 + st_sigma') 3 + st_w~
struct PcvStates {
    unsigned ds, dm, dw, sg, wt;
};

__device__ __forceinline__ PcvStates pcv_unpack(unsigned code) {
    PcvStates st;
    st.wt = code % 3u; code /= 3u;
    st.sg = code % 3u; code /= 3u;
    st.dw = code % 3u; code /= 3u;
    st.dm = code % 3u;
    st.ds = code / 3u;
    return st;
}

__device__ __forceinline__ unsigned pcv_pack(const PcvStates &st) {
    return (((st.ds * 3u + st.dm) * 3u + st.dw) * 3u + st.sg) * 3u + st.wt;
}

template <bool DECIDE>
__device__ __forceinline__ float pcv_sigma_new(const PcvConst &k, float d, float s, float w, PcvStates &st) {
    const float ds = pcv_clip<DECIDE>(k.g1 * pcv_ds_raw(k, d, s, w), -3.0f, 3.0f, st.ds);
    return pcv_clip<DECIDE>(s - ds, 0.1f, 16.0f, st.sg);
}

template <bool DECIDE>
__device__ __forceinline__ float pcv_mu_new(const PcvConst &k, float d, float s, float w, float mu, PcvStates &st) {
    return mu - pcv_clip<DECIDE>(k.g2 * pcv_dm_raw(k, d, s, w), -128.0f, 128.0f, st.dm);
}

// w~ from beta, its mean's numerator and w
template <bool DECIDE>
__device__ __forceinline__ float pcv_w_tilde(const PcvConst &k, float beta, float beta_sum, float w, PcvStates &st) {
    const float dw = pcv_clip<DECIDE>(k.g3 * (beta - __fdiv_rn(beta_sum, k.M)), -k.wlim, k.wlim, st.dw);
    return pcv_clip<DECIDE>(w - dw, 0.0f, 1.0f, st.wt);
}

// ---- V decision bytes of adjacent pixels: one 4-byte access when V == 4 ------------------------------------------------------
template <int V>
__device__ __forceinline__ void pcv_code_store(unsigned char *p, const unsigned (&c)[V]) {
    if constexpr (V == 4) *(unsigned *)p = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
    else p[0] = (unsigned char)c[0];
}

template <int V>
__device__ __forceinline__ void pcv_code_load(const unsigned char *p, unsigned (&c)[V]) {
    if constexpr (V == 4) {
        const unsigned t = *(const unsigned *)p;
        c[0] = t & 255u, c[1] = (t >> 8) & 255u, c[2] = (t >> 16) & 255u, c[3] = t >> 24;
    } else {
        c[0] = p[0];
    }
}

struct PcvFwdArgs {
    const float *delta, *mu, *sigma, *w;
    float *mu_out, *w_out, *sigma_out, *disp;
    unsigned char *code;
    long HW, total;              // total = N * HW / V items
    PcvConst k;
};

template <int M, int V>
__global__ __launch_bounds__(256) void pcv_update_fwd_kernel(PcvFwdArgs a) {
    const PcvConst k = a.k;
    const long per_n = a.HW / V;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < a.total; i += (long)gridDim.x * 256L) {
        const long n = i / per_n;
        const long p = (i - n * per_n) * V;
        const long base = n * M * a.HW + p;
        float bt[M][V], wv[M][V], mun[M][V];
        unsigned cd[M][V];
        float bsum[V], T[V], dsp[V];
#pragma unroll
        for (int v = 0; v < V; ++v) bsum[v] = 0.0f, T[v] = 0.0f, dsp[v] = 0.0f;
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const long o = base + j * a.HW;
            const GateVec<V> d = gate_load<V>(a.delta + o), s = gate_load<V>(a.sigma + o), w = gate_load<V>(a.w + o),
                             mu = gate_load<V>(a.mu + o);
            GateVec<V> sn;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                bt[j][v] = pcv_beta(k, d.v[v], s.v[v], w.v[v]);
                bsum[v] = bsum[v] + bt[j][v];
                wv[j][v] = w.v[v];
                PcvStates st;
                st.dw = 0u, st.wt = 0u;
                sn.v[v] = pcv_sigma_new<true>(k, d.v[v], s.v[v], w.v[v], st);
                mun[j][v] = pcv_mu_new<true>(k, d.v[v], s.v[v], w.v[v], mu.v[v], st);
                cd[j][v] = pcv_pack(st);
            }
            gate_store<V>(a.sigma_out + o, sn);
        }
#pragma unroll
        for (int j = 0; j < M; ++j)
#pragma unroll
            for (int v = 0; v < V; ++v) {
                PcvStates st;
                bt[j][v] = pcv_w_tilde<true>(k, bt[j][v], bsum[v], wv[j][v], st);
                cd[j][v] = cd[j][v] + st.dw * 9u + st.wt;
                T[v] = T[v] + bt[j][v];
            }
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const long o = base + j * a.HW;
            GateVec<V> wn, mn;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                wn.v[v] = __fdiv_rn(bt[j][v], T[v]);
                mn.v[v] = mun[j][v];
                dsp[v] = dsp[v] + wn.v[v] * mn.v[v];
            }
            gate_store<V>(a.w_out + o, wn);
            gate_store<V>(a.mu_out + o, mn);
            if (a.code) pcv_code_store<V>(a.code + o, cd[j]);
        }
        if (a.disp) {
            GateVec<V> dv;
#pragma unroll
            for (int v = 0; v < V; ++v) dv.v[v] = dsp[v];
            gate_store<V>(a.disp + n * a.HW + p, dv);
        }
    }
}

struct PcvBwdUpdArgs {
    const float *delta, *mu, *sigma, *w;
    const unsigned char *code;
    const float *gmu_out, *gw_out, *gsigma_out, *gdisp;        // each may be null: zero
    float *gdelta, *gmu, *gsigma, *gw;                          // each may be null: not wanted
    long HW, total;
    PcvConst k;
};

// With T = sum w~, u = sigma0 M w / s + eps and c the pass indicators of the byte:
//   Gmu' = gmu' + gdisp w'     Gw' = gw' + gdisp mu'     Gw~ = (Gw' - sum_k Gw'_k w'_k) / T
//   A = c_W Gw~     B = -gamma3 c_w A     gbeta = B - (sum_k B_k) / M     E = c_S gs'     g_ds = -gamma1 c_s E     g_dm = -gamma2 c_m Gmu'
//   gd = g_ds (-d / (M s^3)) + g_dm (-0.5 (1 / (M s^2) + w / sigma0^2)) + gbeta d / (2 sigma0^2)
//   gs = E + g_ds 0.5 (-(1 - M w) / (M s^2) + 3 (sigma0^2 + d^2) / (M s^4) + w / sigma0^2) + g_dm d / (M s^3)
//          + gbeta 0.5 (-(sigma0 M w / s^2) / u + s / sigma0^2)
//   gw = A + g_ds 0.5 (-1 / s + s / sigma0^2) + g_dm (-0.5 d / sigma0^2) + gbeta 0.5 (M / (M w + eps)^2 + (sigma0 M / s) / u)
//   gmu = Gmu'
template <int M, int V>
__global__ __launch_bounds__(256) void pcv_update_bwd_kernel(PcvBwdUpdArgs a) {
    const PcvConst k = a.k;
    const long per_n = a.HW / V;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < a.total; i += (long)gridDim.x * 256L) {
        const long n = i / per_n;
        const long p = (i - n * per_n) * V;
        const long base = n * M * a.HW + p;
        float bt[M][V], wv[M][V], ga[M][V];       // bt: beta, then w~, then w';  ga: Gw', then A
        unsigned cd[M][V];
        float bsum[V], T[V], S1[V], Bsum[V], gd[V];
#pragma unroll
        for (int v = 0; v < V; ++v) bsum[v] = 0.0f, T[v] = 0.0f, S1[v] = 0.0f, Bsum[v] = 0.0f, gd[v] = 0.0f;
        if (a.gdisp) {
            const GateVec<V> t = gate_load<V>(a.gdisp + n * a.HW + p);
#pragma unroll
            for (int v = 0; v < V; ++v) gd[v] = t.v[v];
        }
        // the forward again: beta and its sum, w~ and its sum, w'
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const long o = base + j * a.HW;
            const GateVec<V> d = gate_load<V>(a.delta + o), s = gate_load<V>(a.sigma + o), w = gate_load<V>(a.w + o);
            pcv_code_load<V>(a.code + o, cd[j]);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                bt[j][v] = pcv_beta(k, d.v[v], s.v[v], w.v[v]);
                bsum[v] = bsum[v] + bt[j][v];
                wv[j][v] = w.v[v];
            }
        }
#pragma unroll
        for (int j = 0; j < M; ++j)
#pragma unroll
            for (int v = 0; v < V; ++v) {
                PcvStates st = pcv_unpack(cd[j][v]);
                bt[j][v] = pcv_w_tilde<false>(k, bt[j][v], bsum[v], wv[j][v], st);
                T[v] = T[v] + bt[j][v];
            }
        // Gw' = gw' + gdisp mu' and S1 = sum Gw' w'
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const long o = base + j * a.HW;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                bt[j][v] = __fdiv_rn(bt[j][v], T[v]);
                ga[j][v] = 0.0f;
            }
            if (a.gw_out) {
                const GateVec<V> t = gate_load<V>(a.gw_out + o);
#pragma unroll
                for (int v = 0; v < V; ++v) ga[j][v] = t.v[v];
            }
            if (a.gdisp) {
                const GateVec<V> d = gate_load<V>(a.delta + o), s = gate_load<V>(a.sigma + o), mu = gate_load<V>(a.mu + o);
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    PcvStates st = pcv_unpack(cd[j][v]);
                    ga[j][v] = ga[j][v] + gd[v] * pcv_mu_new<false>(k, d.v[v], s.v[v], wv[j][v], mu.v[v], st);
                }
            }
#pragma unroll
            for (int v = 0; v < V; ++v) S1[v] = S1[v] + ga[j][v] * bt[j][v];
        }
        // A and the sum of B
#pragma unroll
        for (int j = 0; j < M; ++j)
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const PcvStates st = pcv_unpack(cd[j][v]);
                ga[j][v] = st.wt == 1u ? __fdiv_rn(ga[j][v] - S1[v], T[v]) : 0.0f;
                Bsum[v] = Bsum[v] + (st.dw == 1u ? -k.g3 * ga[j][v] : 0.0f);
            }
        // the four results
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const long o = base + j * a.HW;
            const GateVec<V> d = gate_load<V>(a.delta + o), s = gate_load<V>(a.sigma + o);
            GateVec<V> gmo, gso, rd, rm, rs, rw;
#pragma unroll
            for (int v = 0; v < V; ++v) gmo.v[v] = 0.0f, gso.v[v] = 0.0f;
            if (a.gmu_out) gmo = gate_load<V>(a.gmu_out + o);
            if (a.gsigma_out) gso = gate_load<V>(a.gsigma_out + o);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const float dd = d.v[v], ss = s.v[v], ww = wv[j][v];
                const PcvStates t = pcv_unpack(cd[j][v]);
                const float A = ga[j][v];
                const float gbeta = (t.dw == 1u ? -k.g3 * A : 0.0f) - __fdiv_rn(Bsum[v], k.M);
                const float E = t.sg == 1u ? gso.v[v] : 0.0f;
                const float g_ds = t.ds == 1u ? -k.g1 * E : 0.0f;
                const float Gmu = gmo.v[v] + gd[v] * bt[j][v];
                const float g_dm = t.dm == 1u ? -k.g2 * Gmu : 0.0f;
                const float s2 = ss * ss;
                const float Ms2 = k.M * s2, Ms3 = k.M * (s2 * ss);
                const float w_s0 = __fdiv_rn(ww, k.s0sq);
                const float d_Ms3 = __fdiv_rn(dd, Ms3);
                const float u = pcv_log_arg(k, ss, ww), mwe = pcv_mw_eps(k, ww);
                rm.v[v] = Gmu;
                rd.v[v] = g_ds * -d_Ms3 + g_dm * (-0.5f * (__fdiv_rn(1.0f, Ms2) + w_s0)) + gbeta * __fdiv_rn(dd, k.two_s0sq);
                rs.v[v] = E + g_ds * (0.5f * (__fdiv_rn(-(1.0f - k.M * ww), Ms2) + __fdiv_rn(3.0f * (k.s0sq + dd * dd), Ms3 * ss) + w_s0))
                          + g_dm * d_Ms3
                          + gbeta * (0.5f * (__fdiv_rn(-__fdiv_rn(k.s0M * ww, s2), u) + __fdiv_rn(ss, k.s0sq)));
                rw.v[v] = A + g_ds * (0.5f * (__fdiv_rn(-1.0f, ss) + __fdiv_rn(ss, k.s0sq))) + g_dm * (-0.5f * __fdiv_rn(dd, k.s0sq))
                          + gbeta * (0.5f * (__fdiv_rn(k.M, mwe * mwe) + __fdiv_rn(__fdiv_rn(k.s0M, ss), u)));
            }
            if (a.gdelta) gate_store<V>(a.gdelta + o, rd);
            if (a.gmu) gate_store<V>(a.gmu + o, rm);
            if (a.gsigma) gate_store<V>(a.gsigma + o, rs);
            if (a.gw) gate_store<V>(a.gw + o, rw);
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
static int pcv_update_dims_status(int N, int M, int H, int W) {
    if (N <= 0 || M <= 0 || H <= 0 || W <= 0) return DKT_E_SHAPE;
    if (M > PCV_MAX_M || N > 65535 || (long)H * W > 2147483647L - 257) return DKT_E_UNSUPPORTED;
    return DKT_OK;
}

// gate_launch's rule: four pixels per thread when H*W and every pointer allow 16-byte accesses (the decision bytes then move
// four at a time from a 4-byte aligned address, which a 16-byte aligned base and H*W % 4 == 0 give)
static bool pcv_vec(long HW, std::initializer_list<const void *> pointers) {
    bool vec = HW % 4 == 0;
    for (const void *p : pointers) vec = vec && dkt_aligned16(p);
    return vec;
}

template <class Args>
static void pcv_launch_m(void (*const *table)(Args), int M, const Args &a, hipStream_t st) {
    hipLaunchKernelGGL(table[M - 1], dim3(dkt_gate_blocks(a.total)), dim3(256), 0, st, a);
}

#define PCV_TABLE(kernel, V) {kernel<1, V>, kernel<2, V>, kernel<3, V>, kernel<4, V>, kernel<5, V>, kernel<6, V>, kernel<7, V>, kernel<8, V>}

extern "C" int dkt_pcv_update_fwd(const float *delta, const float *mu, const float *sigma, const float *w,
                                  float *mu_out, float *w_out, float *sigma_out, float *disp, unsigned char *code,
                                  int N, int M, int H, int W, float sigma0, float eps, float gamma1, float gamma2, float gamma3,
                                  int device, void *stream) {
    if (!delta || !mu || !sigma || !w || !mu_out || !w_out || !sigma_out) return DKT_E_NULL;
    const int rc = pcv_update_dims_status(N, M, H, W);
    if (rc != DKT_OK) return rc;
    PcvFwdArgs a;
    a.delta = delta; a.mu = mu; a.sigma = sigma; a.w = w;
    a.mu_out = mu_out; a.w_out = w_out; a.sigma_out = sigma_out; a.disp = disp; a.code = code;
    a.HW = (long)H * W;
    a.k = pcv_const(M, sigma0, eps, gamma1, gamma2, gamma3);
    const bool vec = pcv_vec(a.HW, {delta, mu, sigma, w, mu_out, w_out, sigma_out, disp, code});
    a.total = (long)N * a.HW / (vec ? 4 : 1);
    static void (*const vec_table[PCV_MAX_M])(PcvFwdArgs) = PCV_TABLE(pcv_update_fwd_kernel, 4);
    static void (*const one_table[PCV_MAX_M])(PcvFwdArgs) = PCV_TABLE(pcv_update_fwd_kernel, 1);
    DKT_ENTER(device);
    if (vec) pcv_launch_m(vec_table, M, a, (hipStream_t)stream);
    else pcv_launch_m(one_table, M, a, (hipStream_t)stream);
    return dkt_launch_status();
}

extern "C" int dkt_pcv_update_bwd(const float *delta, const float *mu, const float *sigma, const float *w,
                                  const unsigned char *code, const float *gmu_out, const float *gw_out,
                                  const float *gsigma_out, const float *gdisp, float *gdelta, float *gmu, float *gsigma,
                                  float *gw, int N, int M, int H, int W, float sigma0, float eps, float gamma1, float gamma2,
                                  float gamma3, int device, void *stream) {
    if (!delta || !mu || !sigma || !w || !code) return DKT_E_NULL;
    if (!gmu_out && !gw_out && !gsigma_out && !gdisp) return DKT_E_NULL;
    if (!gdelta && !gmu && !gsigma && !gw) return DKT_E_NULL;
    const int rc = pcv_update_dims_status(N, M, H, W);
    if (rc != DKT_OK) return rc;
    PcvBwdUpdArgs a;
    a.delta = delta; a.mu = mu; a.sigma = sigma; a.w = w; a.code = code;
    a.gmu_out = gmu_out; a.gw_out = gw_out; a.gsigma_out = gsigma_out; a.gdisp = gdisp;
    a.gdelta = gdelta; a.gmu = gmu; a.gsigma = gsigma; a.gw = gw;
    a.HW = (long)H * W;
    a.k = pcv_const(M, sigma0, eps, gamma1, gamma2, gamma3);
    const bool vec = pcv_vec(a.HW, {delta, mu, sigma, w, code, gmu_out, gw_out, gsigma_out, gdisp, gdelta, gmu, gsigma, gw});
    a.total = (long)N * a.HW / (vec ? 4 : 1);
    static void (*const vec_table[PCV_MAX_M])(PcvBwdUpdArgs) = PCV_TABLE(pcv_update_bwd_kernel, 4);
    static void (*const one_table[PCV_MAX_M])(PcvBwdUpdArgs) = PCV_TABLE(pcv_update_bwd_kernel, 1);
    DKT_ENTER(device);
    if (vec) pcv_launch_m(vec_table, M, a, (hipStream_t)stream);
    else pcv_launch_m(one_table, M, a, (hipStream_t)stream);
    return dkt_launch_status();
}
