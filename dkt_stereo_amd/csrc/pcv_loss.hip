// dkt_pcv_loss / dkt_pcv_loss_bwd: PCVNet's sequence loss (meta_arch/pcvnet/loss.py:4-73) against one or two targets, the
// pair of calls of tools/ft_dkt.py:227-228.
//
// Forward, launch 1 (partials): block = one tile of PLOSS_TILE pixels of one image.  The targets and their masks are loaded
// once into registers; then the predictions stream through: final_disp and the M mu planes of prediction i + 1 are loaded
// before prediction i is reduced, and the M w and M sigma planes of prediction i (read for the finite check only, and only
// when their pointers are given) are in flight over the same reduction.  Each wave reduces every sum in wave_reduce.h's
// shuffle order into LDS; the block writes one fp64 partial per quantity, quantity-major, and one flag word (bit i: a NaN or
// an Inf anywhere in prediction i).  Launch 2 (finalize, one block): every quantity is summed over the blocks in a fixed
// order, then the loss is formed in fp32 in the reference's order and written as a device scalar with the record.
// No atomics on floats anywhere: the results are bit-identical from run to run.
//
// Backward (one launch): the same tiles; reads the upstream gradients, the counts and the masks on the device and stores
// every element of every requested gradient once.
//
// VEC: a thread owns four adjacent pixels and every access is 16 bytes (H W % 4 == 0, every plane 16-byte aligned);
// otherwise a thread owns four pixels PLOSS_THREADS apart and every access is scalar.  Both are instances of one kernel.
#include "dkt_common.h"
#include "wave_reduce.h"

#include <math.h>

#define PLOSS_THREADS 256
#define PLOSS_ITEMS 4
#define PLOSS_TILE (PLOSS_THREADS * PLOSS_ITEMS)
#define PLOSS_WAVES (PLOSS_THREADS / 64)
#define PLOSS_MAX_LOSS 6                         // i_weights has six entries (loss.py:19)
// quantities per target: [0] count, [1 + i] S1_i, [7 + i] S2_i, [13] smooth-L1 sum of disp_refine,
// [14 .. 20] EPE sum and the counts < 1, < 3, < 5, > 1, > 2, > 5 of final_disp_preds[3], [21 .. 27] the same of disp_refine
#define PLOSS_QK 28
#define PLOSS_Q_S1 1
#define PLOSS_Q_S2 7
#define PLOSS_Q_SL1 13
#define PLOSS_Q_EPE3 14
#define PLOSS_Q_EPEF 21
#define PLOSS_METRIC_PRED 3                      // loss.py:53
#define PLOSS_FIN_THREADS 1024
#define PLOSS_REC_K 16                           // doubles of the record per target

static inline int ploss_tiles(int H, int W) { return (int)(((long)H * W + PLOSS_TILE - 1) / PLOSS_TILE); }

struct PlossVec {
    float v[PLOSS_ITEMS];
};

// index of item j of this thread inside the image
template <bool VEC>
__device__ __forceinline__ int ploss_index(int tile, int tid, int j) {
    return VEC ? tile * PLOSS_TILE + tid * PLOSS_ITEMS + j : tile * PLOSS_TILE + j * PLOSS_THREADS + tid;
}

// four pixels of one plane; items past the image hold 0.0f (neither NaN nor Inf)
template <bool VEC>
__device__ __forceinline__ PlossVec ploss_load(const float *__restrict__ p, int tile, int tid, int HW) {
    PlossVec r;
    if (VEC) {
        const int r0 = ploss_index<true>(tile, tid, 0);
        float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (r0 < HW) t = *(const float4 *)(p + r0);
        r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < PLOSS_ITEMS; ++j) {
            const int i = ploss_index<false>(tile, tid, j);
            r.v[j] = i < HW ? p[i] : 0.0f;
        }
    }
    return r;
}

template <bool VEC>
__device__ __forceinline__ void ploss_store(float *__restrict__ p, const PlossVec &x, int tile, int tid, int HW) {
    if (VEC) {
        const int r0 = ploss_index<true>(tile, tid, 0);
        if (r0 < HW) *(float4 *)(p + r0) = make_float4(x.v[0], x.v[1], x.v[2], x.v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < PLOSS_ITEMS; ++j) {
            const int i = ploss_index<false>(tile, tid, j);
            if (i < HW) p[i] = x.v[j];
        }
    }
}

// the mask bytes of four pixels, in one 4-byte access when VEC
template <bool VEC>
__device__ __forceinline__ void ploss_mask_store(unsigned char *__restrict__ p, const bool (&m)[PLOSS_ITEMS], int tile, int tid, int HW) {
    if (VEC) {
        const int r0 = ploss_index<true>(tile, tid, 0);
        if (r0 < HW) *(unsigned *)(p + r0) = (m[0] ? 1u : 0u) | (m[1] ? 1u << 8 : 0u) | (m[2] ? 1u << 16 : 0u) | (m[3] ? 1u << 24 : 0u);
    } else {
#pragma unroll
        for (int j = 0; j < PLOSS_ITEMS; ++j) {
            const int i = ploss_index<false>(tile, tid, j);
            if (i < HW) p[i] = m[j] ? 1 : 0;
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void ploss_mask_load(const unsigned char *__restrict__ p, bool (&m)[PLOSS_ITEMS], int tile, int tid, int HW) {
    if (VEC) {
        const int r0 = ploss_index<true>(tile, tid, 0);
        const unsigned t = r0 < HW ? *(const unsigned *)(p + r0) : 0u;
#pragma unroll
        for (int j = 0; j < PLOSS_ITEMS; ++j) m[j] = ((t >> (8 * j)) & 255u) != 0u;
    } else {
#pragma unroll
        for (int j = 0; j < PLOSS_ITEMS; ++j) {
            const int i = ploss_index<false>(tile, tid, j);
            m[j] = i < HW && p[i] != 0;
        }
    }
}

// NaN or +-Inf: an all-ones exponent
__device__ __forceinline__ bool ploss_nonfinite(const PlossVec &x) {
    bool f = false;
#pragma unroll
    for (int j = 0; j < PLOSS_ITEMS; ++j) f = f || (__float_as_uint(x.v[j]) & 0x7f800000u) == 0x7f800000u;
    return f;
}

// EPE sum and the six strict counts of loss.py:56-62 over the mask, written to part[q0 .. q0 + 6]
__device__ __forceinline__ void ploss_epe(const PlossVec &p, const float (&g)[PLOSS_ITEMS], const bool (&m)[PLOSS_ITEMS], double *part, int lane) {
    double e = 0.0, c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < PLOSS_ITEMS; ++j) {
        if (!m[j]) continue;
        const float ep = fabsf(__fsub_rn(p.v[j], g[j]));
        e += (double)ep;
        c[0] += ep < 1.0f ? 1.0 : 0.0;
        c[1] += ep < 3.0f ? 1.0 : 0.0;
        c[2] += ep < 5.0f ? 1.0 : 0.0;
        c[3] += ep > 1.0f ? 1.0 : 0.0;
        c[4] += ep > 2.0f ? 1.0 : 0.0;
        c[5] += ep > 5.0f ? 1.0 : 0.0;
    }
    e = wave_sum(e);
#pragma unroll
    for (int q = 0; q < 6; ++q) c[q] = wave_sum(c[q]);
    if (lane == 0) {
        part[0] = e;
#pragma unroll
        for (int q = 0; q < 6; ++q) part[1 + q] = c[q];
    }
}

template <bool VEC>
__global__ __launch_bounds__(PLOSS_THREADS) void pcv_loss_partials_kernel(dkt_pcv_loss_desc d, double *__restrict__ ws) {
    __shared__ double part[PLOSS_WAVES][2 * PLOSS_QK];
    __shared__ unsigned long long flag[PLOSS_WAVES];
    const int HW = d.H * d.W, b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = d.ntargets, M = d.M;
    const long nblk = (long)gridDim.x * gridDim.y, blk = (long)b * gridDim.x + blockIdx.x;
    for (int q = tid; q < PLOSS_WAVES * 2 * PLOSS_QK; q += PLOSS_THREADS) (&part[0][0])[q] = 0.0;
    __syncthreads();
    float g[2][PLOSS_ITEMS];
    bool m[2][PLOSS_ITEMS];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma unroll
        for (int j = 0; j < PLOSS_ITEMS; ++j) g[k][j] = 0.0f, m[k][j] = false;
        if (k >= K) continue;
        const PlossVec gv = ploss_load<VEC>(d.gt[k] + (long)b * d.gt_bstride[k], tile, tid, HW);
        const PlossVec vv = ploss_load<VEC>(d.valid[k] + (long)b * d.valid_bstride[k], tile, tid, HW);
        double cnt = 0.0;
#pragma unroll
        for (int j = 0; j < PLOSS_ITEMS; ++j) {
            const bool in = ploss_index<VEC>(tile, tid, j) < HW;
            // valid = (disp_gt < max_disp) & (valid[:, None].bool()) & (disp_gt >= 0): .bool() is "!= 0", true for NaN
            const bool mk = in && gv.v[j] < d.max_disp && vv.v[j] != 0.0f && gv.v[j] >= 0.0f;
            g[k][j] = gv.v[j];
            m[k][j] = mk;
            cnt += mk ? 1.0 : 0.0;
        }
        ploss_mask_store<VEC>(d.mask[k] + (long)b * HW, m[k], tile, tid, HW);
        cnt = wave_sum(cnt);
        if (lane == 0) part[wave][k * PLOSS_QK] = cnt;
    }
    // disp_refine: smooth-L1 sum and the *_final metrics
    {
        const PlossVec rf = ploss_load<VEC>(d.refine + (long)b * d.refine_bstride, tile, tid, HW);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (k >= K) continue;
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < PLOSS_ITEMS; ++j) {
                if (!m[k][j]) continue;
                // F.smooth_l1_loss, beta = 1: 0.5 z z or z - 0.5
                const float z = fabsf(__fsub_rn(rf.v[j], g[k][j]));
                s += (double)(z < 1.0f ? __fmul_rn(__fmul_rn(0.5f, z), z) : __fsub_rn(z, 0.5f));
            }
            s = wave_sum(s);
            if (lane == 0) part[wave][k * PLOSS_QK + PLOSS_Q_SL1] = s;
            ploss_epe(rf, g[k], m[k], &part[wave][k * PLOSS_QK + PLOSS_Q_EPEF], lane);
        }
    }
    unsigned long long bad = 0;
    PlossVec dc, dn, mc[DKT_PCV_LOSS_MAX_M], mn[DKT_PCV_LOSS_MAX_M];
    dc = ploss_load<VEC>(d.disp[0] + (long)b * d.disp_bstride[0], tile, tid, HW);
#pragma unroll
    for (int j = 0; j < DKT_PCV_LOSS_MAX_M; ++j)
        if (j < M) mc[j] = ploss_load<VEC>(d.mu[0] + (long)b * d.mu_bstride[0] + (long)j * d.mu_gstride[0], tile, tid, HW);
    for (int i = 0; i < d.n; ++i) {
        if (i + 1 < d.n) {
            dn = ploss_load<VEC>(d.disp[i + 1] + (long)b * d.disp_bstride[i + 1], tile, tid, HW);
            const float *mp = d.mu[i + 1] + (long)b * d.mu_bstride[i + 1];
            const long gs = d.mu_gstride[i + 1];
#pragma unroll
            for (int j = 0; j < DKT_PCV_LOSS_MAX_M; ++j)
                if (j < M) mn[j] = ploss_load<VEC>(mp + (long)j * gs, tile, tid, HW);
        }
        bool nf = ploss_nonfinite(dc);
        // w and sigma: the finite check of loss.py:31-32 is all the loss takes from them
        if (d.w[i]) {
            const float *wp = d.w[i] + (long)b * d.w_bstride[i];
            const long gs = d.w_gstride[i];
            PlossVec t[DKT_PCV_LOSS_MAX_M];
#pragma unroll
            for (int j = 0; j < DKT_PCV_LOSS_MAX_M; ++j)
                if (j < M) t[j] = ploss_load<VEC>(wp + (long)j * gs, tile, tid, HW);
#pragma unroll
            for (int j = 0; j < DKT_PCV_LOSS_MAX_M; ++j)
                if (j < M) nf = nf || ploss_nonfinite(t[j]);
        }
        if (d.sigma[i]) {
            const float *sp = d.sigma[i] + (long)b * d.sigma_bstride[i];
            const long gs = d.sigma_gstride[i];
            PlossVec t[DKT_PCV_LOSS_MAX_M];
#pragma unroll
            for (int j = 0; j < DKT_PCV_LOSS_MAX_M; ++j)
                if (j < M) t[j] = ploss_load<VEC>(sp + (long)j * gs, tile, tid, HW);
#pragma unroll
            for (int j = 0; j < DKT_PCV_LOSS_MAX_M; ++j)
                if (j < M) nf = nf || ploss_nonfinite(t[j]);
        }
#pragma unroll
        for (int j = 0; j < DKT_PCV_LOSS_MAX_M; ++j)
            if (j < M) nf = nf || ploss_nonfinite(mc[j]);
        if (nf) bad |= 1ull << i;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (k >= K) continue;
            if (i < d.n_loss) {
                // i_loss1 = |final_disp - gt|; i_loss2 = mean_m |mu_m - gt|: the sum over m in fp32 in order m, then / M
                double s1 = 0.0, s2 = 0.0;
#pragma unroll
                for (int j = 0; j < PLOSS_ITEMS; ++j) {
                    if (!m[k][j]) continue;
                    s1 += (double)fabsf(__fsub_rn(dc.v[j], g[k][j]));
                    float a = 0.0f;
#pragma unroll
                    for (int q = 0; q < DKT_PCV_LOSS_MAX_M; ++q)
                        if (q < M) a = __fadd_rn(a, fabsf(__fsub_rn(mc[q].v[j], g[k][j])));
                    s2 += (double)__fdiv_rn(a, (float)M);
                }
                s1 = wave_sum(s1);
                s2 = wave_sum(s2);
                if (lane == 0) {
                    part[wave][k * PLOSS_QK + PLOSS_Q_S1 + i] = s1;
                    part[wave][k * PLOSS_QK + PLOSS_Q_S2 + i] = s2;
                }
            }
            if (i == PLOSS_METRIC_PRED) ploss_epe(dc, g[k], m[k], &part[wave][k * PLOSS_QK + PLOSS_Q_EPE3], lane);
        }
        dc = dn;
#pragma unroll
        for (int j = 0; j < DKT_PCV_LOSS_MAX_M; ++j)
            if (j < M) mc[j] = mn[j];
    }
    bad = wave_or(bad);
    if (lane == 0) flag[wave] = bad;
    __syncthreads();
    for (int q = tid; q < K * PLOSS_QK; q += PLOSS_THREADS) {
        double s = part[0][q];
        for (int w = 1; w < PLOSS_WAVES; ++w) s += part[w][q];
        ws[q * nblk + blk] = s;
    }
    if (tid == 0) {
        unsigned long long f = 0;
        for (int w = 0; w < PLOSS_WAVES; ++w) f |= flag[w];
        ((unsigned long long *)(ws + (long)K * PLOSS_QK * nblk))[blk] = f;
    }
}

__global__ __launch_bounds__(PLOSS_FIN_THREADS) void pcv_loss_finalize_kernel(dkt_pcv_loss_desc d, const double *__restrict__ ws, int nblk) {
    __shared__ double tot[2 * PLOSS_QK];
    __shared__ unsigned long long flags[PLOSS_FIN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = d.ntargets, R = K * PLOSS_QK;
    // one wave per quantity, summed over the blocks in wave_reduce.h's column order
    for (int q = wave; q < R; q += PLOSS_FIN_THREADS / 64) {
        const double s = column_sum(ws + (long)q * nblk, nblk);
        if (lane == 0) tot[q] = s;
    }
    const unsigned long long *fw = (const unsigned long long *)(ws + (long)R * nblk);
    unsigned long long f = 0;
    for (int i = tid; i < nblk; i += PLOSS_FIN_THREADS) f |= fw[i];
    f = wave_or(f);
    if (lane == 0) flags[wave] = f;                    // OR: order-independent
    __syncthreads();
    if (tid != 0) return;
    f = 0;
    for (int w = 0; w < PLOSS_FIN_THREADS / 64; ++w) f |= flags[w];
    for (int k = 0; k < K; ++k) {
        const double *t = tot + k * PLOSS_QK;
        const double N = t[0];
        const float nf = (float)N;
        // disp_loss = 0.0; disp_loss += i_weights[i] * (mean1 + mean2); disp_loss += 1.4 * smooth_l1 (fp32 scalar tensors;
        // the mean of an empty set is NaN)
        float loss = 0.0f;
        for (int i = 0; i < d.n_loss; ++i) {
            const float both = __fadd_rn((float)(t[PLOSS_Q_S1 + i] / N), (float)(t[PLOSS_Q_S2 + i] / N));
            loss = __fadd_rn(loss, __fmul_rn(d.weight[i], both));
        }
        loss = __fadd_rn(loss, __fmul_rn(d.refine_weight, (float)(t[PLOSS_Q_SL1] / N)));
        *d.loss[k] = loss;
        double *rec = d.rec + PLOSS_REC_K * k;
        rec[0] = N;
        for (int h = 0; h < 2; ++h) {
            const double *e = t + (h ? PLOSS_Q_EPEF : PLOSS_Q_EPE3);
            double *o = rec + 1 + 7 * h;
            o[0] = (double)(float)(e[0] / N);
            for (int q = 1; q < 7; ++q) o[q] = (double)__fdiv_rn((float)e[q], nf);
        }
        rec[15] = 0.0;
    }
    for (int q = PLOSS_REC_K * K; q < DKT_PCV_LOSS_REC; ++q) d.rec[q] = 0.0;
    d.rec[2 * PLOSS_REC_K] = (double)f;
}

template <bool VEC>
__global__ __launch_bounds__(PLOSS_THREADS) void pcv_loss_bwd_kernel(dkt_pcv_loss_desc d, dkt_pcv_loss_grad gr) {
    const int HW = d.H * d.W, b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, K = d.ntargets, M = d.M;
    float g[2][PLOSS_ITEMS], up[2], nk[2], norm[2];
    bool m[2][PLOSS_ITEMS], on[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        up[k] = 0.0f, nk[k] = 1.0f, norm[k] = 0.0f, on[k] = false;
#pragma unroll
        for (int j = 0; j < PLOSS_ITEMS; ++j) g[k][j] = 0.0f, m[k][j] = false;
        if (k >= K) continue;
        const double N = d.rec[PLOSS_REC_K * k];
        // an empty mask or an absent upstream gradient contributes exactly 0, never 0 * (1 / 0)
        on[k] = gr.grad_loss[k] != nullptr && N > 0.0;
        if (!on[k]) continue;
        up[k] = *gr.grad_loss[k];
        nk[k] = (float)N;
        norm[k] = (float)(1.0 / N);
        const PlossVec gv = ploss_load<VEC>(d.gt[k] + (long)b * d.gt_bstride[k], tile, tid, HW);
#pragma unroll
        for (int j = 0; j < PLOSS_ITEMS; ++j) g[k][j] = gv.v[j];
        ploss_mask_load<VEC>(d.mask[k] + (long)b * HW, m[k], tile, tid, HW);
    }
    if (gr.grefine) {
        const PlossVec rf = ploss_load<VEC>(d.refine + (long)b * d.refine_bstride, tile, tid, HW);
        PlossVec o;
#pragma unroll
        for (int j = 0; j < PLOSS_ITEMS; ++j) o.v[j] = 0.0f;
        bool first = true;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (!on[k]) continue;
            // smooth_l1 backward: x < -beta ? -norm * grad : x > beta ? norm * grad : norm * x * grad / beta, norm = fl32(1 / N)
            const float gw = __fmul_rn(up[k], d.refine_weight);
#pragma unroll
            for (int j = 0; j < PLOSS_ITEMS; ++j) {
                if (!m[k][j]) continue;
                const float x = __fsub_rn(rf.v[j], g[k][j]);
                const float t = x < -1.0f ? __fmul_rn(-norm[k], gw) : (x > 1.0f ? __fmul_rn(norm[k], gw) : __fmul_rn(__fmul_rn(norm[k], x), gw));
                o.v[j] = first ? t : __fadd_rn(o.v[j], t);
            }
            first = false;
        }
        ploss_store<VEC>(gr.grefine + (long)b * HW, o, tile, tid, HW);
    }
    for (int i = 0; i < d.n; ++i) {
        // d(w_i (mean1 + mean2)): upstream * fl32(w_i), the mean's / N, and for mu the mean over the gaussians' / M
        float q[2], qm[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            q[k] = on[k] && i < d.n_loss ? __fdiv_rn(__fmul_rn(up[k], d.weight[i]), nk[k]) : 0.0f;
            qm[k] = __fdiv_rn(q[k], (float)M);
        }
        const int planes = 1 + M;
        for (int pl = 0; pl < planes; ++pl) {
            float *out = pl == 0 ? gr.gdisp[i] : gr.gmu[i];
            if (!out) {
                if (pl == 0) continue;
                break;
            }
            out += pl == 0 ? (long)b * HW : ((long)b * M + (pl - 1)) * HW;
            PlossVec o;
#pragma unroll
            for (int j = 0; j < PLOSS_ITEMS; ++j) o.v[j] = 0.0f;
            if (i < d.n_loss && (on[0] || on[1])) {
                const float *src = pl == 0 ? d.disp[i] + (long)b * d.disp_bstride[i]
                                           : d.mu[i] + (long)b * d.mu_bstride[i] + (long)(pl - 1) * d.mu_gstride[i];
                const PlossVec p = ploss_load<VEC>(src, tile, tid, HW);
                bool first = true;
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    if (!on[k]) continue;
                    const float s = pl == 0 ? q[k] : qm[k];
#pragma unroll
                    for (int j = 0; j < PLOSS_ITEMS; ++j) {
                        if (!m[k][j]) continue;
                        // abs backward: grad * sgn(x), sgn(0) = sgn(NaN) = 0
                        const float x = __fsub_rn(p.v[j], g[k][j]);
                        const float t = __fmul_rn(s, x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f));
                        o.v[j] = first ? t : __fadd_rn(o.v[j], t);
                    }
                    first = false;
                }
            }
            ploss_store<VEC>(out, o, tile, tid, HW);
        }
    }
}

static int pcv_loss_check(const dkt_pcv_loss_desc *d) {
    if (!d) return DKT_E_NULL;
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->n < 1 || d->n > DKT_PCV_LOSS_MAX_PRED || d->n_loss < 1 || d->n_loss > d->n ||
        d->n_loss > PLOSS_MAX_LOSS || d->M < 1 || d->M > DKT_PCV_LOSS_MAX_M || d->ntargets < 1 || d->ntargets > 2)
        return DKT_E_SHAPE;
    if ((long)d->H * d->W > 0x7fffffffL - PLOSS_TILE || d->B > 65535) return DKT_E_UNSUPPORTED;
    for (int i = 0; i < d->n; ++i)
        if (!d->disp[i] || !d->mu[i]) return DKT_E_NULL;
    for (int k = 0; k < d->ntargets; ++k)
        if (!d->gt[k] || !d->valid[k] || !d->mask[k] || !d->loss[k]) return DKT_E_NULL;
    if (!d->refine || !d->rec) return DKT_E_NULL;
    return DKT_OK;
}

// every plane the kernels touch starts on a 16-byte boundary: H W % 4 == 0, the bases aligned, the strides multiples of 4
static bool pcv_loss_vec(const dkt_pcv_loss_desc *d, const dkt_pcv_loss_grad *g) {
    bool vec = ((long)d->H * d->W) % 4 == 0 && dkt_aligned16(d->refine) && d->refine_bstride % 4 == 0;
    for (int i = 0; i < d->n; ++i) {
        vec = vec && dkt_aligned16(d->disp[i]) && d->disp_bstride[i] % 4 == 0;
        vec = vec && dkt_aligned16(d->mu[i]) && d->mu_bstride[i] % 4 == 0 && d->mu_gstride[i] % 4 == 0;
        vec = vec && dkt_aligned16(d->w[i]) && d->w_bstride[i] % 4 == 0 && d->w_gstride[i] % 4 == 0;
        vec = vec && dkt_aligned16(d->sigma[i]) && d->sigma_bstride[i] % 4 == 0 && d->sigma_gstride[i] % 4 == 0;
        if (g) vec = vec && dkt_aligned16(g->gdisp[i]) && dkt_aligned16(g->gmu[i]);
    }
    for (int k = 0; k < d->ntargets; ++k)
        vec = vec && dkt_aligned16(d->gt[k]) && d->gt_bstride[k] % 4 == 0 && dkt_aligned16(d->valid[k]) && d->valid_bstride[k] % 4 == 0 &&
              dkt_aligned16(d->mask[k]);
    if (g) vec = vec && dkt_aligned16(g->grefine);
    return vec;
}

extern "C" long dkt_pcv_loss_partial_doubles(int ntargets, int B, int H, int W) {
    if (ntargets < 1 || ntargets > 2 || B <= 0 || H <= 0 || W <= 0) return DKT_E_SHAPE;
    return ((long)ntargets * PLOSS_QK + 1) * B * ploss_tiles(H, W);
}

extern "C" int dkt_pcv_loss(const dkt_pcv_loss_desc *d, double *ws, int device, void *stream) {
    const int rc = pcv_loss_check(d);
    if (rc != DKT_OK) return rc;
    if (!ws) return DKT_E_NULL;
    DKT_ENTER(device);
    const dim3 grid(ploss_tiles(d->H, d->W), d->B);
    if (pcv_loss_vec(d, nullptr))
        hipLaunchKernelGGL(pcv_loss_partials_kernel<true>, grid, dim3(PLOSS_THREADS), 0, (hipStream_t)stream, *d, ws);
    else
        hipLaunchKernelGGL(pcv_loss_partials_kernel<false>, grid, dim3(PLOSS_THREADS), 0, (hipStream_t)stream, *d, ws);
    hipLaunchKernelGGL(pcv_loss_finalize_kernel, dim3(1), dim3(PLOSS_FIN_THREADS), 0, (hipStream_t)stream, *d, (const double *)ws,
                       (int)(grid.x * grid.y));
    return dkt_launch_status();
}

extern "C" int dkt_pcv_loss_bwd(const dkt_pcv_loss_desc *d, const dkt_pcv_loss_grad *g, int device, void *stream) {
    const int rc = pcv_loss_check(d);
    if (rc != DKT_OK) return rc;
    if (!g) return DKT_E_NULL;
    DKT_ENTER(device);
    const dim3 grid(ploss_tiles(d->H, d->W), d->B);
    if (pcv_loss_vec(d, g))
        hipLaunchKernelGGL(pcv_loss_bwd_kernel<true>, grid, dim3(PLOSS_THREADS), 0, (hipStream_t)stream, *d, *g);
    else
        hipLaunchKernelGGL(pcv_loss_bwd_kernel<false>, grid, dim3(PLOSS_THREADS), 0, (hipStream_t)stream, *d, *g);
    return dkt_launch_status();
}
