// dkt_seq_loss / dkt_seq_loss_bwd: the sequence losses of RAFT-Stereo (meta_arch/raft_stereo/loss.py:3-40) and GwcNet
// (meta_arch/gwcnet/gwc_loss.py:5-31) against one or two targets, the pair of calls of tools/ft_dkt.py:227-228.
//
// Forward, launch 1 (partials): block = one tile of LOSS_TILE pixels of one image.  The targets and their masks are loaded
// once into registers; then the predictions stream through (the next one's loads are issued before the current one is
// reduced), and each wave reduces every per-prediction sum in a fixed shuffle order into LDS.  The block writes one fp64
// partial per quantity, quantity-major, plus three 64-bit flag words (NaN / Inf per prediction, Inf in gt per target).
// Launch 2 (finalize, one block): every quantity is summed over the blocks in a fixed order, then the losses are formed the
// way the reference does, sum_i fl32(w_i) * mean_i in fp32 in order i, and written as device scalars with the record.
// No float atomics anywhere: the results are bit-identical from run to run.
//
// Backward (one launch): the same tiles; reads the upstream gradients and the mask counts on the device.
#include "dkt_common.h"
#include "wave_reduce.h"

#include <math.h>

#define LOSS_THREADS 256
#define LOSS_ITEMS 4
#define LOSS_TILE (LOSS_THREADS * LOSS_ITEMS)
#define LOSS_WAVES (LOSS_THREADS / 64)
#define LOSS_Q_MAX (2 * (DKT_LOSS_MAX_PRED + 5))   // quantities per block: per target count, n sums, EPE sum, 3 counts
#define LOSS_FLAG_WORDS 3
#define FIN_THREADS 1024

static inline int loss_tiles(int H, int W) { return (int)(((long)H * W + LOSS_TILE - 1) / LOSS_TILE); }

// the per-pixel term of the loss: |p - gt| (loss.py:25) or smooth-L1 with beta = 1 (F.smooth_l1_loss: 0.5 z z / beta or z - 0.5 beta)
__device__ __forceinline__ float loss_term(int kind, float p, float g) {
    const float z = fabsf(__fsub_rn(p, g));
    if (kind == DKT_LOSS_RAFT) return z;
    return z < 1.0f ? __fmul_rn(__fmul_rn(0.5f, z), z) : __fsub_rn(z, 0.5f);
}

__global__ __launch_bounds__(LOSS_THREADS) void seq_loss_partials_kernel(dkt_seq_loss_desc d, double *__restrict__ ws) {
    __shared__ double part[LOSS_WAVES][LOSS_Q_MAX];
    __shared__ unsigned long long flag[LOSS_WAVES][LOSS_FLAG_WORDS];
    const int HW = d.H * d.W, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int QK = d.n + 5, K = d.ntargets;
    const long nblk = (long)gridDim.x * gridDim.y, blk = (long)b * gridDim.x + blockIdx.x;
    const int r0 = blockIdx.x * LOSS_TILE + tid;
    float g[2][LOSS_ITEMS];
    bool m[2][LOSS_ITEMS];
    unsigned long long gtinf = 0, nanb = 0, infb = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (k >= K) continue;
        const float *gp = d.gt[k] + (long)b * d.gt_bstride[k];
        const float *vp = d.valid[k] + (long)b * d.valid_bstride[k];
        unsigned char *mp = d.mask[k] + (long)b * HW;
        double cnt = 0.0;
#pragma unroll
        for (int j = 0; j < LOSS_ITEMS; ++j) {
            const int r = r0 + j * LOSS_THREADS;
            const bool in = r < HW;
            const float gv = in ? gp[r] : 0.0f;
            const float vv = in ? vp[r] : 0.0f;
            // valid = (valid >= 0.5) & (mag < max_flow), mag = sum(gt**2, dim=1).sqrt()
            const bool mk = in && vv >= 0.5f && sqrtf(__fmul_rn(gv, gv)) < d.max_flow;
            if (in) mp[r] = mk ? 1 : 0;
            g[k][j] = gv;
            m[k][j] = mk;
            cnt += mk ? 1.0 : 0.0;
            if (mk && isinf(gv)) gtinf |= 1ull << k;
        }
        cnt = wave_sum(cnt);
        if (lane == 0) part[wave][k * QK] = cnt;
    }
    float pc[LOSS_ITEMS], pn[LOSS_ITEMS];
#pragma unroll
    for (int j = 0; j < LOSS_ITEMS; ++j) {
        const int r = r0 + j * LOSS_THREADS;
        pc[j] = r < HW ? d.pred[0][(long)b * d.pred_bstride[0] + r] : 0.0f;
    }
    for (int i = 0; i < d.n; ++i) {
        if (i + 1 < d.n) {
            const float *pp = d.pred[i + 1] + (long)b * d.pred_bstride[i + 1];
#pragma unroll
            for (int j = 0; j < LOSS_ITEMS; ++j) {
                const int r = r0 + j * LOSS_THREADS;
                pn[j] = r < HW ? pp[r] : 0.0f;
            }
        }
#pragma unroll
        for (int j = 0; j < LOSS_ITEMS; ++j) {
            // out-of-range items hold 0.0f: neither NaN nor Inf
            if (isnan(pc[j])) nanb |= 1ull << i;
            if (isinf(pc[j])) infb |= 1ull << i;
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (k >= K) continue;
            if (i < d.n_loss) {
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < LOSS_ITEMS; ++j)
                    if (m[k][j]) s += (double)loss_term(d.kind, pc[j], g[k][j]);
                s = wave_sum(s);
                if (lane == 0) part[wave][k * QK + 1 + i] = s;
            }
            if (i == d.n - 1) {
                // epe = sum((flow_preds[-1] - flow_gt)**2, dim=1).sqrt() over the mask, and the 1 / 3 / 5 px counts
                double e = 0.0, c1 = 0.0, c3 = 0.0, c5 = 0.0;
#pragma unroll
                for (int j = 0; j < LOSS_ITEMS; ++j) {
                    if (!m[k][j]) continue;
                    const float dd = __fsub_rn(pc[j], g[k][j]);
                    const float ep = sqrtf(__fmul_rn(dd, dd));
                    e += (double)ep;
                    c1 += ep < 1.0f ? 1.0 : 0.0;
                    c3 += ep < 3.0f ? 1.0 : 0.0;
                    c5 += ep < 5.0f ? 1.0 : 0.0;
                }
                e = wave_sum(e);
                c1 = wave_sum(c1);
                c3 = wave_sum(c3);
                c5 = wave_sum(c5);
                if (lane == 0) {
                    part[wave][k * QK + d.n + 1] = e;
                    part[wave][k * QK + d.n + 2] = c1;
                    part[wave][k * QK + d.n + 3] = c3;
                    part[wave][k * QK + d.n + 4] = c5;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < LOSS_ITEMS; ++j) pc[j] = pn[j];
    }
    nanb = wave_or(nanb);
    infb = wave_or(infb);
    gtinf = wave_or(gtinf);
    if (lane == 0) {
        flag[wave][0] = nanb;
        flag[wave][1] = infb;
        flag[wave][2] = gtinf;
    }
    __syncthreads();
    for (int q = tid; q < K * QK; q += LOSS_THREADS) {
        const bool used = (q % QK) == 0 || (q % QK) > d.n || (q % QK) - 1 < d.n_loss;
        double s = 0.0;
        if (used)
            for (int w = 0; w < LOSS_WAVES; ++w) s += part[w][q];
        ws[q * nblk + blk] = s;
    }
    if (tid < LOSS_FLAG_WORDS) {
        unsigned long long f = 0;
        for (int w = 0; w < LOSS_WAVES; ++w) f |= flag[w][tid];
        ((unsigned long long *)(ws + (long)K * QK * nblk))[tid * nblk + blk] = f;
    }
}

__global__ __launch_bounds__(FIN_THREADS) void seq_loss_finalize_kernel(dkt_seq_loss_desc d, const double *__restrict__ ws, int nblk) {
    __shared__ double tot[LOSS_Q_MAX];
    __shared__ unsigned long long flags[LOSS_FLAG_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int QK = d.n + 5, K = d.ntargets, R = K * QK;
    if (tid < LOSS_FLAG_WORDS) flags[tid] = 0;
    __syncthreads();
    // one wave per quantity, summed over the blocks in wave_reduce.h's column order
    for (int q = wave; q < R; q += FIN_THREADS / 64) {
        const double s = column_sum(ws + (long)q * nblk, nblk);
        if (lane == 0) tot[q] = s;
    }
    const unsigned long long *fw = (const unsigned long long *)(ws + (long)R * nblk);
    for (int w = 0; w < LOSS_FLAG_WORDS; ++w) {
        unsigned long long f = 0;
        for (int i = tid; i < nblk; i += FIN_THREADS) f |= fw[(long)w * nblk + i];
        f = wave_or(f);
        if (lane == 0 && f) atomicOr(&flags[w], f);     // OR: order-independent
    }
    __syncthreads();
    if (tid != 0) return;
    for (int k = 0; k < K; ++k) {
        const double *t = tot + k * QK;
        const double N = t[0];
        // flow_loss = 0.0; flow_loss += i_weight * i_loss[valid].mean()  (fp32 scalar tensors; the mean of an empty set is NaN)
        float loss = 0.0f;
        for (int i = 0; i < d.n_loss; ++i) loss = __fadd_rn(loss, __fmul_rn(d.weight[i], (float)(t[1 + i] / N)));
        *d.loss[k] = loss;
        double *rec = d.rec + 8 * k;
        const float nf = (float)N;
        rec[0] = N;
        rec[1] = (double)(float)(t[d.n + 1] / N);
        rec[2] = (double)__fdiv_rn((float)t[d.n + 2], nf);
        rec[3] = (double)__fdiv_rn((float)t[d.n + 3], nf);
        rec[4] = (double)__fdiv_rn((float)t[d.n + 4], nf);
        rec[5] = (flags[2] >> k) & 1 ? 1.0 : 0.0;
        rec[6] = rec[7] = 0.0;
    }
    const unsigned long long all = d.n == 64 ? ~0ull : (1ull << d.n) - 1;
    d.rec[16] = (flags[0] & ~flags[1] & all) ? 1.0 : 0.0;
}

__global__ __launch_bounds__(LOSS_THREADS) void seq_loss_bwd_kernel(dkt_seq_loss_desc d, dkt_seq_loss_grad gr) {
    const int HW = d.H * d.W, b = blockIdx.y, tid = threadIdx.x, K = d.ntargets;
    const int r0 = blockIdx.x * LOSS_TILE + tid;
    float g[2][LOSS_ITEMS], up[2], nk[2];
    bool m[2][LOSS_ITEMS];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        up[k] = nk[k] = 0.0f;
        if (k >= K) continue;
        const float *gp = d.gt[k] + (long)b * d.gt_bstride[k];
        const unsigned char *mp = d.mask[k] + (long)b * HW;
        up[k] = *gr.grad_loss[k];
        const double N = d.rec[8 * k];
        // RAFT: mean backward divides by fl32(N); GWC: smooth_l1 backward multiplies by norm = fl32(1. / N)
        nk[k] = d.kind == DKT_LOSS_RAFT ? (float)N : (float)(1.0 / N);
#pragma unroll
        for (int j = 0; j < LOSS_ITEMS; ++j) {
            const int r = r0 + j * LOSS_THREADS;
            const bool in = r < HW;
            g[k][j] = in ? gp[r] : 0.0f;
            m[k][j] = in && mp[r];
        }
    }
    for (int i = 0; i < d.n; ++i) {
        const float *pp = d.pred[i] + (long)b * d.pred_bstride[i];
        float *op = gr.grad[i] + (long)b * HW;
        float p[LOSS_ITEMS], o[LOSS_ITEMS];
#pragma unroll
        for (int j = 0; j < LOSS_ITEMS; ++j) {
            const int r = r0 + j * LOSS_THREADS;
            p[j] = r < HW && i < d.n_loss ? pp[r] : 0.0f;
            o[j] = 0.0f;
        }
        if (i < d.n_loss) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (k >= K) continue;
                const float gw = __fmul_rn(up[k], d.weight[i]);       // d(w_i * mean_i): upstream * fl32(w_i)
                const float q = __fdiv_rn(gw, nk[k]);                 // RAFT only
#pragma unroll
                for (int j = 0; j < LOSS_ITEMS; ++j) {
                    if (!m[k][j]) continue;
                    const float x = __fsub_rn(p[j], g[k][j]);
                    float t;
                    if (d.kind == DKT_LOSS_RAFT) {
                        // abs backward: grad * sgn(x), sgn(NaN) = 0
                        const float sg = x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f);
                        t = __fmul_rn(q, sg);
                    } else {
                        // smooth_l1 backward: x < -beta ? -norm * grad : x > beta ? norm * grad : norm * x * grad / beta
                        const float norm = nk[k];
                        t = x < -1.0f ? __fmul_rn(-norm, gw) : (x > 1.0f ? __fmul_rn(norm, gw) : __fmul_rn(__fmul_rn(norm, x), gw));
                    }
                    o[j] = k == 0 ? t : __fadd_rn(o[j], t);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < LOSS_ITEMS; ++j) {
            const int r = r0 + j * LOSS_THREADS;
            if (r < HW) op[r] = o[j];
        }
    }
}

static int seq_loss_check(const dkt_seq_loss_desc *d) {
    if (!d) return DKT_E_NULL;
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->n < 1 || d->n > DKT_LOSS_MAX_PRED || d->n_loss < 1 || d->n_loss > d->n ||
        d->ntargets < 1 || d->ntargets > 2)
        return DKT_E_SHAPE;
    if (d->kind != DKT_LOSS_RAFT && d->kind != DKT_LOSS_GWC) return DKT_E_UNSUPPORTED;
    if ((long)d->H * d->W > 0x7fffffffL - LOSS_TILE) return DKT_E_UNSUPPORTED;
    for (int i = 0; i < d->n; ++i)
        if (!d->pred[i]) return DKT_E_NULL;
    for (int k = 0; k < d->ntargets; ++k)
        if (!d->gt[k] || !d->valid[k] || !d->mask[k] || !d->loss[k]) return DKT_E_NULL;
    if (!d->rec) return DKT_E_NULL;
    return DKT_OK;
}

extern "C" long dkt_seq_loss_ws_doubles(int ntargets, int n, int B, int H, int W) {
    if (ntargets < 1 || ntargets > 2 || n < 1 || n > DKT_LOSS_MAX_PRED || B <= 0 || H <= 0 || W <= 0) return DKT_E_SHAPE;
    return ((long)ntargets * (n + 5) + LOSS_FLAG_WORDS) * B * loss_tiles(H, W);
}

extern "C" int dkt_seq_loss(const dkt_seq_loss_desc *d, double *ws, int device, void *stream) {
    const int rc = seq_loss_check(d);
    if (rc != DKT_OK) return rc;
    if (!ws) return DKT_E_NULL;
    DKT_ENTER(device);
    // recipe shape (B = 2, 480 x 896): 840 blocks of 1024 pixels, 3.3 per CU of the 256
    const dim3 grid(loss_tiles(d->H, d->W), d->B);
    hipLaunchKernelGGL(seq_loss_partials_kernel, grid, dim3(LOSS_THREADS), 0, (hipStream_t)stream, *d, ws);
    hipLaunchKernelGGL(seq_loss_finalize_kernel, dim3(1), dim3(FIN_THREADS), 0, (hipStream_t)stream, *d, (const double *)ws,
                       (int)(grid.x * grid.y));
    return dkt_launch_status();
}

extern "C" int dkt_seq_loss_bwd(const dkt_seq_loss_desc *d, const dkt_seq_loss_grad *g, int device, void *stream) {
    const int rc = seq_loss_check(d);
    if (rc != DKT_OK) return rc;
    if (!g) return DKT_E_NULL;
    for (int i = 0; i < d->n; ++i)
        if (!g->grad[i]) return DKT_E_NULL;
    for (int k = 0; k < d->ntargets; ++k)
        if (!g->grad_loss[k]) return DKT_E_NULL;
    DKT_ENTER(device);
    hipLaunchKernelGGL(seq_loss_bwd_kernel, dim3(loss_tiles(d->H, d->W), d->B), dim3(LOSS_THREADS), 0, (hipStream_t)stream, *d, *g);
    return dkt_launch_status();
}
