// dkt_adamw_step: the optimizer step of tools/ft_dkt.py:243-246 (AdamW of :58),
//     scaler.unscale_(optimizer); clip_grad_norm_(model.parameters(), 1.0); scaler.step(optimizer)
// for every parameter of the model in at most three launches and without a host read.  The parameters are a list of tensors
// of arbitrary sizes behind device tables of pointers (p, g, exp_avg, exp_avg_sq) and of offsets; the walk over fixed tiles
// of OPT_TILE elements is flat_walk.h's, the fixed-order sums are wave_reduce.h's, and the kernels below hold their
// element arithmetic.
//
// (a) adamw_norm_kernel     partial[tile] = sum of g^2 over the tile, in fp64 (each square is exact in fp64; the 2048 terms
//                           are added thread, wave, block in a fixed tree), so the value belongs to the TILE and does not depend
//                           on the grid; one integer atomicOr raises `nonfinite` when an element of g is inf or nan.
// (b) adamw_finalize_kernel one block: adds partial[] in a fixed order (thread t takes t, t + 256, ...; then the same tree),
//                               inv        = fl32(inv_scale * (1 / (double)*grad_scale))        (grad_scale null: inv_scale)
//                               total_norm = fl32(sqrt(sum) * (double)inv)
//                               clip       = min(1, fl32(max_norm / fl32(total_norm + 1e-6f)))  (max_norm < 0: 1; +inf: 1, norm only)
//                               skipped    = nonfinite | (*found_inf != 0)
//                           increments the device step counter when not skipped, writes record = {total_norm, clip, skipped, inv}
//                           and clears `nonfinite` for the next call.
// (c) adamw_update_kernel   returns at once when record says skipped.  Per block, once, in fp64 from the device step counter t:
//                               bc1 = 1 - beta1^t, bc2 = 1 - beta2^t, step_size = fl32(lr / bc1), sbc2 = fl32(sqrt(bc2)),
//                           and per element, every operation rounded to fp32 on its own (-ffp-contract=off):
//                               g1 = g * inv;  g2 = g1 * clip
//                               m' = m + omb1 * (g2 - m)                     omb1 = fl32(1 - beta1)
//                               v' = b2 * v + (omb2 * g2) * g2               b2 = fl32(beta2), omb2 = fl32(1 - beta2)
//                               p1 = p * decay                               decay = fl32(1 - lr * weight_decay)
//                               denom = sqrtf(v') / sbc2 + eps
//                               p' = p1 - step_size * (m' / denom)
//                           (torch.optim.AdamW's single-tensor sequence: mul_, lerp_, mul_/addcmul_, sqrt/div/add_, addcdiv_.)
//                           g is NOT rewritten: the clipped gradient exists in registers only.  absmax (optional): max |p'| per
//                           tensor by the integer atomic max of flat_walk.h (max|p| of the unchanged tensor on a skipped step).
// Without clipping, scaling and found_inf only (c) runs: it takes t = counter + 1, and the block that finishes last (an
// integer ticket) stores the counter and the record {-1, 1, 0, 1}.  No float atomics anywhere: every output is bit-identical
// from run to run and for every grid size.  Memory traffic: 28 B per parameter in (c), 4 B in (a), plus the tables.
#include "dkt_common.h"
#include "flat_walk.h"

#include <math.h>

#define OPT_THREADS 256
#define OPT_ITEMS 8
#define OPT_TILE (OPT_THREADS * OPT_ITEMS)
#define OPT_WS_HEADER 64          // bytes: int nonfinite, unsigned ticket, padding; then one double per tile

struct AdamwArgs {
    float *const *p;
    const float *const *g;
    float *const *m;
    float *const *v;
    const long *off;
    int count;
    double lr, beta1, beta2, eps, wd, max_norm;
    float inv_scale;
    const float *grad_scale;
    const float *found_inf;
    float *step;
    float *record;
    unsigned *absmax;
    int *nonfinite;
    unsigned *ticket;
    double *partial;
    int full;                     // (a) and (b) have run: record and the counter are theirs
};

__global__ __launch_bounds__(OPT_THREADS) void adamw_norm_kernel(const float *const *__restrict__ gp, const long *__restrict__ off,
                                                               int count, double *__restrict__ partial, int *__restrict__ nonfinite) {
    __shared__ double red[OPT_THREADS / 64];
    __shared__ int bad_any;
    const int tid = threadIdx.x;
    if (tid == 0) bad_any = 0;
    __syncthreads();
    int bad = 0;
    float x[OPT_ITEMS];           // the thread's items of the current tile; 0 where it has none
#pragma unroll
    for (int j = 0; j < OPT_ITEMS; ++j) x[j] = 0.f;
    // x[] is all zero whenever a tile starts: done() zeroes every slot it has read, so a boundary tile that leaves its
    // loop early (element() fills only the slots the thread has) still sums zeros for the rest
    flat_walk<OPT_THREADS, OPT_ITEMS>(
        off, count, nullptr, nullptr,
        [&](int k, long base, long end) {
            const float *__restrict__ g = gp[k] - off[k];
#pragma unroll
            for (int j = 0; j < OPT_ITEMS; ++j) {
                const long e = base + j * OPT_THREADS + tid;
                x[j] = e < end ? g[e] : 0.f;
            }
            return 0u;
        },
        [&](int k, long i, int j) {
            x[j] = gp[k][i];          // (not squared here: the loads of a boundary tile stay in flight together)
            return 0u;
        },
        [&](long tile) {
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < OPT_ITEMS; ++j) {
                const double d = (double)x[j];
                acc += d * d;
                bad |= !isfinite(x[j]);
                x[j] = 0.f;
            }
            const double s = block_sum<OPT_THREADS / 64>(acc, red);
            if (tid == 0) partial[tile] = s;
        });
    if (bad) bad_any = 1;         // (any writer writes the same value)
    __syncthreads();
    if (tid == 0 && bad_any) atomicOr(nonfinite, 1);
}

__global__ __launch_bounds__(OPT_THREADS) void adamw_finalize_kernel(AdamwArgs a) {
    __shared__ double red[OPT_THREADS / 64];
    const long total = a.off[a.count];
    const long tiles = (total + OPT_TILE - 1) / OPT_TILE;
    double acc = 0.0;
    for (long i = threadIdx.x; i < tiles; i += OPT_THREADS) acc += a.partial[i];
    const double sum = block_sum<OPT_THREADS / 64>(acc, red);
    if (threadIdx.x == 0) {
        float inv = a.inv_scale;
        if (a.grad_scale) inv = (float)((double)a.inv_scale * (1.0 / (double)*a.grad_scale));
        const float tn = (float)(sqrt(sum) * (double)inv);
        float clip = 1.f;
        if (a.max_norm >= 0.0) {
            const float den = tn + 1e-6f;
            const float c = (float)a.max_norm / den;
            clip = c < 1.f ? c : 1.f;
        }
        int bad = *a.nonfinite != 0;
        if (a.found_inf && *a.found_inf != 0.f) bad = 1;
        if (!bad) *a.step = *a.step + 1.f;
        a.record[0] = tn;
        a.record[1] = clip;
        a.record[2] = bad ? 1.f : 0.f;
        a.record[3] = inv;
        *a.nonfinite = 0;
    }
}

struct AdamwConst {
    float inv, clip, omb1, b2, omb2, decay, sbc2, eps, step_size;
};

__device__ __forceinline__ float adamw_element(float &p, float g, float &m, float &v, const AdamwConst &c) {
    const float g1 = g * c.inv;
    const float g2 = g1 * c.clip;
    const float d = g2 - m;
    const float md = c.omb1 * d;
    const float mn = m + md;
    const float va = c.b2 * v;
    const float vb = c.omb2 * g2;
    const float vc = vb * g2;
    const float vn = va + vc;
    const float p1 = p * c.decay;
    const float sq = sqrtf(vn);
    const float dn = sq / c.sbc2;
    const float denom = dn + c.eps;
    const float q = mn / denom;
    const float u = c.step_size * q;
    const float pn = p1 - u;
    p = pn;
    m = mn;
    v = vn;
    return fabsf(pn);
}

__global__ __launch_bounds__(OPT_THREADS) void adamw_update_kernel(AdamwArgs a) {
    __shared__ unsigned red[OPT_THREADS / 64];
    __shared__ AdamwConst sc;
    __shared__ int s_skip;
    __shared__ float s_step;
    const int tid = threadIdx.x;
    const long *__restrict__ off = a.off;
    const int count = a.count;
    if (tid == 0) {
        float t = *a.step;
        int skip = 0;
        float inv = a.inv_scale, clip = 1.f;
        if (a.full) {
            skip = a.record[2] != 0.f;
            clip = a.record[1];
            inv = a.record[3];
        } else {
            t = t + 1.f;
        }
        const double bc1 = 1.0 - pow(a.beta1, (double)t);
        const double bc2 = 1.0 - pow(a.beta2, (double)t);
        sc.inv = inv;
        sc.clip = clip;
        sc.omb1 = (float)(1.0 - a.beta1);
        sc.b2 = (float)a.beta2;
        sc.omb2 = (float)(1.0 - a.beta2);
        sc.decay = (float)(1.0 - a.lr * a.wd);
        sc.sbc2 = (float)sqrt(bc2);
        sc.eps = (float)a.eps;
        sc.step_size = (float)(a.lr / bc1);
        s_skip = skip;
        s_step = t;
    }
    __syncthreads();
    const AdamwConst c = sc;
    const int skip = s_skip;
    if (skip && !a.absmax) return;
    flat_walk<OPT_THREADS, OPT_ITEMS>(
        off, count, a.absmax, red,
        [&](int k, long base, long end) {
            const long o = off[k];
            float *__restrict__ p = a.p[k] - o;
            unsigned mx = 0;
            if (skip) {
#pragma unroll
                for (int j = 0; j < OPT_ITEMS; ++j) {
                    const long e = base + j * OPT_THREADS + tid;
                    const unsigned u = e < end ? __float_as_uint(fabsf(p[e])) : 0u;
                    mx = u > mx ? u : mx;
                }
            } else {
                const float *__restrict__ g = a.g[k] - o;
                float *__restrict__ m = a.m[k] - o;
                float *__restrict__ v = a.v[k] - o;
                float xp[OPT_ITEMS], xg[OPT_ITEMS], xm[OPT_ITEMS], xv[OPT_ITEMS];
#pragma unroll
                for (int j = 0; j < OPT_ITEMS; ++j) {
                    const long e = base + j * OPT_THREADS + tid;
                    const bool in = e < end;
                    xp[j] = in ? p[e] : 0.f;
                    xg[j] = in ? g[e] : 0.f;
                    xm[j] = in ? m[e] : 0.f;
                    xv[j] = in ? v[e] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < OPT_ITEMS; ++j) {
                    const long e = base + j * OPT_THREADS + tid;
                    if (e < end) {
                        const unsigned u = __float_as_uint(adamw_element(xp[j], xg[j], xm[j], xv[j], c));
                        p[e] = xp[j];
                        m[e] = xm[j];
                        v[e] = xv[j];
                        mx = u > mx ? u : mx;
                    }
                }
            }
            return mx;
        },
        [&](int k, long i, int) {
            if (skip) return __float_as_uint(fabsf(a.p[k][i]));
            float xp = a.p[k][i], xm = a.m[k][i], xv = a.v[k][i];
            const unsigned u = __float_as_uint(adamw_element(xp, a.g[k][i], xm, xv, c));
            a.p[k][i] = xp;
            a.m[k][i] = xm;
            a.v[k][i] = xv;
            return u;
        },
        [](long) {});
    if (!a.full) {
        // the single-launch step: every block has read the counter before it takes its ticket; the last one stores it
        __syncthreads();
        if (tid == 0) {
            __threadfence();
            const unsigned ticket = atomicAdd(a.ticket, 1u);
            if (ticket == gridDim.x - 1) {
                *a.step = s_step;
                a.record[0] = -1.f;
                a.record[1] = 1.f;
                a.record[2] = 0.f;
                a.record[3] = a.inv_scale;
                *a.ticket = 0u;
            }
        }
    }
}

extern "C" long dkt_adamw_workspace(int count, long total) {
    if (count < 0 || total < 0) return -1;
    return OPT_WS_HEADER + (long)sizeof(double) * ((total + OPT_TILE - 1) / OPT_TILE);
}

extern "C" int dkt_adamw_step(float *const *p, const float *const *g, float *const *exp_avg, float *const *exp_avg_sq,
                              const long *n, int count, long total, double lr, double beta1, double beta2, double eps,
                              double weight_decay, double max_norm, float inv_scale, const float *grad_scale,
                              const float *found_inf, float *step, float *record, float *absmax, void *workspace, int grid,
                              int device, void *stream) {
    if (count < 0 || total < 0 || grid < 0) return DKT_E_SHAPE;
    if (!isfinite(lr) || !isfinite(beta1) || !isfinite(beta2) || !isfinite(eps) || !isfinite(weight_decay) ||
        isnan(max_norm) || !isfinite(inv_scale))
        return DKT_E_UNSUPPORTED;
    if (lr < 0.0 || eps < 0.0 || weight_decay < 0.0 || beta1 < 0.0 || beta1 >= 1.0 || beta2 < 0.0 || beta2 >= 1.0)
        return DKT_E_UNSUPPORTED;
    if (count == 0) return DKT_OK;
    if (!p || !g || !exp_avg || !exp_avg_sq || !n || !step || !record || !workspace) return DKT_E_NULL;
    DKT_ENTER(device);
    hipStream_t st = (hipStream_t)stream;
    if (absmax) {
        const hipError_t e = hipMemsetAsync(absmax, 0, (size_t)count * sizeof(float), st);
        if (e != hipSuccess) return (int)e;
    }
    AdamwArgs a;
    a.p = p; a.g = g; a.m = exp_avg; a.v = exp_avg_sq; a.off = n; a.count = count;
    a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.wd = weight_decay; a.max_norm = max_norm;
    a.inv_scale = inv_scale; a.grad_scale = grad_scale; a.found_inf = found_inf;
    a.step = step; a.record = record; a.absmax = (unsigned *)absmax;
    a.nonfinite = (int *)workspace;
    a.ticket = (unsigned *)workspace + 1;
    a.partial = (double *)((char *)workspace + OPT_WS_HEADER);
    a.full = max_norm >= 0.0 || grad_scale || found_inf || inv_scale != 1.f;
    long blocks = flat_walk_blocks((total + OPT_TILE - 1) / OPT_TILE);
    if (grid > 0) blocks = grid;          // (tests)
    if (a.full) {
        hipLaunchKernelGGL(adamw_norm_kernel, dim3((unsigned)blocks), dim3(OPT_THREADS), 0, st, g, n, count, a.partial, a.nonfinite);
        hipLaunchKernelGGL(adamw_finalize_kernel, dim3(1), dim3(OPT_THREADS), 0, st, a);
    }
    hipLaunchKernelGGL(adamw_update_kernel, dim3((unsigned)blocks), dim3(OPT_THREADS), 0, st, a);
    return dkt_launch_status();
}
