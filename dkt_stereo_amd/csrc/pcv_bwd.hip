// pcv_bwd.hip -- backward of PCVNet's correlation block (meta_arch/pcvnet/corr.py:18-61): what autograd derives for the
// avg_pool2d([1,f]) chain of :29-31 and for __call__(coords, sigma) of :33-51 (bilinear_sampler = grid_sample, zero padding,
// align_corners).  Unlike RAFT's block this one is differentiated with respect to a call argument: sigma reaches the lookup
// with its graph (model.py:141 -> :122), so the lookup's backward has three results:
//   grad_pyr[lv][n, fl] += g e,  grad_pyr[lv][n, fl+1] += g w            (taps outside the row drop out)
//   gcoords[b,g,p] = sum_{lv,s} d,   gsigma[b,g,p] = sum_{lv,s} (s - S/2) d,   d = g (v1m - v0m) / f^lv
// with v0m, v1m the two taps after the out-of-range one is zeroed: out = v1 w + v0 e, w = ix - floor(ix), e = 1 - w and
// ix = x / f^lv, x = (s - S/2) sigma + coords.  A pixel's row at a level is touched by that pixel's G*S taps only, so one thread
// owns (pixel, level) and adds in (g, s) order; one thread owns (pixel, gaussian) of the two small results and sums in ascending
// (level, s) order: no atomics, no workspace, the same bits every run.  Floors and weights are dkt_tap's on the forward's own
// expression.  HBM-bound, lanes along pixels.
#include "dkt_common.h"

struct PcvBwdArgs {
    DktPtrs pyr;              // level i: (B*H*W1, W_i), W_0 = W2, W_{i+1} = W_i / f
    DktMutPtrs gpyr;          // shaped like pyr, zero-initialised, accumulated into
    const float *coords;      // (B,G,H,W1)
    const float *sigma;       // (B,G,H,W1)
    const float *gout;        // (B, L*G*S, H, W1)
    float *gcoords;           // (B,G,H,W1) or null
    float *gsigma;            // (B,G,H,W1) or null
    long HW;
    int G, W2, L, S, f;
};

// thread = (pixel, level); grid.y = level, grid.z = batch (corr1d_lookup_bwd_kernel with G*S taps of per-pixel spacing).
__global__ __launch_bounds__(256) void pcv_lookup_bwd_pyr_kernel(PcvBwdArgs a) {
    const long p = blockIdx.x * 256L + threadIdx.x;
    if (p >= a.HW) return;
    const int lv = blockIdx.y, b = blockIdx.z;
    int wi = a.W2;
    float div = 1.0f;
    for (int i = 0; i < lv; ++i) {
        wi /= a.f;
        div = __fmul_rn(div, (float)a.f);
    }
    float *row = a.gpyr.p[lv] + ((long)b * a.HW + p) * wi;
    const float wm1 = (float)(wi - 1);
    const float hwm1 = __fdiv_rn(wm1, 2.0f);
    const int half = a.S / 2;
    for (int g = 0; g < a.G; ++g) {
        const long pg = ((long)b * a.G + g) * a.HW + p;
        const float c = a.coords[pg], sg = a.sigma[pg];
        const float *go = a.gout + (((long)b * a.L + lv) * a.G * a.S + (long)g * a.S) * a.HW + p;
        for (int s = 0; s < a.S; ++s) {
            const float x = __fadd_rn(__fmul_rn((float)(s - half), sg), c);
            const DktTap t = dkt_tap(__fdiv_rn(x, div), wm1, hwm1);
            const float gv = go[(long)s * a.HW];
            if (t.fl >= 0.0f && t.fl <= wm1) {
                float *q = row + (int)t.fl;
                *q = __fadd_rn(*q, __fmul_rn(gv, t.e));
            }
            if (t.fl + 1.0f >= 0.0f && t.fl + 1.0f <= wm1) {
                float *q = row + (int)t.fl + 1;
                *q = __fadd_rn(*q, __fmul_rn(gv, t.w));
            }
        }
    }
}

// thread = (pixel, gaussian), grid.z = batch, as the forward; every level and sample of the pair in ascending order.
__global__ __launch_bounds__(256) void pcv_lookup_bwd_arg_kernel(PcvBwdArgs a) {
    const long t = blockIdx.x * 256L + threadIdx.x;
    if (t >= a.HW * a.G) return;
    const int g = (int)(t / a.HW);
    const long p = t - (long)g * a.HW;
    const int b = blockIdx.z;
    const long pg = ((long)b * a.G + g) * a.HW + p;
    const float c = a.coords[pg], sg = a.sigma[pg];
    const int half = a.S / 2;
    int wi = a.W2;
    float div = 1.0f;
    float gc = 0.0f, gs = 0.0f;
    for (int lv = 0; lv < a.L; ++lv) {
        const float *row = a.pyr.p[lv] + ((long)b * a.HW + p) * wi;
        const float wm1 = (float)(wi - 1);
        const float hwm1 = __fdiv_rn(wm1, 2.0f);
        const float *go = a.gout + (((long)b * a.L + lv) * a.G * a.S + (long)g * a.S) * a.HW + p;
        for (int s = 0; s < a.S; ++s) {
            const float dx = (float)(s - half);
            const float x = __fadd_rn(__fmul_rn(dx, sg), c);
            const DktTap tp = dkt_tap(__fdiv_rn(x, div), wm1, hwm1);
            float v0 = 0.0f, v1 = 0.0f;
            if (tp.fl >= 0.0f && tp.fl <= wm1) v0 = row[(int)tp.fl];
            if (tp.fl + 1.0f >= 0.0f && tp.fl + 1.0f <= wm1) v1 = row[(int)tp.fl + 1];
            const float d = __fdiv_rn(__fmul_rn(go[(long)s * a.HW], __fsub_rn(v1, v0)), div);
            gc = __fadd_rn(gc, d);
            gs = __fadd_rn(gs, __fmul_rn(dx, d));
        }
        wi /= a.f;
        div = __fmul_rn(div, (float)a.f);
    }
    if (a.gcoords) a.gcoords[pg] = gc;
    if (a.gsigma) a.gsigma[pg] = gs;
}

// 0, or the error both entries return for these level sizes: every level at least 2 wide (the sampler divides by W_i - 1)
static int pcv_levels_status(int W2, int L, int factor) {
    if (W2 <= 0 || factor < 2) return DKT_E_SHAPE;
    if (L < 1 || L > DKT_MAX_LEVELS) return DKT_E_LEVELS;
    int wi = W2;
    for (int i = 1; i < L; ++i) wi /= factor;
    return wi < 2 ? DKT_E_LEVELS : DKT_OK;
}

extern "C" int dkt_pcv_lookup_bwd(const float *const *pyr, const float *coords, const float *sigma, const float *grad_out,
                                  float *const *grad_pyr, float *gcoords, float *gsigma,
                                  int B, int G, int H, int W1, int W2, int L, int S, int factor,
                                  int device, void *stream) {
    if (!pyr || !coords || !sigma || !grad_out) return DKT_E_NULL;
    if (!grad_pyr && !gcoords && !gsigma) return DKT_E_NULL;
    if (B <= 0 || G <= 0 || H <= 0 || W1 <= 0 || S <= 0 || (S & 1) == 0 || B > 65535) return DKT_E_SHAPE;
    const int rc = pcv_levels_status(W2, L, factor);
    if (rc != DKT_OK) return rc;
    PcvBwdArgs a;
    for (int i = 0; i < DKT_MAX_LEVELS; ++i) {
        a.pyr.p[i] = i < L ? pyr[i] : nullptr;
        a.gpyr.p[i] = (grad_pyr && i < L) ? grad_pyr[i] : nullptr;
        if (i < L && (!pyr[i] || (grad_pyr && !grad_pyr[i]))) return DKT_E_NULL;
    }
    a.coords = coords; a.sigma = sigma; a.gout = grad_out; a.gcoords = gcoords; a.gsigma = gsigma;
    a.HW = (long)H * W1;
    a.G = G; a.W2 = W2; a.L = L; a.S = S; a.f = factor;
    DKT_ENTER(device);
    hipStream_t st = (hipStream_t)stream;
    if (grad_pyr) {
        dim3 grid((unsigned)((a.HW + 255) / 256), (unsigned)L, (unsigned)B);
        hipLaunchKernelGGL(pcv_lookup_bwd_pyr_kernel, grid, dim3(256), 0, st, a);
    }
    if (gcoords || gsigma) {
        dim3 grid((unsigned)((a.HW * G + 255) / 256), 1, (unsigned)B);
        hipLaunchKernelGGL(pcv_lookup_bwd_arg_kernel, grid, dim3(256), 0, st, a);
    }
    return dkt_launch_status();
}

// Chain of avg_pool2d([1,f], stride [1,f]) backward passes folded into one pass over level 0 (corr1d_pool_bwd_kernel with a
// run-time factor and floor widths W_{i+1} = W_i / f):
//   T_{L-1} = g_{L-1};  T_i[c] = g_i[c] + (c / f < W_{i+1} ? T_{i+1}[c / f] / f : 0);  out = T_0 / divisor.
// The columns a floor width leaves out of every window receive nothing from below.  f is 2 or 4: the division by f is exact.
struct PcvPoolBwdArgs {
    DktPtrs gpyr;
    float *out;
    long rows;
    int W2, L, f;
    float divisor;
};

__global__ __launch_bounds__(256) void pcv_pool_bwd_kernel(PcvPoolBwdArgs a) {
    const long total = a.rows * a.W2;
    const float ff = (float)a.f;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long n = i / a.W2;
        const int c = (int)(i - n * a.W2);
        // the deepest level whose window still holds column c (c / f^l < W_l is monotone in l)
        int deepest = 0, cd = c, wd = a.W2;
        for (int l = 1; l < a.L; ++l) {
            const int cn = cd / a.f, wn = wd / a.f;
            if (cn >= wn) break;
            deepest = l; cd = cn; wd = wn;
        }
        float t = a.gpyr.p[deepest][n * (long)wd + cd];
        for (int l = deepest - 1; l >= 0; --l) {
            int cl = c, wl = a.W2;
            for (int j = 0; j < l; ++j) {
                cl /= a.f;
                wl /= a.f;
            }
            t = __fadd_rn(a.gpyr.p[l][n * (long)wl + cl], __fdiv_rn(t, ff));
        }
        a.out[i] = __fdiv_rn(t, a.divisor);
    }
}

extern "C" int dkt_pcv_pool_bwd(const float *const *grad_pyr, float *grad_vol, int B, int H, int W1, int W2,
                                int L, int factor, float divisor, int device, void *stream) {
    if (!grad_pyr || !grad_vol) return DKT_E_NULL;
    if (B <= 0 || H <= 0 || W1 <= 0 || !(divisor > 0.0f)) return DKT_E_SHAPE;
    const int rc = pcv_levels_status(W2, L, factor);
    if (rc != DKT_OK) return rc;
    PcvPoolBwdArgs a;
    for (int i = 0; i < DKT_MAX_LEVELS; ++i) {
        a.gpyr.p[i] = i < L ? grad_pyr[i] : nullptr;
        if (i < L && !grad_pyr[i]) return DKT_E_NULL;
    }
    a.out = grad_vol; a.rows = (long)B * H * W1; a.W2 = W2; a.L = L; a.f = factor; a.divisor = divisor;
    DKT_ENTER(device);
    long blocks = (a.rows * W2 + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(pcv_pool_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return dkt_launch_status();
}
