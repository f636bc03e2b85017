// upsample_train.hip -- convex up-sampling on the training path (RAFTStereo._forward_train, once per refinement iteration):
//   dkt_convex_upsample_fwd   the leading Dout <= D channels of RAFTStereo.upsample_flow,
//                             meta_arch/raft_stereo/raft_stereo.py:70-82, bit-identical to dkt_convex_upsample(...)[:, :Dout]
//   dkt_convex_upsample_bwd   its gradient with respect to flow and mask (torch autograd through :70-82), the softmax
//                             recomputed from the mask: nothing but flow and mask is saved
//
//   p_k = softmax_k(mask[n,(k*f+i)*f+j,h,w]),  v_{d,k} = f * flow[n,d,h+k/3-1,w+k%3-1]  (0 outside)
//   out[n,d,f*h+i,f*w+j]        = sum_k p_k v_{d,k}
//   a_k = sum_{d<Dout} g_d v_{d,k},  s = sum_k p_k a_k,   gmask[n,(k*f+i)*f+j,h,w] = p_k (a_k - s)
//   gflow[n,d,y,x] = f * sum_k C[n,d,k,y-k/3+1,x-k%3+1],  C[n,d,k,h,w] = sum_{i,j} p_k(i,j,h,w) g[n,d,f*h+i,f*w+j]
//
// HBM-bound: the mask (9*f*f floats per coarse pixel) is read once and its gradient written once.  The threads sit in the
// mask's own layout: a block is f waves over 64 consecutive coarse pixels of one image (flattened h*W+w), wave i owns
// fine row i and loops over j, so every mask / gmask access of a wave is 256 contiguous bytes of one (k, i, j) plane and
// every out / gout access is f contiguous floats per lane (one 4-, 8- or 16-byte access; two 16-byte ones for f = 8).
//
// Deterministic, no atomics.  C is summed by one owner per element in a fixed order: thread (i, h, w) adds its f terms
// in ascending j, the f per-row sums meet in LDS and one thread adds them in ascending i, and the result goes to a
// workspace of 9 * Dout floats per coarse pixel (Dout / f^2 of the mask).  A second launch owns one gflow element per
// thread, adds its (up to 9) in-image C terms in ascending k and multiplies by f.  Two launches rather than one
// tile-with-halo launch: a halo means reading the halo pixels' mask again (+16 % of the dominant traffic for a 64 x 16
// tile), the workspace round trip is 2 * 9 * Dout floats per coarse pixel against the 2 * 9 f^2 of mask and gmask (6 %
// at f = 4, Dout = 1), and no shape needs a special case.
// The softmax, the taps, the row accesses, the meeting of the row sums and the second launch are the nine-tap core of
// ups9.h, shared with context_upsample_train.hip; here are the two kernels that read the mask in its own layout.
// Plain scalar fp32 (no packed math: DESIGN 3.4).
#include "ups9.h"

#define UPS_DC 2                        // channels one pass keeps in registers (RAFT: D = 2, training Dout = 1)

// the nine logits of one fine pixel; all f * 9 loads of a thread are issued before the first softmax waits for one
__device__ __forceinline__ void ups_load9(const float *__restrict__ mp, long kstride, float (&m)[9]) {
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = mp[(long)k * kstride];
}

// v_{d,k} of one coarse pixel; fp = flow + (n*D + d)*H*W
__device__ __forceinline__ float ups_tap(const float *__restrict__ fp, int h, int w, int k, int H, int W, float ff) {
    const int hh = h + k / 3 - 1, ww = w + k % 3 - 1;
    return (hh >= 0 && hh < H && ww >= 0 && ww < W) ? __fmul_rn(ff, fp[(long)hh * W + ww]) : 0.0f;
}

// block (64 * F): wave i = fine row i of 64 consecutive coarse pixels of image blockIdx.y; channels [d0, d0 + UPS_DC)
template <int F>
__global__ __launch_bounds__(64 * F) void ups_fwd_kernel(const float *__restrict__ flow, const float *__restrict__ mask,
                                                         float *__restrict__ out, int D, int Dout, int d0, int H, int W) {
    const long HW = (long)H * W;
    const int p = blockIdx.x * 64 + (threadIdx.x & 63);                    // H * W < 2^31 (ups9_check)
    if (p >= HW) return;
    const int i = threadIdx.x >> 6, n = blockIdx.y;
    const int h = p / W, w = p - h * W;
    float v[UPS_DC][9], acc[UPS_DC][F];
    int dch[UPS_DC];
    bool on[UPS_DC];
#pragma unroll
    for (int dd = 0; dd < UPS_DC; ++dd) on[dd] = d0 + dd < Dout, dch[dd] = min(d0 + dd, Dout - 1);
    ups9_taps_load<UPS_DC>(flow + (long)n * D * HW, HW, dch, h, w, H, W, v);
    const float *mp = mask + ((long)n * 9 * F * F + (long)i * F) * HW + p;
    float mm[F][9];
#pragma unroll
    for (int j = 0; j < F; ++j) ups_load9(mp + (long)j * HW, (long)F * F * HW, mm[j]);
    ups9_taps_finish<UPS_DC>(v, on, h, w, H, W, (float)F);
#pragma unroll
    for (int j = 0; j < F; ++j) {
        float (&m)[9] = mm[j];
        ups9_softmax(m);
#pragma unroll
        for (int dd = 0; dd < UPS_DC; ++dd) {
            float a = 0.0f;
#pragma unroll
            for (int k = 0; k < 9; ++k) a = __fadd_rn(a, __fmul_rn(m[k], v[dd][k]));
            acc[dd][j] = a;
        }
    }
#pragma unroll
    for (int dd = 0; dd < UPS_DC; ++dd)
        if (d0 + dd < Dout)
            ups9_store_row<F>(out + ((((long)n * Dout + d0 + dd) * H + h) * F + i) * ((long)W * F) + (long)w * F, acc[dd]);
}

// Same mapping.  gmask (when non-null; only the pass with d0 == 0 gets it) needs every channel of a_k: the pass's own
// channels come from registers, channels beyond them (Dout > UPS_DC) are read again from global memory.
// ws (when non-null) receives C for the pass's channels.  MORE = Dout > UPS_DC: only that instantiation carries the loop
// over the further channels (its loads would put a full wait, stores included, in front of every j of the common case).
template <int F, bool MORE>
__global__ __launch_bounds__(64 * F) void ups_bwd_kernel(const float *__restrict__ gout, long gbs, const float *__restrict__ flow,
                                                         const float *__restrict__ mask, float *__restrict__ gmask,
                                                         float *__restrict__ ws, int D, int Dout, int d0, int H, int W) {
    __shared__ float red[F][UPS_DC * 9][64];
    const long HW = (long)H * W;
    const int lane = threadIdx.x & 63, i = threadIdx.x >> 6, n = blockIdx.y;
    const int p = blockIdx.x * 64 + lane;                                  // H * W < 2^31 (ups9_check)
    const bool live = p < HW;
    const long Wf = (long)W * F, Hf = (long)H * F;
    float c[UPS_DC][9];
#pragma unroll
    for (int dd = 0; dd < UPS_DC; ++dd)
#pragma unroll
        for (int k = 0; k < 9; ++k) c[dd][k] = 0.0f;
    if (live) {
        const int h = p / W, w = p - h * W;
        const float *gp = gout + (long)n * gbs + ((long)h * F + i) * Wf + (long)w * F;      // channel 0, this lane's f pixels
        float v[UPS_DC][9], g[UPS_DC][F];
        int dch[UPS_DC];
        bool on[UPS_DC];
#pragma unroll
        for (int dd = 0; dd < UPS_DC; ++dd) on[dd] = d0 + dd < Dout, dch[dd] = min(d0 + dd, Dout - 1);
        ups9_taps_load<UPS_DC>(flow + (long)n * D * HW, HW, dch, h, w, H, W, v);
#pragma unroll
        for (int dd = 0; dd < UPS_DC; ++dd) ups9_load_row<F>(gp + (long)dch[dd] * Hf * Wf, g[dd]);
        const long cbase = ((long)n * 9 * F * F + (long)i * F) * HW + p;
        float mm[F][9];
#pragma unroll
        for (int j = 0; j < F; ++j) ups_load9(mask + cbase + (long)j * HW, (long)F * F * HW, mm[j]);
        ups9_taps_finish<UPS_DC>(v, on, h, w, H, W, (float)F);
#pragma unroll
        for (int dd = 0; dd < UPS_DC; ++dd)
            if (!on[dd]) {
#pragma unroll
                for (int j = 0; j < F; ++j) g[dd][j] = 0.0f;
            }
#pragma unroll
        for (int j = 0; j < F; ++j) {
            float (&m)[9] = mm[j];
            ups9_softmax(m);
            if (gmask) {
                float a[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    a[k] = __fmul_rn(g[0][j], v[0][k]);
#pragma unroll
                    for (int dd = 1; dd < UPS_DC; ++dd) a[k] = __fadd_rn(a[k], __fmul_rn(g[dd][j], v[dd][k]));
                }
                if constexpr (MORE) {
                    for (int d = UPS_DC; d < Dout; ++d) {                   // ascending d, as the channels above
                        const float gd = gp[(long)d * Hf * Wf + j];
                        const float *fp = flow + ((long)n * D + d) * HW;
#pragma unroll
                        for (int k = 0; k < 9; ++k) a[k] = __fadd_rn(a[k], __fmul_rn(gd, ups_tap(fp, h, w, k, H, W, (float)F)));
                    }
                }
                float s = 0.0f;
#pragma unroll
                for (int k = 0; k < 9; ++k) s = __fadd_rn(s, __fmul_rn(m[k], a[k]));
#pragma unroll
                for (int k = 0; k < 9; ++k)
                    gmask[cbase + ((long)k * F * F + j) * HW] = __fmul_rn(m[k], __fsub_rn(a[k], s));
            }
#pragma unroll
            for (int dd = 0; dd < UPS_DC; ++dd)
#pragma unroll
                for (int k = 0; k < 9; ++k) c[dd][k] = __fadd_rn(c[dd][k], __fmul_rn(m[k], g[dd][j]));
        }
    }
    if (!ws) return;                                                        // uniform: a launch argument
    ups9_reduce_rows<F, UPS_DC>(red, c, i, lane, ws, n, Dout, d0, HW);      // every thread comes here: no return above but that one
}

// every sign before every limit
static int ups_check(int N, int D, int Dout, int H, int W, int factor) {
    if (D <= 0 || factor < 1 || Dout < 1 || Dout > D) return DKT_E_SHAPE;
    const int rc = ups9_check(N, H, W);
    if (rc != DKT_OK) return rc;
    if ((factor != 1 && factor != 2 && factor != 4 && factor != 8) || D > 65535) return DKT_E_UNSUPPORTED;
    return DKT_OK;
}

// rows of f floats are moved as one access of min(4 f, 16) bytes
static bool ups_aligned(const void *p, int factor) {
    return ups9_aligned(p, factor >= 4 ? 16 : 4 * factor);
}

template <int F>
static void ups_fwd_launch(const float *flow, const float *mask, float *out, int N, int D, int Dout, int H, int W, hipStream_t st) {
    const dim3 grid = ups9_grid(N, H, W);
    for (int d0 = 0; d0 < Dout; d0 += UPS_DC)
        hipLaunchKernelGGL(ups_fwd_kernel<F>, grid, dim3(64 * F), 0, st, flow, mask, out, D, Dout, d0, H, W);
}

extern "C" int dkt_convex_upsample_fwd(const float *flow, const float *mask, float *out, int N, int D, int Dout, int H, int W,
                                       int factor, int device, void *stream) {
    if (!flow || !mask || !out) return DKT_E_NULL;
    const int rc = ups_check(N, D, Dout, H, W, factor);
    if (rc != DKT_OK) return rc;
    if (!ups_aligned(out, factor)) return DKT_E_ALIGN;
    DKT_ENTER(device);
    hipStream_t st = (hipStream_t)stream;
    switch (factor) {
    case 1: ups_fwd_launch<1>(flow, mask, out, N, D, Dout, H, W, st); break;
    case 2: ups_fwd_launch<2>(flow, mask, out, N, D, Dout, H, W, st); break;
    case 4: ups_fwd_launch<4>(flow, mask, out, N, D, Dout, H, W, st); break;
    default: ups_fwd_launch<8>(flow, mask, out, N, D, Dout, H, W, st); break;
    }
    return dkt_launch_status();
}

template <int F>
static void ups_bwd_launch(const float *gout, long gbs, const float *flow, const float *mask, float *gmask, float *ws,
                           int N, int D, int Dout, int H, int W, hipStream_t st) {
    const dim3 grid = ups9_grid(N, H, W);
    // without a workspace (no flow gradient asked for) one pass gives gmask; with one, a pass per UPS_DC channels
    for (int d0 = 0; d0 < (ws ? Dout : 1); d0 += UPS_DC) {
        if (Dout > UPS_DC)
            hipLaunchKernelGGL((ups_bwd_kernel<F, true>), grid, dim3(64 * F), 0, st, gout, gbs, flow, mask,
                               d0 == 0 ? gmask : nullptr, ws, D, Dout, d0, H, W);
        else
            hipLaunchKernelGGL((ups_bwd_kernel<F, false>), grid, dim3(64 * F), 0, st, gout, gbs, flow, mask, gmask, ws, D, Dout, d0,
                               H, W);
    }
}

extern "C" int dkt_convex_upsample_bwd(const float *gout, long gout_bstride, const float *flow, const float *mask, float *gflow,
                                       float *gmask, float *ws, int N, int D, int Dout, int H, int W, int factor, int device,
                                       void *stream) {
    if (!gout || !flow || !mask || (!gflow && !gmask) || (gflow && !ws)) return DKT_E_NULL;
    const int rc = ups_check(N, D, Dout, H, W, factor);
    if (rc != DKT_OK) return rc;
    if (gout_bstride < (long)Dout * H * factor * W * factor) return DKT_E_SHAPE;
    if (!ups_aligned(gout, factor) || gout_bstride % factor != 0) return DKT_E_ALIGN;
    DKT_ENTER(device);
    hipStream_t st = (hipStream_t)stream;
    float *w = gflow ? ws : nullptr;
    switch (factor) {
    case 1: ups_bwd_launch<1>(gout, gout_bstride, flow, mask, gmask, w, N, D, Dout, H, W, st); break;
    case 2: ups_bwd_launch<2>(gout, gout_bstride, flow, mask, gmask, w, N, D, Dout, H, W, st); break;
    case 4: ups_bwd_launch<4>(gout, gout_bstride, flow, mask, gmask, w, N, D, Dout, H, W, st); break;
    default: ups_bwd_launch<8>(gout, gout_bstride, flow, mask, gmask, w, N, D, Dout, H, W, st); break;
    }
    if (gflow) ups9_gather(ws, gflow, N, D, Dout, H, W, (float)factor, st);
    return dkt_launch_status();
}
