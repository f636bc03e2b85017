// volumes_bwd.hip -- backward of the cost-volume builders of volumes.hip for gfx950.
//   dkt_gwc_volume_bwd         group-wise correlation volume -> grad of both feature maps
//   dkt_concat_volume_bwd      concatenation volume (GwcNet / IGEV variants) -> grad of both feature maps
//   dkt_gwc_concat_volume_bwd  both parts of the fused (B, G+2C', D, H, W) buffer in one launch
// Reference: meta_arch/igev_stereo/submodule.py:152-170,207-218, meta_arch/gwcnet/submodules.py:25-58
// (torch autograd through the reference's per-disparity slices).
//
//   gwc:    dL[b,gc,h,w]  = (1/cpg) sum_{d <= w, d < D}       dV[b,g,d,h,w]   * R[b,gc,h,w-d]
//           dR[b,gc,h,w'] = (1/cpg) sum_{d < D, w'+d < W}     dV[b,g,d,h,w'+d] * L[b,gc,h,w'+d]
//   concat: dref[c,w]     = sum_{d < D (, d <= w if masked)}  dV[c,d,h,w]
//           dtgt[c,w']    = sum_{d < D, w'+d < W}             dV[C+c,d,h,w'+d]
//
// Deterministic: no atomics, every output element is owned by one thread and summed in ascending d.
// Memory-bound (~2 GFLOP against ~575 MB at cfg5): one gwc block per (b, g, h) row stages the group's cpg rows of
// L and R in LDS (rows that do not fit are cut along W into chunks with a D-1 column halo) and streams the row's
// D x W slab of dV from global memory: its dL pass reads it from HBM, its dR pass from the caches.  (Staging the
// slab in LDS as well -- 73 KB per block at cfg5, two blocks per CU -- measured 619 us: latency-bound.)
// Plain scalar fp32 (no packed math: DESIGN 3.4).
#include "dkt_common.h"

#define VBWD_THREADS 256
#define VBWD_CB 8                       // channels one thread accumulates at a time (per pixel)
#define VBWD_DB 8                       // disparities whose dV loads are in flight together
#define VBWD_LDS_MAX (32 * 1024)        // >= 4 blocks per CU (160 KiB of LDS)
#define VBWD_MIN_TW 32                  // narrower chunks than this: the halo dominates, use the direct kernel

extern __shared__ __attribute__((aligned(16))) float vbwd_lds[];

struct VbwdArgs {
    const float *gv;      // upstream gradient, channel 0 of the gwc part (batch stride bstride)
    const float *gvc;     // upstream gradient, channel 0 of the concat part (same batch stride)
    long bstride;
    const float *ref, *tgt;
    float *gref, *gtgt;   // gwc feature gradients (either may be null)
    float *gcref, *gctgt; // concat feature gradients (either may be null)
    int C, G, Cc, H, W, D, ref_masked;
    int tw, nchunk;       // gwc W chunk width and count
    int gwc_blocks;       // blocks [0, gwc_blocks) are gwc (row, chunk)s, the rest concat (b, c, h) rows
};

// rows x ncols floats from global (row stride sstride) to LDS (row pitch); four independent loads in flight
__device__ inline void vbwd_stage(float *dst, int pitch, const float *src, size_t sstride, int rows, int ncols) {
    const int n = rows * ncols;
    for (int i0 = threadIdx.x; i0 < n; i0 += VBWD_THREADS * 4) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = min(i0 + VBWD_THREADS * k, n - 1);
            const int r = i / ncols, x = i - r * ncols;
            v[k] = src[(size_t)r * sstride + x];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = i0 + VBWD_THREADS * k;
            if (i < n) {
                const int r = i / ncols, x = i - r * ncols;
                dst[r * pitch + x] = v[k];
            }
        }
    }
}

__device__ inline void vbwd_gwc_row(const VbwdArgs &a, int bid) {
    const int cpg = a.C / a.G, D = a.D, W = a.W, H = a.H;
    const int chunk = bid % a.nchunk;
    const int h = (bid / a.nchunk) % H;
    const int g = (bid / (a.nchunk * H)) % a.G;
    const int b = bid / (a.nchunk * H * a.G);
    const size_t HW = (size_t)H * W;
    const int w0 = chunk * a.tw;
    const int tw = min(a.tw, W - w0);                 // pixels this block owns: [w0, w0 + tw)
    const int P = a.tw + D - 1;                       // LDS row pitch
    const int ncol = min(W - w0, tw + D - 1);         // L columns [w0, w0 + ncol): the dR halo on the right
    float *l_s = vbwd_lds;                            // [cpg][P] L[c][w0 + x]
    float *r_s = l_s + (size_t)cpg * P;               // [cpg][P] R[c][w0 - (D-1) + x]  (the dL halo on the left)
    const float *gvrow = a.gv + (size_t)b * a.bstride + (size_t)g * D * HW + (size_t)h * W;
    const size_t chan0 = ((size_t)b * a.C + (size_t)g * cpg) * HW + (size_t)h * W;
    if (a.gtgt) vbwd_stage(l_s, P, a.ref + chan0 + w0, HW, cpg, ncol);
    if (a.gref) {
        const int rlo = max(0, w0 - (D - 1));         // columns left of the image are never read
        vbwd_stage(r_s + (rlo - (w0 - (D - 1))), P, a.tgt + chan0 + rlo, HW, cpg, w0 + tw - rlo);
    }
    __syncthreads();
    const float fcpg = (float)cpg;
    const int nslice = (cpg + VBWD_CB - 1) / VBWD_CB;
    // dV comes straight from global memory, VBWD_DB disparities per batch of independent loads: the dL pass reads
    // dV[d][w] and the dR pass dV[d][w'+d], consecutive across the lanes either way; the dR pass (and any further
    // channel slice) finds the row's slab in the caches.  Disparities past a pixel's band are clamped in the index and
    // their dV zeroed, so the fma adds an exact 0 and the loads stay unconditional.
    for (int item = threadIdx.x; item < nslice * tw; item += VBWD_THREADS) {
        const int sl = item / tw, x = item - sl * tw, w = w0 + x, c0 = sl * VBWD_CB;
        if (a.gref) {
            float s[VBWD_CB];
#pragma unroll
            for (int k = 0; k < VBWD_CB; ++k) s[k] = 0.0f;
            const int dmax = min(D - 1, w);
            const float *rp = r_s + (size_t)c0 * P + x + D - 1;      // R[c0][w - d] at rp[-d]
            for (int d0 = 0; d0 <= dmax; d0 += VBWD_DB) {
                float gvv[VBWD_DB];
#pragma unroll
                for (int j = 0; j < VBWD_DB; ++j) {
                    const float v = gvrow[(size_t)min(d0 + j, dmax) * HW + w];
                    gvv[j] = d0 + j <= dmax ? v : 0.0f;
                }
#pragma unroll
                for (int j = 0; j < VBWD_DB; ++j) {
                    const int d = min(d0 + j, dmax);
#pragma unroll
                    for (int k = 0; k < VBWD_CB; ++k)
                        if (c0 + k < cpg) s[k] = __fmaf_rn(gvv[j], rp[k * P - d], s[k]);
                }
            }
#pragma unroll
            for (int k = 0; k < VBWD_CB; ++k)
                if (c0 + k < cpg) a.gref[chan0 + (size_t)(c0 + k) * HW + w] = __fdiv_rn(s[k], fcpg);
        }
        if (a.gtgt) {
            float s[VBWD_CB];
#pragma unroll
            for (int k = 0; k < VBWD_CB; ++k) s[k] = 0.0f;
            const int dmax = min(D - 1, W - 1 - w);
            const float *lp = l_s + (size_t)c0 * P + x;               // L[c0][w + d] at lp[d]
            for (int d0 = 0; d0 <= dmax; d0 += VBWD_DB) {
                float gvv[VBWD_DB];
#pragma unroll
                for (int j = 0; j < VBWD_DB; ++j) {
                    const int d = min(d0 + j, dmax);
                    const float v = gvrow[(size_t)d * HW + w + d];
                    gvv[j] = d0 + j <= dmax ? v : 0.0f;
                }
#pragma unroll
                for (int j = 0; j < VBWD_DB; ++j) {
                    const int d = min(d0 + j, dmax);
#pragma unroll
                    for (int k = 0; k < VBWD_CB; ++k)
                        if (c0 + k < cpg) s[k] = __fmaf_rn(gvv[j], lp[k * P + d], s[k]);
                }
            }
#pragma unroll
            for (int k = 0; k < VBWD_CB; ++k)
                if (c0 + k < cpg) a.gtgt[chan0 + (size_t)(c0 + k) * HW + w] = __fdiv_rn(s[k], fcpg);
        }
    }
}

// One (b, c, h) row of the concatenation volume's gradient: banded sums straight from HBM (each dV element is read
// by exactly one thread; consecutive lanes read consecutive addresses).
__device__ inline void vbwd_concat_row(const VbwdArgs &a, int bid) {
    const int D = a.D, W = a.W, H = a.H;
    const int h = bid % H;
    const int c = (bid / H) % a.Cc;
    const int b = bid / (H * a.Cc);
    const size_t HW = (size_t)H * W;
    const float *gr = a.gvc + (size_t)b * a.bstride + (size_t)c * D * HW + (size_t)h * W;
    const float *gt = a.gvc + (size_t)b * a.bstride + (size_t)(a.Cc + c) * D * HW + (size_t)h * W;
    const size_t o = ((size_t)b * a.Cc + c) * HW + (size_t)h * W;
    for (int w = threadIdx.x; w < W; w += VBWD_THREADS) {
        if (a.gcref) {
            // masked (GwcNet): the reference half exists only where w >= d; IGEV copies it into every plane
            const int dmax = a.ref_masked ? min(D - 1, w) : D - 1;
            float s = 0.0f;
#pragma unroll 8
            for (int d = 0; d <= dmax; ++d) s = __fadd_rn(s, gr[(size_t)d * HW + w]);
            a.gcref[o + w] = s;
        }
        if (a.gctgt) {
            const int dmax = min(D - 1, W - 1 - w);
            float s = 0.0f;
#pragma unroll 8
            for (int d = 0; d <= dmax; ++d) s = __fadd_rn(s, gt[(size_t)d * HW + w + d]);
            a.gctgt[o + w] = s;
        }
    }
}

__global__ __launch_bounds__(VBWD_THREADS) void volumes_bwd_kernel(VbwdArgs a) {
    const int bid = blockIdx.x;
    if (bid < a.gwc_blocks)
        vbwd_gwc_row(a, bid);
    else
        vbwd_concat_row(a, bid - a.gwc_blocks);
}

// Shapes whose gwc tile does not fit the LDS budget (very deep volumes with wide groups): one thread per output
// element, operands from global memory (L2), same ascending-d order.
__global__ __launch_bounds__(VBWD_THREADS) void gwc_bwd_direct_kernel(VbwdArgs a) {
    const int cpg = a.C / a.G, D = a.D, W = a.W, H = a.H;
    const int h = blockIdx.x % H;
    const int c = (blockIdx.x / H) % a.C;
    const int b = blockIdx.x / (H * a.C);
    const int g = c / cpg;
    const size_t HW = (size_t)H * W;
    const size_t row = ((size_t)b * a.C + c) * HW + (size_t)h * W;
    const float *gvrow = a.gv + (size_t)b * a.bstride + (size_t)g * D * HW + (size_t)h * W;
    const float fcpg = (float)cpg;
    for (int w = threadIdx.x; w < W; w += VBWD_THREADS) {
        if (a.gref) {
            float s = 0.0f;
            for (int d = 0; d <= min(D - 1, w); ++d) s = __fmaf_rn(gvrow[(size_t)d * HW + w], a.tgt[row + w - d], s);
            a.gref[row + w] = __fdiv_rn(s, fcpg);
        }
        if (a.gtgt) {
            float s = 0.0f;
            for (int d = 0; d <= min(D - 1, W - 1 - w); ++d) s = __fmaf_rn(gvrow[(size_t)d * HW + w + d], a.ref[row + w + d], s);
            a.gtgt[row + w] = __fdiv_rn(s, fcpg);
        }
    }
}

// Widest W chunk whose tile (the L and R rows of the group, pitch tw + D - 1) fits VBWD_LDS_MAX, balanced over the
// chunks; 0 when even VBWD_MIN_TW does not fit.
static int vbwd_chunk(int W, int D, int cpg, int *nchunk, size_t *lds) {
    const long per_col = 2L * cpg;
    long tw = (long)(VBWD_LDS_MAX / sizeof(float)) / per_col - (D - 1);
    if (tw < VBWD_MIN_TW && tw < W) return 0;
    if (tw > W) tw = W;
    *nchunk = (int)((W + tw - 1) / tw);
    tw = (W + *nchunk - 1) / *nchunk;
    *lds = (size_t)per_col * (tw + D - 1) * sizeof(float);
    return (int)tw;
}

static int vbwd_launch(VbwdArgs a, int B, int device, void *stream) {
    const bool gwc = a.G > 0 && (a.gref || a.gtgt);
    const bool cat = a.Cc > 0 && (a.gcref || a.gctgt);
    size_t lds = 0;
    int nchunk = 1, tw = 0;
    if (gwc) tw = vbwd_chunk(a.W, a.D, a.C / a.G, &nchunk, &lds);
    const unsigned long long gwc_blocks = gwc && tw ? (unsigned long long)B * a.G * a.H * nchunk : 0;
    const unsigned long long cat_blocks = cat ? (unsigned long long)B * a.Cc * a.H : 0;
    const unsigned long long direct_blocks = gwc && !tw ? (unsigned long long)B * a.C * a.H : 0;
    if (gwc_blocks + cat_blocks > 0x7FFFFFFFull || direct_blocks > 0x7FFFFFFFull) return DKT_E_SHAPE;
    a.tw = tw;
    a.nchunk = nchunk;
    a.gwc_blocks = (int)gwc_blocks;
    if (!cat) a.Cc = 1;                              // (unused; keeps the decomposition free of a zero divisor)
    DKT_ENTER(device);
    hipStream_t st = (hipStream_t)stream;
    if (direct_blocks) {
        hipLaunchKernelGGL(gwc_bwd_direct_kernel, dim3((unsigned)direct_blocks), dim3(VBWD_THREADS), 0, st, a);
        int rc = dkt_launch_status();
        if (rc) return rc;
    }
    if (gwc_blocks + cat_blocks == 0) return DKT_OK;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)volumes_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(volumes_bwd_kernel, dim3((unsigned)(gwc_blocks + cat_blocks)), dim3(VBWD_THREADS), lds, st, a);
    return dkt_launch_status();
}

static int vbwd_check_gwc(const float *ref, const float *tgt, const float *grad_ref, const float *grad_tgt, int C, int G) {
    if (!ref || !tgt || (!grad_ref && !grad_tgt)) return DKT_E_NULL;
    if (C <= 0 || G <= 0) return DKT_E_SHAPE;
    if (C % G != 0) return DKT_E_GROUPS;
    return DKT_OK;
}

extern "C" int dkt_gwc_volume_bwd(const float *grad_vol, long vol_bstride, const float *ref, const float *tgt,
                                  float *grad_ref, float *grad_tgt, int B, int C, int H, int W, int D, int G,
                                  int device, void *stream) {
    if (!grad_vol) return DKT_E_NULL;
    int rc = vbwd_check_gwc(ref, tgt, grad_ref, grad_tgt, C, G);
    if (rc) return rc;
    if (B <= 0 || H <= 0 || W <= 0 || D <= 0) return DKT_E_SHAPE;
    if (vol_bstride < (long)G * D * H * W) return DKT_E_SHAPE;
    VbwdArgs a = {};
    a.gv = grad_vol;
    a.bstride = vol_bstride;
    a.ref = ref;
    a.tgt = tgt;
    a.gref = grad_ref;
    a.gtgt = grad_tgt;
    a.C = C;
    a.G = G;
    a.H = H;
    a.W = W;
    a.D = D;
    return vbwd_launch(a, B, device, stream);
}

extern "C" int dkt_concat_volume_bwd(const float *grad_vol, long vol_bstride, float *grad_ref, float *grad_tgt,
                                     int B, int C, int H, int W, int D, int ref_masked, int device, void *stream) {
    if (!grad_vol || (!grad_ref && !grad_tgt)) return DKT_E_NULL;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || D <= 0) return DKT_E_SHAPE;
    if (vol_bstride < 2L * C * D * H * W) return DKT_E_SHAPE;
    VbwdArgs a = {};
    a.gvc = grad_vol;
    a.bstride = vol_bstride;
    a.gcref = grad_ref;
    a.gctgt = grad_tgt;
    a.Cc = C;
    a.H = H;
    a.W = W;
    a.D = D;
    a.ref_masked = ref_masked ? 1 : 0;
    return vbwd_launch(a, B, device, stream);
}

extern "C" int dkt_gwc_concat_volume_bwd(const float *grad_vol, long vol_bstride, const float *ref, const float *tgt,
                                         float *grad_ref, float *grad_tgt, int B, int C, int G,
                                         float *grad_cat_ref, float *grad_cat_tgt, int Cc, int ref_masked,
                                         int H, int W, int D, int device, void *stream) {
    if (!grad_vol) return DKT_E_NULL;
    const bool gwc = grad_ref || grad_tgt, cat = grad_cat_ref || grad_cat_tgt;
    if (!gwc && !cat) return DKT_E_NULL;
    if (gwc) {
        int rc = vbwd_check_gwc(ref, tgt, grad_ref, grad_tgt, C, G);
        if (rc) return rc;
    }
    if (B <= 0 || H <= 0 || W <= 0 || D <= 0 || G <= 0 || Cc <= 0) return DKT_E_SHAPE;
    if (vol_bstride < ((long)G + 2L * Cc) * D * H * W) return DKT_E_SHAPE;
    VbwdArgs a = {};
    a.gv = grad_vol;
    a.gvc = grad_vol + (size_t)G * D * H * W;
    a.bstride = vol_bstride;
    a.ref = ref;
    a.tgt = tgt;
    a.gref = grad_ref;
    a.gtgt = grad_tgt;
    a.gcref = grad_cat_ref;
    a.gctgt = grad_cat_tgt;
    a.C = C;
    a.G = gwc ? G : 0;
    a.Cc = Cc;
    a.H = H;
    a.W = W;
    a.D = D;
    a.ref_masked = ref_masked ? 1 : 0;
    return vbwd_launch(a, B, device, stream);
}
