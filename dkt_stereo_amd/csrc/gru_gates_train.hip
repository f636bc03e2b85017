// gru_gates_train.hip -- the update operator's gates and resamplers on the training path (BasicMultiUpdateBlock under
// autograd, dkt_stereo_amd/gru_train.py).
// Reference: core/update.py:23-32 (== meta_arch/igev_stereo/update.py:33-41) and core/update.py:87-96, and torch autograd
// through those lines.
//
//   dkt_gru_gate_zr_train   dkt_gru_gate_zr (gru_gates.hip) that also writes r:  the same z and rh, bit for bit
//   dkt_gru_gate_out_train  dkt_gru_gate_out that also writes q:                 the same h', bit for bit
//   dkt_gru_gate_out_bwd    gaq = g z (1 - q q),  gz = g (q - h),  gh = g (1 - z)
//   dkt_gru_gate_zr_bwd     gazr = [gz z (1 - z) | grh h r (1 - r)],  gh = grh r
//   dkt_pool2x_bwd          gradient of avg_pool2d(x, 3, stride=2, padding=1)
//   dkt_interp_bilinear_bwd gradient of F.interpolate(x, (Ho,Wo), mode="bilinear", align_corners=True)
//
// The gates are HBM-bound streaming kernels in the shape of gru_gates.hip: float4 accesses when Ch*HW, every batch
// stride and every pointer allow it, a scalar path otherwise, a grid-stride loop over at most 2048 blocks of 256; every
// load of an item is issued before the first use.  The backward of a resampler is a gather: every input element has one
// owner thread, which adds the element's contributors in ascending (oy, ox).  No LDS, no atomics: bit-identical from run
// to run.
// Every product, sum and difference is one explicitly rounded operation (no contraction, whatever the compiler flags).
#include "gru_gates.h"

// ---- forward ---------------------------------------------------------------------------------------------------------
struct GateZrTrainArgs {
    const float *azr, *cz, *cr, *h;
    float *z, *r, *rh;
    long cz_bs, cr_bs, h_bs, rh_bs;
    long CHW;    // Ch*HW
    long total;  // B*CHW/4 (vector path) or B*CHW (scalar path)
};

template <int V>
__global__ __launch_bounds__(256) void gru_gate_zr_train_kernel(GateZrTrainArgs a) {
    const long per_b = a.CHW / V;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < a.total; i += (long)gridDim.x * 256L) {
        const long b = i / per_b;
        const long e = (i - b * per_b) * V;
        const float *paz = a.azr + b * 2 * a.CHW + e;
        const float *par = paz + a.CHW;
        const float *pcz = a.cz + b * a.cz_bs + e;
        const float *pcr = a.cr + b * a.cr_bs + e;
        const float *ph = a.h + b * a.h_bs + e;
        float *pz = a.z + b * a.CHW + e;
        float *pr = a.r + b * a.CHW + e;
        float *prh = a.rh + b * a.rh_bs + e;
        if (V == 4) {
            float4 az = *(const float4 *)paz, ar = *(const float4 *)par;
            float4 cz = *(const float4 *)pcz, cr = *(const float4 *)pcr;
            float4 h = *(const float4 *)ph;
            float4 z, r, rh;
            z.x = dkt_sigmoid(__fadd_rn(az.x, cz.x)); z.y = dkt_sigmoid(__fadd_rn(az.y, cz.y));
            z.z = dkt_sigmoid(__fadd_rn(az.z, cz.z)); z.w = dkt_sigmoid(__fadd_rn(az.w, cz.w));
            r.x = dkt_sigmoid(__fadd_rn(ar.x, cr.x)); r.y = dkt_sigmoid(__fadd_rn(ar.y, cr.y));
            r.z = dkt_sigmoid(__fadd_rn(ar.z, cr.z)); r.w = dkt_sigmoid(__fadd_rn(ar.w, cr.w));
            rh.x = __fmul_rn(r.x, h.x); rh.y = __fmul_rn(r.y, h.y);
            rh.z = __fmul_rn(r.z, h.z); rh.w = __fmul_rn(r.w, h.w);
            *(float4 *)pz = z;
            *(float4 *)pr = r;
            *(float4 *)prh = rh;
        } else {
            const float az = paz[0], ar = par[0], cz = pcz[0], cr = pcr[0], h = ph[0];
            const float r = dkt_sigmoid(__fadd_rn(ar, cr));
            pz[0] = dkt_sigmoid(__fadd_rn(az, cz));
            pr[0] = r;
            prh[0] = __fmul_rn(r, h);
        }
    }
}

extern "C" int dkt_gru_gate_zr_train(const float *azr, const float *cz, long cz_bstride,
                                     const float *cr, long cr_bstride, const float *h, long h_bstride,
                                     float *z, float *r, float *rh, long rh_bstride,
                                     int B, int Ch, long HW, int device, void *stream) {
    if (!azr || !cz || !cr || !h || !z || !r || !rh) return DKT_E_NULL;
    if (B <= 0 || Ch <= 0 || HW <= 0) return DKT_E_SHAPE;
    DKT_ENTER(device);
    GateZrTrainArgs a;
    a.azr = azr; a.cz = cz; a.cr = cr; a.h = h; a.z = z; a.r = r; a.rh = rh;
    a.cz_bs = cz_bstride; a.cr_bs = cr_bstride; a.h_bs = h_bstride; a.rh_bs = rh_bstride;
    a.CHW = (long)Ch * HW;
    const bool vec = (a.CHW % 4 == 0) && (cz_bstride % 4 == 0) && (cr_bstride % 4 == 0) &&
                     (h_bstride % 4 == 0) && (rh_bstride % 4 == 0) && dkt_aligned16(azr) && dkt_aligned16(cz) &&
                     dkt_aligned16(cr) && dkt_aligned16(h) && dkt_aligned16(z) && dkt_aligned16(r) && dkt_aligned16(rh);
    hipStream_t st = (hipStream_t)stream;
    if (vec) {
        a.total = (long)B * a.CHW / 4;
        hipLaunchKernelGGL(gru_gate_zr_train_kernel<4>, dim3(dkt_gate_blocks(a.total)), dim3(256), 0, st, a);
    } else {
        a.total = (long)B * a.CHW;
        hipLaunchKernelGGL(gru_gate_zr_train_kernel<1>, dim3(dkt_gate_blocks(a.total)), dim3(256), 0, st, a);
    }
    return dkt_launch_status();
}

struct GateOutTrainArgs {
    const float *aq, *cq, *z, *h;
    float *q, *hout;
    long cq_bs, h_bs, hout_bs;
    long CHW;
    long total;
};

template <int V>
__global__ __launch_bounds__(256) void gru_gate_out_train_kernel(GateOutTrainArgs a) {
    const long per_b = a.CHW / V;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < a.total; i += (long)gridDim.x * 256L) {
        const long b = i / per_b;
        const long e = (i - b * per_b) * V;
        const float *paq = a.aq + b * a.CHW + e;
        const float *pcq = a.cq + b * a.cq_bs + e;
        const float *pz = a.z + b * a.CHW + e;
        const float *ph = a.h + b * a.h_bs + e;
        float *pq = a.q + b * a.CHW + e;
        float *po = a.hout + b * a.hout_bs + e;
        if (V == 4) {
            float4 aq = *(const float4 *)paq, cq = *(const float4 *)pcq;
            float4 z = *(const float4 *)pz, h = *(const float4 *)ph;
            float4 q, o;
            q.x = dkt_gru_q(aq.x, cq.x); q.y = dkt_gru_q(aq.y, cq.y);
            q.z = dkt_gru_q(aq.z, cq.z); q.w = dkt_gru_q(aq.w, cq.w);
            o.x = dkt_gru_blend(z.x, h.x, q.x); o.y = dkt_gru_blend(z.y, h.y, q.y);
            o.z = dkt_gru_blend(z.z, h.z, q.z); o.w = dkt_gru_blend(z.w, h.w, q.w);
            *(float4 *)pq = q;
            *(float4 *)po = o;
        } else {
            const float aq = paq[0], cq = pcq[0], z = pz[0], h = ph[0];
            const float q = dkt_gru_q(aq, cq);
            pq[0] = q;
            po[0] = dkt_gru_blend(z, h, q);
        }
    }
}

extern "C" int dkt_gru_gate_out_train(const float *aq, const float *cq, long cq_bstride,
                                      const float *z, const float *h, long h_bstride,
                                      float *q, float *hout, long hout_bstride,
                                      int B, int Ch, long HW, int device, void *stream) {
    if (!aq || !cq || !z || !h || !q || !hout) return DKT_E_NULL;
    if (B <= 0 || Ch <= 0 || HW <= 0) return DKT_E_SHAPE;
    DKT_ENTER(device);
    GateOutTrainArgs a;
    a.aq = aq; a.cq = cq; a.z = z; a.h = h; a.q = q; a.hout = hout;
    a.cq_bs = cq_bstride; a.h_bs = h_bstride; a.hout_bs = hout_bstride;
    a.CHW = (long)Ch * HW;
    const bool vec = (a.CHW % 4 == 0) && (cq_bstride % 4 == 0) && (h_bstride % 4 == 0) &&
                     (hout_bstride % 4 == 0) && dkt_aligned16(aq) && dkt_aligned16(cq) && dkt_aligned16(z) &&
                     dkt_aligned16(h) && dkt_aligned16(q) && dkt_aligned16(hout);
    hipStream_t st = (hipStream_t)stream;
    if (vec) {
        a.total = (long)B * a.CHW / 4;
        hipLaunchKernelGGL(gru_gate_out_train_kernel<4>, dim3(dkt_gate_blocks(a.total)), dim3(256), 0, st, a);
    } else {
        a.total = (long)B * a.CHW;
        hipLaunchKernelGGL(gru_gate_out_train_kernel<1>, dim3(dkt_gate_blocks(a.total)), dim3(256), 0, st, a);
    }
    return dkt_launch_status();
}

// ---- backward of the gates -------------------------------------------------------------------------------------------
// h' = (1 - z) h + z q,  q = tanh(aq + cq):
//   gaq = (g z) (1 - q q)     gz = g (q - h)     gh = g (1 - z)
// Where q is +-1 or z is 0 the affected gradient is an exact 0 (a product with an exact 0 factor).
__device__ __forceinline__ float gate_out_gaq(float g, float z, float q) {
    return __fmul_rn(__fmul_rn(g, z), __fsub_rn(1.0f, __fmul_rn(q, q)));
}
__device__ __forceinline__ float gate_out_gz(float g, float q, float h) { return __fmul_rn(g, __fsub_rn(q, h)); }
__device__ __forceinline__ float gate_out_gh(float g, float z) { return __fmul_rn(g, __fsub_rn(1.0f, z)); }

struct GateOutBwdArgs {
    const float *g, *z, *q, *h;
    float *gaq, *gz, *gh;      // each may be null
    long g_bs, h_bs;
    long CHW;
    long total;
};

template <int V>
__global__ __launch_bounds__(256) void gru_gate_out_bwd_kernel(GateOutBwdArgs a) {
    const long per_b = a.CHW / V;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < a.total; i += (long)gridDim.x * 256L) {
        const long b = i / per_b;
        const long e = (i - b * per_b) * V;
        const long d = b * a.CHW + e;                    // the dense tensors
        const float *pg = a.g + b * a.g_bs + e;
        const float *ph = a.h + b * a.h_bs + e;
        if (V == 4) {
            const float4 g = *(const float4 *)pg, z = *(const float4 *)(a.z + d);
            const float4 q = *(const float4 *)(a.q + d), h = *(const float4 *)ph;
            if (a.gaq)
                *(float4 *)(a.gaq + d) = make_float4(gate_out_gaq(g.x, z.x, q.x), gate_out_gaq(g.y, z.y, q.y),
                                                     gate_out_gaq(g.z, z.z, q.z), gate_out_gaq(g.w, z.w, q.w));
            if (a.gz)
                *(float4 *)(a.gz + d) = make_float4(gate_out_gz(g.x, q.x, h.x), gate_out_gz(g.y, q.y, h.y),
                                                    gate_out_gz(g.z, q.z, h.z), gate_out_gz(g.w, q.w, h.w));
            if (a.gh)
                *(float4 *)(a.gh + d) = make_float4(gate_out_gh(g.x, z.x), gate_out_gh(g.y, z.y),
                                                    gate_out_gh(g.z, z.z), gate_out_gh(g.w, z.w));
        } else {
            const float g = pg[0], z = a.z[d], q = a.q[d], h = ph[0];
            if (a.gaq) a.gaq[d] = gate_out_gaq(g, z, q);
            if (a.gz) a.gz[d] = gate_out_gz(g, q, h);
            if (a.gh) a.gh[d] = gate_out_gh(g, z);
        }
    }
}

extern "C" int dkt_gru_gate_out_bwd(const float *gout, long gout_bstride, const float *z, const float *q,
                                    const float *h, long h_bstride, float *gaq, float *gz, float *gh,
                                    int B, int Ch, long HW, int device, void *stream) {
    if (!gout || !z || !q || !h || (!gaq && !gz && !gh)) return DKT_E_NULL;
    if (B <= 0 || Ch <= 0 || HW <= 0) return DKT_E_SHAPE;
    DKT_ENTER(device);
    GateOutBwdArgs a;
    a.g = gout; a.z = z; a.q = q; a.h = h; a.gaq = gaq; a.gz = gz; a.gh = gh;
    a.g_bs = gout_bstride; a.h_bs = h_bstride;
    a.CHW = (long)Ch * HW;
    const bool vec = (a.CHW % 4 == 0) && (gout_bstride % 4 == 0) && (h_bstride % 4 == 0) && dkt_aligned16(gout) &&
                     dkt_aligned16(z) && dkt_aligned16(q) && dkt_aligned16(h) && dkt_aligned16(gaq) && dkt_aligned16(gz) &&
                     dkt_aligned16(gh);
    hipStream_t st = (hipStream_t)stream;
    if (vec) {
        a.total = (long)B * a.CHW / 4;
        hipLaunchKernelGGL(gru_gate_out_bwd_kernel<4>, dim3(dkt_gate_blocks(a.total)), dim3(256), 0, st, a);
    } else {
        a.total = (long)B * a.CHW;
        hipLaunchKernelGGL(gru_gate_out_bwd_kernel<1>, dim3(dkt_gate_blocks(a.total)), dim3(256), 0, st, a);
    }
    return dkt_launch_status();
}

// z = sigmoid(az + cz), r = sigmoid(ar + cr), rh = r h:
//   gaz = (gz z) (1 - z)     gar = ((grh h) r) (1 - r)     gh = grh r
// gaz | gar are the two halves of one (B, 2Ch, HW) tensor, the layout of the merged pre-activation.
__device__ __forceinline__ float gate_zr_gaz(float gz, float z) { return __fmul_rn(__fmul_rn(gz, z), __fsub_rn(1.0f, z)); }
__device__ __forceinline__ float gate_zr_gar(float grh, float h, float r) {
    return __fmul_rn(__fmul_rn(__fmul_rn(grh, h), r), __fsub_rn(1.0f, r));
}

struct GateZrBwdArgs {
    const float *gz, *grh, *z, *r, *h;
    float *gazr, *gh;          // each may be null
    long grh_bs, h_bs;
    long CHW;
    long total;
};

template <int V>
__global__ __launch_bounds__(256) void gru_gate_zr_bwd_kernel(GateZrBwdArgs a) {
    const long per_b = a.CHW / V;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < a.total; i += (long)gridDim.x * 256L) {
        const long b = i / per_b;
        const long e = (i - b * per_b) * V;
        const long d = b * a.CHW + e;                    // the dense (B, Ch, HW) tensors
        const float *pgrh = a.grh + b * a.grh_bs + e;
        const float *ph = a.h + b * a.h_bs + e;
        float *pgaz = a.gazr ? a.gazr + b * 2 * a.CHW + e : nullptr;
        if (V == 4) {
            const float4 gz = *(const float4 *)(a.gz + d), grh = *(const float4 *)pgrh;
            const float4 z = *(const float4 *)(a.z + d), r = *(const float4 *)(a.r + d), h = *(const float4 *)ph;
            if (pgaz) {
                *(float4 *)pgaz = make_float4(gate_zr_gaz(gz.x, z.x), gate_zr_gaz(gz.y, z.y),
                                              gate_zr_gaz(gz.z, z.z), gate_zr_gaz(gz.w, z.w));
                *(float4 *)(pgaz + a.CHW) = make_float4(gate_zr_gar(grh.x, h.x, r.x), gate_zr_gar(grh.y, h.y, r.y),
                                                        gate_zr_gar(grh.z, h.z, r.z), gate_zr_gar(grh.w, h.w, r.w));
            }
            if (a.gh)
                *(float4 *)(a.gh + d) = make_float4(__fmul_rn(grh.x, r.x), __fmul_rn(grh.y, r.y),
                                                    __fmul_rn(grh.z, r.z), __fmul_rn(grh.w, r.w));
        } else {
            const float gz = a.gz[d], grh = pgrh[0], z = a.z[d], r = a.r[d], h = ph[0];
            if (pgaz) {
                pgaz[0] = gate_zr_gaz(gz, z);
                pgaz[a.CHW] = gate_zr_gar(grh, h, r);
            }
            if (a.gh) a.gh[d] = __fmul_rn(grh, r);
        }
    }
}

extern "C" int dkt_gru_gate_zr_bwd(const float *gz, const float *grh, long grh_bstride, const float *z, const float *r,
                                   const float *h, long h_bstride, float *gazr, float *gh,
                                   int B, int Ch, long HW, int device, void *stream) {
    if (!gz || !grh || !z || !r || !h || (!gazr && !gh)) return DKT_E_NULL;
    if (B <= 0 || Ch <= 0 || HW <= 0) return DKT_E_SHAPE;
    DKT_ENTER(device);
    GateZrBwdArgs a;
    a.gz = gz; a.grh = grh; a.z = z; a.r = r; a.h = h; a.gazr = gazr; a.gh = gh;
    a.grh_bs = grh_bstride; a.h_bs = h_bstride;
    a.CHW = (long)Ch * HW;
    const bool vec = (a.CHW % 4 == 0) && (grh_bstride % 4 == 0) && (h_bstride % 4 == 0) && dkt_aligned16(gz) &&
                     dkt_aligned16(grh) && dkt_aligned16(z) && dkt_aligned16(r) && dkt_aligned16(h) &&
                     dkt_aligned16(gazr) && dkt_aligned16(gh);
    hipStream_t st = (hipStream_t)stream;
    if (vec) {
        a.total = (long)B * a.CHW / 4;
        hipLaunchKernelGGL(gru_gate_zr_bwd_kernel<4>, dim3(dkt_gate_blocks(a.total)), dim3(256), 0, st, a);
    } else {
        a.total = (long)B * a.CHW;
        hipLaunchKernelGGL(gru_gate_zr_bwd_kernel<1>, dim3(dkt_gate_blocks(a.total)), dim3(256), 0, st, a);
    }
    return dkt_launch_status();
}

// ---- backward of the resamplers --------------------------------------------------------------------------------------
// Both kernels: thread = one input element (pool2x: or four adjacent ones) of a plane, blockIdx.x over the plane,
// blockIdx.y strides over the planes.

// avg_pool2d(x, 3, stride=2, padding=1): output oy covers input rows 2 oy - 1 .. 2 oy + 1, so input row iy belongs to
// oy = iy / 2 when iy is even, and to (iy - 1) / 2 and (iy + 1) / 2 (when that is below Ho) when it is odd.
// gx = sum of fl(gy / 9) over the (at most 4) windows, ascending (oy, ox).
__device__ __forceinline__ float pool_sum(float d00, float d01, float d10, float d11, bool x2, bool y2) {
    float s = d00;
    if (x2) s = __fadd_rn(s, d01);
    if (y2) s = __fadd_rn(s, d10);
    if (y2 && x2) s = __fadd_rn(s, d11);
    return s;
}

// V == 4 (W % 4 == 0, gx 16-byte aligned): a thread owns input columns 4k .. 4k + 3, which belong to the output columns
// 2k, 2k + 1 and (when it exists) 2k + 2: six loads and six divisions for four elements, one 16-byte store.
template <int V>
__global__ __launch_bounds__(256) void pool2x_bwd_kernel(const float *__restrict__ gy, float *__restrict__ gx, long planes,
                                                         int H, int W, int Ho, int Wo) {
    const int Wv = W / V, n = H * Wv;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int iy = p / Wv, ix = (p - iy * Wv) * V;
    const int oy0 = iy >> 1, oy1 = (iy + 1) >> 1;
    const bool y2 = oy1 != oy0 && oy1 < Ho;
    const long r0 = (long)oy0 * Wo, r1 = (long)(y2 ? oy1 : oy0) * Wo;   // clamped: the loads are unconditional, the sum selects
    const int ox0 = ix >> 1;
    for (long pl = blockIdx.y; pl < planes; pl += gridDim.y) {
        const float *g = gy + pl * (long)Ho * Wo;
        float *o = gx + pl * (long)H * W + (long)iy * W + ix;
        if (V == 4) {
            const bool last = ox0 + 2 < Wo;                  // the column right of the quad's second window
            const int c2 = last ? ox0 + 2 : ox0 + 1;
            const float a0 = g[r0 + ox0], a1 = g[r0 + ox0 + 1], a2 = g[r0 + c2];
            const float b0 = g[r1 + ox0], b1 = g[r1 + ox0 + 1], b2 = g[r1 + c2];
            const float d00 = __fdiv_rn(a0, 9.0f), d01 = __fdiv_rn(a1, 9.0f), d02 = __fdiv_rn(a2, 9.0f);
            const float d10 = __fdiv_rn(b0, 9.0f), d11 = __fdiv_rn(b1, 9.0f), d12 = __fdiv_rn(b2, 9.0f);
            *(float4 *)o = make_float4(pool_sum(d00, 0.0f, d10, 0.0f, false, y2), pool_sum(d00, d01, d10, d11, true, y2),
                                       pool_sum(d01, 0.0f, d11, 0.0f, false, y2), pool_sum(d01, d02, d11, d12, last, y2));
        } else {
            const int ox1 = (ix + 1) >> 1;
            const bool x2 = ox1 != ox0 && ox1 < Wo;
            const int c1 = x2 ? ox1 : ox0;
            const float a0 = g[r0 + ox0], a1 = g[r0 + c1], b0 = g[r1 + ox0], b1 = g[r1 + c1];
            o[0] = pool_sum(__fdiv_rn(a0, 9.0f), __fdiv_rn(a1, 9.0f), __fdiv_rn(b0, 9.0f), __fdiv_rn(b1, 9.0f), x2, y2);
        }
    }
}

extern "C" int dkt_pool2x_bwd(const float *gy, float *gx, long planes, int H, int W, int device, void *stream) {
    if (!gy || !gx) return DKT_E_NULL;
    if (planes <= 0 || H <= 0 || W <= 0) return DKT_E_SHAPE;
    if ((long)H * W > 0x7fffffffL - 256) return DKT_E_UNSUPPORTED;      // (element indices of a plane are int)
    DKT_ENTER(device);
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const unsigned by = (unsigned)(planes < 65535 ? planes : 65535);
    hipStream_t st = (hipStream_t)stream;
    if (W % 4 == 0 && dkt_aligned16(gx))
        hipLaunchKernelGGL(pool2x_bwd_kernel<4>, dim3((unsigned)(((long)H * (W / 4) + 255) / 256), by), dim3(256), 0, st,
                           gy, gx, planes, H, W, Ho, Wo);
    else
        hipLaunchKernelGGL(pool2x_bwd_kernel<1>, dim3((unsigned)(((long)H * W + 255) / 256), by), dim3(256), 0, st,
                           gy, gx, planes, H, W, Ho, Wo);
    return dkt_launch_status();
}

// The forward (interp_kernel, norm.hip) gives output row oy the source rows and weights
//   fy = fl(sy oy),  y0 = (int)fy,  y1 = y0 + (y0 < H - 1),  ly1 = fl(fy - y0),  ly0 = fl(1 - ly1),
// so input row iy receives ly1 from every oy with y0 == iy - 1 (then y1 == iy), ly0 from every oy with y0 == iy, and from
// those also ly1 when iy == H - 1 (y1 == y0 there); columns alike.  fl(sy oy) does not decrease with oy, so the
// contributors of a row are one run [a, b] of outputs.  The run is found with the forward's own expression -- the map is
// never inverted in real arithmetic: a range around (iy -+ 1) / sy widened by one each side holds every contributor (the
// quotient and fl(sy oy) are each off by less than half a row for oy < 2^22), and its ends move inwards until y0 fits.
struct InterpRun {
    int a, b;                  // contributing outputs (inclusive); a > b: none
};

__device__ __forceinline__ int interp_src(int o, float s) { return (int)__fmul_rn(s, (float)o); }

__device__ __forceinline__ InterpRun interp_run(int i, float s, int No) {
    InterpRun r;
    r.a = 0, r.b = No - 1;
    if (s != 0.0f) {                                        // (s == 0: No == 1 or one input row; every output is a candidate)
        const float top = (float)(No - 1);
        r.a = (int)fminf(fmaxf(floorf(__fdiv_rn((float)(i - 1), s)) - 1.0f, 0.0f), top);
        r.b = (int)fminf(fmaxf(ceilf(__fdiv_rn((float)(i + 1), s)) + 1.0f, 0.0f), top);
    }
    while (r.a <= r.b && interp_src(r.a, s) < i - 1) ++r.a;
    while (r.b >= r.a && interp_src(r.b, s) > i) --r.b;
    return r;
}

// the weights output o of a run gives input i: w through the tap that points at i, and w2 (when `two`) through the
// upper tap as well (i == N - 1 and both taps there)
__device__ __forceinline__ void interp_weights(int o, int i, float s, int N, float &w, float &w2, bool &two) {
    const float f = __fmul_rn(s, (float)o);
    const int i0 = (int)f;
    const float l1 = __fsub_rn(f, (float)i0);
    const bool lower = i0 == i;                             // else i0 == i - 1: the upper tap
    w = lower ? __fsub_rn(1.0f, l1) : l1;
    w2 = l1;
    two = lower && i == N - 1;
}

// gx[iy, ix] = sum over (oy, y tap, ox, x tap), ascending, of fl(fl(wy wx) gy[oy, ox])
__global__ __launch_bounds__(256) void interp_bwd_kernel(const float *__restrict__ gy, float *__restrict__ gx, long planes,
                                                         int H, int W, int Ho, int Wo, float sy, float sx) {
    const int HW = H * W;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int iy = p / W, ix = p - iy * W;
    const InterpRun ry = interp_run(iy, sy, Ho), rx = interp_run(ix, sx, Wo);
    for (long pl = blockIdx.y; pl < planes; pl += gridDim.y) {
        const float *g = gy + pl * (long)Ho * Wo;
        float s = 0.0f;
        for (int oy = ry.a; oy <= ry.b; ++oy) {
            float wy, wy2;
            bool ytwo;
            interp_weights(oy, iy, sy, H, wy, wy2, ytwo);
            const float *row = g + (long)oy * Wo;
            for (int ty = 0; ty < (ytwo ? 2 : 1); ++ty) {
                const float wyt = ty ? wy2 : wy;
                for (int ox = rx.a; ox <= rx.b; ++ox) {
                    float wx, wx2;
                    bool xtwo;
                    interp_weights(ox, ix, sx, W, wx, wx2, xtwo);
                    const float v = row[ox];
                    s = __fadd_rn(s, __fmul_rn(__fmul_rn(wyt, wx), v));
                    if (xtwo) s = __fadd_rn(s, __fmul_rn(__fmul_rn(wyt, wx2), v));
                }
            }
        }
        gx[pl * (long)HW + p] = s;
    }
}

extern "C" int dkt_interp_bilinear_bwd(const float *gy, float *gx, long planes, int H, int W, int Ho, int Wo,
                                       int device, void *stream) {
    if (!gy || !gx) return DKT_E_NULL;
    if (planes <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return DKT_E_SHAPE;
    // element indices of a plane are int; the candidate ranges hold every contributor for up to 2^22 outputs per axis
    if ((long)H * W > 0x7fffffffL - 256 || (long)Ho * Wo > 0x7fffffffL || Ho > (1 << 22) || Wo > (1 << 22))
        return DKT_E_UNSUPPORTED;
    DKT_ENTER(device);
    const float sy = Ho > 1 ? (float)(H - 1) / (float)(Ho - 1) : 0.0f;       // as dkt_interp_bilinear
    const float sx = Wo > 1 ? (float)(W - 1) / (float)(Wo - 1) : 0.0f;
    const long by = planes < 65535 ? planes : 65535;
    hipLaunchKernelGGL(interp_bwd_kernel, dim3((unsigned)(((long)H * W + 255) / 256), (unsigned)by), dim3(256), 0,
                       (hipStream_t)stream, gy, gx, planes, H, W, Ho, Wo, sy, sx);
    return dkt_launch_status();
}
