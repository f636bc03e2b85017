// dkt_ns_loss / dkt_ns_loss_bwd: the NeRF-supervised loss of meta_arch/nerf_stereo/loss.py:128-181 -- the confidence-weighted
// disparity term plus the trinocular photometric term (disp_warp :73-84, photometric_loss :86-90 with SSIM :5-27,
// trinocular_loss :92-109) -- for n predictions against one target.
//
// Forward, three launches:
//   1 (once per call)  ns_pre_kernel: loss_2 = min(p(centre, first), p(centre, third)) from the images alone into the workspace,
//                      and the valid plane.
//   2 (grid z = prediction)  ns_fwd_kernel: block = a 16 x 16 tile of one image.  Both outer views are warped with the mask
//                      applied into LDS on the tile plus a 3-pixel halo (reflection resolved at the image border: a halo
//                      position outside the image is the warp AT the pixel it reflects to, as ReflectionPad2d pads the
//                      reconstruction); every pixel forms its 7 x 7 window sums from LDS, p12, p23, the minimum, the branch
//                      and the automask, kept as one byte per pixel.  Every sum is an fp64 block partial in a fixed shuffle order.
//   3 (one block)      ns_finalize_kernel: partials summed over the blocks in a fixed order; sum_i fl32(w_i) * mean_i in fp32 in
//                      order i, then the two alphas; the scalar loss and the record.
// Backward, one launch (grid z = prediction): the tile recomputes the warps on a 6-pixel halo, then for every window centre q
// on the 3-pixel halo whose automask byte is set the coefficients (a_q, b_q, c_q) per channel of the winning view, with
//   d SSIM_q / d x_p = (a_q + 2 b_q x_p + c_q y_p) / 49          (x the reconstruction, y the centre view, p in the window of q)
// and every pixel gathers them over its windows (more than once where reflection folds the border back onto it), adds the L1
// term and multiplies by d(mask * sample)/d px * s * W/(W-1).  No atomics; every gradient element is stored exactly once.
#include "dkt_common.h"
#include "wave_reduce.h"

#include <math.h>

#define NS_T 16
#define NS_THREADS (NS_T * NS_T)
#define NS_WAVES (NS_THREADS / 64)
#define NS_F (NS_T + 6)                  // tile + 3-pixel halo
#define NS_E (NS_T + 12)                 // tile + 6-pixel halo
#define NS_Q0 8                          // per-call quantities: valid count, EPE sum, <1 <3 <5 counts
#define NS_QP 4                          // per prediction: photometric sum, automask count, disparity sum, NaN/Inf flag
#define NS_Q (NS_Q0 + NS_QP * DKT_NS_MAX_PRED)
#define NS_FIN_THREADS 1024
#define NS_C1 1e-4f
#define NS_C2 9e-4f

static inline int ns_tiles(int n) { return (n + NS_T - 1) / NS_T; }

// ReflectionPad2d's source index (|offset| <= 3 < n), clamped so that positions never used still read inside the image
__device__ __forceinline__ int ns_refl(int i, int n) {
    i = i < 0 ? -i : i;
    i = i > n - 1 ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

// One axis of grid_sample(align_corners=False) at pixel coordinate ix: the two taps and weights of the border-padded
// image sample (cg: the gradient of the clip, 0 outside (0, n-1)), and the zero-padded sample of a plane of ones with its
// derivative (mk, dmk).
struct NsAxis {
    int i0, i1;
    float w0, w1, cg, mk, dmk;
};

__device__ __forceinline__ NsAxis ns_axis(float ix, int n) {
    NsAxis a;
    const float hi = (float)(n - 1);
    const float ic = fminf(fmaxf(ix, 0.0f), hi);
    a.cg = (ix > 0.0f && ix < hi) ? 1.0f : 0.0f;
    const float f0 = floorf(ic);
    a.i0 = (int)f0;
    a.i1 = min(a.i0 + 1, n - 1);            // (weight 0 when clamped: ic == n - 1 there)
    a.w1 = ic - f0;
    a.w0 = (f0 + 1.0f) - ic;
    const float u0 = floorf(ix), u1 = u0 + 1.0f;
    const bool in0 = u0 >= 0.0f && u0 <= hi, in1 = u1 >= 0.0f && u1 <= hi;
    a.mk = (in0 ? u1 - ix : 0.0f) + (in1 ? ix - u0 : 0.0f);
    a.dmk = (in1 ? 1.0f : 0.0f) - (in0 ? 1.0f : 0.0f);
    return a;
}

// norm_grid (:29-36) then grid_sample's unnormalize, in the reference's order of operations
__device__ __forceinline__ float ns_coord(float v, int n) {
    const float g = 2.0f * v / (float)(n - 1) - 1.0f;
    return ((g + 1.0f) * (float)n - 1.0f) / 2.0f;
}

struct NsView {
    float m, dm;            // mask and d mask / d px
    float S[3], dS[3];      // border-padded sample and d sample / d px, per channel
};

__device__ __forceinline__ NsView ns_view(const float *__restrict__ im, long HW, int W, int x, float disp, float s, const NsAxis &ay) {
    const NsAxis ax = ns_axis(ns_coord((float)x + s * disp, W), W);
    const float nw = ax.w0 * ay.w0, ne = ax.w1 * ay.w0, sw = ax.w0 * ay.w1, se = ax.w1 * ay.w1;
    NsView v;
    v.m = ax.mk * ay.mk;
    v.dm = ax.dmk * ay.mk;
    const long r0 = (long)ay.i0 * W, r1 = (long)ay.i1 * W;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float *p = im + c * HW;
        const float i00 = p[r0 + ax.i0], i01 = p[r0 + ax.i1], i10 = p[r1 + ax.i0], i11 = p[r1 + ax.i1];
        v.S[c] = i00 * nw + i01 * ne + i10 * sw + i11 * se;
        v.dS[c] = ax.cg * ((i01 - i00) * ay.w0 + (i11 - i10) * ay.w1);
    }
    return v;
}

// Fills an RS x RS region whose origin is (ty0 - HL, tx0 - HL) in padded coordinates: sR = [view][channel] planes of the
// masked reconstructions (PRE: of the outer views as they are), sA = [channel] planes of the centre view.
template <int RS, int HL, bool PRE>
__device__ __forceinline__ void ns_fill(const dkt_ns_loss_desc &d, const float *__restrict__ pred, int b, int ty0, int tx0,
                                        float *__restrict__ sR, float *__restrict__ sA) {
    const int H = d.H, W = d.W;
    const long HW = (long)H * W;
    const float *im0 = d.im[0] + (long)b * d.im_bstride[0];
    const float *im1 = d.im[1] + (long)b * d.im_bstride[1];
    const float *im2 = d.im[2] + (long)b * d.im_bstride[2];
    for (int i = threadIdx.x; i < RS * RS; i += NS_THREADS) {
        const int ry = i / RS, rx = i - ry * RS;
        const int y = ns_refl(ty0 - HL + ry, H), x = ns_refl(tx0 - HL + rx, W);
        const long r = (long)y * W + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) sA[c * RS * RS + i] = im1[c * HW + r];
        if (PRE) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                sR[c * RS * RS + i] = im0[c * HW + r];
                sR[(3 + c) * RS * RS + i] = im2[c * HW + r];
            }
        } else {
            const float disp = pred[r];
            const NsAxis ay = ns_axis(ns_coord((float)y, H), H);
            const NsView v0 = ns_view(im0, HW, W, x, disp, 1.0f, ay);
            const NsView v1 = ns_view(im2, HW, W, x, disp, -1.0f, ay);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                sR[c * RS * RS + i] = v0.m * v0.S[c];
                sR[(3 + c) * RS * RS + i] = v1.m * v1.S[c];
            }
        }
    }
}

// SSIM's window statistics (:13-21) of the 7 x 7 window whose top-left element X and Y point at
struct NsStat {
    float mx, my, sx, sy, sxy;
};

__device__ __forceinline__ NsStat ns_stat(const float *__restrict__ X, const float *__restrict__ Y, int pitch) {
    float a = 0.0f, b = 0.0f, xx = 0.0f, yy = 0.0f, xy = 0.0f;
    for (int dy = 0; dy < 7; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 7; ++dx) {
            const float x = X[dy * pitch + dx], y = Y[dy * pitch + dx];
            a += x;
            b += y;
            xx += x * x;
            yy += y * y;
            xy += x * y;
        }
    }
    NsStat s;
    s.mx = a / 49.0f;
    s.my = b / 49.0f;
    s.sx = xx / 49.0f - s.mx * s.mx;
    s.sy = yy / 49.0f - s.my * s.my;
    s.sxy = xy / 49.0f - s.mx * s.my;
    return s;
}

// SSIM's parts (:23-25)
struct NsSsim {
    float A1, A2, B1, B2, S, raw;       // raw = (1 - SSIM) / 2 before the clamp
};

__device__ __forceinline__ NsSsim ns_ssim(const NsStat &s) {
    NsSsim q;
    q.A1 = 2.0f * (s.mx * s.my) + NS_C1;
    q.A2 = 2.0f * s.sxy + NS_C2;
    q.B1 = s.mx * s.mx + s.my * s.my + NS_C1;
    q.B2 = s.sx + s.sy + NS_C2;
    q.S = (q.A1 * q.A2) / (q.B1 * q.B2);
    q.raw = (1.0f - q.S) / 2.0f;
    return q;
}

// photometric_loss (:86-90) of one view at the window with top-left offset o of the region's planes
__device__ __forceinline__ float ns_photo(const float *__restrict__ R, const float *__restrict__ A, int plane, int pitch, int o) {
    float l1 = 0.0f, ds = 0.0f;
    for (int c = 0; c < 3; ++c) {
        const float *X = R + c * plane + o, *Y = A + c * plane + o;
        const NsSsim q = ns_ssim(ns_stat(X, Y, pitch));
        l1 += fabsf(Y[3 * pitch + 3] - X[3 * pitch + 3]);
        ds += fminf(fmaxf(q.raw, 0.0f), 1.0f);
    }
    return 0.15f * (l1 / 3.0f) + 0.85f * (ds / 3.0f);
}

// the folded confidence, the photometric weight, the target and the valid bit of pixel r of image b (:132-142)
struct NsPixel {
    float conf, unc, t;
    bool valid;
};

__device__ __forceinline__ NsPixel ns_pixel(const dkt_ns_loss_desc &d, int b, long r) {
    NsPixel p;
    const float c = d.conf[(long)b * d.conf_bstride + r];
    if (d.target) {
        p.t = d.target[(long)b * d.target_bstride + r];
        p.conf = c * (p.t < 0.0f ? 1.0f : 0.0f);
        p.unc = 1.0f - p.conf;
        p.valid = p.conf > d.conf_threshold && sqrtf(p.t * p.t) < d.max_flow;
    } else {
        p.t = 0.0f;
        p.conf = p.unc = c;
        p.valid = d.valid_in[(long)b * d.H * d.W + r] != 0;
    }
    return p;
}

__global__ __launch_bounds__(NS_THREADS) void ns_pre_kernel(dkt_ns_loss_desc d, float *__restrict__ loss2) {
    __shared__ float sR[6 * NS_F * NS_F];
    __shared__ float sA[3 * NS_F * NS_F];
    const int tid = threadIdx.x, b = blockIdx.z;
    const int ty0 = blockIdx.y * NS_T, tx0 = blockIdx.x * NS_T;
    const int ly = tid / NS_T, lx = tid % NS_T, y = ty0 + ly, x = tx0 + lx;
    const bool in = y < d.H && x < d.W;
    const long r = (long)y * d.W + x, HW = (long)d.H * d.W;
    if (d.alpha_photo != 0.0f) {
        ns_fill<NS_F, 3, true>(d, nullptr, b, ty0, tx0, sR, sA);
        __syncthreads();
        if (in) {
            const int o = ly * NS_F + lx;
            const float p1 = ns_photo(sR, sA, NS_F * NS_F, NS_F, o);
            const float p3 = ns_photo(sR + 3 * NS_F * NS_F, sA, NS_F * NS_F, NS_F, o);
            loss2[(long)b * HW + r] = p3 < p1 ? p3 : p1;
        }
    }
    if (in && d.target) d.valid[(long)b * HW + r] = ns_pixel(d, b, r).valid ? 1 : 0;
}

__global__ __launch_bounds__(NS_THREADS) void ns_fwd_kernel(dkt_ns_loss_desc d, const float *__restrict__ loss2, double *__restrict__ ws) {
    __shared__ float sR[6 * NS_F * NS_F];
    __shared__ float sA[3 * NS_F * NS_F];
    __shared__ double part[NS_WAVES][NS_QP + 5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.z % d.n, b = blockIdx.z / d.n;
    const int ty0 = blockIdx.y * NS_T, tx0 = blockIdx.x * NS_T;
    const int ly = tid / NS_T, lx = tid % NS_T, y = ty0 + ly, x = tx0 + lx;
    const bool in = y < d.H && x < d.W;
    const long r = (long)y * d.W + x, HW = (long)d.H * d.W;
    const long nblk = (long)gridDim.x * gridDim.y * d.B, blk = ((long)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const float *pred = d.pred[i] + (long)b * d.pred_bstride[i];
    const bool photo = d.alpha_photo != 0.0f, last = i == d.n - 1;
    if (photo) ns_fill<NS_F, 3, false>(d, pred, b, ty0, tx0, sR, sA);
    __syncthreads();
    double q[NS_QP + 5];
#pragma unroll
    for (int k = 0; k < NS_QP + 5; ++k) q[k] = 0.0;
    if (in) {
        const NsPixel px = ns_pixel(d, b, r);
        const float p = pred[r];
        if (isnan(p) || isinf(p)) q[3] = 1.0;
        if (photo) {
            const int o = ly * NS_F + lx;
            const float p12 = ns_photo(sR, sA, NS_F * NS_F, NS_F, o);
            const float p23 = ns_photo(sR + 3 * NS_F * NS_F, sA, NS_F * NS_F, NS_F, o);
            const bool third = p23 < p12;
            const float lw = third ? p23 : p12, l2 = loss2[(long)b * HW + r];
            const bool am = lw < l2 && px.valid;
            d.state[((long)i * d.B + b) * HW + r] = (unsigned char)((am ? 1 : 0) | (third ? 2 : 0));
            if (am) {
                q[0] = (double)(lw * px.unc);
                q[1] = 1.0;
            }
            if (d.planes && i == 0) {
                d.planes[(long)b * HW + r] = p12;
                d.planes[((long)d.B + b) * HW + r] = p23;
                d.planes[(2L * d.B + b) * HW + r] = l2;
            }
        }
        if (px.valid) {
            if (d.target) q[2] = (double)(fabsf(p - px.t) * px.conf);
            if (last) {
                // epe = sum((pred[-1] - target)**2, dim=1).sqrt() over valid, and the 1 / 3 / 5 px counts (:171-179)
                const float dd = p - px.t;
                const float ep = sqrtf(dd * dd);
                q[4] = 1.0;
                q[5] = (double)ep;
                q[6] = ep < 1.0f ? 1.0 : 0.0;
                q[7] = ep < 3.0f ? 1.0 : 0.0;
                q[8] = ep < 5.0f ? 1.0 : 0.0;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NS_QP + 5; ++k) {
        const double s = wave_sum(q[k]);
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    if (tid < NS_QP + 5) {
        double s = 0.0;
        for (int w = 0; w < NS_WAVES; ++w) s += part[w][tid];
        if (tid < NS_QP)
            ws[(NS_Q0 + NS_QP * i + tid) * nblk + blk] = s;
        else if (last)
            ws[(tid - NS_QP) * nblk + blk] = s;
    }
}

__global__ __launch_bounds__(NS_FIN_THREADS) void ns_finalize_kernel(dkt_ns_loss_desc d, const double *__restrict__ ws, int nblk) {
    __shared__ double tot[NS_Q];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = NS_Q0 + NS_QP * d.n;
    // one wave per quantity, summed over the blocks in wave_reduce.h's column order (rows 5 .. NS_Q0 - 1 are unused: 0)
    for (int k = wave; k < R; k += NS_FIN_THREADS / 64) {
        const double s = column_sum(ws + (long)k * nblk, k < 5 || k >= NS_Q0 ? nblk : 0);
        if (lane == 0) tot[k] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    const double N = tot[0];
    // disp_loss += i_weight * (...)[valid].mean(); photometric_loss += i_weight * loss.mean()  (fp32 scalars, in order i; the
    // mean of an empty set is NaN)
    float disp = 0.0f, photo = 0.0f;
    double bad = 0.0;
    for (int i = 0; i < d.n; ++i) {
        const double *t = tot + NS_Q0 + NS_QP * i;
        if (d.target) disp = disp + d.weight[i] * (float)(t[2] / N);
        if (d.alpha_photo != 0.0f) photo = photo + d.weight[i] * (float)(t[0] / t[1]);
        bad += t[3];
        d.rec[8 + i] = t[1];
    }
    *d.loss = d.target ? d.alpha_disp * disp + d.alpha_photo * photo : d.alpha_photo * photo;
    const float nf = (float)N;
    d.rec[0] = N;
    d.rec[1] = (double)(float)(tot[1] / N);
    d.rec[2] = (double)((float)tot[2] / nf);
    d.rec[3] = (double)((float)tot[3] / nf);
    d.rec[4] = (double)((float)tot[4] / nf);
    d.rec[5] = bad != 0.0 ? 1.0 : 0.0;
    d.rec[6] = (double)disp;
    d.rec[7] = (double)photo;
}

// the a-th padded position that reflects onto coordinate p of an axis of length n: p itself, -p (1 <= p <= 3),
// 2 (n - 1) - p (1 <= n - 1 - p <= 3); false when there is no such position
__device__ __forceinline__ bool ns_image(int a, int p, int n, int &pos) {
    if (a == 0) {
        pos = p;
        return true;
    }
    if (a == 1) {
        pos = -p;
        return p >= 1 && p <= 3;
    }
    pos = 2 * (n - 1) - p;
    return n - 1 - p >= 1 && n - 1 - p <= 3;
}

__global__ __launch_bounds__(NS_THREADS) void ns_bwd_kernel(dkt_ns_loss_desc d, dkt_ns_loss_grad gr) {
    __shared__ float sR[6 * NS_E * NS_E];
    __shared__ float sA[3 * NS_E * NS_E];
    __shared__ float sK[9 * NS_F * NS_F];           // [channel][a, b, c] of the winning view at q
    __shared__ unsigned char sB[NS_F * NS_F];       // 0: no gradient through q; 1 + view otherwise
    const int tid = threadIdx.x;
    const int i = blockIdx.z % d.n, b = blockIdx.z / d.n;
    const int H = d.H, W = d.W;
    const int ty0 = blockIdx.y * NS_T, tx0 = blockIdx.x * NS_T;
    const int ly = tid / NS_T, lx = tid % NS_T, y = ty0 + ly, x = tx0 + lx;
    const bool in = y < H && x < W;
    const long r = (long)y * W + x, HW = (long)H * W;
    const float *pred = d.pred[i] + (long)b * d.pred_bstride[i];
    const unsigned char *state = d.state + ((long)i * d.B + b) * HW;
    const float up = *gr.grad_loss;
    const bool photo = d.alpha_photo != 0.0f;
    // the chain of 1.7 * (alpha * sum_i w_i * mean_i): upstream * alpha, * fl32(w_i), / fl32(count)
    const float gs = photo ? ((up * d.alpha_photo) * d.weight[i]) / (float)d.rec[8 + i] : 0.0f;
    float g = 0.0f;
    if (photo) {
        ns_fill<NS_E, 6, false>(d, pred, b, ty0, tx0, sR, sA);
        __syncthreads();
        for (int j = tid; j < NS_F * NS_F; j += NS_THREADS) {
            const int ry = j / NS_F, rx = j - ry * NS_F;
            const int qy = ty0 - 3 + ry, qx = tx0 - 3 + rx;
            unsigned char bq = 0;
            if (qy >= 0 && qy < H && qx >= 0 && qx < W) {
                const long rq = (long)qy * W + qx;
                const unsigned char st = state[rq];
                if (st & 1) {
                    const int v = st >> 1;
                    bq = (unsigned char)(1 + v);
                    const float G = gs * ns_pixel(d, b, rq).unc;
                    const float k = -(((G * 0.85f) / 3.0f) / 2.0f) / 49.0f;
                    const int o = ry * NS_E + rx;
                    for (int c = 0; c < 3; ++c) {
                        const NsStat s = ns_stat(sR + (3 * v + c) * NS_E * NS_E + o, sA + c * NS_E * NS_E + o, NS_E);
                        const NsSsim m = ns_ssim(s);
                        const bool act = m.raw >= 0.0f && m.raw <= 1.0f;      // clamp's backward
                        const float kd = act ? k / (m.B1 * m.B2) : 0.0f;
                        sK[(3 * c + 0) * NS_F * NS_F + j] =
                            kd * (2.0f * s.my * m.A2 - 2.0f * m.A1 * s.my - 2.0f * m.S * s.mx * m.B2 + 2.0f * m.S * m.B1 * s.mx);
                        sK[(3 * c + 1) * NS_F * NS_F + j] = kd * (-m.S * m.B1);
                        sK[(3 * c + 2) * NS_F * NS_F + j] = kd * (2.0f * m.A1);
                    }
                }
            }
            sB[j] = bq;
        }
        __syncthreads();
        if (in) {
            float acc[2][9];
#pragma unroll
            for (int v = 0; v < 2; ++v)
#pragma unroll
                for (int k = 0; k < 9; ++k) acc[v][k] = 0.0f;
            for (int a = 0; a < 3; ++a) {
                int py, px;
                if (!ns_image(a, y, H, py)) continue;
                const int q0y = max(py - 3, 0), q1y = min(py + 3, H - 1);
                for (int e = 0; e < 3; ++e) {
                    if (!ns_image(e, x, W, px)) continue;
                    const int q0x = max(px - 3, 0), q1x = min(px + 3, W - 1);
                    for (int qy = q0y; qy <= q1y; ++qy) {
                        for (int qx = q0x; qx <= q1x; ++qx) {
                            const int j = (qy - ty0 + 3) * NS_F + (qx - tx0 + 3);
                            const unsigned char bq = sB[j];
                            if (!bq) continue;
                            const float w0 = bq == 1 ? 1.0f : 0.0f, w1 = 1.0f - w0;
#pragma unroll
                            for (int k = 0; k < 9; ++k) {
                                const float kv = sK[k * NS_F * NS_F + j];
                                acc[0][k] += w0 * kv;
                                acc[1][k] += w1 * kv;
                            }
                        }
                    }
                }
            }
            const unsigned char st = state[r];
            const float G = (st & 1) ? gs * ns_pixel(d, b, r).unc : 0.0f;
            const float l1 = (G * 0.15f) / 3.0f;
            const int e = (ly + 6) * NS_E + (lx + 6);
            const float disp = pred[r];
            const NsAxis ay = ns_axis(ns_coord((float)y, H), H);
            const float dpx = (2.0f / (float)(W - 1)) * (float)W / 2.0f;       // d px / d (x + s d)
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                const float s = v == 0 ? 1.0f : -1.0f;
                const NsView vw = ns_view(d.im[2 * v] + (long)b * d.im_bstride[2 * v], HW, W, x, disp, s, ay);
                const bool won = (st & 1) && (st >> 1) == v;
                float t = 0.0f;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float xp = sR[(3 * v + c) * NS_E * NS_E + e], yp = sA[c * NS_E * NS_E + e];
                    float gR = acc[v][3 * c] + 2.0f * acc[v][3 * c + 1] * xp + acc[v][3 * c + 2] * yp;
                    // |y - x| backward: -sgn(y - x), sgn(0) = 0
                    if (won) gR += l1 * (xp > yp ? 1.0f : (xp < yp ? -1.0f : 0.0f));
                    t += gR * (vw.m * vw.dS[c] + vw.S[c] * vw.dm);
                }
                g += t * (s * dpx);
            }
        }
    }
    if (!in) return;
    if (d.target) {
        const NsPixel px = ns_pixel(d, b, r);
        if (px.valid) {
            const float z = pred[r] - px.t;
            const float sg = z > 0.0f ? 1.0f : (z < 0.0f ? -1.0f : 0.0f);
            g += ((((up * d.alpha_disp) * d.weight[i]) / (float)d.rec[0]) * px.conf) * sg;
        }
    }
    gr.grad[i][(long)b * HW + r] = g;
}

static int ns_check(const dkt_ns_loss_desc *d) {
    if (!d) return DKT_E_NULL;
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->n < 1 || d->n > DKT_NS_MAX_PRED) return DKT_E_SHAPE;
    if (d->H < 4 || d->W < 4) return DKT_E_SHAPE;                    // ReflectionPad2d(3) needs more than 3
    const long HW = (long)d->H * d->W;
    if (HW > 0x7fffffffL - 256 || (long)d->B * d->n > 65535 || ns_tiles(d->H) > 65535) return DKT_E_UNSUPPORTED;
    for (int i = 0; i < d->n; ++i) {
        if (!d->pred[i]) return DKT_E_NULL;
        if (d->B > 1 && d->pred_bstride[i] < HW) return DKT_E_SHAPE;
        if ((uintptr_t)d->pred[i] % 4) return DKT_E_ALIGN;
    }
    for (int k = 0; k < 3; ++k) {
        if (!d->im[k]) return DKT_E_NULL;
        if (d->B > 1 && d->im_bstride[k] < 3 * HW) return DKT_E_SHAPE;
        if ((uintptr_t)d->im[k] % 4) return DKT_E_ALIGN;
    }
    if (!d->conf || !d->loss || !d->rec) return DKT_E_NULL;
    if (d->target ? !d->valid : !d->valid_in) return DKT_E_NULL;
    if (d->alpha_photo != 0.0f && !d->state) return DKT_E_NULL;
    if (d->B > 1 && (d->conf_bstride < HW || (d->target && d->target_bstride < HW))) return DKT_E_SHAPE;
    if ((uintptr_t)d->conf % 4 || (uintptr_t)d->target % 4 || (uintptr_t)d->loss % 4 || (uintptr_t)d->planes % 4 || (uintptr_t)d->rec % 8)
        return DKT_E_ALIGN;
    return DKT_OK;
}

static long ns_blocks(int B, int H, int W) { return (long)B * ns_tiles(H) * ns_tiles(W); }

extern "C" long dkt_ns_loss_workspace(int B, int H, int W) {
    if (B <= 0 || H < 4 || W < 4) return DKT_E_SHAPE;
    return 8L * NS_Q * ns_blocks(B, H, W) + ((4L * B * H * W + 7) & ~7L);        // the partials, the loss_2 plane
}

extern "C" int dkt_ns_loss(const dkt_ns_loss_desc *d, void *ws, int device, void *stream) {
    const int rc = ns_check(d);
    if (rc != DKT_OK) return rc;
    if (!ws) return DKT_E_NULL;
    if ((uintptr_t)ws % 8) return DKT_E_ALIGN;
    DKT_ENTER(device);
    const long nblk = ns_blocks(d->B, d->H, d->W);
    double *part = (double *)ws;
    float *loss2 = (float *)(part + NS_Q * nblk);
    const dim3 tiles(ns_tiles(d->W), ns_tiles(d->H), d->B);
    if (d->target || d->alpha_photo != 0.0f)
        hipLaunchKernelGGL(ns_pre_kernel, tiles, dim3(NS_THREADS), 0, (hipStream_t)stream, *d, loss2);
    hipLaunchKernelGGL(ns_fwd_kernel, dim3(tiles.x, tiles.y, d->B * d->n), dim3(NS_THREADS), 0, (hipStream_t)stream, *d,
                       (const float *)loss2, part);
    hipLaunchKernelGGL(ns_finalize_kernel, dim3(1), dim3(NS_FIN_THREADS), 0, (hipStream_t)stream, *d, (const double *)part, (int)nblk);
    return dkt_launch_status();
}

extern "C" int dkt_ns_loss_bwd(const dkt_ns_loss_desc *d, const dkt_ns_loss_grad *g, int device, void *stream) {
    const int rc = ns_check(d);
    if (rc != DKT_OK) return rc;
    if (!g || !g->grad_loss) return DKT_E_NULL;
    for (int i = 0; i < d->n; ++i) {
        if (!g->grad[i]) return DKT_E_NULL;
        if ((uintptr_t)g->grad[i] % 4) return DKT_E_ALIGN;
    }
    DKT_ENTER(device);
    hipLaunchKernelGGL(ns_bwd_kernel, dim3(ns_tiles(d->W), ns_tiles(d->H), d->B * d->n), dim3(NS_THREADS), 0, (hipStream_t)stream, *d, *g);
    return dkt_launch_status();
}
