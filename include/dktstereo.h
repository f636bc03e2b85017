/*
 * dktstereo.h -- C ABI of libdktstereo.so, the MI355X (gfx950) implementation of
 * DKT-Stereo's stereo-inference hot path.
 *
 * The reference (jiaw-z/DKT-Stereo) is pure Python/PyTorch and has no FFI layer
 * of its own; its seam for this path is Python duck typing.  The
 * entry points below are therefore what a binding for that seam needs: one call
 * per reference operator, plain device pointers and sizes, no torch types.  Each
 * declaration cites the reference code it replaces (file:line relative to the
 * reference tree).  dkt_stereo_amd/_ffi.py is the ctypes binding the reference's
 * classes are re-exposed through; INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into memory owned by the caller (torch
 *     tensors); the library never allocates, frees or retains caller memory;
 *   - all tensors are float32, NCHW-contiguous unless a stride argument says
 *     otherwise; strides are in ELEMENTS;
 *   - `stream` is a hipStream_t (passed as void* so that C callers need no HIP
 *     headers); work is enqueued stream-ordered, nothing synchronises;
 *   - `device` is the HIP device ordinal the pointers live on, or -1 for "the
 *     calling thread's current device" (nn.DataParallel drives replicas from
 *     one Python thread per GPU, tools/ft_dkt.py:119);
 *   - return 0 on success; negative = argument error detected on the host
 *     before any launch (DKT_E_*); positive = a hipError_t from the launch.
 *     Nothing throws, nothing exits.  dkt_strerror() names either kind;
 *   - stateless and re-entrant: no globals besides read-only tables.
 */
#ifndef DKTSTEREO_H
#define DKTSTEREO_H

#ifdef __cplusplus
extern "C" {
#endif

#define DKT_ABI_VERSION 1
#define DKT_MAX_LEVELS 8

enum {
    DKT_OK = 0,
    DKT_E_NULL = -1,      /* null pointer argument */
    DKT_E_SHAPE = -2,     /* non-positive or inconsistent dimension */
    DKT_E_LEVELS = -3,    /* num_levels outside 1..DKT_MAX_LEVELS or level width reaches 0 */
    DKT_E_RADIUS = -4,    /* radius outside 0..DKT_MAX_RADIUS */
    DKT_E_GROUPS = -5,    /* channels not divisible by groups */
    DKT_E_ALIGN = -6,     /* pointer/stride alignment requirement not met */
    DKT_E_UNSUPPORTED = -7
};
#define DKT_MAX_RADIUS 8

int dkt_version(void);
const char *dkt_strerror(int rc);

/* ---- RAFT-Stereo 1-D correlation --------------------------------------- */

/* All-pairs 1-D correlation fused with the average-pool pyramid.
 * Replaces CorrBlock1D.corr + the pyramid loop of CorrBlock1D.__init__
 * (core/corr.py:148-156 and :111-125; same body meta_arch/raft_stereo/corr.py)
 * and, with divisor = 1, Combined_Geo_Encoding_Volume.corr + its init_corr
 * pyramid (meta_arch/igev_stereo/geometry.py:62-69, :27-29).
 *   pyr[0][n, w2] = (sum_c f1[b,c,h,w1] * f2[b,c,h,w2]) / divisor,  n = (b*H+h)*W1+w1
 *   (divisor = sqrt(C) as the reference divides, corr.py:156)
 *   pyr[i][n, k]  = (pyr[i-1][n,2k] + pyr[i-1][n,2k+1]) * 0.5,  width W2>>i
 * f1: (B,C,H,W1), f2: (B,C,H,W2); pyr: HOST array of L device pointers.
 * Exact fp32 products and fp32 accumulation (v_mfma_f32_32x32x2_f32). */
int dkt_corr1d_build(const float *f1, const float *f2, float *const *pyr,
                     int B, int C, int H, int W1, int W2, int L, float divisor,
                     int device, void *stream);

/* Per-iteration pyramid lookup.  Replaces CorrBlock1D.__call__
 * (core/corr.py:127-146) including its bilinear_sampler/grid_sample round trip
 * (core/utils/utils.py:59-74) and the final permute(0,3,1,2).contiguous().
 *   coords_x: x coordinates, element (b,h,w) at coords_x[b*coords_bstride + h*W1 + w]
 *             (channel 0 of the (B,2,H,W) coords tensor: coords_bstride = 2*H*W1)
 *   out: (B, L*(2r+1), H, W1), channel = level*(2r+1) + tap */
int dkt_corr1d_lookup(const float *const *pyr, const float *coords_x, long coords_bstride,
                      float *out, int B, int H, int W1, int W2, int L, int r,
                      int device, void *stream);

/* Diagonal-major ("skewed") copy of the pyramid and the lookup that reads it:
 *   skew[i][row][s][w1] = pyr[i][row*W1 + w1][(s + (w1 >> i)) mod (W2>>i)],  row = b*H + h
 * with the w1 axis padded to dkt_corr1d_skew_pitch(W1) floats (a multiple of 32: every (row, s)
 * line is 128-byte aligned), i.e. skew[i] holds B*H*(W2>>i)*pitch floats.  Neighbouring pixels with similar disparity then read neighbouring
 * floats: a wave's tap is one contiguous 256-byte load instead of 64 separate lines
 * (corr1d_skew.hip).  dkt_corr1d_lookup_skew returns exactly what dkt_corr1d_lookup does. */
int dkt_corr1d_skew_pitch(int W1);
int dkt_corr1d_skew(const float *const *pyr, float *const *skew, int B, int H, int W1, int W2, int L,
                    int device, void *stream);
int dkt_corr1d_lookup_skew(const float *const *skew, const float *coords_x, long coords_bstride,
                           float *out, int B, int H, int W1, int W2, int L, int r,
                           int device, void *stream);

/* On-the-fly lookup without a volume.  Replaces PytorchAlternateCorrBlock1D
 * (core/corr.py:64-107): samples the (i-times W-pooled) right feature map at
 * the 2r+1 taps and dots it with the left feature vector, / sqrt(C).
 * f2pyr: HOST array of L device pointers to (B,C,H,W2>>i) pooled right maps
 * (built with dkt_pool_w).  coords: (B,2,H,W1) x and y planes. */
int dkt_corr1d_lookup_otf(const float *f1, const float *const *f2pyr, const float *coords,
                          float *out, int B, int C, int H, int W1, int W2, int L, int r,
                          int device, void *stream);

/* avg_pool2d(x,[1,2],stride=[1,2]) on rows: src (rows,W) -> dst (rows,W/2).
 * core/corr.py:104, :124. */
int dkt_pool_w(const float *src, float *dst, long rows, int W, int device, void *stream);

/* L2 normalisation over channels, the prologue of CorrBlock1D_Cosine.corr
 * (core/corr.py:201-202): dst[b,c,p] = src[b,c,p] / ||src[b,:,p]||_2 */
int dkt_l2norm_channels(const float *src, float *dst, int B, int C, long HW,
                        int device, void *stream);

/* ---- up-sampling after the loop ------------------------------------- */

/* RAFTStereo.upsample_flow, meta_arch/raft_stereo/raft_stereo.py:70-82, in one pass:
 * flow (N,D,H,W), mask (N,9*f*f,H,W) -> out (N,D,f*H,f*W);
 * out[n,d,f*h+i,f*w+j] = sum_k softmax_k(mask[n,(k*f+i)*f+j,h,w]) * f*flow[n,d,h+ky-1,w+kx-1]. */
int dkt_convex_upsample(const float *flow, const float *mask, float *out, int N, int D, int H, int W,
                        int factor, int device, void *stream);

/* context_upsample, meta_arch/igev_stereo/submodule.py:242-254: disp_low (B,1,h,w),
 * up_weights (B,9,4h,4w) -> out (B,4h,4w). */
int dkt_context_upsample(const float *disp_low, const float *up_weights, float *out, int B, int h, int w,
                         int device, void *stream);

/* The training path's upsample_flow (meta_arch/raft_stereo/raft_stereo.py:70-82 and, for the backward, torch autograd
 * through those lines), once per refinement iteration of RAFTStereo.forward with test_mode=False (:168).
 *
 * Forward, the leading Dout <= D channels: out (N,Dout,f*H,f*W), bit-identical to dkt_convex_upsample(...)[:, :Dout]
 * (the same operations in the same order per output).  factor in {1,2,4,8}. */
int dkt_convex_upsample_fwd(const float *flow, const float *mask, float *out, int N, int D, int Dout, int H, int W,
                            int factor, int device, void *stream);

/* Backward.  gout (N,Dout,f*H,f*W): batch stride gout_bstride elements, the other dimensions contiguous.  With
 * p_k = softmax_k(mask[n,(k*f+i)*f+j,h,w]) recomputed from the mask and v_{d,k} = f*flow[n,d,h+k/3-1,w+k%3-1]:
 *   gmask[n,(k*f+i)*f+j,h,w] = p_k (a_k - sum_k' p_k' a_k'),   a_k = sum_{d<Dout} gout[n,d,f*h+i,f*w+j] v_{d,k}
 *   gflow[n,d,y,x] = f * sum_k C[n,d,k,y-k/3+1,x-k%3+1],   C[n,d,k,h,w] = sum_{i,j} p_k(i,j,h,w) gout[n,d,f*h+i,f*w+j]
 *   gflow[:, d >= Dout] = 0.
 * gflow (N,D,H,W) or gmask (N,9*f*f,H,W) may be null (not wanted), not both.  ws: N*Dout*9*H*W floats of scratch, needed
 * when gflow is wanted.  Deterministic (no atomics): C is summed over j ascending, then i ascending, gflow over k
 * ascending.  One launch per two channels of Dout plus one for gflow.
 * Errors (both entries): a null pointer the call needs DKT_E_NULL; N, D, H, W <= 0, factor < 1, Dout outside 1..D or a
 * batch stride shorter than one image DKT_E_SHAPE; another factor, N or D > 65535 or H*W > 2^31 - 257 DKT_E_UNSUPPORTED;
 * out / gout not aligned to min(4*f, 16) bytes or gout_bstride not a multiple of f DKT_E_ALIGN. */
int dkt_convex_upsample_bwd(const float *gout, long gout_bstride, const float *flow, const float *mask, float *gflow,
                            float *gmask, float *ws, int N, int D, int Dout, int H, int W, int factor, int device,
                            void *stream);

/* IGEV-Stereo's up-sampling on the training path (meta_arch/igev_stereo/igev_stereo.py:140-148, called once per refinement
 * iteration at :215 and once for init_disp at :222 when test_mode=False).  disp_low (B,1,h,w); the nine-plane tensors
 * (B,9,4h,4w); out / gout (B,4h,4w), gout with batch stride gout_bstride elements and its rows contiguous.  For fine pixel
 * (Y,X) over coarse pixel (y,x) = (Y/4,X/4): nb_k = disp_low[b,0,y+k/3-1,x+k%3-1], 0 outside the image.
 *
 * Backward of context_upsample (torch autograd through meta_arch/igev_stereo/submodule.py:242-254; the forward is
 * dkt_context_upsample):
 *   gweights[b,k,Y,X] = gout[b,Y,X] * nb_k   (one rounding)
 *   gdisp[b,0,y,x] = sum_k C[b,k,y-k/3+1,x-k%3+1] (terms outside the image absent),
 *   C[b,k,y',x'] = sum_{i,j<4} up_weights[b,k,4y'+i,4x'+j] * gout[b,4y'+i,4x'+j].
 * gdisp or gweights may be null (not wanted), not both.  ws: B*9*h*w floats of scratch, needed when gdisp is wanted.
 * Deterministic (no atomics, one owner per element): the four products of a fine row are added in ascending j, the four
 * row sums in ascending i, gdisp in ascending k.  One launch, plus one for gdisp.
 * Errors (all three entries): a null pointer the call needs DKT_E_NULL; B, h, w <= 0 or a batch stride shorter than one
 * image DKT_E_SHAPE; B > 65535 or h*w > 2^31 - 257 DKT_E_UNSUPPORTED; out / gout or a nine-plane tensor not aligned to 16
 * bytes, or gout_bstride not a multiple of 4, DKT_E_ALIGN. */
int dkt_context_upsample_bwd(const float *gout, long gout_bstride, const float *disp_low, const float *up_weights,
                             float *gdisp, float *gweights, float *ws, int B, int h, int w, int device, void *stream);

/* The tail of upsample_disp (igev_stereo.py:145-147: F.softmax(spx_pred, 1), disp*4., context_upsample) in one pass:
 *   out[b,Y,X] = sum_k p_k v_k,  p_k = softmax_k(logits[b,:,Y,X]),  v_k = scale * nb_k,
 * the softmax in the arithmetic of dkt_convex_upsample (max, expf(m - max), the sum in ascending k, one division each),
 * out summed in ascending k with every product rounded.  scale: a finite positive power of two (v_k is then exact), else
 * DKT_E_UNSUPPORTED. */
int dkt_context_upsample_logits_fwd(const float *disp_low, const float *logits, float scale, float *out, int B, int h, int w,
                                    int device, void *stream);

/* Its backward (torch autograd through igev_stereo.py:145-147), the softmax recomputed from the logits:
 *   a_k = gout * v_k,  s = sum_k p_k a_k,  glogits[b,k,Y,X] = p_k (a_k - s)
 *   gdisp[b,0,y,x] = scale * sum_k C[b,k,y-k/3+1,x-k%3+1],  C = sum_{i,j<4} p_k * gout.
 * Null gradients, ws, summation orders and errors as dkt_context_upsample_bwd. */
int dkt_context_upsample_logits_bwd(const float *gout, long gout_bstride, const float *disp_low, const float *logits,
                                    float scale, float *gdisp, float *glogits, float *ws, int B, int h, int w, int device,
                                    void *stream);

/* ---- soft-argmin heads ------------------------------------------------------------------ */

/* GwcNet's disparity head (meta_arch/gwcnet/gwc_main.py:246-276: F.interpolate(cost, scale_factor=4, mode='trilinear',
 * align_corners=False), F.softmax over the planes, disparity_regression of gwcnet/submodules.py:18-22) and, at factor 1,
 * IGEV's initial disparity (meta_arch/igev_stereo/igev_stereo.py:175-176: F.softmax over the 48 planes and
 * disparity_regression) in one launch.  cost (B,Dc,h,w): batch stride cost_bstride elements, the other dimensions
 * contiguous; factor f in {1,4}, D = f*Dc, H = f*h, W = f*w; out (B,1,H,W) contiguous:
 *   out[b,0,Y,X] = out_scale * sum_d d * softmax_d(up(cost))[b,d,Y,X]
 * up: per axis of coarse length n, fine index o reads i0 = floor(src), i1 = min(i0+1, n-1) at lambda = src - i0 with
 * src = max(0, (o+0.5)/f - 0.5): at f = 4, o = 4q+j: (i0, lambda) = (q-1,.625), (q-1,.875), (q,.125), (q,.375); f = 1 is the
 * identity.  The softmax is shifted by the maximum of the pixel's fine logits, summed in ascending d.  The up-sampled
 * volume is never stored.
 * Errors (all three entries): a null pointer the call needs DKT_E_NULL; B, Dc, h, w <= 0 or a batch stride shorter than
 * one image DKT_E_SHAPE; factor outside {1,4}, D > 256, B > 65535, H*W > 2^31 - 257 or H > 524280 DKT_E_UNSUPPORTED; a
 * pointer that is not a multiple of 4 bytes DKT_E_ALIGN. */
int dkt_soft_argmin_fwd(const float *cost, long cost_bstride, float out_scale, float *out, int B, int Dc, int h, int w,
                        int factor, int device, void *stream);

/* Its backward (torch autograd through the lines above), the softmax recomputed from cost: with p_d the softmax, E its
 * expectation and z_d the fine logits, dL/dz_d = out_scale * gout * p_d * (d - E), carried to gcost (B,Dc,h,w), contiguous,
 * through the transpose of the three interpolations.  gout (B,1,H,W): batch stride gout_bstride elements.  Deterministic
 * (no atomics, one owner per element, fixed summation orders).  factor 4: two launches; ws holds the gradient of every
 * output pixel's blended coarse column, dkt_soft_argmin_bwd_workspace bytes.  factor 1: one launch, ws unused (may be null). */
int dkt_soft_argmin_bwd(const float *gout, long gout_bstride, const float *cost, long cost_bstride, float out_scale,
                        float *gcost, void *ws, int B, int Dc, int h, int w, int factor, int device, void *stream);

/* Bytes of ws: 4*B*Dc*H*W at factor 4 (a quarter of the up-sampled volume), 0 at factor 1; negative = the error code the
 * other two entries return for these sizes. */
long dkt_soft_argmin_bwd_workspace(int B, int Dc, int h, int w, int factor);

/* ---- top-k disparity regression --------------------------------------------------------- */

/* CGI-Stereo's disparity head, regression_topk(cost, disparity_samples, k) (meta_arch/cgi/submodule.py:220-228: cost.sort(1,
 * True), the first k indices, torch.gather of the cost and of the samples, F.softmax over the k, product and sum; called with
 * k = 2 on an arange repeated to (B,D,h,w) at meta_arch/cgi/CGI_Stereo.py:256-259) in one launch, nothing sorted or gathered
 * in memory.  cost, samples (B,D,h,w): batch strides cost_bstride, samples_bstride elements, the other dimensions contiguous;
 * out (B,1,h,w) contiguous.  With d_0 .. d_k-1 the planes of the pixel's k largest costs, largest first (equal values in
 * ascending plane order -- the selection of a stable descending sort, and the reference's wherever the k-th and (k+1)-th
 * values differ; a NaN ranks above every number, as in torch's sort), c_i = cost[b,d_i,y,x] and s_i = samples[b,d_i,y,x], or
 * (float)d_i when samples is null (the form CGI calls: no samples tensor is read or needed):
 *   e_i = exp(c_i - c_0),  p_i = e_i / (e_0 + ... + e_k-1),  out[b,0,y,x] = s_0 p_0 + ... + s_k-1 p_k-1.
 * A pixel whose column holds a NaN yields NaN; no other pixel is affected.  idx, when not null: (B,k,h,w) bytes,
 * idx[b,i,y,x] = d_i -- what the backward needs of the forward.
 * Errors (both entries): a null pointer the call needs, or gsamples without samples, DKT_E_NULL; B, D, h, w <= 0, k < 1, k > D
 * or a batch stride shorter than one image DKT_E_SHAPE; k > 8, D > 256, B > 65535 or h*w > 2^31 - 257 DKT_E_UNSUPPORTED; a
 * float pointer that is not a multiple of 4 bytes DKT_E_ALIGN. */
int dkt_topk_regress_fwd(const float *cost, long cost_bstride, const float *samples /* may be null */, long samples_bstride,
                         float *out, unsigned char *idx /* may be null */, int B, int D, int h, int w, int k,
                         int device, void *stream);

/* Its backward (torch autograd through the lines above), p_i and pred = out recomputed from cost, samples and the forward's
 * idx: gcost[b,d_i,y,x] = gout p_i (s_i - pred), gsamples[b,d_i,y,x] = gout p_i, every other plane of both zero.  gout
 * (B,1,h,w): batch stride gout_bstride elements; gcost, gsamples (B,D,h,w) contiguous, each written in full exactly once (no
 * memset needed) or skipped when null (at least one is given).  One launch, deterministic: one owner per pixel, no atomics. */
int dkt_topk_regress_bwd(const float *gout, long gout_bstride, const float *cost, long cost_bstride,
                         const float *samples /* may be null */, long samples_bstride, const unsigned char *idx,
                         float *gcost /* may be null */, float *gsamples /* may be null */,
                         int B, int D, int h, int w, int k, int device, void *stream);

/* ---- backward of lookup / pyramid (autograd of core/corr.py:119-146) -------- */

/* Gradient of every pyramid level from the gradient of one lookup's output:
 *   grad_pyr[i][n, x0] += g*(1-w),  grad_pyr[i][n, x0+1] += g*w   per tap (zero-padding taps drop out).
 * grad_pyr: HOST array of L device pointers, shaped like the pyramid, ZEROED (or holding the
 * sum of earlier lookups' gradients) by the caller.  coords are detached upstream
 * (raft_stereo.py:152): no coordinate gradient. */
int dkt_corr1d_lookup_bwd(const float *grad_out, const float *coords_x, long coords_bstride,
                          float *const *grad_pyr, int B, int H, int W1, int W2, int L, int r,
                          int device, void *stream);

/* IGEV flavour (autograd of meta_arch/igev_stereo/geometry.py:23-58 w.r.t. the volume and the init
 * correlation; disp is detached upstream, igev_stereo.py:200).  grad_geo[i]: (B,C,D>>i,H,W), grad_init[i]:
 * (B*H*W, W2>>i), both zeroed (or holding earlier lookups' sums) by the caller. */
int dkt_geo_lookup_bwd(const float *grad_out, const float *disp, const float *coords,
                       float *const *grad_geo, float *const *grad_init,
                       int B, int C, int D, int H, int W, int W2, int L, int r, int device, void *stream);
/* grad_vol (BC, D, HW) = T_0 with T_{L-1} = g_{L-1}, T_i[d] = g_i[d] + T_{i+1}[d/2]/2 (pairwise-mean pyramid). */
int dkt_geo_pool_bwd(const float *const *grad_geo, float *grad_vol, long BC, int D, long HW, int L,
                     int device, void *stream);

/* Folds the avg_pool2d backward chain and the 1/sqrt(C) of CorrBlock1D.corr into the gradient
 * of the un-pooled all-pairs product: grad_vol (B*H*W1, W2) = T_0 / divisor with
 * T_{L-1} = g_{L-1}, T_i[c] = g_i[c] + T_{i+1}[c/2]/2.  The two contractions that follow
 * (grad_fmap1 = grad_vol x fmap2, grad_fmap2 = grad_vol^T x fmap1) are plain library GEMMs. */
int dkt_corr1d_pool_bwd(const float *const *grad_pyr, float *grad_vol, int B, int H, int W1, int W2,
                        int L, float divisor, int device, void *stream);

/* ---- PCVNet correlation block / CGI normalised correlation -------- */

/* F.avg_pool2d(x,[1,factor],stride=[1,factor]) on rows: src (rows,W) -> dst (rows,W/factor);
 * the pyramid of meta_arch/pcvnet/corr.py:27-31 (factor 4 when n_downsample == 2, else 2). */
int dkt_pool_rows(const float *src, float *dst, long rows, int W, int factor, int device, void *stream);

/* PCVNet CorrBlock1D.__call__(coords, sigma), meta_arch/pcvnet/corr.py:33-51.
 * pyr: HOST array of L device pointers, level i (B*H*W1, W_i), W_0 = W2, W_{i+1} = W_i/factor.
 * coords, sigma: (B,G,H,W1).  out: (B, L*G*S, H, W1), channel = level*G*S + g*S + s,
 * sampled at (dx_s * sigma + coords) / factor^level, dx = -(S/2)..(S/2) (S odd). */
int dkt_pcv_lookup(const float *const *pyr, const float *coords, const float *sigma, float *out,
                   int B, int G, int H, int W1, int W2, int L, int S, int factor,
                   int device, void *stream);

/* Its backward: torch autograd through meta_arch/pcvnet/corr.py:33-51 and the grid_sample of pcvnet/utils/utils.py:59-74.
 * sigma is differentiated as well as the pyramid: it is the previous iteration's head output and reaches the call with its
 * graph (meta_arch/pcvnet/model.py:141 -> :122).  pyr (the values), coords, sigma as in the forward; grad_out (B, L*G*S, H, W1).
 * Three results, each skipped when null (at least one is given):
 *   grad_pyr  HOST array of L device pointers shaped like pyr, ZEROED (or holding earlier lookups' sums) by the caller:
 *             grad_pyr[lv][n, fl] += g e, grad_pyr[lv][n, fl+1] += g w per tap in (g, s) order, zero-padding taps drop out;
 *   gcoords, gsigma (B,G,H,W1), written in full: with d = g (v1m - v0m) / factor^lv, v0m and v1m the two taps after the
 *             out-of-range one is zeroed, gcoords = sum d and gsigma = sum (s - S/2) d in ascending (level, s) order.
 * Floors and weights are the forward's.  Deterministic: one owner per element, no atomics, no workspace; one launch for
 * grad_pyr and one for gcoords / gsigma.  Errors: a null pointer the call needs or no result asked for DKT_E_NULL; B, G, H,
 * W1, W2, S <= 0, S even, factor < 2 or B > 65535 DKT_E_SHAPE; L outside 1..DKT_MAX_LEVELS or a last level narrower than 2
 * (the reference divides by W_i - 1) DKT_E_LEVELS. */
int dkt_pcv_lookup_bwd(const float *const *pyr, const float *coords, const float *sigma, const float *grad_out,
                       float *const *grad_pyr /* may be null */, float *gcoords /* may be null */,
                       float *gsigma /* may be null */, int B, int G, int H, int W1, int W2, int L, int S, int factor,
                       int device, void *stream);

/* Folds the backward of the F.avg_pool2d(corr, [1,factor], stride=[1,factor]) chain of meta_arch/pcvnet/corr.py:29-31 and
 * the 1/sqrt(D) of CorrBlock1D.corr (:61) into the gradient of the un-pooled all-pairs product: grad_vol (B*H*W1, W2) =
 * T_0 / divisor with T_{L-1} = g_{L-1}, T_i[c] = g_i[c] + (c/factor < W_{i+1} ? T_{i+1}[c/factor] / factor : 0),
 * W_{i+1} = W_i / factor (floor).  grad_pyr: HOST array of L device pointers, level i (B*H*W1, W_i).  Each element of
 * grad_vol has one owner.  Errors as above, without the limit on B (the launch does not put it on the grid) and with
 * DKT_E_SHAPE for a divisor that is not positive.  The two contractions that follow are those of dkt_corr1d_pool_bwd. */
int dkt_pcv_pool_bwd(const float *const *grad_pyr, float *grad_vol, int B, int H, int W1, int W2,
                     int L, int factor, float divisor, int device, void *stream);

/* PCVNet's mixture-parameter update: ParametersUpdater.forward after its conv head (meta_arch/pcvnet/update.py:92-107) and
 * the disparity regression of meta_arch/pcvnet/model.py:154, in one launch.  delta (the head's output), mu, sigma, w and the
 * three results (N,M,H,W) contiguous, M = gauss_num; per pixel, j over the M gaussians:
 *   ds_raw = 0.5 (((1 - M w) sigma^2 - sigma0^2 - delta^2) / (M sigma^3) + w sigma / sigma0^2)
 *   dm_raw = -0.5 delta (1 / (M sigma^2) + w / sigma0^2)
 *   beta   = 0.5 (-1 / (M w + eps) + log(sigma0 M w / sigma + eps) + (sigma^2 + delta^2) / (2 sigma0^2) + 0.5)
 *   dw_raw = beta - (sum_j beta) / M
 *   ds = clip(gamma1 ds_raw, +-3)   dm = clip(gamma2 dm_raw, +-128)   dw = clip(gamma3 dw_raw, +-1/(4M))
 *   sigma_out = clip(sigma - ds, 0.1, 16)   mu_out = mu - dm   w~ = clip(w - dw, 0, 1)   w_out = w~ / sum_j w~
 *   disp (N,1,H,W) = sum_j w_out mu_out                              (skipped when null)
 * code (N,M,H,W) bytes, skipped when null: the five three-state clip decisions of an element (0 below, 1 inside or on an
 * edge, 2 above) as (((ds 3 + dm) 3 + dw) 3 + sigma_out) 3 + w~, at most 242: all the backward needs beside the four inputs.
 * One thread per pixel (four adjacent ones as 16-byte accesses when H*W is a multiple of 4 and every pointer is 16-byte
 * aligned), sums in ascending j, IEEE division and logf: the same bits every run.  A pixel whose w~ are all zero is NaN in
 * w_out and disp, as in the reference.
 * Errors (both entries, before any device call): a null pointer the call needs DKT_E_NULL; N, M, H, W <= 0 DKT_E_SHAPE;
 * M > 8, N > 65535 or H*W > 2^31 - 257 DKT_E_UNSUPPORTED. */
int dkt_pcv_update_fwd(const float *delta, const float *mu, const float *sigma, const float *w,
                       float *mu_out, float *w_out, float *sigma_out, float *disp /* may be null */,
                       unsigned char *code /* may be null */, int N, int M, int H, int W,
                       float sigma0, float eps, float gamma1, float gamma2, float gamma3, int device, void *stream);

/* Its backward (torch autograd through update.py:92-107 and model.py:154), one launch.  The four inputs and code as the
 * forward read and wrote them; upstream gradients gmu_out, gw_out, gsigma_out (N,M,H,W) and gdisp (N,1,H,W), a null one
 * standing for zeros; results gdelta, gmu, gsigma, gw (N,M,H,W), a null one not computed.  All four upstream gradients
 * null, or all four results null, is DKT_E_NULL.  beta, dm_raw, w~ and w_out are recomputed from the inputs by the
 * forward's own functions with the decisions replayed from code; a clip passes its gradient where the value was inside or
 * on the edge (torch.clamp's backward).  With T = sum_j w~, u = sigma0 M w / sigma + eps and c the pass indicators:
 *   Gmu = gmu_out + gdisp w_out   Gw = gw_out + gdisp mu_out   A = c_w~ (Gw - sum_k Gw_k w_out_k) / T   B = -gamma3 c_dw A
 *   gbeta = B - (sum_k B_k) / M   E = c_sigma gsigma_out   g_ds = -gamma1 c_ds E   g_dm = -gamma2 c_dm Gmu
 *   gdelta = g_ds (-delta / (M sigma^3)) + g_dm (-0.5 (1 / (M sigma^2) + w / sigma0^2)) + gbeta delta / (2 sigma0^2)
 *   gsigma = E + g_ds 0.5 (-(1 - M w) / (M sigma^2) + 3 (sigma0^2 + delta^2) / (M sigma^4) + w / sigma0^2)
 *            + g_dm delta / (M sigma^3) + gbeta 0.5 (-(sigma0 M w / sigma^2) / u + sigma / sigma0^2)
 *   gw = A + g_ds 0.5 (-1 / sigma + sigma / sigma0^2) + g_dm (-0.5 delta / sigma0^2)
 *        + gbeta 0.5 (M / (M w + eps)^2 + (sigma0 M / sigma) / u),            gmu = Gmu.
 * Deterministic: one owner per element, no atomics, no workspace. */
int dkt_pcv_update_bwd(const float *delta, const float *mu, const float *sigma, const float *w, const unsigned char *code,
                       const float *gmu_out /* may be null */, const float *gw_out /* may be null */,
                       const float *gsigma_out /* may be null */, const float *gdisp /* may be null */,
                       float *gdelta /* may be null */, float *gmu /* may be null */, float *gsigma /* may be null */,
                       float *gw /* may be null */, int N, int M, int H, int W,
                       float sigma0, float eps, float gamma1, float gamma2, float gamma3, int device, void *stream);

/* y = x / (||x||_2 over each of G contiguous channel groups + eps): the normalisation inside
 * groupwise_correlation_norm / norm_correlation, meta_arch/cgi/submodule.py:149,168 (eps 1e-5).
 * build_gwc_volume_norm(ref,tgt,D,G) = dkt_gwc_volume on the two normalised maps;
 * build_norm_correlation_volume is G = 1. */
int dkt_group_l2norm(const float *x, float *y, int B, int C, long HW, int G, float eps,
                     int device, void *stream);

/* ---- IGEV combined geometry encoding volume ------------------------------ */

/* Pairwise mean along D of a (B*C, D, HW) volume -> (B*C, D/2, HW): the
 * geometry-volume pyramid of geometry.py:23-25 without the permute copy of :18. */
int dkt_pool_d(const float *src, float *dst, long BC, int D, long HW, int device, void *stream);

/* Replaces Combined_Geo_Encoding_Volume.__call__ (geometry.py:34-58).
 *   geo_pyr[i]: (B,C,D>>i,H,W)  -- the network's native layout, read in place
 *   init_pyr[i]: (B*H*W, W2>>i) -- from dkt_corr1d_build(divisor=1)
 *   disp: (B,1,H,W); coords: (B,H,W,1) x positions (igev_stereo.py:195)
 *   out: (B, L*K*(C+1), H, W), per level [c*K+k for c<C] then [init k] */
int dkt_geo_lookup(const float *const *geo_pyr, const float *const *init_pyr,
                   const float *disp, const float *coords, float *out,
                   int B, int C, int D, int H, int W, int W2, int L, int r,
                   int device, void *stream);

/* ---- cost-volume builders -------------------------------------------------- */

/* Replaces build_gwc_volume + groupwise_correlation
 * (meta_arch/igev_stereo/submodule.py:152-170 == meta_arch/gwcnet/submodules.py:39-58).
 *   vol[b,g,d,h,w] = mean_{c in group g} ref[b,c,h,w]*tgt[b,c,h,w-d] (w>=d) else 0
 * vol_bstride: batch stride of vol in elements (G*D*H*W when dense; larger to
 * write straight into a wider (B,G+2C',D,H,W) buffer, gwc_main.py:315). */
int dkt_gwc_volume(const float *ref, const float *tgt, float *vol,
                   int B, int C, int H, int W, int D, int G, long vol_bstride,
                   int device, void *stream);
/* The same volume as a banded matrix product on the exact-fp32 matrix pipe (v_mfma_f32_16x16x4_f32, gwc_mfma.hip):
 * an fma chain over the group's channels in ascending order -- within one rounding per product of dkt_gwc_volume's
 * (and the reference's) sum of rounded products; D = 48, C/G in {4, 8, 12, 16}, W % 4 == 0, 16-byte aligned volume
 * rows, else DKT_E_UNSUPPORTED (callers fall back to dkt_gwc_volume). */
int dkt_gwc_volume_mfma(const float *ref, const float *tgt, float *vol,
                        int B, int C, int H, int W, int D, int G, long vol_batch_stride,
                        int device, void *stream);

/* Replaces build_concat_volume.  ref_masked = 1: GwcNet semantics
 * (meta_arch/gwcnet/submodules.py:25-36, reference half only where w >= d);
 * ref_masked = 0: IGEV copy (meta_arch/igev_stereo/submodule.py:207-218,
 * reference half for every w).  vol: (B,2C,D,H,W) with batch stride vol_bstride. */
int dkt_concat_volume(const float *ref, const float *tgt, float *vol,
                      int B, int C, int H, int W, int D, int ref_masked, long vol_bstride,
                      int device, void *stream);

/* Backward of dkt_gwc_volume: torch autograd through build_gwc_volume's per-disparity slices
 * (meta_arch/igev_stereo/submodule.py:152-170 == meta_arch/gwcnet/submodules.py:39-58).
 *   grad_ref[b,gc,h,w]  = (1/cpg) sum_{d <= w, d < D}   grad_vol[b,g,d,h,w]    * tgt[b,gc,h,w-d]
 *   grad_tgt[b,gc,h,w'] = (1/cpg) sum_{d < D, w'+d < W} grad_vol[b,g,d,h,w'+d] * ref[b,gc,h,w'+d]
 * grad_vol: (B,G,D,H,W) with batch stride vol_bstride (the gwc part of the fused buffer is read in place).
 * grad_ref / grad_tgt: (B,C,H,W), overwritten; either may be null (not both).  Deterministic: no atomics,
 * each element summed by one thread in ascending d. */
int dkt_gwc_volume_bwd(const float *grad_vol, long vol_bstride, const float *ref, const float *tgt,
                       float *grad_ref, float *grad_tgt, int B, int C, int H, int W, int D, int G,
                       int device, void *stream);

/* Backward of dkt_concat_volume (a banded sum of grad_vol over d):
 * ref_masked = 1: meta_arch/gwcnet/submodules.py:25-36   grad_ref[c,w] = sum_{d <= w, d < D} grad_vol[c,d,w]
 * ref_masked = 0: meta_arch/igev_stereo/submodule.py:207-218  grad_ref[c,w] = sum_{d < D} grad_vol[c,d,w]
 * both:  grad_tgt[c,w'] = sum_{d < D, w'+d < W} grad_vol[C+c,d,w'+d]        (h and b implied)
 * grad_vol: (B,2C,D,H,W) with batch stride vol_bstride.  Either output may be null (not both). */
int dkt_concat_volume_bwd(const float *grad_vol, long vol_bstride, float *grad_ref, float *grad_tgt,
                          int B, int C, int H, int W, int D, int ref_masked, int device, void *stream);

/* Both parts of the fused (B, G+2Cc, D, H, W) buffer of dkt_gwc_volume + dkt_concat_volume (the backward of
 * gwc_main.py:310-315's torch.cat): channels [0,G) as dkt_gwc_volume_bwd (ref, tgt: (B,C,H,W)), channels
 * [G, G+2Cc) as dkt_concat_volume_bwd (grad_cat_*: (B,Cc,H,W)), in one launch.  Any one of the four outputs
 * may be null; ref / tgt only matter when a gwc gradient is requested. */
int dkt_gwc_concat_volume_bwd(const float *grad_vol, long vol_bstride, const float *ref, const float *tgt,
                              float *grad_ref, float *grad_tgt, int B, int C, int G,
                              float *grad_cat_ref, float *grad_cat_tgt, int Cc, int ref_masked,
                              int H, int W, int D, int device, void *stream);

/* ---- ConvGRU gate fusions ---------------------------------------------------- */

/* First gate stage of ConvGRU.forward (core/update.py:27-29 ==
 * meta_arch/igev_stereo/update.py:37-39) given the raw outputs of the merged
 * convz|convr convolution:
 *   z  = sigmoid(azr[:, :Ch] + cz);  r = sigmoid(azr[:, Ch:] + cr);  rh = r * h
 * azr: (B,2Ch,HW) dense.  cz, cr, h: (B,Ch,HW) with batch strides (context
 * tensors are split views, raft_stereo.py:114).  z: dense (B,Ch,HW).
 * rh: written with batch stride rh_bstride (straight into the first Ch channels
 * of the [r*h | x] input buffer of convq, replacing the torch.cat of :29). */
int dkt_gru_gate_zr(const float *azr, const float *cz, long cz_bstride,
                    const float *cr, long cr_bstride, const float *h, long h_bstride,
                    float *z, float *rh, long rh_bstride,
                    int B, int Ch, long HW, int device, void *stream);

/* Second gate stage (core/update.py:29-31): q = tanh(aq + cq);
 * h' = (1 - z) * h + z * q.  hout may alias h. */
int dkt_gru_gate_out(const float *aq, const float *cq, long cq_bstride,
                     const float *z, const float *h, long h_bstride,
                     float *hout, long hout_bstride,
                     int B, int Ch, long HW, int device, void *stream);

/* The same two stages on the training path (BasicMultiUpdateBlock under autograd; core/update.py:23-32 ==
 * meta_arch/igev_stereo/update.py:33-41, and torch autograd through those lines for the two backward entries).
 *
 * Forward: the arithmetic of dkt_gru_gate_zr / dkt_gru_gate_out plus the one plane the backward needs: r, q (dense
 * (B,Ch,HW)).  z, rh and hout are bit-identical to what dkt_gru_gate_zr / dkt_gru_gate_out write from the same inputs. */
int dkt_gru_gate_zr_train(const float *azr, const float *cz, long cz_bstride,
                          const float *cr, long cr_bstride, const float *h, long h_bstride,
                          float *z, float *r, float *rh, long rh_bstride,
                          int B, int Ch, long HW, int device, void *stream);
int dkt_gru_gate_out_train(const float *aq, const float *cq, long cq_bstride,
                           const float *z, const float *h, long h_bstride,
                           float *q, float *hout, long hout_bstride,
                           int B, int Ch, long HW, int device, void *stream);

/* Backward of the second stage, one launch.  gout: the gradient of h' (batch stride gout_bstride); z, q: dense, as the
 * forward wrote them; h with its batch stride.  Dense (B,Ch,HW) outputs, each may be null (not wanted), not all three:
 *   gaq = (gout*z)*(1 - q*q)   (the gradient of aq and of cq)
 *   gz  = gout*(q - h)
 *   gh  = gout*(1 - z)
 * Every product and difference rounded once, in the order written. */
int dkt_gru_gate_out_bwd(const float *gout, long gout_bstride, const float *z, const float *q,
                         const float *h, long h_bstride, float *gaq, float *gz, float *gh,
                         int B, int Ch, long HW, int device, void *stream);

/* Backward of the first stage, one launch.  gz: the gradient of z (dense); grh: the gradient of rh (batch stride
 * grh_bstride); z, r: dense, as the forward wrote them.  gazr (B,2Ch,HW) dense: the gradient of the merged z|r
 * pre-activation (its halves are the gradients of cz and cr); gh (B,Ch,HW) dense.  Either may be null, not both:
 *   gazr[:, :Ch] = (gz*z)*(1 - z)
 *   gazr[:, Ch:] = ((grh*h)*r)*(1 - r)
 *   gh           = grh*r
 * All four entries: a null pointer the call needs DKT_E_NULL; B, Ch or HW <= 0 DKT_E_SHAPE.  16-byte accesses when
 * Ch*HW, every batch stride and every pointer allow it, 4-byte ones otherwise. */
int dkt_gru_gate_zr_bwd(const float *gz, const float *grh, long grh_bstride, const float *z, const float *r,
                        const float *h, long h_bstride, float *gazr, float *gh,
                        int B, int Ch, long HW, int device, void *stream);

/* ---- update-operator convolutions ------------------------------------------------ */

/* Correlation lookup fused with the 1x1 convolution that consumes it: core/corr.py:127-146
 * (CorrBlock1D.__call__) followed by relu(convc1(corr)) of BasicMotionEncoder (core/update.py:72,79).
 * One launch; the (B, L*K, H, W1) lookup tensor is never written.  `skew` is the pyramid written by
 * dkt_corr1d_skew; weight_t is convc1.weight viewed (Cout, L*K) and TRANSPOSED to (L*K, Cout), fp32,
 * used as is: the product runs on the exact-fp32 matrix instruction (an fp32 fma chain over the taps).
 *   out[b,co,h,w] = [relu]( bias[co] + sum_k weight[co,k] * lookup[b,k,h,w] )
 * tap (optional, may be NULL): receives lookup[b,k,h,w] itself -- bit-identical to dkt_corr1d_lookup_skew.
 * Supported: Cout <= 64, L in {2,3,4}, r in {3,4}; otherwise DKT_E_UNSUPPORTED (callers then run
 * dkt_corr1d_lookup_skew + dkt_conv2d_f16s_desc). */
int dkt_corr1d_lookup_conv1x1(const float *const *skew, const float *coords_x, long coords_bstride,
                              const float *weight_t, const float *bias, float *out, long out_bstride,
                              float *tap, long tap_bstride,
                              int B, int H, int W1, int W2, int L, int r, int Cout, int relu,
                              int device, void *stream);

/* Weight images of the split-fp16 convolution (dkt_conv2d_f16s_desc / _pair below, where the contract is): packed once per
 * layer, for one list of cat operands. */
#define DKT_CONV_MAX_SRC 4
long dkt_conv2d_packed_elems(const int *src_channels, int nsrc, int Cout, int KH, int KW);
int dkt_conv2d_pack_weights(const float *w /* (Cout,sum(src_channels),KH,KW) */,
                            const int *src_channels, int nsrc, int Cout, int KH, int KW, float scale,
                            void *w_hi /* fp16[packed_elems] */, void *w_lo, int device, void *stream);

/* ---- backward of the update-operator convolutions (training; dkt_stereo_amd/conv.py: _Conv2dFn.backward) ----
 * torch autograd through [relu](conv2d(x, w, b)), stride 1, "same" padding (core/update.py:9-10, 19-21, 72-76, 111-113):
 *   g' = gy * (y > 0),  gb = g'.sum((0, 2, 3)),  gx = conv2d(g', w transposed over (Cout, Cin) and rotated by 180 degrees).
 *
 * dkt_conv_grad_prepass: one streaming pass over gy (B, C, HW; batch stride gy_bstride, each batch element dense) and a
 * one-block finish; the host reads nothing back.
 *   y      (optional) the saved output of a ReLU layer, batch stride y_bstride.  With y:  gmask[b,c,i] = y > 0 ? gy : 0,
 *          dense (B, C, HW), required.  Without y nothing is copied (g' is gy itself) and gmask is ignored.
 *   gb     (optional) C floats: the sum of g' over (b, i) in an order fixed by the shape alone -- a plane in segments of
 *          4096 elements, one segment per block; no float atomics -- bit-identical from run to run, for every grid size and
 *          for the 16-byte and the 4-byte path alike.
 *   scale  two floats {2^e, 2^-e}: e = 12 - floor(log2(max|g'|)), i.e. max|g'| * 2^e in [2^12, 2^13) (the window
 *          dkt_conv2d_pack_weights' callers put the weights in), clamped to |e| <= DKT_CONV_GRAD_MAX_EXP, which keeps both
 *          floats, and the out_scale of a dkt_conv_desc with `dscale` for any weight scale in [2^-46, 2^46], normal; e = 0 when
 *          max|g'| is 0, Inf or NaN (a non-finite gradient is passed on as it is and comes out non-finite).
 *   ws     dkt_conv_grad_prepass_ws_floats(B, C, HW) floats of scratch, written before they are read.
 * 16-byte accesses when HW, the batch strides and the pointers allow it, 4-byte ones otherwise.
 * Errors: gy, scale or ws null, or y without gmask, DKT_E_NULL; B, C, HW <= 0 or a batch stride shorter than C*HW
 * DKT_E_SHAPE. */
#define DKT_CONV_GRAD_MAX_EXP 80
long dkt_conv_grad_prepass_ws_floats(int B, int C, long HW);
int dkt_conv_grad_prepass(const float *gy, long gy_bstride, const float *y, long y_bstride,
                          float *gmask, float *gb, float *scale, float *ws,
                          int B, int C, long HW, int device, void *stream);

/* dkt_conv2d_wgrad: the weight gradient of [relu](conv2d(x, w, b)), stride 1, "same" padding p = K/2, K in {1, 3}
 * (core/update.py:9-10, 19-21, 72-76, 111-113 under training):
 *   gw[co][ci][ky][kx] = sum_{b,y,x} g[b,co,y,x] * x[b,ci,y+ky-p,x+kx-p]
 * x (B, Cin, H, W) and g (B, Cout, H, W; the masked gradient g') fp32 NCHW, every batch element dense, batch strides
 * x_bstride / g_bstride (g may be the upstream gradient read in place); gw (Cout, Cin, K, K) dense fp32.
 *   scale    the device pair {s, 1/s} of g as dkt_conv_grad_prepass writes it: g * s is split into fp16 hi + lo
 *   x_scale  a host power of two: x * x_scale is split the same way (the layer's forward in_scale; 1 by default)
 *   ws       dkt_conv2d_wgrad_ws_floats(B, Cin, Cout, H, W, K) floats of scratch, written before they are read
 * Three v_mfma_f32_32x32x16_f16 products (g_hi*x_hi + g_lo*x_hi + g_hi*x_lo), fp32 accumulation, un-scaled by
 * scale[1] / x_scale; every factor outside the fp16 operands is a power of two, so a power-of-two multiple of g gives that
 * multiple of gw bit for bit.  The reduction is cut into slices (batch element x band of rows) by a rule of the shape alone,
 * partial tiles go to ws and a finishing kernel adds a weight's slices in ascending order: no float atomics, bit-identical
 * from run to run, for every grid size, and for the 16-byte (pointers, strides and W allow it) and the 4-byte load path.
 * A non-finite g (pair e = 0) or x comes out non-finite.  The host reads nothing back.
 * Errors, before any device is touched: x, g, scale, gw or ws null DKT_E_NULL; a size <= 0, K not in {1, 3}, a batch stride
 * shorter than C*H*W, or x_scale not a positive finite power of two DKT_E_SHAPE. */
long dkt_conv2d_wgrad_ws_floats(int B, int Cin, int Cout, int H, int W, int K);
int dkt_conv2d_wgrad(const float *x, long x_bstride, const float *g, long g_bstride,
                     const float *scale /* device {s, 1/s} of g */, float x_scale,
                     float *gw /* (Cout,Cin,K,K) dense */, float *ws,
                     int B, int Cin, int Cout, int H, int W, int K, int device, void *stream);

/* ---- backward of the encoders' stride-2 convolutions (training; core/extractor.py:6-60, :122-175 under training) ----
 * torch autograd through conv2d(x, w, b, stride=2, padding=K/2), K in {1, 3}; x (B, Cin, H, W), g (B, Cout, Ho, Wo) the
 * masked gradient g', Ho = (H-1)/2+1, Wo = (W-1)/2+1, any H, W >= 1.  fp32 NCHW, every batch element dense, batch strides
 * in floats (views with a longer batch stride and pointers 4 bytes past a 16-byte boundary are fine).  scale is the device
 * pair {s, 1/s} dkt_conv_grad_prepass leaves for g, read by the kernels, never by the host.
 *
 * dkt_conv2d_dgrad_s2: gx[b,ci,y,x] = sum g[b,co,oy,ox] * w[co,ci,ky,kx] over y = 2oy+ky-p, x = 2ox+kx-p.
 *   w_hi/w_lo   dkt_conv2d_pack_weights of the input-gradient weight (w transposed over (Cout, Cin), rotated by 180
 *               degrees: shape (Cin, Cout, K, K)) with src_channels = {Cout}, nsrc = 1; w_inv_scale = 1 / its scale.
 *   Decomposed by output parity on the Ho x Wo grid (1 / 2 / 2 / 4 taps; nine products per pixel of g for K = 3): every
 *   element of gx (B, Cin, H, W) is stored exactly once by the kernel, the zeros of a 1x1 layer's odd rows and columns
 *   included -- no memset, no zero-inserted copy of g, no atomics; the same bits from run to run.  g * scale[0] and the
 *   weight as fp16 hi + lo, three v_mfma_f32_32x32x16_f16 products, fp32 accumulation, un-scaled by scale[1] * w_inv_scale:
 *   a power-of-two multiple of g gives that multiple of gx bit for bit.
 *   Errors, before any device is touched: g, w_hi, w_lo, scale or gx null DKT_E_NULL; a size < 1, K not in {1, 3}, a batch
 *   stride shorter than C*H*W of its tensor, or w_inv_scale not positive and finite DKT_E_SHAPE.
 *
 * dkt_conv2d_wgrad_s2: gw[co][ci][ky][kx] = sum_{b,oy,ox} g[b,co,oy,ox] * x[b,ci,2oy+ky-p,2ox+kx-p]; the contract of
 *   dkt_conv2d_wgrad (operands split while staged, three products, split-K over (batch element, band of OUTPUT rows) into
 *   ws, a finishing kernel that adds slices in ascending order and un-scales by scale[1] / x_scale; no float atomics, the
 *   same bits for every grid size and for the 16-byte and the 4-byte load path; scale-equivariant bit for bit).  x is
 *   de-interleaved into even and odd column planes while it is staged, so every LDS read stays aligned.
 *   ws: dkt_conv2d_wgrad_s2_ws_floats(B, Cin, Cout, H, W, K) floats (H, W the INPUT size).  Errors as dkt_conv2d_wgrad. */
int dkt_conv2d_dgrad_s2(const float *g, long g_bstride, const void *w_hi, const void *w_lo, float w_inv_scale,
                        const float *scale /* device {s, 1/s} of g */, float *gx, long gx_bstride,
                        int B, int Cin, int Cout, int H, int W, int K, int device, void *stream);
long dkt_conv2d_wgrad_s2_ws_floats(int B, int Cin, int Cout, int H, int W, int K);
int dkt_conv2d_wgrad_s2(const float *x, long x_bstride, const float *g, long g_bstride,
                        const float *scale /* device {s, 1/s} of g */, float x_scale,
                        float *gw /* (Cout,Cin,K,K) dense */, float *ws,
                        int B, int Cin, int Cout, int H, int W, int K, int device, void *stream);

/* ---- weight gradient of the 7x7 stem layers (training; core/extractor.py:140, :217 conv1 3 -> 64, core/update.py:73
 * convf1 2 -> 64, meta_arch/igev_stereo/update.py:80 convd1 1 -> 64, under training) ----
 * torch autograd's weight gradient through conv2d(x, w, b, padding=3) of a 7x7 stride-1 layer with 1 <= Cin <= 4:
 *   gw[co][ci][ky][kx] = sum_{b,y,x} g[b,co,y,x] * x[b,ci,y+ky-3,x+kx-3],   any Cout, B, H, W >= 1.
 * Operands, scale, x_scale and ws as dkt_conv2d_wgrad, and its contract in every point: both operands split into fp16
 * hi + lo while staged, three v_mfma_f32_32x32x16_f16 products with fp32 accumulation, the GEMM columns are the (ci, ky, kx)
 * triples; split-K over (batch element, band of rows) into ws, the same finishing kernel adds a weight's slices in ascending
 * order and un-scales by scale[1] / x_scale.  No float atomics; the same bits from run to run, for every grid size and for
 * the 16-byte and the 4-byte load path; a power-of-two multiple of g gives that multiple of gw bit for bit; a non-finite
 * g or x comes out non-finite; the host reads nothing back.
 *   ws: dkt_conv2d_wgrad7_ws_floats(B, Cin, Cout, H, W) floats (the negative code for a bad shape).
 * Errors, before any device is touched: x, g, scale, gw or ws null DKT_E_NULL; a size <= 0, Cin > 4, a batch stride shorter
 * than C*H*W, or x_scale not a positive finite power of two DKT_E_SHAPE. */
long dkt_conv2d_wgrad7_ws_floats(int B, int Cin, int Cout, int H, int W);
int dkt_conv2d_wgrad7(const float *x, long x_bstride, const float *g, long g_bstride,
                      const float *scale /* device {s, 1/s} of g */, float x_scale,
                      float *gw /* (Cout,Cin,7,7) dense */, float *ws,
                      int B, int Cin, int Cout, int H, int W, int device, void *stream);

/* nn.Conv2d with "same" zero padding K/2, 1x1 or 3x3, stride 1 or 2, as used by ConvGRU, BasicMotionEncoder,
 * FlowHead/DispHead, the mask heads (core/update.py:9-10, 19-21, 72-76, 111-113; meta_arch/igev_stereo/update.py same
 * lines) and the encoders (core/extractor.py:16,34), evaluated as an implicit GEMM on the fp16 matrix cores with split
 * operands and fp32 accumulation (see conv2d.hip).  One convolution is one dkt_conv_desc; a zero-initialised descriptor
 * leaves every option off.
 *   src       up to DKT_CONV_MAX_SRC NCHW fp32 tensors that the reference concatenates along channels before the
 *             convolution (torch.cat at core/update.py:24-25,29,83) -- they are read in place.  The weights must have been
 *             packed by dkt_conv2d_pack_weights with the SAME src_channels list.
 *   passes    (an argument of the launch) 3 = w_hi*x_hi + w_lo*x_hi + w_hi*x_lo (fp32-class accuracy), 2 = activations
 *             rounded to fp16, 1 = plain fp16.
 *   scales    activations are multiplied by in_scale (a power of two, 1 by default in the Python layer) before they are
 *             split into fp16 parts; out_scale = 1 / (weight scale * in_scale).  Range: |x * in_scale| < 65520; 22
 *             significant bits for |x * in_scale| >= 2^-3, an absolute floor of 2^-25 below.  Out-of-range, Inf and NaN
 *             activations yield non-finite outputs (they are never saturated silently).
 *   stride    H, W are the INPUT size; out is (B, Cout, (H-1)/stride+1, (W-1)/stride+1) with batch stride out_bstride.
 *             Stride 2 (the encoders' 3x3 down-sampling layers and 1x1 projections) takes epilogue 0 only.
 *   epilogue 0: out[b,co,h,w] = out_scale*acc + bias[co] [ReLU];  Cout = layer outputs
 *   epilogue 1: ConvGRU first stage (core/update.py:23-32), the merged convz|convr layer over [h | x...], Cout = 2*Ch with
 *               Ch a multiple of 64: z = sigmoid(conv_z + cz) -> out, r*h = sigmoid(conv_r + cr) * h -> out2
 *               (e0 = cz, e1 = cr)
 *   epilogue 2: ConvGRU second stage, convq over [r*h | x...], Cout = Ch: (1-z)*h + z*tanh(conv_q + cq) -> out
 *               (e0 = cq, e1 = z; out may alias h)
 *   epilogue 3: residual join of a residual block whose norm is folded into the weights (core/extractor.py:52-60):
 *               out = relu(e0 + [ReLU](out_scale*acc + bias)), e0 shaped like out
 *   With epilogues 1 and 2 no z|r / q pre-activation tensor reaches HBM; same arithmetic as dkt_gru_gate_zr/_out.
 *   in_norm, stats_ws / stats_part, dscale: see the fields.
 * Errors, before any device is touched: a null descriptor, w_hi, w_lo, out, source or operand of the epilogue, or a source
 * with src_channels <= 0, DKT_E_NULL; nsrc outside 1..DKT_CONV_MAX_SRC, B, H, W or Cout <= 0, B > 65535, or a scale that
 * is not > 0 DKT_E_SHAPE; KH != KW, KH not in {1, 3}, passes outside 1..3, an epilogue outside 0..3, a stride outside
 * {0, 1, 2}, or a combination of options named above or at a field as unsupported DKT_E_UNSUPPORTED.
 *
 * dkt_conv2d_f16s_pair: two independent stride-1 convolutions (epilogues 0..3, no in_norm / stats / dscale) in ONE
 * launch: the resident blocks of the persistent kernel are split between the two problems in proportion to
 * their work.  Used to fold the coarsest GRU of iteration i+1 (36 tiles at 1/16 KITTI) into the launches of
 * the finest GRU of iteration i (core/update.py:118-127; the two are independent), where it fits in the
 * tile-quantisation slack.  Both problems must have the same KH and fall in the same output-width class
 * (<= 32, <= 64, <= 128, wider), else DKT_E_UNSUPPORTED. */
typedef struct dkt_conv_desc {
    const float *src[DKT_CONV_MAX_SRC];
    long src_bstride[DKT_CONV_MAX_SRC];
    int src_channels[DKT_CONV_MAX_SRC];
    int nsrc;
    const void *w_hi, *w_lo;
    const float *bias;
    float out_scale, in_scale;
    float *out;
    long out_bstride;
    int B, H, W, Cout, KH, KW, relu;
    int epilogue;
    const float *e0; long e0_bstride;
    const float *e1; long e1_bstride;
    const float *h;  long h_bstride;
    float *out2;     long out2_bstride;
    const float *in_norm;   /* optional, dkt_conv2d_f16s_desc only: (B*src_channels[0], 2) = (mean, 1/std) per input
                             * plane; the layer convolves relu((x - mean) * invstd) instead of x (nsrc = 1, 3x3,
                             * 32 < Cout <= 128).  NULL: plain input. */
    int stride;             /* 0 / 1 = stride 1; 2 = stride 2, dkt_conv2d_f16s_desc only */
    float *stats_ws;        /* optional, dkt_conv2d_f16s_desc with epilogue 0: scratch of dkt_conv2d_stats_ws_floats floats; */
    void *stats_part;       /* ... the instance-norm statistics of the OUTPUT (InstanceNorm2d of core/extractor.py:21-33 over
                             * this layer's result) are accumulated in the epilogue and left in stats_part, a
                             * dkt_instance_norm_workspace(B*Cout, Ho*Wo) buffer in the format dkt_instance_norm_stats writes
                             * (dkt_instance_norm_finalize / _add_relu read it): the statistics pass disappears */
    const float *dscale;    /* optional, dkt_conv2d_f16s_desc only: the activation scale in DEVICE memory -- the input-gradient
                             * convolution, whose operand range only the device knows.  {s, 1/s} as dkt_conv_grad_prepass
                             * writes it: the kernel reads in_scale = dscale[0] and multiplies out_scale, here w_inv_scale =
                             * 1 / the weight scale of the pack, by dscale[1] (the field in_scale is not read, but must be
                             * > 0).  A gradient of any magnitude keeps the ~22 bits of the split, and a power-of-two
                             * multiple of the operand gives that multiple of the result bit for bit.  Stride 1, epilogue 0,
                             * no bias, ReLU, in_norm or statistics: DKT_E_UNSUPPORTED with any of them. */
} dkt_conv_desc;
long dkt_conv2d_stats_ws_floats(int B, int Cout, int Ho, int Wo);
int dkt_conv2d_f16s_pair(const dkt_conv_desc *p0, const dkt_conv_desc *p1, int passes, int device, void *stream);
int dkt_conv2d_f16s_desc(const dkt_conv_desc *p, int passes, int device, void *stream);

/* Which kernel and tile shape a dkt_conv2d_f16s_desc / _pair call of these sizes runs on (core/update.py:9-10, 19-21, 72-76, 111-113;
 * core/extractor.py:16,34): the answer of the function every launch asks (csrc/conv_tile.h), for the tests -- no device is
 * touched and no tensor pointer read.  KS the filter size (1 or 3), stride 1 or 2, H, W the INPUT size, epilogue as in
 * dkt_conv_desc, form: 0 = one problem, 1 = the first problem of dkt_conv2d_f16s_pair, 2 = with in_norm,
 * 3 = descriptor with `dscale`.  DKT_CONV_WS is read per call, as by a launch.
 *   tile[8] = {kernel (0 = conv2d_f16s_kernel, 1 = the weights-stationary 64 -> 64 kernel), KS, WM, WN, NF, MF, ST, CK}:
 *   WM x WN waves along (channels, rows), each 32*MF channels x NF rows x 32 columns, stride ST, 16*CK-channel chunks.  KS
 *   and ST are what the kernel runs at: a 1x1 stride-2 layer reports ST = 1 (a stride-1 layer on a sub-sampled source).
 * Returns DKT_OK, or the code the launch of such a call returns (tile is left alone); tile or src_channels null DKT_E_NULL. */
int dkt_conv2d_f16s_tile(int KS, int stride, int passes, int Cout, const int *src_channels, int nsrc, int epilogue,
                         int B, int H, int W, int form, int *tile /* int[8] */);

/* The 7x7 stems (Cin <= 4, stride 1, padding 3: core/update.py:75, igev_stereo/update.py:81,
 * core/extractor.py:136) on the fp16 matrix cores with split operands (stem7.hip): K laid out
 * over (dy, dx, ci) instead of 32-channel chunks.  Weights are pre-packed once per layer
 * (dkt_conv2d_stem7_pack, `scale` a power of two as for dkt_conv2d_pack_weights);
 * out = conv * out_scale + bias [ReLU].  Same fp32-class accuracy as dkt_conv2d_f16s_desc(passes = 3). */
long dkt_conv2d_stem7_packed_elems(int Cout);
int dkt_conv2d_stem7_pack(const float *w, int Cout, int Cin, float scale, void *w_hi, void *w_lo,
                          int device, void *stream);
int dkt_conv2d_stem7(const float *x, long x_bstride, const void *w_hi, const void *w_lo,
                     const float *bias, float out_scale, float in_scale, float *y, long y_bstride,
                     int B, int Cin, int Cout, int H, int W, int relu, int device, void *stream);

/* Direct exact-fp32 convolution (stride 1, "same" padding) for the two extreme shapes of the
 * update block: 3x3 with Cout <= 4 (flow_head.conv2 / disp_head.conv2, core/update.py:10) and
 * 7x7 with Cin <= 4 (convf1 / convd1, core/update.py:75).  w: (Cout,Cin,K,K); optional ReLU. */
int dkt_conv2d_direct(const float *x, long x_bstride, const float *w, const float *bias,
                      float *y, long y_bstride, int B, int Cin, int Cout, int H, int W,
                      int KH, int KW, int relu, int device, void *stream);
/* The 3x3 few-output form with y += conv(x) + bias: the disparity update of the refinement loop
 * (raft_stereo.py:165-168: coords1 = coords1 + delta_flow; igev_stereo.py:209) in the head layer's epilogue. */
int dkt_conv2d_direct_accumulate(const float *x, long x_bstride, const float *w, const float *bias,
                                 float *y, long y_bstride, int B, int Cin, int Cout, int H, int W,
                                 int KH, int KW, int device, void *stream);
/* ... and diff_out = y_new - diff_ref on top (planes shaped like y): the flow operand of the next iteration's motion
 * encoder, flow = coords1 - coords0 (raft_stereo.py:147), written by the same epilogue. */
int dkt_conv2d_direct_accumulate_diff(const float *x, long x_bstride, const float *w, const float *bias,
                                      float *y, long y_bstride, const float *diff_ref, long diff_ref_bstride,
                                      float *diff_out, long diff_out_bstride, int B, int Cin, int Cout,
                                      int H, int W, int KH, int KW, int device, void *stream);

/* ---- streaming helpers around the convolutions ---------------------------------------- */

/* pool2x / interp of the update block (core/update.py:87-95): avg_pool2d(x, 3, stride=2,
 * padding=1) and F.interpolate(x, (Ho,Wo), mode="bilinear", align_corners=True) on
 * `planes` = B*C contiguous H x W planes. */
int dkt_pool2x(const float *x, float *y, long planes, int H, int W, int device, void *stream);
int dkt_interp_bilinear(const float *x, float *y, long planes, int H, int W, int Ho, int Wo,
                        int device, void *stream);

/* Their gradients on the training path (torch autograd through core/update.py:87-96), `planes` contiguous planes,
 * one owner thread per input element, no atomics: bit-identical from run to run.
 *   dkt_pool2x_bwd: gy (planes,Ho,Wo) with Ho = (H-1)/2+1, Wo = (W-1)/2+1 -> gx (planes,H,W);
 *     gx[iy,ix] = sum of fl(gy[oy,ox]/9) over the windows that hold (iy,ix) (|2 oy - iy| <= 1, |2 ox - ix| <= 1: at
 *     most 4), in ascending (oy,ox).
 *   dkt_interp_bilinear_bwd: gy (planes,Ho,Wo) -> gx (planes,H,W); gx[iy,ix] = sum gy[oy,ox]*wy*wx with the forward's own
 *     fp32 weights (fy = fl(sy*oy), y0 = (int)fy, y1 = y0 + (y0 < H-1), ly1 = fl(fy - y0), ly0 = fl(1 - ly1): row oy
 *     gives ly0 to y0 and ly1 to y1; columns alike), each term fl(fl(wy*wx)*gy), in ascending (oy, tap, ox, tap).  An
 *     input element no output reads gets 0.
 * Errors: null pointer DKT_E_NULL; a size <= 0 DKT_E_SHAPE; H*W or Ho*Wo beyond int, Ho or Wo > 2^22 DKT_E_UNSUPPORTED. */
int dkt_pool2x_bwd(const float *gy, float *gx, long planes, int H, int W, int device, void *stream);
int dkt_interp_bilinear_bwd(const float *gy, float *gx, long planes, int H, int W, int Ho, int Wo,
                            int device, void *stream);

/* Encoder glue (core/extractor.py:47-60,176-178; not on the scoped hot path, but inside the
 * timed forward): InstanceNorm2d(affine=False) with optional fused ReLU over `planes` = N*C
 * planes of HW elements (workspace: dkt_instance_norm_workspace() bytes, device memory), and
 * the residual join relu(a + b). */
long dkt_instance_norm_workspace(int planes, long HW);
int dkt_instance_norm(const float *x, float *y, void *workspace, int planes, long HW,
                      float eps, int relu, int device, void *stream);
/* dkt_instance_norm split in two, and the residual-block tail fused (core/extractor.py:52-60):
 * y = relu(a + relu(instance_norm(c))) with the statistics of c from dkt_instance_norm_stats
 * (same workspace, same planes / HW). */
int dkt_instance_norm_stats(const float *x, void *workspace, int planes, long HW, int device, void *stream);
int dkt_instance_norm_add_relu(const float *a, const float *c, float *y, const void *workspace,
                               int planes, long HW, float eps, int device, void *stream);
/* dkt_instance_norm_add_relu whose residual operand `a` is itself still un-normalised (the stem output in front of
 * the first residual block, core/extractor.py:176-178; the projection of a down-sampling block, :36-38):
 * y = relu(a' + relu(instance_norm(c))),  a' = [relu]((a - mean_a) * invstd_a)  with (mean_a, invstd_a) per plane from
 * dkt_instance_norm_finalize -- the normalise pass over `a` is never run. */
int dkt_instance_norm_add_relu_lazy(const float *a, const float *a_mean_invstd /* (planes,2) */, int a_relu,
                                    const float *c, float *y, const void *workspace, int planes, long HW, float eps,
                                    int device, void *stream);
/* The statistics of dkt_instance_norm_stats as (mean, 1/sqrt(var + eps)) float pairs, one per plane: the
 * `in_norm` operand of dkt_conv2d_f16s_desc, which folds relu(instance_norm(x)) between the two 3x3 layers
 * of a residual block (core/extractor.py:46-50) into the second layer's staging. */
int dkt_instance_norm_finalize(const void *workspace, int planes, long HW, float eps, float *mean_invstd /* (planes,2) */,
                               int device, void *stream);

/* Their gradients on the training path (torch autograd through core/extractor.py:21-33 with norm_fn='instance' -- the
 * batch-norm backward behind F.instance_norm plus the threshold backward of the ReLU -- and through the tail of a
 * residual block, core/extractor.py:52-60: two threshold backwards, the add and the norm's backward).  `planes`
 * contiguous planes of HW floats; mean_invstd (planes,2) from dkt_instance_norm_finalize on the forward's workspace.
 * yh = (x - mean) * invstd is recomputed (the forward's own pre-ReLU bits), g is the masked upstream gradient:
 *   dkt_instance_norm_bwd:           g = gy * [yh > 0] (relu) or gy;     gx = invstd * (g - mean(g) - yh * mean(g * yh))
 *   dkt_instance_norm_add_relu_bwd:  ga = gout * [out > 0];  g = ga * [yh_c > 0];  gc as gx above, from c
 * The plane sums are fp64, taken by several blocks per plane into `workspace` (dkt_instance_norm_bwd_workspace() bytes,
 * device memory) and added in slice order: no atomics, bit-identical from run to run.  Two launches; ga or gc may be
 * NULL (not both), and with gc == NULL no sums are taken, one launch runs and c, mean_invstd and workspace are not read.
 * Errors: null pointer DKT_E_NULL; planes <= 0, HW <= 0 or planes > 65535 DKT_E_SHAPE. */
long dkt_instance_norm_bwd_workspace(int planes, long HW);
int dkt_instance_norm_bwd(const float *gy, const float *x, const float *mean_invstd /* (planes,2) */, int relu, float *gx,
                          void *workspace, int planes, long HW, int device, void *stream);
int dkt_instance_norm_add_relu_bwd(const float *gout, const float *out, const float *c,
                                   const float *mean_invstd /* (planes,2) */, float *ga /* nullable */,
                                   float *gc /* nullable */, void *workspace, int planes, long HW, int device, void *stream);

int dkt_add_relu(const float *a, const float *b, float *y, long n, int device, void *stream);

/* ---- EMA teacher update (csrc/ema.hip) ----------------------------------------------------------------------
 * Replaces the loop of tools/ft_dkt.py:179-181,
 *     t_params.data = (ema_decay * t_params.data + (1 - ema_decay) * s_params.data)
 * for `count` tensors in ONE launch: t[i][j] = fl(fl(decay * t[i][j]) + fl(one_minus_decay * s[i][j])), two fp32
 * roundings, bit-identical to torch's evaluation of the expression (Python forms 1 - ema_decay in double; torch rounds
 * both scalars to fp32).  t, s: DEVICE tables of `count` tensor pointers (fp32, dense); n: DEVICE table of count + 1
 * exclusive prefix offsets (n[0] = 0, n[i+1] - n[i] = numel of tensor i, may be 0).  absmax (may be null): `count`
 * floats, max |t_new| per tensor (0 for an empty tensor), deterministic.  count = 0 is a no-op.  Errors: count < 0
 * DKT_E_SHAPE, a table null DKT_E_NULL, a non-finite decay DKT_E_UNSUPPORTED. */
int dkt_ema_update(float *const *t, const float *const *s, const long *n, int count, float decay, float one_minus_decay,
                   float *absmax, int device, void *stream);

/* ---- AdamW step with gradient clipping and loss-scale handling (csrc/optim.hip) --------------------------------
 * Replaces tools/ft_dkt.py:243-246 for the optimizer of :58 (AdamW, eps 1e-8),
 *     scaler.unscale_(optimizer); torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0); scaler.step(optimizer)
 * for `count` tensors in at most three launches and without a host read.  p, g, exp_avg, exp_avg_sq: DEVICE tables of
 * `count` tensor pointers (fp32, dense); n: DEVICE table of count + 1 exclusive prefix offsets as in dkt_ema_update;
 * total = n[count], the host's copy (it sizes the grid and the workspace).  lr, beta1, beta2, eps, weight_decay by value on
 * every call; max_norm < 0 = no clipping, +inf = take and report the norm without clipping (clip_grad_norm_'s own reading).  inv_scale (host) and *grad_scale (device, may be null) give the factor
 * inv = inv_scale / *grad_scale applied to every gradient; *found_inf (device, may be null) != 0 skips the step, and so does
 * any inf or nan in g.  step: DEVICE fp32 scalar, the number of steps taken, incremented unless the step is skipped.
 * record: 4 DEVICE floats {total_norm (of g * inv), clip = min(1, max_norm / (total_norm + 1e-6)), skipped (0 / 1), inv}.
 * A skipped step writes no parameter and no moment.  g is never written.  absmax (may be null): `count` floats, max |p_new|
 * per tensor (of the unchanged p on a skipped step; 0 for an empty tensor).  workspace: dkt_adamw_workspace(count, total)
 * bytes of device memory, 8-byte aligned, ZEROED before its first use; every call leaves it ready for the next.  grid: 0, or
 * a block count that overrides the library's (tests: the results do not depend on it).  With max_norm < 0, inv_scale == 1
 * and grad_scale == found_inf == null the call is ONE launch and record is {-1, 1, 0, 1}.  The rounding sequence is in
 * csrc/optim.hip; every output is bit-identical from run to run.  count = 0 is a no-op.
 * Errors, before any device is touched: count, total or grid < 0 DKT_E_SHAPE; a non-finite lr, beta, eps, weight_decay
 * or inv_scale, a nan max_norm, a beta outside [0, 1), a negative lr, eps or weight_decay DKT_E_UNSUPPORTED; a table, step, record
 * or workspace null DKT_E_NULL.  dkt_adamw_workspace: 64 + 8 * ceil(total / 2048), or -1 for a negative argument. */
long dkt_adamw_workspace(int count, long total);
int dkt_adamw_step(float *const *p, const float *const *g, float *const *exp_avg, float *const *exp_avg_sq, const long *n,
                   int count, long total, double lr, double beta1, double beta2, double eps, double weight_decay,
                   double max_norm, float inv_scale, const float *grad_scale, const float *found_inf, float *step,
                   float *record, float *absmax, void *workspace, int grid, int device, void *stream);

/* ---- round 3: the 3x3 convolution on pre-split activations ("C8S" layout, conv_c8.hip) -------------------------
 * Same operator and arithmetic as dkt_conv2d_f16s_desc(passes = 3) -- core/update.py:19-21,27-31 (ConvGRU), :72-76,84
 * (motion encoder), :9 (FlowHead.conv1) -- but the activation operands arrive as fp16 (hi, lo) pairs written by the
 * producing kernel, so that both operands reach LDS by DMA.
 *
 * C8S tensor of C channels at H x W:  [B][G = 2*ceil(C/16)][2: hi, lo][Hp][Wp][8] fp16 with
 * Hp = roundup(H, 8) + 2, Wp = roundup(W, 32) + 2 (dkt_act_c8_dims); pixel (y, x) lives at (y+1, x+1); the border and the
 * padding channels MUST be zero (allocate zeroed; producers write the interior only).  value = (hi + lo) / scale. */
int dkt_act_c8_dims(int H, int W, int *Hp, int *Wp);
/* fp32 NCHW (B,C,H,W) -> channels [ch0, ch0+C) of a C8S tensor (ch0 a multiple of 8), and back (tests, glue). */
int dkt_act_c8_pack(const float *x, long x_bstride, void *dst, long dst_bstride_bytes, int B, int C, int H, int W,
                    int ch0, float scale, int device, void *stream);
int dkt_act_c8_unpack(const void *src, long src_bstride_bytes, float *y, long y_bstride, int B, int C, int H, int W,
                      int ch0, float scale, int device, void *stream);
/* weights (Cout, sum(src_channels), 3, 3) fp32 -> the kernel's step images [chunk][tap][co/64][hi|lo][k/8][64][8] fp16
 * (every source padded to a multiple of 16 channels, Cout to 64) followed by 12 KB of slack the kernel may read (zero it);
 * `scale` a power of two as for dkt_conv2d_pack_weights. */
long dkt_conv_c8_packed_bytes(const int *src_channels, int nsrc, int Cout);
int dkt_conv_c8_pack_weights(const float *w, const int *src_channels, int nsrc, int Cout, float scale,
                             void *packed, int device, void *stream);
typedef struct dkt_conv_c8_desc {
    const void *src[DKT_CONV_MAX_SRC];      /* C8S operands = the reference's torch.cat list, all H x W */
    long src_bstride[DKT_CONV_MAX_SRC];     /* bytes per batch item */
    int src_channels[DKT_CONV_MAX_SRC];
    int nsrc;
    const void *w;                          /* dkt_conv_c8_pack_weights image */
    const float *bias;
    float out_scale;                        /* 1 / (weight scale * activation scale of the sources) */
    float act_scale;                        /* power of two applied to C8S OUTPUTS before the split */
    int B, H, W, Cout, relu;
    int epilogue;                           /* 0 plain, 1 ConvGRU z|r gates, 2 ConvGRU state update (as dkt_conv_desc),
                                             * 3 flow / disparity head (core/update.py:6-14): relu(conv1(x)) is reduced against conv2's
                                             *   weights per tap instead of being written (cfg 1 or 2); finish with dkt_head_finish
                                             * 4 residual join of a residual block whose norm is folded into the weights
                                             *   (core/extractor.py:52-60): relu(e0 + [relu](conv + bias)), Cout % 4 == 0 */
    float *out; long out_bstride;           /* fp32 NCHW destination (optional when out_c8 is given; epilogue 1: z) */
    void *out_c8; long out_c8_bstride;      /* C8S destination (optional), bytes per batch item; epilogue 2: h' */
    int out_c8_ch0;                         /* first channel written (multiple of 8) */
    const float *e0; long e0_bstride;       /* cz | cq */
    const float *e1; long e1_bstride;       /* cr | z  */
    const float *h;  long h_bstride;
    float *out2; long out2_bstride;         /* epilogue 1: r*h as fp32 NCHW (optional) */
    void *out2_c8; long out2_c8_bstride;    /* epilogue 1: r*h as C8S (optional; same H, W) */
    int out2_c8_ch0;
    const float *tail; long tail_bstride;   /* epilogue 0 + out_c8: channels Cout .. Cout+tail_channels-1 of the C8S output are */
    int tail_channels;                      /* copied from this fp32 NCHW tensor: torch.cat([out, flow]) of core/update.py:85 */
    const float *head_w;                    /* epilogue 3: weights of the head's SECOND 3x3 layer, [outputs][Cout][12] (9 taps + pad) */
    float *head_out; long head_out_bstride; /*   planes [B][(output * blocks + block) * 9 + tap][H][W], blocks = dkt_conv2d_c8_head_blocks */
    int head_outputs;                       /*   1 (stereo: x only / disparity) or 2 */
    int f32_c4;                             /* 1: out, out2, e0, e1, h are "C4" tensors [B][ceil(C/4)][H][W][4] (one 16-byte access per
                                             * lane and channel quad in the epilogue) instead of NCHW; bstrides stay in floats */
    float tail_scale;                       /* power of two applied to the `tail` channels of the C8S output instead of act_scale
                                             * (0 = act_scale): flow / disparity values next to features of another magnitude */
    int passes;                             /* round 5: fp16 MFMA products per weight x activation block. 0 / 3 = w_hi x_hi + w_lo x_hi +
                                             * w_hi x_lo (fp32-class, the parity path); 2 = without w_hi x_lo (activations rounded to
                                             * fp16); 1 = w_hi x_hi only.  Reduced passes serve the precision schedules of the
                                             * refinement loop (the reference's own switch: raft_stereo.py:95,156 `mixed_precision`);
                                             * tile shapes 1..4 */
} dkt_conv_c8_desc;
/* cfg: 0 = tile shape by layer / image size, 1..5 force one (conv_c8.hip c8_dispatch). */
int dkt_conv2d_c8(const dkt_conv_c8_desc *d, int cfg, int device, void *stream);
/* FlowHead.conv2 from epilogue 3's planes, added to `target` (raft_stereo.py:165-168), optionally diff_out = target - diff_ref */
int dkt_conv2d_c8_head_blocks(int Cout, int cfg);
int dkt_head_finish(const float *planes, long planes_bstride, int n_co, const float *bias, float *target,
                    long target_bstride, const float *diff_ref, long diff_ref_bstride, float *diff_out,
                    long diff_out_bstride, int B, int nout, int H, int W, int device, void *stream);
/* two independent convolutions in one launch (the coarsest GRU rides with the finest); cfg != 0 */
int dkt_conv2d_c8_pair(const dkt_conv_c8_desc *d0, const dkt_conv_c8_desc *d1, int cfg, int device, void *stream);

/* Round 4: one whole ConvGRU step (core/update.py:23-32 == meta_arch/igev_stereo/update.py:32-41) in ONE launch on C8S
 * operands (csrc/gru_c8.hip):
 *     z = sigmoid(convz([h, x]) + cz);  r = sigmoid(convr([h, x]) + cr);
 *     q = tanh(convq([r*h, x]) + cq);   h <- (1 - z) h + z q          (fp32 NCHW `h` and its C8S twin `h_c8`, both in place)
 * z never leaves the registers; r*h goes through the C8S scratch `rh_c8`; the q convolution of a tile waits for the
 * flags of its 3x3 neighbour tiles instead of a kernel boundary.  hidden must be 128.
 *   w_zr : dkt_conv_c8_pack_weights image of the 256-output layer whose output channel 64*k + 32*m + i is
 *          (m == 0 ? convz : convr) channel 32*k + i, input channels in the reference's order [h | x...];
 *   w_q  : image of convq with its input channels REORDERED to [x... | r*h] (the x chunks are consumed first);
 *   bz, br, bq : the three biases in the reference's channel order;  scale_* : 1 / (weight scale * activation scale);
 *   flags : dkt_gru_c8_flag_words(B, H, W) zero-initialised 32-bit words owned by this (operator, shape) pair -- every
 *           launch increments them, they must not be shared with a launch of another shape or written by the caller;
 *   err_word (optional, device memory): bit 0 (value 1) is OR-ed in if a neighbour wait timed out (results are then invalid).
 * DKT_E_UNSUPPORTED when the device cannot hold the launch's tiles the way the flags need (fall back to two
 * dkt_conv2d_c8 launches with epilogues 1 and 2). */
typedef struct dkt_gru_c8_desc {
    void *h_c8; long h_c8_bstride;              /* C8S hidden state (hidden channels), bytes per batch item */
    const void *x[3]; long x_bstride[3]; int x_channels[3]; int nx;   /* the reference's x_list as C8S tensors */
    void *rh_c8; long rh_c8_bstride;            /* C8S scratch for r*h (zero border, as every C8S tensor) */
    const void *w_zr, *w_q;
    const float *bz, *br, *bq;
    const float *cz, *cr, *cq; long cz_bstride, cr_bstride, cq_bstride;   /* context terms, fp32 NCHW, strides in floats */
    float *h; long h_bstride;                   /* fp32 NCHW hidden state */
    float scale_zr, scale_q, act_scale;
    int B, H, W, hidden;
    unsigned *flags;
    int passes;                                 /* as dkt_conv_c8_desc.passes (0 / 3, 2, 1); both steps of a pair launch alike */
} dkt_gru_c8_desc;
long dkt_gru_c8_flag_words(int B, int H, int W);
int dkt_gru_c8(const dkt_gru_c8_desc *d, unsigned *err_word, int device, void *stream);
/* two independent ConvGRU steps (the finest level and the coarsest one of the next iteration) in one launch */
int dkt_gru_c8_pair(const dkt_gru_c8_desc *d0, const dkt_gru_c8_desc *d1, unsigned *err_word, int device, void *stream);

/* Producers of C8S operands besides the convolution epilogues (same arithmetic as their fp32 twins):
 *   dkt_pool2x_c8 / dkt_interp_c8 : pool2x / interp of core/update.py:87-95, fp32 NCHW in (B,C,H,W);
 *   dkt_conv2d_stem7_c8           : the 7x7 stem (convf1, core/update.py:75);
 *   dkt_corr1d_lookup_conv1x1_c8  : lookup fused with convc1 (core/corr.py:127-146 + core/update.py:76), L = 4 only.
 * ch0 (multiple of 8) = first channel written, act_scale the C8S tensor's power-of-two scale. */
int dkt_pool2x_c8(const float *x, long x_bstride, void *dst, long dst_bstride_bytes, int B, int C, int H, int W,
                  int ch0, float scale, int device, void *stream);
int dkt_interp_c8(const float *x, long x_bstride, void *dst, long dst_bstride_bytes, int B, int C, int H, int W,
                  int Ho, int Wo, int ch0, float scale, int device, void *stream);
/* The motion encoder's front as one launch (round 4): the coordinate update that closes the flow head (what dkt_head_finish
 * does: coords1[:, 0] += conv2(relu(conv1(h)))[:, 0], flow[:, 0] = coords1[:, 0] - coords0[:, 0]; raft_stereo.py:165-168),
 * dkt_corr1d_lookup_conv1x1_c8 at the NEW coordinate (core/corr.py:127-146 + core/update.py:76,84) and dkt_conv2d_stem7_c8 on
 * the NEW flow (core/update.py:77,85).  x_new must be another buffer than x_old (the caller alternates two).  Same arithmetic,
 * bit for bit, as the three launches.  L = 4, r = 3 or 4, cor_channels <= 64. */
typedef struct dkt_motion_front_desc {
    const float *const *skew;                   /* dkt_corr1d_skew pyramids (L pointers) */
    const float *planes; long planes_bstride; int n_co;   /* epilogue-3 planes of the head's first layer, (B, n_co*9, H, W1) */
    const float *head_bias;                     /* bias of the head's second layer (first output) or null */
    const float *x_old; long x_old_bstride;     /* coords1[:, 0] in */
    float *x_new; long x_new_bstride;           /* coords1[:, 0] out */
    const float *x0; long x0_bstride;           /* coords0[:, 0] */
    float *flow; long flow_bstride;             /* (B, stem_cin, H, W1): channel 0 written, the others read */
    const float *w_cor, *b_cor; int cor_channels;   /* convc1: weight k-major (L*K, cor_channels), bias or null */
    void *cor_c8; long cor_c8_bstride_bytes; int cor_c8_ch0; float cor_act_scale;
    const void *stem_w_hi, *stem_w_lo; const float *stem_bias;   /* dkt_conv2d_stem7_pack images of convf1 */
    float stem_out_scale, stem_in_scale; int stem_cin, stem_cout;
    void *flo_c8; long flo_c8_bstride_bytes; int flo_c8_ch0; float flo_act_scale;
    int B, H, W1, W2, L, r;
} dkt_motion_front_desc;
int dkt_motion_front_c8(const dkt_motion_front_desc *d, int device, void *stream);
/* two of the resampling jobs above in one launch (round 4: the loop's pool2x(net[0]) | interp(net[2]) in front of the
 * middle ConvGRU and interp(net[1]) | pool2x(net[1]) behind it, core/update.py:120-132); kind 0 = pool2x (Ho, Wo ignored),
 * kind 1 = interp to (Ho, Wo).  Same arithmetic as the single launches. */
typedef struct dkt_resample_c8_job {
    const float *x; long x_bstride;             /* fp32 NCHW source (B, C, H, W), batch stride in floats */
    void *dst; long dst_bstride_bytes;          /* C8S destination */
    int B, C, H, W, Ho, Wo, ch0, kind;
    float scale;                                /* the destination's power-of-two scale */
} dkt_resample_c8_job;
int dkt_resample_pair_c8(const dkt_resample_c8_job *job0, const dkt_resample_c8_job *job1, int device, void *stream);
int dkt_conv2d_stem7_c8(const float *x, long x_bstride, const void *w_hi, const void *w_lo,
                        const float *bias, float out_scale, float in_scale, void *y_c8, long y_c8_bstride_bytes,
                        int y_c8_ch0, float act_scale, int B, int Cin, int Cout, int H, int W, int relu,
                        int device, void *stream);
/* the same stem writing fp32 NCHW and C8S at once (the encoders' first layer: the fp32 copy is the residual operand of
 * layer1, core/extractor.py:167-171) */
int dkt_conv2d_stem7_dual(const float *x, long x_bstride, const void *w_hi, const void *w_lo,
                          const float *bias, float out_scale, float in_scale, float *y, long y_bstride,
                          void *y_c8, long y_c8_bstride_bytes, int y_c8_ch0, float act_scale,
                          int B, int Cin, int Cout, int H, int W, int relu, int device, void *stream);
/* Instance-norm glue of the feature encoder (core/extractor.py:21-60 with norm_fn='instance') producing C8S operands:
 *   t = (c - mean_c) * invstd_c;  if c_relu: t = relu(t);
 *   if a:  t = relu(a' + t),  a' = a or [relu]((a - mean_a) * invstd_a) when a_mean_invstd is given
 * c, a: fp32 NCHW (B, C, H, W), dense per batch item; *_mean_invstd: (B*C, 2) from dkt_instance_norm_finalize.
 * Writes y (fp32 NCHW, optional) and / or channels [ch0, ch0+C) of the C8S tensor dst (optional).  Same arithmetic as
 * dkt_instance_norm / dkt_instance_norm_add_relu_lazy. */
int dkt_instance_norm_join_c8(const float *c, const float *c_mean_invstd, int c_relu,
                              const float *a, const float *a_mean_invstd, int a_relu,
                              float *y, void *dst, long dst_bstride_bytes, int ch0, float act_scale,
                              int B, int C, int H, int W, int device, void *stream);
/* Input normalisation of a stereo pair in one pass (meta_arch/raft_stereo/raft_stereo.py:91-92):
 * out[0:B] = 2*(image1/255) - 1, out[B:2B] = 2*(image2/255) - 1, out = (2B, C, H, W) dense -- the feature encoder's
 * concatenated batch (core/extractor.py:180-183).  image*_bstride / per_image in floats (per_image = C*H*W, dense per item). */
int dkt_normalize_pair(const float *image1, long image1_bstride, const float *image2, long image2_bstride,
                       float *out, int B, long per_image, int device, void *stream);
/* IGEV's geometry-encoding lookup (dkt_geo_lookup; meta_arch/igev_stereo/geometry.py:29-69) fused with the motion
 * encoder's 1x1 layer (convc1, igev_stereo/update.py:78,86): out[b, co] = [relu](bias[co] + sum_k weight_t[k][co] *
 * lookup[b, k]) -- the L*(2r+1)*(C+1)-channel lookup is never written.  weight_t: (L*(2r+1)*(C+1), Cout) k-major, k in the
 * lookup's channel order.  disp: (B,1,H,W) with batch stride disp_bstride (floats); coords: (B,H,W) dense.  Destinations:
 * out (fp32 NCHW) and / or out_c8 (C8S, first channel out_c8_ch0); tap (optional) receives the lookup itself, bit-identical
 * to dkt_geo_lookup.  Supported: L = 2, C = 8, r = 4, Cout <= 64; otherwise DKT_E_UNSUPPORTED. */
int dkt_geo_lookup_conv1x1(const float *const *geo_pyr, const float *const *init_pyr,
                           const float *disp, long disp_bstride, const float *coords,
                           const float *weight_t, const float *bias,
                           float *out, long out_bstride, void *out_c8, long out_c8_bstride_bytes, int out_c8_ch0,
                           float act_scale, float *tap, long tap_bstride,
                           int B, int C, int D, int H, int W, int W2, int L, int r, int Cout, int relu,
                           int device, void *stream);
int dkt_corr1d_lookup_conv1x1_c8(const float *const *skew, const float *coords_x, long coords_bstride,
                                 const float *weight, const float *bias, void *out_c8, long out_c8_bstride_bytes,
                                 int out_c8_ch0, float act_scale, int B, int H, int W1, int W2, int L, int r, int Cout,
                                 int relu, int device, void *stream);

/* ---- round 6: the post-conditions of one pair, in one launch ----------------------------------------------------------
 * The reference's forward (meta_arch/raft_stereo/raft_stereo.py:85-187, igev_stereo.py:192-210) is plain fp32 and needs no
 * check; this implementation equals it only while (i) nothing overflowed the split-fp16 operands, (ii) no fused ConvGRU
 * launch timed out on a neighbour flag (dkt_gru_c8: `err`), (iii) the C8S tensors that follow the input's magnitude
 * still sit in the window their scales were picked for.  dkt_loop_status gathers all three for the caller's ONE host read:
 *   status[0]         = *err_word (0 when err_word is NULL), as is: bit 0 = a fused ConvGRU launch timed out, the only bit
 *                       any kernel sets; the word is cleared (atomic exchange)
 *   status[1]         = 1 when finite_src[0 .. finite_n) holds an Inf or a NaN
 *   status[2 + 2 j]   = max over the body channels of C8S tensor j of the fp16 BIT PATTERN of |hi| (0x7c00 = Inf, above = NaN)
 *   status[3 + 2 j]   = the same over its `tail` trailing channels (0 when tail = 0)
 * status: 2 + 2 njobs words, zeroed by the call (stream-ordered).  njobs <= DKT_STATUS_MAX_JOBS. */
#define DKT_STATUS_MAX_JOBS 8
typedef struct dkt_c8_range_job {
    const void *t; long bstride_bytes;          /* C8S tensor (B, C channels, H x W) */
    int B, C, H, W;
    int tail;                                   /* trailing channels reported separately (their own scale) */
} dkt_c8_range_job;
int dkt_loop_status(const dkt_c8_range_job *jobs, int njobs, const float *finite_src, long finite_n, int *err_word,
                    unsigned *status, int device, void *stream);

/* ---- DKT Filter-and-Ensemble (csrc/fande.hip) ----------------------------------------------------------------------
 * Replaces FandE/__init__.py:4-39 (FandE_Ensemble, FandE_Filter) and the four calls of tools/ft_dkt.py:203-210 that
 * chain them.  One job = one disparity map (B,1,H,W) filtered against the EMA teacher's output and/or ensembled with it:
 *   filter = 0  Ensemble only (FandE/__init__.py:4-21): src ensembled against tgt under `valid`;
 *   filter = 1  Filter, withprob=False (:24-27,36-37), then Ensemble under the filtered mask when ensemble = 1;
 *   filter = 2  Filter, withprob=True (:24-35,38), same.  rand[b] = torch.rand((B,1))[b] drawn by the caller.
 * ens_prob = fl32(random.random()) of the Ensemble call; clamp != 0 applies torch.clamp(offset, max=clamp_max).
 * Every expression is evaluated in the reference's order with fp32 roundings: sqrt(d*d) < tau, products left to right,
 * direction in {+1,-1,0} (NaN -> 0), clamp propagates NaN.  The withprob ratio is fl32(sum vc) / fl32(sum valid) per image,
 * the sums formed in fp64 (exact for 0/1 masks).  valid = NULL means valid == 1 (the pseudo label's, never materialised).
 * out: AUG source (B,1,H,W); out_valid (filter != 0): the filtered mask (B,H,W).  All planes H x W contiguous, batch
 * strides in elements.  ws: DKT_FANDE_WS_DOUBLES_PER_IMAGE * B * njobs doubles (caller-allocated, only read back by the
 * same call).  Launches: one count pass when a job has filter = 2, then one apply pass for all jobs.
 * Errors: null jobs / a null pointer a job needs / null ws DKT_E_NULL; njobs outside 1..DKT_FANDE_MAX_JOBS, B, H or W <= 0
 * DKT_E_SHAPE; B > DKT_FANDE_MAX_B or an unknown filter mode DKT_E_UNSUPPORTED. */
#define DKT_FANDE_MAX_B 64
#define DKT_FANDE_MAX_JOBS 2
#define DKT_FANDE_WS_DOUBLES_PER_IMAGE 512
typedef struct dkt_fande_job {
    const float *src; long src_bstride;
    const float *tgt; long tgt_bstride;
    const float *valid; long valid_bstride;     /* NULL: valid == 1 */
    float *out; long out_bstride;
    float *out_valid; long out_valid_bstride;   /* filter != 0 */
    float tau;
    int filter, ensemble, clamp;
    float clamp_max, ens_prob;
    float rand[DKT_FANDE_MAX_B];
} dkt_fande_job;
int dkt_fande(const dkt_fande_job *jobs, int njobs, int B, int H, int W, double *ws, int device, void *stream);

/* ---- stereo sequence losses (csrc/stereo_loss.hip) -------------------------------------------------------------------
 * Replaces sequence_loss_raft (meta_arch/raft_stereo/loss.py:3-40) and loss_gwcnet (meta_arch/gwcnet/gwc_loss.py:5-31)
 * for one or two targets against the same predictions (tools/ft_dkt.py:227-228 calls the loss twice).
 * Per target k: mask = (valid >= 0.5) & (sqrt(gt*gt) < max_flow), written as bool (B,1,H,W) contiguous;
 *   kind DKT_LOSS_RAFT: mean_i = mean |p_i - gt| over the mask; kind DKT_LOSS_GWC: mean smooth-L1 (beta = 1);
 *   loss_k = sum_{i < n_loss} weight[i] * mean_i, accumulated in fp32 in order i = 0 .. n_loss-1 (weight[i] already fp32).
 * Sums are fp64 per-block partials reduced in a fixed order by a finalize launch: bit-identical from run to run, no atomics.
 * rec (DKT_LOSS_REC doubles), written by the finalize launch:
 *   rec[8k + 0] = number of mask pixels N_k   rec[8k + 1] = fl32 EPE mean of prediction n-1 over the mask
 *   rec[8k + 2..4] = fl32 fractions of EPE < 1, 3, 5   rec[8k + 5] = 1 when gt is +-Inf on a mask pixel (loss.py:17)
 *   rec[16] = 1 when some prediction holds a NaN and no Inf (loss.py:22, over the whole tensor)
 * pred[i]: (B,1,H,W) with H x W planes contiguous and batch stride pred_bstride[i] (views such as [:, :1] are read in
 * place).  gt, valid: (B,1,H,W) / (B,H,W) with batch strides.  ws: dkt_seq_loss_ws_doubles(ntargets, n, B, H, W) doubles.
 * Two launches (partials, finalize); no host synchronisation.
 * Errors: null desc / ws / a pointer the call needs DKT_E_NULL; B, H, W <= 0, n outside 1..DKT_LOSS_MAX_PRED, n_loss
 * outside 1..n or ntargets outside 1..2 DKT_E_SHAPE; an unknown kind DKT_E_UNSUPPORTED. */
#define DKT_LOSS_MAX_PRED 64
#define DKT_LOSS_RAFT 0
#define DKT_LOSS_GWC 1
#define DKT_LOSS_REC 24
typedef struct dkt_seq_loss_desc {
    const float *pred[DKT_LOSS_MAX_PRED];
    long pred_bstride[DKT_LOSS_MAX_PRED];
    float weight[DKT_LOSS_MAX_PRED];
    int n, n_loss, kind, ntargets;
    const float *gt[2]; long gt_bstride[2];
    const float *valid[2]; long valid_bstride[2];
    float max_flow;
    unsigned char *mask[2];                     /* out */
    float *loss[2];                             /* out, device scalars */
    double *rec;                                /* out */
    int B, H, W;
} dkt_seq_loss_desc;
long dkt_seq_loss_ws_doubles(int ntargets, int n, int B, int H, int W);
int dkt_seq_loss(const dkt_seq_loss_desc *d, double *ws, int device, void *stream);
/* Backward of dkt_seq_loss in ONE launch, after it on the same stream, reading its mask and rec on the device:
 *   grad[i] = sum_k [mask_k] * (RAFT: fl(fl(g_k * weight[i]) / N_k) * sgn(p_i - gt_k);
 *                               GWC:  smooth-L1 backward with norm fl32(1/N_k) and upstream fl(g_k * weight[i]))
 * and exactly 0 off every mask and for i >= n_loss.  g_k = *grad_loss[k] (device scalars).  grad[i]: (B,1,H,W)
 * contiguous.  Errors as dkt_seq_loss, plus a null grad pointer DKT_E_NULL. */
typedef struct dkt_seq_loss_grad {
    float *grad[DKT_LOSS_MAX_PRED];
    const float *grad_loss[2];
} dkt_seq_loss_grad;
int dkt_seq_loss_bwd(const dkt_seq_loss_desc *d, const dkt_seq_loss_grad *g, int device, void *stream);

/* ---- NeRF-supervised loss (csrc/ns_loss.hip) ---------------------------------------------------------------------------
 * Replaces ns_loss (meta_arch/nerf_stereo/loss.py:128-181) with everything it calls: disp_warp (:73-84, mesh_grid :38-44,
 * norm_grid :29-36), SSIM (:5-27), photometric_loss (:86-90) and trinocular_loss (:92-109), for n predictions.
 *   With target: conf' = conf * (target < 0); valid = (conf' > conf_threshold) & (sqrt(target^2) < max_flow), written to
 *   `valid` as bool (B,H,W); the photometric weight is 1 - conf'; disparity term mean_i = mean over valid of |p_i - target| conf'.
 *   Without target (null; trinocular_loss alone): conf is the weight as given, valid_in (B,H,W bytes, contiguous) the mask,
 *   there is no disparity term.
 *   Warp: view im[0] is sampled at x + d, im[2] at x - d (d = p_i, negative), grid_sample with align_corners=False after
 *   norm_grid's (W-1, H-1) normalisation: px = (x + s d) W/(W-1) - 0.5, py = y H/(H-1) - 0.5; border padding for the image,
 *   zero padding for the mask (a sampled plane of ones); reconstruction = mask * sample.
 *   p(view) = 0.15 mean_c |im[1] - rec| + 0.85 mean_c clamp((1 - SSIM(rec, im[1]))/2, 0, 1), SSIM over 7 x 7 windows of the
 *   ReflectionPad2d(3)-padded planes; loss_warp = min(p12, p23); loss_2 the same from the unwarped views;
 *   automask = (loss_warp < loss_2) & valid; photo_i = mean over automask of loss_warp * weight.
 *   loss = alpha_disp * sum_i weight[i] mean_i + alpha_photo * sum_i weight[i] photo_i, each sum accumulated in fp32 in order
 *   i (weight[i] already fp32); without target, loss = alpha_photo * sum_i weight[i] photo_i.  alpha_photo == 0 skips the
 *   photometric term (:164-167) and `state` may be null.  The mean of an empty set is NaN, as torch's is.
 * state: n x (B,H,W) bytes, out: bit 0 the automask, bit 1 set where the third view (im[2]) won the minimum.
 * planes: null, or (3,B,H,W) floats, out: p12, p23 and loss_2 of prediction 0 (the handle of the tests).
 * rec (DKT_NS_REC doubles), written by the finalize launch: rec[0] = number of valid pixels, rec[1] = fl32 EPE mean of
 * prediction n-1 over valid, rec[2..4] = fl32 fractions of EPE < 1, 3, 5, rec[5] = 1 when some prediction holds a NaN or an
 * Inf (:155), rec[6], rec[7] = the two weighted sums, rec[8 + i] = automask count of prediction i.
 * pred[i]: (B,1,H,W) with contiguous H x W planes and batch stride pred_bstride[i] (views such as [:, :1] are read in
 * place).  im[k]: (B,3,H,W), the three planes of an image contiguous.  conf, target: (B,H,W) with batch strides.
 * ws: dkt_ns_loss_workspace(B, H, W) bytes (block partials and the loss_2 plane; it does not depend on n), 8-byte aligned.
 * Forward: three launches (loss_2 and valid once; one tiled launch over (tile, image, prediction); finalize); backward: one
 * launch after it on the same stream, reading state and rec on the device.  fp64 partials in a fixed order, no atomics:
 * bit-identical from run to run.  No host synchronisation.
 *   grad[i] (B,1,H,W) contiguous: every element stored exactly once; g = *grad_loss (device scalar).
 * Errors (every entry, before any device call): a null desc / ws / pointer the call needs DKT_E_NULL; B, H, W <= 0, H or W
 * < 4 (ReflectionPad2d(3)), n outside 1..DKT_NS_MAX_PRED or a batch stride shorter than an image DKT_E_SHAPE; H*W > 2^31 - 257
 * or B*n > 65535 DKT_E_UNSUPPORTED; a float pointer that is not a multiple of 4 bytes, ws or rec of 8, DKT_E_ALIGN.
 * dkt_ns_loss_workspace returns DKT_E_SHAPE for B <= 0, H < 4 or W < 4. */
#define DKT_NS_MAX_PRED 64
#define DKT_NS_REC 72
typedef struct dkt_ns_loss_desc {
    const float *pred[DKT_NS_MAX_PRED];
    long pred_bstride[DKT_NS_MAX_PRED];
    float weight[DKT_NS_MAX_PRED];
    int n;
    const float *im[3]; long im_bstride[3];
    const float *conf; long conf_bstride;
    const float *target; long target_bstride;   /* or null */
    const unsigned char *valid_in;              /* with target == null */
    float conf_threshold, max_flow, alpha_disp, alpha_photo;
    unsigned char *valid;                       /* out, with target != null */
    unsigned char *state;                       /* out */
    float *planes;                              /* out, or null */
    float *loss;                                /* out, device scalar */
    double *rec;                                /* out */
    int B, H, W;
} dkt_ns_loss_desc;
typedef struct dkt_ns_loss_grad {
    float *grad[DKT_NS_MAX_PRED];
    const float *grad_loss;
} dkt_ns_loss_grad;
long dkt_ns_loss_workspace(int B, int H, int W);
int dkt_ns_loss(const dkt_ns_loss_desc *d, void *ws, int device, void *stream);
int dkt_ns_loss_bwd(const dkt_ns_loss_desc *d, const dkt_ns_loss_grad *g, int device, void *stream);

/* ---- PCVNet sequence loss (csrc/pcv_loss.hip) ---------------------------------------------------------------------------
 * Replaces sequence_loss_pcvnet (meta_arch/pcvnet/loss.py:4-73) for one or two targets against the same predictions
 * (tools/ft_dkt.py:227-228 calls the loss twice).  n predictions, each final_disp_i (B,1,H,W) and mu_i, w_i, sigma_i of M
 * gaussians; disp_refine (B,1,H,W).  Per target k:
 *   mask_k = (gt < max_disp) & (valid != 0) & (gt >= 0), written as bool (B,1,H,W) contiguous (valid NaN counts as set; a
 *   NaN or +-Inf gt is off the mask, so loss.py:17 cannot fire);  N_k = its count;
 *   mean1_i = mean over the mask of |fl32(disp_i - gt)|;  mean2_i = mean over the mask of fl32(fl32(sum_m |fl32(mu_i,m - gt)|) / M);
 *   sl1 = mean over the mask of smooth-L1 (beta = 1) of disp_refine - gt;
 *   loss_k = sum_{i < n_loss} weight[i] * (mean1_i + mean2_i) + refine_weight * sl1, accumulated in fp32 in that order
 *   (weight[i], refine_weight already fp32).  The mean of an empty set is NaN, as torch's is.
 * Sums are fp64 per-block partials reduced in a fixed order by a finalize launch: bit-identical from run to run, no atomics.
 * rec (DKT_PCV_LOSS_REC doubles), written by the finalize launch:
 *   rec[16k + 0] = N_k;  rec[16k + 1 .. 7] = of final_disp 3 over the mask (0 when n < 4): the fl32 EPE mean, then the fl32
 *   fractions of EPE < 1, < 3, < 5, > 1, > 2, > 5 (all strict, on |fl32(p - gt)|);  rec[16k + 8 .. 14] = the same of disp_refine;
 *   rec[32] = the flag word: bit i set when mu_i, w_i, sigma_i or final_disp_i holds a NaN or an Inf anywhere, on or off the
 *   mask (loss.py:30-33).  disp_refine has no flag: its NaN goes into the loss.
 * disp[i], refine, gt, valid: contiguous H x W planes with a batch stride; mu[i], w[i], sigma[i]: plane (b, m) at
 * b * bstride + m * gstride, so (B M,1,H,W), (B,M,1,H,W) and [:, :1] views are read in place.  w[i] / sigma[i] may be null:
 * that tensor is then not read (they enter through the finite check only).  ws: dkt_pcv_loss_partial_doubles(ntargets, B, H, W)
 * doubles.  Accesses are 16 bytes when H W % 4 == 0 and every pointer and stride allows it, scalar otherwise.
 * Two launches (partials, finalize); no host synchronisation.
 * Errors (every entry, before any device call): null desc / ws / a pointer the call needs DKT_E_NULL; B, H, W <= 0, n outside
 * 1..DKT_PCV_LOSS_MAX_PRED, n_loss outside 1..min(n, 6), M outside 1..DKT_PCV_LOSS_MAX_M or ntargets outside 1..2
 * DKT_E_SHAPE; H*W > 2^31 - 1025 or B > 65535 DKT_E_UNSUPPORTED.  dkt_pcv_loss_partial_doubles returns DKT_E_SHAPE for ntargets
 * outside 1..2 or B, H, W <= 0. */
#define DKT_PCV_LOSS_MAX_PRED 7
#define DKT_PCV_LOSS_MAX_M 8
#define DKT_PCV_LOSS_REC 40
typedef struct dkt_pcv_loss_desc {
    const float *disp[DKT_PCV_LOSS_MAX_PRED]; long disp_bstride[DKT_PCV_LOSS_MAX_PRED];
    const float *mu[DKT_PCV_LOSS_MAX_PRED]; long mu_bstride[DKT_PCV_LOSS_MAX_PRED], mu_gstride[DKT_PCV_LOSS_MAX_PRED];
    const float *w[DKT_PCV_LOSS_MAX_PRED]; long w_bstride[DKT_PCV_LOSS_MAX_PRED], w_gstride[DKT_PCV_LOSS_MAX_PRED];
    const float *sigma[DKT_PCV_LOSS_MAX_PRED]; long sigma_bstride[DKT_PCV_LOSS_MAX_PRED], sigma_gstride[DKT_PCV_LOSS_MAX_PRED];
    float weight[DKT_PCV_LOSS_MAX_PRED];
    const float *refine; long refine_bstride;
    float refine_weight;
    int n, n_loss, M, ntargets;
    const float *gt[2]; long gt_bstride[2];
    const float *valid[2]; long valid_bstride[2];
    float max_disp;
    unsigned char *mask[2];                     /* out */
    float *loss[2];                             /* out, device scalars */
    double *rec;                                /* out */
    int B, H, W;
} dkt_pcv_loss_desc;
long dkt_pcv_loss_partial_doubles(int ntargets, int B, int H, int W);
int dkt_pcv_loss(const dkt_pcv_loss_desc *d, double *ws, int device, void *stream);
/* Backward of dkt_pcv_loss in ONE launch, after it on the same stream, reading its masks and rec on the device.  On mask_k,
 * with g_k = *grad_loss[k] (device scalars) and q_i,k = fl(fl(g_k * weight[i]) / N_k):
 *   gdisp[i] = sum_k q_i,k * sgn(disp_i - gt_k)            gmu[i] = sum_k fl(q_i,k / M) * sgn(mu_i,m - gt_k)      (sgn(0) = 0)
 *   grefine  = sum_k smooth-L1 backward with norm fl32(1 / N_k) and upstream fl(g_k * refine_weight)
 * and exactly 0 off every mask and for i >= n_loss.  A target with N_k = 0 or a null grad_loss[k] contributes exactly 0.
 * gdisp[i], grefine: (B,1,H,W) contiguous; gmu[i]: (B,M,H,W) contiguous; a null one is not required and is skipped; every
 * element of the others is stored once.  w and sigma have no gradient.  Errors as dkt_pcv_loss, plus a null g DKT_E_NULL. */
typedef struct dkt_pcv_loss_grad {
    float *gdisp[DKT_PCV_LOSS_MAX_PRED];
    float *gmu[DKT_PCV_LOSS_MAX_PRED];
    float *grefine;
    const float *grad_loss[2];
} dkt_pcv_loss_grad;
int dkt_pcv_loss_bwd(const dkt_pcv_loss_desc *d, const dkt_pcv_loss_grad *g, int device, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DKTSTEREO_H */
