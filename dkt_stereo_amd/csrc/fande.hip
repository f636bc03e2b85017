// dkt_fande: DKT's Filter-and-Ensemble (FandE/__init__.py:4-39) for up to two disparity maps in at most two launches --
// the four calls of tools/ft_dkt.py:203-210 (GT: Filter withprob + Ensemble with clamp; PL: Filter + Ensemble).
//
// Pass 1 (only when a job filters withprob): per image, fp64 block partials of sum(valid_consistent) and sum(valid),
// grid (FANDE_NB blocks, B, njobs), each block striding over its image.
// Pass 2: every block first reduces its image's partials in a fixed order (so every block of an image forms the same
// ratio), then applies Filter then Ensemble per pixel.  No float atomics: the result does not depend on the schedule.
//
// Arithmetic (the library builds with -ffp-contract=off; division is __fdiv_rn and sqrt is sqrtf, which hipcc expands to the
// correctly rounded sequence -- __fsqrt_rn lowers to the bare v_sqrt_f32, which is not, and missed the reference by an ulp):
// each line below is one torch elementwise op of the reference, in its order, with its fp32 rounding.  Multiplications by
// a 0/1 mask are kept as multiplications: 0 * NaN = NaN and 0 * -x = -0 are what the reference computes.
#include "dkt_common.h"
#include "wave_reduce.h"

#include <math.h>

#define FANDE_THREADS 256
#define FANDE_NB 256      // count-pass blocks per image (x 2 doubles = DKT_FANDE_WS_DOUBLES_PER_IMAGE)

static_assert(FANDE_NB == FANDE_THREADS, "the apply pass reduces one partial per thread");
static_assert(FANDE_NB * 2 == DKT_FANDE_WS_DOUBLES_PER_IMAGE, "workspace size of include/dktstereo.h");

struct FandeArgs {
    dkt_fande_job job[DKT_FANDE_MAX_JOBS];
    int B, HW;
};

// sqrt(sum((target - source)**2, dim=1)) < threshold for one channel: pow(x, 2) is x * x, the sum of one term is the term
__device__ __forceinline__ float fande_consistent(float s, float t, float tau) {
    const float d = __fsub_rn(t, s);
    return sqrtf(__fmul_rn(d, d)) < tau ? 1.0f : 0.0f;
}

__global__ __launch_bounds__(FANDE_THREADS) void fande_count_kernel(FandeArgs a, double *__restrict__ ws) {
    __shared__ double red[FANDE_THREADS / 64];
    const dkt_fande_job &j = a.job[blockIdx.z];
    if (j.filter != 2) return;
    const int b = blockIdx.y;
    const float *src = j.src + (long)b * j.src_bstride;
    const float *tgt = j.tgt + (long)b * j.tgt_bstride;
    const float *val = j.valid ? j.valid + (long)b * j.valid_bstride : nullptr;
    double nvc = 0.0, nv = 0.0;
    for (int r = blockIdx.x * FANDE_THREADS + threadIdx.x; r < a.HW; r += FANDE_NB * FANDE_THREADS) {
        const float v = val ? val[r] : 1.0f;
        nvc += (double)__fmul_rn(fande_consistent(src[r], tgt[r], j.tau), v);
        nv += (double)v;
    }
    nvc = block_sum<FANDE_THREADS / 64>(nvc, red);
    nv = block_sum<FANDE_THREADS / 64>(nv, red);
    if (threadIdx.x == 0) {
        double *o = ws + (((long)blockIdx.z * a.B + b) * FANDE_NB + blockIdx.x) * 2;
        o[0] = nvc;
        o[1] = nv;
    }
}

__global__ __launch_bounds__(FANDE_THREADS) void fande_apply_kernel(FandeArgs a, const double *__restrict__ ws) {
    __shared__ double red[FANDE_THREADS / 64];
    const dkt_fande_job &j = a.job[blockIdx.z];
    const int b = blockIdx.y;
    float select = 0.0f;
    if (j.filter == 2) {
        // prob_threshold = num_valid_consistent / num_valid (fp32 tensors; exact counts for 0/1 masks), prob < prob_threshold
        const double *p = ws + ((long)blockIdx.z * a.B + b) * FANDE_NB * 2;
        const double nvc = block_sum<FANDE_THREADS / 64>(p[threadIdx.x * 2], red);
        const double nv = block_sum<FANDE_THREADS / 64>(p[threadIdx.x * 2 + 1], red);
        const float thr = __fdiv_rn((float)nvc, (float)nv);
        select = j.rand[b] < thr ? 1.0f : 0.0f;
    }
    const float *src = j.src + (long)b * j.src_bstride;
    const float *tgt = j.tgt + (long)b * j.tgt_bstride;
    const float *val = j.valid ? j.valid + (long)b * j.valid_bstride : nullptr;
    float *out = j.out + (long)b * j.out_bstride;
    float *out_valid = j.filter ? j.out_valid + (long)b * j.out_valid_bstride : nullptr;
    for (int r = blockIdx.x * FANDE_THREADS + threadIdx.x; r < a.HW; r += gridDim.x * FANDE_THREADS) {
        float v = val ? val[r] : 1.0f;
        float s = src[r];
        const float t = tgt[r];
        if (j.filter) {
            // FandE_Filter
            const float vc = __fmul_rn(fande_consistent(s, t, j.tau), v);
            s = __fmul_rn(s, v);
            float aug_valid = vc;
            if (j.filter == 2) {
                const float one_m = __fsub_rn(1.0f, vc);
                const float bs = __fmul_rn(__fmul_rn(select, one_m), v);
                aug_valid = __fmul_rn(__fadd_rn(vc, __fmul_rn(one_m, bs)), v);
            }
            s = __fmul_rn(s, aug_valid);
            v = aug_valid;
            out_valid[r] = aug_valid;
        }
        if (j.ensemble) {
            // FandE_Ensemble
            const float vc = __fmul_rn(fande_consistent(s, t, j.tau), v);
            s = __fmul_rn(s, v);
            const float tv = __fmul_rn(t, v);
            const float d = __fsub_rn(s, tv);
            float off = __fmul_rn(j.ens_prob, sqrtf(__fmul_rn(d, d)));
            if (j.clamp) off = off > j.clamp_max ? j.clamp_max : off;      // torch.clamp(max=): NaN stays NaN
            const float dir = s < tv ? 1.0f : (s > tv ? -1.0f : 0.0f);
            const float aug = __fmul_rn(__fmul_rn(dir, off), vc);
            s = __fmul_rn(__fadd_rn(s, aug), v);
        }
        out[r] = s;
    }
}

extern "C" int dkt_fande(const dkt_fande_job *jobs, int njobs, int B, int H, int W, double *ws, int device, void *stream) {
    if (!jobs || !ws) return DKT_E_NULL;
    if (njobs < 1 || njobs > DKT_FANDE_MAX_JOBS || B <= 0 || H <= 0 || W <= 0) return DKT_E_SHAPE;
    if (B > DKT_FANDE_MAX_B || (long)H * W > 0x7fffffffL - FANDE_NB * FANDE_THREADS) return DKT_E_UNSUPPORTED;
    FandeArgs a;
    bool counts = false;
    for (int i = 0; i < njobs; ++i) {
        const dkt_fande_job &j = jobs[i];
        if (j.filter < 0 || j.filter > 2) return DKT_E_UNSUPPORTED;
        if (!j.src || !j.tgt || !j.out || (j.filter && !j.out_valid)) return DKT_E_NULL;
        counts = counts || j.filter == 2;
        a.job[i] = j;
    }
    a.B = B;
    a.HW = H * W;
    DKT_ENTER(device);
    if (counts)
        hipLaunchKernelGGL(fande_count_kernel, dim3(FANDE_NB, B, njobs), dim3(FANDE_THREADS), 0, (hipStream_t)stream, a, ws);
    // about 2048 blocks over all images and jobs (8 per CU of the 256), at least one pixel per thread
    const int per_image = (a.HW + FANDE_THREADS - 1) / FANDE_THREADS;
    int nb = 2048 / (B * njobs);
    nb = nb < 1 ? 1 : (nb > per_image ? per_image : nb);
    hipLaunchKernelGGL(fande_apply_kernel, dim3(nb, B, njobs), dim3(FANDE_THREADS), 0, (hipStream_t)stream, a, ws);
    return dkt_launch_status();
}
