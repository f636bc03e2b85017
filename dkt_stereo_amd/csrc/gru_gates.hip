// gru_gates.hip -- ConvGRU gate fusions for gfx950: inference, and the training path (BasicMultiUpdateBlock under
// autograd, dkt_stereo_amd/gru_train.py).
// Reference: core/update.py:23-32 (== meta_arch/igev_stereo/update.py:33-41), and torch autograd through those lines.
//
// The reference evaluates each GRU as ~12 elementwise torch kernels plus three
// torch.cat copies.  Here the z|r convolutions are one merged convolution and
// the gate arithmetic is two streaming kernels:
//   gate_zr : z = sigmoid(az+cz), r = sigmoid(ar+cr), rh = r*h   (7 planes of traffic)
//   gate_out: q = tanh(aq+cq), h' = (1-z)*h + z*q                (5 planes)
// rh is stored straight into the first Ch channels of convq's [r*h | x] input
// buffer, so the second torch.cat of the reference never happens.
//
//   dkt_gru_gate_zr_train   dkt_gru_gate_zr that also writes r:  the same z and rh, bit for bit
//   dkt_gru_gate_out_train  dkt_gru_gate_out that also writes q: the same h', bit for bit
//   dkt_gru_gate_out_bwd    gaq = g z (1 - q q),  gz = g (q - h),  gh = g (1 - z)
//   dkt_gru_gate_zr_bwd     gazr = [gz z (1 - z) | grh h r (1 - r)],  gh = grh r
//
// All six are HBM-bound streaming kernels on the one walk of gru_gates.h: float4 accesses when Ch*HW, every batch stride and
// every pointer allow it, a scalar path otherwise, a grid-stride loop over at most 2048 blocks of 256; every load of an item
// is issued before the first use.  No LDS, no atomics: bit-identical from run to run.
// Every product, sum and difference is one explicitly rounded operation (no contraction, whatever the compiler flags).
#include "gru_gates.h"

// the plane only a training forward keeps (r, q): the inference instantiation has no such member
template <bool KEEP>
struct GateKept {
    float *kept;
};
template <>
struct GateKept<false> {};

// ---- forward ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gate_sigmoid_sum(float a, float c) { return dkt_sigmoid(__fadd_rn(a, c)); }
__device__ __forceinline__ float gate_mul(float a, float b) { return __fmul_rn(a, b); }

template <bool KEEP_R>
struct GateZr : GateKept<KEEP_R> {
    const float *azr, *cz, *cr, *h;
    float *z, *rh;
    long cz_bs, cr_bs, h_bs, rh_bs;
    long CHW;  // Ch*HW

    template <int V>
    __device__ __forceinline__ void item(long b, long e) const {
        // (every address before the first load, here and below: the loads of an item then issue back to back)
        const float *paz = azr + b * 2 * CHW + e, *par = paz + CHW;
        const float *pcz = cz + b * cz_bs + e, *pcr = cr + b * cr_bs + e, *ph = h + b * h_bs + e;
        float *pz = z + b * CHW + e, *prh = rh + b * rh_bs + e;
        const GateVec<V> az = gate_load<V>(paz), ar = gate_load<V>(par);
        const GateVec<V> vcz = gate_load<V>(pcz), vcr = gate_load<V>(pcr), vh = gate_load<V>(ph);
        const GateVec<V> vz = gate_map<V>(gate_sigmoid_sum, az, vcz), vr = gate_map<V>(gate_sigmoid_sum, ar, vcr);
        gate_store<V>(pz, vz);
        if constexpr (KEEP_R) gate_store<V>(this->kept + b * CHW + e, vr);
        gate_store<V>(prh, gate_map<V>(gate_mul, vr, vh));
    }
};

template <bool KEEP_R>
static int gate_zr(const float *azr, const float *cz, long cz_bstride, const float *cr, long cr_bstride, const float *h,
                   long h_bstride, float *z, float *r, float *rh, long rh_bstride, int B, int Ch, long HW, int device,
                   void *stream) {
    DKT_ENTER(device);
    GateZr<KEEP_R> a;
    a.azr = azr; a.cz = cz; a.cr = cr; a.h = h; a.z = z; a.rh = rh;
    if constexpr (KEEP_R) a.kept = r;
    a.cz_bs = cz_bstride; a.cr_bs = cr_bstride; a.h_bs = h_bstride; a.rh_bs = rh_bstride;
    a.CHW = (long)Ch * HW;
    return gate_launch(a, B, {azr, cz, cr, h, z, r, rh}, {cz_bstride, cr_bstride, h_bstride, rh_bstride}, stream);
}

extern "C" int dkt_gru_gate_zr(const float *azr, const float *cz, long cz_bstride,
                               const float *cr, long cr_bstride, const float *h, long h_bstride,
                               float *z, float *rh, long rh_bstride,
                               int B, int Ch, long HW, int device, void *stream) {
    if (!azr || !cz || !cr || !h || !z || !rh) return DKT_E_NULL;
    if (B <= 0 || Ch <= 0 || HW <= 0) return DKT_E_SHAPE;
    return gate_zr<false>(azr, cz, cz_bstride, cr, cr_bstride, h, h_bstride, z, nullptr, rh, rh_bstride, B, Ch, HW, device,
                          stream);
}

extern "C" int dkt_gru_gate_zr_train(const float *azr, const float *cz, long cz_bstride,
                                     const float *cr, long cr_bstride, const float *h, long h_bstride,
                                     float *z, float *r, float *rh, long rh_bstride,
                                     int B, int Ch, long HW, int device, void *stream) {
    if (!azr || !cz || !cr || !h || !z || !r || !rh) return DKT_E_NULL;
    if (B <= 0 || Ch <= 0 || HW <= 0) return DKT_E_SHAPE;
    return gate_zr<true>(azr, cz, cz_bstride, cr, cr_bstride, h, h_bstride, z, r, rh, rh_bstride, B, Ch, HW, device, stream);
}

template <bool KEEP_Q>
struct GateOut : GateKept<KEEP_Q> {
    const float *aq, *cq, *z, *h;
    float *hout;
    long cq_bs, h_bs, hout_bs;
    long CHW;

    template <int V>
    __device__ __forceinline__ void item(long b, long e) const {
        const long d = b * CHW + e;                      // the dense tensors
        const float *paq = aq + d, *pcq = cq + b * cq_bs + e, *pz = z + d, *ph = h + b * h_bs + e;
        const GateVec<V> vaq = gate_load<V>(paq), vcq = gate_load<V>(pcq), vz = gate_load<V>(pz), vh = gate_load<V>(ph);
        const GateVec<V> vq = gate_map<V>(dkt_gru_q, vaq, vcq);
        if constexpr (KEEP_Q) gate_store<V>(this->kept + d, vq);
        gate_store<V>(hout + b * hout_bs + e, gate_map<V>(dkt_gru_blend, vz, vh, vq));
    }
};

template <bool KEEP_Q>
static int gate_out(const float *aq, const float *cq, long cq_bstride, const float *z, const float *h, long h_bstride,
                    float *q, float *hout, long hout_bstride, int B, int Ch, long HW, int device, void *stream) {
    DKT_ENTER(device);
    GateOut<KEEP_Q> a;
    a.aq = aq; a.cq = cq; a.z = z; a.h = h; a.hout = hout;
    if constexpr (KEEP_Q) a.kept = q;
    a.cq_bs = cq_bstride; a.h_bs = h_bstride; a.hout_bs = hout_bstride;
    a.CHW = (long)Ch * HW;
    return gate_launch(a, B, {aq, cq, z, h, q, hout}, {cq_bstride, h_bstride, hout_bstride}, stream);
}

extern "C" int dkt_gru_gate_out(const float *aq, const float *cq, long cq_bstride,
                                const float *z, const float *h, long h_bstride,
                                float *hout, long hout_bstride,
                                int B, int Ch, long HW, int device, void *stream) {
    if (!aq || !cq || !z || !h || !hout) return DKT_E_NULL;
    if (B <= 0 || Ch <= 0 || HW <= 0) return DKT_E_SHAPE;
    return gate_out<false>(aq, cq, cq_bstride, z, h, h_bstride, nullptr, hout, hout_bstride, B, Ch, HW, device, stream);
}

extern "C" int dkt_gru_gate_out_train(const float *aq, const float *cq, long cq_bstride,
                                      const float *z, const float *h, long h_bstride,
                                      float *q, float *hout, long hout_bstride,
                                      int B, int Ch, long HW, int device, void *stream) {
    if (!aq || !cq || !z || !h || !q || !hout) return DKT_E_NULL;
    if (B <= 0 || Ch <= 0 || HW <= 0) return DKT_E_SHAPE;
    return gate_out<true>(aq, cq, cq_bstride, z, h, h_bstride, q, hout, hout_bstride, B, Ch, HW, device, stream);
}

// ---- backward --------------------------------------------------------------------------------------------------------
// h' = (1 - z) h + z q,  q = tanh(aq + cq):
//   gaq = (g z) (1 - q q)     gz = g (q - h)     gh = g (1 - z)
// Where q is +-1 or z is 0 the affected gradient is an exact 0 (a product with an exact 0 factor).
__device__ __forceinline__ float gate_out_gaq(float g, float z, float q) {
    return __fmul_rn(__fmul_rn(g, z), __fsub_rn(1.0f, __fmul_rn(q, q)));
}
__device__ __forceinline__ float gate_out_gz(float g, float q, float h) { return __fmul_rn(g, __fsub_rn(q, h)); }
__device__ __forceinline__ float gate_out_gh(float g, float z) { return __fmul_rn(g, __fsub_rn(1.0f, z)); }

struct GateOutBwd {
    const float *g, *z, *q, *h;
    float *gaq, *gz, *gh;      // each may be null
    long g_bs, h_bs;
    long CHW;

    template <int V>
    __device__ __forceinline__ void item(long b, long e) const {
        const long d = b * CHW + e;                      // the dense tensors
        const float *pg = g + b * g_bs + e, *pz = z + d, *pq = q + d, *ph = h + b * h_bs + e;
        const GateVec<V> vg = gate_load<V>(pg), vz = gate_load<V>(pz), vq = gate_load<V>(pq), vh = gate_load<V>(ph);
        if (gaq) gate_store<V>(gaq + d, gate_map<V>(gate_out_gaq, vg, vz, vq));
        if (gz) gate_store<V>(gz + d, gate_map<V>(gate_out_gz, vg, vq, vh));
        if (gh) gate_store<V>(gh + d, gate_map<V>(gate_out_gh, vg, vz));
    }
};

extern "C" int dkt_gru_gate_out_bwd(const float *gout, long gout_bstride, const float *z, const float *q,
                                    const float *h, long h_bstride, float *gaq, float *gz, float *gh,
                                    int B, int Ch, long HW, int device, void *stream) {
    if (!gout || !z || !q || !h || (!gaq && !gz && !gh)) return DKT_E_NULL;
    if (B <= 0 || Ch <= 0 || HW <= 0) return DKT_E_SHAPE;
    DKT_ENTER(device);
    GateOutBwd a;
    a.g = gout; a.z = z; a.q = q; a.h = h; a.gaq = gaq; a.gz = gz; a.gh = gh;
    a.g_bs = gout_bstride; a.h_bs = h_bstride;
    a.CHW = (long)Ch * HW;
    return gate_launch(a, B, {gout, z, q, h, gaq, gz, gh}, {gout_bstride, h_bstride}, stream);
}

// z = sigmoid(az + cz), r = sigmoid(ar + cr), rh = r h:
//   gaz = (gz z) (1 - z)     gar = ((grh h) r) (1 - r)     gh = grh r
// gaz | gar are the two halves of one (B, 2Ch, HW) tensor, the layout of the merged pre-activation.
__device__ __forceinline__ float gate_zr_gaz(float gz, float z) { return __fmul_rn(__fmul_rn(gz, z), __fsub_rn(1.0f, z)); }
__device__ __forceinline__ float gate_zr_gar(float grh, float h, float r) {
    return __fmul_rn(__fmul_rn(__fmul_rn(grh, h), r), __fsub_rn(1.0f, r));
}

struct GateZrBwd {
    const float *gz, *grh, *z, *r, *h;
    float *gazr, *gh;          // each may be null
    long grh_bs, h_bs;
    long CHW;

    template <int V>
    __device__ __forceinline__ void item(long b, long e) const {
        const long d = b * CHW + e;                      // the dense (B, Ch, HW) tensors
        const float *pgz = gz + d, *pgrh = grh + b * grh_bs + e, *pz = z + d, *pr = r + d, *ph = h + b * h_bs + e;
        const GateVec<V> vgz = gate_load<V>(pgz), vgrh = gate_load<V>(pgrh);
        const GateVec<V> vz = gate_load<V>(pz), vr = gate_load<V>(pr), vh = gate_load<V>(ph);
        if (gazr) {
            float *pgaz = gazr + b * 2 * CHW + e;
            gate_store<V>(pgaz, gate_map<V>(gate_zr_gaz, vgz, vz));
            gate_store<V>(pgaz + CHW, gate_map<V>(gate_zr_gar, vgrh, vh, vr));
        }
        if (gh) gate_store<V>(gh + d, gate_map<V>(gate_mul, vgrh, vr));
    }
};

extern "C" int dkt_gru_gate_zr_bwd(const float *gz, const float *grh, long grh_bstride, const float *z, const float *r,
                                   const float *h, long h_bstride, float *gazr, float *gh,
                                   int B, int Ch, long HW, int device, void *stream) {
    if (!gz || !grh || !z || !r || !h || (!gazr && !gh)) return DKT_E_NULL;
    if (B <= 0 || Ch <= 0 || HW <= 0) return DKT_E_SHAPE;
    DKT_ENTER(device);
    GateZrBwd a;
    a.gz = gz; a.grh = grh; a.z = z; a.r = r; a.h = h; a.gazr = gazr; a.gh = gh;
    a.grh_bs = grh_bstride; a.h_bs = h_bstride;
    a.CHW = (long)Ch * HW;
    return gate_launch(a, B, {gz, grh, z, r, h, gazr, gh}, {grh_bstride, h_bstride}, stream);
}
