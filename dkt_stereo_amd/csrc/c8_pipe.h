// c8_pipe.h -- the (chunk, tap) MFMA step pipeline shared by conv_c8.hip (conv_c8_kernel) and gru_c8.hip (gru_c8_kernel):
// the activation-patch DMA, the fp16 hi/lo split of C8S outputs, the pinned MFMA / fragment-read primitives and the three-,
// two- and one-pass steps with their counted waits.  ONE copy: a change to the step is made here, once, for both kernels.
//
// The steps are macros (the LDS offsets of the fragment reads must be literals for the asm immediates, and the fragments and
// accumulators must stay in registers), expanded inside a kernel body that has these names in scope:
//   constants   NF (rows per wave: B fragments per tap column), RING (weight ring slots), PASSES, NPP (patch pixels),
//               NIA (activation DMA pieces per wave and chunk), ACT_BYTES, WSLOT
//   registers   f16x8 Ahi[2], Alo[2], Bhi[NF + 2], Blo[NF + 2]; the accumulators behind C8_ACC
//   state       int sl (ring slot of the step being computed); per chunk: cur, nxt (activation buffers of this / the next chunk)
//   addresses   unsigned lds_b_addr (the lane's B fragment base in activation buffer 0)
// and that defines, before the first expansion, what genuinely differs between the kernels:
//   C8_ACC(m, n)       the accumulator block of channel block m, row n
//   C8_WBASE           the lane's A fragment base in ring slot 0
//   C8_WAIT_DMA(T)     the vmcnt wait of step T: this step's weight image (and, at the step that needs it, the patch) has landed
//   C8_ISSUE_DMA(T)    the DMA issued between the X and Y passes of step T (the ring's next image, at step 0 the next patch)
// Inside a step MFP (1 or 2: 32-channel blocks per wave, the step macros' second argument) is a constant the four may use.
#pragma once
#include <hip/hip_runtime.h>

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

#define C8_PC 34                 // patch columns: 32 + halo

__device__ __forceinline__ float c8_sigmoid(float x) { return __frcp_rn(1.0f + __expf(-x)); }
__device__ __forceinline__ float c8_tanh(float x) {
    const float xc = x < -15.0f ? -15.0f : (x > 15.0f ? 15.0f : x);      // NaN passes through
    const float t = __expf(2.0f * xc);
    return (t - 1.0f) * __frcp_rn(t + 1.0f);
}
__device__ __forceinline__ unsigned c8_pack_h2(_Float16 a, _Float16 b) {
    union { _Float16 h[2]; unsigned u; } v;
    v.h[0] = a;
    v.h[1] = b;
    return v.u;
}

template <int N>
__device__ __forceinline__ void c8_wait_vm() {
    // vmcnt(N) only (expcnt / lgkmcnt fields at their no-wait maxima).  The builtin, not inline asm: hipcc keeps its own
    // LDS-read bookkeeping across it, so the first pass after the barrier waits for ITS fragments only (counted lgkmcnt)
    static_assert(N < 64, "vmcnt immediate");
    __builtin_amdgcn_s_waitcnt(0x0F70 | (N & 15) | ((N >> 4) << 14));
}

// Fragment reads are inline asm with hand-counted lgkmcnt waits: hipcc answers every LDS read that is in flight
// across the step's barrier with lgkmcnt(0) at the first MFMA behind it, which exposed the latency of the six reads
// issued just before the barrier in EVERY step (ablation: 296 us with the reads, 200 us without, MFMAs alone 182 us).
template <int OFF>
__device__ __forceinline__ void c8_lds_read(f16x8 &dst, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
}
template <int N>
__device__ __forceinline__ void c8_wait_lgkm() {
    asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
}

// ---- activation DMA: piece p = j * NW + wave covers units u = 64 p + lane of the chunk image
//      [q = 2 kg + hl][patch pixel]; the source offset of a lane inside the chunk's 4 planes is fixed per tile.
// NW waves, NPP patch pixels, NU = 4 NPP 16-byte units per chunk, NPR 1-KiB pieces that carry data, NIA pieces per wave.
template <int NW, int NPP, int NU, int NIA, class Args>
__device__ __forceinline__ void c8_tile_offsets(const Args &a, const int &wave, const int &lane, int th0, int tw0, unsigned (&off)[NIA]) {
#pragma unroll
    for (int j = 0; j < NIA; ++j) {
        int u = 64 * (j * NW + wave) + lane;
        u = u < NU ? u : 0;                              // slack lanes of the last piece re-read unit 0 into slack LDS
        const int q = u / NPP, pp = u - q * NPP;
        const int pr = pp / C8_PC, pc = pp - pr * C8_PC;
        off[j] = (unsigned)(q * a.plane_bytes + ((long)(th0 + pr) * a.Wp + (tw0 + pc)) * 16);
    }
}
template <int NW, int NPR, int NIA>
__device__ __forceinline__ void c8_issue_act(int wave, const char *base, const unsigned (&off)[NIA], char *dst) {
#pragma unroll
    for (int j = 0; j < NIA; ++j)
        __builtin_amdgcn_global_load_lds((const void *)(base + off[j]),
                                         (__attribute__((address_space(3))) void *)(dst + min(j * NW + wave, NPR) * 1024), 16, 0, 0);
}

// ---- C8S outputs need 8 consecutive channels per 16 bytes.  A lane holds four groups j = r >> 2 of four CONSECUTIVE channels
// of its accumulator block (channel (r & 3) + 8 (r >> 2) + 4 kg): the quads (va, vb) of a pair of groups (2 jp, 2 jp + 1) are
// scaled, split into fp16 (hi, lo) and completed to 8-channel groups by exchanging halves with lane ^ 32
// (v_permlane32_swap), after which the lane holds group 2 jp + kg of the block: `hi` and `lo` are its two 16-byte stores.
__device__ __forceinline__ void c8_split_pair(const float (&va)[4], const float (&vb)[4], float act_scale, u32x4 &hi, u32x4 &lo) {
    unsigned ha[2], la[2], hb[2], lb[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const float x0 = va[2 * d] * act_scale, x1 = va[2 * d + 1] * act_scale;
        const float y0 = vb[2 * d] * act_scale, y1 = vb[2 * d + 1] * act_scale;
        const _Float16 a0 = (_Float16)x0, a1 = (_Float16)x1, b0 = (_Float16)y0, b1 = (_Float16)y1;
        ha[d] = c8_pack_h2(a0, a1);
        la[d] = c8_pack_h2((_Float16)(x0 - (float)a0), (_Float16)(x1 - (float)a1));
        hb[d] = c8_pack_h2(b0, b1);
        lb[d] = c8_pack_h2((_Float16)(y0 - (float)b0), (_Float16)(y1 - (float)b1));
    }
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        auto r = __builtin_amdgcn_permlane32_swap(ha[d], hb[d], false, false);
        ha[d] = r[0]; hb[d] = r[1];
        auto q = __builtin_amdgcn_permlane32_swap(la[d], lb[d], false, false);
        la[d] = q[0]; lb[d] = q[1];
    }
    hi = (u32x4){ha[0], ha[1], hb[0], hb[1]};
    lo = (u32x4){la[0], la[1], lb[0], lb[1]};
}

// One MFMA / one fragment read, each pinned in program order: the steps below place at most one LDS read in the
// issue shadow of each MFMA (clusters of six reads between passes cost ~90 us of the 290 on the 384 -> 256 layer --
// not their waits, their issue).  Offsets must be literals for the asm immediates: macros, not loops.
#define C8_MM(A, m, B, r, n)                                                                       \
    {                                                                                              \
        C8_ACC(m, n) = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[m], B[r], C8_ACC(m, n), 0, 0, 0);  \
        __builtin_amdgcn_sched_barrier(0);                                                         \
    }
#define C8_MM2(A, B, r, n) /* row n of every channel block of the wave */                          \
    {                                                                                              \
        C8_MM(A, 0, B, r, n)                                                                       \
        if constexpr (MFP == 2) C8_MM(A, 1, B, r, n)                                               \
    }
#define C8_RD(dst, off, addr)                                  \
    {                                                          \
        c8_lds_read<(off)>(dst, addr);                         \
        __builtin_amdgcn_sched_barrier(0);                     \
    }
#define C8_ROW(r, dx, plane) ((plane) + ((r) * C8_PC + (dx)) * 16)      /* fragment of patch row r at tap column dx */

// The fragments of a tile's (or phase's) first step that the steps do not fetch themselves: Alo, rows 0 .. NF-1 (in the
// order the waits count), from ring slot `sl` / activation buffer g_ & 1, after the DMA of both has landed.
// PASSES == 1 keeps the A fragments double-buffered in the registers the other forms call Ahi / Alo: a chunk has nine steps,
// so even chunks start from Ahi and odd ones from Alo -- the chunk loops run two chunks per trip (the host refuses odd chunk
// counts at one pass; a run-time choice between the two step sequences sent the accumulators to scratch).
#define C8_FIRST_FRAGS(MFP_, g_)                                                                            \
    {                                                                                                       \
        constexpr int MFP = (MFP_);                                                                         \
        const unsigned aw = C8_WBASE + sl * WSLOT, ab = lds_b_addr + ((g_) & 1) * ACT_BYTES;                \
        if constexpr (PASSES == 1) { C8_RD(Ahi[0], 0, aw) if constexpr (MFP == 2) C8_RD(Ahi[1], 512, aw) } \
        else { C8_RD(Alo[0], 2048, aw) if constexpr (MFP == 2) C8_RD(Alo[1], 2048 + 512, aw) }              \
        C8_RD(Bhi[0], C8_ROW(0, 0, 0), ab)                                                                  \
        if constexpr (NF > 1) C8_RD(Bhi[1], C8_ROW(1, 0, 0), ab)                                            \
        if constexpr (NF > 2) C8_RD(Bhi[2], C8_ROW(2, 0, 0), ab)                                            \
        if constexpr (NF > 3) C8_RD(Bhi[3], C8_ROW(3, 0, 0), ab)                                            \
        if constexpr (PASSES == 3) {                                                                        \
            C8_RD(Blo[0], C8_ROW(0, 0, NPP * 16), ab)                                                       \
            if constexpr (NF > 1) C8_RD(Blo[1], C8_ROW(1, 0, NPP * 16), ab)                                 \
            if constexpr (NF > 2) C8_RD(Blo[2], C8_ROW(2, 0, NPP * 16), ab)                                 \
            if constexpr (NF > 3) C8_RD(Blo[3], C8_ROW(3, 0, NPP * 16), ab)                                 \
        }                                                                                                   \
        c8_wait_lgkm<0>();                                                                                  \
    }

// ---- the head every step form shares: its constants, the wait for this step's DMA and the step's ONE raw barrier
// (no drained waits: DMA and fragment reads stay in flight across it)
#define C8_STEP_HEAD(T, MFP_)                                                                                          \
        constexpr int MFP = (MFP_), DX = (T) / 3, DY = (T) % 3, NDX = (DX + 1) % 3;                                    \
        static_assert(MFP == 2 || NF == 4, "the one-block (MFP == 1) MFMA order is written for four rows");         \
        const int sl1 = sl + 1 == RING ? 0 : sl + 1, sl2 = sl == 0 ? RING - 1 : sl - 1;                                \
        const unsigned adw_s = C8_WBASE + sl * WSLOT;                                                                  \
        const unsigned adw_n = C8_WBASE + sl1 * WSLOT;                                                                 \
        const unsigned adb_c = lds_b_addr + cur * ACT_BYTES;                     /* this column's patch */             \
        const unsigned adb_n = lds_b_addr + (DX < 2 ? cur : nxt) * ACT_BYTES;    /* the next column's   */             \
        (void)sl2; (void)adw_s; (void)adw_n; (void)adb_c; (void)adb_n;                                                 \
        C8_WAIT_DMA(T)                                                                                                 \
        __builtin_amdgcn_s_barrier();

// One (chunk, tap) step at PASSES == 3.  Steps run tap COLUMN by column (dx outer, dy inner: the weight images are packed in
// that order), so that a B fragment -- one patch row r at column dx -- serves the (up to) three steps dy = r - n:
// step (dx, dy) multiplies row n + dy for its output row n.  Rows are re-read into their own registers when
// they die: row 0 after step dy = 0, row 1 after dy = 1, rows 2 .. NF-1 during dy = 2 (each after the MFMAs of
// n = r - 2), always for the NEXT column (or the next chunk's column 0); rows NF and NF+1, first needed at
// dy = 1 / dy = 2, are fetched one step ahead (during dy = 0 / dy = 1 of their own column).  8 reads per step for
// the 64 x 4-row wave tile instead of 12: the convolution's time follows its LDS read volume (ablation: 278 us
// at 12 reads per step, 228 at 8, 208 at 0).  LDS reads in issue order (the waits count them):
//   X (Alo x Bhi): Ahi[0], Ahi[1]; dy = 0: row NF (hi, lo); dy = 1: row NF+1 (hi, lo)
//   Y (Ahi x Bhi): Alo'[0], Alo'[1], then the hi halves of the dying rows
//   Z (Ahi x Blo): the lo halves of the dying rows
// With ONE channel block per wave (MFP == 1, four rows) there are half as many MFMA shadows: the same reads sit between the
// MFMAs of consecutive rows instead of between those of the two blocks of a row.
#define C8_STEP3(T, MFP_)                                                                                              \
    {                                                                                                                  \
        C8_STEP_HEAD(T, MFP_)                                                                                          \
        /* Alo and this step's hi rows are in; what the previous step read after them may still fly */                \
        if constexpr (DY == 0) c8_wait_lgkm<(NF > 2 ? NF - 2 : 0)>();                                                  \
        else if constexpr (DY == 1) c8_wait_lgkm<2>();                                                                 \
        else c8_wait_lgkm<(NF > 1 ? 2 : 0)>();                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
        /* ---- X */                                                                                                   \
        C8_MM(Alo, 0, Bhi, DY, 0) C8_RD(Ahi[0], 0, adw_s)                                                              \
        if constexpr (MFP == 2) { C8_MM(Alo, 1, Bhi, DY, 0) C8_RD(Ahi[1], 512, adw_s) }                                \
        if constexpr (NF > 1) { C8_MM(Alo, 0, Bhi, 1 + DY, 1)                                                          \
            if constexpr (DY < 2) C8_RD(Bhi[NF + DY], C8_ROW(NF + DY, DX, 0), adb_c)                                   \
            if constexpr (MFP == 2) C8_MM(Alo, 1, Bhi, 1 + DY, 1)                                                      \
            if constexpr (MFP == 1 && NF > 2) C8_MM(Alo, 0, Bhi, 2 + DY, 2)                                            \
            if constexpr (DY < 2) C8_RD(Blo[NF + DY], C8_ROW(NF + DY, DX, NPP * 16), adb_c) }                          \
        else if constexpr (DY < 2) { C8_RD(Bhi[NF + DY], C8_ROW(NF + DY, DX, 0), adb_c)                                \
            C8_RD(Blo[NF + DY], C8_ROW(NF + DY, DX, NPP * 16), adb_c) }                                                \
        if constexpr (MFP == 2 && NF > 2) C8_MM2(Alo, Bhi, 2 + DY, 2)                                                  \
        if constexpr (NF > 3) C8_MM2(Alo, Bhi, 3 + DY, 3)                                                              \
        C8_ISSUE_DMA(T)                                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
        c8_wait_lgkm<(DY < 2 ? 2 : 0)>(); /* Ahi is in (the row read ahead may still fly) */                           \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
        /* ---- Y */                                                                                                   \
        C8_MM(Ahi, 0, Bhi, DY, 0) C8_RD(Alo[0], 2048, adw_n)                                                           \
        if constexpr (MFP == 2) { C8_MM(Ahi, 1, Bhi, DY, 0) C8_RD(Alo[1], 2048 + 512, adw_n) }                         \
        if constexpr (MFP == 1 && NF > 1) C8_MM(Ahi, 0, Bhi, 1 + DY, 1)                                                \
        if constexpr (DY == 0) C8_RD(Bhi[0], C8_ROW(0, NDX, 0), adb_n)                                                 \
        if constexpr (DY == 1 && NF > 1) C8_RD(Bhi[1], C8_ROW(1, NDX, 0), adb_n)                                       \
        if constexpr (DY == 2 && NF > 2) C8_RD(Bhi[2], C8_ROW(2, NDX, 0), adb_n)                                       \
        if constexpr (NF > 1) {                                                                                        \
            if constexpr (MFP == 2) C8_MM2(Ahi, Bhi, 1 + DY, 1)                                                        \
            if constexpr (MFP == 1 && NF > 2) C8_MM(Ahi, 0, Bhi, 2 + DY, 2)                                            \
            if constexpr (DY == 2 && NF > 3) C8_RD(Bhi[3], C8_ROW(3, NDX, 0), adb_n) }                                 \
        if constexpr (MFP == 2 && NF > 2) C8_MM2(Ahi, Bhi, 2 + DY, 2)                                                  \
        if constexpr (NF > 3) C8_MM2(Ahi, Bhi, 3 + DY, 3)                                                              \
        /* ---- Z (every lo row of this step was read before this step's X reads: in since the wait before Y) */       \
        C8_MM2(Ahi, Blo, DY, 0)                                                                                        \
        if constexpr (DY == 0) C8_RD(Blo[0], C8_ROW(0, NDX, NPP * 16), adb_n)                                          \
        if constexpr (DY == 1 && NF > 1) C8_RD(Blo[1], C8_ROW(1, NDX, NPP * 16), adb_n)                                \
        if constexpr (DY == 2 && NF > 2) C8_RD(Blo[2], C8_ROW(2, NDX, NPP * 16), adb_n)                                \
        if constexpr (NF > 1) { C8_MM2(Ahi, Blo, 1 + DY, 1)                                                            \
            if constexpr (DY == 2 && NF > 3) C8_RD(Blo[3], C8_ROW(3, NDX, NPP * 16), adb_n) }                          \
        if constexpr (NF > 2) C8_MM2(Ahi, Blo, 2 + DY, 2)                                                              \
        if constexpr (NF > 3) C8_MM2(Ahi, Blo, 3 + DY, 3)                                                              \
        sl = sl1;                                                                                                      \
    }
// PASSES == 2: C8_STEP3 without its Z pass and without any lo row.  LDS reads in issue order:
//   X (Alo x Bhi): Ahi[0], Ahi[1]; dy = 0: row NF; dy = 1: row NF+1
//   Y (Ahi x Bhi): Alo'[0], Alo'[1], then the dying rows (for the next column)
// so a step starts with its Alo and rows in once at most the previous step's dying-row reads fly (1 after dy = 0,
// 1 after dy = 1 when NF > 1, none after dy = 2: the rows re-read there are this step's)
#define C8_STEP2(T, MFP_)                                                                                              \
    {                                                                                                                  \
        C8_STEP_HEAD(T, MFP_)                                                                                          \
        if constexpr (DY == 1) c8_wait_lgkm<1>();                                                                      \
        else if constexpr (DY == 2) c8_wait_lgkm<(NF > 1 ? 1 : 0)>();                                                  \
        else c8_wait_lgkm<0>();                                                                                        \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
        C8_MM(Alo, 0, Bhi, DY, 0) C8_RD(Ahi[0], 0, adw_s)                                                              \
        if constexpr (MFP == 2) { C8_MM(Alo, 1, Bhi, DY, 0) C8_RD(Ahi[1], 512, adw_s) }                                \
        if constexpr (NF > 1) { C8_MM(Alo, 0, Bhi, 1 + DY, 1)                                                          \
            if constexpr (DY < 2) C8_RD(Bhi[NF + DY], C8_ROW(NF + DY, DX, 0), adb_c)                                   \
            if constexpr (MFP == 2) C8_MM(Alo, 1, Bhi, 1 + DY, 1) }                                                    \
        else if constexpr (DY < 2) C8_RD(Bhi[NF + DY], C8_ROW(NF + DY, DX, 0), adb_c)                                  \
        if constexpr (NF > 2) C8_MM2(Alo, Bhi, 2 + DY, 2)                                                              \
        if constexpr (NF > 3) C8_MM2(Alo, Bhi, 3 + DY, 3)                                                              \
        C8_ISSUE_DMA(T)                                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
        c8_wait_lgkm<(DY < 2 ? 1 : 0)>(); /* Ahi is in (the row read ahead may still fly) */                           \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
        C8_MM(Ahi, 0, Bhi, DY, 0) C8_RD(Alo[0], 2048, adw_n)                                                           \
        if constexpr (MFP == 2) { C8_MM(Ahi, 1, Bhi, DY, 0) C8_RD(Alo[1], 2048 + 512, adw_n) }                         \
        if constexpr (DY == 0) C8_RD(Bhi[0], C8_ROW(0, NDX, 0), adb_n)                                                 \
        if constexpr (DY == 1 && NF > 1) C8_RD(Bhi[1], C8_ROW(1, NDX, 0), adb_n)                                       \
        if constexpr (DY == 2 && NF > 2) C8_RD(Bhi[2], C8_ROW(2, NDX, 0), adb_n)                                       \
        if constexpr (NF > 1) { C8_MM2(Ahi, Bhi, 1 + DY, 1)                                                            \
            if constexpr (DY == 2 && NF > 3) C8_RD(Bhi[3], C8_ROW(3, NDX, 0), adb_n) }                                 \
        if constexpr (NF > 2) C8_MM2(Ahi, Bhi, 2 + DY, 2)                                                              \
        if constexpr (NF > 3) C8_MM2(Ahi, Bhi, 3 + DY, 3)                                                              \
        sl = sl1;                                                                                                      \
    }
// PASSES == 1: one product per block, A fragments double-buffered (PA: this step's, PB: the next step's, fetched first
// thing behind the barrier), MFMAs row by row so that a dying row is re-read as soon as its last product has issued.
// LDS reads in issue order: PB[0], PB[1]; dy < 2: row NF + dy; then the dying rows.  Waits as in C8_STEP2.
#define C8_STEP1(T, MFP_, PA, PB)                                                                                      \
    {                                                                                                                  \
        C8_STEP_HEAD(T, MFP_)                                                                                          \
        if constexpr (DY == 1) c8_wait_lgkm<1>();                                                                      \
        else if constexpr (DY == 2) c8_wait_lgkm<(NF > 1 ? 1 : 0)>();                                                  \
        else c8_wait_lgkm<0>();                                                                                        \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
        C8_RD(PB[0], 0, adw_n)                                                                                         \
        if constexpr (MFP == 2) C8_RD(PB[1], 512, adw_n)                                                               \
        if constexpr (DY < 2) C8_RD(Bhi[NF + DY], C8_ROW(NF + DY, DX, 0), adb_c)                                       \
        C8_MM2(PA, Bhi, DY, 0)                                                                                         \
        if constexpr (DY == 0) C8_RD(Bhi[0], C8_ROW(0, NDX, 0), adb_n)                                                 \
        if constexpr (DY == 1 && NF > 1) C8_RD(Bhi[1], C8_ROW(1, NDX, 0), adb_n)                                       \
        if constexpr (DY == 2 && NF > 2) C8_RD(Bhi[2], C8_ROW(2, NDX, 0), adb_n)                                       \
        C8_ISSUE_DMA(T)                                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
        if constexpr (NF > 1) { C8_MM2(PA, Bhi, 1 + DY, 1)                                                             \
            if constexpr (DY == 2 && NF > 3) C8_RD(Bhi[3], C8_ROW(3, NDX, 0), adb_n) }                                 \
        if constexpr (NF > 2) C8_MM2(PA, Bhi, 2 + DY, 2)                                                               \
        if constexpr (NF > 3) C8_MM2(PA, Bhi, 3 + DY, 3)                                                               \
        sl = sl1;                                                                                                      \
    }
// The nine steps of a chunk (PASSES == 3 or 2) / of an even or odd chunk at PASSES == 1 (PA, PB = Ahi, Alo or Alo, Ahi)
#define C8_CHUNK(MFP_)                                                                                                 \
    if constexpr (PASSES == 3) {                                                                                       \
        C8_STEP3(0, MFP_) C8_STEP3(1, MFP_) C8_STEP3(2, MFP_) C8_STEP3(3, MFP_) C8_STEP3(4, MFP_) C8_STEP3(5, MFP_)    \
        C8_STEP3(6, MFP_) C8_STEP3(7, MFP_) C8_STEP3(8, MFP_)                                                          \
    } else {                                                                                                           \
        C8_STEP2(0, MFP_) C8_STEP2(1, MFP_) C8_STEP2(2, MFP_) C8_STEP2(3, MFP_) C8_STEP2(4, MFP_) C8_STEP2(5, MFP_)    \
        C8_STEP2(6, MFP_) C8_STEP2(7, MFP_) C8_STEP2(8, MFP_)                                                          \
    }
#define C8_CHUNK1(MFP_, PA, PB)                                                                                        \
    C8_STEP1(0, MFP_, PA, PB) C8_STEP1(1, MFP_, PB, PA) C8_STEP1(2, MFP_, PA, PB) C8_STEP1(3, MFP_, PB, PA)            \
    C8_STEP1(4, MFP_, PA, PB) C8_STEP1(5, MFP_, PB, PA) C8_STEP1(6, MFP_, PA, PB) C8_STEP1(7, MFP_, PB, PA)            \
    C8_STEP1(8, MFP_, PA, PB)
