// conv_c8.hip -- round-3 3x3 convolution of the update operator (core/update.py:16-32, 64-85, 6-13) on gfx950:
// the same split-fp16 arithmetic as conv2d.hip (w*x ~= w_hi*x_hi + w_lo*x_hi + w_hi*x_lo, fp32 accumulation, three
// v_mfma_f32_32x32x16_f16 per product block), rebuilt around the measured limiter of that kernel (the
// weight stream through the vector-memory path, staging VALU work and registers, one drained barrier per chunk):
//
//   * ACTIVATIONS ARRIVE PRE-SPLIT ("C8S" layout): the producing kernel's epilogue writes fp16 (hi, lo) pairs,
//     [batch][channel group of 8][hi|lo][Hp][Wp][8 channels] with a zero border (Hp = roundup(H,8)+2,
//     Wp = roundup(W,32)+2) -- the same bytes as fp32.  A (rows+2) x 34 pixel patch of a 16-channel chunk is then
//     copied global -> LDS by the DMA path (global_load_lds, 16 B per lane, no registers, no VALU, no bounds
//     logic: the border is part of the tensor) into the exact image the B fragments are read from
//     ([plane][pixel] x 16 B: conflict-free ds_read_b128).
//   * WEIGHTS go through LDS too, shared by all waves of the block: per (chunk, tap) step one contiguous
//     [co64 block][hi|lo][k8][64 co][8] image (4 KB per 64 output channels) is DMA'd into a 3-slot ring two steps
//     ahead.  Per block and step the vector-memory path carries 16 KB instead of the 32 KB the per-wave weight loads
//     of conv2d.hip pull through L1 (and blocks are twice as large, so half as many of them stream the image).
//   * ONE raw s_barrier per step, counted vmcnt AND counted lgkmcnt, no drained waits: DMA and fragment reads stay
//     in flight across barriers.  Fragment registers are single-buffered: every fragment is re-read into its own
//     register as soon as its last MFMA of the step has issued, one read per MFMA issue shadow (see C8_STEP3, c8_pipe.h).
//   * wave tile 64 co x NF rows x 32 columns (NF = 4: 128 accumulators); steps walk the taps column by column so that
//     a B fragment (one patch row) serves three steps: 24 MFMAs per 8 fragment reads.
//
// Outputs: fp32 NCHW and / or C8S (the next convolution's operand), fused ConvGRU gate epilogues as conv2d.hip.
#include "dkt_common.h"
#include "c8_pipe.h"
#include <cstdlib>

#define C8_MAX_SRC 4

// Translation units (build.py, as for conv2d.hip): the kernel's instantiations are the long pole of the build, so the file is
// compiled once per value of C8_TU -- 0: the host side and the small kernels; 1, 2, 3: conv_c8_kernel at that many passes.
// Without the definition the whole file is one unit (tools/c8_variant.py).
#ifndef C8_TU
#define C8_TU (-1)
#endif

struct C8Args {
    const char *src[C8_MAX_SRC];      // C8S tensors (all with the same Hp, Wp)
    long src_bs[C8_MAX_SRC];          // bytes per batch item
    int src_n16[C8_MAX_SRC];          // 16-channel chunks per source
    int nsrc, nchunks;
    long plane_bytes;                 // Hp * Wp * 16
    int Wp;
    const char *w;                    // [chunk][tap][co64][hi|lo][k8][64][8] fp16
    int n_co64;
    const float *bias;
    float out_scale;
    int H, W, Cout;
    int tiles_w, tiles_xy, n_co, total_tiles;
    int relu, epi;
    float *out;  long out_bs;          // fp32 NCHW destination (or null)
    char *out_c8; long out_c8_bs, out_c8_plane; int out_c8_Wp, out_c8_ch0;   // C8S destination (or null)
    float act_scale;                   // power of two applied before the fp16 split of C8S outputs
    const float *e_c0, *e_c1, *e_h;    // gate operands (fp32 NCHW), see conv2d.hip
    long e_c0_bs, e_c1_bs, e_h_bs;
    float *out2; long out2_bs;         // epi 1: r*h as fp32 NCHW (or null)
    char *out2_c8; long out2_c8_bs;    // epi 1: r*h as C8S (same Hp/Wp/plane as out_c8; channel offset out2_c8_ch0)
    int out2_c8_ch0;
    // epi 3 (flow / disparity head, core/update.py:9-13 with 1 or 2 outputs): the layer's ReLU output is never written;
    // its epilogue reduces it over the block's channels against the NEXT layer's 3x3 weights, one plane per (output, tap):
    // head_out[b][(o * n_co + co block) * 9 + tap][H][W] = sum_co head_w[o][co][tap] * relu(conv)[co]; dkt_head_finish sums
    // the shifted planes.
    const float *head_w;               // [n_out][Cout][12] (9 taps + 3 pad)
    float *head_out; long head_out_bs; int head_nout;
    int f32_c4;                        // the fp32 tensors above (out, out2, e_c0, e_c1, e_h) are [B][C/4][H][W][4] instead of NCHW
    const float *tail; long tail_bs; int tail_ch;   // epi 0: channels Cout .. Cout+tail_ch-1 of the C8S output are copied from here
    float tail_ratio;                  // ... times tail_scale / act_scale (the tail channels may carry their own power-of-two scale)
};

struct C8ArgsPair {
    C8Args p[2];
};

// A wave-uniform value pinned to scalar registers: what comes out cannot be recomputed (or re-loaded) from what went in.
// (readfirstlane first: a uniform value the compiler computed on the vector ALU -- a division, say -- is in a vector register)
__device__ __forceinline__ unsigned c8_hold(unsigned x) {
    x = __builtin_amdgcn_readfirstlane(x);
    asm volatile("" : "+s"(x));
    return x;
}
__device__ __forceinline__ int c8_hold(int x) { return (int)c8_hold((unsigned)x); }
__device__ __forceinline__ float c8_hold(float x) { return __uint_as_float(c8_hold(__float_as_uint(x))); }
template <class T>
__device__ __forceinline__ T *c8_hold(T *p) {
    // (every pointer of the argument structure is a global one; rebuilt from two integers it would be a flat one)
    const unsigned long long v = (unsigned long long)p;
    return (T *)(__attribute__((address_space(1))) T *)(((unsigned long long)c8_hold((unsigned)(v >> 32)) << 32) | c8_hold((unsigned)v));
}
// The same for an address formed per access, without `volatile`: a volatile statement is a fence for the memory operations
// around it (the loads of an operand batch would go out one by one); this one only cannot be folded into its neighbours.
template <class T>
__device__ __forceinline__ T *c8_base(T *p) {
    unsigned long long v = (unsigned long long)p;
    unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    asm("" : "+s"(lo), "+s"(hi));
    return (T *)(__attribute__((address_space(1))) T *)(((unsigned long long)hi << 32) | lo);
}
template <int V>
struct C8Tag {
    static constexpr int value = V;
};

#if C8_TU != 0
// WM x WN waves along (output channels, rows); wave tile 64 co x NF rows x 32 columns.
// RING = weight ring slots: step s computes from slot s % RING while the images of steps s+1 .. s+RING-1 are in the ring or
// on their way (short steps -- small wave tiles -- need the deeper rings to cover the DMA latency).
// PASSES (round 5): 3 = the fp32-class product above; 2 = w_hi*x_hi + w_lo*x_hi (activations rounded to fp16: their lo planes are
// never read); 1 = w_hi*x_hi only (plain fp16 operands).  Reduced-pass launches are NOT parity paths by themselves: they serve the
// precision schedules of loop_c8 (early refinement iterations at fewer passes).  The DMA stream, the ring and the
// vmcnt waits are the same in all three; what changes is which fragments are read and multiplied (and the lgkmcnt counts).
// The kernel's body as a device function (round 5): `nblocks` persistent blocks, this one `bid`, walk the tiles of the launch's
// one or two problems; `lds` = the block's dynamic LDS.  conv_c8_kernel is this body.
template <int WM, int WN, int NF, int RING, int PASSES>
__device__ __forceinline__ void conv_c8_body(const C8ArgsPair &ap, const int nb0, const int nblocks, const int bid, char *const lds) {
    static_assert(PASSES >= 1 && PASSES <= 3, "passes");
    constexpr int NW = WM * WN;
    constexpr int TR = WN * NF;                      // output rows per block
    constexpr int PR = TR + 2;
    constexpr int NPP = PR * C8_PC;                  // patch pixels
    constexpr int NU = NPP * 4;                      // 16-byte units per chunk: (2 k8 groups) x (hi, lo)
    constexpr int NPR = (NU + 63) / 64;              // 1-KiB DMA pieces that carry data
    constexpr int NIA = (NPR + NW - 1) / NW;         // activation DMA pieces per wave and chunk (every wave issues the same
                                                     // number -- the vmcnt waits count them; surplus pieces land in one slack KiB)
    constexpr int ACT_BYTES = (NIA * NW > NPR ? NPR + 1 : NPR) * 1024;
    constexpr int WSLOT = WM * 4096;
    constexpr int WPI = (WM * 4) / NW;               // weight DMA pieces per wave and step
    static_assert((WM * 4) % NW == 0, "weight image must split evenly over the waves");
    constexpr int MF = 2;
    char *const lds_act = lds;                       // act[2][ACT_BYTES] | wring[RING][WSLOT]
    char *const lds_w = lds + 2 * ACT_BYTES;

    const bool second = bid >= nb0;
    const C8Args &a = ap.p[second ? 1 : 0];
    const int blk_first = second ? nb0 : 0;
    const int blk_count = second ? nblocks - nb0 : nb0;
    if (blk_count <= 0 || bid - blk_first >= a.total_tiles) return;      // (a guard: c8_launch gives no problem more blocks than tiles)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WM, wn = wave / WM;
    const int li = lane & 31, kg = lane >> 5;

    auto decode = [&](int t, int &th0, int &tw0, int &tco, int &tb) {
        const int xy = t % a.tiles_xy, r = t / a.tiles_xy;
        tw0 = (xy % a.tiles_w) * 32;
        th0 = (xy / a.tiles_w) * TR;
        tco = (r % a.n_co) * (64 * WM);
        tb = r / a.n_co;
    };
    int h0, w0, co_blk, b;
    int tile = bid - blk_first;       // (the XCD-aware order of the fused ConvGRU launch measured -0.6 % here: r05_cfg_variants.txt)
    decode(tile, h0, w0, co_blk, b);

    // ---- activation DMA (c8_pipe.h): the source offset of a lane inside the chunk's 4 planes is fixed per tile.
    unsigned aoff_cur[NIA], aoff_nxt[NIA];
    auto tile_offsets = [&](int th0, int tw0, unsigned (&off)[NIA]) {
        c8_tile_offsets<NW, NPP, NU>(a, wave, lane, th0, tw0, off);
    };
    auto chunk_base = [&](int tb, int chunk) -> const char * {       // wave-uniform
        int s = 0, c = chunk;
        while (s + 1 < a.nsrc && c >= a.src_n16[s]) {
            c -= a.src_n16[s];
            ++s;
        }
        return a.src[s] + (long)tb * a.src_bs[s] + (long)c * 4 * a.plane_bytes;
    };
    auto issue_act = [&](const char *base, const unsigned (&off)[NIA], int buf) {
        c8_issue_act<NW, NPR>(wave, base, off, lds_act + buf * ACT_BYTES);
    };
    // ---- weight DMA: the step image of this block's WM co64 blocks is contiguous (WM * 4 KB)
    // The images of consecutive steps of one tile are wstep bytes apart ((chunk, tap) is the outer index).
    auto w_tile = [&](int tco) -> const char * {
        int c64 = tco >> 6;
        c64 = c64 + WM <= a.n_co64 ? c64 : 0;                // blocks past the padded channel count idle on valid data
        return a.w + (long)c64 * 4096;
    };
    const long wstep = (long)a.n_co64 * 4096;
    auto issue_w = [&](const char *img, int slot) {
        char *dst = lds_w + slot * WSLOT;
#pragma unroll
        for (int j = 0; j < WPI; ++j) {
            const int p = wave * WPI + j;
            __builtin_amdgcn_global_load_lds((const void *)(img + p * 1024 + lane * 16),
                                             (__attribute__((address_space(3))) void *)(dst + p * 1024), 16, 0, 0);
        }
    };

    f32x16 acc[MF][NF];
    auto zero_acc = [&]() {
#pragma unroll
        for (int m = 0; m < MF; ++m)
#pragma unroll
            for (int n = 0; n < NF; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.0f;
    };
    zero_acc();

    // fragment addresses: A = slot + wm*4096 + hl*2048 + kg*1024 + (m*32 + li)*16
    //                     B = act + ((2 kg + hl) * NPP + (wn*NF + n + dy) * 34 + li + dx) * 16
    const int a_lane = wm * 4096 + kg * 1024 + li * 16;
    const int b_lane = (2 * kg * NPP + wn * NF * C8_PC + li) * 16;
    f16x8 Ahi[MF], Alo[MF], Bhi[NF + 2], Blo[NF + 2];      // B: one fragment per patch ROW of the current tap column (see C8_STEP3, c8_pipe.h)
    const unsigned lds_w_addr = (unsigned)(size_t)(__attribute__((address_space(3))) char *)lds_w + a_lane;
    const unsigned lds_b_addr = (unsigned)(size_t)(__attribute__((address_space(3))) char *)lds_act + b_lane;
    // The (chunk, tap) steps are c8_pipe.h's, with both 32-channel blocks of the wave (MFP = MF = 2); what this kernel supplies:
#define C8_ACC(m, n) acc[m][n]
#define C8_WBASE lds_w_addr
    // the weights of step s+1 (issued RING-2 steps ago) and, from step 6 on, the following chunk's patch
    // have landed once at most the pieces issued after them are outstanding
#define C8_WAIT_DMA(T)                                                                                                 \
        if ((T) >= 1 && (T) <= RING - 3) c8_wait_vm<(RING - 3) * WPI + NIA>();                                         \
        else c8_wait_vm<(RING - 3) * WPI>();
    // the image of step s+RING-1 into the slot of step s-1 (all of its reads were consumed before this step's barrier);
    // at the chunk's first step also the following chunk's patch
#define C8_ISSUE_DMA(T)                                                                                                \
        if ((T) == 10 - RING && !in_tile) wptr = w_next; /* the stream continues with the next tile's first image */  \
        if ((T) == 0) { /* (before the weights: the patch must be older than every image the waits let fly) */        \
            if (in_tile || !have_next) issue_act(act_f, aoff_cur, nxt);                                                \
            else issue_act(act_f, aoff_nxt, nxt);                                                                      \
        }                                                                                                              \
        issue_w(wptr, sl2);                                                                                            \
        wptr += wstep;

    // ------------------------------------------------------------------------------------------------
    // epilogue (after the tile's last step; the next tile's first DMA pieces are already in flight)
    // ------------------------------------------------------------------------------------------------
    // A lane holds, per accumulator block (m, n), 16 values v[r]: channel (r&3) + 8*(r>>2) + 4*kg of its block, pixel
    // (row n, column li) -- i.e. four groups j = r>>2 of four CONSECUTIVE channels.  fp32 tensors on the epilogue side
    // (gate operands, state, z) may therefore be kept in the "C4" layout [B][C/4][H][W][4]: one 16-byte access per
    // group instead of four strided 4-byte ones (a.f32_c4); NCHW remains for tensors other kernels read.
    // C8S outputs: c8_split_pair completes a pair of groups (j, j+1) to 8 consecutive channels per 16 bytes, after which the
    // lane stores group 2*jp + kg of its block.
    // ARGUMENTS: `a` lives in the kernel-argument segment, so every `a.field` is a scalar load, and with the scalar registers
    // this kernel has left the compiler re-issues that load (and waits for it) at each use instead of keeping the value.  At one
    // wave per SIMD nothing hides those round trips, so the epilogues read what they need ONCE per tile into locals that
    // c8_hold() makes opaque (a value that came out of an asm statement cannot be rematerialised as a load), decide the
    // wave-uniform switches once (epilogue(): one dispatch to bodies specialised at compile time) and address every tensor as
    // wave-uniform base + one 32-bit lane offset per row (the saddr + voffset form: no per-value 64-bit vector arithmetic).
    char *const lds_head = lds + 2 * ACT_BYTES + RING * WSLOT;      // epi 3 only: [wave][NF][9][32] floats
    auto epilogue_head = [&]() __attribute__((always_inline)) {
        // (the arguments of this epilogue, read once per tile: see ARGUMENTS above)
        const int H = c8_hold(a.H), W = c8_hold(a.W);
        const int iHW = c8_hold(H * W);
        const float out_scale = c8_hold(a.out_scale);
        const float *const head_w = c8_hold(a.head_w);
        const float *const bias_p = c8_hold(a.bias);
        float *const head_out = c8_hold(a.head_out + (long)b * a.head_out_bs + (long)(co_blk / (64 * WM)) * 9 * iHW);
        const int co_w = c8_hold(co_blk + wm * 64);
        const bool idle = c8_hold((int)(co_w >= a.n_co64 * 64)) != 0;
        float *red = (float *)lds_head;
        int kgo = kg;                          // the lane's channel half, opaque from here on: nothing derived from it
        asm volatile("" : "+v"(kgo));          // can be pre-computed at kernel entry and kept live (spilled) through the main loop
        // ONE output (stereo: the x component / the disparity), two tile rows at a time: the accumulators, the next tile's
        // prefetched fragments and 18 partial sums fit the register file (all NF rows at once, or a loop over outputs that
        // keeps every accumulator live, spilled 250-400 registers)
        constexpr int NH = NF > 1 ? 2 : 1;
#pragma unroll
        for (int n0 = 0; n0 < NF; n0 += NH) {
            float P[NH][9];
#pragma unroll
            for (int n = 0; n < NH; ++n)
#pragma unroll
                for (int t = 0; t < 9; ++t) P[n][t] = 0.0f;
            if (!idle) {
#pragma unroll
                for (int m = 0; m < MF; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        // channel co = cu + 4 kg: wave-uniform base pointers + one lane offset (Cout is a multiple of 64 here)
                        const int cu = co_w + m * 32 + (r & 3) + 8 * (r >> 2);
                        const float *wp = head_w + (long)cu * 12 + kgo * 48;
                        const float4 w0 = *(const float4 *)wp, w1 = *(const float4 *)(wp + 4);
                        const float w8 = wp[8];
                        const float wt[9] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w8};
                        const float bias = bias_p[cu + 4 * kgo];                 // (bias is mandatory here: a branch per channel wrecks the allocation)
#pragma unroll
                        for (int n = 0; n < NH; ++n) {
                            const float v = dkt_relu(acc[m][n0 + n][r] * out_scale + bias);
#pragma unroll
                            for (int t = 0; t < 9; ++t) P[n][t] = __fmaf_rn(wt[t], v, P[n][t]);
                        }
                        __builtin_amdgcn_sched_barrier(0);       // one channel at a time: no hoisting of all the weight loads
                    }
            }
            // the two half-waves hold different channels of the same pixels
#pragma unroll
            for (int n = 0; n < NH; ++n)
#pragma unroll
                for (int t = 0; t < 9; ++t) P[n][t] = __fadd_rn(P[n][t], __shfl_xor(P[n][t], 32));
            if (kg == 0) {
#pragma unroll
                for (int n = 0; n < NH; ++n)
#pragma unroll
                    for (int t = 0; t < 9; ++t) red[((wave * NF + n0 + n) * 9 + t) * 32 + li] = P[n][t];
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        // wave (wm = 0, wn) sums the WM channel quarters of its rows in wave order and writes the planes
        if (wm == 0) {
            for (int item = lane; item < NF * 9 * 32; item += 64) {
                const int px = item & 31, t = (item >> 5) % 9, n = item / (9 * 32);
                float sum = red[(((0 + WM * wn) * NF + n) * 9 + t) * 32 + px];
#pragma unroll
                for (int q = 1; q < WM; ++q) sum = __fadd_rn(sum, red[(((q + WM * wn) * NF + n) * 9 + t) * 32 + px]);
                const int oh = h0 + wn * NF + n, ow = w0 + px;
                if (oh < H && ow < W) head_out[(long)t * iHW + (long)oh * W + ow] = sum;
            }
        }
        __builtin_amdgcn_s_barrier();                            // `red` is free again before the next tile's epilogue
    };
    auto epilogue = [&]() __attribute__((always_inline)) {
        const int epi = c8_hold(a.epi);
        if constexpr (NW == 8) {                 // (the two 8-wave shapes carry the head epilogue; round 4: in the NF = 4
            if (epi == 3) {                      //  shapes its code costs hundreds of spilled registers)
                epilogue_head();
                return;
            }
        }
        const int Cout = c8_hold(a.Cout);
        const int co_w = c8_hold(co_blk + wm * 64);
        if (co_w >= a.n_co64 * 64) return;                   // idle wave
        // ---- per tile: every argument this epilogue needs, read once and held (see ARGUMENTS above)
        const int H = c8_hold(a.H), W = c8_hold(a.W);
        const int iHW = c8_hold(H * W);
        const int Ch = epi == 1 ? Cout / 2 : Cout;           // channels of the destination tensors
        const bool rpart = epi == 1 && co_w >= Ch;           // wave-uniform: this wave owns r channels
        const int cw = c8_hold(co_w - (rpart ? Ch : 0));     // first channel of this wave inside the Ch-wide tensors
        const float out_scale = c8_hold(a.out_scale), act_scale = c8_hold(a.act_scale);
        const float *const bias_p = c8_hold(a.bias);
        // wave-uniform selections
        const float *const pc = c8_hold(epi ? (rpart ? a.e_c1 + (long)b * a.e_c1_bs : a.e_c0 + (long)b * a.e_c0_bs) : nullptr);
        const float *const pz = c8_hold(epi == 2 ? a.e_c1 + (long)b * a.e_c1_bs : nullptr);
        const float *const ph = c8_hold((epi == 2 || rpart) ? a.e_h + (long)b * a.e_h_bs : nullptr);
        float *const po = c8_hold(rpart ? (a.out2 ? a.out2 + (long)b * a.out2_bs : nullptr) : (a.out ? a.out + (long)b * a.out_bs : nullptr));
        char *const pc8 = c8_hold(rpart ? (a.out2_c8 ? a.out2_c8 + (long)b * a.out2_c8_bs : nullptr)
                                        : (a.out_c8 ? a.out_c8 + (long)b * a.out_c8_bs : nullptr));
        const int tail_ch = c8_hold(epi == 0 && a.tail ? a.tail_ch : 0);
        const float *const ptail = c8_hold(tail_ch > 0 ? a.tail + (long)b * a.tail_bs : nullptr);
        const float tail_ratio = c8_hold(a.tail_ratio);
        const int c8_ch0 = rpart ? a.out2_c8_ch0 : a.out_c8_ch0;
        const int c8_g0 = c8_hold((c8_ch0 + cw) >> 3);                      // first 8-channel group of this wave in the C8S destination
        const int c8_gend = c8_hold(2 * ((c8_ch0 + Ch + tail_ch + 15) / 16));   // 8-channel groups the C8S destination holds
        const unsigned c8_plane = c8_hold((unsigned)a.out_c8_plane);        // (3 planes + a pixel fit 32 bits: the patch DMA offsets need that too)
        const int c8_Wp = c8_hold(a.out_c8_Wp);
        const int relu = c8_hold(a.relu), c4 = c8_hold(a.f32_c4);
        // lane parts of the addresses: the lane's channel half (fp32: 4 kg channels = kg quads, 16 kg iHW bytes in both layouts)
        // and column; a row adds wave-uniform terms
        const unsigned kg_f32 = (unsigned)kg * 16u * (unsigned)iHW;
        const unsigned kg_c8 = (unsigned)kg * 2u * c8_plane;
        const int ow = w0 + li;
        const bool col_in = ow < W;

        // EPI: epilogue kind; C4: layout of the fp32 tensors; RPART (kind 1): the wave owns r channels.  ReLU is a select on a held
        // flag; kinds 0 and 4 (the only ones whose channel count is free) test channels against the layer's last one per lane,
        // and only their groups that can reach it (`rag`, wave-uniform) take the paths that differ: tail copy, clamped loads.
        auto body = [&](auto kEpi, auto kC4, auto kRpart) __attribute__((always_inline)) {
            constexpr int EPI = decltype(kEpi)::value;
            constexpr bool C4 = decltype(kC4)::value != 0, RPART = decltype(kRpart)::value != 0;
            constexpr bool FREE = EPI == 0 || EPI == 4;          // any channel count: lanes may hold channels that do not exist
            constexpr bool LOAD_C = EPI != 0, LOAD_H = EPI == 2 || RPART, LOAD_Z = EPI == 2;
            constexpr unsigned PXB = C4 ? 16u : 4u;              // bytes per pixel step
            // address of channel cs + i (cs a multiple of 4) of an fp32 tensor; the lane adds `loff` bytes.  f32_at: wave-uniform
            // and held, so that the access keeps the form scalar base + 32-bit lane offset (left to itself the compiler moves
            // the lane offset into the base once per tile and adds the channel term with 64-bit vector arithmetic)
            auto f32_lane = [&](const float *base, int cs, int i) -> const char * {
                return (const char *)base + (C4 ? (long)(cs >> 2) * iHW * 16 : (long)(cs + i) * iHW * 4);
            };
            auto f32_at = [&](const float *base, int cs, int i) -> const char * { return c8_base(f32_lane(base, cs, i)); };
            auto load4 = [&](const float *base, int cs, unsigned loff, float (&v)[4]) {
                if constexpr (C4) {
                    const float4 t = *(const float4 *)(f32_at(base, cs, 0) + loff);
                    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = *(const float *)(f32_at(base, cs, i) + loff);
                }
            };
            auto load4_lane = [&](const float *base, int cs, unsigned loff, float (&v)[4]) {      // cs differs between lanes
                if constexpr (C4) {
                    const float4 t = *(const float4 *)(f32_lane(base, cs, 0) + loff);
                    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = *(const float *)(f32_lane(base, cs, i) + loff);
                }
            };
#pragma unroll
            for (int m = 0; m < MF; ++m) {
                float bv[16];                                      // this lane's 16 biases of block m
                if (bias_p) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int cu = co_w + m * 32 + (r & 3) + 8 * (r >> 2);      // the lane's channel is cu + 4 kg
                        if constexpr (FREE) {
                            const int co = cu + 4 * kg;
                            bv[r] = bias_p[co < Cout ? co : Cout - 1];
                        } else bv[r] = ((const float *)((const char *)c8_base(bias_p + (cu & ~3)) + (unsigned)kg * 16u))[r & 3];
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) bv[r] = 0.0f;
                }
#pragma unroll
                for (int n = 0; n < NF; ++n) {
                    const int oh = h0 + wn * NF + n;               // wave-uniform
                    const bool inside = oh < H && col_in;
                    const unsigned px = inside ? (unsigned)(oh * W + ow) : 0u;
                    const unsigned loff = kg_f32 + px * PXB;
                    // The fp32 operands of the fused epilogues (gate terms, state, residual) of all four channel groups of this
                    // accumulator block are fetched BEFORE the block's first store.  Interleaved with the stores, as they were, a
                    // group's loads waited behind the previous group's stores (a load cannot move above a store that may alias
                    // it): the epilogue was a chain of memory round trips -- counters of an epilogue-only launch: 57 % of the wave
                    // cycles in s_waitcnt (tools/c8_epi_pmc.sh) -- 32 per wave, 8 now.  The registers come from the next tile's
                    // prefetched fragments, which are re-read after the epilogue instead of being held across it.
                    float gca[4][4], gha[4][4], gza[4][4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int cs = cw + m * 32 + 8 * j;        // the lane's 4 channels start at cs + 4 kg
                        if constexpr (LOAD_C) {
                            if (FREE && cs + 8 > Ch) {             // channels past the layer's last read channel 0 (and are not used)
                                const bool ok = cs + 4 * kg < Ch;
                                load4_lane(pc, ok ? cs : 0, ok ? loff : px * PXB, gca[j]);
                            } else load4(pc, cs, loff, gca[j]);
                        }
                        if constexpr (LOAD_H) load4(ph, cs, loff, gha[j]);
                        if constexpr (LOAD_Z) load4(pz, cs, loff, gza[j]);
                    }
#pragma unroll
                    for (int jp = 0; jp < 2; ++jp) {
                        float v[2][4];
#pragma unroll
                        for (int jj = 0; jj < 2; ++jj) {
                            const int j = 2 * jp + jj;
                            const int cs = cw + m * 32 + 8 * j;
                            const int cl = cs + 4 * kg;            // first of this lane's 4 channels (destination numbering)
                            const bool rag = FREE && cs + 8 > Ch;  // wave-uniform: this group reaches past the last channel
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const float x = acc[m][n][4 * j + i] * out_scale + bv[4 * j + i];
                                if constexpr (EPI == 0) {
                                    v[jj][i] = relu ? dkt_relu(x) : x;
                                } else if constexpr (EPI == 1) {
                                    const float g = c8_sigmoid(__fadd_rn(x, gca[j][i]));
                                    v[jj][i] = RPART ? __fmul_rn(g, gha[j][i]) : g;
                                } else if constexpr (EPI == 4) {
                                    // residual join of core/extractor.py:52-60: relu(x + [relu](conv + bias)); padded channels stay 0
                                    const float t = relu ? dkt_relu(x) : x;
                                    v[jj][i] = dkt_relu(__fadd_rn(gca[j][i], t));
                                } else {
                                    const float q = c8_tanh(__fadd_rn(x, gca[j][i]));
                                    v[jj][i] = __fadd_rn(__fmul_rn(__fsub_rn(1.0f, gza[j][i]), gha[j][i]), __fmul_rn(gza[j][i], q));
                                }
                            }
                            if constexpr (FREE) {
                                if (rag) {
#pragma unroll
                                    for (int i = 0; i < 4; ++i) {
                                        if (cl + i >= Cout) {
                                            float y = 0.0f;
                                            if constexpr (EPI == 0) {      // (tail_ch is 0 where the layer has no tail)
                                                if (cl + i < Cout + tail_ch && inside) y = ptail[(long)(cl + i - Cout) * iHW + px] * tail_ratio;
                                            }
                                            v[jj][i] = y;
                                        }
                                    }
                                }
                            }
                            if (po) {                              // (wave-uniform, per group of four values)
                                if constexpr (C4) {                // (C4 tensors are padded to 4 channels)
                                    if (inside && (!FREE || cl < Ch))
                                        *(float4 *)(const_cast<char *>(f32_at(po, cs, 0)) + loff) = make_float4(v[jj][0], v[jj][1], v[jj][2], v[jj][3]);
                                } else {
#pragma unroll
                                    for (int i = 0; i < 4; ++i)
                                        if (inside && (!FREE || cl + i < Ch)) *(float *)(const_cast<char *>(f32_at(po, cs, i)) + loff) = v[jj][i];
                                }
                            }
                        }
                        if (pc8) {
                            // C8S: c8_split_pair completes the pair of groups to 8 consecutive channels per 16 bytes, after which the
                            // lane stores group 2 jp + kg of its block
                            u32x4 hi, lo;
                            c8_split_pair(v[0], v[1], act_scale, hi, lo);
                            const int gs = c8_g0 + m * 4 + 2 * jp;     // wave-uniform; the lane's group is gs + kg
                            // (groups past the destination's padded channel count do not exist)
                            if (inside && (!FREE || gs + kg < c8_gend)) {
                                char *const p = pc8 + (long)gs * 2 * c8_plane;
                                const unsigned off = kg_c8 + (unsigned)((oh + 1) * c8_Wp + (ow + 1)) * 16u;
                                *(u32x4 *)(c8_base(p) + off) = hi;
                                *(u32x4 *)(c8_base(p + c8_plane) + off) = lo;
                            }
                        }
                    }
                }
            }
        };
        // ---- the one dispatch of the tile
        constexpr C8Tag<0> k0{};
        constexpr C8Tag<1> k1{};
        constexpr C8Tag<2> k2{};
        constexpr C8Tag<4> k4{};
        auto by_c4 = [&](auto kEpi, auto kRpart) __attribute__((always_inline)) {
            if (c4) body(kEpi, k1, kRpart);
            else body(kEpi, k0, kRpart);
        };
        if (epi == 0) by_c4(k0, k0);
        else if (epi == 1) {
            if (rpart) by_c4(k1, k1);
            else by_c4(k1, k0);
        } else if (epi == 2) by_c4(k2, k0);
        else by_c4(k4, k0);
    };

    // ------------------------------------------------------------------------------------------------
    // main stream
    // ------------------------------------------------------------------------------------------------
    tile_offsets(h0, w0, aoff_cur);
    // prologue: chunk 0's patch and the weight images of steps 0..2
    issue_act(chunk_base(b, 0), aoff_cur, 0);
    const char *wptr = w_tile(co_blk);          // image of the next step to fetch
#pragma unroll
    for (int s = 0; s < RING - 1; ++s) {
        issue_w(wptr, s);
        wptr += wstep;
    }
    c8_wait_vm<0>();
    __builtin_amdgcn_s_barrier();
    // the fragments of step 0 that the steps do not fetch themselves (C8_FIRST_FRAGS, c8_pipe.h)
    int g = 0;              // chunks consumed by this block: activation buffer parity
    int sl = 0;             // ring slot of the step being computed
    C8_FIRST_FRAGS(MF, 0)
    for (;;) {
        const int tn = tile + blk_count;
        const bool have_next = tn < a.total_tiles;
        int nh0 = h0, nw0 = w0, nco = co_blk, nb = b;
        if (have_next) decode(tn, nh0, nw0, nco, nb);
#define C8_CHUNK_SETUP(c)                                                                                     \
            const bool in_tile = (c) + 1 < a.nchunks;                                                             \
            /* the chunk that follows in this block's stream: this tile's next one, else the next tile's first, */ \
            /* else (the block's very last chunk) this one again, harmlessly */                                   \
            const int c_f = in_tile ? (c) + 1 : (have_next ? 0 : (c));                                            \
            const char *w_next = w_tile(have_next ? nco : co_blk);                                                \
            const int b_f = in_tile ? b : nb;                                                                     \
            if (!in_tile && have_next) tile_offsets(nh0, nw0, aoff_nxt);                                          \
            const char *act_f = chunk_base(b_f, c_f);                                                             \
            const int cur = g & 1, nxt = cur ^ 1;
        if constexpr (PASSES == 1) {
            for (int c = 0; c < a.nchunks; c += 2) {
                { C8_CHUNK_SETUP(c) C8_CHUNK1(MF, Ahi, Alo) }
                ++g;
                { C8_CHUNK_SETUP(c + 1) C8_CHUNK1(MF, Alo, Ahi) }
                ++g;
            }
        } else {
            for (int c = 0; c < a.nchunks; ++c, ++g) {
                C8_CHUNK_SETUP(c)
                C8_CHUNK(MF)
            }
        }
        c8_wait_lgkm<0>();      // the prefetched fragments of the next tile have landed: their registers are stable
        epilogue();
        if (!have_next) break;
        tile = tn; h0 = nh0; w0 = nw0; co_blk = nco; b = nb;
#pragma unroll
        for (int j = 0; j < NIA; ++j) aoff_cur[j] = aoff_nxt[j];
        zero_acc();
        // The fragments the last step fetched for this tile's first step are fetched AGAIN here (their LDS images are
        // untouched: no DMA is issued during the epilogue): that makes the 16 + 8 NF fragment registers dead across the
        // epilogue, which needs them for its operand batches (see epilogue()).
        C8_FIRST_FRAGS(MF, g)
    }
    c8_wait_vm<0>();        // no DMA may land in this block's LDS after it has been released
}

template <int WM, int WN, int NF, int RING, int PASSES = 3>
__global__ __launch_bounds__(64 * WM * WN, (WM * WN > 4 ? 1 : 2)) void conv_c8_kernel(C8ArgsPair ap, int nb0) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    conv_c8_body<WM, WN, NF, RING, PASSES>(ap, nb0, (int)gridDim.x, (int)blockIdx.x, lds);
}

// ---- launch
template <int WM, int WN, int NF, int RING, int PASSES = 3>
static int c8_launch(C8Args a, int B, hipStream_t st, const C8Args *second, int B2) {
    constexpr int NW = WM * WN, TR = WN * NF;
    constexpr int NU = (TR + 2) * C8_PC * 4;
    constexpr int NPR = (NU + 63) / 64, NIA = (NPR + NW - 1) / NW;
    size_t lds = (size_t)2 * (NIA * NW > NPR ? NPR + 1 : NPR) * 1024 + (size_t)RING * WM * 4096;
    const bool head = a.epi == 3 || (second && second->epi == 3);
    if (head) {
        if (NW != 8) return DKT_E_UNSUPPORTED;                // one block per CU: the extra LDS costs no residency
        lds += (size_t)NW * NF * 9 * 32 * 4;
    }
    auto kern = conv_c8_kernel<WM, WN, NF, RING, PASSES>;
    static int slots[64] = {0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (!slots[dev & 63]) {
        size_t want = lds + (NW == 8 && !head ? (size_t)NW * NF * 9 * 32 * 4 : 0);     // (room for a later head launch of this shape)
        if (want > 160 * 1024) want = lds;
        hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want);
        if (e != hipSuccess) return (int)e;
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 64 * NW, lds) != hipSuccess || per_cu < 1) per_cu = 1;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
        slots[dev & 63] = per_cu * cus;
    }
    auto shape = [&](C8Args &x, int nb) -> long {
        x.tiles_w = (x.W + 31) / 32;
        x.tiles_xy = x.tiles_w * ((x.H + TR - 1) / TR);
        x.n_co = (x.n_co64 + WM - 1) / WM;
        const long total = (long)x.tiles_xy * x.n_co * nb;
        x.total_tiles = (int)total;
        return total;
    };
    const long cap = slots[dev & 63];
    C8ArgsPair ap;
    const long total0 = shape(a, B);
    if (total0 > 0x7fffffffL) return DKT_E_SHAPE;
    ap.p[0] = a;
    ap.p[1] = a;
    long nb0 = total0 > cap ? cap : total0, nb1 = 0;
    if (second) {
        C8Args b = *second;
        const long total1 = shape(b, B2);
        if (total1 > 0x7fffffffL) return DKT_E_SHAPE;
        ap.p[1] = b;
        nb0 = total0; nb1 = total1;
        if (total0 + total1 > cap) {
            const double w0 = (double)total0 * a.nchunks, w1 = (double)total1 * b.nchunks;
            nb1 = (long)(cap * w1 / (w0 + w1) + 0.5);
            nb1 = nb1 < 1 ? 1 : (nb1 > total1 ? total1 : nb1);
            nb0 = cap - nb1;
            if (nb0 > total0) nb0 = total0;
            if (nb0 < 1) nb0 = 1;
        }
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)(nb0 + nb1)), dim3(64 * NW), lds, st, ap, (int)nb0);
    return dkt_launch_status();
}


// cfg: 0 = by shape; 1: 256 co x 8 rows (8 waves); 2: 128 co x 8 rows (8 waves); 3: 64 co x 8 rows (4 waves, two blocks per CU);
//      4: 64 co x 4 rows (4 waves); 5: 256 co x 4 rows (4 waves, two blocks per CU); 6: 128 co x 8 rows (4 waves, two blocks per CU)
template <int PASSES>
int c8_dispatch_p(const C8Args &a, int B, int cfg, hipStream_t st, const C8Args *second, int B2) {
    switch (cfg) {
    case 1: return c8_launch<4, 2, 4, 4, PASSES>(a, B, st, second, B2);
    case 2: return c8_launch<2, 4, 2, 4, PASSES>(a, B, st, second, B2);
    case 3: return c8_launch<1, 4, 2, 6, PASSES>(a, B, st, second, B2);
    case 4: return c8_launch<1, 4, 1, 8, PASSES>(a, B, st, second, B2);
    default: break;
    }
    if constexpr (PASSES == 3) {          // (the 4-wave forms kept for the tests exist at full precision only)
        if (cfg == 5) return c8_launch<4, 1, 4, 3>(a, B, st, second, B2);
        if (cfg == 6) return c8_launch<2, 2, 4, 4>(a, B, st, second, B2);
    }
    return DKT_E_UNSUPPORTED;
}

#if C8_TU == -1 || C8_TU == 1
template int c8_dispatch_p<1>(const C8Args &, int, int, hipStream_t, const C8Args *, int);
#endif
#if C8_TU == -1 || C8_TU == 2
template int c8_dispatch_p<2>(const C8Args &, int, int, hipStream_t, const C8Args *, int);
#endif
#if C8_TU == -1 || C8_TU == 3
template int c8_dispatch_p<3>(const C8Args &, int, int, hipStream_t, const C8Args *, int);
#endif
#endif      // C8_TU != 0

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
#if C8_TU <= 0
// (defined in the units that hold the kernel)
template <int PASSES>
int c8_dispatch_p(const C8Args &a, int B, int cfg, hipStream_t st, const C8Args *second, int B2);

static int c8_round(int x, int m) { return (x + m - 1) / m * m; }

extern "C" int dkt_act_c8_dims(int H, int W, int *Hp, int *Wp) {
    if (H <= 0 || W <= 0 || !Hp || !Wp) return DKT_E_SHAPE;
    *Hp = c8_round(H, 8) + 2;
    *Wp = c8_round(W, 32) + 2;
    return DKT_OK;
}

// fp32 NCHW -> C8S (interior only: the border and the padding channels of the destination must be zero already)
__global__ __launch_bounds__(256) void act_c8_pack_kernel(const float *x, long x_bs, char *dst, long dst_bs, int C, int H, int W,
                                                          int Wp, long plane, int ch0, float scale) {
    const int g = blockIdx.y, b = blockIdx.z;                 // 8-channel group of the source
    const long HW = (long)H * W;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < HW; i += (long)gridDim.x * 256) {
        const int oh = (int)(i / W), ow = (int)(i - (long)oh * W);
        unsigned hw[4], lw[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int c0 = g * 8 + 2 * d;
            const float x0 = c0 < C ? x[(long)b * x_bs + (long)c0 * HW + i] * scale : 0.0f;
            const float x1 = c0 + 1 < C ? x[(long)b * x_bs + (long)(c0 + 1) * HW + i] * scale : 0.0f;
            const _Float16 a0 = (_Float16)x0, a1 = (_Float16)x1;
            hw[d] = c8_pack_h2(a0, a1);
            lw[d] = c8_pack_h2((_Float16)(x0 - (float)a0), (_Float16)(x1 - (float)a1));
        }
        char *p = dst + (long)b * dst_bs + (long)((ch0 >> 3) + g) * 2 * plane + ((long)(oh + 1) * Wp + (ow + 1)) * 16;
        *(uint4 *)p = make_uint4(hw[0], hw[1], hw[2], hw[3]);
        *(uint4 *)(p + plane) = make_uint4(lw[0], lw[1], lw[2], lw[3]);
    }
}

__global__ __launch_bounds__(256) void act_c8_unpack_kernel(const char *src, long src_bs, float *y, long y_bs, int C, int H, int W,
                                                            int Wp, long plane, int ch0, float inv_scale) {
    const int g = blockIdx.y, b = blockIdx.z;
    const long HW = (long)H * W;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < HW; i += (long)gridDim.x * 256) {
        const int oh = (int)(i / W), ow = (int)(i - (long)oh * W);
        const char *p = src + (long)b * src_bs + (long)((ch0 >> 3) + g) * 2 * plane + ((long)(oh + 1) * Wp + (ow + 1)) * 16;
        const f16x8 hi = *(const f16x8 *)p, lo = *(const f16x8 *)(p + plane);
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (g * 8 + k < C) y[(long)b * y_bs + (long)(g * 8 + k) * HW + i] = ((float)hi[k] + (float)lo[k]) * inv_scale;
    }
}

extern "C" int dkt_act_c8_pack(const float *x, long x_bstride, void *dst, long dst_bstride_bytes, int B, int C, int H, int W,
                               int ch0, float scale, int device, void *stream) {
    if (!x || !dst) return DKT_E_NULL;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || B > 65535 || (ch0 & 7)) return DKT_E_SHAPE;
    int Hp, Wp;
    dkt_act_c8_dims(H, W, &Hp, &Wp);
    DKT_ENTER(device);
    const long HW = (long)H * W;
    dim3 grid((unsigned)((HW + 255) / 256 > 1024 ? 1024 : (HW + 255) / 256), (unsigned)((C + 7) / 8), (unsigned)B);
    hipLaunchKernelGGL(act_c8_pack_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, x_bstride, (char *)dst, dst_bstride_bytes,
                       C, H, W, Wp, (long)Hp * Wp * 16, ch0, scale);
    return dkt_launch_status();
}

extern "C" int dkt_act_c8_unpack(const void *src, long src_bstride_bytes, float *y, long y_bstride, int B, int C, int H, int W,
                                 int ch0, float scale, int device, void *stream) {
    if (!src || !y) return DKT_E_NULL;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || B > 65535 || (ch0 & 7) || !(scale > 0.0f)) return DKT_E_SHAPE;
    int Hp, Wp;
    dkt_act_c8_dims(H, W, &Hp, &Wp);
    DKT_ENTER(device);
    const long HW = (long)H * W;
    dim3 grid((unsigned)((HW + 255) / 256 > 1024 ? 1024 : (HW + 255) / 256), (unsigned)((C + 7) / 8), (unsigned)B);
    hipLaunchKernelGGL(act_c8_unpack_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const char *)src, src_bstride_bytes, y,
                       y_bstride, C, H, W, Wp, (long)Hp * Wp * 16, ch0, 1.0f / scale);
    return dkt_launch_status();
}

// ---- weights: (Cout, Cin, 3, 3) fp32 -> [chunk][tap][co64][hi|lo][k8][64 co][8] fp16, sources padded to 16 channels
struct C8PackArgs {
    const float *w;
    _Float16 *dst;
    int Cout, Cin, n_co64, nchunks;
    int src_ch[C8_MAX_SRC];
    int nsrc;
    float scale;
};

__global__ __launch_bounds__(256) void conv_c8_pack_kernel(C8PackArgs a) {
    const long total = (long)a.nchunks * 9 * a.n_co64 * 2048;       // halfs
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= total) return;
    const int k = (int)(i & 7);
    const int co_in = (int)((i >> 3) & 63);
    const int k8 = (int)((i >> 9) & 1);
    const int hl = (int)((i >> 10) & 1);
    long r = i >> 11;
    const int c64 = (int)(r % a.n_co64); r /= a.n_co64;
    const int tp = (int)(r % 9);
    const int tap = (tp % 3) * 3 + tp / 3;      // step order is dx-major: image tp holds tap (dy = tp % 3, dx = tp / 3)
    const int chunk = (int)(r / 9);
    int pc = chunk * 16 + k8 * 8 + k, s = 0, cbase = 0;
    while (s + 1 < a.nsrc && pc >= ((a.src_ch[s] + 15) & ~15)) {
        pc -= (a.src_ch[s] + 15) & ~15;
        cbase += a.src_ch[s];
        ++s;
    }
    const int co = c64 * 64 + co_in;
    float v = 0.0f;
    if (co < a.Cout && pc < a.src_ch[s]) v = a.w[((long)co * a.Cin + cbase + pc) * 9 + tap] * a.scale;
    const _Float16 hi = (_Float16)v;
    a.dst[i] = hl ? (_Float16)(v - (float)hi) : hi;
}

static int c8_chunks(const int *src_ch, int nsrc) {
    int t = 0;
    for (int s = 0; s < nsrc; ++s) t += (src_ch[s] + 15) / 16;
    return t;
}

extern "C" long dkt_conv_c8_packed_bytes(const int *src_channels, int nsrc, int Cout) {
    if (!src_channels || nsrc < 1 || nsrc > C8_MAX_SRC || Cout <= 0) return DKT_E_SHAPE;
    // + 12 KB of slack: a block always copies its tile shape's full 4 x 64 channel step image, also where the layer has fewer
    // channel blocks (the surplus waves idle on whatever follows)
    return (long)c8_chunks(src_channels, nsrc) * 9 * ((Cout + 63) / 64) * 4096 + 3 * 4096;
}

extern "C" int dkt_conv_c8_pack_weights(const float *w, const int *src_channels, int nsrc, int Cout, float scale,
                                        void *packed, int device, void *stream) {
    if (!w || !src_channels || !packed) return DKT_E_NULL;
    if (nsrc < 1 || nsrc > C8_MAX_SRC || Cout <= 0 || !(scale > 0.0f)) return DKT_E_SHAPE;
    C8PackArgs a;
    a.w = w; a.dst = (_Float16 *)packed; a.Cout = Cout; a.Cin = 0; a.nsrc = nsrc; a.scale = scale;
    for (int s = 0; s < C8_MAX_SRC; ++s) {
        a.src_ch[s] = s < nsrc ? src_channels[s] : 0;
        if (s < nsrc && src_channels[s] <= 0) return DKT_E_SHAPE;
        a.Cin += a.src_ch[s];
    }
    a.n_co64 = (Cout + 63) / 64;
    a.nchunks = c8_chunks(src_channels, nsrc);
    DKT_ENTER(device);
    const long total = (long)a.nchunks * 9 * a.n_co64 * 2048;
    hipLaunchKernelGGL(conv_c8_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return dkt_launch_status();
}


static int c8_fill(C8Args &a, const dkt_conv_c8_desc *d) {
    if (!d) return DKT_E_NULL;
    if (d->nsrc < 1 || d->nsrc > C8_MAX_SRC || d->B <= 0 || d->B > 65535 || d->H <= 0 || d->W <= 0 || d->Cout <= 0) return DKT_E_SHAPE;
    if (!d->w || (!d->out && !d->out_c8 && d->epilogue != 1 && d->epilogue != 3)) return DKT_E_NULL;
    if (!(d->out_scale > 0.0f) || !(d->act_scale > 0.0f)) return DKT_E_SHAPE;
    if (d->epilogue < 0 || d->epilogue > 4) return DKT_E_UNSUPPORTED;
    int Hp, Wp;
    dkt_act_c8_dims(d->H, d->W, &Hp, &Wp);
    a.nchunks = 0;
    for (int s = 0; s < C8_MAX_SRC; ++s) {
        a.src[s] = s < d->nsrc ? (const char *)d->src[s] : nullptr;
        a.src_bs[s] = s < d->nsrc ? d->src_bstride[s] : 0;
        a.src_n16[s] = s < d->nsrc ? (d->src_channels[s] + 15) / 16 : 0;
        if (s < d->nsrc && (!d->src[s] || d->src_channels[s] <= 0)) return DKT_E_NULL;
        a.nchunks += a.src_n16[s];
    }
    a.nsrc = d->nsrc;
    a.plane_bytes = (long)Hp * Wp * 16;
    a.Wp = Wp;
    a.w = (const char *)d->w;
    a.n_co64 = (d->Cout + 63) / 64;
    a.bias = d->bias;
    a.out_scale = d->out_scale;
    a.H = d->H; a.W = d->W; a.Cout = d->Cout;
    a.relu = d->relu ? 1 : 0;
    a.epi = d->epilogue;
    a.out = d->out; a.out_bs = d->out_bstride;
    a.out_c8 = (char *)d->out_c8; a.out_c8_bs = d->out_c8_bstride; a.out_c8_plane = a.plane_bytes; a.out_c8_Wp = Wp;
    a.out_c8_ch0 = d->out_c8_ch0;
    a.act_scale = d->act_scale;
    a.e_c0 = d->e0; a.e_c1 = d->e1; a.e_h = d->h;
    a.e_c0_bs = d->e0_bstride; a.e_c1_bs = d->e1_bstride; a.e_h_bs = d->h_bstride;
    a.out2 = d->out2; a.out2_bs = d->out2_bstride;
    a.out2_c8 = (char *)d->out2_c8; a.out2_c8_bs = d->out2_c8_bstride; a.out2_c8_ch0 = d->out2_c8_ch0;
    a.f32_c4 = d->f32_c4 ? 1 : 0;
    a.head_w = d->head_w; a.head_out = d->head_out; a.head_out_bs = d->head_out_bstride; a.head_nout = d->head_outputs;
    if (a.epi == 3 && (!a.head_w || !a.head_out || !a.bias)) return DKT_E_NULL;
    if (a.epi == 3 && (a.head_nout != 1 || a.Cout % 64 != 0)) return DKT_E_UNSUPPORTED;       // one output (stereo heads); the 2-output flow head keeps the hidden tensor
    a.tail = d->tail; a.tail_bs = d->tail_bstride; a.tail_ch = d->tail ? d->tail_channels : 0;
    a.tail_ratio = d->tail_scale > 0.0f ? d->tail_scale / d->act_scale : 1.0f;
    if ((a.out_c8_ch0 & 7) || (a.out2_c8_ch0 & 7)) return DKT_E_SHAPE;
    if (a.epi == 1) {
        if (!d->e0 || !d->e1 || !d->h || (!d->out2 && !d->out2_c8) || !d->out) return DKT_E_NULL;
        if (d->Cout % 128 != 0) return DKT_E_UNSUPPORTED;
    } else if (a.epi == 2) {
        if (!d->e0 || !d->e1 || !d->h) return DKT_E_NULL;
        if (d->Cout % 64 != 0) return DKT_E_UNSUPPORTED;
    } else if (a.epi == 4) {
        if (!d->e0) return DKT_E_NULL;
        if (d->Cout % 4 != 0) return DKT_E_UNSUPPORTED;
    }
    if (a.tail && (a.epi != 0 || !a.out_c8 || a.tail_ch <= 0 || a.Cout + a.tail_ch > a.n_co64 * 64)) return DKT_E_UNSUPPORTED;
    a.tiles_w = a.tiles_xy = a.n_co = a.total_tiles = 0;
    return DKT_OK;
}

static int c8_dispatch(const C8Args &a, int B, int cfg, int passes, hipStream_t st, const C8Args *second, int B2) {
    if (cfg == 0) {
        const long tiles8 = (long)((a.W + 31) / 32) * ((a.H + 7) / 8) * B;
        if (a.n_co64 >= 4 && tiles8 >= 128) cfg = 1;
        else if (a.n_co64 >= 2 && tiles8 * ((a.n_co64 + 1) / 2) >= 128) cfg = 2;
        else cfg = tiles8 * a.n_co64 >= 200 ? 3 : 4;
    }
    // (one pass: the chunk loop runs two chunks per trip -- odd chunk counts take two passes or more)
    if (passes == 1 && ((a.nchunks & 1) || (second && (second->nchunks & 1)))) return DKT_E_UNSUPPORTED;
    switch (passes) {
    case 0: case 3: return c8_dispatch_p<3>(a, B, cfg, st, second, B2);
    case 2: return c8_dispatch_p<2>(a, B, cfg, st, second, B2);
    case 1: return c8_dispatch_p<1>(a, B, cfg, st, second, B2);
    default: return DKT_E_UNSUPPORTED;
    }
}

extern "C" int dkt_conv2d_c8(const dkt_conv_c8_desc *d, int cfg, int device, void *stream) {
    C8Args a;
    const int rc = c8_fill(a, d);
    if (rc != DKT_OK) return rc;
    DKT_ENTER(device);
    return c8_dispatch(a, d->B, cfg, d->passes, (hipStream_t)stream, nullptr, 0);
}

extern "C" int dkt_conv2d_c8_pair(const dkt_conv_c8_desc *d0, const dkt_conv_c8_desc *d1, int cfg, int device, void *stream) {
    C8Args a, b;
    int rc = c8_fill(a, d0);
    if (rc != DKT_OK) return rc;
    rc = c8_fill(b, d1);
    if (rc != DKT_OK) return rc;
    if (cfg == 0) return DKT_E_UNSUPPORTED;          // both problems run one instantiation: the caller names it
    if ((d0->passes ? d0->passes : 3) != (d1->passes ? d1->passes : 3)) return DKT_E_UNSUPPORTED;
    DKT_ENTER(device);
    return c8_dispatch(a, d0->B, cfg, d0->passes, (hipStream_t)stream, &b, d1->B);
}

// ---- second layer of the flow / disparity head from the planes of epilogue 3 (core/update.py:10-13, 3x3, padding 1):
//   y[o] = bias[o] + sum over (co block, tap) of plane[(o * n_co + block) * 9 + tap] shifted by the tap;
//   target[o] += y[o]  (raft_stereo.py:165-168: coords1 = coords1 + delta_flow);  diff_out[o] = target[o] - diff_ref[o]
__global__ __launch_bounds__(256) void head_finish_kernel(const float *planes, long planes_bs, int n_co, const float *bias,
                                                          float *target, long target_bs, const float *diff_ref, long diff_ref_bs,
                                                          float *diff_out, long diff_out_bs, int nout, int H, int W) {
    const long HW = (long)H * W;
    const int b = blockIdx.y;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < HW; i += (long)gridDim.x * 256) {
        const int oh = (int)(i / W), ow = (int)(i - (long)oh * W);
        for (int o = 0; o < nout; ++o) {
            float s = 0.0f;
            for (int cb = 0; cb < n_co; ++cb) {
                const float *p = planes + (long)b * planes_bs + (long)(o * n_co + cb) * 9 * HW;
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const int ih = oh + t / 3 - 1, iw = ow + t % 3 - 1;
                    const bool in = ih >= 0 && ih < H && iw >= 0 && iw < W;
                    const float v = p[(long)t * HW + (in ? (long)ih * W + iw : 0)];
                    s = __fadd_rn(s, in ? v : 0.0f);
                }
            }
            s = __fadd_rn(s, bias ? bias[o] : 0.0f);
            float *tp = target + (long)b * target_bs + (long)o * HW + i;
            const float nv = __fadd_rn(*tp, s);
            *tp = nv;
            if (diff_out) diff_out[(long)b * diff_out_bs + (long)o * HW + i] = __fsub_rn(nv, diff_ref[(long)b * diff_ref_bs + (long)o * HW + i]);
        }
    }
}

extern "C" int dkt_head_finish(const float *planes, long planes_bstride, int n_co, const float *bias, float *target,
                               long target_bstride, const float *diff_ref, long diff_ref_bstride, float *diff_out,
                               long diff_out_bstride, int B, int nout, int H, int W, int device, void *stream) {
    if (!planes || !target || (diff_out && !diff_ref)) return DKT_E_NULL;
    if (B <= 0 || B > 65535 || nout < 1 || nout > 2 || n_co < 1 || H <= 0 || W <= 0) return DKT_E_SHAPE;
    DKT_ENTER(device);
    const long HW = (long)H * W;
    hipLaunchKernelGGL(head_finish_kernel, dim3((unsigned)((HW + 255) / 256 > 2048 ? 2048 : (HW + 255) / 256), (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, planes, planes_bstride, n_co, bias, target, target_bstride, diff_ref, diff_ref_bstride,
                       diff_out, diff_out_bstride, nout, H, W);
    return dkt_launch_status();
}

// number of output-channel blocks (= planes per output and tap) a head launch with tile shape `cfg` produces
extern "C" int dkt_conv2d_c8_head_blocks(int Cout, int cfg) {
    const int n64 = (Cout + 63) / 64;
    if (cfg == 2) return (n64 + 1) / 2;
    if (cfg == 1) return (n64 + 3) / 4;
    return DKT_E_UNSUPPORTED;
}
#endif      // C8_TU <= 0
