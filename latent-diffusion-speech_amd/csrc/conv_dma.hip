// DMA-fed, VALU-free implicit-GEMM convolution for the UNet (gfx950, v_mfma_f32_32x32x2_f32).
//
// Why this kernel exists.  On gfx950 the fp32 MFMA executes on the SIMD's vector ALU: measured with
// tools/ubench/mfma_valu_coexec.hip, an MFMA-only wave and a VALU-only wave on one SIMD take the SUM of
// their times (154.7 TFLOP/s alone; every co-resident FMA / exp / integer instruction adds its full issue
// time).  So in an fp32 GEMM every VALU instruction -- address arithmetic, normalisation, SiLU, bounds
// selects, register->LDS staging -- is paid in matrix throughput, whichever wave issues it.  This kernel
// therefore contains no per-element VALU work at all:
//   * activations live in HBM in the "K4P" layout (k4p.h): [B][C/8][2][T+2][4], channel 8q+2j+h at element j of
//     row (q,h), one zero pad frame on both sides.  A k-interleaved row is byte-for-byte the LDS image the MFMA
//     wants (one ds_read_b128 = the B operands of four consecutive MFMAs), and the pad frames ARE the
//     convolution's zero padding, so a tile is a plain linear copy;
//   * both operand tiles are moved HBM/L2 -> LDS by LDS-DMA (global_load_lds_dwordx4): no staging registers, no
//     ds_write, loop-invariant per-lane offsets, one scalar pointer bump per K-step;
//   * normalisation + activation are applied ONCE per tensor by the small memory-bound kernels in k4p_ops.hip
//     (instead of once per output-channel block inside the GEMM);
//   * the k3 taps are shifted reads of the same LDS window; skip-concat = second source pointer selected per
//     K-step; nearest-2x upsample = (frame >> 1) in the operand address; stride 2 = operand stride.
// Pipeline: NST-stage LDS ring; every wave issues 1/4 of each tile's DMA.  The operand registers form a ring that is
// read NB-1 MFMA groups ahead and runs THROUGH the K-step boundary: the per-tile synchronisation (counted vmcnt for
// this wave's share of the next tile, one s_barrier, refill of the stage just finished) sits NB-1 groups before the
// end of a K-step, where the ring starts reading the next tile, so no K-step begins with an exposed LDS latency.
#include "gn_chan.h"
#include "k4p.h"
#include "kernels.h"
#include "../../include/lds_test.h"

#include <hip/hip_ext.h>

#include <stdio.h>
#include <stdlib.h>

namespace lds {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// erf for the GEGLU epilogue (reference activations.py GEGLU -> F.gelu, exact form).  Abramowitz & Stegun 7.1.26:
// |error| <= 1.5e-7 absolute, i.e. at the level of fp32 rounding of erf itself; one v_rcp_f32, one v_exp_f32 and seven
// multiply-adds instead of the ~40-instruction library routine -- the epilogue's vector work is paid in matrix time.
static __device__ __forceinline__ float erf_fast(float x) {
    const float ax = fabsf(x);
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.0f));
    float pl = fmaf(1.061405429f, t, -1.453152027f);
    pl = fmaf(pl, t, 1.421413741f);
    pl = fmaf(pl, t, -0.284496736f);
    pl = fmaf(pl, t, 0.254829592f);
    const float e = __builtin_amdgcn_exp2f(ax * ax * -1.4426950408889634f);
    return copysignf(fmaf(-pl * t, e, 1.0f), x);
}

// Wave64 sum in a fixed order (DPP row shifts + row broadcasts, no LDS): the total is valid in lane 63.
template <int CTRL, int ROW_MASK, bool BOUND>
static __device__ __forceinline__ float dpp_add(float v) {
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, BOUND));
}
static __device__ __forceinline__ float wave_sum_to_lane63(float v) {
    v = dpp_add<0x111, 0xf, true>(v);      // row_shr:1
    v = dpp_add<0x112, 0xf, true>(v);      // row_shr:2
    v = dpp_add<0x114, 0xf, true>(v);      // row_shr:4
    v = dpp_add<0x118, 0xf, true>(v);      // row_shr:8   lane 15 of every 16-lane row = the row's sum
    v = dpp_add<0x142, 0xa, false>(v);     // row_bcast:15 into rows 1 and 3
    v = dpp_add<0x143, 0xc, false>(v);     // row_bcast:31 into rows 2 and 3
    return v;
}

template <int BM, int BN, int KT, int STRIDE, bool UPS, int BK, int NST, int DIL = 1>
struct DmaCfg {
    // BM = 32: split-K inside the workgroup for grids smaller than the chip.  The tile is 32 x 64; waves (wn, ks) take
    // column block wn and half ks of every K-step's k range, and the two partial sums meet through LDS in the epilogue
    // (fixed order: ks = 0 adds the ks = 1 partial), so a 64 x 64 tile's work spreads over two workgroups / CUs.
    static constexpr bool SPLIT = BM == 32;
    static constexpr int TM = SPLIT ? 1 : BM / 64, TN = BN / 64;
    static constexpr int KR = BK / 4;                                   // staged k-rows per K-step
    static constexpr int XW = UPS ? (BN / 2 + 2) : ((BN - 1) * STRIDE + (KT - 1) * DIL + 1);   // window entries (frames) per k-row; taps are DIL entries apart
    static constexpr int WI = KT * KR * BM / 64;                        // weight DMA wave-instructions per tile
    static constexpr int WPW = WI / 4;                                  // ... per wave
    static constexpr int RPW = KR / 4;                                  // activation k-rows staged by each wave
    static constexpr int NXI = (RPW * XW + 63) / 64;                    // activation DMA wave-instructions per wave
    static constexpr int PER_TILE = WPW + NXI;                          // VMEM ops per wave per tile
    static constexpr int KQW = SPLIT ? BK / 16 : BK / 8;                // 8-channel k groups per tap handled by one wave
    static constexpr int G = KT * KQW;                                  // MFMA groups per K-step and wave (4 k-pairs each)
    static constexpr int NB = (G % 3 == 0 && TM * TN < 4) ? 3 : 2;      // operand ring depth (divides G: slots keep their phase across K-steps)
    static constexpr int NACC = (TM * TN >= 2) ? 1 : 2;                 // independent accumulator chains per tile
    static constexpr int STAGE = KT * BK * BM + KR * XW * 4;            // floats
    static constexpr size_t LDS_BYTES = (size_t)NST * STAGE * sizeof(float);
    // workgroups per CU allowed by LDS = waves per SIMD to ask the register allocator for (each workgroup puts one wave on each SIMD)
    static constexpr int OCC_LDS = (int)((160 * 1024) / LDS_BYTES);
    static constexpr int OCC = (TM * TN >= 4) ? (OCC_LDS < 2 ? OCC_LDS : 2) : (OCC_LDS < 4 ? (OCC_LDS < 1 ? 1 : OCC_LDS) : 4);
    static_assert(WI % 4 == 0 && KR % 4 == 0, "tile does not split evenly over 4 waves");
    static_assert(!SPLIT || (BN == 64 && BK % 16 == 0), "split-K tile is 32 x 64");
};

// GNF: the GroupNorm fold of DmaConvArgs::gnf_part (its own instantiations: the other launches carry none of its registers)
template <int BM, int BN, int KT, int STRIDE, bool UPS, int BK, int NST, int DIL = 1, bool VOC = false, bool GNF = false, bool GELU = false, int ACT2 = 0>
struct DmaKernel {
    using Cfg = DmaCfg<BM, BN, KT, STRIDE, UPS, BK, NST, DIL>;
    static constexpr int TM = Cfg::TM, TN = Cfg::TN, KR = Cfg::KR, XW = Cfg::XW, WPW = Cfg::WPW, RPW = Cfg::RPW, NXI = Cfg::NXI;
    static constexpr int G = Cfg::G, NB = Cfg::NB, NACC = Cfg::NACC, STAGE = Cfg::STAGE, PER_TILE = Cfg::PER_TILE, KQW = Cfg::KQW;
    static constexpr bool SPLIT = Cfg::SPLIT;

    const DmaConvArgs& p;
    float* smem;
    // The arguments that the first DMA issue depends on.  load_hot() requests them all at kernel entry and pins them behind ONE wait
    // (an empty asm that takes every one of them as an operand), instead of one scalar-memory round trip per branch that first uses a
    // field; the code in front of the first issue_tile reads these copies only.  Every other field is read from `p` where it is used.
    struct Hot {
        const float *x1, *x2, *w;      // (used as buffer bases only; `lens` is dereferenced and stays a kernel-argument pointer: a scalar load)
        int C1, C2, Tsrc, Mp, Ci, xpad, pad, ksplit, To, lvl_out;
        unsigned om0, om1, om2, os, gx, gy;
    } hp;
    int lane, wave, c, h, wm, wn, ks, b, m0, t0;
    int ksp, kc0, ctile;      // cluster split-K (DmaConvArgs::ksplit): this workgroup's share index, its first K-step, its tile's linear index
    int Lout;                 // valid output frames of this batch element (ragged batches, k4p.h ragged_len; = To otherwise)
    float gcg[GNF ? 8 : 1], gkc;      // (threads < BM: the terms of their row's constant, in flight across the first barrier)
    GnPart gp0, gp1;                  // this wave's two groups' partial statistics, in flight across the first DMAs
    float gs, gsn, ginv;              // rstd of the group of this wave's share of the current / the next K-step; 1 / (channels per group)
    int kofs_a, kofs_b;       // split-K: float offsets of this wave's half of the staged k rows (weights / activations)
    int woff[WPW];            // per-lane byte offsets of this wave's weight chunks (loop invariant)
    int xoff[NXI];            // per-lane byte offsets of this wave's activation chunks inside a source slab
    __amdgpu_buffer_rsrc_t rw, rx1, rx2;   // packed weights; this batch element's slab of either source
    bool xact[NXI];
    int arow;
    int bcol[TN];
    f32x16 acc[NACC][TM][TN];
    f32x4 aop[NB][TM], bop[NB][TN];
    float lmu[TN], lrs[TN];   // folded input-LayerNorm statistics of this lane's output columns
    // single-tile waves fetch the epilogue's operands at kernel start (16 + 16 registers): the residual entries and the bias
    // rows have landed long before the main loop ends, so the epilogue begins without a memory round trip
    // (vocoder tiles too: their K loops run 20-40 us, the 8 residual registers per 32 x 32 tile fit beside the accumulators)
    static constexpr bool EARLY = TM * TN == 1 || VOC;
    // ... and the UNet's and the encoders' single-tile waves request them BEHIND the first NST tiles' DMAs (late_loads): the first DMA
    // then waits for neither their address arithmetic nor -- vmcnt completes in order -- their data.  NLATE = the vector memory operations
    // late_loads() issues, the same number whatever the arguments are (a null residual or bias is a buffer of zero bytes, which reads as
    // zeros): the counted waits below rely on it.  The GroupNorm fold keeps its own order (gnf_request), the vocoder the old one.
    static constexpr bool LATE = EARLY && !VOC && !GNF;
    static constexpr int NLATE = LATE ? TM * TN * 8 + TM * 4 : 0;
    static_assert(PER_TILE * (NST - 1) + NLATE <= 63 || !LATE, "vmcnt is a 6-bit field");
    f32x2 rsv[EARLY ? TM * TN * 8 : 1];
    float kbv[EARLY ? TM * 16 : 1];
    __device__ __forceinline__ DmaKernel(const DmaConvArgs& p_, float* s_) : p(p_), smem(s_) {}

    // k4p.h ragged_len / the vocoder's lengths, read through the constant address space: the lengths do not change during a launch, and so
    // the read stays a scalar load behind load_hot()'s asm statement (which the compiler must assume to write memory)
    typedef const __attribute__((address_space(4))) int* const_int_ptr;
    __device__ __forceinline__ int len_at(int lvl, int T) const {
        if (!p.lens) return T;
        int n = ((const_int_ptr)(unsigned long long)p.lens)[b];
        for (int i = 0; i < lvl; ++i) n = (n - 1) / 2 + 1;
        return n < T ? n : T;
    }
    __device__ __forceinline__ void load_hot() {
        hp.x1 = p.x1; hp.x2 = p.x2; hp.w = p.w;
        hp.C1 = p.C1; hp.C2 = p.C2; hp.Tsrc = p.Tsrc; hp.Mp = p.Mp; hp.Ci = p.Ci; hp.xpad = p.xpad; hp.pad = p.pad; hp.ksplit = p.ksplit; hp.To = p.To;
        hp.lvl_out = p.lvl_out; hp.om0 = p.ord_m[0]; hp.om1 = p.ord_m[1]; hp.om2 = p.ord_m[2]; hp.os = p.ord_s; hp.gx = gridDim.x; hp.gy = gridDim.y;
        asm volatile("" : "+s"(hp.x1), "+s"(hp.x2), "+s"(hp.w), "+s"(hp.C1), "+s"(hp.C2), "+s"(hp.Tsrc), "+s"(hp.Mp), "+s"(hp.Ci),
                          "+s"(hp.xpad), "+s"(hp.pad), "+s"(hp.ksplit), "+s"(hp.To), "+s"(hp.lvl_out), "+s"(hp.om0), "+s"(hp.om1), "+s"(hp.om2),
                          "+s"(hp.os), "+s"(hp.gx), "+s"(hp.gy));
    }
    __device__ __forceinline__ void setup_keep_acc() {      // everything but the accumulators (second phase of conv_dma_pair_kernel)
        load_hot();
        const int tid = threadIdx.x;
        lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        c = lane & 31; h = lane >> 5;
        wm = SPLIT ? 0 : wave >> 1; ks = SPLIT ? wave >> 1 : 0; wn = wave & 1;
        kofs_a = ks * KQW * 2 * BM * 4; kofs_b = ks * KQW * 2 * XW * 4;
        // XCD-aware tile order.  Workgroups are dispatched in linear order, round-robin over the 8 XCDs, each with a private
        // L2.  The workgroups that read the same activation window (all M-blocks of one (batch, frame-block)) are given
        // consecutive slots of ONE XCD, so the window is fetched from the fabric once instead of once per XCD.
        // The three divisions (by nMb, nN and S) are multiplications by the launcher's constants (kernels.h dma_magic): exact quotients
        // on the scalar unit, instead of a detour through the vector unit's reciprocal each.
        const int nMb = (int)((unsigned)hp.Mp / BM), nN = (int)((unsigned)(hp.To + BN - 1) / BN);
        const int gx = (int)hp.gx, total = gx * (int)hp.gy;
        const int id = blockIdx.y * gx + blockIdx.x;
        const int xcd = id & 7, slot = id >> 3, per = total >> 3, rem = total & 7;
        const unsigned L = (unsigned)(xcd * per + (xcd < rem ? xcd : rem) + slot);
        const unsigned tb = dma_magic_div(L, hp.om0, hp.os & 255);
        const int mb = (int)(L - tb * nMb);       // M fastest: neighbours share the activation tile
        const unsigned by = dma_magic_div(tb, hp.om1, (hp.os >> 8) & 255);
        const int nb = (int)(tb - by * nN);
        const int S = hp.ksplit > 1 ? hp.ksplit : 1;      // grid.y = B * S
        b = (int)dma_magic_div(by, hp.om2, (hp.os >> 16) & 255); ksp = (int)by - b * S;
        kc0 = ksp * steps_per_share();
        ctile = (b * nN + nb) * nMb + mb;
        m0 = mb * BM; t0 = nb * BN;
        Lout = len_at(hp.lvl_out, hp.To);
#pragma unroll
        for (int i = 0; i < WPW; ++i) {
            const unsigned q = (unsigned)(wave + 4 * i) * 64u + (unsigned)lane;      // chunk = (tap, k-row, m)  (unsigned: shifts and masks, no sign fix-ups)
            const unsigned tap = q / (unsigned)(KR * BM);
            const unsigned rem = q - tap * (unsigned)(KR * BM);
            const unsigned rr = rem / (unsigned)BM, m = rem - rr * (unsigned)BM;
            woff[i] = (int)(((tap * ((unsigned)hp.Ci / 4u) + rr) * (unsigned)hp.Mp + (unsigned)m0 + m) * 16u);
        }
        const int Tp = hp.Tsrc + 2 * hp.xpad;
        const int e0 = UPS ? (((t0 - 1) >> 1) + hp.xpad) : (t0 * STRIDE - hp.pad + hp.xpad);   // first window entry (entry xpad = frame 0)
#pragma unroll
        for (int i = 0; i < NXI; ++i) {
            const unsigned qq = (unsigned)(i * 64 + lane);
            const int rl = (int)(qq / (unsigned)XW), col = (int)qq - rl * XW;
            xact[i] = (int)qq < RPW * XW;
            xoff[i] = ((wave * RPW + rl) * Tp + e0 + col) * 16;
        }
        rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(hp.w), 0, KT * hp.Ci * hp.Mp * 4, 0x00020000);
        rx1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(hp.x1 + (long long)b * hp.C1 * Tp), 0, hp.C1 * Tp * 4, 0x00020000);
        rx2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(hp.x2 ? hp.x2 + (long long)b * hp.C2 * Tp : hp.x1), 0, hp.C2 * Tp * 4, 0x00020000);
        arow = wm * TM * 32 + c;
#pragma unroll
        for (int j = 0; j < TN; ++j) bcol[j] = wn * TN * 32 + j * 32 + c;
    }
    // this workgroup's K-steps: Ci / BK / S (S = the cluster split, a divisor of Ci / BK: the launchers check it)
    __device__ __forceinline__ int steps_per_share() const { return (int)dma_magic_div((unsigned)hp.Ci / BK, hp.om2, (hp.os >> 16) & 255); }
    __device__ __forceinline__ bool dead_tile() const { return !VOC && p.lens && t0 >= Lout; }
    // the vocoder's lengths multiply per stage: given outright (kernels.h DmaConvArgs::vlen), fetched where they are used (the epilogue)
    __device__ __forceinline__ int voc_len() const { return ((const_int_ptr)(unsigned long long)p.vlen)[b]; }
    __device__ __forceinline__ void zero_acc() {
#pragma unroll
        for (int a = 0; a < NACC; ++a)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[a][i][j][r] = 0.f;
    }

    // tile kc -> LDS stage `st`: this wave's share of the weight chunks and of the activation window.  Buffer-addressed
    // LDS-DMA: per-lane byte offsets are loop invariant (VGPR), the K-step advance is a scalar offset, so issuing a tile
    // costs no vector ALU work; reads past a source slab return zeros (hardware range check).
    __device__ __forceinline__ void issue_tile(int kc, float* st) {
        const int ws = kc * (KR * 16) * hp.Mp;                   // bytes
#pragma unroll
        for (int i = 0; i < WPW; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (__attribute__((address_space(3))) void*)(st + ((wave + 4 * i) * 64) * 4), 16, woff[i], ws, 0, 0);
        const int k0 = kc * BK;
        const bool s2 = k0 >= hp.C1;                             // C1 % BK == 0: a K-step reads one source only
        const int xsoff = (s2 ? k0 - hp.C1 : k0) * (hp.Tsrc + 2 * hp.xpad) * 4;
        float* xs = st + KT * BK * BM + wave * RPW * XW * 4;
#pragma unroll
        for (int i = 0; i < NXI; ++i)
            if (xact[i]) {
                if (s2) __builtin_amdgcn_raw_ptr_buffer_load_lds(rx2, (__attribute__((address_space(3))) void*)(xs + i * 64 * 4), 16, xoff[i], xsoff, 0, 0);
                else __builtin_amdgcn_raw_ptr_buffer_load_lds(rx1, (__attribute__((address_space(3))) void*)(xs + i * 64 * 4), 16, xoff[i], xsoff, 0, 0);
            }
    }

    template <int SLOT>
    __device__ __forceinline__ void load_ops(const float* st, int tap, int kq) {
        const float* wt = st + ((tap * KR + kq * 2 + h) * BM + arow) * 4 + kofs_a;
        const float* xs = st + KT * BK * BM + (kq * 2 + h) * XW * 4 + kofs_b;
#pragma unroll
        for (int i = 0; i < TM; ++i) aop[SLOT][i] = *reinterpret_cast<const f32x4*>(wt + i * 32 * 4);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int col = UPS ? (((t0 + bcol[j] + tap - 1) >> 1) - ((t0 - 1) >> 1)) : (bcol[j] * STRIDE + tap * DIL);
            bop[SLOT][j] = *reinterpret_cast<const f32x4*>(xs + col * 4);
        }
    }
    template <int SLOT>
    __device__ __forceinline__ void mfma_ops() {
        if constexpr (GNF) {      // GroupNorm fold: the activations of this K-step's group times its rstd (2 packed multiplies per operand entry)
#pragma unroll
            for (int j = 0; j < TN; ++j) bop[SLOT][j] *= gs;
        }
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[jj % NACC][i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(aop[SLOT][i][jj], bop[SLOT][j][jj], acc[jj % NACC][i][j], 0, 0, 0);
    }
    template <int g0, int g1>
    __device__ __forceinline__ void preload(const float* cur) {
        if constexpr (g0 < g1 && g0 < G) {
            load_ops<g0 % NB>(cur, g0 / KQW, g0 % KQW);
            preload<g0 + 1, g1>(cur);
        }
    }
    // Tile boundary, reached when the operand ring is about to read its first group of tile kc+1: this wave has issued
    // (and, after the lgkmcnt wait, completed) all its reads of tile kc.  After the barrier tile kc+1 is visible to
    // everyone and tile kc's stage is free, so it is refilled with tile kc+NST.
    template <bool EPI>
    __device__ __forceinline__ void tile_sync(int kc, int nk, float* cur) {
        const int younger = (nk - 2 - kc < NST - 2) ? (nk - 2 - kc) : (NST - 2);     // tiles after kc+1 still in flight
        // (tile kc+1 < NST belongs to the first burst, which late_loads() follows: its NLATE operations are younger too.  A later tile
        // was issued after them: they are older and count for nothing.)
        if (EPI && NLATE > 0 && kc + 1 < NST) wait_younger<NST - 2, NLATE>(younger);
        else wait_younger<NST - 2, 0>(younger);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (kc + NST < nk) issue_tile(kc0 + kc + NST, cur);
    }
    template <int g, bool EPI>
    __device__ __forceinline__ void kstep(float* cur, const float* nxt, int kc, int nk) {
        if constexpr (g < G) {
            constexpr int gp = g + NB - 1;                     // group whose operands are fetched now
            if constexpr (gp < G) {
                load_ops<gp % NB>(cur, gp / KQW, gp % KQW);
            } else {
                if (kc + 1 < nk) {
                    if constexpr (gp == G) tile_sync<EPI>(kc, nk, cur);
                    load_ops<gp % NB>(nxt, (gp - G) / KQW, (gp - G) % KQW);
                }
            }
            mfma_ops<g % NB>();
            __builtin_amdgcn_sched_barrier(0);     // keep the operand reads NB-1 groups ahead of their MFMAs
            kstep<g + 1, EPI>(cur, nxt, kc, nk);
        }
    }

    // LayerNorm over the input channels (reference attention.py:83,102,118), folded into the epilogue: per output column
    // combine the producer's per-32-channel (mean, M2) partials in a fixed order (gn_chan.h ln_column_stats).  Called right
    // after the first tiles' DMAs are issued; all partials of a column are requested at once (no chain of dependent round trips).
    __device__ __forceinline__ void ln_columns() {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = t0 + wn * TN * 32 + j * 32 + c;
            const bool ok = n < p.To;
            const float2* src = p.ln_part + (long long)b * p.ln_np * p.Tsrc + (ok ? n : 0);
            ln_column_stats(src, p.Tsrc, p.ln_np, p.ln_eps, ok, lmu[j], lrs[j]);      // (gn_chan.h: two plain sums in a fixed order)
        }
    }

    // ---- GroupNorm fold (DmaConvArgs::gnf_part) ----
    // LDS behind the ring: [0, BM) the per-row constants, then 8 x rstd_g and 8 x rstd_g * mean_g of this batch element
    __device__ __forceinline__ float* gnf_tail() const { return smem + NST * STAGE + BM; }
    // group of this wave's share of K-step k (of this workgroup's range), clamped to the last one (look-ahead past the end)
    __device__ __forceinline__ int gnf_group(int k) const {
        const int pos = (kc0 + k) * BK + ks * (SPLIT ? BK / 2 : BK);
        const int g = (int)(((float)pos + 0.5f) * ginv);
        return g < p.gnf_groups ? g : p.gnf_groups - 1;
    }
    // kernel start, before the first DMA (so that waiting for them does not wait for the tiles): the requests for this wave's two groups'
    // partials (wave w takes groups w and w + 4) and for the terms of the row constants
    __device__ __forceinline__ void gnf_request() {
        const int G_ = p.gnf_groups, gsz = p.Ci / G_;
        const int gTv = len_at(p.lvl_in, p.Tsrc);      // the statistics stop at the utterance's own length
        ginv = 1.0f / (float)gsz;
        gp0 = gn_part_load(p.gnf_part, b, p.Ci, p.Tsrc, gsz >> 4, wave, lane, 0, gTv);                              // (8 groups at most: wave < G_ or an unused slot)
        gp1 = gn_part_load(p.gnf_part, b, p.Ci, p.Tsrc, gsz >> 4, (wave + 4 < G_) ? wave + 4 : wave, lane, 0, gTv);
        if ((int)threadIdx.x < BM) {
            const int m = m0 + (int)threadIdx.x;
            gkc = p.gnf_c2[m];
#pragma unroll
            for (int g = 0; g < 8; ++g) gcg[g] = (g < G_) ? p.gnf_cg[g * p.Mp + m] : 0.f;
        }
    }
    // after the first tiles' DMAs are issued, before the first barrier: the statistics into LDS
    __device__ __forceinline__ void gnf_prepare() {
        const int G_ = p.gnf_groups, gsz = p.Ci / G_;
        float* tail = gnf_tail();
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int g = wave + 4 * e;
            float rs = 1.f, rm = 0.f;      // (slots of absent groups: finite, they multiply zeros)
            if (g < G_) {
                float mu, var;
                gnf_group_stats(p.gnf_part, b, p.Ci, p.Tsrc, gsz >> 4, g, lane, e ? gp1 : gp0, mu, var, len_at(p.lvl_in, p.Tsrc));
                rs = __builtin_amdgcn_rsqf(var + p.gnf_eps); rm = rs * mu;
            }
            if (lane == 0) { tail[g] = rs; tail[8 + g] = rm; }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the stores are in LDS before this wave passes the barrier (s_barrier alone does not wait)
    }
    // after the first barrier: kc[m] = gnf_c2[m] - sum_g rstd_g mean_g gnf_cg[g][m]  (read in finalize, behind further barriers), and the
    // scale of this wave's first two K-steps
    __device__ __forceinline__ void gnf_rows() {
        const float* tail = gnf_tail();
        if ((int)threadIdx.x < BM) {
            float kc = gkc;
#pragma unroll
            for (int g = 0; g < 8; ++g) kc = fmaf(-tail[8 + g], gcg[g], kc);      // (groups beyond gnf_groups: gcg = 0, tail finite)
            smem[NST * STAGE + threadIdx.x] = kc;
        }
        gs = tail[gnf_group(0)];
        gsn = tail[gnf_group(1)];
    }
    // after K-step k: the next step's scale becomes current, the one after it is requested (its LDS latency hides under the next step)
    __device__ __forceinline__ void gnf_advance(int k) {
        gs = gsn;
        gsn = gnf_tail()[gnf_group(k + 2)];
    }

    // s_waitcnt vmcnt(y * PER_TILE + X) for a wave-uniform y in [0, Y]: the y younger tiles' DMAs and X further operations that are
    // younger than the awaited tile may stay in flight.
    // INVARIANT: the count must never exceed the number of vector memory operations this wave has ISSUED AFTER the last DMA of the tile
    // it waits for.  vmcnt completes in order, so with N <= that number the tile has landed when the wait returns; a count that is too
    // small only waits longer, one that is too large lets the MFMAs read LDS before the DMA has written it -- silently wrong tiles.  So X
    // may only name operations that are issued unconditionally, by every lane mask, between the burst and the wait (late_loads()).
    template <int Y, int X = 0>
    __device__ __forceinline__ void wait_younger(int y) {
        if constexpr (Y == 0) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(X > 63 ? 63 : X) : "memory");
        } else {
            constexpr int N = (Y * PER_TILE + X > 63) ? 63 : Y * PER_TILE + X;      // vmcnt is a 6-bit field; a smaller count only waits longer
            if (y >= Y) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
            else wait_younger<Y - 1, X>(y);
        }
    }

    __device__ __forceinline__ bool res_tile(int tile0, int n) const {
        return p.res && tile0 < p.plain_from && tile0 < p.Cout && n < p.To;      // the residual is always a K4P tensor
    }
    __device__ __forceinline__ void early_loads() {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int tile0 = m0 + wm * TM * 32 + i * 32;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = t0 + wn * TN * 32 + j * 32 + c;
                f32x2* rs = rsv + (i * TN + j) * 8;
#pragma unroll
                for (int e = 0; e < 8; ++e) rs[e] = f32x2{0.f, 0.f};
                if (res_tile(tile0, n)) {
                    const int Tpo = p.To + 2 * p.opad;
                    const float* rb = p.res + (long long)b * k4p_ck() * Tpo + k4p_off(tile0, n);
#pragma unroll
                    for (int e = 0; e < 8; ++e) rs[e] = *reinterpret_cast<const f32x2*>(rb + e * Tpo * 4);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) kbv[i * 16 + r] = (p.bias && !p.ln_part) ? p.bias[tile0 + (r & 3) + 8 * (r >> 2) + 4 * h] : 0.f;
        }
    }

    // The same operands through buffer loads, issued right behind the first tiles' DMAs: EXACTLY NLATE vector memory operations (8 residual
    // entries and 4 bias quads per tile), for every argument set and by every lane -- no branch and no lane mask around them (see
    // wait_younger).  A launch without a residual, or a tile outside it, reads a buffer of zero bytes: zeros, as before.  Frames beyond To
    // read whatever the range check lets through; add_residual() does not use them.
    // A LayerNorm-fold launch without a residual (the QKV projections) has no use for either: its slots fetch the fold's row constants
    // instead, ln_c1 through the eight residual slots (8 bytes each: rows 8g + 4h + 2k + 0..1) and ln_c2 through the four bias quads, so
    // they too have landed before the K loop ends (row_consts).  The choice is scalar: buffer base, size and steps; the loads are the same.
    // (wave-uniform) a LayerNorm-fold launch without a residual: late_loads() fetches ln_c1 through the residual slots, ln_c2 through the bias slots
    __device__ __forceinline__ bool ln_late() const { return LATE && KT == 1 && p.ln_part && !p.res; }      // (the fold belongs to 1x1 convolutions: the other kernels compile the choice out)
    template <bool FOLD>      // (false: the fused pair's second phase, which never carries a LayerNorm fold -- its code stays as it was)
    __device__ __forceinline__ void late_loads() {
        static_assert(TM * TN == 1, "single-tile waves");
        const int tile0 = m0 + wm * 32, n = t0 + wn * 32 + c;
        const int Tpo = p.To + 2 * p.opad, Ck = k4p_ck();
        const bool rt = p.res && tile0 < p.plain_from && tile0 < p.Cout;      // (wave-uniform)
        const bool lnf = FOLD && ln_late();                                          // (wave-uniform) the slots carry the LayerNorm fold's row constants
        const float* rbase = lnf ? p.ln_c1 : (rt ? p.res + (long long)b * Ck * Tpo : p.res);
        const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(rbase), 0, lnf ? p.Mp * 4 : (rt ? Ck * Tpo * 4 : 0), 0x00020000);
        const int vo = lnf ? (tile0 + 4 * h) * 4 : k4p_off(tile0, n) * 4;
#pragma unroll
        for (int e = 0; e < 8; ++e) {      // fold: rows 8g + 4h + 2k + (0, 1) = registers 4g + 2k + (0, 1), slot e = 2g + k (a scalar step either way)
            const int step = lnf ? (e >> 1) * 32 + (e & 1) * 8 : e * Tpo * 16;
            rsv[e] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rr, vo + step, 0, 0));
        }
        const bool hb = (p.bias && !p.ln_part) || lnf;
        const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(lnf ? p.ln_c2 : p.bias), 0, hb ? p.Mp * 4 : 0, 0x00020000);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb, (tile0 + 8 * g + 4 * h) * 4, 0, 0));      // rows 8g + 4h + (0..3) = registers 4g + (0..3)
#pragma unroll
            for (int k = 0; k < 4; ++k) kbv[4 * g + k] = v[k];
        }
    }

    // EPI: this reduction is followed by the epilogue (false: the first phase of conv_dma_pair_kernel, whose epilogue operands are the second
    // phase's -- its late loads would be dead code, and the compiler would drop them while the waits still counted them).  ZERO: clear the
    // accumulators (behind the first DMAs, not in front of them).
    template <bool EPI = true, bool ZERO = true>
    __device__ __forceinline__ void mainloop() {
        static_assert(G % NB == 0 && NB - 1 <= G, "ring slots must keep their phase across K-steps");
        constexpr int XL = EPI ? NLATE : 0;
        const int nk = steps_per_share();      // this workgroup's K-steps: kc0 .. kc0 + nk - 1
        if constexpr (GNF) gnf_request();
        if constexpr (EARLY && !LATE) early_loads();
        for (int t = 0; t < NST && t < nk; ++t) issue_tile(kc0 + t, smem + t * STAGE);
        if constexpr (XL > 0) {
            // nothing of late_loads() may move in front of the burst or behind the wait: both would make the count of wait_younger too large
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            late_loads<ZERO>();
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (ZERO) {
            // (written as instructions so that they stay here: as plain constants the compiler materialises them in front of the burst)
#pragma unroll
            for (int a = 0; a < NACC; ++a)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            float z;
                            asm volatile("v_mov_b32 %0, 0" : "=v"(z));
                            acc[a][i][j][r] = z;
                        }
        }
        if (p.ln_part) ln_columns();
        if constexpr (GNF) gnf_prepare();
        wait_younger<NST - 1, XL>((nk - 1 < NST - 1) ? nk - 1 : NST - 1);      // tile 0 landed (this wave's share)
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if constexpr (GNF) gnf_rows();
        preload<0, NB - 1>(smem);
        int sc = 0;
        for (int kc = 0; kc < nk; ++kc) {
            const int sn = (sc + 1 == NST) ? 0 : sc + 1;
            kstep<0, EPI>(smem + sc * STAGE, smem + sn * STAGE, kc, nk);
            sc = sn;
            if constexpr (GNF) gnf_advance(kc);
        }
        if constexpr (GNF) __syncthreads();      // (the row constants are read in finalize: a one-K-step launch has met no barrier since)
    }
    // The row constants of tile row i in the accumulators' plain layout (register 4g + k = packed weight row 8g + 4h + k): k1 = ln_c1 (the
    // LayerNorm fold only), k2 = ln_c2 or the bias.  Single-tile waves hold them since late_loads() / early_loads(); the others (and a fold
    // with a residual, whose slots carry the residual) fetch them here as four 16-byte loads per array -- the rows of a register quad
    // are contiguous -- from one address per array with immediate offsets.  Global loads, not buffer loads: the register buffer loads
    // of these kernels are the counted late loads and nothing else.
    // (HELD is the caller's branch: each source gets its own copy of the code that uses the values)
    template <bool HELD>
    __device__ __forceinline__ void row_consts(int i, bool ln, float* k1, float* k2) const {
        if constexpr (HELD) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                k2[r] = kbv[i * 16 + r];
                if constexpr (LATE) k1[r] = ln ? rsv[r >> 1][r & 1] : 0.f;
                else k1[r] = 0.f;
            }
        } else {
            // (scalar base + one unsigned 32-bit lane offset + immediates: no 64-bit vector address arithmetic)
            const unsigned ro = (unsigned)(m0 + wm * TM * 32 + i * 32 + 4 * h) * 4u;
            const char* a2 = reinterpret_cast<const char*>(ln ? p.ln_c2 : p.bias);      // (not null: the callers come here with a fold or a bias only)
            f32x4 q1[4], q2[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                q1[g] = f32x4{0.f, 0.f, 0.f, 0.f};
                q2[g] = *reinterpret_cast<const f32x4*>(a2 + ro + 32 * g);
            }
            if (ln) {
                const char* a1 = reinterpret_cast<const char*>(p.ln_c1);
#pragma unroll
                for (int g = 0; g < 4; ++g) q1[g] = *reinterpret_cast<const f32x4*>(a1 + ro + 32 * g);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
#pragma unroll
                for (int k = 0; k < 4; ++k) { k1[4 * g + k] = q1[g][k]; k2[4 * g + k] = q2[g][k]; }
            }
        }
    }

    template <bool HELD>
    __device__ __forceinline__ void apply_rows(bool ln) {
        float k1[TM][16], k2[TM][16];
#pragma unroll
        for (int i = 0; i < TM; ++i) row_consts<HELD>(i, ln, k1[i], k2[i]);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float v = acc[0][i][j][r];
                    // rstd * (v - mean * k1) + k2 with its roundings spelled out, so that they do not hang on how the compiler contracts the
                    // expression: two fused multiply-adds in single-tile kernels, and
                    // fma, multiply, add in the multi-tile ones -- what either kind has always computed
                    const float t = fmaf(-lmu[j], k1[i][r], v);
                    if constexpr (EARLY) acc[0][i][j][r] = ln ? fmaf(lrs[j], t, k2[i][r]) : v + k2[i][r];
                    else acc[0][i][j][r] = ln ? __fadd_rn(__fmul_rn(lrs[j], t), k2[i][r]) : v + k2[i][r];
                }
    }

    // Epilogue, phase 1: accumulators -> output values in place (acc[0]).  All loads of a phase are issued before their
    // first use and before any store: a load placed after a store cannot be moved above it (possible aliasing), and a
    // load -> wait -> store chain costs one memory round trip per element.
    template <bool FOLD>
    __device__ __forceinline__ void finalize(bool geglu) {
        if constexpr (NACC == 2) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[0][i][j] += acc[1][i][j];
        }
        const bool ln = FOLD && KT == 1 && p.ln_part != nullptr;      // (the fold belongs to 1x1 convolutions: launch_conv_dma; never to the fused pair)
        if (EARLY && !ln) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[0][i][j][r] += kbv[i * 16 + r];
        } else if (ln || p.bias) {
            if (LATE && ln_late()) apply_rows<LATE>(ln);
            else apply_rows<false>(ln);
        }
        if constexpr (GNF) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float kc = smem[NST * STAGE + wm * TM * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h];
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[0][i][j][r] += kc;
                }
        }
        if (geglu) {      // rows of tile 0 are the values, rows of tile 1 the gates (pack_geglu)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float g = acc[0][TM - 1][j][r];
                    if constexpr (ACT2 == 2) acc[0][0][j][r] *= 1.0f / (1.0f + expf(-g));      // GLU: value * sigmoid(gate) (the Conformer's pointwise_conv1)
                    else acc[0][0][j][r] *= 0.5f * g * (1.0f + erf_fast(g * 0.70710678118654752440f));
                }
        }
        if constexpr (ACT2 == 1) {      // swish (the Conformer's feed-forwards): instantiations of its own, as for GELU below
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float v = acc[0][i][j][r];
                        acc[0][i][j][r] = v / (1.0f + expf(-v));
                    }
        }
        if constexpr (GELU) {      // plain GELU, exact form (the Whisper encoder's conv1 / conv2 / mlp.0, reference encoder/whisper/model.py:96,122-123):
                                   // instantiations of its own (launch_conv_dma), so that no other launch's code changes
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float v = acc[0][i][j][r];
                        acc[0][i][j][r] = 0.5f * v * (1.0f + erf_fast(v * 0.70710678118654752440f));
                    }
        }
    }

    // frame-major store of one 32x32 tile: out[b][co][n], co = c0 + local row
    __device__ __forceinline__ void store_plain(float* base, int Cn, int c0, int i, int j, int n) {
        if (n >= p.To) return;
        float* ob = base + ((long long)b * Cn + c0) * p.To + n;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = (r & 3) + 8 * (r >> 2) + 4 * h;
            float v = acc[0][i][j][r];
            if constexpr (VOC) {
                if (p.out_div != 1.0f) v = v / p.out_div;
                if (p.act_slope != 0.f) v = (v >= 0.f) ? v : v * p.act_slope;
                if constexpr (BN < 256) {      // (ragged batch: zeros beyond the utterance's length; the launcher keeps ragged calls off the 256-wide tile, which has no register to spare)
                    if (p.vlen && n >= voc_len()) v = 0.f;
                }
            }
            if (c0 + rl < Cn) ob[rl * p.To] = v;
        }
    }

    // attention's VT layout for the value channels (attention_k4p.hip): [B][head][ceil(To/4)][D][4], element = V[d] at 4
    // consecutive frames; frames To .. ceil4(To)-1 are written as zeros (they are multiplied by zero probabilities).
    // Sixteen predicated 4-byte stores per lane: a VT entry is one channel at four frames, and a lane of the MFMA's output holds one frame.
    // Whole 16-byte entries from a transposed tile (operands exchanged) were built and measured 0.46 ms per step, inside the A/B's spread:
    // taken out again.  As write-through stores (sc1) these measured 0.9 ms per step SLOWER than left dirty
    __device__ __forceinline__ void store_vt(int c0, int i, int j, int n) {
        const int T4 = (p.To + 3) & ~3, D = p.vt_D, Cv = p.Cout - p.plain_from;
        if (n >= T4) return;
        const bool real = n < p.To;
        const int head0 = c0 / D, rem0 = c0 - head0 * D;
        float* ob = p.out2 + (long long)b * Cv * T4 + (long long)(n >> 2) * D * 4 + (n & 3);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = (r & 3) + 8 * (r >> 2) + 4 * h;
            int d = rem0 + rl, head = head0;
            if (d >= D) { d -= D; ++head; }
            if (c0 + rl < Cv) ob[(long long)head * D * T4 + d * 4] = real ? acc[0][i][j][r] : 0.f;
        }
    }

    // K4P addressing of one 32x32 tile.  Registers (4g+hh, 4g+2+hh) of this lane are elements (2h, 2h+1) of row
    // (q = tile0/8 + g, hh): two 8-byte accesses per 8-channel block; the two lane halves together fill the 16-byte entry,
    // and consecutive lanes are consecutive frames.
    __device__ __forceinline__ int k4p_off(int tile0, int n) const { return (((tile0 >> 3) * 2) * (p.To + 2 * p.opad) + n + p.opad) * 4 + 2 * h; }
    __device__ __forceinline__ int k4p_ck() const { return (p.plain_from < p.Cout) ? p.plain_from : p.Cout; }

    // phase 2: residual add (all loads in flight together, before any store)
    __device__ __forceinline__ void add_residual(int tile0, int i, int j, int n) {
        if (n >= p.To) return;
        f32x2 rv[8];
        if constexpr (EARLY) {
#pragma unroll
            for (int e = 0; e < 8; ++e) rv[e] = rsv[(i * TN + j) * 8 + e];
        } else {
            const int Tpo = p.To + 2 * p.opad;
            const float* rb = p.res + (long long)b * k4p_ck() * Tpo + k4p_off(tile0, n);
#pragma unroll
            for (int e = 0; e < 8; ++e) rv[e] = *reinterpret_cast<const f32x2*>(rb + e * Tpo * 4);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                acc[0][i][j][4 * g + hh] += rv[2 * g + hh][0];
                acc[0][i][j][4 * g + 2 + hh] += rv[2 * g + hh][1];
            }
    }

    // phase 2b (vocoder): the MRF running sum, a K4P tensor with the output's channels / frames / padding whatever the output layout is;
    // its loads for all tiles of the wave are in flight together, before any store
    __device__ __forceinline__ void add_running_sum(int tile0, int i, int j, int n) {
        if (n >= p.To) return;
        const int Tpo = p.To + 2 * p.opad;
        const float* ab = p.acc_in + (long long)b * (p.out_plain ? p.Cout : k4p_ck()) * Tpo + k4p_off(tile0, n);
        f32x2 av[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) av[e] = *reinterpret_cast<const f32x2*>(ab + e * Tpo * 4);
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                acc[0][i][j][4 * g + hh] += av[2 * g + hh][0];
                acc[0][i][j][4 * g + 2 + hh] += av[2 * g + hh][1];
            }
    }

    // polyphase ConvTranspose store (vocoder upsamplers): row m = co * phases + phase, column n -> frame n * phases + phase - tpad of
    // channel co; the raw value goes to `out` and its LeakyReLU to `out_act` (the next resblocks' residual and first input).  A
    // workgroup's 64 rows x 128 columns cover whole 64-byte lines between them (8 channels x 4 frames per line), written back from L2.
    __device__ __forceinline__ void store_phases(int tile0, int i, int j, int n) {
        const int lg = p.ph_log2, Tpo = p.ph_Tout + 2 * p.opad;
        const long long ob = (long long)b * p.ph_Cout * Tpo;
        const int Lv = p.vlen ? voc_len() : 0x7fffffff;      // ragged batch: zeros beyond the utterance's output length
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = tile0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            const int co = m >> lg, f = (n << lg) + (m & ((1 << lg) - 1)) - p.ph_tpad;
            const bool ok = n < p.To && f >= 0 && f < p.ph_Tout && co < p.ph_Cout;
            const long long off = ob + (long long)(((co >> 3) * 2 + (co & 1)) * Tpo + f + p.opad) * 4 + ((co & 7) >> 1);
            const float v = (f < Lv) ? acc[0][i][j][r] : 0.f;
            if (ok) {
                p.out[off] = v;
                if (p.out_act) p.out_act[off] = (v >= 0.f) ? v : v * p.act_slope;
            }
        }
    }

    // phase 3: K4P store of one 32x32 tile (+ pad frames, + GroupNorm / LayerNorm partials).  Vocoder epilogues: the running
    // sum of the MRF (acc_in, out_div), LeakyReLU of the value for the next convolution (act_slope; out_act = second tensor
    // when the raw value is needed too, as a residual).
    __device__ __forceinline__ void store_k4p(int tile0, int i, int j, int n) {
        const int Tpo = p.To + 2 * p.opad;
        const int Ck = k4p_ck();
        const bool ok = n < p.To;
        const long long o0 = (long long)b * Ck * Tpo + k4p_off(tile0, n);
        float* ob = p.out + o0;
        if constexpr (!VOC) {
            // 16-byte write-through entries (k4p.h k4p_tile_entries): the swaps run here, with every lane active; lane half h then
            // owns row (q, hh = h) of each 8-channel block, pad frames included.  The statistics below read the accumulators as they were.
            k4p_f32x4 ent[4];
            k4p_tile_entries(acc[0][i][j], ent);
            const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(p.out + (long long)b * Ck * Tpo, 0, Ck * Tpo * 4, 0x00020000);
            const int e0 = k4p_entry_off(tile0 >> 3, h, Tpo, n + p.opad);
            if (ok) {
#pragma unroll
                for (int g = 0; g < 4; ++g) k4p_store16_wt(ro, e0 + g * 2 * Tpo * 16, ent[g]);
                if (p.opad == 1) {                // one pad frame per side is written with the tensor; wider pads are zeroed by k4p_zero_pads
                    if (n == 0) {                 // left pad frame
#pragma unroll
                        for (int g = 0; g < 4; ++g) k4p_store16(ro, e0 + g * 2 * Tpo * 16 - 16, k4p_f32x4{0.f, 0.f, 0.f, 0.f});
                    }
                    if (n == p.To - 1) {          // right pad frame
#pragma unroll
                        for (int g = 0; g < 4; ++g) k4p_store16(ro, e0 + g * 2 * Tpo * 16 + 16, k4p_f32x4{0.f, 0.f, 0.f, 0.f});
                    }
                }
            }
        } else if (ok) {      // the vocoder's store path: its epilogue options, then 8-byte halves of the entries
            if constexpr (BN < 256) {
                if (p.vlen && n >= voc_len()) {      // ragged batch: this stage's frames beyond the utterance's length are written as zeros
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[0][i][j][r] = 0.f;
                }
            }
            if (p.out_div != 1.0f) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[0][i][j][r] = acc[0][i][j][r] / p.out_div;
            }
            if (p.act_slope != 0.f && p.out_act) {      // raw value to `out`, activated value to `out_act`
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int hh = 0; hh < 2; ++hh) k4p_store_wt(ob + (2 * g + hh) * Tpo * 4, f32x2{acc[0][i][j][4 * g + hh], acc[0][i][j][4 * g + 2 + hh]});
                ob = p.out_act + o0;
            }
            if (p.act_slope != 0.f) {
#pragma unroll
                for (int r = 0; r < 16; ++r) { const float v = acc[0][i][j][r]; acc[0][i][j][r] = (v >= 0.f) ? v : v * p.act_slope; }
            }
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int hh = 0; hh < 2; ++hh)
                    k4p_store_wt(ob + (2 * g + hh) * Tpo * 4, f32x2{acc[0][i][j][4 * g + hh], acc[0][i][j][4 * g + 2 + hh]});
            if (p.opad == 1) {                    // one pad frame per side is written with the tensor; wider pads are zeroed by k4p_zero_pads
                if (n == 0) {                     // left pad frame
#pragma unroll
                    for (int e = 0; e < 8; ++e) *reinterpret_cast<f32x2*>(ob + e * Tpo * 4 - 4) = f32x2{0.f, 0.f};
                }
                if (n == p.To - 1) {              // right pad frame
#pragma unroll
                    for (int e = 0; e < 8; ++e) *reinterpret_cast<f32x2*>(ob + e * Tpo * 4 + 4) = f32x2{0.f, 0.f};
                }
            }
        }
        if (p.gnpart_out) {
            // GroupNorm statistics of the tensor being written, for the consumer's streaming normalisation (k4p_ops.hip
            // gn_stream): per (16 channels x 32 frames) block one (mean, M2) over its valid frames.  Registers 0..7 of a
            // lane are channels tile0 + 0..15, registers 8..15 channels tile0 + 16..31; sums of (x - k) and (x - k)^2 with
            // k = the block's first element (a shift near the mean keeps the sum-of-squares form free of cancellation),
            // reduced over the wave in a fixed order.
            const float k0 = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, acc[0][i][j][0])));
            const float k1 = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, acc[0][i][j][8])));
            float a1 = 0.f, a2 = 0.f, b1 = 0.f, b2 = 0.f;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const float d0 = acc[0][i][j][r] - k0, d1 = acc[0][i][j][r + 8] - k1;
                a1 += d0; a2 = fmaf(d0, d0, a2);
                b1 += d1; b2 = fmaf(d1, d1, b2);
            }
            if (n >= Lout) { a1 = 0.f; a2 = 0.f; b1 = 0.f; b2 = 0.f; }      // (Lout <= To: frames beyond the utterance's length carry no statistics)
            a1 = wave_sum_to_lane63(a1); a2 = wave_sum_to_lane63(a2);
            b1 = wave_sum_to_lane63(b1); b2 = wave_sum_to_lane63(b2);
            const int n0 = n - c;                                   // first frame of this 32-frame block
            const int nv = (Lout - n0 < 32) ? Lout - n0 : 32;       // valid frames
            if (lane == 63 && nv > 0) {
                const float cnt = 16.0f * (float)nv, rc = 1.0f / cnt;
                float2* gp = p.gnpart_out + ((long long)b * (Ck >> 4) + (tile0 >> 4)) * ((p.To + 31) >> 5) + (n0 >> 5);
                gp[0] = make_float2(k0 + a1 * rc, fmaxf(a2 - a1 * a1 * rc, 0.f));
                if (tile0 + 16 < Ck) gp[(p.To + 31) >> 5] = make_float2(k1 + b1 * rc, fmaxf(b2 - b1 * b1 * rc, 0.f));
            }
        }
        if (p.lnpart_out) {
            // per-frame (mean, M2) over this tile's 32 channels -> LayerNorm partials (combined by the consumer, ln_columns)
            float s1 = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) s1 += acc[0][i][j][r];
            const float m16 = s1 * (1.0f / 16.0f);
            float qv = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) { const float d = acc[0][i][j][r] - m16; qv += d * d; }
            const float mo = __shfl_xor(m16, 32, 64), qo = __shfl_xor(qv, 32, 64);
            const float d = mo - m16;
            if (h == 0 && ok)
                p.lnpart_out[((long long)b * (Ck >> 5) + (tile0 >> 5)) * p.To + n] = make_float2(0.5f * (m16 + mo), (qv + qo) + d * d * 8.0f);
        }
    }

    __device__ __forceinline__ int tile_ch(int i, bool geglu) const {      // first output channel of tile row i
        return geglu ? (m0 + wm * 64) / 2 : (m0 + wm * TM * 32 + i * 32);
    }

    // split-K: the ks = 1 waves hand their partial tile to the ks = 0 wave of the same column block through LDS
    __device__ __forceinline__ bool join_halves() {
        if constexpr (NACC == 2) acc[0][0][0] += acc[1][0][0];
        __syncthreads();                                   // every wave is done reading operand tiles: the stages are free
        float* red = smem + wn * 16 * 64 + lane;
        if (ks == 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) red[r * 64] = acc[0][0][0][r];
        }
        __syncthreads();
        if (ks == 1) return false;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][0][0][r] += red[r * 64];
        if constexpr (NACC == 2) acc[1][0][0] = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        return true;
    }

    // Cluster split-K (latency mode, DmaConvArgs::ksplit = S > 1): S workgroups share one output tile, each reducing 1/S of the K range.
    // The hand-off follows ONE row of the hand-off table in MI355X_MICROARCH.md (inter-workgroup visibility, "ONE lane of each storing
    // workgroup, for ALL that workgroup's stores ... all those lanes add to ONE unsharded counter, the workgroup whose add came last, told
    // by the value its add returned"), in every cell:
    //   * every wave stores its partial accumulators with sc1 (write-through) stores, 4 bytes each, and waits for their acknowledgement
    //     (s_waitcnt vmcnt(0)); a workgroup barrier then makes that true of ALL the workgroup's stores;
    //   * one lane of the workgroup adds 1 to the tile's counter (agent-scope atomic, one counter per tile); the add that returns S - 1 came last;
    //   * that lane tells the workgroup's other waves through an LDS word behind a second barrier -- nobody loads a partial before it;
    //   * the last workgroup's waves read all S partials back with sc1 loads (its own included) in the fixed order s = 0 .. S-1, so the sum does
    //     not depend on the order of arrival, and run the epilogue; the others leave.  Nobody ever waits for another workgroup.
    // One workgroup per CU (the launcher keeps a split grid within the chip), memory from hipMalloc.  The counter is put back to zero by the
    // last workgroup after its loads are issued: the next reader of the counter is the next launch.
    __device__ __forceinline__ bool cluster_join() {
        const int S = p.ksplit;
        if constexpr (NACC == 2) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[0][i][j] += acc[1][i][j];
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[1][i][j][r] = 0.f;
                }
        }
        const int slot = ctile * 4 + wave;
        float* mine = p.kpart + ((long long)slot * S + ksp) * (TM * TN * 1024) + lane;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    __hip_atomic_store(mine + ((i * TN + j) * 16 + r) * 64, acc[0][i][j][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's stores are acknowledged ...
        __syncthreads();                                      // ... and so are those of every other (live) wave of the workgroup; the stages are free
        int* last = reinterpret_cast<int*>(smem);
        if (threadIdx.x == 0) {                               // (wave 0 is a joining wave of every tile shape: split tiles keep waves 0 and 1)
            const unsigned old = __hip_atomic_fetch_add(p.kcount + ctile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *last = (old == (unsigned)(S - 1)) ? 1 : 0;
        }
        __syncthreads();
        if (*last == 0) return false;
        const float* all = p.kpart + (long long)slot * S * (TM * TN * 1024) + lane;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[0][i][j][r] = __hip_atomic_load(all + ((i * TN + j) * 16 + r) * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int q = 1; q < S; ++q) {
            const float* pq = all + (long long)q * (TM * TN * 1024);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[0][i][j][r] += __hip_atomic_load(pq + ((i * TN + j) * 16 + r) * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (threadIdx.x == 0) __hip_atomic_store(p.kcount + ctile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return true;
    }

    template <bool FOLD = true>      // (false: the fused pair, whose launcher admits no LayerNorm fold -- its epilogue carries none of the fold's code)
    __device__ __forceinline__ void epilogue() {
        const bool geglu = (p.epi == EPI_GEGLU || (ACT2 == 2 && p.epi == EPI_GLU)) && (TM == 2);
        if constexpr (SPLIT) {
            if (!join_halves()) return;
        }
        if constexpr (TM * TN <= 2 && !VOC) {      // (the launcher asks for a cluster split on waves of one or two blocks only)
            if (p.ksplit > 1) {
                if (!cluster_join()) return;
            }
        }
        finalize<FOLD>(geglu);
        const int ni = geglu ? 1 : TM;
        if (p.res) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                if (i >= ni) break;
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int tile0 = tile_ch(i, geglu);
                    if (tile0 < p.plain_from && tile0 < p.Cout) add_residual(tile0, i, j, t0 + wn * TN * 32 + j * 32 + c);
                }
            }
        }
        if constexpr (VOC) {
            if (p.acc_in) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        const int tile0 = tile_ch(i, geglu);
                        if (tile0 < p.Cout) add_running_sum(tile0, i, j, t0 + wn * TN * 32 + j * 32 + c);
                    }
            }
        } else {
            if (p.lens) {      // ragged batch: frames at and beyond this utterance's length are written as zeros, in whatever layout
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if (t0 + wn * TN * 32 + j * 32 + c >= Lout) {
#pragma unroll
                        for (int i = 0; i < TM; ++i)
#pragma unroll
                            for (int r = 0; r < 16; ++r) acc[0][i][j][r] = 0.f;
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            if (i >= ni) break;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = t0 + wn * TN * 32 + j * 32 + c;
                const int tile0 = tile_ch(i, geglu);
                if constexpr (VOC && KT == 2) {      // (the polyphase upsamplers are the 2-tap instantiations)
                    if (p.ph_Tout) { store_phases(tile0, i, j, n); continue; }
                }
                if (p.out_plain) store_plain(p.out, p.Cout, tile0, i, j, n);
                else if (tile0 >= p.plain_from) {
                    if (p.vt_D) store_vt(tile0 - p.plain_from, i, j, n);
                    else store_plain(p.out2, p.Cout - p.plain_from, tile0 - p.plain_from, i, j, n);
                }
                else if (tile0 < p.Cout) store_k4p(tile0, i, j, n);
            }
        }
    }
};

template <int BM, int BN, int KT, int STRIDE, bool UPS, int BK, int NST, int DIL = 1, bool VOC = false, bool GNF = false, bool GELU = false, int ACT2 = 0>
// (the polyphase upsampler's scatter epilogue needs more than the 128 registers of 4 workgroups per CU: 2 per CU, no spills)
__global__ void __launch_bounds__(256, ((VOC && KT == 2) ? 2 : DmaCfg<BM, BN, KT, STRIDE, UPS, BK, NST, DIL>::OCC)) conv_dma_kernel(const DmaConvArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    DmaKernel<BM, BN, KT, STRIDE, UPS, BK, NST, DIL, VOC, GNF, GELU, ACT2> k(p, smem);
    k.setup_keep_acc();
    // ragged batch: a tile that lies wholly beyond its utterance's length has nothing to reduce -- the epilogue writes its zeros (what it
    // computes from the untouched accumulators never reaches memory: masked columns are stored as literal zeros)
    if (!k.dead_tile()) k.mainloop();
    else k.zero_acc();
    k.epilogue();
}

// Two reductions into one set of accumulators: the k 3 convolution of a resnet's second half, then its 1x1 shortcut over the block
// input (two K4P sources), then ONE epilogue (launch_conv_dma_pair).  The second phase starts its own DMA ring after the first has
// drained (one exposed first-tile latency, ~2 us, against a launch, ~8 us, and the shortcut tensor's round trip through memory).
struct DmaPairArgs { DmaConvArgs a3, a1; };

template <int BM, int BN, int BK3, int BK1, int NST>
struct PairCfg {
    using C3 = DmaCfg<BM, BN, 3, 1, false, BK3, NST, 1>;
    using C1 = DmaCfg<BM, BN, 1, 1, false, BK1, NST, 1>;
    static constexpr size_t LDS_BYTES = C3::LDS_BYTES > C1::LDS_BYTES ? C3::LDS_BYTES : C1::LDS_BYTES;
    static constexpr int OCC = C3::OCC < C1::OCC ? C3::OCC : C1::OCC;
    static_assert(C3::NACC == C1::NACC && C3::TM == C1::TM && C3::TN == C1::TN && C3::SPLIT == C1::SPLIT, "the phases share the accumulators");
};

template <int BM, int BN, int BK3, int BK1, int NST>
__global__ void __launch_bounds__(256, (PairCfg<BM, BN, BK3, BK1, NST>::OCC)) conv_dma_pair_kernel(const DmaPairArgs pp) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    using K3 = DmaKernel<BM, BN, 3, 1, false, BK3, NST, 1, false>;
    using K1 = DmaKernel<BM, BN, 1, 1, false, BK1, NST, 1, false>;
    K1 k1(pp.a1, smem);
    {
        K3 k3(pp.a3, smem);
        k3.setup_keep_acc();
        if (!k3.dead_tile()) k3.template mainloop<false, true>();
        else k3.zero_acc();
#pragma unroll
        for (int a = 0; a < K3::NACC; ++a)
#pragma unroll
            for (int i = 0; i < K3::TM; ++i)
#pragma unroll
                for (int j = 0; j < K3::TN; ++j) k1.acc[a][i][j] = k3.acc[a][i][j];
    }
    __syncthreads();                // every wave is done reading the first phase's stages
    k1.setup_keep_acc();
    if (!k1.dead_tile()) k1.template mainloop<true, false>();
    k1.template epilogue<false>();
}

// the constants of the kernel's block-index decomposition (kernels.h dma_tile_of): divisors nMb, nN, S
static void dma_set_order(DmaConvArgs& a, int nMb, int nN, int S) {
    const DmaMagic m0 = dma_magic((unsigned)nMb), m1 = dma_magic((unsigned)nN), m2 = dma_magic((unsigned)S);
    a.ord_m[0] = m0.m; a.ord_m[1] = m1.m; a.ord_m[2] = m2.m;
    a.ord_s = m0.s | (m1.s << 8) | (m2.s << 16);
}

static thread_local char g_dcfg[96] = "";
const char* conv_dma_last_config() { return g_dcfg; }

template <int BM, int BN, int KT, int STRIDE, bool UPS, int BK, int NST, int DIL = 1, bool VOC = false, bool GNF = false, bool GELU = false, int ACT2 = 0>
static hipError_t launch_dma_cfg(DmaConvArgs& a, hipStream_t s) {      // (a: the copy launch_conv_dma owns; the order constants are set in it)
    using Cfg = DmaCfg<BM, BN, KT, STRIDE, UPS, BK, NST, DIL>;
    if (GNF != (a.gnf_part != nullptr) || GELU != (a.epi == EPI_GELU) || (ACT2 == 1) != (a.epi == EPI_SWISH) || (ACT2 == 2) != (a.epi == EPI_GLU)) return hipErrorInvalidValue;
    const size_t lds_bytes = Cfg::LDS_BYTES + (GNF ? (BM + 32) * sizeof(float) : 0);      // the fold's row constants and group statistics sit behind the ring
    const int nN = (a.To + BN - 1) / BN;
    const int S = a.ksplit > 1 ? a.ksplit : 1;
    if (S > 1 && (Cfg::TM * Cfg::TN > 2 || VOC || (a.Ci / BK) % S)) return hipErrorInvalidValue;
    dim3 grid((a.Mp / BM) * nN, a.B * S);
    dma_set_order(a, a.Mp / BM, nN, S);
    auto kern = conv_dma_kernel<BM, BN, KT, STRIDE, UPS, BK, NST, DIL, VOC, GNF, GELU, ACT2>;
    if (lds_bytes > 48 * 1024) {
        static std::atomic<unsigned long long> attr_done{0};
        hipError_t e = ensure_max_dynamic_lds(reinterpret_cast<const void*>(kern), attr_done);
        if (e != hipSuccess) return e;
    }
    const char* gtag = GNF ? " GNF" : GELU ? " GELU" : ACT2 == 1 ? " SWISH" : ACT2 == 2 ? " GLU" : "";
    if (!VOC && S > 1) snprintf(g_dcfg, sizeof(g_dcfg), "BM%d BN%d KT%d S%d U%d BK%d NST%d KS%d%s grid %ux%u lds %zu", BM, BN, KT, STRIDE, (int)UPS, BK, NST, S, gtag, grid.x, grid.y, lds_bytes);
    else if (!VOC) snprintf(g_dcfg, sizeof(g_dcfg), "BM%d BN%d KT%d S%d U%d BK%d NST%d%s grid %ux%u lds %zu", BM, BN, KT, STRIDE, (int)UPS, BK, NST, gtag, grid.x, grid.y, lds_bytes);
    else snprintf(g_dcfg, sizeof(g_dcfg), "BM%d BN%d KT%d S%d U%d BK%d NST%d D%d grid %ux%u lds %zu", BM, BN, KT, STRIDE, (int)UPS, BK, NST, DIL, grid.x, grid.y, Cfg::LDS_BYTES);
    hipEvent_t e0, e1;
    if (prof_attach_events(&e0, &e1)) hipExtLaunchKernelGGL(kern, grid, dim3(256), lds_bytes, s, e0, e1, 0, a);      // bench.py's roofline leg
    else hipLaunchKernelGGL(kern, grid, dim3(256), lds_bytes, s, a);
    return hipGetLastError();
}

#define DCASE(BM, BN, KT, ST, UP, BK, NS) return launch_dma_cfg<BM, BN, KT, ST, UP, BK, NS>(a, s)

// tile shape / K-step / ring depth of one launch (cfg = 0: the measured rules below)
static void dma_pick(const DmaConvArgs& a, int cfg, int& bm, int& bn, int& bk, int& nst) {
    const bool k32 = (a.Ci % 32 == 0) && (a.C1 % 32 == 0), k64 = (a.Ci % 64 == 0) && (a.C1 % 64 == 0);
    // The tile shape fixes the order of the K reduction, so it must not depend on the batch size: an utterance's result is then
    // bit-identical for any batch split.  Grid sizes are therefore judged at the nominal per-GPU batch of
    // BASELINE.json (16 utterances), whatever a.B is.
    // (a.tile_batch > 0: the opt-in latency mode judges them at the actual batch instead, kernels.h)
    const long long kNominalBatch = a.tile_batch > 0 ? a.tile_batch : 16;
    auto blocks = [&](int bm, int bn) -> long long { return (a.Mp % bm) ? -1 : (long long)(a.Mp / bm) * ((a.To + bn - 1) / bn) * kNominalBatch; };
    if (cfg) {
        bm = cfg / 1000000; bn = (cfg / 1000) % 1000; bk = (cfg / 10) % 100; nst = cfg % 10;
    } else if (a.stride == 1 && !a.ups && a.epi != EPI_GEGLU && k32 && (blocks(64, 64) <= 256 || (blocks(64, 64) < 512 && blocks(64, 64) % 256))) {
        // fewer 64 x 64 tiles than CUs (the T/8 and T/4 levels at small batch): 32 x 64 tiles with the K range split over the
        // workgroup's two wave pairs put twice as many CUs to work (tools/bench_dconv.py: 1.6x at 128 tiles, ~1.1x at 256);
        // 1.5 tiles per CU (384: the T/2 level) leave half the chip idle in the second round, 3 half tiles per CU do not (1.2x)
        bm = 32; bn = 64; bk = (a.KT == 1 && k64) ? 64 : 32; nst = 2;
    } else {
        // Pick the tile by a small occupancy model fitted to tools/bench_dconv.py sweeps: a CU runs its n workgroups r at a
        // time (r = LDS residency, <= 4); r >= 3 co-resident workgroups keep the matrix pipe full, 2 reach ~0.9, a lone one
        // ~0.62 (nothing hides its barriers / LDS latency).  Short reductions (Ci <= 512) prefer many small stages (BK 16, 3-deep
        // ring), long ones few big stages (BK 64, 2-deep).
        struct Cand { int bm, bn, bk, nst; double eff; };
        Cand cands[3];
        int nc = 0;
        if (a.stride == 2 || a.ups) {
            cands[nc++] = {64, 64, 32, 2, 0.93};
        } else if (a.KT == 3) {
            cands[nc++] = {64, 64, 32, 2, 0.93};
            if (a.Mp % 128 == 0) cands[nc++] = {128, 128, 16, 2, 1.0};
        } else if (a.epi == EPI_GEGLU) {
            // measured (tools/bench_dconv.py ff1_*): the 128 x 128 tile wins whenever a frame block is not half empty
            if (a.To > 64) cands[nc++] = {128, 128, a.Ci >= 384 ? 16 : 32, 2, 1.0};
            else cands[nc++] = {128, 64, 32, 2, 0.97};
        } else {
            // short reductions: one resident wave of workgroups (<= 768) prefers BK 32 x 2 stages, a grid several waves deep the
            // lighter BK 16 x 3 (more workgroups per CU to overlap prologues / epilogues); long ones few big stages
            if (a.Ci > 512) cands[nc++] = {64, 64, 64, 2, 0.93};
            else if (blocks(64, 64) <= 768) cands[nc++] = {64, 64, 32, 2, 0.93};
            else cands[nc++] = {64, 64, 16, 3, 0.93};
            if (a.Mp % 128 == 0) cands[nc++] = {128, 64, 32, 2, 0.97};
        }
        double best = 1e300;
        bm = cands[0].bm; bn = cands[0].bn; bk = cands[0].bk; nst = cands[0].nst;
        for (int i = 0; i < nc; ++i) {
            const Cand& c = cands[i];
            const long long nblk = blocks(c.bm, c.bn);
            if (nblk < 0) continue;
            const int xw = a.ups ? c.bn / 2 + 2 : (c.bn - 1) * a.stride + a.KT;
            const double lds = 4.0 * c.nst * (a.KT * c.bk * c.bm + (c.bk / 4) * xw * 4);
            int r = (int)(160.0 * 1024 / lds);
            r = r < 1 ? 1 : (r > 4 ? 4 : r);
            if (c.bm * c.bn >= 128 * 128 && r > 2) r = 2;
            const long long n = (nblk + 255) / 256;
            static const double e[5] = {1.0, 0.62, 0.9, 1.0, 1.0};
            const double cost = ((double)(n / r) * r / e[r] + (double)(n % r) / e[n % r]) * c.bm * c.bn / c.eff;
            if (cost < best) { best = cost; bm = c.bm; bn = c.bn; bk = c.bk; nst = c.nst; }
        }
        // Small ACTUAL batches (the one-utterance caller): a 128 x 64 tile sums k in exactly the order of the 128 x 128 tile (one
        // accumulator chain per output, same BK), so splitting the tile when the real grid leaves most of the chip idle changes the
        // timing and nothing else -- the bit-identity between B = 1 and batched results holds.
        if (bm == 128 && bn == 128 && (long long)(a.Mp / 128) * ((a.To + 127) / 128) * a.B < 192) bn = 64;
    }
}

// Latency mode: how many workgroups share one output tile's K range (1 = no cluster split).  Doubled while the grid stays within
// one workgroup per CU (a CU with two takes twice as long), the K-steps divide evenly and every share keeps >= min_steps of them.
static int cluster_split(const DmaConvArgs& a, int bm, int bn, int nk, int nk2, int min_steps) {
    if (a.tile_batch <= 0 || !a.kpart || !a.kcount || a.voc || bm * bn > 128 * 64) return 1;
    const int blk = bm * bn > 64 * 64 ? 2 : 1;      // 32 x 32 blocks per wave
    const long long tiles = (long long)(a.Mp / bm) * ((a.To + bn - 1) / bn) * a.B;
    if (tiles * 4 > a.kcount_cap) return 1;
    int S = 1;
    while (S < 16 && tiles * S * 2 <= 256 && nk % (S * 2) == 0 && nk / (S * 2) >= min_steps && (nk2 == 0 || (nk2 % (S * 2) == 0)) &&
           tiles * 4 * (S * 2) * blk * 1024 <= a.kpart_cap)
        S *= 2;
    return S;
}

template <int BM, int BN, int BK3, int BK1, int NST>
static hipError_t launch_pair_cfg(DmaConvArgs& a3, DmaConvArgs& a1, hipStream_t s) {      // (the copies launch_conv_dma_pair owns)
    using Cfg = PairCfg<BM, BN, BK3, BK1, NST>;
    const int nN = (a1.To + BN - 1) / BN;
    const int S = a1.ksplit > 1 ? a1.ksplit : 1;
    if (S > 1 && (Cfg::C1::TM * Cfg::C1::TN != 1 || a3.ksplit != a1.ksplit || (a3.Ci / BK3) % S || (a1.Ci / BK1) % S)) return hipErrorInvalidValue;
    dim3 grid((a1.Mp / BM) * nN, a1.B * S);
    dma_set_order(a3, a1.Mp / BM, nN, S);
    dma_set_order(a1, a1.Mp / BM, nN, S);
    auto kern = conv_dma_pair_kernel<BM, BN, BK3, BK1, NST>;
    if (Cfg::LDS_BYTES > 48 * 1024) {
        static std::atomic<unsigned long long> attr_done{0};
        hipError_t e = ensure_max_dynamic_lds(reinterpret_cast<const void*>(kern), attr_done);
        if (e != hipSuccess) return e;
    }
    if (S > 1) snprintf(g_dcfg, sizeof(g_dcfg), "BM%d BN%d KT3+1 S1 U0 BK%d+%d NST%d KS%d grid %ux%u lds %zu", BM, BN, BK3, BK1, NST, S, grid.x, grid.y, Cfg::LDS_BYTES);
    else snprintf(g_dcfg, sizeof(g_dcfg), "BM%d BN%d KT3+1 S1 U0 BK%d+%d NST%d grid %ux%u lds %zu", BM, BN, BK3, BK1, NST, grid.x, grid.y, Cfg::LDS_BYTES);
    DmaPairArgs pp{a3, a1};
    hipEvent_t e0, e1;
    if (prof_attach_events(&e0, &e1)) hipExtLaunchKernelGGL(kern, grid, dim3(256), Cfg::LDS_BYTES, s, e0, e1, 0, pp);
    else hipLaunchKernelGGL(kern, grid, dim3(256), Cfg::LDS_BYTES, s, pp);
    return hipGetLastError();
}

// fused variant code for the pair, 0 = none: (BM << 16) | (BN << 8) | BK1
static int pair_variant(const DmaConvArgs& a3, const DmaConvArgs& a1) {
    auto plain = [](const DmaConvArgs& a) {
        return !a.voc && a.stride == 1 && !a.ups && a.dil == 1 && a.epi == EPI_NONE && a.xpad == 1 && a.opad == 1 && !a.ln_part && !a.ph_Tout && a.act_slope == 0.f &&
               !a.acc_in && a.out_div == 1.0f && a.Ci % 16 == 0 && a.C1 % 16 == 0 && a.Mp % 64 == 0 && a.B > 0 && a.To > 0;
    };
    if (!plain(a3) || !plain(a1) || a3.KT != 3 || a3.pad != 1 || a1.KT != 1 || a1.pad != 0 || a3.Mp != a1.Mp || a3.To != a1.To || a3.B != a1.B ||
        a3.Tsrc != a1.Tsrc || a1.res || a1.out_plain || a1.plain_from < a1.Cout || a1.lnpart_out)
        return 0;
    int bm, bn, bk, nst;
    dma_pick(a3, 0, bm, bn, bk, nst);      // the k 3 half carries most of the work: its tile
    const bool k3_32 = (a3.Ci % 32 == 0) && (a3.C1 % 32 == 0);
    const bool k1_64 = (a1.Ci % 64 == 0) && (a1.C1 % 64 == 0), k1_32 = (a1.Ci % 32 == 0) && (a1.C1 % 32 == 0);
    if (!k3_32 || bk != 32 || nst != 2 || !k1_32 || bn != 64 || (bm != 32 && bm != 64)) return 0;
    return (bm << 16) | (bn << 8) | (k1_64 ? 64 : 32);
}
bool conv_dma_pair_applies(const DmaConvArgs& a3, const DmaConvArgs& a1) { return pair_variant(a3, a1) != 0; }

hipError_t launch_conv_dma_pair(const DmaConvArgs& a3_, const DmaConvArgs& a1_, hipStream_t s) {
    DmaConvArgs a3 = a3_, a1 = a1_;
    const int pv = pair_variant(a3, a1);
    if (pv) {
        const int bm = pv >> 16, bn = (pv >> 8) & 255, bk1 = pv & 255;
        a3.ksplit = a1.ksplit = cluster_split(a1, bm, bn, a3.Ci / 32, a1.Ci / bk1, 1);
    }
    switch (pv) {
        case (32 << 16) | (64 << 8) | 64: return launch_pair_cfg<32, 64, 32, 64, 2>(a3, a1, s);
        case (32 << 16) | (64 << 8) | 32: return launch_pair_cfg<32, 64, 32, 32, 2>(a3, a1, s);
        case (64 << 16) | (64 << 8) | 64: return launch_pair_cfg<64, 64, 32, 64, 2>(a3, a1, s);
        case (64 << 16) | (64 << 8) | 32: return launch_pair_cfg<64, 64, 32, 32, 2>(a3, a1, s);
        default: return hipErrorNotSupported;
    }
}

// cfg = BM*1000000 + BN*1000 + BK*10 + NST (0 = auto)
hipError_t launch_conv_dma(const DmaConvArgs& a_, int cfg, hipStream_t s) {
    DmaConvArgs a = a_;
    a.ksplit = 1;
    if (a.Ci % 16 || a.C1 % 16 || a.Mp % 64 || a.B <= 0 || a.To <= 0 || a.xpad < 1 || a.opad < 1 || a.pad < 0 || a.pad > a.xpad) return hipErrorInvalidValue;
    if (a.ln_part && a.KT != 1) return hipErrorInvalidValue;      // the LayerNorm fold's epilogue exists in the 1x1 kernels only
    if (a.voc) {
        // vocoder resblock convolutions (k 3 / 7 / 11, dilation 1 / 3 / 5; LeakyReLU / running-sum epilogues): one 64 x 128 tile shape,
        // BK 16 (a K-step = 16 channels x all taps: 6 / 14 / 22 MFMA groups of 8 per wave), 2 stages (the weight tile of k 11 is 45 KB per stage)
        if (a.stride != 1 || a.ups || a.epi != EPI_NONE || cfg != 0) return hipErrorInvalidValue;
        if (a.ph_Tout) {      // upsampler: 2 taps per phase
            if (a.KT != 2 || a.dil != 1 || a.pad != 1 || a.res || a.acc_in || a.out_plain || a.out_div != 1.0f || a.ph_log2 < 0 || a.ph_log2 > 4 ||
                a.ph_Cout << a.ph_log2 != a.Co || a.ph_Cout % 8)
                return hipErrorInvalidValue;
            return launch_dma_cfg<64, 128, 2, 1, false, 16, 2, 1, true>(a, s);
        }
#define VCASE(KT_, D_) if (a.KT == KT_ && a.dil == D_) return launch_dma_cfg<64, 128, KT_, 1, false, 16, 2, D_, true>(a, s)
        // one M-block (64 output channels) and 11 taps: a 256-frame tile amortises the 45 KB weight tile over twice the columns
        // (measured 104 -> 114 TFLOP/s with the residual epilogue; k 3 / k 7 lose 7 % on the wide tile)
        if (a.Mp == 64 && a.KT == 11 && a.To >= 1024 && !a.vlen) {
#define WCASE(D_) if (a.dil == D_) return launch_dma_cfg<64, 256, 11, 1, false, 16, 2, D_, true>(a, s)
            WCASE(1); WCASE(3); WCASE(5);
#undef WCASE
        }
        VCASE(3, 1); VCASE(3, 3); VCASE(3, 5); VCASE(7, 1); VCASE(7, 3); VCASE(7, 5); VCASE(11, 1); VCASE(11, 3); VCASE(11, 5);
#undef VCASE
        return hipErrorInvalidValue;
    }
    if (a.dil != 1 || a.act_slope != 0.f || a.acc_in || a.out_div != 1.0f || a.ph_Tout) return hipErrorInvalidValue;      // vocoder-only features
    if (a.KT != 1 && a.KT != 3 && !(a.KT == 2 && a.stride == 2 && (a.epi == EPI_GELU || a.epi == EPI_NONE))) return hipErrorInvalidValue;      // (k 2: HuBERT's / wav2vec 2.0's conv5 / conv6)
    const bool k32 = (a.Ci % 32 == 0) && (a.C1 % 32 == 0), k64 = (a.Ci % 64 == 0) && (a.C1 % 64 == 0);
    int bm, bn, bk, nst;
    if (a.epi == EPI_GLU) {      // the tile rules of EPI_GEGLU (value and gate rows interleaved the same way)
        DmaConvArgs t = a;
        t.epi = EPI_GEGLU;
        dma_pick(t, cfg, bm, bn, bk, nst);
    } else {
        dma_pick(a, cfg, bm, bn, bk, nst);
    }
    if ((a.epi == EPI_GEGLU || a.epi == EPI_GLU) && bm != 128) return hipErrorInvalidValue;
    if (a.Mp % bm) return hipErrorInvalidValue;
    if ((bk == 64 && !k64) || (bk == 32 && !k32)) bk = 16;
    if (a.gnf_part) {
        // GroupNorm fold: a 1x1 convolution over one source whose every wave's share of a K-step lies inside one group
        if (a.KT != 1 || a.stride != 1 || a.ups || a.C2 != 0 || a.ln_part || a.epi != EPI_NONE || a.bias || !a.gnf_cg || !a.gnf_c2 || a.gnf_groups < 1 ||
            a.gnf_groups > 8 || a.Ci % a.gnf_groups || (a.Ci / a.gnf_groups) % 16)
            return hipErrorInvalidValue;
        const int gsz = a.Ci / a.gnf_groups;
        if (bm * bn > 128 * 64) bn = 64;
        while (gsz % (bm == 32 ? bk / 2 : bk)) bk /= 2;      // (a split tile's half K-step of 16 channels divides every group size)
        if (bm != 32 && bk == 16) nst = 3;
        if (cfg == 0) a.ksplit = cluster_split(a, bm, bn, a.Ci / bk, 0, 2);
#define GCASE(BM, BN, BK, NS) if (bm == BM && bn == BN && bk == BK && nst == NS) return launch_dma_cfg<BM, BN, 1, 1, false, BK, NS, 1, false, true>(a, s)
        GCASE(32, 64, 32, 2); GCASE(32, 64, 64, 2); GCASE(64, 64, 32, 2); GCASE(64, 64, 16, 3); GCASE(128, 64, 32, 2); GCASE(128, 64, 16, 3);
#undef GCASE
        return hipErrorInvalidValue;
    }
    if (a.epi == EPI_SWISH || a.epi == EPI_GLU) {
        // The Conformer's epilogues (w2v-BERT 2.0): instantiations of their own, so that the kernels of every other launch are compiled as before.
        // 1x1, stride 1, K4P output only.  Swish on EPI_GELU's tiles; GLU on EPI_GEGLU's (128 output rows = 64 value + 64 gate rows per workgroup).
        if (a.KT != 1 || a.stride != 1 || a.ups || a.plain_from < a.Cout || a.out_plain || a.gnf_part) return hipErrorInvalidValue;
#define XCASE(BM, BN, BK, NS, ACT) return launch_dma_cfg<BM, BN, 1, 1, false, BK, NS, 1, false, false, false, ACT>(a, s)
        if (a.epi == EPI_SWISH) {
            if (bm == 128 && k32) XCASE(128, 64, 32, 2, 1);
            if (k32) XCASE(64, 64, 32, 2, 1);
            XCASE(64, 64, 16, 2, 1);
        }
        if (bn == 128 && bk == 32) XCASE(128, 128, 32, 2, 2);
        if (bn == 128) XCASE(128, 128, 16, 2, 2);
        if (bk == 32) XCASE(128, 64, 32, 2, 2);
        XCASE(128, 64, 16, 2, 2);
#undef XCASE
    }
    if (a.epi == EPI_GELU) {
        // Plain-GELU epilogue (the Whisper encoder's conv1, conv2, mlp.0): a template flag, so that the kernels of every other launch are
        // compiled exactly as before, and a reduced set of tiles: the picked tile where it is one of these (it is for every shape of
        // the large-v3 encoder), else 64 x 64.  The choice depends on the shape and the nominal batch only, like dma_pick's.
        if (a.ups || a.plain_from < a.Cout || a.out_plain) return hipErrorInvalidValue;
#define ECASE(BM, BN, KT, ST, BK, NS) return launch_dma_cfg<BM, BN, KT, ST, false, BK, NS, 1, false, false, true>(a, s)
        if (a.KT == 1 && a.stride == 1) {
            if (bm == 128 && k32) ECASE(128, 64, 1, 1, 32, 2);
            if (k32) ECASE(64, 64, 1, 1, 32, 2);
            ECASE(64, 64, 1, 1, 16, 2);
        } else if (a.KT == 3 && a.stride == 1) {
            if (bm == 128 && bn == 128) ECASE(128, 128, 3, 1, 16, 2);
            if (bm == 128 && bn == 64) ECASE(128, 64, 3, 1, 16, 2);      // (the 128 x 128 tile's summation order: dma_pick)
            if (k32) ECASE(64, 64, 3, 1, 32, 2);
            ECASE(64, 64, 3, 1, 16, 2);
        } else if (a.KT == 3 && a.stride == 2) {
            if (k32) ECASE(64, 64, 3, 2, 32, 2);
            ECASE(64, 64, 3, 2, 16, 2);
        } else if (a.KT == 2 && a.stride == 2) {      // the HuBERT feature extractor's last two convolutions
            if (k32) ECASE(64, 64, 2, 2, 32, 2);
            ECASE(64, 64, 2, 2, 16, 2);
        }
#undef ECASE
        return hipErrorInvalidValue;
    }
    if (cfg == 0) a.ksplit = cluster_split(a, bm, bn, a.Ci / bk, 0, 2);
    const int key = a.KT * 100 + a.stride * 10 + (a.ups ? 1 : 0);
    const int tk = bm * 1000 + bn;
    if (key == 110) {
        if (tk == 64064) {
            if (bk == 64 && nst == 2) DCASE(64, 64, 1, 1, false, 64, 2);
            if (bk == 64 && nst == 3) DCASE(64, 64, 1, 1, false, 64, 3);
            if (bk == 32 && nst == 2) DCASE(64, 64, 1, 1, false, 32, 2);
            if (bk == 32 && nst == 3) DCASE(64, 64, 1, 1, false, 32, 3);
            if (bk == 16 && nst == 2) DCASE(64, 64, 1, 1, false, 16, 2);
            if (bk == 16 && nst == 3) DCASE(64, 64, 1, 1, false, 16, 3);
            if (bk == 64 && nst == 4) DCASE(64, 64, 1, 1, false, 64, 4);
            if (bk == 32 && nst == 4) DCASE(64, 64, 1, 1, false, 32, 4);
            if (bk == 32 && nst == 5) DCASE(64, 64, 1, 1, false, 32, 5);
            if (bk == 16 && nst == 4) DCASE(64, 64, 1, 1, false, 16, 4);
            if (bk == 16 && nst == 6) DCASE(64, 64, 1, 1, false, 16, 6);
        } else if (tk == 32064) {
            if (bk == 64) DCASE(32, 64, 1, 1, false, 64, 2);
            if (bk == 32) DCASE(32, 64, 1, 1, false, 32, 2);
        } else if (tk == 128064) {
            if (bk == 32 && nst == 2) DCASE(128, 64, 1, 1, false, 32, 2);
            if (bk == 32 && nst == 3) DCASE(128, 64, 1, 1, false, 32, 3);
            if (bk == 16 && nst == 2) DCASE(128, 64, 1, 1, false, 16, 2);
            if (bk == 16 && nst == 3) DCASE(128, 64, 1, 1, false, 16, 3);
            if (bk == 32 && nst == 4) DCASE(128, 64, 1, 1, false, 32, 4);
            if (bk == 16 && nst == 4) DCASE(128, 64, 1, 1, false, 16, 4);
        } else if (tk == 128128) {
            if (bk == 32 && nst == 2) DCASE(128, 128, 1, 1, false, 32, 2);
            if (bk == 32 && nst == 3) DCASE(128, 128, 1, 1, false, 32, 3);
            if (bk == 16 && nst == 2) DCASE(128, 128, 1, 1, false, 16, 2);
            if (bk == 16 && nst == 3) DCASE(128, 128, 1, 1, false, 16, 3);
            if (bk == 16 && nst == 4) DCASE(128, 128, 1, 1, false, 16, 4);
        }
    } else if (key == 310) {
        if (tk == 64064) {
            if (bk == 32 && nst == 2) DCASE(64, 64, 3, 1, false, 32, 2);
            if (bk == 32 && nst == 3) DCASE(64, 64, 3, 1, false, 32, 3);
            if (bk == 16 && nst == 2) DCASE(64, 64, 3, 1, false, 16, 2);
            if (bk == 16 && nst == 3) DCASE(64, 64, 3, 1, false, 16, 3);
            if (bk == 16 && nst == 4) DCASE(64, 64, 3, 1, false, 16, 4);
            if (bk == 32 && nst == 4) DCASE(64, 64, 3, 1, false, 32, 4);
        } else if (tk == 32064) {
            if (bk == 32) DCASE(32, 64, 3, 1, false, 32, 2);      // BK 64 and a 3-deep ring measured 0-25 % slower here (tools/bench_dconv.py)
        } else if (tk == 128064) {
            if (bk == 16 && nst == 2) DCASE(128, 64, 3, 1, false, 16, 2);
            if (bk == 16 && nst == 3) DCASE(128, 64, 3, 1, false, 16, 3);
        } else if (tk == 128128) {
            if (bk == 16 && nst == 2) DCASE(128, 128, 3, 1, false, 16, 2);
            if (bk == 16 && nst == 3) DCASE(128, 128, 3, 1, false, 16, 3);
        }
    } else if (key == 320 && tk == 64064) {
        if (bk == 32 && nst == 2) DCASE(64, 64, 3, 2, false, 32, 2);
        if (bk >= 16 && nst == 3) DCASE(64, 64, 3, 2, false, 16, 3);
        if (bk == 16 && nst == 2) DCASE(64, 64, 3, 2, false, 16, 2);
    } else if (key == 220 && tk == 64064) {      // the wav2vec 2.0 feature extractor's last two convolutions (their LayerNorm + GELU follow as a pass)
        if (bk == 32) DCASE(64, 64, 2, 2, false, 32, 2);
        DCASE(64, 64, 2, 2, false, 16, 2);
    } else if (key == 311 && tk == 64064) {
        if (bk == 32 && nst == 2) DCASE(64, 64, 3, 1, true, 32, 2);
        if (bk >= 16 && nst == 3) DCASE(64, 64, 3, 1, true, 16, 3);
        if (bk == 16 && nst == 2) DCASE(64, 64, 3, 1, true, 16, 2);
    }
    return hipErrorInvalidValue;
}

}  // namespace lds

// Test entries (include/lds_test.h), host only: the launchers' division constants and the kernel's block-index decomposition
extern "C" int lds_test_dma_magic_div(uint32_t d, uint32_t n_count, uint32_t* out) {
    if (d < 1 || d >= (1u << 31) || n_count > (1u << 31) || !out) return (int)hipErrorInvalidValue;
    const lds::DmaMagic m = lds::dma_magic(d);
    for (uint32_t n = 0; n < n_count; ++n) out[n] = lds::dma_magic_div(n, m.m, m.s);
    return 0;
}
extern "C" int lds_test_dma_tile_order(int nMb, int nN, int B, int S, int32_t* out) {
    if (nMb < 1 || nN < 1 || B < 1 || S < 1 || !out || (long long)nMb * nN * B * S >= (1ll << 31)) return (int)hipErrorInvalidValue;
    lds::DmaConvArgs a{};
    lds::dma_set_order(a, nMb, nN, S);
    const int total = nMb * nN * B * S;
    for (int id = 0; id < total; ++id) {
        const lds::DmaTile t = lds::dma_tile_of(id, total, nMb, nN, S, a.ord_m, a.ord_s);
        out[4 * id] = t.mb; out[4 * id + 1] = t.nb; out[4 * id + 2] = t.b; out[4 * id + 3] = t.ksp;
    }
    return 0;
}
