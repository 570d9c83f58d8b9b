// The resnets' k 3 / stride 1 / pad 1 convolution in the 1-D Winograd form F(2,3) (gfx950, v_mfma_f32_32x32x2_f32).
//
// Why this kernel exists.  The fp32 MFMA runs at the vector rate and does not overlap vector work (conv_dma.hip), so the only way left to
// shorten a K loop is to issue fewer MFMAs.  With g the three taps and d the zero-padded input, per output pair i:
//   U0 = g0, U1 = (g0 + g1 + g2) / 2, U2 = (g0 - g1 + g2) / 2, U3 = g2                              (pack time, model.hip wino_taps)
//   V0 = d[2i] - d[2i+2], V1 = d[2i+1] + d[2i+2], V2 = d[2i+2] - d[2i+1], V3 = d[2i+1] - d[2i+3]    (k4p_ops.hip gn_wino_kernel)
//   Mj = Uj . Vj   (a Ci-deep GEMM over T / 2 columns each);   Y[2i] = M0 + M1 + M2,   Y[2i+1] = M1 - M2 - M3
// Four column-products per output pair instead of six: two thirds of the MFMAs of the direct form.
// A resnet's conv2 + 1x1 shortcut runs through the same kernel as one reduction over Cm + Cin / 2 channels: the shortcut's taps and planes are
// appended along K so that they enter through the join above (model.hip wino_pair_taps / run_wconv_pair); nothing here knows.
//
// The kernel is built from conv_dma's parts.  A workgroup owns 32 output rows x 32 pairs (64 frames); wave j accumulates Mj, a 32 x 32
// tile in two chains, over the whole Ci.  Both operand tiles of a K-step -- the four taps' weight rows and the four planes' pair columns --
// arrive by buffer-addressed LDS-DMA into an NST-stage ring with counted vmcnt; the operand registers form a ring read one MFMA group
// ahead, through the K-step boundary.  No per-element vector work in the K loop.  The four tiles meet through LDS in a fixed order; the
// epilogue is spread over all four waves: wave (cb, fb) forms the 16 channels x 32 frames block (cb, fb) of the output, adds bias and
// residual, writes it as 16-byte write-through K4P entries (a lane's two frames of one row are 32 contiguous bytes) and reduces that
// block's GroupNorm partial (mean, M2) -- one partial is exactly one wave's block, so no second exchange is needed.
#include "k4p.h"
#include "kernels.h"
#include "../../include/lds_test.h"

#include <hip/hip_ext.h>

#include <stdio.h>

namespace lds {

typedef float wf32x16 __attribute__((ext_vector_type(16)));
typedef float wf32x4 __attribute__((ext_vector_type(4)));

template <int CTRL, int ROW_MASK, bool BOUND>
static __device__ __forceinline__ float wino_dpp_add(float v) {
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, BOUND));
}
// wave64 sum in a fixed order (conv_dma.hip wave_sum_to_lane63): the total is valid in lane 63
static __device__ __forceinline__ float wino_wave_sum(float v) {
    v = wino_dpp_add<0x111, 0xf, true>(v);
    v = wino_dpp_add<0x112, 0xf, true>(v);
    v = wino_dpp_add<0x114, 0xf, true>(v);
    v = wino_dpp_add<0x118, 0xf, true>(v);
    v = wino_dpp_add<0x142, 0xa, false>(v);
    v = wino_dpp_add<0x143, 0xc, false>(v);
    return v;
}

template <int BK, int NST>
struct WinoCfg {
    static constexpr int BM = 32, BP = 32;                       // output rows, frame pairs
    static constexpr int KR = BK / 4;                            // staged k-rows per K-step
    static constexpr int WFL = 4 * KR * BM * 4;                  // floats of a stage's weight half: [tap][k-row][row][4]
    static constexpr int VFL = KR * 4 * BP * 4;                  // ... and of its plane half: [k-row][plane][pair][4]
    static constexpr int STAGE = WFL + VFL;
    static constexpr int WPW = 4 * KR * BM / 256, VPW = KR * 4 * BP / 256;      // DMA wave-instructions per wave and tile
    static constexpr int PER_TILE = WPW + VPW;
    static constexpr int G = BK / 8;                             // MFMA groups (4 k-pairs each) per K-step and wave
    static constexpr int NB = 2;                                 // operand ring depth
    static constexpr int NLATE = 6;                              // the epilogue's operands, requested behind the first burst (late_loads)
    static constexpr int RS = 34;                                // row stride (floats) of the join buffer [4][32][RS]
    static constexpr size_t LDS_BYTES = (size_t)NST * STAGE * sizeof(float);
    static constexpr int OCC_LDS = (int)((160 * 1024) / LDS_BYTES);
    static constexpr int OCC = OCC_LDS < 4 ? OCC_LDS : 4;
    static_assert(G % NB == 0 && NB - 1 <= G, "ring slots must keep their phase across K-steps");
    static_assert(PER_TILE * (NST - 1) + NLATE <= 63, "vmcnt is a 6-bit field");
    static_assert(4 * BM * RS <= NST * STAGE, "the join buffer lives in the ring");
};

template <int BK, int NST>
struct WinoKernel {
    using Cfg = WinoCfg<BK, NST>;
    static constexpr int BM = Cfg::BM, BP = Cfg::BP, KR = Cfg::KR, WFL = Cfg::WFL, STAGE = Cfg::STAGE, WPW = Cfg::WPW, VPW = Cfg::VPW;
    static constexpr int PER_TILE = Cfg::PER_TILE, G = Cfg::G, NB = Cfg::NB, NLATE = Cfg::NLATE, RS = Cfg::RS;

    const WinoConvArgs& p;
    float* smem;
    // the arguments the first DMA issue depends on, requested in one burst at kernel entry (conv_dma.hip load_hot)
    struct Hot {
        const float *v, *u;
        int Ci, Mp, T, lvl;
        unsigned om0, om1, os, gx, gy;
    } hp;
    int lane, wave, c, h, b, m0, p0, P, Lout;
    int woff[WPW], voff[VPW];
    __amdgpu_buffer_rsrc_t rw, rv;
    wf32x16 acc[2];
    wf32x4 aop[NB], bop[NB];
    // epilogue role of this lane: channel block cb (16 rows), frame half fb (16 pairs); pair c16, 8-channel block qq, K4P row hh
    int cb, fb, c16, qq, hh;
    wf32x4 rs0, rs1, kb;      // residual entries of the lane's two frames, bias of its four channels

    __device__ __forceinline__ WinoKernel(const WinoConvArgs& p_, float* s_) : p(p_), smem(s_) {}

    typedef const __attribute__((address_space(4))) int* const_int_ptr;
    __device__ __forceinline__ int len_at(int lvl, int T) const {
        if (!p.lens) return T;
        int n = ((const_int_ptr)(unsigned long long)p.lens)[b];
        for (int i = 0; i < lvl; ++i) n = (n - 1) / 2 + 1;
        return n < T ? n : T;
    }
    __device__ __forceinline__ void setup() {
        hp.v = p.v; hp.u = p.u; hp.Ci = p.Ci; hp.Mp = p.Mp; hp.T = p.T; hp.lvl = p.lvl;
        hp.om0 = p.ord_m[0]; hp.om1 = p.ord_m[1]; hp.os = p.ord_s; hp.gx = gridDim.x; hp.gy = gridDim.y;
        asm volatile("" : "+s"(hp.v), "+s"(hp.u), "+s"(hp.Ci), "+s"(hp.Mp), "+s"(hp.T), "+s"(hp.lvl), "+s"(hp.om0), "+s"(hp.om1), "+s"(hp.os),
                          "+s"(hp.gx), "+s"(hp.gy));
        const int tid = threadIdx.x;
        lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        c = lane & 31; h = lane >> 5;
        cb = wave >> 1; fb = wave & 1; c16 = lane & 15; qq = lane >> 5; hh = (lane >> 4) & 1;
        P = (hp.T + 1) >> 1;
        // XCD-aware tile order (conv_dma.hip): the M-blocks of one (batch, pair block) take consecutive slots of one XCD
        const int nMb = (int)((unsigned)hp.Mp / BM), nN = (int)((unsigned)(P + BP - 1) / BP);
        const int gx = (int)hp.gx, total = gx * (int)hp.gy;
        const int id = blockIdx.y * gx + blockIdx.x;
        const int xcd = id & 7, slot = id >> 3, per = total >> 3, rem = total & 7;
        const unsigned L = (unsigned)(xcd * per + (xcd < rem ? xcd : rem) + slot);
        const unsigned tb = dma_magic_div(L, hp.om0, hp.os & 255);
        const int mb = (int)(L - tb * nMb);
        b = (int)dma_magic_div(tb, hp.om1, (hp.os >> 8) & 255);
        const int nb = (int)tb - b * nN;
        m0 = mb * BM; p0 = nb * BP;
        Lout = len_at(hp.lvl, hp.T);
#pragma unroll
        for (int i = 0; i < WPW; ++i) {
            const unsigned q = (unsigned)(wave + 4 * i) * 64u + (unsigned)lane;      // chunk = (tap, k-row, row)
            const unsigned tap = q / (unsigned)(KR * BM);
            const unsigned r2 = q - tap * (unsigned)(KR * BM);
            const unsigned rr = r2 / (unsigned)BM, m = r2 - rr * (unsigned)BM;
            woff[i] = (int)(((tap * ((unsigned)hp.Ci / 4u) + rr) * (unsigned)hp.Mp + (unsigned)m0 + m) * 16u);
        }
#pragma unroll
        for (int i = 0; i < VPW; ++i) {
            const unsigned q = (unsigned)(wave + 4 * i) * 64u + (unsigned)lane;      // chunk = (k-row, plane, pair)
            const unsigned rp = q / (unsigned)BP, col = q - rp * (unsigned)BP;
            voff[i] = (int)((rp * (unsigned)P + (unsigned)p0 + col) * 16u);
        }
        // (a pair column beyond P reads the next row's entries, or -- beyond the batch element's planes -- zeros by the range check: finite
        // values either way, which only reach output frames >= T that are never stored)
        rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(hp.u), 0, 4 * hp.Ci * hp.Mp * 4, 0x00020000);
        rv = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(hp.v + (long long)b * hp.Ci * P * 4), 0, hp.Ci * P * 16, 0x00020000);
    }
    __device__ __forceinline__ bool dead_tile() const { return p.lens && 2 * p0 >= Lout; }

    __device__ __forceinline__ void issue_tile(int kc, float* st) {
        const int ws = kc * (KR * 16) * hp.Mp;                   // bytes
#pragma unroll
        for (int i = 0; i < WPW; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (__attribute__((address_space(3))) void*)(st + ((wave + 4 * i) * 64) * 4), 16, woff[i], ws, 0, 0);
        const int vs = kc * (KR * 4 * 16) * P;
        float* xs = st + WFL;
#pragma unroll
        for (int i = 0; i < VPW; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, (__attribute__((address_space(3))) void*)(xs + ((wave + 4 * i) * 64) * 4), 16, voff[i], vs, 0, 0);
    }
    // group kq of a K-step: tap `wave`'s rows and plane `wave`'s pairs of k-row 2 kq + h (four consecutive MFMAs' operands each)
    template <int SLOT>
    __device__ __forceinline__ void load_ops(const float* st, int kq) {
        aop[SLOT] = *reinterpret_cast<const wf32x4*>(st + ((wave * KR + kq * 2 + h) * BM + c) * 4);
        bop[SLOT] = *reinterpret_cast<const wf32x4*>(st + WFL + (((kq * 2 + h) * 4 + wave) * BP + c) * 4);
    }
    template <int SLOT>
    __device__ __forceinline__ void mfma_ops() {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc[jj & 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(aop[SLOT][jj], bop[SLOT][jj], acc[jj & 1], 0, 0, 0);
    }
    // s_waitcnt vmcnt(y * PER_TILE + X), y in [0, Y] wave-uniform (conv_dma.hip wait_younger and its invariant: the count never exceeds the
    // vector memory operations this wave issued after the last DMA of the awaited tile)
    template <int Y, int X = 0>
    __device__ __forceinline__ void wait_younger(int y) {
        if constexpr (Y == 0) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(X > 63 ? 63 : X) : "memory");
        } else {
            constexpr int N = (Y * PER_TILE + X > 63) ? 63 : Y * PER_TILE + X;
            if (y >= Y) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
            else wait_younger<Y - 1, X>(y);
        }
    }
    __device__ __forceinline__ void tile_sync(int kc, int nk, float* cur) {
        const int younger = (nk - 2 - kc < NST - 2) ? (nk - 2 - kc) : (NST - 2);     // tiles after kc+1 still in flight
        if (kc + 1 < NST) wait_younger<NST - 2, NLATE>(younger);      // tile kc+1 belongs to the first burst: the late loads are younger too
        else wait_younger<NST - 2, 0>(younger);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (kc + NST < nk) issue_tile(kc + NST, cur);
    }
    template <int g>
    __device__ __forceinline__ void kstep(float* cur, const float* nxt, int kc, int nk) {
        if constexpr (g < G) {
            constexpr int gp = g + NB - 1;                     // group whose operands are fetched now
            if constexpr (gp < G) {
                load_ops<gp % NB>(cur, gp);
            } else {
                if (kc + 1 < nk) {
                    if constexpr (gp == G) tile_sync(kc, nk, cur);
                    load_ops<gp % NB>(nxt, gp - G);
                }
            }
            mfma_ops<g % NB>();
            __builtin_amdgcn_sched_barrier(0);     // keep the operand reads one group ahead of their MFMAs
            kstep<g + 1>(cur, nxt, kc, nk);
        }
    }

    // this lane's output block of the epilogue
    __device__ __forceinline__ int out_q() const { return (m0 >> 3) + 2 * cb + qq; }                  // 8-channel block of the output tensor
    __device__ __forceinline__ bool live() const { return m0 + 16 * cb < p.Co; }                        // (wave-uniform; Co % 16 == 0)
    __device__ __forceinline__ int pair() const { return p0 + 16 * fb + c16; }
    // The epilogue's operands through buffer loads right behind the first tiles' DMAs: EXACTLY NLATE vector memory operations, by every lane
    // and for every argument set (a launch without residual or bias, or a block beyond Co, reads a buffer of zero bytes: zeros).
    __device__ __forceinline__ void late_loads() {
        const int Tp = p.T + 2;
        const bool lv = live();
        const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.res ? p.res + (long long)b * p.Co * Tp : p.res), 0,
                                                                            (p.res && lv) ? p.Co * Tp * 4 : 0, 0x00020000);
        const int e0 = k4p_entry_off(out_q(), hh, Tp, 2 * pair() + 1);
        rs0 = __builtin_bit_cast(wf32x4, __builtin_amdgcn_raw_buffer_load_b128(rr, e0, 0, 0));
        rs1 = __builtin_bit_cast(wf32x4, __builtin_amdgcn_raw_buffer_load_b128(rr, e0 + 16, 0, 0));      // (frame T of an odd T: the pad frame, zeros)
        const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.bias), 0, p.bias ? p.Mp * 4 : 0, 0x00020000);
        const int bo = (m0 + 16 * cb + 8 * qq + hh) * 4;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) kb[jj] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb, bo + 8 * jj, 0, 0));
    }

    __device__ __forceinline__ void mainloop() {
        const int nk = (int)((unsigned)hp.Ci / BK);
        for (int t = 0; t < NST && t < nk; ++t) issue_tile(t, smem + t * STAGE);
        // nothing of late_loads() may move in front of the burst or behind the wait: both would make the count of wait_younger too large
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        late_loads();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float z;
                asm volatile("v_mov_b32 %0, 0" : "=v"(z));      // (as instructions: they stay behind the burst)
                acc[a][r] = z;
            }
        wait_younger<NST - 1, NLATE>((nk - 1 < NST - 1) ? nk - 1 : NST - 1);      // tile 0 landed (this wave's share)
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        load_ops<0>(smem, 0);
        int sc = 0;
        for (int kc = 0; kc < nk; ++kc) {
            const int sn = (sc + 1 == NST) ? 0 : sc + 1;
            kstep<0>(smem + sc * STAGE, smem + sn * STAGE, kc, nk);
            sc = sn;
        }
    }

    __device__ __forceinline__ void epilogue() {
        acc[0] += acc[1];
        __syncthreads();                                   // every wave is done reading operand tiles: the stages are free
        float* red = smem + (wave * BM + 4 * h) * RS + c;  // M_wave[row 8g + 4h + k][pair c] = register 4g + k
#pragma unroll
        for (int r = 0; r < 16; ++r) red[((r & 3) + 8 * (r >> 2)) * RS] = acc[0][r];
        __syncthreads();
        // rows 16 cb + 8 qq + 2 jj + hh (jj = 0..3: one K4P entry), pair 16 fb + c16; the four tiles combine in a fixed order
        const float* mr = smem + (16 * cb + 8 * qq + hh) * RS + 16 * fb + c16;
        wf32x4 ye, yo;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const float t0 = mr[(0 * BM + 2 * jj) * RS], t1 = mr[(1 * BM + 2 * jj) * RS], t2 = mr[(2 * BM + 2 * jj) * RS], t3 = mr[(3 * BM + 2 * jj) * RS];
            ye[jj] = __fadd_rn(__fadd_rn(t0, t1), t2);
            yo[jj] = __fsub_rn(__fsub_rn(t1, t2), t3);
        }
        ye = ye + kb + rs0;
        yo = yo + kb + rs1;
        const int Tp = p.T + 2, n0 = 2 * pair(), n1 = n0 + 1;
        const bool lv = live();
        if (p.gnpart_out) {
            // GroupNorm statistics of this wave's (16 channels x 32 frames) block, conv_dma's definition: (mean, M2) over its valid frames.
            // The whole block sits in one wave, so the sum of squares is taken about the block's own mean (two reductions in a fixed
            // order, the mean broadcast from lane 63 in between): no cancellation, whatever the block's offset.
            const int nb0 = 2 * p0 + 32 * fb;                            // first frame of this 32-frame block
            const int nv = (Lout - nb0 < 32) ? Lout - nb0 : 32;          // valid frames
            const bool v0 = n0 < Lout, v1 = n1 < Lout;
            float s1 = 0.f;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) s1 += (v0 ? ye[jj] : 0.f) + (v1 ? yo[jj] : 0.f);
            s1 = wino_wave_sum(s1);
            const float mean = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, s1), 63)) * (1.0f / (16.0f * (float)(nv > 0 ? nv : 1)));
            float s2 = 0.f;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const float d0 = v0 ? ye[jj] - mean : 0.f, d1 = v1 ? yo[jj] - mean : 0.f;
                s2 = fmaf(d0, d0, s2);
                s2 = fmaf(d1, d1, s2);
            }
            s2 = wino_wave_sum(s2);
            if (lane == 63 && nv > 0 && lv)
                p.gnpart_out[((long long)b * (p.Co >> 4) + (m0 >> 4) + cb) * ((p.T + 31) >> 5) + (nb0 >> 5)] = make_float2(mean, s2);
        }
        if (n0 >= Lout) ye = wf32x4{0.f, 0.f, 0.f, 0.f};      // ragged batch: zeros from the utterance's length on
        if (n1 >= Lout) yo = wf32x4{0.f, 0.f, 0.f, 0.f};      // (... and frame T of an odd T is the right pad frame: Lout <= T)
        if (lv && n0 < p.T) {
            const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(p.out + (long long)b * p.Co * Tp, 0, p.Co * Tp * 4, 0x00020000);
            const int e0 = k4p_entry_off(out_q(), hh, Tp, n0 + 1);
            k4p_store16_wt(ro, e0, ye);
            k4p_store16_wt(ro, e0 + 16, yo);
            if (n0 == 0) k4p_store16(ro, e0 - 16, k4p_f32x4{0.f, 0.f, 0.f, 0.f});                // left pad frame
            if (n1 == p.T - 1) k4p_store16(ro, e0 + 32, k4p_f32x4{0.f, 0.f, 0.f, 0.f});          // right pad frame of an even T
        }
    }
};

template <int BK, int NST>
__global__ void __launch_bounds__(256, (WinoCfg<BK, NST>::OCC)) conv_wino_kernel(const WinoConvArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    WinoKernel<BK, NST> k(p, smem);
    k.setup();
    // ragged batch: a tile wholly beyond its utterance's length has nothing to reduce; the epilogue writes its zeros
    if (!k.dead_tile()) {
        k.mainloop();
    } else {
        k.acc[0] = k.acc[1] = wf32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        k.rs0 = k.rs1 = k.kb = wf32x4{0.f, 0.f, 0.f, 0.f};
    }
    k.epilogue();
}

static thread_local char g_wcfg[96] = "";
const char* conv_wino_last_config() { return g_wcfg; }

template <int BK, int NST>
static hipError_t launch_wino_cfg(WinoConvArgs& a, hipStream_t s) {
    using Cfg = WinoCfg<BK, NST>;
    const int P = (a.T + 1) / 2, nMb = a.Mp / Cfg::BM, nN = (P + Cfg::BP - 1) / Cfg::BP;
    const DmaMagic m0 = dma_magic((unsigned)nMb), m1 = dma_magic((unsigned)nN);
    a.ord_m[0] = m0.m; a.ord_m[1] = m1.m; a.ord_s = m0.s | (m1.s << 8);
    const dim3 grid(nMb * nN, a.B);
    auto kern = conv_wino_kernel<BK, NST>;
    if (Cfg::LDS_BYTES > 48 * 1024) {
        static std::atomic<unsigned long long> attr_done{0};
        hipError_t e = ensure_max_dynamic_lds(reinterpret_cast<const void*>(kern), attr_done);
        if (e != hipSuccess) return e;
    }
    snprintf(g_wcfg, sizeof(g_wcfg), "BM32 BP32 BK%d NST%d grid %ux%u lds %zu", BK, NST, grid.x, grid.y, Cfg::LDS_BYTES);
    hipEvent_t e0, e1;
    if (prof_attach_events(&e0, &e1)) hipExtLaunchKernelGGL(kern, grid, dim3(256), Cfg::LDS_BYTES, s, e0, e1, 0, a);
    else hipLaunchKernelGGL(kern, grid, dim3(256), Cfg::LDS_BYTES, s, a);
    return hipGetLastError();
}

hipError_t launch_conv_wino(const WinoConvArgs& a_, int cfg, hipStream_t s) {
    WinoConvArgs a = a_;
    if (a.B <= 0 || a.T <= 0 || a.Ci <= 0 || a.Mp % 32 || a.Co % 16 || a.Co > a.Mp || !a.v || !a.u || !a.out) return hipErrorInvalidValue;
    // 32-bit byte offsets inside one batch element's planes / the packed taps / one batch element's output
    if ((long long)a.Ci * ((a.T + 1) / 2) * 16 >= (1ll << 31) || 16ll * a.Ci * a.Mp >= (1ll << 31) || 4ll * a.Co * (a.T + 2) >= (1ll << 31)) return hipErrorInvalidValue;
    if (cfg == 0) {
        // The ring by the grid at the NOMINAL batch of 16, never the actual one (an utterance's sums keep their order for any batch split:
        // conv_dma.hip dma_pick).  BK 32 x 2 stages takes 64 KB: two workgroups per CU.  A grid of more than two per CU (the T / 1 and T / 2
        // levels) runs BK 16 x 2 stages, 32 KB, four per CU: measured 3-16 us per launch faster there and 0-4 us slower below
        // (tools/bench_wino.py).
        const long long nominal = 16ll * (a.Mp / 32) * (((a.T + 1) / 2 + 31) / 32);
        cfg = (nominal > 512 && a.Ci % 16 == 0) ? 162 : 322;
        if (a.Ci % 32) cfg = 162;
    }
    if (a.Ci % (cfg / 10)) return hipErrorInvalidValue;
    switch (cfg) {
        case 322: return launch_wino_cfg<32, 2>(a, s);
        case 162: return launch_wino_cfg<16, 2>(a, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace lds
