// Internal kernel interfaces of liblds (gfx950 only).  Activations: fp32 [B,C,T], T contiguous.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <string>

namespace lds {

// ---------------------------------------------------------------------------------------------
// conv_gemm (vocoder / front end): out[b,co,t] = epi( bias[co] + sum_{tap,ci} Wp[tap][ci][co] * f(X[b,ci, t + tap*dil - pad]) )
// f = optional LeakyReLU applied while staging; out-of-range taps read exact zeros.
// The MFMA is v_mfma_f32_32x32x2_f32 (exact fp32); A = packed weights (M = co), B = activations (N = t).
// ---------------------------------------------------------------------------------------------
enum { ACT_NONE = 0, ACT_LRELU = 2 };      // activation applied to the input while staging (conv_gemm)
enum { EPI_NONE = 0, EPI_GEGLU = 1, EPI_TANH = 2, EPI_GELU = 3, EPI_SWISH = 4, EPI_GLU = 5 };      // EPI_GELU (conv_dma): exact-form GELU of the biased / normalised value, before the residual
// EPI_SWISH (conv_dma): v * sigmoid(v) in EPI_GELU's place; EPI_GLU (conv_dma): value * sigmoid(gate) over weights packed as for EPI_GEGLU (pack_geglu)

struct ConvArgs {
    // input: virtual channel-concat of two sources (x2 for ci >= C1)
    const float* x1; const float* x2;
    int C1, C2;
    int Tsrc;            // stored row length of the sources
    int Tin;             // logical input length (2*Tsrc when ups)
    long long xb1, xb2;  // batch strides (elements)
    // packed weights [KT][Ci][Mp]
    const float* w;
    int Mp, Co, Ci, KT, stride, dil, pad, ups;
    int act_in; float slope;
    // epilogue
    const float* bias;       // [Mp] packed-row bias or null
    const float* bias_bc;    // [B][Co] extra per-(batch,channel) bias or null
    const float* res;        // [B][Cout][To] residual or null
    int epi;
    int accum;               // 1: out = (out + y) / out_div  (MRF running sum), 0: out = y / out_div
    float out_div;           // 1.0 normally
    float* out;
    int Cout;                // channels of `out` (Co, or Co/phases for transposed conv)
    int To;                  // columns computed (N)
    // transposed-conv scatter: row m = co*phases + phi -> out[b][co][n*phases + phi - tpad] (phases=1: plain)
    int phases, tpad, Tout;  // Tout = row length of out
    int B;
    // Ragged batches (vocoder): valid frames per batch element of the OUTPUT tensor (device int32 [B]; output frames at and beyond are
    // written as zeros) and of the INPUT (frames at and beyond read as zeros); null = the buffers' lengths
    const int* vlen; const int* vlen_in;
};

// tile: 0 = auto, else BM*1000+BN in {128128, 64064, 128064, 64128, 32128}
hipError_t launch_conv_gemm(const ConvArgs& a, int tile, hipStream_t s);
const char* conv_gemm_last_config();

// conv_small (conv_small.hip): the vocoder's 16- / 32-channel resblock convolutions on v_mfma_f32_16x16x4_f32, weights resident in
// registers, plain tensors.  Same ConvArgs semantics (LeakyReLU on the input, bias, residual, running sum, division).
bool conv_small_applies(const ConvArgs& a);
hipError_t launch_conv_small(const ConvArgs& a, hipStream_t s);
bool conv_mono_applies(const ConvArgs& a);      // one output channel, k 7: the generator's conv_post as a stream
hipError_t launch_conv_mono(const ConvArgs& a, hipStream_t s);
const char* conv_small_last_config();

// conv_down (conv_down.hip): the VAE encoder's convolutions over plain tensors, x [B][Ci][L] -> out [B][Co][To] with
// out[b,co,t] = bias[co] + sum_{ci,k} w[co][ci][k] * lrelu_slope(x[b,ci, t*stride - pad + k]) (taps outside [0, L) read zeros;
// slope 1 = no activation); w is the unpacked device weight [Co][Ci][K].  v_mfma_f32_32x32x2_f32, exact fp32.
// Ragged batch: vlen_in / vlen (device int32 [B], null = L / To) are each batch element's valid input / output frames; the input reads
// as zeros from vlen_in[b] on (whatever x holds there) and the output is stored as zeros from vlen[b] on.
struct ConvDownArgs {
    const float* x; const float* w; const float* bias; float* out;
    int Ci, Co, K, stride, pad, L, To, B;
    float slope;
    int tile;      // 0 = auto (by workgroup count against the CU count), else BM*1000+BN in {64064, 64128, 128128}
    const int* vlen_in; const int* vlen;
};
hipError_t launch_conv_down(const ConvDownArgs& a, hipStream_t s);
const char* conv_down_last_config();
// y [B][2C][T] (conv_post) -> out [B][T][2C] = (m, only_mean ? 0 : logs); z [B][T][C] = m + noise * exp(logs) when z (needs noise [B][C][T]);
// tlen (device int32 [B], null = T): rows t >= tlen[b] of out and z are zeros and noise is not read there
hipError_t launch_vae_head(const float* y, const float* noise, float* out, float* z, int B, int C, int T, int only_mean, hipStream_t s,
                           const int* tlen = nullptr);

// voc_pair (voc_pair.hip): one residual step of the vocoder's ResBlock1 at 16 / 32 channels as one launch over plain [B][C][T] tensors:
// out = (accum ? out : 0) + c2(lrelu(c1(lrelu(x)))) + x, divided by out_div; c1 dilated by `dil`, both k = KT, "same" zero padding;
// frames at and beyond vlen[b] (device int32 [B], null = T) are outside the utterance: x and the intermediate read as zero there (whatever
// x holds) and the output is written as zeros.  x and out must not alias (neighbouring tiles read x's halo).
struct VocPairArgs {
    const float* x; float* out;
    const float* w1; const float* b1; int Mp1;      // packed weights [KT][C/8][2][Mp][4] and packed-row biases (model.hip pack_conv)
    const float* w2; const float* b2; int Mp2;
    int C, KT, dil, B, T;
    int accum; float out_div; float slope;
    const int* vlen;
};
bool voc_pair_applies(int C, int KT, int dil);
hipError_t launch_voc_pair(const VocPairArgs& a, hipStream_t s);
const char* voc_pair_last_config();

// Weight packers (host side): reference layout -> [KT][Ci][Mp]
size_t packed_conv_elems(int Co, int Ci, int K, int* Mp_out);

// ---------------------------------------------------------------------------------------------
// conv_dma: the UNet's VALU-free GEMM over K4P activations (k4p.h, conv_dma.hip)
// ---------------------------------------------------------------------------------------------
struct DmaConvArgs {
    const float* x1; const float* x2;   // K4P sources [B][C1][Tsrc], [B][C2][Tsrc] (virtual channel concat)
    int C1, C2, Tsrc;
    const float* w;                     // packed weights [KT][Ci/8][2][Mp][4]
    const float* bias;                  // packed-row bias [Mp] or null
    int Mp, Co, Ci, KT, stride, pad, ups;
    const float* res;                   // K4P residual [B][Cout(K4P part)][To] or null
    int epi;                            // EPI_NONE | EPI_GEGLU | EPI_GELU | EPI_SWISH | EPI_GLU
    float* out;                         // K4P [B][min(Cout, plain_from)][To], or plain [B][Cout][To] when out_plain
    int out_plain;
    int plain_from; float* out2;        // output channels >= plain_from go frame-major to out2 [B][Cout-plain_from][To] ...
    int vt_D;                           // ... or, when vt_D > 0, in attention's VT layout [B][(Cout-plain_from)/vt_D][ceil(To/4)][vt_D][4]
    float2* lnpart_out;                 // optional [B][C/32][To] per-frame (mean, M2) partials over 32-channel tiles
    float2* gnpart_out;                 // optional [B][C/16][ceil(To/32)] (mean, M2) of every (16 channels x 32 frames) block of the K4P output (GroupNorm statistics for gn_stream)
    // LayerNorm of the INPUT folded into the epilogue (weights pre-multiplied by gamma on the host):
    //   y[m,t] = rstd_t * (acc[m,t] - mean_t * ln_c1[m]) + ln_c2[m],  c1 = sum_c W[m,c]*gamma_c,  c2 = sum_c W[m,c]*beta_c + bias[m]
    // mean_t / rstd_t are combined per column from the producer's partials ln_part [B][ln_np][Tsrc]
    const float2* ln_part; int ln_np; float ln_eps; const float* ln_c1; const float* ln_c2;
    // GroupNorm of the INPUT (affine, no activation: the transformer's `norm` in front of proj_in, reference transformer_1d.py:256-266)
    // folded into a 1x1 convolution over ONE source (weights pre-multiplied by gamma on the host):
    //   y[m,t] = sum_g rstd_g * (sum_{c in g} Wg[m,c] x[c,t]) - sum_g rstd_g mean_g gnf_cg[g][m] + gnf_c2[m]
    //   gnf_cg[g][m] = sum_{c in g} W[m,c] gamma_c,  gnf_c2[m] = sum_c W[m,c] beta_c + bias[m]
    // The channels of a group are contiguous and every wave's share of a K-step lies inside one group: its activation operands are
    // multiplied by that group's rstd on their way from LDS to the MFMA (two packed multiplies per four MFMAs); the per-(batch, group)
    // statistics are combined from the producer's partials gnf_part [B][Ci/16][ceil(Tsrc/32)] (the same ones gn_stream reads) at kernel start.
    const float2* gnf_part; int gnf_groups; float gnf_eps; const float* gnf_cg; const float* gnf_c2;
    int Cout, To, B;
    // vocoder extensions (HiFi-VAEGAN MRF, reference models.py:161-262); the UNet leaves them at dil 1, xpad = opad = 1, rest 0 / 1.0
    int voc;                            // 1: vocoder kernel family (the fields below are honoured)
    int dil;                            // tap spacing in frames (1, 3, 5)
    int xpad, opad;                     // zero frames on each side of every K4P row of the inputs / of out, res, acc_in, out_act (>= pad)
    float act_slope;                    // != 0: LeakyReLU(slope) of the final value is what the next convolution reads ...
    float* out_act;                     // ... written here while `out` keeps the raw value (null: `out` receives the activated value)
    const float* acc_in;                // K4P running sum added before the division: out = (acc_in + y) / out_div
    float out_div;
    // polyphase ConvTranspose (vocoder upsamplers; weights packed by pack_convT: row m = co * phases + phase, KT = K / stride taps):
    // column n of row m is output frame n * phases + phase - ph_tpad of channel co, stored to K4P tensors with ph_Tout frames
    int ph_log2, ph_tpad, ph_Tout, ph_Cout;      // ph_Tout > 0 selects the mode; phases = 1 << ph_log2; ph_Cout = Co / phases
    // conv_bf3 only (split-bf16 path, k8b3.h): x1 / x2 / res / out are K8B3 tensors; out_f32 = 1 keeps the K4P-range output channels
    // in fp32 K4P instead (q / k rows for the attention kernel)
    int out_f32;
    float acc_scale;                    // != 0: the accumulators are multiplied by it first (fp16-plane weights are stored times a power of two)
    // Batch size the tile / split choice is judged at.  0 = the nominal per-GPU batch (16): the choice then never depends on the actual
    // batch and an utterance's result is bit-identical for any batch split.  > 0 (lds_unet_set_latency_mode): the actual batch, so that
    // one or two utterances spread over the chip -- same tolerances against the oracle, not bit-identical with batched results.
    int tile_batch;
    // Ragged batches (k4p.h ragged_len): per-utterance lengths at the UNet's input resolution and the levels of this launch's input and
    // output tensors; output frames at and beyond an utterance's length are written as zeros.  nullptr: no masking.
    const int* lens; int lvl_in, lvl_out;
    // ... and of the vocoder's stages, whose lengths multiply instead of halving: valid OUTPUT frames per batch element (device int32 [B];
    // of the scattered tensor in polyphase mode), written as zeros beyond; null = none
    const int* vlen;
    // Cluster split-K (latency mode only; conv_dma.hip cluster_join): ksplit = S > 1 workgroups share an output tile, each reducing 1/S
    // of the K-steps; kpart = scratch for the partial tiles (tiles x 4 waves x S x 1024 floats), kcount = one zeroed counter per tile,
    // left zeroed.  The launchers choose S (conv_dma_cluster_split) when tile_batch > 0 and kpart / kcount are given.
    int ksplit;
    float* kpart; unsigned* kcount;
    long long kpart_cap; int kcount_cap;      // capacities (floats / counters)
    // conv_dma only, filled by its launchers (dma_set_order): the three divisors of the block-index decomposition (M-blocks, frame blocks,
    // cluster shares) as multiplier / shift pairs, so that the kernel finds its tile on the scalar unit alone (dma_magic below)
    unsigned ord_m[3], ord_s;                 // ord_s = the three shifts, 8 bits each
};
// n / d for 0 <= n < 2^31, 1 <= d < 2^31 as (mulhi(2 n, m) >> s):  s = ceil(log2 d), m = floor(2^(31 + s) / d) + 1 < 2^32, and
// m d - 2^(31 + s) is in (0, d] <= 2^s, which makes the quotient exact over the whole range (Granlund & Montgomery 1994, theorem 4.2)
struct DmaMagic { unsigned m, s; };
inline DmaMagic dma_magic(unsigned d) {
    unsigned s = 0;
    while ((1ull << s) < d) ++s;
    return DmaMagic{(unsigned)((1ull << (31 + s)) / d + 1), s};
}
__host__ __device__ inline unsigned dma_magic_div(unsigned n, unsigned m, unsigned s) {
    return (unsigned)(((unsigned long long)(n << 1) * m) >> 32) >> s;
}
// The tile of workgroup `id` of a grid of `total` = nMb * nN * B * S workgroups (conv_dma.hip, XCD-aware order): the same arithmetic on
// the host, for the tests (lds_test_dma_tile_order)
struct DmaTile { int mb, nb, b, ksp; };
inline DmaTile dma_tile_of(int id, int total, int nMb, int nN, int S, const unsigned* ord_m, unsigned ord_s) {
    const int xcd = id & 7, slot = id >> 3, per = total >> 3, rem = total & 7;
    const unsigned L = (unsigned)(xcd * per + (xcd < rem ? xcd : rem) + slot);
    const unsigned tb = dma_magic_div(L, ord_m[0], ord_s & 255);
    const unsigned by = dma_magic_div(tb, ord_m[1], (ord_s >> 8) & 255);
    const unsigned b = dma_magic_div(by, ord_m[2], (ord_s >> 16) & 255);
    return DmaTile{(int)(L - tb * nMb), (int)(tb - by * nN), (int)b, (int)(by - b * S)};
}
// cfg: 0 = auto, else BM*1000000 + BN*1000 + BK*10 + NST
hipError_t launch_conv_dma(const DmaConvArgs& a, int cfg, hipStream_t s);
// Resnet tail in one launch (reference resnet.py:636-641): out = conv2_k3(h) + shortcut_1x1([x ; skip]) + bias.  `a3` carries the k 3
// convolution's sources / weights (its epilogue fields are ignored), `a1` the 1x1 shortcut's sources / weights AND the epilogue
// (bias = the two biases added on the host, GroupNorm partials, output).  Both reductions run into the same accumulators: one
// launch and one K4P round trip less per resnet that changes its width.  hipErrorNotSupported: no fused variant for these shapes
// (the caller launches the two convolutions separately).
hipError_t launch_conv_dma_pair(const DmaConvArgs& a3, const DmaConvArgs& a1, hipStream_t s);
bool conv_dma_pair_applies(const DmaConvArgs& a3, const DmaConvArgs& a1);
const char* conv_dma_last_config();

// ---------------------------------------------------------------------------------------------
// conv_wino: the resnets' k 3 / stride 1 / pad 1 convolution in the 1-D Winograd form F(2,3) (conv_wino.hip): two output frames from
// four products instead of six.  The input is not a K4P tensor but the four planes V0..V3 that launch_gn_wino writes over P = ceil(T / 2)
// frame pairs, [B][Ci/8][2][4][P][4] (row (q, h) of K4P, then plane, then pair; no pad entries); the weights are the four taps U0..U3 in
// conv_dma's packed layout [4][Ci/8][2][Mp][4].  Output: K4P (pads written), + bias, + residual, GroupNorm partials as DmaConvArgs.
// ---------------------------------------------------------------------------------------------
struct WinoConvArgs {
    const float* v; const float* u;
    const float* bias;            // [Mp] or null
    const float* res;             // K4P [B][Co][T] or null
    float* out;                   // K4P [B][Co][T]
    float2* gnpart_out;           // [B][Co/16][ceil(T/32)] (mean, M2) or null
    const int* lens; int lvl;     // ragged batches (k4p.h ragged_len): this tensor's level; null = every utterance has T frames
    int B, Ci, Mp, Co, T;
    unsigned ord_m[2], ord_s;     // filled by the launcher: the divisors (M-blocks, pair blocks) of the block-index decomposition (dma_magic)
};
// cfg = BK * 10 + NST in {322, 162} (0 = by the grid at the nominal batch); Ci % BK == 0, Mp % 32 == 0, Co % 16 == 0
hipError_t launch_conv_wino(const WinoConvArgs& a, int cfg, hipStream_t s);
const char* conv_wino_last_config();
// launch_gn_stream's pass with the Winograd input transform behind it: d = act(GroupNorm(...)) exactly as launch_gn_stream computes it (frames
// outside [0, ragged length) are zero), then V0 = d[2i] - d[2i+2], V1 = d[2i+1] + d[2i+2], V2 = d[2i+2] - d[2i+1], V3 = d[2i+1] - d[2i+3]
// into the planes of WinoConvArgs::v (y: B * (C1 + C2) * 4 * ceil(T / 2) floats)
hipError_t launch_gn_wino(const float* x1, const float* x2, int C1, int C2, int T, int groups, float eps, const float* gamma, const float* beta,
                          const float* scale_shift, int ss_stride, int ss_off, int silu, const float2* gp1, const float2* gp2, float* y, int B,
                          hipStream_t s, const int* lens = nullptr, int lvl = 0);
// The two passes in front of a resnet's conv2 + shortcut launch in the Winograd form (model.hip run_wconv_pair).  That launch reduces over
// Cm + Cin / 2 channels: conv2's planes in the first Cm / 8 blocks of a plane tensor [B][(Cm + Cin/2)/8][2][4][P][4], the shortcut's operand
// planes in the last Cin / 16 blocks -- for the first half A of the raw block input's 8-channel blocks plane 0 = x_e, plane 3 = x_o (x_e[i] =
// x[2i], x_o[i] = x[2i+1], zero from the utterance's length on), for the second half B plane 1 = x_e + x_o, plane 2 = x_e - x_o.
//   side == null (profiler name gn_wpair): launch_gn_wino's pass with the batch stride `y_bstride` (floats) on the output: conv2's planes.
//   side != null (gn_wino): launch_gn_wino's pass, y as there with y_bstride = (C1 + C2) * 4 * P, and the shortcut's planes beside it: block q
//   of [x1 ; x2] writes two planes of side block q mod (C / 16), `side` = the first side block of batch element 0, side_bstride in floats.
hipError_t launch_gn_wino_pair(const float* x1, const float* x2, int C1, int C2, int T, int groups, float eps, const float* gamma, const float* beta,
                               const float* scale_shift, int ss_stride, int ss_off, int silu, const float2* gp1, const float2* gp2, float* y,
                               long long y_bstride, float* side, long long side_bstride, int B, hipStream_t s, const int* lens = nullptr, int lvl = 0);

// ---------------------------------------------------------------------------------------------
// conv_bf3: the same operator on the bf16 matrix pipe with fp32-equivalent split operands (conv_bf3.hip, k8b3.h).  Same argument
// struct; activations (x1, x2, res, out) are K8B3 tensors, weights packed [KT][Ci/8][3][Mp][8] bf16 (pack_conv_bf3, model.hip).
// nprod: bf16 products per fp32 product (6 = product path; 3 / 9 exist for tools/split_bf16_probe.py's error study only).
// ---------------------------------------------------------------------------------------------
// fmt: FMT_BF16X3 (three bf16 planes, 6 products) or FMT_F16X2 (two fp16 planes, 3 products; k8b3.h); nprod 0 = the format's default
hipError_t launch_conv_bf3(const DmaConvArgs& a, int cfg, int nprod, int fmt, hipStream_t s);
hipError_t launch_conv_bf3_pair(const DmaConvArgs& a3, const DmaConvArgs& a1, int fmt, hipStream_t s);
bool conv_bf3_pair_applies(const DmaConvArgs& a3, const DmaConvArgs& a1);
const char* conv_bf3_last_config();
void conv_bf3_set_debug_rule(int r);      // tuning only (lds_debug_set_split_rule)
// split-plane helpers (k8b3_ops.hip): plain [B][C][T] <-> K8B3 / K8H2 (channels [c_off, c_off + C) of a tensor with Ctot channels); fmt as above
hipError_t launch_to_k8b3(const float* in, void* out, int B, int C, int T, int Ctot, int c_off, hipStream_t s, int fmt = 0, const int* lens = nullptr);
hipError_t launch_from_k8b3(const void* in, float* out, int B, int C, int T, hipStream_t s, int fmt = 0);
// GroupNorm(+scale/shift)(+SiLU) of the virtual concat [x1;x2], split planes in and out; same statistics path as launch_gn_stream
hipError_t launch_gn_stream_bf3(const void* x1, const void* x2, int C1, int C2, int T, int groups, float eps, const float* gamma,
                                const float* beta, const float* scale_shift, int ss_stride, int ss_off, int silu, const float2* gp1,
                                const float2* gp2, void* y, int B, hipStream_t s, int fmt = 0, const int* lens = nullptr, int lvl = 0);
hipError_t launch_gn_partials_bf3(const void* x, int C, int T, float2* gp, int B, hipStream_t s, int fmt = 0);
hipError_t launch_resample_k8b3(const void* in, void* out, int B, int C, int Tin, int Tout, hipStream_t s, int fmt = 0, const int* lens = nullptr, int lvl_in = 0, int lvl_out = 0);

// ---------------------------------------------------------------------------------------------
// K4P helpers (k4p_ops.hip)
// ---------------------------------------------------------------------------------------------
// plain [B][C][T] -> channels [c_off, c_off+C) of a K4P tensor with Ctot channels (pads of those rows zeroed)
hipError_t launch_to_k4p(const float* in, float* out, int B, int C, int T, int Ctot, int c_off, hipStream_t s, const int* lens = nullptr);
hipError_t launch_from_k4p(const float* in, float* out, int B, int C, int T, hipStream_t s);
hipError_t launch_from_k4p_pad(const float* in, float* out, int B, int C, int T, int pad, hipStream_t s);
// plain [B][C][T] -> attention's VT layout [B][C/D][ceil(T/4)][D][4] (tail keys zeroed); the UNet gets this layout straight
// from the QKV convolution's epilogue, this kernel serves the stand-alone attention entry point
hipError_t launch_plain_to_vt(const float* in, float* out, int B, int C, int T, int D, hipStream_t s);
// GroupNorm of the virtual concat [x1;x2] (K4P) -> y (K4P, C1+C2 channels):
//   y = act(((x - mean_g) * rstd_g * gamma + beta) * (1 + scale) + shift), act = SiLU if silu
// One streaming pass (1 read + 1 write, one workgroup per (batch, 8-channel block)): the group statistics come from
// the per-(16 channels x 32 frames) (mean, M2) partials gp1 / gp2 [B][C/16][ceil(T/32)] that the producers of x1 / x2
// wrote in their epilogues (DmaConvArgs::gnpart_out) and are combined per workgroup with Chan's formula in a fixed order
// while the tensor loads are in flight.
hipError_t launch_gn_stream(const float* x1, const float* x2, int C1, int C2, int T, int groups, float eps,
                            const float* gamma, const float* beta, const float* scale_shift, int ss_stride, int ss_off,
                            int silu, const float2* gp1, const float2* gp2, float* y, int B, hipStream_t s, const int* lens = nullptr, int lvl = 0);
// the same partials computed from a K4P tensor by a stand-alone pass (tensors not produced by conv_dma; test entry points)
// (lens: the ragged batch's per-utterance lengths, k4p.h ragged_len at level lvl -- the statistics stop there, and blocks wholly beyond get no partial)
hipError_t launch_gn_partials(const float* x, int C, int T, float2* gp, int B, hipStream_t s, const int* lens = nullptr, int lvl = 0);
// test support: NaN / Inf into the pad frames and the frames at and beyond each utterance's length (level 0) of a K4P tensor
hipError_t launch_k4p_poison(float* x, int B, int C, int T, const int* lens, hipStream_t s);
// nearest-neighbour resample along frames (K4P -> K4P), reference F.interpolate(size=Tout)
// plain [B][C][T] -> K4P with `pad` zero frames per side: raw copy and (slope != 0) LeakyReLU copy (either output may be null)
hipError_t launch_to_k4p_act(const float* in, float* raw, float* act, float slope, int B, int C, int T, int pad, hipStream_t s, const int* vlen = nullptr);
// zero the `pad` frames on both sides of every row of a K4P tensor (tensors whose writers only store real frames)
hipError_t launch_k4p_zero_pads(float* x, int B, int C, int T, int pad, hipStream_t s);
// lens: per-utterance lengths (ragged_len) at levels lvl_in / lvl_out of the two tensors
hipError_t launch_resample_k4p(const float* in, float* out, int B, int C, int Tin, int Tout, hipStream_t s, const int* lens = nullptr, int lvl_in = 0, int lvl_out = 0);
// self-attention: q,k in K4P (tensor qk [B][2C][T]: q channels 0..C-1, k channels C..2C-1), v in the VT layout
// [B][heads][ceil(T/4)][D][4] (key tail zeroed); out K4P [B][C][T]
// tile_batch: as DmaConvArgs::tile_batch (0 = nominal batch of 16)
hipError_t launch_attention_k4p(const float* qk, const float* vt, float* out, int B, int C, int T, int heads, hipStream_t s, int tile_batch = 0,
                                const int* lens = nullptr, int lvl = 0);
// the same with the output written as a K8B3 tensor (split-bf16 path: the output feeds the to_out projection)
hipError_t launch_attention_k4p_f16math(const float* qk, const float* vt, float* out, int B, int C, int T, int heads, hipStream_t s, int tile_batch = 0, const int* lens = nullptr);
hipError_t launch_attention_k4p_out_bf3(const float* qk, const float* vt, void* out, int B, int C, int T, int heads, hipStream_t s, int fmt = 0, int tile_batch = 0,
                                        const int* lens = nullptr, int lvl = 0);

// ---------------------------------------------------------------------------------------------
// Whisper units encoder: front and back end (logmel.hip)
// ---------------------------------------------------------------------------------------------
// audio [B][L] -> Whisper's log-mel spectrogram of every clip taken alone (reference encoder/whisper/audio.py:62-82), F_b = slen[b] / 160
// frames of Fmax = L / 160.  slen: device int32 [B] sample counts (null = L), 400 <= slen[b] <= L; nothing at or beyond slen[b] is read.
// basis: double [400][201][2] windowed (cos, sin); filtT [201][n_mels]; scratch logspec [B][n_mels][Fmax], pmax [B][ceil(Fmax / 16)].
// out: K4P [B][n_mels][Fmax] (out_k4p; pads and frames beyond F_b zero) or plain [B][n_mels][Fmax] (zeros beyond F_b).
hipError_t launch_logmel(const float* audio, const int* slen, long long L, int Fmax, const double* basis, const float* filtT, int n_mels,
                         float* logspec, float* pmax, float* out, int out_k4p, int B, hipStream_t s);
// x (K4P [B][C][T]) += posk (the positional table as one K4P element of n_ctx frames) on frames below ragged_len(lens, b, 1, T);
// lnpart [B][C/32][T] = the LayerNorm partials of the sum (DmaConvArgs::lnpart_out's format)
hipError_t launch_whisper_pos(float* x, const float* posk, int n_ctx, float2* lnpart, const int* lens, int B, int C, int T, hipStream_t s);
// out [B][T][C] frame-major = LayerNorm(x) from the partials lnpart; rows at and beyond ragged_len(lens, b, lvl, T) are zeros (lvl 1: Whisper,
// whose lens count mel frames; lvl 0: lens are the clips' own frame counts)
hipError_t launch_whisper_ln_post(const float* x, const float2* lnpart, const float* gamma, const float* beta, float eps, float* out, const int* lens,
                                  int B, int C, int T, hipStream_t s, int lvl = 1);

// ---------------------------------------------------------------------------------------------
// HuBERT units encoder: the kernels of its own (hubert.hip); nlen / slen are device int32 [B] or null (= the buffer's length)
// ---------------------------------------------------------------------------------------------
// audio [B][L] -> out K4P [B][C][N0] = GELU(GroupNorm(C, C)(conv0(clip padded by `pad` zeros per side))), N0 = (L + 2 pad - 10) / 5 + 1;
// clip b = audio[b, :slen[b]] with its own nlen[b] frames and its own statistics; w0 [C][10]; scratch part [B][ceil(N0 / 256)][C], stat [B][C]
hipError_t launch_hubert_conv0(const float* audio, const int* slen, long long L, int pad, const float* w0, const float* gamma, const float* beta, float eps,
                               const int* nlen, int N0, int C, float2* part, float2* stat, float* out, int B, hipStream_t s);
// out (K4P) = x + GELU(grouped conv of x, k = K taps, padding K / 2, last frame dropped); wp packed [group][k][ci / 4][row tile][64]
hipError_t launch_hubert_posconv(const float* x, const float* wp, const float* bias, float* out, const int* nlen, int B, int C, int T, int K, int groups,
                                 hipStream_t s);
// out (K4P) = LayerNorm over the channels of x (K4P), zeros beyond a clip's frames
hipError_t launch_hubert_ln(const float* x, const float* gamma, const float* beta, float eps, float* out, const int* nlen, int B, int C, int T, hipStream_t s);
// x (K4P [B][C][T]) -> out [B][T][C] frame-major, zero rows beyond a clip's frames
hipError_t launch_hubert_store_frames(const float* x, float* out, const int* nlen, int B, int C, int T, hipStream_t s);
// out = (first ? 0 : out) + w * x in the same layout: one term of a weighted sum of hidden states
hipError_t launch_hubert_store_frames_acc(const float* x, float* out, const int* nlen, float w, int first, int B, int C, int T, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// wav2vec 2.0 (XLSR-53) units encoder: the kernels of its own (w2v.hip); nlen / slen are device int32 [B] or null (= the buffer's length)
// ---------------------------------------------------------------------------------------------
// audio [B][L] -> out K4P [B][C][N0] = GELU(LayerNorm over the C channels of each frame(bias + conv0(clip))), N0 = (L - 10) / 5 + 1;
// clip b = audio[b, :slen[b]] with its own nlen[b] frames; w0 [C][10]; C a multiple of 64, at most 1024
hipError_t launch_w2v_conv0(const float* audio, const int* slen, long long L, const float* w0, const float* bias, const float* gamma, const float* beta,
                            float eps, const int* nlen, int N0, int C, float* out, int B, hipStream_t s);
// out (K4P, not x) = GELU(LayerNorm over the channels of x (K4P)), zeros beyond a clip's frames; part (or null) [B][C / 32][T] = the
// (mean, M2) partials of out in DmaConvArgs::lnpart_out's format
hipError_t launch_w2v_ln_act(const float* x, const float* gamma, const float* beta, float eps, float* out, float2* part, const int* nlen, int B, int C, int T,
                             hipStream_t s);
// part [B][C / 32][T] = the (mean, M2) partials of x (K4P) in DmaConvArgs::lnpart_out's format
hipError_t launch_w2v_lnpart(const float* x, float2* part, const int* nlen, int B, int C, int T, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// w2v-BERT 2.0 units encoder: the kernels of its own (w2vbert.hip, attention_k4p.hip); slen / nlen / vlen / qlens / klens are device int32 [B]
// or null (= the buffer's length)
// ---------------------------------------------------------------------------------------------
constexpr int kW2vbertRelStride = 80;      // floats per query row of the relative-key table (left_max + right_max + 1 <= 80)
// audio [B][L] -> out [B][Rmax][n_mels * stride] = SeamlessM4TFeatureExtractor's input_features of every clip taken alone: N_b = 1 + (slen[b] - 400) / 160
// frames of Nmax (the same of L), log Kaldi mel powers normalised per bin over the clip's own frames, `stride` frames per row; zeros beyond a clip's
// frames / rows.  basis: double [400][257][2] (model.hip w2vbert_basis); filtT [257][n_mels]; scratch logspec [B][n_mels][Nmax], stat [B][n_mels] (double pairs)
hipError_t launch_w2vbert_fbank(const float* audio, const int* slen, long long L, int Nmax, int Rmax, const double* basis, const float* filtT, int n_mels,
                                int stride, float mel_floor, float* logspec, double2* stat, float* out, int B, hipStream_t s);
// feats [B][T][C] frame-major -> out K4P [B][C][T], part [B][C / 32][T] = its (mean, M2) partials (DmaConvArgs::ln_part's format); rows at and
// beyond vlen[b] are not read: zeros
hipError_t launch_w2vbert_feats_k4p(const float* feats, float* out, float2* part, const int* vlen, int B, int C, int T, hipStream_t s);
// relp [B][heads][T][kW2vbertRelStride]: entry r < NR = log2(e) / 8 * q_t . E[r] (q = the first C channels of the K4P tensor qk [B][2C][T], heads of 64;
// E [NR][64]); zeros for queries at and beyond qlen[b]
hipError_t launch_w2vbert_relpos(const float* qk, const float* E, float* relp, const int* qlen, int B, int C, int T, int heads, int NR, hipStream_t s);
// launch_attention_k4p at heads of 64 with score(i, j) += relp[i][clamp(j - i, -left, right) + left]; queries = the clip's qlens[b] rows (zeros beyond),
// keys = its first klens[b] <= qlens[b] rows
hipError_t launch_attention_k4p_rel(const float* qk, const float* vt, const float* relp, float* out, int B, int C, int T, int heads, const int* qlens,
                                    const int* klens, int left, int right, hipStream_t s);
// out (K4P, not x) = swish(LayerNorm over the channels(causal depthwise conv of x (K4P), K <= 32 taps packed wp [C / 4][K][4])); input frames at
// and beyond vlen[b] read as zeros, output frames at and beyond nlen[b] are zeros
hipError_t launch_w2vbert_dwconv(const float* x, const float* wp, const float* gamma, const float* beta, float eps, float* out, const int* vlen,
                                 const int* nlen, int B, int C, int T, int K, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// WavLM units encoder: the kernels of its own (wavlm.hip, attention_k4p.hip); slen / nlen / lens are device int32 [B] or null (= the
// buffer's length)
// ---------------------------------------------------------------------------------------------
// gate [B][heads][T] = a (b cst[head] - 1) + 2 with (a, b) = the sigmoids of the two sums of four of w [8][64] x + bias [8] over the 64
// channels of the head at frame t of x (K4P [B][C][T]); 0 at and beyond nlen[b] (nothing is read there)
hipError_t launch_wavlm_gate(const float* x, const float* w, const float* bias, const float* cst, float* gate, const int* nlen, int B, int C, int T, int heads,
                             hipStream_t s);
// out [B][L] = (audio - mean_b) / sqrt(var_b + 1e-7) over clip b's own slen[b] samples (statistics in double; scratch stat [B]); samples at
// and beyond slen[b] are neither read nor written
hipError_t launch_wavlm_wave_norm(const float* audio, const int* slen, long long L, double2* stat, float* out, int B, hipStream_t s);
// launch_attention_k4p at heads of 64 with score(i, j) += gate[b][head][i] * toep[head][j - i + n_ctx - 1] (toep [heads][2 n_ctx - 1] in
// natural units); queries and keys = the clip's lens[b] rows (zeros beyond); T <= n_ctx
hipError_t launch_attention_k4p_bias(const float* qk, const float* vt, const float* gate, const float* toep, float* out, int B, int C, int T, int heads,
                                     const int* lens, int n_ctx, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Small dense layers with N = batch columns (time embedding path)
// out[b][m] = sum_k W[m][k] * g(in[b][k]) + bias[m];  g = identity | SiLU | sinusoid(t[b])
// ---------------------------------------------------------------------------------------------
enum { IN_PLAIN = 0, IN_SILU = 1, IN_SINUSOID = 2 };
hipError_t launch_small_linear(const float* W, const float* bias, const float* in, int in_stride, int in_mode,
                               const float* freqs, float* out, int out_stride, int out_silu, int M, int K, int B, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Elementwise sampler updates over n = B*M*T elements
// ---------------------------------------------------------------------------------------------
enum {
    EW_X0 = 1,        // out = (a - c0*b) / c1                         (x0 = (x - sigma*eps)/alpha)
    EW_AXPBY = 2,     // out = c0*a - c1*b                             (DPM first-order / UniPC x_t_)
    EW_DPM2 = 3,      // out = c0*a - c1*b - c2*(c3*(b - c))           (DPM-Solver++ 2M)
    EW_UNIPC_PRED = 4,// out = a - c0*(c1*((c - b)/c2))                (a = x_t_, b = m0, c = m_prev1)
    EW_UNIPC_CORR = 5,// out = a - c0*(c1*((d - b)/c2) + c3*(c - b))   (a = x_t_, b = m0, c = m_t, d = m_prev1)
    EW_UNIPC_CORR1 = 6,// out = a - c0*(c3*(c - b))                    (order-1 corrector)
    EW_DDPM = 7,      // x0 = clamp(c0*a - c1*b, -1, 1); out = c2*x0 + c3*a + c4*c   (a = x, b = eps, c = noise)
    EW_DDIM = 8,      // out = c0*(a/c1 + c2*b)
    EW_PLMS_PRED = 9, // out = a + c0*(c1*a - c2*b)
    EW_LIN4 = 10,     // out = (c0*a + c1*b + c2*c + c3*d) / c4
    EW_COPY = 11
};
hipError_t launch_ew(int op, float* out, const float* a, const float* b, const float* c, const float* d,
                     float c0, float c1, float c2, float c3, float c4, long long n, hipStream_t s);
hipError_t launch_dpm_step(float* x, const float* eps, float* m0, const float* m1, float sigma, float alpha, int second, float c4, float c5, float c6,
                           float c7, long long n, hipStream_t s);      // EW_X0 + EW_AXPBY / EW_DPM2 in one pass
hipError_t launch_fill(float* p, float v, long long n, hipStream_t s);
hipError_t launch_touch_lines(const float* p, long long bytes, hipStream_t s);      // experiment: lds_debug_set_touch_weights
struct FloatList64 { float f[64]; };
// dst[0..n) = host[0..n), n <= 64, carried in the kernel arguments (the host array is read during the call only)
hipError_t launch_set_list(float* dst, const float* host, int n, hipStream_t s);
hipError_t launch_transpose(const float* in, float* out, int B, int R, int C, float scale, hipStream_t s);
hipError_t launch_gather_rows(const float* table, const int64_t* idx, int idx_off, float* out, int B, int C,
                              int nrows, hipStream_t s);
hipError_t launch_resample_frames(const float* in, float* out, int B, int Tin, int Tout, int C, float step, hipStream_t s);
hipError_t launch_resample_nearest(const float* in, float* out, int B, int C, int Tin, int Tout, hipStream_t s);


// ---------------------------------------------------------------------------------------------
// Optional per-launch timing with HIP events on the launch stream (bench.py's roofline leg).
// ---------------------------------------------------------------------------------------------
// Called by a launcher inside an open ProfScope of this thread: two fresh events for hipExtLaunchKernelGGL's start / stop slots, which
// the runtime binds to the kernel's own begin / end timestamps (no extra packets on the stream, so neighbouring launches still
// overlap their dispatch as in an un-instrumented run).  false: no scope is open / the profiler is off -- launch normally.
bool prof_attach_events(hipEvent_t* start, hipEvent_t* stop);
// records the thread-local message returned by lds_last_error() and returns `code` (model.hip)
int set_error(int code, const char* fmt, ...);

struct ProfScope {
    bool on;
    hipStream_t s;
    int idx = -1;
    bool attached = false;      // the launch itself carries the two events (prof_attach_events): the destructor records nothing
    // attachable: the launcher inside the scope will bind the events to its dispatch (prof_attach_events): no event is recorded here
    ProfScope(hipStream_t st, const char* name, double flops, double bytes, bool attachable = false);
    ~ProfScope();
    void rename(const std::string& n);
};

// hipFuncAttributeMaxDynamicSharedMemorySize must be raised once per (kernel, device); `done` is that kernel's per-device bit mask
inline hipError_t ensure_max_dynamic_lds(const void* kern, std::atomic<unsigned long long>& done) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
    e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);      // idempotent: a concurrent second call is harmless
    if (e == hipSuccess) done.fetch_or(bit, std::memory_order_release);
    return e;
}

}  // namespace lds
