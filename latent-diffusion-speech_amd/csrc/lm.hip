// text2semantic RoFormer on gfx950 (reference text2semantic/roformer/roformer.py:59-255 over HF transformers RoFormerModel /
// RoFormerForCausalLM + GenerationMixin): phone/tone encoder prefill and the key/value-cached autoregressive decode with greedy or
// top-k / top-p sampling.  The model is tiny (hidden 256, 4 + 1 layers, 4.3 M parameters) and the caller decodes one to a few
// utterances, so every step is launch- and latency-bound: the design keeps the whole loop on the stream (no host round trip except
// an EOS poll every few steps), fuses bias / residual / LayerNorm / GELU into the matrix-vector kernels and reads each weight once
// per step with coalesced loads (weights stored transposed [K][M]).  Accumulation is one fp32 fmaf chain over k in ascending order
// per output, independent of the batch size.
#include "../../include/lds.h"
#include "kernels.h"
#include "host.h"
#include "lm_common.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <type_traits>
#include <vector>

namespace lds {

typedef float f32x4 __attribute__((ext_vector_type(4)));

static __device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// ---- embeddings: x = LN(word[tok] + type[tt]); encoder: x = LN(x + spk[spk_id] + type[0]) as well (roformer.py:196, the
//      embeddings module is applied a second time to inputs_embeds).  One workgroup per token, H <= 1024. ----
__global__ void __launch_bounds__(256) lm_embed_kernel(const float* __restrict__ word, const float* __restrict__ type, const float* __restrict__ spk,
                                                       const float* __restrict__ g, const float* __restrict__ bta, const int64_t* __restrict__ tok,
                                                       int tok_stride, const int64_t* __restrict__ tt, const int64_t* __restrict__ spk_id, int twice,
                                                       float eps, int H, int vocab, int type_vocab, int spk_rows, float* __restrict__ out) {
    __shared__ float red[4];
    const int n = blockIdx.x, tid = threadIdx.x;
    long long t = tok[(long long)n * tok_stride];
    long long ty = tt ? tt[n] : 0;
    t = (t < 0) ? 0 : (t >= vocab ? vocab - 1 : t);                 // ids are validated on the host; this only keeps a corrupted id from faulting
    ty = (ty < 0) ? 0 : (ty >= type_vocab ? type_vocab - 1 : ty);
    float v[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = tid + 256 * i;
        v[i] = (c < H) ? word[t * H + c] + type[ty * H + c] : 0.f;
        s += v[i];
    }
    for (int pass = 0; pass < (twice ? 2 : 1); ++pass) {
        const float mean = block_sum256(s, red) / (float)H;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) { const float d = (tid + 256 * i < H) ? v[i] - mean : 0.f; q += d * d; }
        const float rstd = 1.0f / sqrtf(block_sum256(q, red) / (float)H + eps);
        s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + 256 * i;
            if (c < H) {
                v[i] = (v[i] - mean) * rstd * g[c] + bta[c];
                if (pass == 0 && twice) {
                    long long sp = (spk && spk_id) ? spk_id[n] : 0;
                    sp = (sp < 0) ? 0 : (sp >= spk_rows ? spk_rows - 1 : sp);
                    v[i] += (spk && spk_id ? spk[sp * H + c] : 0.f) + type[c];
                }
            }
            s += (c < H) ? v[i] : 0.f;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (tid + 256 * i < H) out[(long long)n * H + tid + 256 * i] = v[i];
}

// ---- Y[n][m] = epi(sum_k LNopt(X)[n][k] * Wt[k][m] + b[m]) for a tile of 8 tokens per workgroup.  A decode step has 1-8 rows, so the
//      kernels are a latency problem, not a FLOP problem: a workgroup is 64 output columns x 16 K-slices (each thread walks K/16 weights
//      with 16 coalesced loads in flight), the partial sums meet through LDS in a fixed order (slice 0 adds slices 1, 2, ...). ----
// rotary embedding + cache append of the self-attention q | k | v projection (EPI 4): table row = [sin(d/2) | cos(d/2)], pairs (2p, 2p+1)
// (modeling_roformer.py:220-245); rotated q goes to Y, rotated k and v to kc / vc [B][heads][cap][d] at slot pos0 + l (row n = b * L + l)
struct LmRope { const float* table; float* kc; float* vc; int pos0, L, heads, cap; };
// PROW (prompted decode, L = 1): row b sits at its own position plen[b] - 1 + pos0 (pos0 = the global step).  A row that has run past the
// cache (position >= cap: it reached max_length at an earlier step) stores nothing.
struct LmRopeRow : LmRope { const int32_t* plen; };

// ---- Deferred LayerNorm.  A linear whose epilogue normalises complete rows needs one workgroup per row tile, i.e. ONE CU streaming the
//      whole weight matrix (~55 GB/s: 11 us for 256 x 256, four of them per decode step).  Here the producing linear keeps its
//      M / 64 column workgroups (5 us) and stores the PRE-normalisation rows; whoever reads them next normalises on the way in:
//        * a consumer linear stages its 8 input rows in LDS anyway -- it computes their mean / variance there (xg, xb != null);
//        * a consumer that adds them as the residual stages those rows as well (rg, rb != null).
//      The statistics are recomputed by every consuming workgroup (8 x 256 values: two block reductions), in a fixed order.
//      EPI 0: none, 1: GELU, 4: rotary + cache append (LmRope), 5: y + residual. ----
template <int NT>
static __device__ __forceinline__ void lm_rows_ln_inplace(float* buf, int L, const float* __restrict__ g, const float* __restrict__ bta, float eps, float* red8) {
    // wave j (< 8) owns row j: two wave reductions, no workgroup-wide reduction; the (mean, rstd) pairs are published through LDS
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (wave < 8) {
        float sum = 0.f;
        for (int k = lane; k < L; k += 64) sum += buf[8 * k + wave];
        const float mean = wave_sum(sum) / (float)L;
        float q = 0.f;
        for (int k = lane; k < L; k += 64) { const float d = buf[8 * k + wave] - mean; q += d * d; }
        const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)L + eps);
        if (lane == 0) { red8[2 * wave] = mean; red8[2 * wave + 1] = rstd; }
    }
    __syncthreads();
    float mean[8], rstd[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { mean[j] = red8[2 * j]; rstd[j] = red8[2 * j + 1]; }
    for (int k = tid; k < L; k += NT) {
        const float gk = g[k], bk = bta[k];
#pragma unroll
        for (int j = 0; j < 8; ++j) buf[8 * k + j] = (buf[8 * k + j] - mean[j]) * rstd[j] * gk + bk;
    }
    __syncthreads();
}

template <int EPI, bool PROW = false>
__global__ void __launch_bounds__(1024) lm_linear_dln_kernel(const float* __restrict__ X, int ldx, const float* __restrict__ xg, const float* __restrict__ xb,
                                                            const float* __restrict__ Wt, const float* __restrict__ bias, const float* __restrict__ R,
                                                            const float* __restrict__ rg, const float* __restrict__ rb, float eps, float* __restrict__ Y, int ldy,
                                                            int N, int K, int M, const std::conditional_t<PROW, LmRopeRow, LmRope> rope) {
    static_assert(!PROW || EPI == 4, "per-row positions belong to the rotary epilogue");
    constexpr int COLS = 64, KS = 16;
    extern __shared__ __attribute__((aligned(16))) float sm[];      // xs [K][8], part [KS-1][COLS][8], rs [M][8] (residual rows), red8 [16][8]
    float* xs = sm;
    float* part = sm + (size_t)K * 8;
    float* rs = part + (size_t)(KS - 1) * COLS * 8;
    float* red8 = rs + (size_t)((EPI == 5) ? M : 0) * 8;
    const int tid = threadIdx.x, col = tid % COLS, ks = tid / COLS;
    const int m = blockIdx.x * COLS + col, n0 = blockIdx.y * 8;
    for (int i = tid; i < K * 8; i += 1024) {
        const int k = i >> 3, j = i & 7;
        xs[i] = (n0 + j < N) ? X[(long long)(n0 + j) * ldx + k] : 0.f;
    }
    if constexpr (EPI == 5) {
        for (int i = tid; i < M * 8; i += 1024) {
            const int k = i >> 3, j = i & 7;
            rs[i] = (n0 + j < N) ? R[(long long)(n0 + j) * M + k] : 0.f;
        }
    }
    __syncthreads();
    if (xg) lm_rows_ln_inplace<1024>(xs, K, xg, xb, eps, red8);
    if constexpr (EPI == 5) {
        if (rg) lm_rows_ln_inplace<1024>(rs, M, rg, rb, eps, red8);
    }
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int kq = K / KS, k0 = ks * kq;                            // K % 256 == 0 (checked by the launcher)
    if (m < M) {
        const float* wp = Wt + (long long)k0 * M + m;
        for (int kk = 0; kk < kq; kk += 16) {
            float w[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) w[u] = wp[(long long)(kk + u) * M];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(xs + 8 * (k0 + kk + u)), b = *reinterpret_cast<const f32x4*>(xs + 8 * (k0 + kk + u) + 4);
                acc[0] = fmaf(w[u], a[0], acc[0]); acc[1] = fmaf(w[u], a[1], acc[1]); acc[2] = fmaf(w[u], a[2], acc[2]); acc[3] = fmaf(w[u], a[3], acc[3]);
                acc[4] = fmaf(w[u], b[0], acc[4]); acc[5] = fmaf(w[u], b[1], acc[5]); acc[6] = fmaf(w[u], b[2], acc[6]); acc[7] = fmaf(w[u], b[3], acc[7]);
            }
        }
    }
    if (ks > 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) part[((ks - 1) * COLS + col) * 8 + j] = acc[j];
    }
    __syncthreads();
    if (ks > 0) return;
#pragma unroll 1
    for (int q0 = 0; q0 < KS - 1; q0 += 5) {      // five slices in flight at a time (register budget of a 1024-thread workgroup)
        float t[5][8];
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
            for (int j = 0; j < 8; ++j) t[q][j] = part[((q0 + q) * COLS + col) * 8 + j];
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += t[q][j];
    }
    const float bm = (m < M && bias) ? bias[m] : 0.f;
    float y[8];
    bool ok[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        y[j] = acc[j] + bm;
        ok[j] = m < M && n0 + j < N;
        if constexpr (EPI == 1) y[j] = gelu_erf(y[j]);
        if constexpr (EPI == 5) { if (m < M) y[j] += rs[8 * m + j]; }
    }
    if constexpr (EPI == 4) {
        // slice 0 is exactly wave 0 and M % 64 == 0: the rotation partner of column m sits in the neighbouring lane
        const int H = M / 3, d = H / rope.heads, hp = d >> 1;
        const int sec = m / H, c = m - sec * H, hd = c / d, e = c - hd * d;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int n = (n0 + j < N) ? n0 + j : n0;
            const int b = n / rope.L;
            int pos = rope.pos0 + (n - b * rope.L);
            bool live = true;
            if constexpr (PROW) {
                pos += rope.plen[b] - 1;
                live = pos < rope.cap;
                pos = live ? pos : rope.cap - 1;      // (a finished row: its table row only has to exist)
            }
            const float sn = rope.table[(long long)pos * d + (e >> 1)], cs = rope.table[(long long)pos * d + hp + (e >> 1)];
            const float other = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, y[j]), 0xb1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
            const float rot = (e & 1) ? y[j] * cs + other * sn : y[j] * cs - other * sn;
            const long long co = (((long long)b * rope.heads + hd) * rope.cap + pos) * d + e;
            if (ok[j] && live) {
                if (sec == 0) Y[(long long)n * ldy + m] = rot;
                else if (sec == 1) rope.kc[co] = rot;
                else rope.vc[co] = y[j];
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (ok[j]) Y[(long long)(n0 + j) * ldy + m] = y[j];
    }
}

// LayerNorm of rows [N][H] (the encoder's final states, which leave the library normalised): one workgroup per row, H <= 1024
__global__ void __launch_bounds__(256) lm_ln_rows_kernel(const float* __restrict__ in, const float* __restrict__ g, const float* __restrict__ bta, float eps, int H,
                                                         float* __restrict__ out) {
    __shared__ float red[4];
    const long long n = blockIdx.x;
    const int tid = threadIdx.x;
    float v[4], s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int c = tid + 256 * i; v[i] = (c < H) ? in[n * H + c] : 0.f; s += v[i]; }
    const float mean = block_sum256(s, red) / (float)H;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const float d = (tid + 256 * i < H) ? v[i] - mean : 0.f; q += d * d; }
    const float rstd = 1.0f / sqrtf(block_sum256(q, red) / (float)H + eps);
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int c = tid + 256 * i; if (c < H) out[n * H + c] = (v[i] - mean) * rstd * g[c] + bta[c]; }
}

// cross-attention keys / values of the encoder states into the cache layout: kv [N][2H] (k | v) -> kc / vc [B][heads][cap][d]
__global__ void __launch_bounds__(256) lm_kv_pack_kernel(const float* __restrict__ kv, int B, int L, int H, int heads, float* __restrict__ kc,
                                                         float* __restrict__ vc, int cap) {
    const int d = H / heads;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * L * H) return;
    const int c = (int)(i % H);
    const long long n = i / H;
    const int l = (int)(n % L), b = (int)(n / L), hd = c / d, e = c - hd * d;
    const long long co = (((long long)b * heads + hd) * cap + l) * d + e;
    kc[co] = kv[n * 2 * H + c];
    vc[co] = kv[n * 2 * H + H + c];
}

// ---- attention of one query per workgroup: softmax(q K^T / sqrt(d)) V over Lk cached keys (no mask: the decoder's cache holds exactly
//      the causal context, the encoder is bidirectional).  q [N][ldq] (head slice at hd*d), out [N][H].  The four waves take alternate
//      64-key blocks; inside a wave, phase 1 has one key per lane (scores), phase 2 one output channel per lane with the two half-waves on
//      alternate keys; the waves' (max, sum, partial output) meet through LDS in a fixed order.  d <= 32. ----
// BEAM (lm_attn_beam_kernel, beam-search decode, Lq = 1): cache rows are beam rows.  src != null (self-attention): key p < Lk - 1 of row n
// lives in cache row src[n * src_cap + p] (the beam's ancestry, see lm_beam_step_kernel), the last key in row n itself.  group: rows per
// batch item of the cross-attention's keys / values and klen (b = n / group).  The source rows ride along the scores in LDS.
// CAUSAL (lm_attn_causal_kernel, the teacher-forced prefill of lds_lm_score, Lq = Lk_all = T, klen null): query l sees keys 0 .. l of the cache
// that the projection of all T rows has just filled -- the Lk of the cached decode at step l, hence its key striding over the waves, its
// block boundaries and its merge order: the row's arithmetic is the decode step's, bit for bit.
// PROW (lm_attn_rows_kernel, prompted decode, Lq = 1): klen = the rows' prompt lengths, row b sees its own plen[b] + kadd cached keys (kadd = the
// global step; the key the row has just appended at slot plen[b] - 1 + kadd is the last of them), at most Lk_all.  The lane blocks, the wave
// striding and the merge order depend on that count alone, so the row's arithmetic is that of the row decoded alone.
template <bool BEAM, bool CAUSAL = false, bool PROW = false>
static __device__ __forceinline__ void lm_attn_body(const float* __restrict__ q, int ldq, const float* __restrict__ kc, const float* __restrict__ vc, int cap,
                                                    int Lq, int Lk_all, const int* __restrict__ klen, int H, int heads, float* __restrict__ out,
                                                    const int* __restrict__ src, int src_cap, int group, int kadd = 0) {
    extern __shared__ float sc[];                      // [Lk rounded to 64] scores, then 4 x (max, sum, acc[32]) (BEAM: then [Lk rounded to 64] source rows)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int item = blockIdx.x;                       // (b, l, head)
    const int d = H / heads, Lkp = (Lk_all + 63) & ~63;
    const int hd = item % heads;
    const long long n = item / heads;                  // token index b * Lq + l
    const int b = BEAM ? (int)(n / Lq) / group : (int)(n / Lq);
    int* srow = reinterpret_cast<int*>(sc + Lkp + 4 * 34);
    // padding mask (reference roformer.py:209-236: attention_mask on the encoder's keys, encoder_attention_mask on the cross-attention's):
    // right-padded rows, so the mask of batch row b is "keys [0, klen[b])"; masked keys get probability exactly 0 as with HF's -inf bias
    const int kl = klen ? klen[b] : Lk_all;
    const int Lk = CAUSAL ? (int)(n - (long long)b * Lq) + 1 : PROW ? (kl + kadd < Lk_all ? kl + kadd : Lk_all) : (kl < Lk_all) ? (kl < 1 ? 1 : kl) : Lk_all;
    float* mrg = sc + Lkp;
    float qr[32];
#pragma unroll
    for (int e = 0; e < 32; ++e) qr[e] = (e < d) ? q[n * ldq + hd * d + e] : 0.f;
    const float* kb = kc + ((long long)b * heads + hd) * cap * d;
    const float* vb = vc + ((long long)b * heads + hd) * cap * d;
    const float scale = 1.0f / sqrtf((float)d);
    float mx = -INFINITY;
    for (int k0 = wave * 64; k0 < Lk; k0 += 256) {
        const int key = k0 + lane;
        float dot = -INFINITY;
        if (key < Lk) {
            dot = 0.f;
            const float* kbk = kb;
            if constexpr (BEAM) {
                if (src) {
                    const int r = (key == Lk - 1) ? (int)n : src[n * src_cap + key];
                    srow[key] = r;
                    kbk = kc + ((long long)r * heads + hd) * cap * d;
                }
            }
            if (d == 32) {      // the key row as eight 16-byte loads (a lane per key: every load instruction gathers 64 rows)
                const f32x4* kr = reinterpret_cast<const f32x4*>(kbk + (long long)key * 32);
                f32x4 kv[8];
#pragma unroll
                for (int e4 = 0; e4 < 8; ++e4) kv[e4] = kr[e4];
#pragma unroll
                for (int e = 0; e < 32; ++e) dot = fmaf(qr[e], kv[e >> 2][e & 3], dot);
            } else {
#pragma unroll
                for (int e = 0; e < 32; ++e)
                    if (e < d) dot = fmaf(qr[e], kbk[(long long)key * d + e], dot);
            }
            dot *= scale;
        }
        sc[key] = dot;
        mx = fmaxf(mx, dot);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    if (mx > -INFINITY) {
        for (int k0 = wave * 64; k0 < Lk; k0 += 256) {
            const int key = k0 + lane;
            const float p = (key < Lk) ? expf(sc[key] - mx) : 0.f;
            sc[key] = p;
            sum += p;
        }
    }
    sum = wave_sum(sum);
    __builtin_amdgcn_s_waitcnt(0xc07f);                // lgkmcnt(0): this wave's LDS writes are done before its reads below
    const int e = lane & 31, half = lane >> 5;
    float acc = 0.f;
    if (e < d && mx > -INFINITY)
        for (int k0 = wave * 64; k0 < Lk; k0 += 256) {
            const int kend = (k0 + 64 < Lk) ? k0 + 64 : Lk;
            if (BEAM && src) {
#pragma unroll 8
                for (int key = k0 + half; key < kend; key += 2)
                    acc = fmaf(sc[key], vc[(((long long)srow[key] * heads + hd) * cap + key) * d + e], acc);
            } else {
#pragma unroll 8
                for (int key = k0 + half; key < kend; key += 2) acc = fmaf(sc[key], vb[(long long)key * d + e], acc);
            }
        }
    acc += __shfl_xor(acc, 32, 64);
    if (lane == 0) { mrg[wave * 34] = mx; mrg[wave * 34 + 1] = sum; }
    if (half == 0) mrg[wave * 34 + 2 + e] = acc;
    __syncthreads();
    if (wave == 0 && half == 0 && e < d) {
        float m = fmaxf(fmaxf(mrg[0], mrg[34]), fmaxf(mrg[68], mrg[102]));
        float tot = 0.f, o = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float f = (mrg[w * 34] > -INFINITY) ? expf(mrg[w * 34] - m) : 0.f;
            tot += mrg[w * 34 + 1] * f;
            o += mrg[w * 34 + 2 + e] * f;
        }
        out[n * H + hd * d + e] = o / tot;
    }
}
__global__ void __launch_bounds__(256) lm_attn_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ kc, const float* __restrict__ vc, int cap,
                                                      int Lq, int Lk_all, const int* __restrict__ klen, int H, int heads, float* __restrict__ out) {
    lm_attn_body<false>(q, ldq, kc, vc, cap, Lq, Lk_all, klen, H, heads, out, nullptr, 0, 1);
}
__global__ void __launch_bounds__(256) lm_attn_beam_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ kc, const float* __restrict__ vc, int cap,
                                                           int Lq, int Lk_all, const int* __restrict__ klen, int H, int heads, float* __restrict__ out,
                                                           const int* __restrict__ src, int src_cap, int group) {
    lm_attn_body<true>(q, ldq, kc, vc, cap, Lq, Lk_all, klen, H, heads, out, src, src_cap, group);
}
__global__ void __launch_bounds__(256) lm_attn_causal_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ kc, const float* __restrict__ vc, int cap,
                                                             int T, int H, int heads, float* __restrict__ out) {
    lm_attn_body<false, true>(q, ldq, kc, vc, cap, T, T, nullptr, H, heads, out, nullptr, 0, 1);
}

__global__ void __launch_bounds__(256) lm_attn_rows_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ kc, const float* __restrict__ vc, int cap,
                                                           int Lk_all, const int* __restrict__ plen, int kadd, int H, int heads, float* __restrict__ out) {
    lm_attn_body<false, false, true>(q, ldq, kc, vc, cap, 1, Lk_all, plen, H, heads, out, nullptr, 0, 1, kadd);
}

// ---- teacher-forced scoring (lds_lm_score): the statistics of one logits row, one workgroup per row of a chunk [rows][V] whose first row is
//      row n0 = b * T + t of the batch.  Position t is counted when t + 1 < len_b and y = labels[b][t + 1] is a vocabulary id (HF's shift,
//      ForCausalLMLoss; -100 is the ignore index and every other id outside [0, V) is ignored with it):
//        lp   = logit_y - logsumexp_v logit_v        max and sum of exp in a fixed order (256 strided chains, DPP wave order, waves 0 .. 3),
//                                                     the final log in double, rounded once
//        rank = #{v : logit_v > logit_y} + #{v < y : logit_v == logit_y}      (the library's lowest-index tie rule)
//      Positions that are not counted get lp = 0, rank = -1; rows t = T - 1 have no label and write nothing. ----
__global__ void __launch_bounds__(256) lm_score_rows_kernel(const float* __restrict__ logits, long long n0, int V, int T, const int64_t* __restrict__ labels,
                                                            const int32_t* __restrict__ sem_len, float* __restrict__ lp, int32_t* __restrict__ rank) {
    __shared__ float red[4];
    const long long n = n0 + blockIdx.x;
    const int tid = threadIdx.x, b = (int)(n / T), t = (int)(n - (long long)b * T);
    if (t >= T - 1) return;
    int len = sem_len ? sem_len[b] : T;
    len = len > T ? T : len;
    const long long y = (t + 1 < len) ? labels[(long long)b * T + t + 1] : -100;
    const long long o = (long long)b * (T - 1) + t;
    if (y < 0 || y >= V) {      // (uniform over the workgroup)
        if (tid == 0) { lp[o] = 0.f; rank[o] = -1; }
        return;
    }
    const float* lg = logits + (long long)blockIdx.x * V;
    const float ly = lg[y];
    float m = -INFINITY, cnt = 0.f;      // the count stays below V (<= 8300 for the Llama's whole vocabulary), far below 2^24: exact in fp32 in any order
    for (int c = tid; c < V; c += 256) {
        const float v = lg[c];
        m = fmaxf(m, v);
        cnt += (v > ly || (v == ly && c < y)) ? 1.f : 0.f;
    }
    m = wave_max(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float s = 0.f;
    for (int c = tid; c < V; c += 256) s += expf(lg[c] - m);
    s = block_sum256(s, red);
    cnt = block_sum256(cnt, red);
    if (tid == 0) {
        lp[o] = (float)((double)ly - ((double)m + log((double)s)));
        rank[o] = (int)cnt;
    }
}
// loss = -(sum of the counted lp) / n_counted over the whole batch (HF's mean reduction; 0 / 0 = NaN when nothing is counted), as a fixed-order
// two-stage sum in double without atomics: one workgroup per batch row (256 strided chains, then a fixed tree), then one thread over the rows
__global__ void __launch_bounds__(256) lm_score_rowsum_kernel(const float* __restrict__ lp, const int32_t* __restrict__ rank, int T1, double* __restrict__ psum,
                                                              int32_t* __restrict__ pcnt) {
    __shared__ double sh[256];
    __shared__ int shc[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    double s = 0.0;
    int c = 0;
    for (int t = tid; t < T1; t += 256)
        if (rank[(long long)b * T1 + t] >= 0) { s += (double)lp[(long long)b * T1 + t]; ++c; }
    sh[tid] = s; shc[tid] = c;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) { sh[tid] += sh[tid + w]; shc[tid] += shc[tid + w]; }
        __syncthreads();
    }
    if (tid == 0) { psum[b] = sh[0]; pcnt[b] = shc[0]; }
}
__global__ void lm_score_loss_kernel(const double* __restrict__ psum, const int32_t* __restrict__ pcnt, int B, float* __restrict__ loss, int32_t* __restrict__ n_counted) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    int n = 0;
    for (int b = 0; b < B; ++b) { s += psum[b]; n += pcnt[b]; }
    *loss = (float)(-s / (double)n);
    *n_counted = n;
}

// ---- next-token choice per sequence (HF GenerationMixin._sample with RepetitionPenalty -> Temperature -> TopK -> TopP, then
//      softmax + one draw; greedy = argmax).  The draw is the inverse-CDF rule over the vocabulary order with a caller-supplied
//      uniform (torch.multinomial's own stream cannot be reproduced outside torch).  One workgroup per sequence, V <= 256 * 32. ----
constexpr int kMaxTopK = kLmMaxTopK;
// NoRepeatNGramLogitsProcessor (transformers generation/logits_process.py) over the history seq[0, len), BOS included: every window of n tokens
// whose first n - 1 equal the last n - 1 tokens of the history bans its last token (n = 1: every token seen so far).  Nothing is banned while
// len < n.  The banned ids are set as bits of ban[] (LDS, V <= 8192) by the threads [t0, t0 + nt); the caller zeroes ban and synchronises.
static __device__ __forceinline__ void lm_ngram_mark(const int64_t* __restrict__ seq, int len, int n, int V, unsigned* ban, int t0, int nt) {
    for (int i = t0; i + n <= len; i += nt) {
        bool match = true;
        for (int j = 0; j < n - 1 && match; ++j) match = seq[i + j] == seq[len - n + 1 + j];
        const long long t = seq[i + n - 1];
        if (match && t >= 0 && t < V) atomicOr(ban + (t >> 5), 1u << (t & 31));
    }
}

// PROW (prompted decode): row b continues a prompt of plen[b] tokens, so at the global step `step` it sits at position plen[b] - 1 + step: that is
// its history's last index, seq[that + 1] is the slot it writes, and a row whose slot would lie beyond the sequence (it reached max_length =
// cap_tokens at an earlier step) does nothing.  A row that writes the last slot counts as finished; every finishing row records its length in
// rowlen[b].  `step` still indexes the uniforms, the logits and the flag array.
template <int NI, bool NG, bool PROW = false>      // NI * 256 >= V: vocabulary slots per thread; NG: n-gram ban of size `ngram` after the repetition penalty
static __device__ __forceinline__ void lm_sample_body(const float* __restrict__ logits, int V, int do_sample, int top_k, float top_p, float inv_temp,
                                                      float rep_pen, const float* __restrict__ uniforms, int64_t* __restrict__ tokens, int cap_tokens,
                                                      int step, int* __restrict__ unfinished, int eos, int pad, int* __restrict__ any_unfinished,
                                                      const float* __restrict__ word, const float* __restrict__ type, const float* __restrict__ eg,
                                                      const float* __restrict__ eb, float eps, int H, float* __restrict__ xnext, int ngram,
                                                      const int32_t* __restrict__ plen = nullptr, int* __restrict__ rowlen = nullptr) {
    __shared__ float rv[4];
    __shared__ int ri[4];
    __shared__ int chosen;
    __shared__ float topv[kMaxTopK], pr[kMaxTopK];
    __shared__ int topi[kMaxTopK], ord[kMaxTopK];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int gstep = step;
    if constexpr (PROW) {
        step += plen[b] - 1;
        if (step + 1 >= cap_tokens) return;      // (uniform over the workgroup)
    }
    const float* lg = logits + (long long)b * V;
    int64_t* seq = tokens + (long long)b * cap_tokens;
    // thread 0 needs these at the very end: fetched now, their latency hides behind the top-k rounds
    const float u_draw = (tid == 0 && do_sample) ? uniforms[b] : 0.f;
    const int alive = (tid == 0) ? unfinished[b] : 0;
    float v[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int c = tid + 256 * i;
        v[i] = (c < V) ? lg[c] : -INFINITY;
    }
    if (rep_pen != 1.0f) {      // RepetitionPenaltyLogitsProcessor: every distinct token of the sequence so far is penalised once (gather / scatter)
        unsigned done = 0;
        for (int j = 0; j <= step; ++j) {
            const int t = (int)seq[j];
            if (t >= 0 && (t & 255) == tid && !((done >> (t >> 8)) & 1u)) {      // (negative: an id outside the columns, llama.hip's phone ids)
                done |= 1u << (t >> 8);
#pragma unroll
                for (int i = 0; i < NI; ++i)
                    if (i == (t >> 8)) v[i] = (v[i] < 0.f) ? v[i] * rep_pen : v[i] / rep_pen;
            }
        }
    }
    if constexpr (NG) {      // NoRepeatNGram comes after the repetition penalty and before the temperature (HF _get_logits_processor)
        __shared__ unsigned ban[256];
        ban[tid] = 0u;
        __syncthreads();
        lm_ngram_mark(seq, step + 1, ngram, V, ban, tid, 256);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = tid + 256 * i;
            if (c < V && ((ban[c >> 5] >> (c & 31)) & 1u)) v[i] = -INFINITY;
        }
    }
    if (do_sample && inv_temp != 1.0f) {
#pragma unroll
        for (int i = 0; i < NI; ++i) v[i] *= inv_temp;
    }
    // TopKLogitsWarper removes the scores BELOW the k-th largest (modeling: `scores < topk(scores, k)[..., -1]`), so every score tied with the
    // k-th one survives too: the selection runs on past k rounds while the next maximum still equals the k-th value (up to kMaxTopK survivors).
    const int rounds = do_sample ? top_k : 1;
    int n_sel = rounds;
    for (int r = 0; r < (do_sample ? kMaxTopK : 1); ++r) {      // r-th largest remaining value, ties to the lowest index
        float bv = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = tid + 256 * i;
            if (v[i] > bv || (v[i] == bv && c < bi && v[i] > -INFINITY)) { bv = v[i]; bi = c; }
        }
        {   // wave argmax: the largest value, then the lowest index among the lanes that hold it (NaNs never win)
            const float m = wave_max(bv);
            bi = wave_min_i((bv == m) ? bi : 0x7fffffff);
            bv = m;
        }
        __syncthreads();
        if (lane == 0) { rv[wave] = bv; ri[wave] = bi; }
        __syncthreads();
        bv = rv[0]; bi = ri[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (rv[w] > bv || (rv[w] == bv && ri[w] < bi)) { bv = rv[w]; bi = ri[w]; }
        if (r >= rounds) {      // (bv, topv are the same in every thread: the loop's exit is uniform)
            __syncthreads();
            if (!(bv == topv[rounds - 1]) || !(bv > -INFINITY)) { n_sel = r; break; }
            n_sel = r + 1;
        }
        if (tid == 0) { topv[r] = bv; topi[r] = bi; }
        if ((bi & 255) == tid) {
#pragma unroll
            for (int i = 0; i < NI; ++i)
                if (i == (bi >> 8)) v[i] = -INFINITY;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int next;
        if (!do_sample) {
            next = topi[0];
        } else {
            // softmax over the survivors (descending order in topv), optional nucleus cut, renormalise, draw in vocabulary order
            int kept = n_sel;
            float sum = 0.f;
            for (int j = 0; j < kept; ++j) { pr[j] = expf(topv[j] - topv[0]); sum += pr[j]; }
            if (top_p < 1.0f) {      // TopPLogitsWarper: drop the tail whose ascending cumulative probability stays <= 1 - top_p
                float tail = 0.f;
                int cut = kept;
                for (int j = kept - 1; j >= 1; --j) {
                    tail += pr[j] / sum;
                    if (tail <= 1.0f - top_p) cut = j; else break;
                }
                kept = cut;
                sum = 0.f;
                for (int j = 0; j < kept; ++j) sum += pr[j];
            }
            for (int j = 0; j < kept; ++j) pr[j] = pr[j] / sum;
            // vocabulary order (insertion sort of <= 64 entries), running sum, first index whose sum exceeds u
            for (int j = 0; j < kept; ++j) ord[j] = j;
            for (int j = 1; j < kept; ++j) {
                const int o = ord[j];
                int q = j - 1;
                while (q >= 0 && topi[ord[q]] > topi[o]) { ord[q + 1] = ord[q]; --q; }
                ord[q + 1] = o;
            }
            const float u = u_draw;
            float c = 0.f;
            next = topi[ord[kept - 1]];
            for (int j = 0; j < kept; ++j) {
                c += pr[ord[j]];
                if (c > u) { next = topi[ord[j]]; break; }
            }
        }
        if (next < 0 || next >= V) next = pad;                          // all-NaN logits: nothing compares greater than -inf
        if (!alive) next = pad;
        seq[step + 1] = next;
        chosen = next;
        const bool full = PROW && step + 2 >= cap_tokens;                  // the row has just written its last slot
        if (alive && (next == eos || full)) unfinished[b] = 0;
        if (alive && next != eos && !full) atomicOr(any_unfinished + gstep, 1);      // flag array indexed by step, zeroed by the host wrapper
        if constexpr (PROW) { if (alive && (next == eos || full)) rowlen[b] = step + 2; }
    }
    // the next decode step's input row, LayerNorm(word[next] + type[0]) (what lm_embed_kernel computes), without a launch of its own
    if (xnext) {
        __syncthreads();
        long long t = chosen;
        t = (t < 0) ? 0 : (t >= V ? V - 1 : t);
        float ev[4];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + 256 * i;
            ev[i] = (c < H) ? word[t * H + c] + type[c] : 0.f;
            s += ev[i];
        }
        const float mean = block_sum256(s, rv) / (float)H;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) { const float dd = (tid + 256 * i < H) ? ev[i] - mean : 0.f; q += dd * dd; }
        const float rstd = 1.0f / sqrtf(block_sum256(q, rv) / (float)H + eps);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + 256 * i;
            if (c < H) xnext[(long long)b * H + c] = (ev[i] - mean) * rstd * eg[c] + eb[c];
        }
    }
}

template <int NI>
__global__ void __launch_bounds__(256) lm_sample_kernel(const float* __restrict__ logits, int V, int do_sample, int top_k, float top_p, float inv_temp,
                                                        float rep_pen, const float* __restrict__ uniforms, int64_t* __restrict__ tokens, int cap_tokens,
                                                        int step, int* __restrict__ unfinished, int eos, int pad, int* __restrict__ any_unfinished,
                                                        const float* __restrict__ word, const float* __restrict__ type, const float* __restrict__ eg,
                                                        const float* __restrict__ eb, float eps, int H, float* __restrict__ xnext) {
    lm_sample_body<NI, false>(logits, V, do_sample, top_k, top_p, inv_temp, rep_pen, uniforms, tokens, cap_tokens, step, unfinished, eos, pad, any_unfinished,
                              word, type, eg, eb, eps, H, xnext, 0);
}
// the same with no_repeat_ngram_size = ngram >= 1
template <int NI>
__global__ void __launch_bounds__(256) lm_sample_ngram_kernel(const float* __restrict__ logits, int V, int do_sample, int top_k, float top_p, float inv_temp,
                                                              float rep_pen, const float* __restrict__ uniforms, int64_t* __restrict__ tokens, int cap_tokens,
                                                              int step, int* __restrict__ unfinished, int eos, int pad, int* __restrict__ any_unfinished,
                                                              const float* __restrict__ word, const float* __restrict__ type, const float* __restrict__ eg,
                                                              const float* __restrict__ eb, float eps, int H, float* __restrict__ xnext, int ngram) {
    lm_sample_body<NI, true>(logits, V, do_sample, top_k, top_p, inv_temp, rep_pen, uniforms, tokens, cap_tokens, step, unfinished, eos, pad, any_unfinished,
                             word, type, eg, eb, eps, H, xnext, ngram);
}

// ---- the same choice with NO top-k filter (HF: top_k = None / 0): RepetitionPenalty -> Temperature -> [TopP] -> softmax -> one draw over the whole
//      vocabulary.  An optional path (the reference's caller passes top_k = 5): the softmax normalisation and the inverse-CDF walk are serial loops of
//      one thread over an LDS copy of the row (~4 k adds each: tens of microseconds), in vocabulary order -- exactly what a sequential float32
//      cumsum computes, so the oracle restates it to the bit.  TopP (modeling: sort ascending, drop while the cumulative probability stays
//      <= 1 - top_p, always keep the largest): the cut is found as the largest probability value t with sum{p_j <= t} <= 1 - top_p by bisection
//      over the ordered bit patterns of the probabilities (31 block reductions); probabilities tied with the cut are dropped together. ----
template <bool NG, bool PROW = false>
static __device__ __forceinline__ void lm_sample_full_body(const float* __restrict__ logits, int V, float top_p, float inv_temp, float rep_pen,
                                                           const float* __restrict__ uniforms, int64_t* __restrict__ tokens, int cap_tokens, int step,
                                                           int* __restrict__ unfinished, int eos, int pad, int* __restrict__ any_unfinished,
                                                           const float* __restrict__ word, const float* __restrict__ type, const float* __restrict__ eg,
                                                           const float* __restrict__ eb, float eps, int H, float* __restrict__ xnext, int ngram,
                                                           const int32_t* __restrict__ plen = nullptr, int* __restrict__ rowlen = nullptr) {
    extern __shared__ float prob[];      // [V]
    __shared__ float rv[4];
    __shared__ int chosen;
    __shared__ float sh_max, sh_z;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int gstep = step;
    if constexpr (PROW) {      // the row's own position, as in lm_sample_body
        step += plen[b] - 1;
        if (step + 1 >= cap_tokens) return;
    }
    const float* lg = logits + (long long)b * V;
    int64_t* seq = tokens + (long long)b * cap_tokens;
    for (int c = tid; c < V; c += 256) prob[c] = lg[c];
    __syncthreads();
    if (rep_pen != 1.0f && tid == 0) {      // every distinct token of the sequence so far, once (a token met again finds its score already changed: marked by a NaN-free sentinel list)
        for (int j = 0; j <= step; ++j) {
            const int t = (int)seq[j];
            bool seen = false;
            for (int q = 0; q < j; ++q) seen = seen || ((int)seq[q] == t);
            if (!seen && t >= 0 && t < V) prob[t] = (prob[t] < 0.f) ? prob[t] * rep_pen : prob[t] / rep_pen;
        }
    }
    __syncthreads();
    if constexpr (NG) {      // the n-gram ban, between the repetition penalty and the temperature
        __shared__ unsigned ban[256];
        ban[tid] = 0u;
        __syncthreads();
        lm_ngram_mark(seq, step + 1, ngram, V, ban, tid, 256);
        __syncthreads();
        for (int c = tid; c < V; c += 256)
            if ((ban[c >> 5] >> (c & 31)) & 1u) prob[c] = -INFINITY;
        __syncthreads();
    }
    float m = -INFINITY;
    for (int c = tid; c < V; c += 256) {
        if (inv_temp != 1.0f) prob[c] *= inv_temp;
        m = fmaxf(m, prob[c]);
    }
    m = wave_max(m);
    if ((tid & 63) == 63) rv[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) sh_max = fmaxf(fmaxf(rv[0], rv[1]), fmaxf(rv[2], rv[3]));
    __syncthreads();
    for (int c = tid; c < V; c += 256) prob[c] = expf(prob[c] - sh_max);
    __syncthreads();
    if (tid == 0) {
        float z = 0.f;
        for (int c = 0; c < V; ++c) z += prob[c];
        sh_z = z;
    }
    __syncthreads();
    for (int c = tid; c < V; c += 256) prob[c] = prob[c] / sh_z;
    __syncthreads();
    if (top_p < 1.0f) {
        unsigned lo = 0u, hi = __float_as_uint(1.0f / sh_z);      // bit patterns of non-negative floats are ordered like the values; the largest p = 1 / z
        // largest t in [lo, hi) with f(t) = sum{p_j : bits(p_j) <= t} <= 1 - top_p; f(0) = 0 always qualifies (p = +0 entries)
        while (lo + 1 < hi) {
            const unsigned mid = lo + ((hi - lo) >> 1);
            float s = 0.f;
            for (int c = tid; c < V; c += 256) s += (__float_as_uint(prob[c]) <= mid) ? prob[c] : 0.f;
            s = block_sum256(s, rv);
            if (s <= 1.0f - top_p) lo = mid; else hi = mid;
            __syncthreads();
        }
        for (int c = tid; c < V; c += 256)
            if (__float_as_uint(prob[c]) <= lo) prob[c] = 0.f;      // (the largest probability has the pattern hi's upper end: never dropped)
        __syncthreads();
    }
    if (tid == 0) {
        const int alive = unfinished[b];
        float z = 0.f;
        for (int c = 0; c < V; ++c) z += prob[c];
        const float u = uniforms[b];
        float cs = 0.f;
        int next = -1, last = pad;
        for (int c = 0; c < V; ++c) {
            if (prob[c] > 0.f) last = c;
            cs += prob[c] / z;
            if (cs > u) { next = c; break; }
        }
        if (next < 0) next = last;      // (rounding left the running sum at or below u: the last candidate)
        if (!alive) next = pad;
        seq[step + 1] = next;
        chosen = next;
        const bool full = PROW && step + 2 >= cap_tokens;
        if (alive && (next == eos || full)) unfinished[b] = 0;
        if (alive && next != eos && !full) atomicOr(any_unfinished + gstep, 1);
        if constexpr (PROW) { if (alive && (next == eos || full)) rowlen[b] = step + 2; }
    }
    if (xnext) {      // the next decode step's input row, as lm_sample_kernel writes it
        __syncthreads();
        long long t = chosen;
        t = (t < 0) ? 0 : (t >= V ? V - 1 : t);
        float ev[4];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + 256 * i;
            ev[i] = (c < H) ? word[t * H + c] + type[c] : 0.f;
            s += ev[i];
        }
        const float mean = block_sum256(s, rv) / (float)H;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) { const float dd = (tid + 256 * i < H) ? ev[i] - mean : 0.f; q += dd * dd; }
        const float rstd = 1.0f / sqrtf(block_sum256(q, rv) / (float)H + eps);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + 256 * i;
            if (c < H) xnext[(long long)b * H + c] = (ev[i] - mean) * rstd * eg[c] + eb[c];
        }
    }
}

__global__ void __launch_bounds__(256) lm_sample_full_kernel(const float* __restrict__ logits, int V, float top_p, float inv_temp, float rep_pen,
                                                             const float* __restrict__ uniforms, int64_t* __restrict__ tokens, int cap_tokens, int step,
                                                             int* __restrict__ unfinished, int eos, int pad, int* __restrict__ any_unfinished,
                                                             const float* __restrict__ word, const float* __restrict__ type, const float* __restrict__ eg,
                                                             const float* __restrict__ eb, float eps, int H, float* __restrict__ xnext) {
    lm_sample_full_body<false>(logits, V, top_p, inv_temp, rep_pen, uniforms, tokens, cap_tokens, step, unfinished, eos, pad, any_unfinished, word, type, eg, eb,
                               eps, H, xnext, 0);
}
__global__ void __launch_bounds__(256) lm_sample_full_ngram_kernel(const float* __restrict__ logits, int V, float top_p, float inv_temp, float rep_pen,
                                                                   const float* __restrict__ uniforms, int64_t* __restrict__ tokens, int cap_tokens, int step,
                                                                   int* __restrict__ unfinished, int eos, int pad, int* __restrict__ any_unfinished,
                                                                   const float* __restrict__ word, const float* __restrict__ type, const float* __restrict__ eg,
                                                                   const float* __restrict__ eb, float eps, int H, float* __restrict__ xnext, int ngram) {
    lm_sample_full_body<true>(logits, V, top_p, inv_temp, rep_pen, uniforms, tokens, cap_tokens, step, unfinished, eos, pad, any_unfinished, word, type, eg, eb,
                              eps, H, xnext, ngram);
}

// the four choices above with per-row positions (lds_lm_generate_prompt): NG false ignores `ngram`
template <int NI, bool NG>
__global__ void __launch_bounds__(256) lm_sample_rows_kernel(const float* __restrict__ logits, int V, int do_sample, int top_k, float top_p, float inv_temp,
                                                             float rep_pen, const float* __restrict__ uniforms, int64_t* __restrict__ tokens, int cap_tokens,
                                                             int step, int* __restrict__ unfinished, int eos, int pad, int* __restrict__ any_unfinished,
                                                             const float* __restrict__ word, const float* __restrict__ type, const float* __restrict__ eg,
                                                             const float* __restrict__ eb, float eps, int H, float* __restrict__ xnext, int ngram,
                                                             const int32_t* __restrict__ plen, int* __restrict__ rowlen) {
    lm_sample_body<NI, NG, true>(logits, V, do_sample, top_k, top_p, inv_temp, rep_pen, uniforms, tokens, cap_tokens, step, unfinished, eos, pad, any_unfinished,
                                 word, type, eg, eb, eps, H, xnext, ngram, plen, rowlen);
}
template <bool NG>
__global__ void __launch_bounds__(256) lm_sample_full_rows_kernel(const float* __restrict__ logits, int V, float top_p, float inv_temp, float rep_pen,
                                                                  const float* __restrict__ uniforms, int64_t* __restrict__ tokens, int cap_tokens, int step,
                                                                  int* __restrict__ unfinished, int eos, int pad, int* __restrict__ any_unfinished,
                                                                  const float* __restrict__ word, const float* __restrict__ type, const float* __restrict__ eg,
                                                                  const float* __restrict__ eb, float eps, int H, float* __restrict__ xnext, int ngram,
                                                                  const int32_t* __restrict__ plen, int* __restrict__ rowlen) {
    lm_sample_full_body<NG, true>(logits, V, top_p, inv_temp, rep_pen, uniforms, tokens, cap_tokens, step, unfinished, eos, pad, any_unfinished, word, type, eg, eb,
                                  eps, H, xnext, ngram, plen, rowlen);
}

// the start of a prompted decode, one workgroup per row: tokens[b] = the row's prompt (ids clamped to the vocabulary), PAD from plen[b] on;
// ids [B][Pq] = the first Pq prompt positions of every row for the prefill's embedding (clamped as well; beyond plen[b] whatever the caller left there);
// last[b] = the row's last prompt token, the first decode step's input
__global__ void __launch_bounds__(256) lm_prompt_init_kernel(const int64_t* __restrict__ prompt, int P, const int32_t* __restrict__ plen, int V, int pad, int cap,
                                                             int Pq, int64_t* __restrict__ tokens, int64_t* __restrict__ ids, int64_t* __restrict__ last) {
    const int b = blockIdx.x, pl = plen[b];
    for (int l = threadIdx.x; l < cap; l += 256) {
        long long t = pad;
        if (l < P) {
            t = prompt[(long long)b * P + l];
            t = (t < 0) ? 0 : (t >= V ? V - 1 : t);
            if (l < Pq) ids[(long long)b * Pq + l] = t;
            if (l == pl - 1) last[b] = t;
            if (l >= pl) t = pad;
        }
        tokens[(long long)b * cap + l] = t;
    }
}

// ---- one step of HF's greedy beam search (transformers generation/utils.py _beam_search with _get_top_k_continuations,
//      _get_running_beams_for_next_iteration, _update_finished_beams, _check_early_stop_heuristic, _beam_search_has_unfinished_sequences;
//      length_penalty 1).  One workgroup per batch item b, whose K running beams are rows b * K + k of logits [B * K][V]:
//        scores = log_softmax(logits) -> RepetitionPenalty (on the log-probabilities) -> NoRepeatNGram (each beam's own history)
//                 + running score;  top 2K of the K * V scores (ties: the lower flat index k * V + token);
//        a candidate hits the stopping criteria on EOS or when its length reaches max_length;
//        next running beams = top K of (score + hit * -1e9); finished hypotheses = top K of the old ones and the new candidates
//        (score / generated length, plus the -1e9 masks as fp32 additions, in HF's order);  then the early-stop heuristic.
//      Each wave takes whole beam rows (K <= 8): the row sits in registers, NW = ceil(V / 64) values per lane, and the row's top 2K come
//      out of 2K wave argmax rounds; one thread merges the K lists of 2K (the running score is constant across a row, so the global top 2K
//      are among them) and does the O(K) bookkeeping from LDS copies of the item's state.  Sequences and the key/value ancestry table are
//      double-buffered (_in -> _out);
//      per-row scores and flags are read before they are rewritten, in place is allowed.  prev_flag (null at step 0): the previous step's
//      bits; when they say the search has ended the step changes nothing.  flag_out gets (OR over the batch) 1 = some item may still
//      improve, 2 = some item has an unfinished hypothesis slot, 4 = some candidate did not hit the stopping criteria, 8 = ended before.
//      ROWS (lm_beam_step_kernel<NW, true>, the Llama's decode: LmBeamRows in lm_common.h): every item continues a prompt of its own length plen[b], so
//      cur_len = plen[b] + step, the finished score divides by cur_len + 1 - plen[b] and the heuristic by that or by max_length - plen[b]; the
//      ids below first_free get -inf after the n-gram ban (HF's bad-word ban); the table holds generated positions only (entry p - plen[b]);
//      an item whose own loop has ended (ended_in 1) copies its state through ONCE, after which both buffers hold it (ended 2: the step does
//      nothing for it), and leaves the flag bits alone; flag_out gets 16 = some item still runs after this step.  No input row is written: the next step's embedding reads the token from the running sequence. ----
static __device__ __forceinline__ bool lm_beam_running(int f, int early_stopping) {      // _beam_search_has_unfinished_sequences over the batch
    return !(f & 8) && (f & 1) && (early_stopping != 1 || (f & 2)) && (f & 4);
}
// (The RoFormer's instantiation takes an empty struct last, where the per-row form takes LmBeamRows: its arguments lie where they lay before
// the per-row form existed, and the compiler gives it the code it had then.)
struct LmNoRows { static constexpr const int32_t* plen = nullptr; static constexpr int first_free = 0, tcap = 0; };
template <int NW, bool ROWS>
__global__ void __launch_bounds__(256) lm_beam_step_kernel(const float* __restrict__ logits, int V, int K, int step, int cap, int max_length, int eos,
                                                           float rep_pen, int ngram, int early_stopping, const LmBeamState st,
                                                           const float* __restrict__ word, const float* __restrict__ type, const float* __restrict__ eg,
                                                           const float* __restrict__ eb, float eps, int H, float* __restrict__ xnext,
                                                           const std::conditional_t<ROWS, LmBeamRows, LmNoRows> rw) {
    __shared__ unsigned pen_bits[4][256], ban_bits[4][256];
    __shared__ float cv[kMaxBeams][2 * kMaxBeams], topv[2 * kMaxBeams], sel_sc[kMaxBeams], nf_sc[kMaxBeams], f_sc[kMaxBeams];
    __shared__ int ci[kMaxBeams][2 * kMaxBeams], topb[2 * kMaxBeams], topt[2 * kMaxBeams], sel_j[kMaxBeams], nf_m[kMaxBeams], nf_fin[kMaxBeams], nf_len[kMaxBeams];
    __shared__ int f_fin[kMaxBeams], f_len[kMaxBeams], unsat_sh;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K2 = 2 * K, base = b * K;
    const int pl = ROWS ? rw.plen[b] : 1, cur_len = ROWS ? pl + step : step + 1;
    const int gen = ROWS ? cur_len + 1 - pl : cur_len;      // generated tokens of a hypothesis that ends at this step
    const int tp0 = ROWS ? pl : 0, tcap = ROWS ? rw.tcap : cap;      // the position of the table's entry 0, and its row stride
    if constexpr (ROWS) {
        const int was_ended = rw.ended_in[b];
        if (was_ended > 1) return;      // (uniform over the workgroup) frozen, and an earlier step has already left both buffers alike
        if (was_ended) {      // frozen: the state goes through as it is, once (ended 1 -> 2), the flag bits are not touched
            for (int i = tid; i < K * cap; i += 256) {
                const long long a = (long long)base * cap + i;
                st.rseq_out[a] = st.rseq_in[a]; st.fseq_out[a] = st.fseq_in[a];
            }
            if (st.tab_out)
                for (int i = tid; i < K * tcap; i += 256) st.tab_out[(long long)base * tcap + i] = st.tab_in[(long long)base * tcap + i];
            if (tid < K) {
                const int row = base + tid;
                const float rs = st.rscore_in[row], fs = st.fscore_in[row];
                const int ff = st.ffin_in[row], fl = st.flen_in[row];
                st.rscore_out[row] = rs; st.fscore_out[row] = fs; st.ffin_out[row] = ff; st.flen_out[row] = fl;
                if (st.parent) st.parent[row] = tid;
            }
            if (tid == 64) { const int u = st.unsat_in[b]; st.unsat_out[b] = u; rw.ended_out[b] = 2; }
            return;
        }
    } else if (st.prev_flag && !lm_beam_running(*st.prev_flag, early_stopping)) {
        if (tid == 0) atomicOr(st.flag_out, 8);
        return;
    }
    // the item's finished-hypothesis state, staged for the serial bookkeeping below (its loads overlap the rows' work)
    if (tid < K) { f_sc[tid] = st.fscore_in[base + tid]; f_fin[tid] = st.ffin_in[base + tid]; f_len[tid] = st.flen_in[base + tid]; }
    if (tid == 64) unsat_sh = st.unsat_in[b];
    for (int r0 = 0; r0 < K; r0 += 4) {      // (uniform trip count: the barriers below are reached by every wave)
        const int k = r0 + wave, row = base + k;
        const bool act = k < K;
        for (int i = lane; i < 256; i += 64) { pen_bits[wave][i] = 0u; ban_bits[wave][i] = 0u; }
        __syncthreads();
        if (act) {
            const int64_t* hist = st.rseq_in + (long long)row * cap;
            if (rep_pen != 1.0f)
                for (int j = lane; j < cur_len; j += 64) {
                    const long long t = hist[j];
                    if (t >= 0 && t < V) atomicOr(&pen_bits[wave][t >> 5], 1u << (t & 31));
                }
            if (ngram > 0) lm_ngram_mark(hist, cur_len, ngram, V, ban_bits[wave], lane, 64);
        }
        __syncthreads();
        if (act) {
            const float* lg = logits + (long long)row * V;
            float v[NW];
            float m = -INFINITY;
#pragma unroll
            for (int i = 0; i < NW; ++i) {
                const int c = lane + 64 * i;
                v[i] = (c < V) ? lg[c] : -INFINITY;
                m = fmaxf(m, v[i]);
            }
            m = wave_max(m);
            float z = 0.f;
#pragma unroll
            for (int i = 0; i < NW; ++i) z += (lane + 64 * i < V) ? expf(v[i] - m) : 0.f;
            const float lse = logf(wave_sum(z));
            const float rs = st.rscore_in[row];
#pragma unroll
            for (int i = 0; i < NW; ++i) {
                const int c = lane + 64 * i;
                float x = (v[i] - m) - lse;
                if ((pen_bits[wave][c >> 5] >> (c & 31)) & 1u) x = (x < 0.f) ? x * rep_pen : x / rep_pen;
                if ((ban_bits[wave][c >> 5] >> (c & 31)) & 1u) x = -INFINITY;
                if (ROWS && c < rw.first_free) x = -INFINITY;
                v[i] = (c < V) ? x + rs : -INFINITY;
            }
            for (int j = 0; j < K2; ++j) {      // the row's j-th largest score, ties to the lower token id
                float bv = -INFINITY;
                int bi = 0x7fffffff;
#pragma unroll
                for (int i = 0; i < NW; ++i)
                    if (v[i] > bv) { bv = v[i]; bi = lane + 64 * i; }
                const float mx = wave_max(bv);
                bi = wave_min_i((bv == mx) ? bi : 0x7fffffff);
                if (lane == 0) { cv[k][j] = mx; ci[k][j] = (bi < V) ? bi : 0; }
                if ((bi & 63) == lane) {
#pragma unroll
                    for (int i = 0; i < NW; ++i)
                        if (i == (bi >> 6)) v[i] = -INFINITY;
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        // _get_top_k_continuations: merge the K sorted lists (value descending, then flat index k * V + token ascending)
        int head[kMaxBeams];
        for (int k = 0; k < K; ++k) head[k] = 0;
        for (int j = 0; j < K2; ++j) {
            int bk = -1;
            for (int k = 0; k < K; ++k) {
                if (head[k] >= K2) continue;
                if (bk < 0 || cv[k][head[k]] > cv[bk][head[bk]]) bk = k;      // (k ascending: an equal value keeps the lower flat index)
            }
            topv[j] = cv[bk][head[bk]]; topb[j] = bk; topt[j] = ci[bk][head[bk]];
            ++head[bk];
        }
        bool hit[2 * kMaxBeams];
        bool all_hit = true;
        for (int j = 0; j < K2; ++j) { hit[j] = topt[j] == eos || cur_len + 1 >= max_length; all_hit = all_hit && hit[j]; }
        // _get_running_beams_for_next_iteration
        float trl[2 * kMaxBeams];
        for (int j = 0; j < K2; ++j) trl[j] = topv[j] + (hit[j] ? -1.0e9f : -0.0f);
        unsigned taken = 0u;
        for (int k = 0; k < K; ++k) {
            int bj = -1;
            for (int j = 0; j < K2; ++j)
                if (!((taken >> j) & 1u) && (bj < 0 || trl[j] > trl[bj])) bj = j;
            taken |= 1u << bj;
            sel_j[k] = bj; sel_sc[k] = trl[bj];
        }
        // _update_finished_beams (length_penalty 1: divide by the generated length cur_len + 1 - decoder_prompt_len)
        bool all_fin = true;
        for (int k = 0; k < K; ++k) all_fin = all_fin && f_fin[k] != 0;
        const int unsat = unsat_sh;
        float ms[3 * kMaxBeams];
        for (int k = 0; k < K; ++k) ms[k] = f_sc[k];
        for (int j = 0; j < K2; ++j) {
            const bool did = hit[j] && j < K;
            float f = topv[j] / (float)gen;
            f = f + ((all_fin && early_stopping == 1) ? -1.0e9f : -0.0f);
            f = f + (unsat ? -0.0f : -1.0e9f);
            f = f + (did ? -0.0f : -1.0e9f);
            ms[K + j] = f;
        }
        unsigned mtaken = 0u;
        float worst = INFINITY;
        bool nall_fin = true;
        for (int k = 0; k < K; ++k) {
            int bm = -1;
            for (int m = 0; m < K + K2; ++m)
                if (!((mtaken >> m) & 1u) && (bm < 0 || ms[m] > ms[bm])) bm = m;
            mtaken |= 1u << bm;
            nf_m[k] = bm; nf_sc[k] = ms[bm];
            nf_fin[k] = (bm < K) ? f_fin[bm] : (hit[bm - K] && bm - K < K) ? 1 : 0;
            nf_len[k] = (bm < K) ? f_len[bm] : gen;
            worst = fminf(worst, ms[bm]);
            nall_fin = nall_fin && nf_fin[k];
        }
        // _check_early_stop_heuristic at cur_len + 1 (early_stopping "never" with a positive length penalty: the best length is max_length)
        const int hyp = (early_stopping == 2) ? max_length - pl : gen;
        const float best = sel_sc[0] / (float)hyp;
        bool improve = false;
        for (int k = 0; k < K; ++k) improve = improve || best > (nf_fin[k] ? worst : -1.0e9f);
        const int nunsat = (unsat && improve) ? 1 : 0;
        st.unsat_out[b] = nunsat;
        int bits = (nunsat ? 1 : 0) | (nall_fin ? 0 : 2) | (all_hit ? 0 : 4);
        if constexpr (ROWS) {      // the item's own loop condition: the batch's OR would let a longer row keep a finished one running
            const bool run = nunsat && (early_stopping != 1 || !nall_fin) && !all_hit;
            rw.ended_out[b] = run ? 0 : 1;
            bits |= run ? 16 : 0;
        }
        atomicOr(st.flag_out, bits);
    }
    __syncthreads();
    // the new running sequences, finished hypotheses and ancestry tables: every (beam, position) pair at once
    const int n1 = cur_len + 1;
    for (int i = tid; i < K * n1; i += 256) {
        const int k = i / n1, p = i - k * n1;
        const int row = base + k, j = sel_j[k], par = base + topb[j], m = nf_m[k];
        const int64_t* fi = (m < K) ? st.fseq_in + (long long)(base + m) * cap : st.rseq_in + (long long)(base + topb[m - K]) * cap;
        st.rseq_out[(long long)row * cap + p] = (p < cur_len) ? st.rseq_in[(long long)par * cap + p] : (int64_t)topt[j];
        st.fseq_out[(long long)row * cap + p] = (m >= K && p == cur_len) ? (int64_t)topt[m - K] : fi[p];
        if (st.tab_out && (!ROWS || p >= tp0) && p < cur_len) st.tab_out[(long long)row * tcap + p - tp0] = (p < cur_len - 1) ? st.tab_in[(long long)par * tcap + p - tp0] : par;
    }
    if (tid < K) {
        const int row = base + tid;
        st.rscore_out[row] = sel_sc[tid];
        st.fscore_out[row] = nf_sc[tid]; st.ffin_out[row] = nf_fin[tid]; st.flen_out[row] = nf_len[tid];
        if (st.parent) st.parent[row] = topb[sel_j[tid]];
    }
    // the next step's input rows, LayerNorm(word[token] + type[0]) (lm_embed_kernel's rows): wave w takes beams w, w + 4 with
    // fixed-order wave sums (H <= 256, lds_lm_create allows 256)
    if (!ROWS && xnext) {
        for (int k = wave; k < K; k += 4) {
            long long t = topt[sel_j[k]];
            t = (t < 0) ? 0 : (t >= V ? V - 1 : t);
            float ev[4];
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = lane + 64 * i;
                ev[i] = (c < H) ? word[t * H + c] + type[c] : 0.f;
                s += ev[i];
            }
            const float mean = wave_sum(s) / (float)H;
            float q = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) { const float dd = (lane + 64 * i < H) ? ev[i] - mean : 0.f; q += dd * dd; }
            const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)H + eps);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = lane + 64 * i;
                if (c < H) xnext[(long long)(base + k) * H + c] = (ev[i] - mean) * rstd * eg[c] + eb[c];
            }
        }
    }
}

}  // namespace lds

using namespace lds;

// ================================================================================================
// host side
// ================================================================================================
struct LmLinear { float* wt = nullptr; float* b = nullptr; int K = 0, M = 0; };
struct LmLN { float* g = nullptr; float* b = nullptr; };
struct LmAttn { LmLinear qkv, q, kv, o; LmLN ln; };      // self: qkv fused; cross: q and kv separately
struct LmLayer { LmAttn self, cross; LmLinear ff1, ff2; LmLN ln_ff; bool has_cross = false; };
struct LmStack { float *word = nullptr, *type = nullptr, *table = nullptr; LmLN ln_emb; std::vector<LmLayer> layers; };

struct lds_lm {
    lds_lm_cfg cfg;
    Owner own;
    LmStack enc, dec;
    float* spk = nullptr;
    LmLinear head_t, head_d;
    LmLN head_ln;
};

namespace {
// reference layout W [M][K] -> transposed [K][M] (several matrices may be concatenated along M)
bool lm_linear(WeightLoader& T, const std::vector<std::string>& prefixes, int K, int Mper, LmLinear& out) {
    const int M = Mper * (int)prefixes.size();
    std::vector<float> wt((size_t)K * M), b(M);
    for (size_t s = 0; s < prefixes.size(); ++s) {
        const float* w = T.get(prefixes[s] + "weight", (int64_t)Mper * K);
        const float* bb = T.get(prefixes[s] + "bias", Mper);
        if (!w || !bb) return false;
        for (int m = 0; m < Mper; ++m) {
            for (int k = 0; k < K; ++k) wt[(size_t)k * M + s * Mper + m] = w[(size_t)m * K + k];
            b[s * Mper + m] = bb[m];
        }
    }
    out.wt = T.o.upload(wt); out.b = T.o.upload(b); out.K = K; out.M = M;
    return out.wt && out.b;
}
bool lm_vec(WeightLoader& T, const std::string& k, int64_t n, float*& out) {
    out = T.vec(k, n);
    return out != nullptr;
}
bool lm_ln(WeightLoader& T, const std::string& p, int H, LmLN& out) { return lm_vec(T, p + "weight", H, out.g) && lm_vec(T, p + "bias", H, out.b); }
bool lm_attn(WeightLoader& T, const std::string& p, int H, bool cross, LmAttn& a) {
    bool ok = true;
    if (cross) ok = lm_linear(T, {p + "self.query."}, H, H, a.q) && lm_linear(T, {p + "self.key.", p + "self.value."}, H, H, a.kv);
    else ok = lm_linear(T, {p + "self.query.", p + "self.key.", p + "self.value."}, H, H, a.qkv);
    return ok && lm_linear(T, {p + "output.dense."}, H, H, a.o) && lm_ln(T, p + "output.LayerNorm.", H, a.ln);
}
bool lm_stack(lds_lm* lm, WeightLoader& T, const std::string& p, int vocab, int type_vocab, int n_layers, bool cross, LmStack& s) {
    const lds_lm_cfg& c = lm->cfg;
    const int H = c.hidden, d = H / c.heads;
    bool ok = lm_vec(T, p + "embeddings.word_embeddings.weight", (int64_t)vocab * H, s.word) &&
              lm_vec(T, p + "embeddings.token_type_embeddings.weight", (int64_t)type_vocab * H, s.type) &&
              lm_ln(T, p + "embeddings.LayerNorm.", H, s.ln_emb) && lm_vec(T, p + "encoder.embed_positions.weight", (int64_t)c.max_pos * d, s.table);
    for (int i = 0; i < n_layers && ok; ++i) {
        LmLayer L;
        const std::string q = p + "encoder.layer." + std::to_string(i) + ".";
        L.has_cross = cross;
        ok = lm_attn(T, q + "attention.", H, false, L.self) && (!cross || lm_attn(T, q + "crossattention.", H, true, L.cross)) &&
             lm_linear(T, {q + "intermediate.dense."}, H, c.inter, L.ff1) && lm_linear(T, {q + "output.dense."}, c.inter, H, L.ff2) &&
             lm_ln(T, q + "output.LayerNorm.", H, L.ln_ff);
        s.layers.push_back(L);
    }
    return ok;
}
}  // namespace

extern "C" int lds_lm_create(const lds_lm_cfg* cfg, int n, const char* const* names, const float* const* ptrs, const int64_t* numel, lds_lm** out) {
    if (!cfg || !names || !ptrs || !numel || !out) return set_error(LDS_EINVAL, "null argument");
    if (cfg->hidden != 256 || cfg->heads <= 0 || cfg->hidden % cfg->heads || cfg->hidden / cfg->heads > 32 || (cfg->hidden / cfg->heads) % 2 ||
        cfg->sem_vocab > 256 * 32 || cfg->inter <= 0 || cfg->inter % 256 || cfg->inter > 3840)      // (inter: the staged rows of ff2 must fit in LDS)
        return set_error(LDS_EINVAL, "unsupported LM shape (hidden must be 256, head dim even and <= 32, vocabulary <= 8192, intermediate size a multiple of 256 <= 3840)");
    lds_lm* lm = new lds_lm();
    lm->cfg = *cfg;
    WeightLoader T(lm->own, n, names, ptrs, numel);
    const int H = cfg->hidden;
    bool ok = lm_stack(lm, T, "text_encoder.", cfg->text_vocab, cfg->type_vocab, cfg->enc_layers, false, lm->enc) &&
              lm_stack(lm, T, "semantic_decoder.roformer.", cfg->sem_vocab, 1, cfg->dec_layers, true, lm->dec);
    const std::string c = "semantic_decoder.cls.predictions.";
    ok = ok && lm_linear(T, {c + "transform.dense."}, H, H, lm->head_t) && lm_ln(T, c + "transform.LayerNorm.", H, lm->head_ln) &&
         lm_linear(T, {c + "decoder."}, H, cfg->sem_vocab, lm->head_d);
    if (ok && cfg->n_spk_rows > 0) ok = lm_vec(T, "spk_emb.weight", (int64_t)cfg->n_spk_rows * H, lm->spk);
    return T.finish(ok, "LM", lm, out, "LM weight tensor");
}
extern "C" void lds_lm_destroy(lds_lm* lm) { delete lm; }

namespace {
// beam-search state (K > 1): two buffers of the running sequences, of the ancestry table and of the finished hypotheses, per-row scores / flags
struct LmBeamWs { int64_t *rseq[2], *fseq[2]; int* tab[2]; float *rscore, *fscore; int *ffin, *flen, *unsat; };
// a prompted decode (P > 1): the prefill's token ids [B][P], every row's last prompt token [B] and the prompt lengths on the device [B]
struct LmPromptWs { int64_t *ids, *last; int32_t* plen; };
struct LmWs { float *x, *y, *z, *qkv, *ctx, *ff, *kv, *logits, *kc_tmp, *vc_tmp; int* flags; std::vector<float*> kc, vc, ckc, cvc; LmBeamWs beam; LmPromptWs prompt; };
// N = rows processed at once (B * L for the prefill, B * K for a decode step); K = beams per batch item (1: the layout of a plain decode)
// P = the prompt's width (1: no prompt, today's layout byte for byte): the prefill runs B * P rows through the activation buffers
void lm_plan(const lds_lm* lm, Arena& A, int B, int L, int cap, LmWs& w, int K = 1, int P = 1) {
    const lds_lm_cfg& c = lm->cfg;
    const size_t R = (size_t)B * K, BL = (size_t)B * (L > 1 ? L : 1), BP = (size_t)B * P, N0 = BL > R ? BL : R, N = N0 > BP ? N0 : BP, H = c.hidden;
    w.x = A.f(N * H); w.y = A.f(N * H); w.z = A.f(N * H); w.qkv = A.f(N * 3 * H); w.ctx = A.f(N * H); w.ff = A.f(N * c.inter); w.kv = A.f(N * 2 * H);
    w.logits = A.f(R * c.sem_vocab);
    w.kc_tmp = A.f(N * H); w.vc_tmp = A.f(N * H);
    w.flags = (int*)A.f((size_t)cap + R + 64);
    w.kc.clear(); w.vc.clear(); w.ckc.clear(); w.cvc.clear();
    for (int i = 0; i < c.dec_layers; ++i) {
        w.kc.push_back(A.f(R * H * cap)); w.vc.push_back(A.f(R * H * cap));
        w.ckc.push_back(A.f((size_t)B * H * L)); w.cvc.push_back(A.f((size_t)B * H * L));
    }
    w.beam = LmBeamWs{};
    if (K > 1) {
        for (int i = 0; i < 2; ++i) {
            w.beam.rseq[i] = (int64_t*)A.f(2 * R * cap); w.beam.fseq[i] = (int64_t*)A.f(2 * R * cap); w.beam.tab[i] = (int*)A.f(R * cap);
        }
        w.beam.rscore = A.f(R); w.beam.fscore = A.f(R); w.beam.ffin = (int*)A.f(R); w.beam.flen = (int*)A.f(R); w.beam.unsat = (int*)A.f(B);
    }
    w.prompt = LmPromptWs{};
    if (P > 1) { w.prompt.ids = (int64_t*)A.f(2 * BP); w.prompt.last = (int64_t*)A.f(2 * (size_t)B); w.prompt.plen = (int32_t*)A.f((size_t)B); }
}
hipError_t lm_attention(const float* q, int ldq, const float* kc, const float* vc, int cap, int B, int Lq, int Lk, const int* klen, const lds_lm_cfg& c, float* out,
                        hipStream_t st) {
    const int total = B * Lq * c.heads;
    const size_t lds = (size_t)(((Lk + 63) & ~63) + 4 * 34) * sizeof(float);
    hipLaunchKernelGGL(lm_attn_kernel, dim3(total), dim3(256), lds, st, q, ldq, kc, vc, cap, Lq, Lk, klen, c.hidden, c.heads, out);
    return hipGetLastError();
}
// the self-attention of the teacher-forced prefill (lm_attn_causal_kernel): T queries per item over the T keys just appended
hipError_t lm_attention_causal(const float* q, int ldq, const float* kc, const float* vc, int cap, int B, int T, const lds_lm_cfg& c, float* out, hipStream_t st) {
    const size_t lds = (size_t)(((T + 63) & ~63) + 4 * 34) * sizeof(float);
    hipLaunchKernelGGL(lm_attn_causal_kernel, dim3((unsigned)(B * T * c.heads)), dim3(256), lds, st, q, ldq, kc, vc, cap, T, c.hidden, c.heads, out);
    return hipGetLastError();
}
// beam rows of a decode step (lm_attn_beam_kernel): src = ancestry table of the self-attention (null for the cross-attention), group = beams
struct LmBeamAttn { const int* src; int K; };
hipError_t lm_attention_beam(const float* q, int ldq, const float* kc, const float* vc, int cap, int B, int Lq, int Lk, const int* klen, const lds_lm_cfg& c,
                             float* out, const int* src, int src_cap, int group, hipStream_t st) {
    const int total = B * Lq * c.heads, Lkp = (Lk + 63) & ~63;
    const size_t lds = (size_t)(Lkp + 4 * 34) * sizeof(float) + (src ? (size_t)Lkp * sizeof(int) : 0);
    hipLaunchKernelGGL(lm_attn_beam_kernel, dim3(total), dim3(256), lds, st, q, ldq, kc, vc, cap, Lq, Lk, klen, c.hidden, c.heads, out, src, src_cap, group);
    return hipGetLastError();
}
// one query per row over the row's own plen[b] + step cached keys (lm_attn_rows_kernel); Lk_max = the longest row's count, for the LDS size
hipError_t lm_attention_rows(const float* q, int ldq, const float* kc, const float* vc, int cap, int B, int Lk_max, const int32_t* plen, int step,
                             const lds_lm_cfg& c, float* out, hipStream_t st) {
    const size_t lds = (size_t)(((Lk_max + 63) & ~63) + 4 * 34) * sizeof(float);
    hipLaunchKernelGGL(lm_attn_rows_kernel, dim3((unsigned)(B * c.heads)), dim3(256), lds, st, q, ldq, kc, vc, cap, Lk_max, plen, step, c.hidden, c.heads, out);
    return hipGetLastError();
}
// rows [N][hidden] together with the LayerNorm that is still owed to them (ln == nullptr: already normalised)
struct LmRows { float* p; const LmLN* ln; };

template <int EPI>
hipError_t lm_dln(const LmLinear& W, const LmRows& X, int ldx, const LmRows* R, float eps, float* Y, int ldy, int N, hipStream_t st, const LmRope* rope = nullptr) {
    if (W.K % 256 || ((EPI == 4 || EPI == 5) && W.M % 64)) return hipErrorInvalidValue;
    if (EPI == 5 && !R) return hipErrorInvalidValue;
    if (EPI == 4 && (!rope || W.M % 192 || (W.M / 3 / rope->heads) % 2)) return hipErrorInvalidValue;
    auto kern = lm_linear_dln_kernel<EPI>;
    static std::atomic<unsigned long long> attr_done{0};
    hipError_t e = ensure_max_dynamic_lds(reinterpret_cast<const void*>(kern), attr_done);
    if (e != hipSuccess) return e;
    const size_t lds = ((size_t)W.K * 8 + (size_t)15 * 64 * 8 + (EPI == 5 ? (size_t)W.M * 8 : 0) + 16 * 8) * sizeof(float);
    const LmRope ro = rope ? *rope : LmRope{nullptr, nullptr, nullptr, 0, 1, 1, 0};
    hipLaunchKernelGGL(kern, dim3((W.M + 63) / 64, (N + 7) / 8), dim3(1024), lds, st, (const float*)X.p, ldx, X.ln ? X.ln->g : nullptr, X.ln ? X.ln->b : nullptr, W.wt, W.b,
                       R ? (const float*)R->p : nullptr, (R && R->ln) ? R->ln->g : nullptr, (R && R->ln) ? R->ln->b : nullptr, eps, Y, ldy, N, W.K, W.M, ro);
    return hipGetLastError();
}

// the self-attention projection of a prompted decode step (EPI 4 with per-row positions, N = B rows)
hipError_t lm_dln_rope_rows(const LmLinear& W, const LmRows& X, float eps, float* Y, int N, hipStream_t st, const LmRopeRow& rope) {
    if (W.K % 256 || W.M % 192 || (W.M / 3 / rope.heads) % 2 || rope.L != 1 || !rope.plen) return hipErrorInvalidValue;
    auto kern = lm_linear_dln_kernel<4, true>;
    static std::atomic<unsigned long long> attr_done{0};
    hipError_t e = ensure_max_dynamic_lds(reinterpret_cast<const void*>(kern), attr_done);
    if (e != hipSuccess) return e;
    const size_t lds = ((size_t)W.K * 8 + (size_t)15 * 64 * 8 + 16 * 8) * sizeof(float);
    hipLaunchKernelGGL(kern, dim3((W.M + 63) / 64, (N + 7) / 8), dim3(1024), lds, st, (const float*)X.p, W.K, X.ln ? X.ln->g : nullptr, X.ln ? X.ln->b : nullptr, W.wt,
                       W.b, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, eps, Y, W.M, N, W.K, W.M, rope);
    return hipGetLastError();
}

// one BERT-style post-LN layer over N = B * L rows; self-attention over [pos0, pos0 + L) appended to the cache (kc, vc).
// Every LayerNorm is deferred to the readers of its rows (lm_linear_dln_kernel): `x` comes in, and goes out, as rows + owed LayerNorm.
// The three row buffers of the workspace rotate: input -> a (attention block) -> c (cross-attention block) -> output in the input's buffer.
// self_klen / cross_klen: per-batch-row key counts of the padding mask (device int32 [B]) or null
// mode: which self-attention the layer runs (LmLayerMode; the default is the plain one over the keys [0, pos0 + L))
struct LmLayerMode {
    // decode steps of a beam search (B = rows = items * beam->K): the self-attention follows the ancestry table, the cross-attention maps row n to item n / K
    const LmBeamAttn* beam = nullptr;
    // the teacher-forced prefill (pos0 = 0, cap >= L): query l of the self-attention sees keys 0 .. l
    bool causal = false;
    // a prompted decode step (L = 1, pos0 = the global step): row b sits at position plen[b] - 1 + pos0; Lk_max = the longest row's key count
    const int32_t* plen = nullptr;
    int Lk_max = 0;
    static LmLayerMode beams(const LmBeamAttn* b) { LmLayerMode m; m.beam = b; return m; }
    static LmLayerMode prefill() { LmLayerMode m; m.causal = true; return m; }
    static LmLayerMode rows(const int32_t* plen, int Lk_max) { LmLayerMode m; m.plen = plen; m.Lk_max = Lk_max; return m; }
};
int lm_layer(const lds_lm* lm, const LmStack& s, const LmLayer& Ly, const LmWs& w, LmRows& x, int B, int L, int pos0, float* kc, float* vc, int cap,
             const float* ckc, const float* cvc, int Lenc, const int* self_klen, const int* cross_klen, hipStream_t st, const LmLayerMode& mode = LmLayerMode()) {
    const LmBeamAttn* beam = mode.beam;
    const bool causal = mode.causal;
    const int32_t* plen = mode.plen;
    const int Lk_max = mode.Lk_max;
    const lds_lm_cfg& c = lm->cfg;
    const int H = c.hidden, N = B * L;
    if (Ly.self.o.M != H || Ly.ff2.M != H || (Ly.has_cross && (Ly.cross.o.M != H || Ly.cross.q.K != H))) return set_error(LDS_EINVAL, "layer shapes");
    float* free1 = (x.p == w.x) ? w.y : w.x;
    float* free2 = (x.p == w.z) ? w.y : w.z;
    if (free1 == free2) free2 = w.x;
    if (plen) {
        LmRopeRow rope;
        rope.table = s.table; rope.kc = kc; rope.vc = vc; rope.pos0 = pos0; rope.L = L; rope.heads = c.heads; rope.cap = cap; rope.plen = plen;
        HIP_TRY(lm_dln_rope_rows(Ly.self.qkv, x, c.eps, w.qkv, N, st, rope));
    } else {
        const LmRope rope{s.table, kc, vc, pos0, L, c.heads, cap};      // rotary embedding and cache append in the projection's epilogue
        HIP_TRY(lm_dln<4>(Ly.self.qkv, x, H, nullptr, c.eps, w.qkv, 3 * H, N, st, &rope));
    }
    if (plen) HIP_TRY(lm_attention_rows(w.qkv, 3 * H, kc, vc, cap, B, Lk_max, plen, pos0, c, w.ctx, st));
    else if (causal) HIP_TRY(lm_attention_causal(w.qkv, 3 * H, kc, vc, cap, B, L, c, w.ctx, st));
    else if (beam) HIP_TRY(lm_attention_beam(w.qkv, 3 * H, kc, vc, cap, B, L, pos0 + L, self_klen, c, w.ctx, beam->src, cap, 1, st));
    else HIP_TRY(lm_attention(w.qkv, 3 * H, kc, vc, cap, B, L, pos0 + L, self_klen, c, w.ctx, st));
    const LmRows ctx{w.ctx, nullptr};
    HIP_TRY(lm_dln<5>(Ly.self.o, ctx, H, &x, c.eps, free1, H, N, st));               // a = W_o ctx + LN(x)
    LmRows cur{free1, &Ly.self.ln};
    if (Ly.has_cross) {
        HIP_TRY(lm_dln<0>(Ly.cross.q, cur, H, nullptr, c.eps, w.qkv, H, N, st));
        if (beam) HIP_TRY(lm_attention_beam(w.qkv, H, ckc, cvc, Lenc, B, L, Lenc, cross_klen, c, w.ctx, nullptr, 0, beam->K, st));
        else HIP_TRY(lm_attention(w.qkv, H, ckc, cvc, Lenc, B, L, Lenc, cross_klen, c, w.ctx, st));
        HIP_TRY(lm_dln<5>(Ly.cross.o, ctx, H, &cur, c.eps, free2, H, N, st));        // c = W_o' ctx' + LN(a)
        cur = LmRows{free2, &Ly.cross.ln};
    }
    HIP_TRY(lm_dln<1>(Ly.ff1, cur, H, nullptr, c.eps, w.ff, c.inter, N, st));
    const LmRows ff{w.ff, nullptr};
    HIP_TRY(lm_dln<5>(Ly.ff2, ff, c.inter, &cur, c.eps, x.p, H, N, st));              // g = W_2 f + LN(cur), into the input's buffer (no longer read)
    x.ln = &Ly.ln_ff;
    return LDS_OK;
}
}  // namespace

extern "C" int lds_lm_workspace_bytes(const lds_lm* lm, int B, int L, int max_length, size_t* out) {
    if (!lm || !out || B <= 0 || L <= 0 || max_length < 2) return set_error(LDS_EINVAL, "bad argument");
    Arena A(nullptr, 0);
    LmWs w;
    lm_plan(lm, A, B, L, max_length, w);
    *out = A.used;
    return LDS_OK;
}

// phone, tone [B,L] int64 (dev), spk_id [B,L] int64 or NULL, enc_len [B] int32 (dev) or NULL = the padding mask's key counts -> enc [B,L,hidden] (dev)
extern "C" int lds_lm_encode(lds_lm* lm, const int64_t* phone, const int64_t* tone, const int64_t* spk_id, const int32_t* enc_len, float* enc, void* ws,
                             size_t ws_bytes, int B, int L, void* stream) {
    if (!lm || !phone || !tone || !enc || !ws || B <= 0 || L <= 0) return set_error(LDS_EINVAL, "bad argument");
    const lds_lm_cfg& c = lm->cfg;
    if (L > c.max_pos) return set_error(LDS_EINVAL, "sequence longer than max_position_embeddings");
    hipStream_t st = (hipStream_t)stream;
    Arena A(ws, ws_bytes);
    LmWs w;
    lm_plan(lm, A, B, L, 2, w);
    if (!A.ok) return set_error(LDS_ENOMEM, "LM workspace too small: need %zu bytes", A.used);
    const int N = B * L, H = c.hidden;
    hipLaunchKernelGGL(lm_embed_kernel, dim3(N), dim3(256), 0, st, lm->enc.word, lm->enc.type, lm->spk, lm->enc.ln_emb.g, lm->enc.ln_emb.b, phone, 1, tone,
                       lm->spk ? spk_id : nullptr, 1, c.eps, H, c.text_vocab, c.type_vocab, c.n_spk_rows > 0 ? c.n_spk_rows : 1, w.x);
    HIP_TRY(hipGetLastError());
    LmRows cx{w.x, nullptr};
    for (const LmLayer& Ly : lm->enc.layers) {
        // the encoder's "cache" is just this layer's keys / values for all L positions
        int r = lm_layer(lm, lm->enc, Ly, w, cx, B, L, 0, w.kc_tmp, w.vc_tmp, L, nullptr, nullptr, 0, enc_len, nullptr, st);
        if (r != LDS_OK) return r;
    }
    if (cx.ln) {      // the states leave the library normalised
        hipLaunchKernelGGL(lm_ln_rows_kernel, dim3(N), dim3(256), 0, st, (const float*)cx.p, cx.ln->g, cx.ln->b, c.eps, H, enc);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemcpyAsync(enc, cx.p, sizeof(float) * N * H, hipMemcpyDeviceToDevice, st));
    }
    return LDS_OK;
}

namespace {
// the token choice of one decode step (K = 1): the n-gram variants only when no_repeat_ngram_size > 0, so a plain decode runs today's kernels
hipError_t lm_launch_choice(const lds_lm_decode_opts& o, int B, int V, const float* lg, float inv_temp, const float* u, int64_t* tokens, int cap, int step,
                            int* unfinished, int eos, int pad, int* any_unf, const float* word, const float* type, const float* eg, const float* eb, float eps,
                            int H, float* xnext, hipStream_t st) {
    const int ds = o.do_sample, tk = ds ? o.top_k : 1, ng = o.no_repeat_ngram_size;
    const float pen = o.repetition_penalty, tp = o.top_p;
    if (ds && o.top_k == 0) {
        if (ng > 0)
            hipLaunchKernelGGL(lm_sample_full_ngram_kernel, dim3(B), dim3(256), sizeof(float) * V, st, lg, V, tp, inv_temp, pen, u, tokens, cap, step, unfinished,
                               eos, pad, any_unf, word, type, eg, eb, eps, H, xnext, ng);
        else
            hipLaunchKernelGGL(lm_sample_full_kernel, dim3(B), dim3(256), sizeof(float) * V, st, lg, V, tp, inv_temp, pen, u, tokens, cap, step, unfinished,
                               eos, pad, any_unf, word, type, eg, eb, eps, H, xnext);
        return hipGetLastError();
    }
#define LM_CHOICE(NI)                                                                                                                                    \
    do {                                                                                                                                                 \
        if (ng > 0)                                                                                                                                      \
            hipLaunchKernelGGL(lm_sample_ngram_kernel<NI>, dim3(B), dim3(256), 0, st, lg, V, ds, tk, tp, inv_temp, pen, u, tokens, cap, step, unfinished, \
                               eos, pad, any_unf, word, type, eg, eb, eps, H, xnext, ng);                                                                \
        else                                                                                                                                             \
            hipLaunchKernelGGL(lm_sample_kernel<NI>, dim3(B), dim3(256), 0, st, lg, V, ds, tk, tp, inv_temp, pen, u, tokens, cap, step, unfinished,      \
                               eos, pad, any_unf, word, type, eg, eb, eps, H, xnext);                                                                    \
    } while (0)
    if (V <= 256 * 9) LM_CHOICE(9);
    else if (V <= 256 * 17) LM_CHOICE(17);      // (the reference's 4096-entry semantic codebook + 3 special ids)
    else LM_CHOICE(32);
#undef LM_CHOICE
    return hipGetLastError();
}
hipError_t lm_launch_beam_step(int B, int K, int V, const float* lg, int step, int cap, int max_length, int eos, float pen, int ngram, int es,
                               const LmBeamState& bs, const float* word, const float* type, const float* eg, const float* eb, float eps, int H, float* xnext,
                               hipStream_t st) {
    if (V <= 64 * 36)
        hipLaunchKernelGGL((lm_beam_step_kernel<36, false>), dim3(B), dim3(256), 0, st, lg, V, K, step, cap, max_length, eos, pen, ngram, es, bs, word, type, eg, eb, eps, H, xnext, LmNoRows{});
    else if (V <= kMaxBeamVocab)      // (4096 codes + 3 special ids; a row of 128 values per lane would spill)
        hipLaunchKernelGGL((lm_beam_step_kernel<68, false>), dim3(B), dim3(256), 0, st, lg, V, K, step, cap, max_length, eos, pen, ngram, es, bs, word, type, eg, eb, eps, H, xnext, LmNoRows{});
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}
}  // namespace

hipError_t lds::lm_launch_beam_rows(int B, int K, int V, const float* lg, int step, int cap, int max_length, int eos, float pen, int ngram, int es,
                                    const LmBeamState& bs, const LmBeamRows& rw, hipStream_t st) {
    const float* nf = nullptr;      // (no input row is written)
    if (V <= 64 * 36)
        hipLaunchKernelGGL((lm_beam_step_kernel<36, true>), dim3(B), dim3(256), 0, st, lg, V, K, step, cap, max_length, eos, pen, ngram, es, bs, nf, nf, nf, nf, 0.f, 0, (float*)nullptr, rw);
    else if (V <= kMaxBeamVocab)
        hipLaunchKernelGGL((lm_beam_step_kernel<68, true>), dim3(B), dim3(256), 0, st, lg, V, K, step, cap, max_length, eos, pen, ngram, es, bs, nf, nf, nf, nf, 0.f, 0, (float*)nullptr, rw);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// the option checks that need no model (they come before every other check of lds_lm_generate_opts; no device call)
int lds::lm_check_opts(const lds_lm_decode_opts& o, const float* logits_out) {
    if (o.num_beams < 1 || o.num_beams > kMaxBeams) return set_error(LDS_EINVAL, "num_beams %d out of range (1 .. %d)", o.num_beams, kMaxBeams);
    if (o.no_repeat_ngram_size < 0) return set_error(LDS_EINVAL, "no_repeat_ngram_size %d < 0", o.no_repeat_ngram_size);
    if (o.num_beams > 1 && o.do_sample)
        return set_error(LDS_EINVAL, "beam sampling (num_beams > 1 with do_sample) is not built: only greedy beam search");
    if (o.num_beams > 1 && (o.early_stopping < 0 || o.early_stopping > 2)) return set_error(LDS_EINVAL, "early_stopping must be 0 (False), 1 (True) or 2 (\"never\")");
    if (o.num_beams > 1 && logits_out) return set_error(LDS_EINVAL, "logits_out is not available with num_beams > 1");
    return LDS_OK;
}

extern "C" int lds_lm_workspace_bytes_opts(const lds_lm* lm, int B, int L, int max_length, int num_beams, size_t* out) {
    if (num_beams < 1 || num_beams > kMaxBeams) return set_error(LDS_EINVAL, "num_beams %d out of range (1 .. %d)", num_beams, kMaxBeams);
    if (!lm || !out || B <= 0 || L <= 0 || max_length < 2) return set_error(LDS_EINVAL, "bad argument");
    Arena A(nullptr, 0);
    LmWs w;
    lm_plan(lm, A, B, L, max_length, w, num_beams);
    *out = A.used;
    return LDS_OK;
}

// enc [B,L,hidden] (dev); uniforms [max_length-1][B] (dev, sampling only); tokens [B][max_length] int64 (dev): BOS then the generated ids,
// positions past the returned length are unspecified; logits_out optional [max_length-1][B][vocab] (dev).  *n_tokens_host = sequence length incl. BOS.
extern "C" int lds_lm_generate_opts(lds_lm* lm, const float* enc, const int32_t* enc_len, int B, int L, int max_length, const lds_lm_decode_opts* opts,
                                    const float* uniforms, int64_t* tokens, float* logits_out, int* n_tokens_host, void* ws, size_t ws_bytes, void* stream) {
    if (!opts) return set_error(LDS_EINVAL, "null options");
    const lds_lm_decode_opts o = *opts;
    if (int r = lm_check_opts(o, logits_out)) return r;
    if (!lm || !enc || !tokens || !n_tokens_host || !ws || B <= 0 || L <= 0 || max_length < 2) return set_error(LDS_EINVAL, "bad argument");
    const lds_lm_cfg& c = lm->cfg;
    const int do_sample = o.do_sample, top_k = o.top_k, K = o.num_beams;
    const float top_p = o.top_p, temperature = o.temperature;
    if (K > 1 && (2 * K > c.sem_vocab || c.sem_vocab > kMaxBeamVocab))
        return set_error(LDS_EINVAL, "beam search is built for vocabularies of 2 * num_beams .. %d entries", kMaxBeamVocab);
    if (do_sample && (!uniforms || top_k < 0 || top_k > kMaxTopK || top_k > c.sem_vocab || !(top_p > 0.f) || !(temperature > 0.f)))
        return set_error(LDS_EINVAL, "sampling needs uniforms, 0 <= top_k <= %d (0 = no top-k filter), top_p > 0, temperature > 0", kMaxTopK);
    if (do_sample && top_k == 0 && (size_t)c.sem_vocab * sizeof(float) > 60 * 1024) return set_error(LDS_EINVAL, "top_k = 0 needs the vocabulary row in LDS (<= 15360 entries)");
    if (max_length > c.max_pos) return set_error(LDS_EINVAL, "max_length exceeds max_position_embeddings");
    // the encoder states come from lds_lm_encode (L <= max_pos); the cross-attention stages one score per encoder position in LDS
    if (L < 1 || L > c.max_pos || (size_t)(((L + 63) & ~63) + 4 * 34) * sizeof(float) > 64 * 1024)
        return set_error(LDS_EINVAL, "encoder length %d out of range (1 .. min(max_position_embeddings = %d, 16000))", L, c.max_pos);
    // a beam decode stages one score and one source row per cached position in LDS
    if (K > 1 && (size_t)(((max_length + 63) & ~63) * 2 + 4 * 34) * sizeof(float) > 64 * 1024)
        return set_error(LDS_EINVAL, "max_length %d too long for a beam decode (<= 8000)", max_length);
    hipStream_t st = (hipStream_t)stream;
    Arena A(ws, ws_bytes);
    LmWs w;
    lm_plan(lm, A, B, L, max_length, w, K);
    if (!A.ok) return set_error(LDS_ENOMEM, "LM workspace too small: need %zu bytes", A.used);
    const int H = c.hidden, V = c.sem_vocab, R = B * K;
    int* unfinished = w.flags;                 // [R]
    int* any_unf = w.flags + R;                // [max_length]: 1 when a sequence is still running after step s (beam search: lm_beam_step_kernel's bits)
    // cross-attention keys / values of every decoder layer, once (one set per batch item, shared by its beams)
    for (int i = 0; i < c.dec_layers; ++i) {
        {
            const LmRows er{const_cast<float*>(enc), nullptr};
            HIP_TRY(lm_dln<0>(lm->dec.layers[i].cross.kv, er, H, nullptr, c.eps, w.kv, 2 * H, B * L, st));
        }
        hipLaunchKernelGGL(lm_kv_pack_kernel, dim3((unsigned)(((long long)B * L * H + 255) / 256)), dim3(256), 0, st, w.kv, B, L, H, c.heads, w.ckc[i], w.cvc[i], L);
        HIP_TRY(hipGetLastError());
    }
    std::vector<int64_t> bos((size_t)R * max_length, (int64_t)c.sem_pad);
    for (int r = 0; r < R; ++r) bos[(size_t)r * max_length] = c.sem_bos;
    {
        std::vector<int> init(R + max_length, 0);
        for (int b = 0; b < R; ++b) init[b] = 1;
        HIP_TRY(hipMemcpyAsync(unfinished, init.data(), sizeof(int) * (R + max_length), hipMemcpyHostToDevice, st));
        if (K == 1) {
            HIP_TRY(hipMemcpyAsync(tokens, bos.data(), sizeof(int64_t) * B * max_length, hipMemcpyHostToDevice, st));
        } else {      // HF _beam_search: running scores 0, -1e9, ...; finished scores -1e9; sequences BOS then PAD
            std::vector<float> rs(R, -1.0e9f), fs(R, -1.0e9f);
            std::vector<int> zero((size_t)R * max_length, 0), one(B, 1);
            for (int b = 0; b < B; ++b) rs[(size_t)b * K] = 0.f;
            for (int i = 0; i < 2; ++i) {
                HIP_TRY(hipMemcpyAsync(w.beam.rseq[i], bos.data(), sizeof(int64_t) * R * max_length, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(w.beam.fseq[i], bos.data(), sizeof(int64_t) * R * max_length, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(w.beam.tab[i], zero.data(), sizeof(int) * R * max_length, hipMemcpyHostToDevice, st));
            }
            HIP_TRY(hipMemcpyAsync(w.beam.rscore, rs.data(), sizeof(float) * R, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(w.beam.fscore, fs.data(), sizeof(float) * R, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(w.beam.ffin, zero.data(), sizeof(int) * R, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(w.beam.flen, zero.data(), sizeof(int) * R, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(w.beam.unsat, one.data(), sizeof(int) * B, hipMemcpyHostToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));      // (zero, one, rs, fs go out of scope)
        }
        HIP_TRY(hipStreamSynchronize(st));      // the host staging vectors go out of scope
    }
    const float inv_temp = do_sample ? 1.0f / temperature : 1.0f;
    int n_tokens = max_length, last_step = max_length - 2;
    std::vector<int> host_flags(max_length, 0);
    int checked = 0;
    for (int step = 0; step + 1 < max_length; ++step) {
        const int cur = step & 1;
        // token at position `step` -> logits -> token at position step + 1
        if (step == 0) {      // the BOS embedding; every later step's input row is written by the previous step's token-choice kernel
            hipLaunchKernelGGL(lm_embed_kernel, dim3(R), dim3(256), 0, st, lm->dec.word, lm->dec.type, (const float*)nullptr, lm->dec.ln_emb.g, lm->dec.ln_emb.b,
                               (const int64_t*)(K == 1 ? tokens : w.beam.rseq[0]), max_length, (const int64_t*)nullptr, (const int64_t*)nullptr, 0, c.eps, H,
                               c.sem_vocab, 1, 1, w.x);
            HIP_TRY(hipGetLastError());
        }
        LmRows cx{w.x, nullptr};
        const LmBeamAttn ba{w.beam.tab[cur], K};
        for (int i = 0; i < c.dec_layers; ++i) {
            int r = lm_layer(lm, lm->dec, lm->dec.layers[i], w, cx, R, 1, step, w.kc[i], w.vc[i], max_length, w.ckc[i], w.cvc[i], L, nullptr, enc_len, st,
                             LmLayerMode::beams(K > 1 ? &ba : nullptr));
            if (r != LDS_OK) return r;
        }
        // LM head: h = GELU(W_t LN(x)) stored un-normalised, logits = W_d LN(h)
        HIP_TRY(lm_dln<1>(lm->head_t, cx, H, nullptr, c.eps, w.ctx, H, R, st));
        const LmRows hrows{w.ctx, &lm->head_ln};
        float* lg = logits_out ? logits_out + (size_t)step * B * V : w.logits;
        HIP_TRY(lm_dln<0>(lm->head_d, hrows, H, nullptr, c.eps, lg, V, R, st));
        if (K == 1) {
            HIP_TRY(lm_launch_choice(o, B, V, lg, inv_temp, do_sample ? uniforms + (size_t)step * B : nullptr, tokens, max_length, step, unfinished, c.sem_eos,
                                    c.sem_pad, any_unf, lm->dec.word, lm->dec.type, lm->dec.ln_emb.g, lm->dec.ln_emb.b, c.eps, H, w.x, st));
        } else {
            const int nxt = cur ^ 1;
            const LmBeamState bs{w.beam.rseq[cur], w.beam.rseq[nxt], w.beam.rscore, w.beam.rscore, w.beam.tab[cur], w.beam.tab[nxt], w.beam.fseq[cur],
                                 w.beam.fseq[nxt], w.beam.fscore, w.beam.fscore, w.beam.ffin, w.beam.ffin, w.beam.flen, w.beam.flen, w.beam.unsat,
                                 w.beam.unsat, nullptr, step ? any_unf + step - 1 : nullptr, any_unf + step};
            HIP_TRY(lm_launch_beam_step(B, K, V, lg, step, max_length, max_length, c.sem_eos, o.repetition_penalty, o.no_repeat_ngram_size, o.early_stopping, bs,
                                       lm->dec.word, lm->dec.type, lm->dec.ln_emb.g, lm->dec.ln_emb.b, c.eps, H, w.x, st));
        }
        // EOS poll every 8 steps: the loop ends after the step in which the last running sequence emitted EOS (beam search: after the step
        // at which HF's loop condition turned false; the steps enqueued after it change nothing)
        if ((step & 7) == 7 || step + 2 == max_length) {
            HIP_TRY(hipMemcpyAsync(host_flags.data() + checked, any_unf + checked, sizeof(int) * (step + 1 - checked), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            bool done = false;
            for (int s = checked; s <= step; ++s) {
                const int f = host_flags[s];
                const bool running = (K == 1) ? f != 0 : (!(f & 8) && (f & 1) && (o.early_stopping != 1 || (f & 2)) && (f & 4));
                if (!running) { n_tokens = s + 2; last_step = s; done = true; break; }
            }
            checked = step + 1;
            if (done) break;
        }
    }
    if (K > 1) {      // the best finished hypothesis of every item (slot 0), cropped to the longest one; BOS first, EOS kept, PAD after it
        const int64_t* best = w.beam.fseq[(last_step + 1) & 1];
        std::vector<int> flen(R, 0);
        HIP_TRY(hipMemcpy2DAsync(tokens, sizeof(int64_t) * max_length, best, sizeof(int64_t) * max_length * K, sizeof(int64_t) * max_length, B,
                                hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(flen.data(), w.beam.flen, sizeof(int) * R, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        int gen = 0;
        for (int b = 0; b < B; ++b) gen = flen[(size_t)b * K] > gen ? flen[(size_t)b * K] : gen;
        n_tokens = 1 + gen;
    }
    *n_tokens_host = n_tokens;
    return LDS_OK;
}

extern "C" int lds_lm_generate(lds_lm* lm, const float* enc, const int32_t* enc_len, int B, int L, int max_length, int do_sample, int top_k, float top_p,
                               float temperature, float repetition_penalty, const float* uniforms, int64_t* tokens, float* logits_out, int* n_tokens_host,
                               void* ws, size_t ws_bytes, void* stream) {
    const lds_lm_decode_opts o{do_sample, top_k, top_p, temperature, repetition_penalty, 0, 1, 1};
    return lds_lm_generate_opts(lm, enc, enc_len, B, L, max_length, &o, uniforms, tokens, logits_out, n_tokens_host, ws, ws_bytes, stream);
}

// ---- prompted decode (lds_lm_generate_prompt): every row continues its own prompt of plen[b] tokens.
//      Prefill: the positions 0 .. Pq - 1 (Pq = the longest prompt - 1) of all rows go through the decoder layers in ONE causal pass
//      (lm_layer with causal = true, the pass of lds_lm_score) that appends their keys / values to the decode's own caches.  The head is skipped.
//      Decode: global step s handles row b at position plen[b] - 1 + s -- the row's last prompt token at s = 0 -- with the per-row forms of
//      the projection, the self-attention and the token choice.
//      INVARIANT: the prefill also fills the cache slots plen[b] - 1 .. Pq - 1 of a shorter row, from ids the caller never meant to be read
//      (clamped to the vocabulary).  No query ever sees them: step s of row b first overwrites slot plen[b] - 1 + s with the row's real token
//      and then reads the slots 0 .. plen[b] - 1 + s, so every slot a query reads was written from the prompt proper or by an earlier step
//      of the same row.  The same argument covers whatever the workspace held on entry. ----
namespace {
constexpr int kMaxPromptBatch = 64;      // the rows' final lengths live in the 64 spare ints behind the step flags (lm_plan)
// the shape checks, which need no model (they come before every check that does; no device call)
int lm_prompt_check(int B, int L, int max_length, int P) {
    if (B <= 0 || L <= 0 || max_length < 2 || P < 1) return set_error(LDS_EINVAL, "bad argument");
    if (B > kMaxPromptBatch) return set_error(LDS_EINVAL, "a prompted decode takes at most %d rows, got %d", kMaxPromptBatch, B);
    // the prefill's causal self-attention stages one score per key in LDS; its linears take 8 rows per workgroup along grid.y
    if ((size_t)(((P + 63) & ~63) + 4 * 34) * sizeof(float) > 64 * 1024 || (long long)B * P > 8 * 65535LL)
        return set_error(LDS_EINVAL, "prompt width %d too large (<= 16000, B * P <= 524280)", P);
    return LDS_OK;
}
}  // namespace

// (declared in lm_common.h: llama.hip's decode chooses its tokens through the same kernels)
hipError_t lds::lm_launch_choice_rows(const lds_lm_decode_opts& o, int B, int V, const float* lg, float inv_temp, const float* u, int64_t* tokens, int cap, int step,
                                 int* unfinished, int eos, int pad, int* any_unf, const float* word, const float* type, const float* eg, const float* eb, float eps,
                                 int H, float* xnext, const int32_t* plen, int* rowlen, hipStream_t st) {
    const int ds = o.do_sample, tk = ds ? o.top_k : 1, ng = o.no_repeat_ngram_size;
    const float pen = o.repetition_penalty, tp = o.top_p;
    if (ds && o.top_k == 0) {
        auto kern = ng > 0 ? lm_sample_full_rows_kernel<true> : lm_sample_full_rows_kernel<false>;
        hipLaunchKernelGGL(kern, dim3(B), dim3(256), sizeof(float) * V, st, lg, V, tp, inv_temp, pen, u, tokens, cap, step, unfinished, eos, pad, any_unf, word, type,
                           eg, eb, eps, H, xnext, ng, plen, rowlen);
        return hipGetLastError();
    }
    auto kern = (V <= 256 * 9)    ? (ng > 0 ? lm_sample_rows_kernel<9, true> : lm_sample_rows_kernel<9, false>)
                : (V <= 256 * 17) ? (ng > 0 ? lm_sample_rows_kernel<17, true> : lm_sample_rows_kernel<17, false>)
                                  : (ng > 0 ? lm_sample_rows_kernel<32, true> : lm_sample_rows_kernel<32, false>);
    hipLaunchKernelGGL(kern, dim3(B), dim3(256), 0, st, lg, V, ds, tk, tp, inv_temp, pen, u, tokens, cap, step, unfinished, eos, pad, any_unf, word, type, eg, eb, eps,
                       H, xnext, ng, plen, rowlen);
    return hipGetLastError();
}

extern "C" int lds_lm_workspace_bytes_prompt(const lds_lm* lm, int B, int L, int max_length, int P, size_t* out) {
    if (int r = lm_prompt_check(B, L, max_length, P)) return r;
    if (!lm || !out) return set_error(LDS_EINVAL, "bad argument");
    Arena A(nullptr, 0);
    LmWs w;
    lm_plan(lm, A, B, L, max_length, w, 1, P);
    *out = A.used;
    return LDS_OK;
}

extern "C" int lds_lm_generate_prompt(lds_lm* lm, const float* enc, const int32_t* enc_len, int B, int L, int max_length, const lds_lm_decode_opts* opts,
                                      const int64_t* prompt, const int32_t* prompt_len, int P, const float* uniforms, int64_t* tokens, float* logits_out,
                                      int* n_tokens_host, void* ws, size_t ws_bytes, void* stream) {
    if (!opts) return set_error(LDS_EINVAL, "null options");
    const lds_lm_decode_opts o = *opts;
    if (int r = lm_check_opts(o, logits_out)) return r;
    if (o.num_beams > 1) return set_error(LDS_EINVAL, "beam search from a prompt is not built (num_beams must be 1 with a prompt)");
    if (int r = lm_prompt_check(B, L, max_length, P)) return r;
    int Pmax = 0, Pmin = P;
    for (int b = 0; b < B; ++b) {
        const int pl = prompt_len ? prompt_len[b] : P;
        if (pl < 1 || pl > P) return set_error(LDS_EINVAL, "prompt_len[%d] = %d out of range (1 .. P = %d)", b, pl, P);
        if (pl >= max_length) return set_error(LDS_EINVAL, "prompt_len[%d] = %d leaves no room below max_length = %d (the total length, prompt included)", b, pl, max_length);
        Pmax = pl > Pmax ? pl : Pmax;
        Pmin = pl < Pmin ? pl : Pmin;
    }
    if (!lm || !enc || !tokens || !n_tokens_host || !ws || !prompt) return set_error(LDS_EINVAL, "bad argument");
    {   // the workspace is checked against the prompted plan whatever the lengths are
        Arena A(ws, ws_bytes);
        LmWs w;
        lm_plan(lm, A, B, L, max_length, w, 1, P);
        if (!A.ok) return set_error(LDS_ENOMEM, "LM workspace too small: need %zu bytes", A.used);
    }
    // every row is BOS alone: the plain decode, through its own launches (its plan is a prefix of the prompted one when P > 1)
    if (Pmax == 1) return lds_lm_generate_opts(lm, enc, enc_len, B, L, max_length, opts, uniforms, tokens, logits_out, n_tokens_host, ws, ws_bytes, stream);
    const lds_lm_cfg& c = lm->cfg;
    const int do_sample = o.do_sample, top_k = o.top_k;
    const float top_p = o.top_p, temperature = o.temperature;
    if (do_sample && (!uniforms || top_k < 0 || top_k > kMaxTopK || top_k > c.sem_vocab || !(top_p > 0.f) || !(temperature > 0.f)))
        return set_error(LDS_EINVAL, "sampling needs uniforms, 0 <= top_k <= %d (0 = no top-k filter), top_p > 0, temperature > 0", kMaxTopK);
    if (do_sample && top_k == 0 && (size_t)c.sem_vocab * sizeof(float) > 60 * 1024) return set_error(LDS_EINVAL, "top_k = 0 needs the vocabulary row in LDS (<= 15360 entries)");
    if (max_length > c.max_pos) return set_error(LDS_EINVAL, "max_length exceeds max_position_embeddings");
    if (L > c.max_pos || (size_t)(((L + 63) & ~63) + 4 * 34) * sizeof(float) > 64 * 1024)
        return set_error(LDS_EINVAL, "encoder length %d out of range (1 .. min(max_position_embeddings = %d, 16000))", L, c.max_pos);
    if ((size_t)(((max_length + 63) & ~63) + 4 * 34) * sizeof(float) > 64 * 1024) return set_error(LDS_EINVAL, "max_length %d too long for a prompted decode (<= 16000)", max_length);
    hipStream_t st = (hipStream_t)stream;
    Arena A(ws, ws_bytes);
    LmWs w;
    lm_plan(lm, A, B, L, max_length, w, 1, P);
    const int H = c.hidden, V = c.sem_vocab, Pq = Pmax - 1;
    int* unfinished = w.flags;                       // [B]
    int* any_unf = w.flags + B;                      // [max_length]: 1 when a row is still running after global step s
    int* rowlen = w.flags + B + max_length;          // [B <= 64]: every row's final length, prompt included
    for (int i = 0; i < c.dec_layers; ++i) {         // cross-attention keys / values, as in lds_lm_generate_opts
        const LmRows er{const_cast<float*>(enc), nullptr};
        HIP_TRY(lm_dln<0>(lm->dec.layers[i].cross.kv, er, H, nullptr, c.eps, w.kv, 2 * H, B * L, st));
        hipLaunchKernelGGL(lm_kv_pack_kernel, dim3((unsigned)(((long long)B * L * H + 255) / 256)), dim3(256), 0, st, w.kv, B, L, H, c.heads, w.ckc[i], w.cvc[i], L);
        HIP_TRY(hipGetLastError());
    }
    {
        std::vector<int> init(B + max_length + kMaxPromptBatch, 0), pl(B);
        for (int b = 0; b < B; ++b) { init[b] = 1; init[B + max_length + b] = max_length; pl[b] = prompt_len ? prompt_len[b] : P; }
        HIP_TRY(hipMemcpyAsync(unfinished, init.data(), sizeof(int) * init.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(w.prompt.plen, pl.data(), sizeof(int) * B, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));      // the host staging vectors go out of scope
    }
    const int32_t* plen = w.prompt.plen;
    hipLaunchKernelGGL(lm_prompt_init_kernel, dim3(B), dim3(256), 0, st, prompt, P, plen, V, c.sem_pad, max_length, Pq, tokens, w.prompt.ids, w.prompt.last);
    HIP_TRY(hipGetLastError());
    {   // prefill: positions 0 .. Pq - 1 of every row, keys / values straight into the decode caches (see the invariant above)
        hipLaunchKernelGGL(lm_embed_kernel, dim3(B * Pq), dim3(256), 0, st, lm->dec.word, lm->dec.type, (const float*)nullptr, lm->dec.ln_emb.g, lm->dec.ln_emb.b,
                           (const int64_t*)w.prompt.ids, 1, (const int64_t*)nullptr, (const int64_t*)nullptr, 0, c.eps, H, V, 1, 1, w.x);
        HIP_TRY(hipGetLastError());
        LmRows px{w.x, nullptr};
        for (int i = 0; i < c.dec_layers; ++i) {
            int r = lm_layer(lm, lm->dec, lm->dec.layers[i], w, px, B, Pq, 0, w.kc[i], w.vc[i], max_length, w.ckc[i], w.cvc[i], L, nullptr, enc_len, st, LmLayerMode::prefill());
            if (r != LDS_OK) return r;
        }
    }
    // the first step's input rows: every row's last prompt token; later rows come from the token choice
    hipLaunchKernelGGL(lm_embed_kernel, dim3(B), dim3(256), 0, st, lm->dec.word, lm->dec.type, (const float*)nullptr, lm->dec.ln_emb.g, lm->dec.ln_emb.b,
                       (const int64_t*)w.prompt.last, 1, (const int64_t*)nullptr, (const int64_t*)nullptr, 0, c.eps, H, V, 1, 1, w.x);
    HIP_TRY(hipGetLastError());
    const float inv_temp = do_sample ? 1.0f / temperature : 1.0f;
    const int n_steps = max_length - Pmin;      // the shortest row writes its last slot at step n_steps - 1
    std::vector<int> host_flags(n_steps, 0);
    int checked = 0;
    for (int step = 0; step < n_steps; ++step) {
        LmRows cx{w.x, nullptr};
        const int Lk_max = (Pmax + step < max_length) ? Pmax + step : max_length;
        for (int i = 0; i < c.dec_layers; ++i) {
            int r = lm_layer(lm, lm->dec, lm->dec.layers[i], w, cx, B, 1, step, w.kc[i], w.vc[i], max_length, w.ckc[i], w.cvc[i], L, nullptr, enc_len, st,
                             LmLayerMode::rows(plen, Lk_max));
            if (r != LDS_OK) return r;
        }
        HIP_TRY(lm_dln<1>(lm->head_t, cx, H, nullptr, c.eps, w.ctx, H, B, st));
        const LmRows hrows{w.ctx, &lm->head_ln};
        float* lg = logits_out ? logits_out + (size_t)step * B * V : w.logits;
        HIP_TRY(lm_dln<0>(lm->head_d, hrows, H, nullptr, c.eps, lg, V, B, st));
        HIP_TRY(lm_launch_choice_rows(o, B, V, lg, inv_temp, do_sample ? uniforms + (size_t)step * B : nullptr, tokens, max_length, step, unfinished, c.sem_eos,
                                     c.sem_pad, any_unf, lm->dec.word, lm->dec.type, lm->dec.ln_emb.g, lm->dec.ln_emb.b, c.eps, H, w.x, plen, rowlen, st));
        if ((step & 7) == 7 || step + 1 == n_steps) {      // the EOS poll of lds_lm_generate_opts; a row that reached max_length counts as finished
            HIP_TRY(hipMemcpyAsync(host_flags.data() + checked, any_unf + checked, sizeof(int) * (step + 1 - checked), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            bool done = false;
            for (int s = checked; s <= step && !done; ++s) done = host_flags[s] == 0;
            checked = step + 1;
            if (done) break;
        }
    }
    // cropped to the longest row.  (Steps enqueued past the last running row's end only wrote PAD behind finished rows.)
    std::vector<int> len(B, 0);
    HIP_TRY(hipMemcpyAsync(len.data(), rowlen, sizeof(int) * B, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int n_tokens = 0;
    for (int b = 0; b < B; ++b) n_tokens = len[b] > n_tokens ? len[b] : n_tokens;
    *n_tokens_host = n_tokens;
    return LDS_OK;
}

// ---- teacher-forced scoring: the decoder stack over all B * T rows in one causal pass, then the head over row chunks of kScoreChunk rows
//      through one reused buffer (or straight into logits_out), each chunk followed by its row statistics.  Every row goes through the
//      kernels of the decode (lm_linear_dln_kernel's fmaf chain per row does not depend on the row count; lm_attn_causal_kernel restates the
//      cached step), so the logits equal the decode's bit for bit. ----
namespace {
constexpr int kScoreChunk = 256;
struct LmScoreWs { LmWs w; float *kc, *vc, *ckc, *cvc, *chunk; double* psum; int32_t* pcnt; };
void lm_score_plan(const lds_lm* lm, Arena& A, int B, int L, int T, LmScoreWs& s) {
    const lds_lm_cfg& c = lm->cfg;
    const size_t N = (size_t)B * T, NL = (size_t)B * L, H = c.hidden;
    s.w = LmWs{};
    s.w.x = A.f(N * H); s.w.y = A.f(N * H); s.w.z = A.f(N * H); s.w.qkv = A.f(N * 3 * H); s.w.ctx = A.f(N * H); s.w.ff = A.f(N * c.inter);
    s.w.kv = A.f(NL * 2 * H);
    s.kc = A.f(N * H); s.vc = A.f(N * H);              // one layer's self-attention keys / values at a time
    s.ckc = A.f(NL * H); s.cvc = A.f(NL * H);          // and its cross-attention keys / values
    s.chunk = A.f((size_t)kScoreChunk * c.sem_vocab);
    s.psum = (double*)A.f(2 * (size_t)B);
    s.pcnt = (int32_t*)A.f((size_t)B);
}
int lm_score_check(const lds_lm* lm, int B, int L, int T) {
    if (!lm || B <= 0) return set_error(LDS_EINVAL, "bad argument");
    const lds_lm_cfg& c = lm->cfg;
    if (T < 2 || T > c.max_pos) return set_error(LDS_EINVAL, "sequence length %d out of range (2 .. max_position_embeddings = %d)", T, c.max_pos);
    if (L < 1 || L > c.max_pos || (size_t)(((L + 63) & ~63) + 4 * 34) * sizeof(float) > 64 * 1024)
        return set_error(LDS_EINVAL, "encoder length %d out of range (1 .. min(max_position_embeddings = %d, 16000))", L, c.max_pos);
    // the causal self-attention stages one score per key in LDS; the linears take 8 rows per workgroup along grid.y
    if ((size_t)(((T + 63) & ~63) + 4 * 34) * sizeof(float) > 64 * 1024) return set_error(LDS_EINVAL, "sequence length %d too long for scoring (<= 16000)", T);
    if ((long long)B * T > 8 * 65535LL || (long long)B * L > 8 * 65535LL) return set_error(LDS_EINVAL, "batch too large for one scoring call (B * T and B * L <= 524280)");
    return LDS_OK;
}
}  // namespace

extern "C" int lds_lm_score_workspace_bytes(const lds_lm* lm, int B, int L, int T, size_t* out) {
    if (!out) return set_error(LDS_EINVAL, "bad argument");
    if (int r = lm_score_check(lm, B, L, T)) return r;
    Arena A(nullptr, 0);
    LmScoreWs s;
    lm_score_plan(lm, A, B, L, T, s);
    *out = A.used;
    return LDS_OK;
}

extern "C" int lds_lm_score(lds_lm* lm, const float* enc, const int32_t* enc_len, int B, int L, const int64_t* semantic, const int32_t* sem_len, const int64_t* labels,
                            int T, float* logprobs, int32_t* ranks, float* loss, int32_t* n_counted, float* logits_out, void* ws, size_t ws_bytes, void* stream) {
    if (int r = lm_score_check(lm, B, L, T)) return r;
    if (!enc || !semantic || !logprobs || !ranks || !loss || !n_counted || !ws) return set_error(LDS_EINVAL, "null argument");
    const lds_lm_cfg& c = lm->cfg;
    hipStream_t st = (hipStream_t)stream;
    Arena A(ws, ws_bytes);
    LmScoreWs s;
    lm_score_plan(lm, A, B, L, T, s);
    if (!A.ok) return set_error(LDS_ENOMEM, "LM scoring workspace too small: need %zu bytes", A.used);
    const int H = c.hidden, V = c.sem_vocab, N = B * T;
    if (!labels) labels = semantic;
    // ids are clamped to the vocabulary (lm_embed_kernel); rows at and beyond a sequence's length are computed and never counted
    hipLaunchKernelGGL(lm_embed_kernel, dim3(N), dim3(256), 0, st, lm->dec.word, lm->dec.type, (const float*)nullptr, lm->dec.ln_emb.g, lm->dec.ln_emb.b, semantic, 1,
                       (const int64_t*)nullptr, (const int64_t*)nullptr, 0, c.eps, H, V, 1, 1, s.w.x);
    HIP_TRY(hipGetLastError());
    LmRows cx{s.w.x, nullptr};
    for (int i = 0; i < c.dec_layers; ++i) {
        const LmRows er{const_cast<float*>(enc), nullptr};
        HIP_TRY(lm_dln<0>(lm->dec.layers[i].cross.kv, er, H, nullptr, c.eps, s.w.kv, 2 * H, B * L, st));
        hipLaunchKernelGGL(lm_kv_pack_kernel, dim3((unsigned)(((long long)B * L * H + 255) / 256)), dim3(256), 0, st, s.w.kv, B, L, H, c.heads, s.ckc, s.cvc, L);
        HIP_TRY(hipGetLastError());
        int r = lm_layer(lm, lm->dec, lm->dec.layers[i], s.w, cx, B, T, 0, s.kc, s.vc, T, s.ckc, s.cvc, L, nullptr, enc_len, st, LmLayerMode::prefill());
        if (r != LDS_OK) return r;
    }
    // LM head as in the decode: h = GELU(W_t LN(x)) stored un-normalised, logits = W_d LN(h), the latter chunk by chunk
    HIP_TRY(lm_dln<1>(lm->head_t, cx, H, nullptr, c.eps, s.w.ctx, H, N, st));
    for (int r0 = 0; r0 < N; r0 += kScoreChunk) {
        const int rows = (N - r0 < kScoreChunk) ? N - r0 : kScoreChunk;
        const LmRows hrows{s.w.ctx + (size_t)r0 * H, &lm->head_ln};
        float* lg = logits_out ? logits_out + (size_t)r0 * V : s.chunk;
        HIP_TRY(lm_dln<0>(lm->head_d, hrows, H, nullptr, c.eps, lg, V, rows, st));
        HIP_TRY(lm_launch_score_rows(lg, r0, rows, V, T, labels, sem_len, logprobs, ranks, st));
    }
    HIP_TRY(lm_launch_score_loss(logprobs, ranks, B, T - 1, s.psum, s.pcnt, loss, n_counted, st));
    return LDS_OK;
}

// (declared in lm_common.h: llama.hip's scoring takes its row statistics and its loss from the same kernels)
hipError_t lds::lm_launch_score_rows(const float* logits, long long n0, int rows, int V, int T, const int64_t* labels, const int32_t* len, float* lp, int32_t* rank,
                                     hipStream_t st) {
    hipLaunchKernelGGL(lm_score_rows_kernel, dim3(rows), dim3(256), 0, st, logits, n0, V, T, labels, len, lp, rank);
    return hipGetLastError();
}
hipError_t lds::lm_launch_score_loss(const float* lp, const int32_t* rank, int B, int T1, double* psum, int32_t* pcnt, float* loss, int32_t* n_counted, hipStream_t st) {
    hipLaunchKernelGGL(lm_score_rowsum_kernel, dim3(B), dim3(256), 0, st, lp, rank, T1, psum, pcnt);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lm_score_loss_kernel, dim3(1), dim3(64), 0, st, (const double*)psum, (const int32_t*)pcnt, B, loss, n_counted);
    return hipGetLastError();
}

// Test entry (include/lds_test.h): ONE token choice per row of `logits` [B][V] with the generate loop's own kernels, after a history of n_hist tokens
// per row (hist [B][n_hist] int64, dev; what the repetition penalty looks at).  out [B] int64 (dev).  top_k 0 = no top-k filter.
extern "C" int lds_test_lm_sample(const float* logits, int B, int V, int do_sample, int top_k, float top_p, float temperature, float repetition_penalty,
                                  const float* uniforms, const int64_t* hist, int n_hist, int64_t* out, void* stream) {
    if (!logits || !out || B <= 0 || V <= 0 || V > 256 * 32 || n_hist < 1 || !hist || (do_sample && !uniforms) || top_k < 0 || top_k > kMaxTopK) return set_error(LDS_EINVAL, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int cap = n_hist + 1;
    int64_t* seq = nullptr;
    int* flags = nullptr;
    if (hipMalloc(&seq, sizeof(int64_t) * B * cap) != hipSuccess || hipMalloc(&flags, sizeof(int) * (B + cap)) != hipSuccess) return set_error(LDS_ENOMEM, "alloc");
    std::vector<int> init(B + cap, 0);
    for (int b = 0; b < B; ++b) init[b] = 1;
    int rc = LDS_OK;
    do {
        if (hipMemcpy(flags, init.data(), sizeof(int) * (B + cap), hipMemcpyHostToDevice) != hipSuccess) { rc = set_error(LDS_EHIP, "copy"); break; }
        if (hipMemcpy2DAsync(seq, sizeof(int64_t) * cap, hist, sizeof(int64_t) * n_hist, sizeof(int64_t) * n_hist, B, hipMemcpyDeviceToDevice, st) != hipSuccess) {
            rc = set_error(LDS_EHIP, "copy"); break;
        }
        const float inv_temp = do_sample ? 1.0f / temperature : 1.0f;
        const int step = n_hist - 1;
        const float* nf = nullptr;
        if (do_sample && top_k == 0)
            hipLaunchKernelGGL(lm_sample_full_kernel, dim3(B), dim3(256), sizeof(float) * V, st, logits, V, top_p, inv_temp, repetition_penalty, uniforms, seq, cap, step,
                               flags, -1, -1, flags + B, nf, nf, nf, nf, 0.f, 0, (float*)nullptr);
        else if (V <= 256 * 9)
            hipLaunchKernelGGL(lm_sample_kernel<9>, dim3(B), dim3(256), 0, st, logits, V, do_sample, do_sample ? top_k : 1, top_p, inv_temp, repetition_penalty, uniforms, seq, cap,
                               step, flags, -1, -1, flags + B, nf, nf, nf, nf, 0.f, 0, (float*)nullptr);
        else if (V <= 256 * 17)
            hipLaunchKernelGGL(lm_sample_kernel<17>, dim3(B), dim3(256), 0, st, logits, V, do_sample, do_sample ? top_k : 1, top_p, inv_temp, repetition_penalty, uniforms, seq, cap,
                               step, flags, -1, -1, flags + B, nf, nf, nf, nf, 0.f, 0, (float*)nullptr);
        else
            hipLaunchKernelGGL(lm_sample_kernel<32>, dim3(B), dim3(256), 0, st, logits, V, do_sample, do_sample ? top_k : 1, top_p, inv_temp, repetition_penalty, uniforms, seq, cap,
                               step, flags, -1, -1, flags + B, nf, nf, nf, nf, 0.f, 0, (float*)nullptr);
        if (hipGetLastError() != hipSuccess) { rc = set_error(LDS_EHIP, "launch"); break; }
        if (hipMemcpy2DAsync(out, sizeof(int64_t), seq + n_hist, sizeof(int64_t) * cap, sizeof(int64_t), B, hipMemcpyDeviceToDevice, st) != hipSuccess) {
            rc = set_error(LDS_EHIP, "copy"); break;
        }
        if (hipStreamSynchronize(st) != hipSuccess) rc = set_error(LDS_EHIP, "sync");
    } while (0);
    (void)hipFree(seq);
    (void)hipFree(flags);
    return rc;
}

// Test entry (include/lds_test.h): ONE beam-search step (lm_beam_step_kernel) on logits [B * K][V] and the given state (all dev); the step is
// cur_len - 1 (history = the first cur_len ids of every running sequence, sequences [B * K][max_length] int64).  Outputs as in the kernel;
// parent_out [B * K] = parent beam (0 .. K - 1) of every new running beam; flag_out [1] = the step's bits (1 | 2 | 4, see lm_beam_step_kernel).
extern "C" int lds_test_lm_beam_step(const float* logits, int B, int K, int V, int cur_len, int max_length, int eos, float repetition_penalty,
                                     int no_repeat_ngram_size, int early_stopping, const int64_t* run_seq, const float* run_score, const int64_t* fin_seq,
                                     const float* fin_score, const int32_t* fin_flag, const int32_t* fin_len, const int32_t* unsat, int64_t* run_seq_out,
                                     float* run_score_out, int32_t* parent_out, int64_t* fin_seq_out, float* fin_score_out, int32_t* fin_flag_out,
                                     int32_t* fin_len_out, int32_t* unsat_out, int32_t* flag_out, void* stream) {
    if (!logits || !run_seq || !run_score || !fin_seq || !fin_score || !fin_flag || !fin_len || !unsat || !run_seq_out || !run_score_out || !parent_out ||
        !fin_seq_out || !fin_score_out || !fin_flag_out || !fin_len_out || !unsat_out || !flag_out)
        return set_error(LDS_EINVAL, "null argument");
    if (B <= 0 || K < 1 || K > kMaxBeams || V < 2 * K || V > kMaxBeamVocab || cur_len < 1 || cur_len >= max_length || no_repeat_ngram_size < 0 ||
        early_stopping < 0 || early_stopping > 2)
        return set_error(LDS_EINVAL, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    const LmBeamState bs{run_seq, run_seq_out, run_score, run_score_out, nullptr, nullptr, fin_seq, fin_seq_out, fin_score, fin_score_out, fin_flag, fin_flag_out,
                         fin_len, fin_len_out, unsat, unsat_out, parent_out, nullptr, flag_out};
    if (hipMemsetAsync(flag_out, 0, sizeof(int32_t), st) != hipSuccess) return set_error(LDS_EHIP, "memset");
    const float* nf = nullptr;
    if (lm_launch_beam_step(B, K, V, logits, cur_len - 1, max_length, max_length, eos, repetition_penalty, no_repeat_ngram_size, early_stopping, bs, nf, nf, nf, nf,
                            0.f, 0, nullptr, st) != hipSuccess)
        return set_error(LDS_EHIP, "launch");
    if (hipStreamSynchronize(st) != hipSuccess) return set_error(LDS_EHIP, "sync");
    return LDS_OK;
}
