// text2semantic Llama on gfx950 (reference text2semantic/llama/llama.py:23-184 over HF transformers LlamaForCausalLM + GenerationMixin): a
// decoder-only LM over one token stream [phone BOS, phones, phone EOS, semantic BOS, semantic tokens ...].  One causal prefill of the prompts
// fills the key/value caches, then the cached decode continues row by row; the token choice is lm.hip's (lm_common.h).
// Everything is fp32 and follows lm.hip's rules: one fixed-order accumulation per output that depends neither on the batch size nor on whether
// a row is a prefill row or a decode step (both go through the SAME kernels, a row's position being the only thing that tells them apart), no
// atomics, the whole decode loop on the stream with an EOS poll every 8 steps.
//   RMSNorm        (x * rsqrt(mean(x^2) + eps)) * w, fused into the consuming linear: the mean of squares is a lane-strided sum + the DPP tree
//   linear         weights transposed [K][M]; a workgroup = 64 columns x 16 K-slices over 8 rows staged in LDS; every slice is one ascending
//                  fmaf chain, the slices meet through LDS in the order 0, 1, .. 15
//   q | k | v      one projection; the epilogue rotates q and k in the half-split convention (element i pairs with i + d/2) at the row's own
//                  position and writes k, v into the row's cache slot: caches are [B][kv_heads][cap][d]
//   attention      one workgroup per (row, query head) over the keys 0 .. pos of kv head h / (heads / kv_heads)
//   MLP            gate and up in one pass with silu(g) * u in the epilogue; down and o_proj add the residual in theirs
//   head           the final norm fused in; only the columns first_free_id .. vocab (the bad-word ban makes the others unobservable)
//   scoring        lds_llama_score: ONE causal pass over all B * S rows of given streams through the same kernels (a row's position is all that
//                  tells it from a decode step), then the head over the WHOLE vocabulary -- the low columns from a second packed matrix, the
//                  columns first_free_id .. by the decode's own launch at another column address -- and lm.hip's row statistics and loss
//   beam search    lds_llama_generate_beam: B * K beam rows behind ONE prefill row per item; ll_attn_beam_kernel reads generated keys through the
//                  beams' ancestry table and prompt keys from the item's prefilled cache row; the head over the whole vocabulary as in scoring;
//                  lm.hip's beam step in its per-row form (lm_common.h)
#include "../../include/lds.h"
#include "kernels.h"
#include "host.h"
#include "lm_common.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

namespace lds {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Which (batch row, position) row n of a pass is.  L > 0: the prefill, n = b * L + l at position l.  L == 0: a decode step, row b at position
// plen[b] - 1 + step; a row that has run past the cache (it reached max_length at an earlier step) is not live and stores nothing.
// (A beam decode's step has a row per beam: plen then has one entry per BEAM row, its item's length.)
struct LlRows { const int32_t* plen; int L, step, cap; };
static __device__ __forceinline__ void ll_row(const LlRows& r, int n, int& b, int& pos, bool& live) {
    if (r.L > 0) {
        b = n / r.L; pos = n - b * r.L; live = true;
    } else {
        b = n; pos = r.plen[b] - 1 + r.step;
        live = pos < r.cap;
        pos = live ? pos : r.cap - 1;      // (its table row and token slot only have to exist)
    }
}

// the start of a decode, one workgroup per row: stok[b] = the row's ids, clamped to the vocabulary and shifted by -shift (the token-choice kernels'
// column numbering: phone ids turn negative), PAD (shifted) from plen[b] on -- ids beyond a row's length are never looked at
__global__ void __launch_bounds__(256) ll_init_kernel(const int64_t* __restrict__ ids, int P, const int32_t* __restrict__ plen, int vocab, int shift, int pad_s,
                                                      int cap, int64_t* __restrict__ stok) {
    const int b = blockIdx.x, pl = plen[b];
    for (int l = threadIdx.x; l < cap; l += 256) {
        long long t = pad_s;
        if (l < pl && l < P) {
            t = ids[(long long)b * P + l];
            t = (t < 0) ? 0 : (t >= vocab ? vocab - 1 : t);
            t -= shift;
        }
        stok[(long long)b * cap + l] = t;
    }
}
// the start of a scoring pass, one workgroup per row: the same shifted ids over cap = S slots, len null = S everywhere (no host copy feeds it)
__global__ void __launch_bounds__(256) ll_score_init_kernel(const int64_t* __restrict__ ids, int S, const int32_t* __restrict__ len, int vocab, int shift, int pad_s,
                                                            int64_t* __restrict__ stok) {
    const int b = blockIdx.x, n = len ? len[b] : S;
    for (int l = threadIdx.x; l < S; l += 256) {
        long long t = pad_s;
        if (l < n) {
            t = ids[(long long)b * S + l];
            t = (t < 0) ? 0 : (t >= vocab ? vocab - 1 : t);
            t -= shift;
        }
        stok[(long long)b * S + l] = t;
    }
}
// tokens = stok + shift: the ids of the model's vocabulary again
__global__ void __launch_bounds__(256) ll_finish_kernel(const int64_t* __restrict__ stok, long long n, int shift, int64_t* __restrict__ tokens) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) tokens[i] = stok[i] + shift;
}
// x[n] = embed_tokens[id of row n], ids clamped
__global__ void __launch_bounds__(256) ll_embed_kernel(const float* __restrict__ emb, const int64_t* __restrict__ stok, const LlRows rows, int shift, int vocab,
                                                       int H, float* __restrict__ x) {
    const int n = blockIdx.x;
    int b, pos;
    bool live;
    ll_row(rows, n, b, pos, live);
    long long t = stok[(long long)b * rows.cap + pos] + shift;
    t = (t < 0) ? 0 : (t >= vocab ? vocab - 1 : t);
    for (int c = threadIdx.x; c < H; c += 256) x[(long long)n * H + c] = emb[t * H + c];
}

// ---- Y[n][m] = epi(sum_k rms(X)[n][k] * Wt[k][m]) for a tile of 8 rows per workgroup (lm_linear_dln_kernel's shape: 64 columns x 16 K-slices,
//      the staged rows normalised in LDS when nw != null).  K is arbitrary: slice s walks k in [s * ceil(K / 16), ...) ascending.
//      LL_RESID: + R[n][m] (R may be Y).  LL_SWIGLU: Wt = gate, Wt2 = up, y = silu(g) * u.
//      LL_ROPE: the q | k | v projection.  The first column blocks hold 32 rotation pairs each -- lane c < 32 element i of a head, lane c + 32
//      its partner i + d/2 -- so the partner's value is one cross-lane move away whatever d is; the remaining blocks are v's plain columns. ----
enum { LL_PLAIN = 0, LL_RESID = 1, LL_SWIGLU = 2, LL_ROPE = 3 };
struct LlRope { const float* cs; float* kc; float* vc; int heads, kv_heads, d; LlRows rows; };      // cs [max_pos][d]: cos[d/2] | sin[d/2]
constexpr int kLlCols = 64, kLlSlices = 16;

template <int EPI>
__global__ void __launch_bounds__(1024) ll_linear_kernel(const float* __restrict__ X, int K, const float* __restrict__ nw, float eps, const float* __restrict__ Wt,
                                                        const float* __restrict__ Wt2, int M, const float* R, float* Y, int ldy, int N, const LlRope rope) {
    constexpr int COLS = kLlCols, KS = kLlSlices, NP = (EPI == LL_SWIGLU) ? 2 : 1;
    extern __shared__ __attribute__((aligned(16))) float sm[];      // xs [K][8], part [NP][KS-1][COLS][8], rstd [8]
    float* xs = sm;
    float* part = sm + (size_t)K * 8;
    float* rstd_s = part + (size_t)NP * (KS - 1) * COLS * 8;
    const int tid = threadIdx.x, col = tid % COLS, ks = tid / COLS, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.y * 8;
    // the column this thread owns
    int m;
    bool valid;
    int hq = 0, ri = 0, half = 0, npb = 0;
    if constexpr (EPI == LL_ROPE) {
        const int hd = rope.d >> 1, npairs = (rope.heads + rope.kv_heads) * hd;
        npb = (npairs + 31) / 32;
        if ((int)blockIdx.x < npb) {
            const int p = blockIdx.x * 32 + (col & 31);
            valid = p < npairs;
            hq = p / hd; ri = p - hq * hd; half = col >> 5;
            m = hq * rope.d + ri + half * hd;
        } else {
            const int vcol = (blockIdx.x - npb) * COLS + col;
            valid = vcol < rope.kv_heads * rope.d;
            m = (rope.heads + rope.kv_heads) * rope.d + vcol;
        }
    } else {
        m = blockIdx.x * COLS + col;
        valid = m < M;
    }
    for (int i = tid; i < K * 8; i += 1024) {
        const int k = i >> 3, j = i & 7;
        xs[i] = (n0 + j < N) ? X[(long long)(n0 + j) * K + k] : 0.f;
    }
    __syncthreads();
    if (nw) {      // RMSNorm of the staged rows: wave j owns row j (lane-strided sum of squares, DPP tree), then every thread scales
        if (wave < 8) {
            float ss = 0.f;
            for (int k = lane; k < K; k += 64) { const float v = xs[8 * k + wave]; ss = fmaf(v, v, ss); }
            ss = wave_sum(ss);
            if (lane == 0) rstd_s[wave] = 1.0f / sqrtf(ss / (float)K + eps);
        }
        __syncthreads();
        float rs[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) rs[j] = rstd_s[j];
        for (int k = tid; k < K; k += 1024) {
            const float wk = nw[k];
#pragma unroll
            for (int j = 0; j < 8; ++j) xs[8 * k + j] = (xs[8 * k + j] * rs[j]) * wk;
        }
        __syncthreads();
    }
    float acc[NP][8];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[p][j] = 0.f;
    const int kq = (K + KS - 1) / KS, k0 = ks * kq, k1 = (k0 + kq < K) ? k0 + kq : K;
    if (valid) {
        const float* wp = Wt + m;
        const float* wp2 = (EPI == LL_SWIGLU) ? Wt2 + m : nullptr;
        int k = k0;
        for (; k + 8 <= k1; k += 8) {
            float w[NP][8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                w[0][u] = wp[(long long)(k + u) * M];
                if constexpr (EPI == LL_SWIGLU) w[NP - 1][u] = wp2[(long long)(k + u) * M];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(xs + 8 * (k + u)), b = *reinterpret_cast<const f32x4*>(xs + 8 * (k + u) + 4);
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    acc[p][0] = fmaf(w[p][u], a[0], acc[p][0]); acc[p][1] = fmaf(w[p][u], a[1], acc[p][1]);
                    acc[p][2] = fmaf(w[p][u], a[2], acc[p][2]); acc[p][3] = fmaf(w[p][u], a[3], acc[p][3]);
                    acc[p][4] = fmaf(w[p][u], b[0], acc[p][4]); acc[p][5] = fmaf(w[p][u], b[1], acc[p][5]);
                    acc[p][6] = fmaf(w[p][u], b[2], acc[p][6]); acc[p][7] = fmaf(w[p][u], b[3], acc[p][7]);
                }
            }
        }
        for (; k < k1; ++k) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(xs + 8 * k), b = *reinterpret_cast<const f32x4*>(xs + 8 * k + 4);
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const float w = (p == 0) ? wp[(long long)k * M] : wp2[(long long)k * M];
                acc[p][0] = fmaf(w, a[0], acc[p][0]); acc[p][1] = fmaf(w, a[1], acc[p][1]); acc[p][2] = fmaf(w, a[2], acc[p][2]); acc[p][3] = fmaf(w, a[3], acc[p][3]);
                acc[p][4] = fmaf(w, b[0], acc[p][4]); acc[p][5] = fmaf(w, b[1], acc[p][5]); acc[p][6] = fmaf(w, b[2], acc[p][6]); acc[p][7] = fmaf(w, b[3], acc[p][7]);
            }
        }
    }
    if (ks > 0) {
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int j = 0; j < 8; ++j) part[(((size_t)p * (KS - 1) + ks - 1) * COLS + col) * 8 + j] = acc[p][j];
    }
    __syncthreads();
    if (ks > 0) return;      // slice 0 is exactly wave 0
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll 1
        for (int q = 0; q < KS - 1; ++q) {
            const float* pp = part + (((size_t)p * (KS - 1) + q) * COLS + col) * 8;
            const f32x4 a = *reinterpret_cast<const f32x4*>(pp), b = *reinterpret_cast<const f32x4*>(pp + 4);
            acc[p][0] += a[0]; acc[p][1] += a[1]; acc[p][2] += a[2]; acc[p][3] += a[3];
            acc[p][4] += b[0]; acc[p][5] += b[1]; acc[p][6] += b[2]; acc[p][7] += b[3];
        }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int n = n0 + j;
        const bool ok = valid && n < N;
        float y = acc[0][j];
        if constexpr (EPI == LL_SWIGLU) y = (y / (1.0f + expf(-y))) * acc[NP - 1][j];
        if constexpr (EPI == LL_ROPE) {
            int b, pos;
            bool live;
            ll_row(rope.rows, n < N ? n : n0, b, pos, live);
            const float other = __shfl_xor(y, 32, 64);      // (all of wave 0 takes part; only the pair blocks use it)
            const int d = rope.d, hd = d >> 1;
            if ((int)blockIdx.x < npb) {
                const float cs = valid ? rope.cs[(long long)pos * d + ri] : 0.f, sn = valid ? rope.cs[(long long)pos * d + hd + ri] : 0.f;
                // HF apply_rotary_pos_emb: x * cos + rotate_half(x) * sin, rotate_half(x) = [-x2 | x1]
                const float rot = half ? y * cs + other * sn : y * cs - other * sn;
                if (ok && live) {
                    if (hq < rope.heads) Y[(long long)n * ldy + m] = rot;
                    else rope.kc[(((long long)b * rope.kv_heads + (hq - rope.heads)) * rope.rows.cap + pos) * d + ri + half * hd] = rot;
                }
            } else if (ok && live) {
                const int vcol = m - (rope.heads + rope.kv_heads) * d, hv = vcol / d;
                rope.vc[(((long long)b * rope.kv_heads + hv) * rope.rows.cap + pos) * d + (vcol - hv * d)] = y;
            }
        } else {
            if constexpr (EPI == LL_RESID) { if (ok) y += R[(long long)n * M + m]; }
            if (ok) Y[(long long)n * ldy + m] = y;
        }
    }
}

// ---- attention of one (row, query head) per workgroup: softmax(q K^T / sqrt(d)) V over the row's keys 0 .. pos, which its cache holds -- the
//      causal context, for a prefill row and for a decode step alike, so the arithmetic depends on the position alone.  lm_attn_body's scheme
//      for head dims up to 256: the four waves take alternate 64-key blocks; phase 1 has a key per lane, phase 2 the channels lane, lane + 64, ..
//      over the wave's keys in ascending order; the waves' (max, sum, partial output) meet through LDS in the order 0 .. 3.
//      q, out [N][heads * d]; query head h reads kv head h / (heads / kv_heads). ----
//      ll_attn_beam_kernel (a beam decode's step; ba.K beams per item) is the same arithmetic in the same order, written out a second time so
//      that the plain decode runs the very kernel it ran before beams existed; there key p lives in cache
//      row  item * K  for p < plen[item] (the ONE row the item's prefill filled: no look-up),  n itself for p = pos,  tab[n][p - plen[item]]
//      otherwise -- the beam's ancestry over generated positions (lm_beam_step_kernel's table).  The source row of every key is kept beside its score
//      in LDS for the value pass.  ended[item] != 0: the item's search is over, its rows give zeros like a row past its end. ----
constexpr int kLlMaxHeadDim = 256;
struct LlBeamAttn { const int* tab; const int* ended; int tcap, K; };
__global__ void __launch_bounds__(256) ll_attn_kernel(const float* __restrict__ q, const float* __restrict__ kc, const float* __restrict__ vc, const LlRows rows,
                                                      int heads, int kv_heads, int d, int Lkp, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float sa[];      // qs [256], sc [Lkp], mrg [4][2 + 256]
    float* qs = sa;
    float* sc = sa + kLlMaxHeadDim;
    float* mrg = sc + Lkp;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.x % heads, n = blockIdx.x / heads;
    int b, pos;
    bool live;
    ll_row(rows, n, b, pos, live);
    const int QD = heads * d, kvh = h / (heads / kv_heads);
    if (!live) {      // (uniform over the workgroup) a row past its end: zeros, so that what follows in its row stays finite and depends on nothing stale
        if (tid < d) out[(long long)n * QD + h * d + tid] = 0.f;
        return;
    }
    int Lk = pos + 1;
    Lk = Lk < Lkp ? Lk : Lkp;
    if (tid < d) qs[tid] = q[(long long)n * QD + h * d + tid];
    __syncthreads();
    const float* kb = kc + ((long long)b * kv_heads + kvh) * rows.cap * d;
    const float* vb = vc + ((long long)b * kv_heads + kvh) * rows.cap * d;
    const float scale = 1.0f / sqrtf((float)d);
    float mx = -INFINITY;
    for (int k0 = wave * 64; k0 < Lk; k0 += 256) {
        const int key = k0 + lane;
        float dot = -INFINITY;
        if (key < Lk) {
            dot = 0.f;
            const f32x4* kr = reinterpret_cast<const f32x4*>(kb + (long long)key * d);
            const f32x4* q4 = reinterpret_cast<const f32x4*>(qs);
            for (int e4 = 0; e4 < (d >> 2); e4 += 4) {      // d is a multiple of 16
                f32x4 kv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) kv[u] = kr[e4 + u];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const f32x4 qv = q4[e4 + u];
                    dot = fmaf(qv[0], kv[u][0], dot); dot = fmaf(qv[1], kv[u][1], dot); dot = fmaf(qv[2], kv[u][2], dot); dot = fmaf(qv[3], kv[u][3], dot);
                }
            }
            dot *= scale;
            sc[key] = dot;
        }
        mx = fmaxf(mx, dot);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int k0 = wave * 64; k0 < Lk; k0 += 256) {
        const int key = k0 + lane;
        float p = 0.f;
        if (key < Lk) { p = expf(sc[key] - mx); sc[key] = p; }
        sum += p;
    }
    sum = wave_sum(sum);
    __syncthreads();      // the probabilities are in LDS
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = wave * 64; k0 < Lk; k0 += 256) {
        const int kend = (k0 + 64 < Lk) ? k0 + 64 : Lk;
        for (int key = k0; key < kend; ++key) {
            const float p = sc[key];
            const float* vr = vb + (long long)key * d;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (lane + 64 * i < d) acc[i] = fmaf(p, vr[lane + 64 * i], acc[i]);
        }
    }
    float* mw = mrg + wave * (2 + kLlMaxHeadDim);
    if (lane == 0) { mw[0] = mx; mw[1] = sum; }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (lane + 64 * i < d) mw[2 + lane + 64 * i] = acc[i];
    __syncthreads();
    if (tid < d) {
        constexpr int S = 2 + kLlMaxHeadDim;
        const float m = fmaxf(fmaxf(mrg[0], mrg[S]), fmaxf(mrg[2 * S], mrg[3 * S]));
        float tot = 0.f, o = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float f = (mrg[w * S] > -INFINITY) ? expf(mrg[w * S] - m) : 0.f;
            tot += mrg[w * S + 1] * f;
            o += mrg[w * S + 2 + tid] * f;
        }
        out[(long long)n * QD + h * d + tid] = o / tot;
    }
}
// the beam decode's sibling: ll_attn_kernel line for line, but for where a key's row comes from (above); a change to either belongs in both --
// tests/test_gpu_llama_beam.py holds the two bit for bit
__global__ void __launch_bounds__(256) ll_attn_beam_kernel(const float* __restrict__ q, const float* __restrict__ kc, const float* __restrict__ vc, const LlRows rows,
                                                           int heads, int kv_heads, int d, int Lkp, float* __restrict__ out, const LlBeamAttn ba) {
    extern __shared__ __attribute__((aligned(16))) float sa[];      // qs [256], sc [Lkp], mrg [4][2 + 256], src [Lkp]
    float* qs = sa;
    float* sc = sa + kLlMaxHeadDim;
    float* mrg = sc + Lkp;
    int* src = reinterpret_cast<int*>(mrg + 4 * (2 + kLlMaxHeadDim));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.x % heads, n = blockIdx.x / heads;
    int b, pos;
    bool live;
    ll_row(rows, n, b, pos, live);
    const int QD = heads * d, kvh = h / (heads / kv_heads);
    const int item = n / ba.K, row0 = item * ba.K, pl = rows.plen[n];
    if (ba.ended && ba.ended[item]) live = false;
    if (!live) {      // (uniform over the workgroup) a row past its end: zeros, so that what follows in its row stays finite and depends on nothing stale
        if (tid < d) out[(long long)n * QD + h * d + tid] = 0.f;
        return;
    }
    int Lk = pos + 1;
    Lk = Lk < Lkp ? Lk : Lkp;
    if (tid < d) qs[tid] = q[(long long)n * QD + h * d + tid];
    __syncthreads();
    const float scale = 1.0f / sqrtf((float)d);
    float mx = -INFINITY;
    for (int k0 = wave * 64; k0 < Lk; k0 += 256) {
        const int key = k0 + lane;
        float dot = -INFINITY;
        if (key < Lk) {
            dot = 0.f;
            int r = row0;
            if (key >= pl) {
                r = (key == pos) ? n : ba.tab[(long long)n * ba.tcap + key - pl];
                r = r < row0 ? row0 : (r >= row0 + ba.K ? row0 + ba.K - 1 : r);      // (a row of the item's, whatever the table holds)
            }
            src[key] = r;
            const f32x4* kr = reinterpret_cast<const f32x4*>(kc + (((long long)r * kv_heads + kvh) * rows.cap + key) * d);
            const f32x4* q4 = reinterpret_cast<const f32x4*>(qs);
            for (int e4 = 0; e4 < (d >> 2); e4 += 4) {      // d is a multiple of 16
                f32x4 kv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) kv[u] = kr[e4 + u];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const f32x4 qv = q4[e4 + u];
                    dot = fmaf(qv[0], kv[u][0], dot); dot = fmaf(qv[1], kv[u][1], dot); dot = fmaf(qv[2], kv[u][2], dot); dot = fmaf(qv[3], kv[u][3], dot);
                }
            }
            dot *= scale;
            sc[key] = dot;
        }
        mx = fmaxf(mx, dot);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int k0 = wave * 64; k0 < Lk; k0 += 256) {
        const int key = k0 + lane;
        float p = 0.f;
        if (key < Lk) { p = expf(sc[key] - mx); sc[key] = p; }
        sum += p;
    }
    sum = wave_sum(sum);
    __syncthreads();      // the probabilities are in LDS
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = wave * 64; k0 < Lk; k0 += 256) {
        const int kend = (k0 + 64 < Lk) ? k0 + 64 : Lk;
        for (int key = k0; key < kend; ++key) {
            const float p = sc[key];
            const float* vr = vc + (((long long)src[key] * kv_heads + kvh) * rows.cap + key) * d;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (lane + 64 * i < d) acc[i] = fmaf(p, vr[lane + 64 * i], acc[i]);
        }
    }
    float* mw = mrg + wave * (2 + kLlMaxHeadDim);
    if (lane == 0) { mw[0] = mx; mw[1] = sum; }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (lane + 64 * i < d) mw[2 + lane + 64 * i] = acc[i];
    __syncthreads();
    if (tid < d) {
        constexpr int S = 2 + kLlMaxHeadDim;
        const float m = fmaxf(fmaxf(mrg[0], mrg[S]), fmaxf(mrg[2 * S], mrg[3 * S]));
        float tot = 0.f, o = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float f = (mrg[w * S] > -INFINITY) ? expf(mrg[w * S] - m) : 0.f;
            tot += mrg[w * S + 1] * f;
            o += mrg[w * S + 2 + tid] * f;
        }
        out[(long long)n * QD + h * d + tid] = o / tot;
    }
}

// the start of a beam decode, one workgroup per beam row r of item r / K: the item's prompt ids (clamped, not shifted), PAD from plen on, into both
// buffers of the running sequences and of the finished hypotheses; HF's initial scores (running 0, -1e9, ..; finished -1e9) and flags
__global__ void __launch_bounds__(256) ll_beam_init_kernel(const int64_t* __restrict__ ids, int P, const int32_t* __restrict__ plen, int vocab, int pad, int cap, int K,
                                                           int64_t* __restrict__ r0, int64_t* __restrict__ r1, int64_t* __restrict__ f0, int64_t* __restrict__ f1,
                                                           float* __restrict__ rscore, float* __restrict__ fscore, int* __restrict__ ffin, int* __restrict__ flen,
                                                           int* __restrict__ unsat, int* __restrict__ ended) {
    const int r = blockIdx.x, item = r / K, pl = plen[item];
    for (int l = threadIdx.x; l < cap; l += 256) {
        long long t = pad;
        if (l < pl && l < P) {
            t = ids[(long long)item * P + l];
            t = (t < 0) ? 0 : (t >= vocab ? vocab - 1 : t);
        }
        const long long a = (long long)r * cap + l;
        r0[a] = t; r1[a] = t; f0[a] = t; f1[a] = t;
    }
    if (threadIdx.x == 0) {
        const bool first = r == item * K;
        rscore[r] = first ? 0.f : -1.0e9f; fscore[r] = -1.0e9f; ffin[r] = 0; flen[r] = 0;
        if (first) { unsat[item] = 1; ended[item] = 0; }
    }
}
// after a beam decode's prefill, which filled cache rows 0 .. B - 1 like any prefill: item b's positions 0 .. Pq - 1 move to cache row b * K, the
// first of its K beam rows.  A thread owns ONE (kv head, position, channel) of a cache (blockIdx.y: keys, values) and walks the items downwards:
// b * K > b, so no row is overwritten before it has been moved, and no two threads touch the same float.
__global__ void __launch_bounds__(256) ll_beam_spread_kernel(float* __restrict__ kc, float* __restrict__ vc, int B, int K, int kv_heads, int cap, int d, int Pq) {
    float* c = blockIdx.y ? vc : kc;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x, per = (long long)Pq * d;
    if (e >= kv_heads * per) return;
    const long long off = (e / per) * cap * d + e % per, row = (long long)kv_heads * cap * d;
    for (int b = B - 1; b >= 1; --b) c[(long long)b * K * row + off] = c[b * row + off];
}
// the end of a beam decode, one workgroup per item: its best finished hypothesis (slot 0) up to its end, PAD after it; rowlen[b] = its length
__global__ void __launch_bounds__(256) ll_beam_finish_kernel(const int64_t* __restrict__ fseq, const int* __restrict__ flen, const int32_t* __restrict__ plen, int K,
                                                             int cap, int pad, int64_t* __restrict__ tokens, int* __restrict__ rowlen) {
    const int b = blockIdx.x;
    int n = plen[b] + flen[b * K];
    n = n < cap ? n : cap;
    for (int l = threadIdx.x; l < cap; l += 256) tokens[(long long)b * cap + l] = (l < n) ? fseq[(long long)b * K * cap + l] : (int64_t)pad;
    if (threadIdx.x == 0) rowlen[b] = n;
}

}  // namespace lds

using namespace lds;

// ================================================================================================
// host side
// ================================================================================================
struct LlLayer { float *nw_attn = nullptr, *wqkv = nullptr, *wo = nullptr, *nw_mlp = nullptr, *wgate = nullptr, *wup = nullptr, *wdown = nullptr; };
struct lds_llama {
    lds_llama_cfg cfg;
    Owner own;
    float *embed = nullptr, *cs = nullptr, *nw_final = nullptr, *head = nullptr, *head_lo = nullptr;
    std::vector<LlLayer> layers;
};

namespace {
constexpr int kLlMaxBatch = 64;          // the rows' final lengths live in 64 ints behind the step flags
constexpr int kLlMaxLength = 15000;      // the attention stages one score per key in LDS
// reference layout W [M][K] (rows r0 .. r0 + Mper of each) -> transposed [K][M], several matrices concatenated along M
float* ll_linear_up(WeightLoader& T, const std::vector<std::pair<std::string, int>>& mats, int K, int r0 = 0, int rows_all = -1) {
    int M = 0;
    for (auto& s : mats) M += s.second;
    std::vector<float> wt((size_t)K * M);
    int c0 = 0;
    for (auto& s : mats) {
        const int full = rows_all < 0 ? s.second : rows_all;
        const float* w = T.get(s.first, (int64_t)full * K);
        if (!w) return nullptr;
        for (int m = 0; m < s.second; ++m)
            for (int k = 0; k < K; ++k) wt[(size_t)k * M + c0 + m] = w[(size_t)(r0 + m) * K + k];
        c0 += s.second;
    }
    return T.o.upload(wt);
}
int ll_check_cfg(const lds_llama_cfg& c) {
    if (c.hidden < 1 || c.hidden > 2048 || c.inter < 1 || c.inter > 3840 || c.layers < 1 || c.max_pos < 2)
        return set_error(LDS_EINVAL, "unsupported Llama shape (1 <= hidden <= 2048, 1 <= intermediate size <= 3840, layers >= 1, max_position_embeddings >= 2)");
    if (c.head_dim < 16 || c.head_dim > kLlMaxHeadDim || c.head_dim % 16) return set_error(LDS_EINVAL, "head_dim %d must be a multiple of 16 in 16 .. %d", c.head_dim, kLlMaxHeadDim);
    if (c.heads < 1 || c.kv_heads < 1 || c.heads % c.kv_heads) return set_error(LDS_EINVAL, "num_key_value_heads %d must divide num_attention_heads %d", c.kv_heads, c.heads);
    if ((long long)c.heads * c.head_dim > 3840) return set_error(LDS_EINVAL, "heads * head_dim = %lld too wide (<= 3840)", (long long)c.heads * c.head_dim);
    if (c.first_free_id < 0 || c.vocab <= c.first_free_id || c.vocab - c.first_free_id > kLmMaxChoiceVocab)
        return set_error(LDS_EINVAL, "the token choice takes 1 .. %d columns (vocab %d - first_free_id %d)", kLmMaxChoiceVocab, c.vocab, c.first_free_id);
    for (int id : {c.bos, c.eos, c.pad})
        if (id < c.first_free_id || id >= c.vocab) return set_error(LDS_EINVAL, "bos / eos / pad id %d outside [first_free_id, vocab)", id);
    if (!(c.eps > 0.f) || !(c.rope_theta > 0.f)) return set_error(LDS_EINVAL, "rms_norm_eps and rope_theta must be positive");
    return LDS_OK;
}
}  // namespace

extern "C" int lds_llama_create(const lds_llama_cfg* cfg, int n, const char* const* names, const float* const* ptrs, const int64_t* numel, lds_llama** out) {
    if (!cfg || !names || !ptrs || !numel || !out || n < 0) return set_error(LDS_EINVAL, "null argument");
    if (int r = ll_check_cfg(*cfg)) return r;
    const lds_llama_cfg& c = *cfg;
    lds_llama* L = new lds_llama();
    L->cfg = c;
    WeightLoader T(L->own, n, names, ptrs, numel);
    const int H = c.hidden, d = c.head_dim, QD = c.heads * d, KD = c.kv_heads * d, hd = d / 2;
    const std::string p = "llama.model.";
    bool ok = (L->embed = T.vec(p + "embed_tokens.weight", (int64_t)c.vocab * H)) != nullptr;
    for (int i = 0; i < c.layers && ok; ++i) {
        LlLayer y;
        const std::string q = p + "layers." + std::to_string(i) + ".";
        y.nw_attn = T.vec(q + "input_layernorm.weight", H);
        y.wqkv = ll_linear_up(T, {{q + "self_attn.q_proj.weight", QD}, {q + "self_attn.k_proj.weight", KD}, {q + "self_attn.v_proj.weight", KD}}, H);
        y.wo = ll_linear_up(T, {{q + "self_attn.o_proj.weight", H}}, QD);
        y.nw_mlp = T.vec(q + "post_attention_layernorm.weight", H);
        y.wgate = ll_linear_up(T, {{q + "mlp.gate_proj.weight", c.inter}}, H);
        y.wup = ll_linear_up(T, {{q + "mlp.up_proj.weight", c.inter}}, H);
        y.wdown = ll_linear_up(T, {{q + "mlp.down_proj.weight", H}}, c.inter);
        ok = y.nw_attn && y.wqkv && y.wo && y.nw_mlp && y.wgate && y.wup && y.wdown;
        L->layers.push_back(y);
    }
    ok = ok && (L->nw_final = T.vec(p + "norm.weight", H)) != nullptr;
    // the head's observable columns only: rows first_free_id .. vocab of lm_head.weight
    ok = ok && (L->head = ll_linear_up(T, {{"llama.lm_head.weight", c.vocab - c.first_free_id}}, H, c.first_free_id, c.vocab)) != nullptr;
    // and the columns below, which only scoring looks at (HF's log_softmax runs over the whole vocabulary): rows 0 .. first_free_id, a matrix of its own
    if (c.first_free_id > 0) ok = ok && (L->head_lo = ll_linear_up(T, {{"llama.lm_head.weight", c.first_free_id}}, H, 0, c.vocab)) != nullptr;
    if (ok) {
        // HF LlamaRotaryEmbedding (default rope): angle = fp32(position) * inv_freq as an fp32 product, cos / sin of THAT angle.  inv_freq =
        // theta^(-2i/d) in fp32; a caller that has HF's own numbers hands them in (torch's vectorised pow is not correctly rounded, and one ulp
        // of inv_freq is 6e-5 rad at position 1000)
        std::vector<float> inv(hd), cs((size_t)c.max_pos * d);
        if (const float* given = T.opt(p + "rotary_emb.inv_freq", hd)) memcpy(inv.data(), given, sizeof(float) * hd);
        else for (int i = 0; i < hd; ++i) inv[i] = 1.0f / powf(c.rope_theta, (float)(2 * i) / (float)d);
        for (int pos = 0; pos < c.max_pos; ++pos)
            for (int i = 0; i < hd; ++i) {
                const float ang = (float)pos * inv[i];
                cs[(size_t)pos * d + i] = (float)cos((double)ang);
                cs[(size_t)pos * d + hd + i] = (float)sin((double)ang);
            }
        ok = (L->cs = T.o.upload(cs)) != nullptr;
    }
    return T.finish(ok, "Llama", L, out, "Llama weight tensor");
}
extern "C" void lds_llama_destroy(lds_llama* L) { delete L; }

namespace {
struct LlWs { float *x, *q, *ctx, *ff, *logits; int* flags; int64_t* stok; int32_t* plen; std::vector<float*> kc, vc; };
// rows of a pass: B * (P - 1) for the prefill (the prompts' positions but the last), B for a decode step
void ll_plan(const lds_llama* L, Arena& A, int B, int P, int cap, LlWs& w) {
    const lds_llama_cfg& c = L->cfg;
    const size_t N = (size_t)B * (P > 2 ? P - 1 : 1), QD = (size_t)c.heads * c.head_dim, KD = (size_t)c.kv_heads * c.head_dim;
    w.x = A.f(N * c.hidden); w.q = A.f(N * QD); w.ctx = A.f(N * QD); w.ff = A.f(N * c.inter);
    w.logits = A.f((size_t)B * (c.vocab - c.first_free_id));
    w.flags = (int*)A.f((size_t)B + cap + kLlMaxBatch);
    w.stok = (int64_t*)A.f(2 * (size_t)B * cap);
    w.plen = (int32_t*)A.f((size_t)B);
    w.kc.clear(); w.vc.clear();
    for (int i = 0; i < c.layers; ++i) { w.kc.push_back(A.f((size_t)B * KD * cap)); w.vc.push_back(A.f((size_t)B * KD * cap)); }
}
// the shape checks, which need no model
int ll_check_shape(int B, int P, int max_length) {
    if (B <= 0 || P < 1 || max_length < 2) return set_error(LDS_EINVAL, "bad argument");
    if (B > kLlMaxBatch) return set_error(LDS_EINVAL, "a Llama decode takes at most %d rows, got %d", kLlMaxBatch, B);
    if (P > kLlMaxLength || max_length > kLlMaxLength) return set_error(LDS_EINVAL, "prompt width %d / max_length %d too long (<= %d)", P, max_length, kLlMaxLength);
    return LDS_OK;
}
// the rows' prompt lengths (host): each inside 1 .. P and below max_length -> the longest and the shortest
int ll_check_lens(const int32_t* in_len, int B, int P, int max_length, int& Pmax, int& Pmin) {
    Pmax = 0; Pmin = P;
    for (int b = 0; b < B; ++b) {
        const int pl = in_len ? in_len[b] : P;
        if (pl < 1 || pl > P) return set_error(LDS_EINVAL, "in_len[%d] = %d out of range (1 .. P = %d)", b, pl, P);
        if (pl >= max_length) return set_error(LDS_EINVAL, "in_len[%d] = %d leaves no room below max_length = %d (the total length, prompt included)", b, pl, max_length);
        Pmax = pl > Pmax ? pl : Pmax;
        Pmin = pl < Pmin ? pl : Pmin;
    }
    return LDS_OK;
}

template <int EPI>
hipError_t ll_linear(const float* X, int K, const float* nw, float eps, const float* Wt, const float* Wt2, int M, const float* R, float* Y, int ldy, int N,
                     hipStream_t st, const LlRope* rope = nullptr) {
    auto kern = ll_linear_kernel<EPI>;
    static std::atomic<unsigned long long> attr_done{0};
    hipError_t e = ensure_max_dynamic_lds(reinterpret_cast<const void*>(kern), attr_done);
    if (e != hipSuccess) return e;
    const size_t lds = ((size_t)K * 8 + (size_t)(EPI == LL_SWIGLU ? 2 : 1) * (kLlSlices - 1) * kLlCols * 8 + 8) * sizeof(float);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    unsigned gx = (M + kLlCols - 1) / kLlCols;
    LlRope ro{};
    if (EPI == LL_ROPE) {
        if (!rope) return hipErrorInvalidValue;
        ro = *rope;
        gx = ((ro.heads + ro.kv_heads) * (ro.d / 2) + 31) / 32 + (ro.kv_heads * ro.d + kLlCols - 1) / kLlCols;
    }
    hipLaunchKernelGGL(kern, dim3(gx, (N + 7) / 8), dim3(1024), lds, st, X, K, nw, eps, Wt, Wt2, M, R, Y, ldy, N, ro);
    return hipGetLastError();
}

// the decoder layers over N rows (a prefill pass or a decode step, told apart by `rows` alone); Lk_max = the most keys any row sees
int ll_layers(const lds_llama* L, const LlWs& w, int N, const LlRows& rows, int Lk_max, hipStream_t st, const LlBeamAttn* beam = nullptr) {
    const lds_llama_cfg& c = L->cfg;
    const int H = c.hidden, d = c.head_dim, QD = c.heads * d, KD = c.kv_heads * d, Lkp = (Lk_max + 63) & ~63;
    const size_t attn_lds = (size_t)(kLlMaxHeadDim + Lkp + 4 * (2 + kLlMaxHeadDim)) * sizeof(float);
    for (int i = 0; i < c.layers; ++i) {
        const LlLayer& y = L->layers[i];
        const LlRope rope{L->cs, w.kc[i], w.vc[i], c.heads, c.kv_heads, d, rows};
        HIP_TRY(ll_linear<LL_ROPE>(w.x, H, y.nw_attn, c.eps, y.wqkv, nullptr, QD + 2 * KD, nullptr, w.q, QD, N, st, &rope));
        if (beam)      // (one more int per key in LDS: the key's source row)
            hipLaunchKernelGGL(ll_attn_beam_kernel, dim3((unsigned)(N * c.heads)), dim3(256), attn_lds + (size_t)Lkp * sizeof(int), st, (const float*)w.q,
                               (const float*)w.kc[i], (const float*)w.vc[i], rows, c.heads, c.kv_heads, d, Lkp, w.ctx, *beam);
        else
            hipLaunchKernelGGL(ll_attn_kernel, dim3((unsigned)(N * c.heads)), dim3(256), attn_lds, st, (const float*)w.q, (const float*)w.kc[i], (const float*)w.vc[i], rows,
                               c.heads, c.kv_heads, d, Lkp, w.ctx);
        HIP_TRY(hipGetLastError());
        HIP_TRY(ll_linear<LL_RESID>(w.ctx, QD, nullptr, c.eps, y.wo, nullptr, H, w.x, w.x, H, N, st));
        HIP_TRY(ll_linear<LL_SWIGLU>(w.x, H, y.nw_mlp, c.eps, y.wgate, y.wup, c.inter, nullptr, w.ff, c.inter, N, st));
        HIP_TRY(ll_linear<LL_RESID>(w.ff, c.inter, nullptr, c.eps, y.wdown, nullptr, H, w.x, w.x, H, N, st));
    }
    return LDS_OK;
}
}  // namespace

extern "C" int lds_llama_workspace_bytes(const lds_llama* L, int B, int P, int max_length, size_t* out) {
    if (int r = ll_check_shape(B, P, max_length)) return r;
    if (!L || !out) return set_error(LDS_EINVAL, "bad argument");
    Arena A(nullptr, 0);
    LlWs w;
    ll_plan(L, A, B, P, max_length, w);
    *out = A.used;
    return LDS_OK;
}

extern "C" int lds_llama_generate(lds_llama* L, const int64_t* input_ids, const int32_t* in_len, int B, int P, int max_length, const lds_lm_decode_opts* opts,
                                  const float* uniforms, int64_t* tokens, float* logits_out, int* n_tokens_host, void* ws, size_t ws_bytes, void* stream) {
    if (!opts) return set_error(LDS_EINVAL, "null options");
    const lds_lm_decode_opts o = *opts;
    if (int r = lm_check_opts(o, logits_out)) return r;
    if (o.num_beams != 1) return set_error(LDS_EINVAL, "lds_llama_generate takes num_beams 1; beam search over the whole vocabulary is lds_llama_generate_beam");
    if (int r = ll_check_shape(B, P, max_length)) return r;
    int Pmax = 0, Pmin = P;
    if (int r = ll_check_lens(in_len, B, P, max_length, Pmax, Pmin)) return r;
    if (!L || !input_ids || !tokens || !n_tokens_host || !ws) return set_error(LDS_EINVAL, "bad argument");
    const lds_llama_cfg& c = L->cfg;
    const int H = c.hidden, V = c.vocab - c.first_free_id, shift = c.first_free_id;
    if (o.do_sample && (!uniforms || o.top_k < 0 || o.top_k > kLmMaxTopK || o.top_k > V || !(o.top_p > 0.f) || !(o.temperature > 0.f)))
        return set_error(LDS_EINVAL, "sampling needs uniforms, 0 <= top_k <= %d (0 = no top-k filter), top_p > 0, temperature > 0", kLmMaxTopK);
    if (max_length > c.max_pos) return set_error(LDS_EINVAL, "max_length %d exceeds max_position_embeddings %d", max_length, c.max_pos);
    hipStream_t st = (hipStream_t)stream;
    Arena A(ws, ws_bytes);
    LlWs w;
    ll_plan(L, A, B, P, max_length, w);
    if (!A.ok) return set_error(LDS_ENOMEM, "Llama workspace too small: need %zu bytes", A.used);
    int* unfinished = w.flags;                       // [B]
    int* any_unf = w.flags + B;                      // [max_length]: 1 when a row is still running after global step s
    int* rowlen = w.flags + B + max_length;          // [B <= 64]: every row's final length, prompt included
    {
        std::vector<int> init(B + max_length + kLlMaxBatch, 0), pl(B);
        for (int b = 0; b < B; ++b) { init[b] = 1; init[B + max_length + b] = max_length; pl[b] = in_len ? in_len[b] : P; }
        HIP_TRY(hipMemcpyAsync(unfinished, init.data(), sizeof(int) * init.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(w.plen, pl.data(), sizeof(int) * B, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));      // the host staging vectors go out of scope
    }
    const int32_t* plen = w.plen;
    const int pad_s = c.pad - shift, eos_s = c.eos - shift;
    hipLaunchKernelGGL(ll_init_kernel, dim3(B), dim3(256), 0, st, input_ids, P, plen, c.vocab, shift, pad_s, max_length, w.stok);
    HIP_TRY(hipGetLastError());
    // Prefill: the positions 0 .. Pq - 1 (Pq = the longest prompt - 1) of every row in one causal pass that fills the decode's caches; the head is
    // skipped.  A shorter row's slots in_len[b] - 1 .. Pq - 1 are filled from PAD; no query ever sees them: step s of row b first overwrites slot
    // in_len[b] - 1 + s with the row's real token and then reads the slots 0 .. in_len[b] - 1 + s.  The same covers the workspace's contents on entry.
    const int Pq = Pmax - 1;
    if (Pq > 0) {
        if ((long long)B * Pq > 8 * 65535LL) return set_error(LDS_EINVAL, "B * P too large for the prefill (<= 524280)");
        const LlRows rows{plen, Pq, 0, max_length};
        hipLaunchKernelGGL(ll_embed_kernel, dim3(B * Pq), dim3(256), 0, st, (const float*)L->embed, (const int64_t*)w.stok, rows, shift, c.vocab, H, w.x);
        HIP_TRY(hipGetLastError());
        if (int r = ll_layers(L, w, B * Pq, rows, Pq, st)) return r;
    }
    const float inv_temp = o.do_sample ? 1.0f / o.temperature : 1.0f;
    const int n_steps = max_length - Pmin;      // the shortest row writes its last slot at step n_steps - 1
    std::vector<int> host_flags(n_steps, 0);
    int checked = 0;
    for (int step = 0; step < n_steps; ++step) {
        const LlRows rows{plen, 0, step, max_length};
        hipLaunchKernelGGL(ll_embed_kernel, dim3(B), dim3(256), 0, st, (const float*)L->embed, (const int64_t*)w.stok, rows, shift, c.vocab, H, w.x);
        HIP_TRY(hipGetLastError());
        const int Lk_max = (Pmax + step < max_length) ? Pmax + step : max_length;
        if (int r = ll_layers(L, w, B, rows, Lk_max, st)) return r;
        float* lg = logits_out ? logits_out + (size_t)step * B * V : w.logits;
        HIP_TRY(ll_linear<LL_PLAIN>(w.x, H, L->nw_final, c.eps, L->head, nullptr, V, nullptr, lg, V, B, st));
        HIP_TRY(lm_launch_choice_rows(o, B, V, lg, inv_temp, o.do_sample ? uniforms + (size_t)step * B : nullptr, w.stok, max_length, step, unfinished, eos_s, pad_s,
                                     any_unf, nullptr, nullptr, nullptr, nullptr, c.eps, H, nullptr, plen, rowlen, st));
        if ((step & 7) == 7 || step + 1 == n_steps) {      // the EOS poll; a row that reached max_length counts as finished
            HIP_TRY(hipMemcpyAsync(host_flags.data() + checked, any_unf + checked, sizeof(int) * (step + 1 - checked), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            bool done = false;
            for (int s = checked; s <= step && !done; ++s) done = host_flags[s] == 0;
            checked = step + 1;
            if (done) break;
        }
    }
    const long long total = (long long)B * max_length;
    hipLaunchKernelGGL(ll_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const int64_t*)w.stok, total, shift, tokens);
    HIP_TRY(hipGetLastError());
    std::vector<int> len(B, 0);
    HIP_TRY(hipMemcpyAsync(len.data(), rowlen, sizeof(int) * B, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int n_tokens = 0;
    for (int b = 0; b < B; ++b) n_tokens = len[b] > n_tokens ? len[b] : n_tokens;
    *n_tokens_host = n_tokens;
    return LDS_OK;
}

// ---- teacher-forced scoring: the decoder layers over all B * S rows in one causal pass (LlRows with L = S: row n = b * S + l at position l, its
//      keys the slots 0 .. l of a cache of S slots), then the head over row chunks of kLlScoreChunk rows through one reused buffer (or straight
//      into logits_out), each chunk followed by its row statistics.  One layer's cache at a time: layer i's keys are dead once its rows are done. ----
namespace {
constexpr int kLlScoreChunk = 256;
struct LlScoreWs { LlWs w; float* chunk; double* psum; int32_t* pcnt; };
void ll_score_plan(const lds_llama* L, Arena& A, int B, int S, LlScoreWs& s) {
    const lds_llama_cfg& c = L->cfg;
    const size_t N = (size_t)B * S, QD = (size_t)c.heads * c.head_dim, KD = (size_t)c.kv_heads * c.head_dim;
    LlWs& w = s.w;
    w.x = A.f(N * c.hidden); w.q = A.f(N * QD); w.ctx = A.f(N * QD); w.ff = A.f(N * c.inter);
    w.logits = nullptr; w.flags = nullptr; w.plen = nullptr;
    w.stok = (int64_t*)A.f(2 * N);
    float *kc = A.f(N * KD), *vc = A.f(N * KD);
    w.kc.assign(c.layers, kc); w.vc.assign(c.layers, vc);
    s.chunk = A.f((size_t)kLlScoreChunk * c.vocab);
    s.psum = (double*)A.f(2 * (size_t)B);
    s.pcnt = (int32_t*)A.f((size_t)B);
}
// the shape checks that need no model, then the model's
int ll_score_check(const lds_llama* L, int B, int S) {
    if (B < 1) return set_error(LDS_EINVAL, "scoring needs B >= 1, got %d", B);
    if (S < 2 || S > kLlMaxLength) return set_error(LDS_EINVAL, "stream length %d out of range for scoring (2 .. %d)", S, kLlMaxLength);
    // the linears take 8 rows per workgroup along grid.y
    if ((long long)B * S > 8 * 65535LL) return set_error(LDS_EINVAL, "batch too large for one scoring call (B * S <= 524280, got %lld)", (long long)B * S);
    if (!L) return set_error(LDS_EINVAL, "null handle");
    if (S > L->cfg.max_pos) return set_error(LDS_EINVAL, "stream length %d exceeds max_position_embeddings %d", S, L->cfg.max_pos);
    return LDS_OK;
}
}  // namespace

extern "C" int lds_llama_score_workspace_bytes(const lds_llama* L, int B, int S, size_t* out) {
    if (int r = ll_score_check(L, B, S)) return r;
    if (!out) return set_error(LDS_EINVAL, "bad argument");
    Arena A(nullptr, 0);
    LlScoreWs s;
    ll_score_plan(L, A, B, S, s);
    *out = A.used;
    return LDS_OK;
}

extern "C" int lds_llama_score(lds_llama* L, const int64_t* input_ids, const int32_t* ids_len, const int64_t* labels, int B, int S, float* logprobs, int32_t* ranks,
                               float* loss, int32_t* n_counted, float* logits_out, void* ws, size_t ws_bytes, void* stream) {
    if (int r = ll_score_check(L, B, S)) return r;
    if (!input_ids || !logprobs || !ranks || !loss || !n_counted || !ws) return set_error(LDS_EINVAL, "null argument");
    const lds_llama_cfg& c = L->cfg;
    hipStream_t st = (hipStream_t)stream;
    Arena A(ws, ws_bytes);
    LlScoreWs s;
    ll_score_plan(L, A, B, S, s);
    if (!A.ok) return set_error(LDS_ENOMEM, "Llama scoring workspace too small: need %zu bytes", A.used);
    const int H = c.hidden, V = c.vocab, lo = c.first_free_id, N = B * S;
    if (!labels) labels = input_ids;      // the loader's choice (dataloader.py:182-183)
    // slots at and beyond a row's length are filled from PAD, as in the prefill: their rows are computed and never counted, and no counted
    // row's query sees their keys (row l reads the slots 0 .. l)
    hipLaunchKernelGGL(ll_score_init_kernel, dim3(B), dim3(256), 0, st, input_ids, S, ids_len, c.vocab, lo, c.pad - lo, s.w.stok);
    HIP_TRY(hipGetLastError());
    const LlRows rows{nullptr, S, 0, S};
    hipLaunchKernelGGL(ll_embed_kernel, dim3(N), dim3(256), 0, st, (const float*)L->embed, (const int64_t*)s.w.stok, rows, lo, c.vocab, H, s.w.x);
    HIP_TRY(hipGetLastError());
    if (int r = ll_layers(L, s.w, N, rows, S, st)) return r;
    for (int r0 = 0; r0 < N; r0 += kLlScoreChunk) {
        const int nr = (N - r0 < kLlScoreChunk) ? N - r0 : kLlScoreChunk;
        const float* x = s.w.x + (size_t)r0 * H;
        float* lg = logits_out ? logits_out + (size_t)r0 * V : s.chunk;
        // rows of width vocab: the low columns from their own matrix, the columns first_free_id .. by the decode's launch -- the same fmaf chain per
        // output, only the column's address differs
        if (lo > 0) HIP_TRY(ll_linear<LL_PLAIN>(x, H, L->nw_final, c.eps, L->head_lo, nullptr, lo, nullptr, lg, V, nr, st));
        HIP_TRY(ll_linear<LL_PLAIN>(x, H, L->nw_final, c.eps, L->head, nullptr, V - lo, nullptr, lg + lo, V, nr, st));
        HIP_TRY(lm_launch_score_rows(lg, r0, nr, V, S, labels, ids_len, logprobs, ranks, st));
    }
    HIP_TRY(lm_launch_score_loss(logprobs, ranks, B, S - 1, s.psum, s.pcnt, loss, n_counted, st));
    return LDS_OK;
}

// ---- greedy beam search (lds_llama_generate_beam): HF's _beam_search over B * K beam rows, every item from its own prompt.
//      Prefill: ONE row per item (B rows, not B * K), the plain decode's own, then moved into the item's first cache row; every beam reads the
//      positions below the item's prompt length from there.  Step s handles beam row n of item n / K at position plen[item] - 1 + s: the row's token comes from the running
//      sequences (ll_embed_kernel), its key / value go into cache row n, ll_attn_beam_kernel follows the ancestry table over the generated
//      positions, the head runs over the WHOLE vocabulary (scoring's two launches: HF's log_softmax sees the banned columns), and lm.hip's
//      per-row beam step selects.  An item whose own loop has ended freezes (lm_beam_step_kernel), so every item equals its stand-alone run and the
//      result does not depend on when the poll notices that all have ended. ----
namespace {
constexpr int kLlMaxBeamRows = 256;        // B * num_beams
constexpr int kLlMaxBeamLength = 7488;     // the beam attention stages a score and a source row per key in LDS
constexpr int kLlBeamPoll = 8;             // steps between two polls of the flag bits
struct LlBeamWs { LlWs w; int64_t *rseq[2], *fseq[2]; int* tab[2]; float *rscore, *fscore; int *ffin, *flen, *unsat, *ended, *flags, *rowlen; int32_t* plen_rows; };
void ll_beam_plan(const lds_llama* L, Arena& A, int B, int P, int cap, int K, LlBeamWs& s) {
    const lds_llama_cfg& c = L->cfg;
    const size_t R = (size_t)B * K, Npre = (size_t)B * (P > 2 ? P - 1 : 1), N = Npre > R ? Npre : R;
    const size_t QD = (size_t)c.heads * c.head_dim, KD = (size_t)c.kv_heads * c.head_dim;
    LlWs& w = s.w;
    w.x = A.f(N * c.hidden); w.q = A.f(N * QD); w.ctx = A.f(N * QD); w.ff = A.f(N * c.inter);
    w.logits = A.f(R * c.vocab);
    w.flags = nullptr; w.stok = nullptr;
    w.plen = (int32_t*)A.f((size_t)B);      // per item (the beam step, the init and finish kernels)
    s.plen_rows = (int32_t*)A.f(R);         // per beam row (LlRows)
    w.kc.clear(); w.vc.clear();
    for (int i = 0; i < c.layers; ++i) { w.kc.push_back(A.f(R * KD * cap)); w.vc.push_back(A.f(R * KD * cap)); }
    for (int i = 0; i < 2; ++i) { s.rseq[i] = (int64_t*)A.f(2 * R * cap); s.fseq[i] = (int64_t*)A.f(2 * R * cap); s.tab[i] = (int*)A.f(R * cap); }
    s.rscore = A.f(R); s.fscore = A.f(R); s.ffin = (int*)A.f(R); s.flen = (int*)A.f(R);
    s.unsat = (int*)A.f((size_t)B); s.ended = (int*)A.f((size_t)B); s.rowlen = (int*)A.f((size_t)B);
    s.flags = (int*)A.f((size_t)cap);
}
// the checks that need no model
int ll_beam_check_shape(int B, int P, int max_length, int K) {
    if (K < 2 || K > kMaxBeams) return set_error(LDS_EINVAL, "num_beams %d out of range for a beam decode (2 .. %d)", K, kMaxBeams);
    if (int r = ll_check_shape(B, P, max_length)) return r;
    if ((long long)B * K > kLlMaxBeamRows) return set_error(LDS_EINVAL, "a Llama beam decode takes at most %d beam rows, got B * num_beams = %d", kLlMaxBeamRows, B * K);
    if (max_length > kLlMaxBeamLength) return set_error(LDS_EINVAL, "max_length %d too long for a beam decode (<= %d)", max_length, kLlMaxBeamLength);
    return LDS_OK;
}
int ll_beam_check_model(const lds_llama* L, int K, int max_length) {
    const lds_llama_cfg& c = L->cfg;
    if (c.vocab > kMaxBeamVocab) return set_error(LDS_EINVAL, "beam search is built for vocabularies of at most %d entries, got %d", kMaxBeamVocab, c.vocab);
    if (c.vocab - c.first_free_id < 2 * K) return set_error(LDS_EINVAL, "beam search needs 2 * num_beams = %d ids that are not banned, got %d", 2 * K, c.vocab - c.first_free_id);
    if (max_length > c.max_pos) return set_error(LDS_EINVAL, "max_length %d exceeds max_position_embeddings %d", max_length, c.max_pos);
    return LDS_OK;
}
}  // namespace

extern "C" int lds_llama_beam_workspace_bytes(const lds_llama* L, int B, int P, int max_length, int num_beams, size_t* out) {
    if (int r = ll_beam_check_shape(B, P, max_length, num_beams)) return r;
    if (!L || !out) return set_error(LDS_EINVAL, "bad argument");
    Arena A(nullptr, 0);
    LlBeamWs s;
    ll_beam_plan(L, A, B, P, max_length, num_beams, s);
    *out = A.used;
    return LDS_OK;
}

namespace {
// the decode; poll = the steps between two polls (the public entry's is fixed; a test entry varies it to show that the result does not depend on it)
int ll_generate_beam(lds_llama* L, const int64_t* input_ids, const int32_t* in_len, int B, int P, int max_length, const lds_lm_decode_opts* opts, int64_t* tokens,
                     int* n_tokens_host, void* ws, size_t ws_bytes, void* stream, int poll) {
    if (!opts) return set_error(LDS_EINVAL, "null options");
    const lds_lm_decode_opts o = *opts;
    if (int r = lm_check_opts(o, nullptr)) return r;
    if (o.do_sample) return set_error(LDS_EINVAL, "beam sampling (do_sample with beams) is not built: only greedy beam search");
    const int K = o.num_beams;
    if (int r = ll_beam_check_shape(B, P, max_length, K)) return r;
    int Pmax = 0, Pmin = P;
    if (int r = ll_check_lens(in_len, B, P, max_length, Pmax, Pmin)) return r;
    if (!L || !input_ids || !tokens || !n_tokens_host || !ws) return set_error(LDS_EINVAL, "bad argument");
    if (int r = ll_beam_check_model(L, K, max_length)) return r;
    const lds_llama_cfg& c = L->cfg;
    const int H = c.hidden, V = c.vocab, lo = c.first_free_id, R = B * K, cap = max_length;
    const int Pq = Pmax - 1;
    if ((long long)B * Pq > 8 * 65535LL) return set_error(LDS_EINVAL, "B * P too large for the prefill (<= 524280)");
    hipStream_t st = (hipStream_t)stream;
    Arena A(ws, ws_bytes);
    LlBeamWs s;
    ll_beam_plan(L, A, B, P, max_length, K, s);
    if (!A.ok) return set_error(LDS_ENOMEM, "Llama beam workspace too small: need %zu bytes", A.used);
    const LlWs& w = s.w;
    {
        std::vector<int> pl(B), plr(R);
        for (int b = 0; b < B; ++b) pl[b] = in_len ? in_len[b] : P;
        for (int r = 0; r < R; ++r) plr[r] = pl[r / K];
        HIP_TRY(hipMemcpyAsync(w.plen, pl.data(), sizeof(int) * B, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(s.plen_rows, plr.data(), sizeof(int) * R, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));      // the host staging vectors go out of scope
    }
    const int32_t* plen = w.plen;
    HIP_TRY(hipMemsetAsync(s.flags, 0, sizeof(int) * cap, st));
    // Prefill: lds_llama_generate's own, B rows into cache rows 0 .. B - 1 (the ids, not shifted, wait in the first B rows of a sequence buffer
    // that the init kernel below fills afterwards); then item b's keys and values move to cache row b * K.  A shorter row's slots in_len[b] - 1 ..
    // Pq - 1 are filled from PAD and overwritten by the item's first beam row (which IS cache row b * K) before any query reads them.
    if (Pq > 0) {
        hipLaunchKernelGGL(ll_init_kernel, dim3(B), dim3(256), 0, st, input_ids, P, plen, V, 0, c.pad, cap, s.rseq[1]);
        HIP_TRY(hipGetLastError());
        const LlRows rows{plen, Pq, 0, cap};
        hipLaunchKernelGGL(ll_embed_kernel, dim3(B * Pq), dim3(256), 0, st, (const float*)L->embed, (const int64_t*)s.rseq[1], rows, 0, V, H, w.x);
        HIP_TRY(hipGetLastError());
        if (int r = ll_layers(L, w, B * Pq, rows, Pq, st)) return r;
        if (B > 1) {
            const long long elems = (long long)c.kv_heads * Pq * c.head_dim;
            for (int i = 0; i < c.layers; ++i)
                hipLaunchKernelGGL(ll_beam_spread_kernel, dim3((unsigned)((elems + 255) / 256), 2), dim3(256), 0, st, w.kc[i], w.vc[i], B, K, c.kv_heads, cap,
                                   c.head_dim, Pq);
            HIP_TRY(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(ll_beam_init_kernel, dim3(R), dim3(256), 0, st, input_ids, P, plen, V, c.pad, cap, K, s.rseq[0], s.rseq[1], s.fseq[0], s.fseq[1], s.rscore,
                       s.fscore, s.ffin, s.flen, s.unsat, s.ended);
    HIP_TRY(hipGetLastError());
    const int n_steps = max_length - Pmin;      // the shortest row's candidates all hit max_length at step n_steps - 1
    std::vector<int> host_flags(n_steps, 0);
    int checked = 0, last = 0;
    for (int step = 0; step < n_steps; ++step) {
        const int cur = step & 1, nxt = cur ^ 1;
        last = step;
        const LlRows rows{s.plen_rows, 0, step, cap};
        hipLaunchKernelGGL(ll_embed_kernel, dim3(R), dim3(256), 0, st, (const float*)L->embed, (const int64_t*)s.rseq[cur], rows, 0, V, H, w.x);
        HIP_TRY(hipGetLastError());
        const int Lk_max = (Pmax + step < max_length) ? Pmax + step : max_length;
        const LlBeamAttn ba{s.tab[cur], s.ended, cap, K};
        if (int r = ll_layers(L, w, R, rows, Lk_max, st, &ba)) return r;
        // rows of width vocab, as lds_llama_score forms them: the low columns from their own matrix, the others by the decode's launch
        if (lo > 0) HIP_TRY(ll_linear<LL_PLAIN>(w.x, H, L->nw_final, c.eps, L->head_lo, nullptr, lo, nullptr, w.logits, V, R, st));
        HIP_TRY(ll_linear<LL_PLAIN>(w.x, H, L->nw_final, c.eps, L->head, nullptr, V - lo, nullptr, w.logits + lo, V, R, st));
        const LmBeamState bs{s.rseq[cur], s.rseq[nxt], s.rscore, s.rscore, s.tab[cur], s.tab[nxt], s.fseq[cur], s.fseq[nxt], s.fscore, s.fscore, s.ffin, s.ffin,
                             s.flen, s.flen, s.unsat, s.unsat, nullptr, nullptr, s.flags + step};
        const LmBeamRows rw{plen, lo, s.ended, s.ended, cap};
        HIP_TRY(lm_launch_beam_rows(B, K, V, w.logits, step, cap, max_length, c.eos, o.repetition_penalty, o.no_repeat_ngram_size, o.early_stopping, bs, rw, st));
        if ((step + 1) % poll == 0 || step + 1 == n_steps) {      // the poll: bit 16 = some item's own loop still runs
            HIP_TRY(hipMemcpyAsync(host_flags.data() + checked, s.flags + checked, sizeof(int) * (step + 1 - checked), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            bool done = false;
            for (int q = checked; q <= step && !done; ++q) done = !(host_flags[q] & 16);
            checked = step + 1;
            if (done) break;
        }
    }
    // every item is frozen in both buffers from the step after its end on; the last step run wrote buffer (last + 1) & 1
    hipLaunchKernelGGL(ll_beam_finish_kernel, dim3(B), dim3(256), 0, st, (const int64_t*)s.fseq[(last + 1) & 1], (const int*)s.flen, plen, K, cap, c.pad, tokens, s.rowlen);
    HIP_TRY(hipGetLastError());
    std::vector<int> len(B, 0);
    HIP_TRY(hipMemcpyAsync(len.data(), s.rowlen, sizeof(int) * B, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int n_tokens = 0;
    for (int b = 0; b < B; ++b) n_tokens = len[b] > n_tokens ? len[b] : n_tokens;
    *n_tokens_host = n_tokens;
    return LDS_OK;
}
}  // namespace

extern "C" int lds_llama_generate_beam(lds_llama* L, const int64_t* input_ids, const int32_t* in_len, int B, int P, int max_length, const lds_lm_decode_opts* opts,
                                       int64_t* tokens, int* n_tokens_host, void* ws, size_t ws_bytes, void* stream) {
    return ll_generate_beam(L, input_ids, in_len, B, P, max_length, opts, tokens, n_tokens_host, ws, ws_bytes, stream, kLlBeamPoll);
}

// Test entries (include/lds_test.h).  lds_test_llama_generate_beam_poll: lds_llama_generate_beam with a poll interval of the caller's.
// lds_test_llama_beam_step: ONE step of the per-row beam step (lm_beam_step_kernel<NW, true>) on logits [B * K][V] and the
// given state; item b is at cur_len = prompt_len[b] + step.  lds_test_llama_beam_attn: ONE attention call over given q and caches.
extern "C" int lds_test_llama_generate_beam_poll(lds_llama* L, const int64_t* input_ids, const int32_t* in_len, int B, int P, int max_length,
                                                 const lds_lm_decode_opts* opts, int64_t* tokens, int* n_tokens_host, void* ws, size_t ws_bytes, void* stream, int poll) {
    if (poll < 1) return set_error(LDS_EINVAL, "poll interval %d (>= 1)", poll);
    return ll_generate_beam(L, input_ids, in_len, B, P, max_length, opts, tokens, n_tokens_host, ws, ws_bytes, stream, poll);
}
extern "C" int lds_test_llama_beam_step(const float* logits, int B, int K, int V, int step, int max_length, int eos, float repetition_penalty,
                                        int no_repeat_ngram_size, int early_stopping, int first_free_id, const int32_t* prompt_len, const int32_t* ended,
                                        const int64_t* run_seq, const float* run_score, const int64_t* fin_seq, const float* fin_score, const int32_t* fin_flag,
                                        const int32_t* fin_len, const int32_t* unsat, int64_t* run_seq_out, float* run_score_out, int32_t* parent_out,
                                        int64_t* fin_seq_out, float* fin_score_out, int32_t* fin_flag_out, int32_t* fin_len_out, int32_t* unsat_out,
                                        int32_t* ended_out, int32_t* flag_out, void* stream) {
    if (!logits || !prompt_len || !ended || !run_seq || !run_score || !fin_seq || !fin_score || !fin_flag || !fin_len || !unsat || !run_seq_out || !run_score_out ||
        !parent_out || !fin_seq_out || !fin_score_out || !fin_flag_out || !fin_len_out || !unsat_out || !ended_out || !flag_out)
        return set_error(LDS_EINVAL, "null argument");
    if (B <= 0 || B > kLlMaxBeamRows || K < 1 || K > kMaxBeams || V > kMaxBeamVocab || first_free_id < 0 || V - first_free_id < 2 * K || step < 0 ||
        no_repeat_ngram_size < 0 || early_stopping < 0 || early_stopping > 2)
        return set_error(LDS_EINVAL, "bad argument");
    for (int b = 0; b < B; ++b)      // a running item writes slot prompt_len[b] + step
        if (prompt_len[b] < 1 || (!ended[b] && prompt_len[b] + step >= max_length)) return set_error(LDS_EINVAL, "prompt_len[%d] + step outside the sequences", b);
    hipStream_t st = (hipStream_t)stream;
    int* dev = nullptr;      // prompt_len [B] | ended [B]
    if (hipMalloc((void**)&dev, sizeof(int) * 2 * B) != hipSuccess) return set_error(LDS_ENOMEM, "hipMalloc");
    int rc = LDS_OK;
    const LmBeamState bs{run_seq, run_seq_out, run_score, run_score_out, nullptr, nullptr, fin_seq, fin_seq_out, fin_score, fin_score_out, fin_flag, fin_flag_out,
                         fin_len, fin_len_out, unsat, unsat_out, parent_out, nullptr, flag_out};
    const LmBeamRows rw{dev, first_free_id, dev + B, ended_out, max_length};
    if (hipMemcpyAsync(dev, prompt_len, sizeof(int) * B, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(dev + B, ended, sizeof(int) * B, hipMemcpyHostToDevice, st) != hipSuccess || hipMemsetAsync(flag_out, 0, sizeof(int32_t), st) != hipSuccess ||
        lm_launch_beam_rows(B, K, V, logits, step, max_length, max_length, eos, repetition_penalty, no_repeat_ngram_size, early_stopping, bs, rw, st) != hipSuccess)
        rc = set_error(LDS_EHIP, "launch");
    if (hipStreamSynchronize(st) != hipSuccess) rc = set_error(LDS_EHIP, "sync");
    (void)hipFree(dev);
    return rc;
}
extern "C" int lds_test_llama_beam_attn(const float* q, const float* kc, const float* vc, const int32_t* tab, const int32_t* prompt_len, int R, int K, int heads,
                                        int kv_heads, int d, int cap, int tcap, int step, float* out, void* stream) {
    if (!q || !kc || !vc || !prompt_len || !out) return set_error(LDS_EINVAL, "null argument");
    if (R < 1 || R > 4096 || K < 1 || K > kMaxBeams || R % K || heads < 1 || kv_heads < 1 || heads % kv_heads || d < 16 || d > kLlMaxHeadDim || d % 16 || cap < 1 ||
        cap > kLlMaxBeamLength || step < 0 || (tab && tcap < step) || (!tab && K != 1))
        return set_error(LDS_EINVAL, "bad argument");
    int pos_max = 0;
    for (int i = 0; i < R / K; ++i) {
        const int pos = prompt_len[i] - 1 + step;
        if (prompt_len[i] < 1 || pos >= cap) return set_error(LDS_EINVAL, "prompt_len[%d] - 1 + step outside the cache", i);
        pos_max = pos > pos_max ? pos : pos_max;
    }
    hipStream_t st = (hipStream_t)stream;
    int* dev = nullptr;      // the lengths per row
    if (hipMalloc((void**)&dev, sizeof(int) * R) != hipSuccess) return set_error(LDS_ENOMEM, "hipMalloc");
    std::vector<int> plr(R);
    for (int r = 0; r < R; ++r) plr[r] = prompt_len[r / K];
    int rc = LDS_OK;
    const int Lkp = (pos_max + 1 + 63) & ~63;
    const size_t lds = (size_t)(kLlMaxHeadDim + Lkp + 4 * (2 + kLlMaxHeadDim)) * sizeof(float);
    const LlRows rows{dev, 0, step, cap};
    if (hipMemcpyAsync(dev, plr.data(), sizeof(int) * R, hipMemcpyHostToDevice, st) != hipSuccess) rc = set_error(LDS_EHIP, "copy");
    if (rc == LDS_OK) {
        if (tab)
            hipLaunchKernelGGL(ll_attn_beam_kernel, dim3((unsigned)(R * heads)), dim3(256), lds + (size_t)Lkp * sizeof(int), st, q, kc, vc, rows, heads, kv_heads, d, Lkp,
                               out, LlBeamAttn{tab, nullptr, tcap, K});
        else      // the plain kernel: K is 1, every row has its own prompt length and cache row
            hipLaunchKernelGGL(ll_attn_kernel, dim3((unsigned)(R * heads)), dim3(256), lds, st, q, kc, vc, rows, heads, kv_heads, d, Lkp, out);
        if (hipGetLastError() != hipSuccess) rc = set_error(LDS_EHIP, "launch");
    }
    if (hipStreamSynchronize(st) != hipSuccess) rc = set_error(LDS_EHIP, "sync");
    (void)hipFree(dev);
    return rc;
}
