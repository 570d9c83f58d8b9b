// Whisper's text decoder on gfx950 (OpenAI whisper/model.py TextDecoder; the reference's encoder/whisper/model.py:85-110 holds its blocks,
// ResidualAttentionBlock(cross_attention=True), and :150-154 the interface, Whisper.logits / Whisper.forward, that ends in it): token
// embedding + learned positions, n_layer pre-LN blocks of causal self-attention, cross-attention over the audio encoder's output and a GELU
// MLP, a final LayerNorm and the tied head x @ token_embedding^T.  Everything is fp32 and follows the rules of lm.hip / llama.hip: one
// fixed-order accumulation per output that depends neither on the batch size nor on whether a row is a prefill row or a decode step (both go
// through the SAME kernels, a row's position being the only thing that tells them apart), no atomics, the decode loop on the stream with an
// EOS poll every 8 steps.
//   linear      weights transposed [K][M]; a workgroup = 32 columns x 32 K-slices over 8 rows.  K is walked in chunks of 1280 staged in LDS
//               (8 x 1280 floats; mlp.2's K = 5120 is four chunks), slice s of a chunk is one ascending fmaf chain that carries on through the
//               chunks, the slices meet through LDS in the order 0, 1, .. 31.  32 columns (two 128-byte lines per wave and k) rather than
//               llama.hip's 64: the width-1280 projections then fill 40 workgroups, not 20.
//   LayerNorm   attn_ln / cross_attn_ln / mlp_ln / ln fused into the consuming linear: two-pass mean and variance of a row by one wave, the
//               normalised row staged chunk by chunk
//   q | k | v   one projection (key has no bias); the epilogue writes k, v into the row's cache slot: caches are [B][heads][cap][64]
//   q, k scale  Whisper multiplies q and k by d^-0.25 each; at d = 64 the product of the two is 2^-3, so the score is scaled once by 0.125, which
//               is exact in binary floating point -- the 2e-5 tolerance, not bit equality with torch's two roundings, is the contract
//   attention   one workgroup per (row, head) over the row's keys: the self cache's slots 0 .. pos, or the n_frames[b] cross keys
//   cross k, v  every layer's key | value rows of the encoder output in one launch per layer of the same linear (cache [B][heads][T][64]);
//               rows at and beyond n_frames[b] are neither read nor written
//   head        the linear with the final LayerNorm fused over 32-column tiles of the transposed embedding; the epilogue stores the logits only
//               when asked, applies the suppress mask and leaves each tile's (max, arg-max with ties to the lowest id, sum of exponentials);
//               wd_choose_kernel combines a row's tiles in one fixed order (thread t the tiles t, t + 256, .. ascending, then a tree over the
//               threads; ties to the lowest id) into the token, its log-prob and the log-sum-exp
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

// Which (batch row, position) row n of a pass is (llama.hip's LlRows).  L > 0: a causal pass, n = b * L + l at position l.  L == 0: a decode
// step, row b at position plen[b] - 1 + step; a row that has run past the cache is not live and stores nothing.
struct WdRows { const int32_t* plen; int L, step, cap; };
static __device__ __forceinline__ void wd_row(const WdRows& r, int n, int& b, int& pos, bool& live) {
    if (r.L > 0) {
        b = n / r.L; pos = n - b * r.L; live = true;
    } else {
        b = n; pos = r.plen[b] - 1 + r.step;
        live = pos < r.cap;
        pos = live ? pos : r.cap - 1;
    }
}

// stok [B][cap] = the row's ids clamped to the vocabulary, `fill` from len[b] on (len null: P everywhere)
__global__ void __launch_bounds__(256) wd_init_kernel(const int64_t* __restrict__ ids, int P, const int32_t* __restrict__ len, int vocab, int fill, int cap,
                                                      int64_t* __restrict__ stok) {
    const int b = blockIdx.x, pl = len ? len[b] : P;
    for (int l = threadIdx.x; l < cap; l += 256) {
        long long t = fill;
        if (l < pl && l < P) {
            t = ids[(long long)b * P + l];
            t = (t < 0) ? 0 : (t >= vocab ? vocab - 1 : t);
        }
        stok[(long long)b * cap + l] = t;
    }
}
// x[n] = token_embedding[id of row n] + positional_embedding[its position]
__global__ void __launch_bounds__(256) wd_embed_kernel(const float* __restrict__ emb, const float* __restrict__ pe, const int64_t* __restrict__ stok, const WdRows rows,
                                                       int vocab, int C, float* __restrict__ x) {
    const int n = blockIdx.x;
    int b, pos;
    bool live;
    wd_row(rows, n, b, pos, live);
    long long t = stok[(long long)b * rows.cap + pos];
    t = (t < 0) ? 0 : (t >= vocab ? vocab - 1 : t);
    for (int c = threadIdx.x; c < C; c += 256) x[(long long)n * C + c] = emb[t * C + c] + pe[(long long)pos * C + c];
}
// mask[v] = 0, then |= bit for the listed ids (two launches; a repeated id writes the same value twice)
__global__ void __launch_bounds__(256) wd_mask_kernel(int* __restrict__ mask, int V, const int32_t* __restrict__ list, int n, int bit) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (!list) { if (i < V) mask[i] = 0; return; }
    if (i < n) { const int id = list[i]; if (id >= 0 && id < V) mask[id] |= bit; }
}

// ---- Y[n][m] = epi(sum_k ln(X)[n][k] * Wt[k][m] + bias[m]) for 8 rows x 32 columns per workgroup (the head of this file) ----
enum { WD_PLAIN = 0, WD_GELU = 1, WD_RESID = 2, WD_QKV = 3, WD_CROSSKV = 4, WD_HEAD = 5 };
struct WdEpi {
    float *kc, *vc;                 // WD_QKV: the self caches [B][heads][cap][64]; WD_CROSSKV: the cross caches [B][heads][T][64]
    WdRows rows;                    // WD_QKV
    const int32_t* nfr; int T;      // WD_CROSSKV: row n = b * T + t, live when t < nfr[b]
    int C;                          // n_state
    const int* mask; int bits;      // WD_HEAD: column m counts as -inf when mask[m] & bits
    float* logits; long long ldl;   //          the raw logits row, or null
    float* pmax; int* parg; float* psum; int ntiles;      // the tiles' statistics [N][ntiles], or null
};
constexpr int kWdCols = 32, kWdSlices = 32, kWdChunk = 1280, kWdUnroll = 20;      // (a slice of a full chunk is 40 k: two batches of loads)

template <int EPI>
__global__ void __launch_bounds__(1024) wd_linear_kernel(const float* __restrict__ X, int K, const float* __restrict__ g, const float* __restrict__ bt, float eps,
                                                        const float* __restrict__ Wt, const float* __restrict__ bias, int M, const float* R, float* Y, int ldy, int N,
                                                        const WdEpi ep) {
    constexpr int COLS = kWdCols, KS = kWdSlices;
    extern __shared__ __attribute__((aligned(16))) float sm[];      // xs [KC][8], part [KS-1][COLS][8], mean [8], rstd [8], ok [8]
    const int KC = K < kWdChunk ? K : kWdChunk;
    float* xs = sm;
    float* part = sm + (size_t)KC * 8;
    float* mean_s = part + (size_t)(KS - 1) * COLS * 8;
    float* rstd_s = mean_s + 8;
    int* ok_s = reinterpret_cast<int*>(rstd_s + 8);
    const int tid = threadIdx.x, col = tid % COLS, ks = tid / COLS, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.y * 8;
    const int m = blockIdx.x * COLS + col;
    const bool valid = m < M;
    if (tid < 8) {
        const int n = n0 + tid;
        bool ok = n < N;
        if (EPI == WD_CROSSKV && ok) {
            const int b = n / ep.T, t = n - b * ep.T;
            ok = t < (ep.nfr ? ep.nfr[b] : ep.T);
        }
        ok_s[tid] = ok ? 1 : 0;
    }
    __syncthreads();
    if constexpr (EPI == WD_CROSSKV) {      // (uniform) a tile that lies wholly at or beyond its clips' frames: no weight is streamed for it
        if (!(ok_s[0] | ok_s[1] | ok_s[2] | ok_s[3] | ok_s[4] | ok_s[5] | ok_s[6] | ok_s[7])) return;
    }
    if (g) {      // LayerNorm statistics: wave j owns row j (lane-strided sums in ascending k, the DPP tree)
        if (wave < 8) {
            float mu = 0.f, rs = 0.f;
            if (ok_s[wave]) {
                const float* xr = X + (long long)(n0 + wave) * K;
                float s = 0.f, ss = 0.f;      // (eight loads in flight per lane; each lane adds its elements in ascending k)
                for (int k = lane; k < K; k += 512) {
                    float v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) v[u] = (k + 64 * u < K) ? xr[k + 64 * u] : 0.f;
#pragma unroll
                    for (int u = 0; u < 8; ++u) s += v[u];
                }
                mu = wave_sum(s) / (float)K;
                for (int k = lane; k < K; k += 512) {
                    float v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) v[u] = (k + 64 * u < K) ? xr[k + 64 * u] - mu : 0.f;
#pragma unroll
                    for (int u = 0; u < 8; ++u) ss = fmaf(v[u], v[u], ss);
                }
                rs = 1.0f / sqrtf(wave_sum(ss) / (float)K + eps);
            }
            if (lane == 0) { mean_s[wave] = mu; rstd_s[wave] = rs; }
        }
        __syncthreads();
    }
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    const bool upper = N - n0 > 4;      // (uniform) rows 4 .. 7 of the tile exist; otherwise they are staged zeros and their sums stay 0
    for (int c0 = 0; c0 < K; c0 += KC) {
        const int kc = (K - c0 < KC) ? K - c0 : KC;
        if (c0 > 0) __syncthreads();      // the chunk before has been read
        for (int i = tid; i < kc * 8; i += 1024) {
            const int k = i >> 3, j = i & 7;
            float v = 0.f;
            if (ok_s[j]) {
                v = X[(long long)(n0 + j) * K + c0 + k];
                if (g) v = ((v - mean_s[j]) * rstd_s[j]) * g[c0 + k] + bt[c0 + k];
            }
            xs[i] = v;
        }
        __syncthreads();
        const int kq = (kc + KS - 1) / KS, k0 = ks * kq, k1 = (k0 + kq < kc) ? k0 + kq : kc;
        if (valid) {
            const float* wp = Wt + (long long)c0 * M + m;
            int k = k0;
            for (; k + kWdUnroll <= k1; k += kWdUnroll) {
                float w[kWdUnroll];
#pragma unroll
                for (int u = 0; u < kWdUnroll; ++u) w[u] = wp[(long long)(k + u) * M];
#pragma unroll
                for (int u = 0; u < kWdUnroll; ++u) {
                    const f32x4 a = *reinterpret_cast<const f32x4*>(xs + 8 * (k + u));
                    acc[0] = fmaf(w[u], a[0], acc[0]); acc[1] = fmaf(w[u], a[1], acc[1]); acc[2] = fmaf(w[u], a[2], acc[2]); acc[3] = fmaf(w[u], a[3], acc[3]);
                    if (upper) {
                        const f32x4 b = *reinterpret_cast<const f32x4*>(xs + 8 * (k + u) + 4);
                        acc[4] = fmaf(w[u], b[0], acc[4]); acc[5] = fmaf(w[u], b[1], acc[5]); acc[6] = fmaf(w[u], b[2], acc[6]); acc[7] = fmaf(w[u], b[3], acc[7]);
                    }
                }
            }
            for (; k < k1; ++k) {
                const float w = wp[(long long)k * M];
                const f32x4 a = *reinterpret_cast<const f32x4*>(xs + 8 * k), b = *reinterpret_cast<const f32x4*>(xs + 8 * k + 4);
                acc[0] = fmaf(w, a[0], acc[0]); acc[1] = fmaf(w, a[1], acc[1]); acc[2] = fmaf(w, a[2], acc[2]); acc[3] = fmaf(w, a[3], acc[3]);
                acc[4] = fmaf(w, b[0], acc[4]); acc[5] = fmaf(w, b[1], acc[5]); acc[6] = fmaf(w, b[2], acc[6]); acc[7] = fmaf(w, b[3], acc[7]);
            }
        }
    }
    if (ks > 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) part[((size_t)(ks - 1) * COLS + col) * 8 + j] = acc[j];
    }
    __syncthreads();      // (xs is free from here on: the head keeps its tile there)
    if (ks == 0) {
#pragma unroll 1
        for (int q = 0; q < KS - 1; ++q) {
            const float* pp = part + ((size_t)q * COLS + col) * 8;
            const f32x4 a = *reinterpret_cast<const f32x4*>(pp), b = *reinterpret_cast<const f32x4*>(pp + 4);
            acc[0] += a[0]; acc[1] += a[1]; acc[2] += a[2]; acc[3] += a[3];
            acc[4] += b[0]; acc[5] += b[1]; acc[6] += b[2]; acc[7] += b[3];
        }
        const float bv = (bias && valid) ? bias[m] : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int n = n0 + j;
            const bool ok = valid && ok_s[j];
            float y = acc[j] + bv;
            if constexpr (EPI == WD_GELU) y = 0.5f * y * (1.0f + erff(y * 0.70710678118654752440f));
            if constexpr (EPI == WD_RESID) { if (ok) y += R[(long long)n * M + m]; }
            if constexpr (EPI == WD_QKV) {
                int b, pos;
                bool live;
                wd_row(ep.rows, n < N ? n : n0, b, pos, live);
                if (ok && live) {
                    const int C = ep.C, heads = C >> 6;
                    if (m < C) Y[(long long)n * ldy + m] = y;
                    else {
                        const int mm = (m < 2 * C) ? m - C : m - 2 * C;
                        float* cache = (m < 2 * C) ? ep.kc : ep.vc;
                        cache[(((long long)b * heads + (mm >> 6)) * ep.rows.cap + pos) * 64 + (mm & 63)] = y;
                    }
                }
            } else if constexpr (EPI == WD_CROSSKV) {
                if (ok) {
                    const int C = ep.C, heads = C >> 6, b = n / ep.T, t = n - b * ep.T;
                    const int mm = (m < C) ? m : m - C;
                    float* cache = (m < C) ? ep.kc : ep.vc;
                    cache[(((long long)b * heads + (mm >> 6)) * ep.T + t) * 64 + (mm & 63)] = y;
                }
            } else if constexpr (EPI == WD_HEAD) {
                if (ok && ep.logits) ep.logits[(long long)n * ep.ldl + m] = y;
                const bool banned = !valid || (ep.mask && (ep.mask[m] & ep.bits));
                xs[j * COLS + col] = banned ? -INFINITY : y;
            } else {
                if (ok) Y[(long long)n * ldy + m] = y;
            }
        }
    }
    if constexpr (EPI == WD_HEAD) {
        __syncthreads();
        if (tid < 8 && n0 + tid < N && ep.pmax) {      // row tid of the tile: one thread, the columns in ascending order
            const float* tl = xs + tid * COLS;
            float mx = tl[0];
            int arg = 0;
            for (int c = 1; c < COLS; ++c)
                if (tl[c] > mx) { mx = tl[c]; arg = c; }
            float s = 0.f;
            if (mx > -INFINITY)
                for (int c = 0; c < COLS; ++c) s += expf(tl[c] - mx);      // (exp(-inf) = 0 for a banned column)
            const long long o = (long long)(n0 + tid) * ep.ntiles + blockIdx.x;
            ep.pmax[o] = mx; ep.parg[o] = blockIdx.x * COLS + arg; ep.psum[o] = s;
        }
    }
}

// ---- attention of one (row, head) per workgroup, d = 64 (ll_attn_kernel's scheme on sixteen waves): wave w takes the 64-key blocks w, w + 16, ..; phase 1 has a
//      key per lane, phase 2 a channel per lane over the wave's keys in ascending order; the waves' (max, sum, partial output) meet through LDS
//      in the order 0 .. 15.  nfr == null && T == 0: self-attention over the cache slots 0 .. pos of the row ([B][heads][cap][64]).  Otherwise
//      cross-attention over the keys 0 .. nfr[b] of [B][heads][T][64].  q, out [N][heads * 64]. ----
__global__ void __launch_bounds__(1024) wd_attn_kernel(const float* __restrict__ q, const float* __restrict__ kc, const float* __restrict__ vc, const WdRows rows,
                                                      int heads, const int32_t* __restrict__ nfr, int T, int Lkp, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float sa[];      // qs [64], sc [Lkp], mrg [16][2 + 64]
    float* qs = sa;
    float* sc = sa + 64;
    float* mrg = sc + Lkp;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.x % heads, n = blockIdx.x / heads;
    int b, pos;
    bool live;
    wd_row(rows, n, b, pos, live);
    const int C = heads * 64;
    if (!live) {      // (uniform over the workgroup) a row past its end: zeros
        if (tid < 64) out[(long long)n * C + h * 64 + tid] = 0.f;
        return;
    }
    const bool cross = T > 0;
    int Lk = cross ? (nfr ? nfr[b] : T) : pos + 1;
    Lk = Lk < Lkp ? Lk : Lkp;
    const long long stride = cross ? T : rows.cap;
    if (tid < 64) qs[tid] = q[(long long)n * C + h * 64 + tid];
    __syncthreads();
    const float* kb = kc + ((long long)b * heads + h) * stride * 64;
    const float* vb = vc + ((long long)b * heads + h) * stride * 64;
    float mx = -INFINITY;
    for (int k0 = wave * 64; k0 < Lk; k0 += 1024) {
        const int key = k0 + lane;
        float dot = -INFINITY;
        if (key < Lk) {
            dot = 0.f;
            const f32x4* kr = reinterpret_cast<const f32x4*>(kb + (long long)key * 64);
            const f32x4* q4 = reinterpret_cast<const f32x4*>(qs);
            for (int e4 = 0; e4 < 16; e4 += 4) {
                f32x4 kv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) kv[u] = kr[e4 + u];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const f32x4 qv = q4[e4 + u];
                    dot = fmaf(qv[0], kv[u][0], dot); dot = fmaf(qv[1], kv[u][1], dot); dot = fmaf(qv[2], kv[u][2], dot); dot = fmaf(qv[3], kv[u][3], dot);
                }
            }
            dot *= 0.125f;      // (64^-0.25)^2
            sc[key] = dot;
        }
        mx = fmaxf(mx, dot);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int k0 = wave * 64; k0 < Lk; k0 += 1024) {
        const int key = k0 + lane;
        float p = 0.f;
        if (key < Lk) { p = expf(sc[key] - mx); sc[key] = p; }
        sum += p;
    }
    sum = wave_sum(sum);
    __syncthreads();      // the probabilities are in LDS
    float acc = 0.f;
    for (int k0 = wave * 64; k0 < Lk; k0 += 1024) {
        const int kend = (k0 + 64 < Lk) ? k0 + 64 : Lk;
        int key = k0;
        for (; key + 8 <= kend; key += 8) {      // eight value rows in flight, added in key order
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = vb[(long long)(key + u) * 64 + lane];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = fmaf(sc[key + u], v[u], acc);
        }
        for (; key < kend; ++key) acc = fmaf(sc[key], vb[(long long)key * 64 + lane], acc);
    }
    float* mw = mrg + wave * 66;
    if (lane == 0) { mw[0] = mx; mw[1] = sum; }
    mw[2 + lane] = acc;
    __syncthreads();
    if (tid < 64) {
        float m = mrg[0];
#pragma unroll
        for (int w = 1; w < 16; ++w) m = fmaxf(m, mrg[w * 66]);
        float tot = 0.f, o = 0.f;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const float f = (mrg[w * 66] > -INFINITY) ? expf(mrg[w * 66] - m) : 0.f;
            tot += mrg[w * 66 + 1] * f;
            o += mrg[w * 66 + 2 + tid] * f;
        }
        out[(long long)n * C + h * 64 + tid] = o / tot;
    }
}

// ---- the head's second stage, one workgroup per row: the tiles' (max, arg, sum) in one fixed order (thread t its tiles t, t + 256, .. ascending, then the threads' partials: a
//      tree for the max, block_sum256 for the sum) -> the arg-max over the unsuppressed
//      columns (ties: the lowest id), the log-sum-exp, the chosen id's log-prob.  st != null: a decode step's bookkeeping for row b --
//      the id goes to slot plen[b] + step, a row ends at EOS, after max_new ids or when the sequence is full. ----
struct WdStep { int64_t* stok; const int32_t* plen; int* unfinished; int* rowlen; float* tlp; int step, cap, max_new, eos; };
__global__ void __launch_bounds__(256) wd_choose_kernel(const float* __restrict__ pmax, const int* __restrict__ parg, const float* __restrict__ psum, int ntiles,
                                                       int64_t* __restrict__ tok_out, float* __restrict__ lp_out, float* __restrict__ lse_out, const WdStep sp, int has_step) {
    __shared__ float red[4];
    __shared__ float bm[256];
    __shared__ int ba[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long o = (long long)b * ntiles;
    float mx = -INFINITY;
    int arg = 0x7fffffff;
    for (int t = tid; t < ntiles; t += 256) {
        const float v = pmax[o + t];
        if (v > mx || (v == mx && parg[o + t] < arg)) { mx = v; arg = parg[o + t]; }
    }
    bm[tid] = mx; ba[tid] = arg;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {      // max is exact in any order; equal maxima keep the lowest id
        if (tid < s) {
            const float v = bm[tid + s];
            const int a = ba[tid + s];
            if (v > bm[tid] || (v == bm[tid] && a < ba[tid])) { bm[tid] = v; ba[tid] = a; }
        }
        __syncthreads();
    }
    mx = bm[0]; arg = ba[0];
    float s = 0.f;
    for (int t = tid; t < ntiles; t += 256) {
        const float v = pmax[o + t];
        if (v > -INFINITY) s += psum[o + t] * expf(v - mx);
    }
    s = block_sum256(s, red);
    if (tid != 0) return;
    const float lp = -logf(s), lse = mx + logf(s);
    if (tok_out) tok_out[b] = arg;
    if (lp_out) lp_out[b] = lp;
    if (lse_out) lse_out[b] = lse;
    if (!has_step || !sp.unfinished[b]) return;
    const int slot = sp.plen[b] + sp.step;
    if (slot < sp.cap && sp.step < sp.max_new) {
        sp.stok[(long long)b * sp.cap + slot] = arg;
        sp.tlp[(long long)b * sp.max_new + sp.step] = lp;
        if (arg == sp.eos || slot + 1 >= sp.cap || sp.step + 1 >= sp.max_new) { sp.unfinished[b] = 0; sp.rowlen[b] = slot + 1; }
    } else {
        sp.unfinished[b] = 0; sp.rowlen[b] = slot < sp.cap ? slot : sp.cap;
    }
}
// any_unf[step] = does some row still run after this step
__global__ void __launch_bounds__(64) wd_flag_kernel(const int* __restrict__ unfinished, int B, int* __restrict__ flag) {
    if (threadIdx.x != 0) return;
    int any = 0;
    for (int b = 0; b < B; ++b) any |= unfinished[b];
    *flag = any;
}
// the end of a decode: tokens = stok, sum_logprob[b] = the row's log-probs in step order
__global__ void __launch_bounds__(256) wd_finish_kernel(const int64_t* __restrict__ stok, int cap, int64_t* __restrict__ tokens, const float* __restrict__ tlp, int max_new,
                                                       float* __restrict__ sum_lp) {
    const int b = blockIdx.x;
    for (int l = threadIdx.x; l < cap; l += 256) tokens[(long long)b * cap + l] = stok[(long long)b * cap + l];
    if (threadIdx.x == 0 && sum_lp) {
        float s = 0.f;
        for (int i = 0; i < max_new; ++i) s += tlp[(long long)b * max_new + i];
        sum_lp[b] = s;
    }
}

}  // namespace lds

using namespace lds;

// ================================================================================================
// host side
// ================================================================================================
struct WdLayer {
    float *ag = nullptr, *ab = nullptr, *wqkv = nullptr, *bqkv = nullptr, *wo = nullptr, *bo = nullptr;
    float *cg = nullptr, *cb = nullptr, *wcq = nullptr, *bcq = nullptr, *wckv = nullptr, *bckv = nullptr, *wco = nullptr, *bco = nullptr;
    float *mg = nullptr, *mb = nullptr, *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr;
};
struct lds_whisper_decoder {
    lds_whisper_decoder_cfg cfg;
    Owner own;
    float *emb = nullptr, *pe = nullptr, *lg = nullptr, *lb = nullptr, *head = nullptr;      // head [n_state][n_vocab]: the embedding transposed
    std::vector<WdLayer> layers;
};

namespace {
constexpr int kWdMaxBatch = 64, kWdMaxTextCtx = 448, kWdMaxAudioCtx = 1500, kWdMaxVocab = 1 << 20, kWdScoreChunk = 64;

// reference layout W [M][K] -> transposed [K][M], several matrices concatenated along M; a bias of the same columns (a null name: zeros)
bool wd_linear_up(WeightLoader& T, const std::vector<std::pair<std::string, std::string>>& mats, int Mper, int K, float*& wt_out, float*& b_out) {
    const int M = Mper * (int)mats.size();
    std::vector<float> wt((size_t)K * M), bs((size_t)M, 0.f);
    int c0 = 0;
    for (auto& s : mats) {
        const float* w = T.get(s.first, (int64_t)Mper * K);
        if (!w) return false;
        for (int m = 0; m < Mper; ++m)
            for (int k = 0; k < K; ++k) wt[(size_t)k * M + c0 + m] = w[(size_t)m * K + k];
        if (!s.second.empty()) {
            const float* b = T.get(s.second, Mper);
            if (!b) return false;
            memcpy(bs.data() + c0, b, sizeof(float) * Mper);
        }
        c0 += Mper;
    }
    return (wt_out = T.o.upload(wt)) != nullptr && (b_out = T.o.upload(bs)) != nullptr;
}
int wd_check_cfg(const lds_whisper_decoder_cfg& c) {
    LDS_TRY(width_check("whisper decoder", "n_state", c.n_state, false));
    LDS_TRY(heads_check("whisper decoder", c.n_state, c.n_head));
    LDS_TRY(range_check("whisper decoder", "n_layer", c.n_layer, 1, 64));
    LDS_TRY(range_check("whisper decoder", "n_text_ctx", c.n_text_ctx, 2, kWdMaxTextCtx));
    LDS_TRY(range_check("whisper decoder", "n_audio_ctx", c.n_audio_ctx, 1, kWdMaxAudioCtx));
    LDS_TRY(range_check("whisper decoder", "n_vocab", c.n_vocab, 2, kWdMaxVocab));
    if (c.n_state > 8192) return set_error(LDS_EINVAL, "whisper decoder: n_state %d too wide (<= 8192)", c.n_state);
    return LDS_OK;
}
}  // namespace

extern "C" int lds_whisper_decoder_create(const lds_whisper_decoder_cfg* cfg, int n, const char* const* names, const float* const* ptrs, const int64_t* numel,
                                          lds_whisper_decoder** out) {
    if (!cfg || !names || !ptrs || !numel || !out || n < 0) return set_error(LDS_EINVAL, "null argument");
    LDS_TRY(wd_check_cfg(*cfg));
    const lds_whisper_decoder_cfg& c = *cfg;
    lds_whisper_decoder* h = new lds_whisper_decoder();
    h->cfg = c;
    WeightLoader T(h->own, n, names, ptrs, numel);
    const int C = c.n_state, V = c.n_vocab;
    bool ok = (h->emb = T.vec("decoder.token_embedding.weight", (int64_t)V * C)) != nullptr &&
              (h->pe = T.vec("decoder.positional_embedding", (int64_t)c.n_text_ctx * C)) != nullptr;
    for (int i = 0; i < c.n_layer && ok; ++i) {
        WdLayer y;
        const std::string p = "decoder.blocks." + std::to_string(i) + ".";
        ok = (y.ag = T.vec(p + "attn_ln.weight", C)) && (y.ab = T.vec(p + "attn_ln.bias", C)) &&
             wd_linear_up(T, {{p + "attn.query.weight", p + "attn.query.bias"}, {p + "attn.key.weight", ""}, {p + "attn.value.weight", p + "attn.value.bias"}}, C, C,
                          y.wqkv, y.bqkv) &&
             wd_linear_up(T, {{p + "attn.out.weight", p + "attn.out.bias"}}, C, C, y.wo, y.bo) && (y.cg = T.vec(p + "cross_attn_ln.weight", C)) &&
             (y.cb = T.vec(p + "cross_attn_ln.bias", C)) && wd_linear_up(T, {{p + "cross_attn.query.weight", p + "cross_attn.query.bias"}}, C, C, y.wcq, y.bcq) &&
             wd_linear_up(T, {{p + "cross_attn.key.weight", ""}, {p + "cross_attn.value.weight", p + "cross_attn.value.bias"}}, C, C, y.wckv, y.bckv) &&
             wd_linear_up(T, {{p + "cross_attn.out.weight", p + "cross_attn.out.bias"}}, C, C, y.wco, y.bco) && (y.mg = T.vec(p + "mlp_ln.weight", C)) &&
             (y.mb = T.vec(p + "mlp_ln.bias", C)) && wd_linear_up(T, {{p + "mlp.0.weight", p + "mlp.0.bias"}}, 4 * C, C, y.w1, y.b1) &&
             wd_linear_up(T, {{p + "mlp.2.weight", p + "mlp.2.bias"}}, C, 4 * C, y.w2, y.b2);
        h->layers.push_back(y);
    }
    ok = ok && (h->lg = T.vec("decoder.ln.weight", C)) != nullptr && (h->lb = T.vec("decoder.ln.bias", C)) != nullptr;
    if (ok) {      // the tied head: the embedding once more, transposed for the head's column walk
        const float* e = T.get("decoder.token_embedding.weight", (int64_t)V * C);
        std::vector<float> et((size_t)C * V);
        for (int v = 0; v < V; ++v)
            for (int k = 0; k < C; ++k) et[(size_t)k * V + v] = e[(size_t)v * C + k];
        ok = (h->head = T.o.upload(et)) != nullptr;
    }
    return T.finish(ok, "whisper decoder", h, out);
}
extern "C" void lds_whisper_decoder_destroy(lds_whisper_decoder* h) { delete h; }

namespace {
struct WdWs {
    int32_t* nfr;                        // [64] the clips' frame counts, written by lds_whisper_decoder_cross
    std::vector<float*> ck, cv;          // cross caches [B][heads][T][64] per layer, written by lds_whisper_decoder_cross
    float *x, *q, *ctx, *ff, *chunk, *pmax, *psum;
    int *parg, *mask, *flags;
    int64_t* stok;
    int32_t *plen, *pcnt;
    double* psum_d;
    std::vector<float*> kc, vc;          // self caches [B][heads][S][64] per layer
};
// one plan for the three calls: the cross part first (it depends on B and T alone, so a later call finds what `cross` left), then S positions
void wd_plan(const lds_whisper_decoder* h, Arena& A, int B, int T, int S, WdWs& w) {
    const lds_whisper_decoder_cfg& c = h->cfg;
    const size_t C = c.n_state, N = (size_t)B * S, V = c.n_vocab, ntiles = (V + kWdCols - 1) / kWdCols;
    w.nfr = (int32_t*)A.f(64);
    w.ck.clear(); w.cv.clear(); w.kc.clear(); w.vc.clear();
    for (int i = 0; i < c.n_layer; ++i) { w.ck.push_back(A.f((size_t)B * T * C)); w.cv.push_back(A.f((size_t)B * T * C)); }
    w.x = A.f(N * C); w.q = A.f(N * C); w.ctx = A.f(N * C); w.ff = A.f(N * 4 * C);
    for (int i = 0; i < c.n_layer; ++i) { w.kc.push_back(A.f(N * C)); w.vc.push_back(A.f(N * C)); }
    w.chunk = A.f((size_t)kWdScoreChunk * V);
    w.pmax = A.f((size_t)kWdMaxBatch * ntiles); w.psum = A.f((size_t)kWdMaxBatch * ntiles); w.parg = (int*)A.f((size_t)kWdMaxBatch * ntiles);
    w.mask = (int*)A.f(V);
    w.flags = (int*)A.f((size_t)B + S + kWdMaxBatch);
    w.stok = (int64_t*)A.f(2 * N);
    w.plen = (int32_t*)A.f((size_t)B);
    w.psum_d = (double*)A.f(2 * (size_t)B);
    w.pcnt = (int32_t*)A.f((size_t)B);
}
int wd_check_shape(const lds_whisper_decoder* h, int B, int T, int S) {
    if (!h) return set_error(LDS_EINVAL, "whisper decoder: null handle");
    LDS_TRY(range_check("whisper decoder", "B", B, 1, kWdMaxBatch));
    LDS_TRY(range_check("whisper decoder", "T", T, 1, h->cfg.n_audio_ctx));
    if (S < 2 || S > h->cfg.n_text_ctx) return set_error(LDS_EINVAL, "whisper decoder: %d positions outside 2 .. n_text_ctx = %d", S, h->cfg.n_text_ctx);
    return LDS_OK;
}

template <int EPI>
hipError_t wd_linear(const float* X, int K, const float* g, const float* bt, const float* Wt, const float* bias, int M, const float* R, float* Y, int ldy, int N,
                     const WdEpi& ep, hipStream_t st) {
    auto kern = wd_linear_kernel<EPI>;
    static std::atomic<unsigned long long> attr_done{0};
    hipError_t e = ensure_max_dynamic_lds(reinterpret_cast<const void*>(kern), attr_done);
    if (e != hipSuccess) return e;
    const int KC = K < kWdChunk ? K : kWdChunk;
    const size_t lds = ((size_t)KC * 8 + (size_t)(kWdSlices - 1) * kWdCols * 8 + 24) * sizeof(float);
    hipLaunchKernelGGL(kern, dim3((M + kWdCols - 1) / kWdCols, (N + 7) / 8), dim3(1024), lds, st, X, K, g, bt, 1e-5f, Wt, bias, M, R, Y, ldy, N, ep);
    return hipGetLastError();
}
hipError_t wd_attn(const float* q, const float* kc, const float* vc, const WdRows& rows, int heads, const int32_t* nfr, int T, int Lk_max, float* out, int N,
                   hipStream_t st) {
    const int Lkp = (Lk_max + 63) & ~63;
    hipLaunchKernelGGL(wd_attn_kernel, dim3((unsigned)(N * heads)), dim3(1024), (size_t)(64 + Lkp + 16 * 66) * sizeof(float), st, q, kc, vc, rows, heads, nfr, T, Lkp, out);
    return hipGetLastError();
}
// the blocks over N rows (a causal pass or a decode step, told apart by `rows` alone); Lk_max = the most self keys any row sees
int wd_layers(const lds_whisper_decoder* h, const WdWs& w, int N, const WdRows& rows, int Lk_max, int T, hipStream_t st) {
    const lds_whisper_decoder_cfg& c = h->cfg;
    const int C = c.n_state;
    for (int i = 0; i < c.n_layer; ++i) {
        const WdLayer& y = h->layers[i];
        WdEpi ep{};
        ep.kc = w.kc[i]; ep.vc = w.vc[i]; ep.rows = rows; ep.C = C;
        HIP_TRY(wd_linear<WD_QKV>(w.x, C, y.ag, y.ab, y.wqkv, y.bqkv, 3 * C, nullptr, w.q, C, N, ep, st));
        HIP_TRY(wd_attn(w.q, w.kc[i], w.vc[i], rows, c.n_head, nullptr, 0, Lk_max, w.ctx, N, st));
        HIP_TRY(wd_linear<WD_RESID>(w.ctx, C, nullptr, nullptr, y.wo, y.bo, C, w.x, w.x, C, N, WdEpi{}, st));
        HIP_TRY(wd_linear<WD_PLAIN>(w.x, C, y.cg, y.cb, y.wcq, y.bcq, C, nullptr, w.q, C, N, WdEpi{}, st));
        HIP_TRY(wd_attn(w.q, w.ck[i], w.cv[i], rows, c.n_head, w.nfr, T, T, w.ctx, N, st));
        HIP_TRY(wd_linear<WD_RESID>(w.ctx, C, nullptr, nullptr, y.wco, y.bco, C, w.x, w.x, C, N, WdEpi{}, st));
        HIP_TRY(wd_linear<WD_GELU>(w.x, C, y.mg, y.mb, y.w1, y.b1, 4 * C, nullptr, w.ff, 4 * C, N, WdEpi{}, st));
        HIP_TRY(wd_linear<WD_RESID>(w.ff, 4 * C, nullptr, nullptr, y.w2, y.b2, C, w.x, w.x, C, N, WdEpi{}, st));
    }
    return LDS_OK;
}
// the head over N rows of x: the raw logits to `logits` (or nowhere), the tiles' statistics when `stats`
hipError_t wd_head(const lds_whisper_decoder* h, const WdWs& w, const float* x, int N, float* logits, bool stats, int bits, hipStream_t st) {
    const int V = h->cfg.n_vocab;
    WdEpi ep{};
    ep.mask = w.mask; ep.bits = bits; ep.logits = logits; ep.ldl = V; ep.ntiles = (V + kWdCols - 1) / kWdCols;
    if (stats) { ep.pmax = w.pmax; ep.parg = w.parg; ep.psum = w.psum; }
    return wd_linear<WD_HEAD>(x, h->cfg.n_state, h->lg, h->lb, h->head, nullptr, V, nullptr, nullptr, 0, N, ep, st);
}
}  // namespace

extern "C" int lds_whisper_decoder_workspace_bytes(const lds_whisper_decoder* h, int B, int T, int S, size_t* out) {
    return plan_bytes(out, [&] { return wd_check_shape(h, B, T, S); }, [&](Arena& A) { WdWs w; wd_plan(h, A, B, T, S, w); });
}

extern "C" int lds_whisper_decoder_cross(lds_whisper_decoder* h, const float* units, const int32_t* n_frames, int B, int T, void* ws, size_t ws_bytes,
                                         void* stream) {
    const int S = 2;      // the cross part of the plan comes first and does not depend on the positions: the smallest plan has to fit
    LDS_TRY(wd_check_shape(h, B, T, S));
    if (!units || !ws) return set_error(LDS_EINVAL, "whisper decoder: null argument");
    if (n_frames) LDS_TRY(clip_lens_check("n_frames", n_frames, B, 1, T));
    hipStream_t st = (hipStream_t)stream;
    Arena A(ws, ws_bytes);
    WdWs w;
    wd_plan(h, A, B, T, S, w);
    if (!A.ok) return set_error(LDS_ENOMEM, "whisper decoder workspace too small: need %zu bytes", A.used);
    int32_t nf[64];
    for (int b = 0; b < B; ++b) nf[b] = n_frames ? n_frames[b] : T;
    LDS_TRY(upload_clip_ints(nf, B, (int*)w.nfr, st));
    const int C = h->cfg.n_state;
    for (int i = 0; i < h->cfg.n_layer; ++i) {
        WdEpi ep{};
        ep.kc = w.ck[i]; ep.vc = w.cv[i]; ep.nfr = w.nfr; ep.T = T; ep.C = C;
        HIP_TRY(wd_linear<WD_CROSSKV>(units, C, nullptr, nullptr, h->layers[i].wckv, h->layers[i].bckv, 2 * C, nullptr, nullptr, 0, B * T, ep, st));
    }
    return LDS_OK;
}

extern "C" int lds_whisper_decoder_logits(lds_whisper_decoder* h, const int64_t* tokens, const int32_t* tok_len, const int64_t* labels, int B, int S, int T,
                                          float* logits, float* logprobs, int32_t* ranks, float* loss, int32_t* n_counted, void* ws, size_t ws_bytes, void* stream) {
    LDS_TRY(wd_check_shape(h, B, T, S));
    if (!tokens || !ws) return set_error(LDS_EINVAL, "whisper decoder: null argument");
    const bool score = logprobs || ranks || loss || n_counted;
    if (score && (!logprobs || !ranks || !loss || !n_counted)) return set_error(LDS_EINVAL, "whisper decoder: scoring needs logprobs, ranks, loss and n_counted together");
    if (!score && !logits) return set_error(LDS_EINVAL, "whisper decoder: nothing to compute (no logits, no scores)");
    const lds_whisper_decoder_cfg& c = h->cfg;
    hipStream_t st = (hipStream_t)stream;
    Arena A(ws, ws_bytes);
    WdWs w;
    wd_plan(h, A, B, T, S, w);
    if (!A.ok) return set_error(LDS_ENOMEM, "whisper decoder workspace too small: need %zu bytes", A.used);
    const int C = c.n_state, V = c.n_vocab, N = B * S;
    if (!labels) labels = tokens;
    // slots at and beyond a row's length hold id 0: their rows are computed and never counted, and no earlier row's query sees their keys
    hipLaunchKernelGGL(wd_init_kernel, dim3(B), dim3(256), 0, st, tokens, S, tok_len, V, 0, S, w.stok);
    HIP_TRY(hipGetLastError());
    const WdRows rows{nullptr, S, 0, S};
    hipLaunchKernelGGL(wd_embed_kernel, dim3(N), dim3(256), 0, st, (const float*)h->emb, (const float*)h->pe, (const int64_t*)w.stok, rows, V, C, w.x);
    HIP_TRY(hipGetLastError());
    LDS_TRY(wd_layers(h, w, N, rows, S, T, st));
    for (int r0 = 0; r0 < N; r0 += kWdScoreChunk) {
        const int nr = (N - r0 < kWdScoreChunk) ? N - r0 : kWdScoreChunk;
        float* lg = logits ? logits + (size_t)r0 * V : w.chunk;
        HIP_TRY(wd_head(h, w, w.x + (size_t)r0 * C, nr, lg, false, 0, st));
        if (score) HIP_TRY(lm_launch_score_rows(lg, r0, nr, V, S, labels, tok_len, logprobs, ranks, st));
    }
    if (score) HIP_TRY(lm_launch_score_loss(logprobs, ranks, B, S - 1, w.psum_d, w.pcnt, loss, n_counted, st));
    return LDS_OK;
}

extern "C" int lds_whisper_decoder_generate(lds_whisper_decoder* h, const int64_t* prompt, const int32_t* prompt_len, int B, int P, int T, int cap,
                                            const lds_whisper_decode_opts* opts, int64_t* tokens, float* token_logprob, float* sum_logprob, float* logits_out,
                                            int* n_tokens_host, void* ws, size_t ws_bytes, void* stream) {
    if (!opts) return set_error(LDS_EINVAL, "whisper decoder: null options");
    const lds_whisper_decode_opts o = *opts;
    LDS_TRY(wd_check_shape(h, B, T, cap));
    const lds_whisper_decoder_cfg& c = h->cfg;
    const int C = c.n_state, V = c.n_vocab;
    if (o.num_beams != 1) return set_error(LDS_EINVAL, "whisper decoder: beam search is not built (num_beams must be 1, got %d)", o.num_beams);
    if (o.temperature != 0.f) return set_error(LDS_EINVAL, "whisper decoder: sampling and temperature fallback are not built (temperature must be 0)");
    if (o.no_repeat_ngram_size != 0)
        return set_error(LDS_EINVAL, "whisper decoder: no_repeat_ngram_size must be 0 -- the n-gram ban's bit set spans %d columns, not a vocabulary of %d", kLmMaxChoiceVocab, V);
    if (o.max_new_tokens < 1) return set_error(LDS_EINVAL, "whisper decoder: max_new_tokens %d (>= 1)", o.max_new_tokens);
    if (o.eos < 0 || o.eos >= V || o.pad < 0 || o.pad >= V) return set_error(LDS_EINVAL, "whisper decoder: eos %d / pad %d outside the vocabulary of %d", o.eos, o.pad, V);
    if (o.n_suppress < 0 || o.n_begin_suppress < 0 || (o.n_suppress > 0 && !o.suppress) || (o.n_begin_suppress > 0 && !o.begin_suppress))
        return set_error(LDS_EINVAL, "whisper decoder: a suppress list with a count needs its ids");
    if (P < 1 || P >= cap) return set_error(LDS_EINVAL, "whisper decoder: prompt width %d leaves no room below the sequence capacity %d", P, cap);
    if (!prompt || !prompt_len || !tokens || !token_logprob || !n_tokens_host || !ws) return set_error(LDS_EINVAL, "whisper decoder: null argument");
    int Pmax = 0, Pmin = P;
    for (int b = 0; b < B; ++b) {
        const int pl = prompt_len[b];
        if (pl < 1 || pl > P) return set_error(LDS_EINVAL, "whisper decoder: prompt_len[%d] = %d outside 1 .. P = %d", b, pl, P);
        Pmax = pl > Pmax ? pl : Pmax;
        Pmin = pl < Pmin ? pl : Pmin;
    }
    hipStream_t st = (hipStream_t)stream;
    Arena A(ws, ws_bytes);
    WdWs w;
    wd_plan(h, A, B, T, cap, w);
    if (!A.ok) return set_error(LDS_ENOMEM, "whisper decoder workspace too small: need %zu bytes", A.used);
    int* unfinished = w.flags;                  // [B]
    int* any_unf = w.flags + B;                 // [cap]
    int* rowlen = w.flags + B + cap;            // [B <= 64]
    const int max_new = o.max_new_tokens;
    {
        std::vector<int> init(B + cap + kWdMaxBatch, 0), pl(B);
        for (int b = 0; b < B; ++b) { init[b] = 1; init[B + cap + b] = cap; pl[b] = prompt_len[b]; }
        HIP_TRY(hipMemcpyAsync(unfinished, init.data(), sizeof(int) * init.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(w.plen, pl.data(), sizeof(int) * B, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));      // the host staging vectors go out of scope
    }
    HIP_TRY(hipMemsetAsync(token_logprob, 0, sizeof(float) * (size_t)B * max_new, st));
    const unsigned gv = (V + 255) / 256;
    hipLaunchKernelGGL(wd_mask_kernel, dim3(gv), dim3(256), 0, st, w.mask, V, (const int32_t*)nullptr, 0, 0);
    if (o.n_suppress > 0) hipLaunchKernelGGL(wd_mask_kernel, dim3((o.n_suppress + 255) / 256), dim3(256), 0, st, w.mask, V, o.suppress, o.n_suppress, 1);
    if (o.n_begin_suppress > 0)
        hipLaunchKernelGGL(wd_mask_kernel, dim3((o.n_begin_suppress + 255) / 256), dim3(256), 0, st, w.mask, V, o.begin_suppress, o.n_begin_suppress, 2);
    hipLaunchKernelGGL(wd_init_kernel, dim3(B), dim3(256), 0, st, prompt, P, (const int32_t*)w.plen, V, o.pad, cap, w.stok);
    HIP_TRY(hipGetLastError());
    // Prefill: the positions 0 .. Pq - 1 (Pq = the longest prompt - 1) of every row in one causal pass that fills the self caches; no head.  A
    // shorter row's slots prompt_len[b] - 1 .. Pq - 1 are filled from PAD; step s of row b first overwrites slot prompt_len[b] - 1 + s with the
    // row's real token and then reads the slots 0 .. prompt_len[b] - 1 + s.  The same covers the workspace's contents on entry.
    const int Pq = Pmax - 1;
    if (Pq > 0) {
        const WdRows rows{w.plen, Pq, 0, cap};
        hipLaunchKernelGGL(wd_embed_kernel, dim3(B * Pq), dim3(256), 0, st, (const float*)h->emb, (const float*)h->pe, (const int64_t*)w.stok, rows, V, C, w.x);
        HIP_TRY(hipGetLastError());
        LDS_TRY(wd_layers(h, w, B * Pq, rows, Pq, T, st));
    }
    int n_steps = cap - Pmin;      // the shortest row writes its last slot at step n_steps - 1
    n_steps = n_steps < max_new ? n_steps : max_new;
    std::vector<int> host_flags(n_steps, 0);
    int checked = 0;
    for (int step = 0; step < n_steps; ++step) {
        const WdRows rows{w.plen, 0, step, cap};
        hipLaunchKernelGGL(wd_embed_kernel, dim3(B), dim3(256), 0, st, (const float*)h->emb, (const float*)h->pe, (const int64_t*)w.stok, rows, V, C, w.x);
        HIP_TRY(hipGetLastError());
        const int Lk_max = (Pmax + step < cap) ? Pmax + step : cap;
        LDS_TRY(wd_layers(h, w, B, rows, Lk_max, T, st));
        HIP_TRY(wd_head(h, w, w.x, B, logits_out ? logits_out + (size_t)step * B * V : nullptr, true, step == 0 ? 3 : 1, st));
        const WdStep sp{w.stok, w.plen, unfinished, rowlen, token_logprob, step, cap, max_new, o.eos};
        hipLaunchKernelGGL(wd_choose_kernel, dim3(B), dim3(256), 0, st, (const float*)w.pmax, (const int*)w.parg, (const float*)w.psum, (V + kWdCols - 1) / kWdCols,
                           (int64_t*)nullptr, (float*)nullptr, (float*)nullptr, sp, 1);
        hipLaunchKernelGGL(wd_flag_kernel, dim3(1), dim3(64), 0, st, (const int*)unfinished, B, any_unf + step);
        HIP_TRY(hipGetLastError());
        if ((step & 7) == 7 || step + 1 == n_steps) {      // the EOS poll
            HIP_TRY(hipMemcpyAsync(host_flags.data() + checked, any_unf + checked, sizeof(int) * (step + 1 - checked), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            bool done = false;
            for (int s = checked; s <= step && !done; ++s) done = host_flags[s] == 0;
            checked = step + 1;
            if (done) break;
        }
    }
    hipLaunchKernelGGL(wd_finish_kernel, dim3(B), dim3(256), 0, st, (const int64_t*)w.stok, cap, tokens, (const float*)token_logprob, max_new, sum_logprob);
    HIP_TRY(hipGetLastError());
    std::vector<int> len(B, 0);
    HIP_TRY(hipMemcpyAsync(len.data(), rowlen, sizeof(int) * B, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int n_tokens = 0;
    for (int b = 0; b < B; ++b) n_tokens = len[b] > n_tokens ? len[b] : n_tokens;
    *n_tokens_host = n_tokens;
    return LDS_OK;
}

// Test entry (include/lds_test.h): the head alone.  x dev [N][K], ln_g / ln_b dev [K], et dev [K][V] (the embedding transposed), suppress dev
// int32 [n_suppress] or null -> token dev int64 [N], logprob / lse dev [N], logits dev [N][V] or null.  Synchronises.
extern "C" int lds_test_whisper_head(const float* x, const float* ln_g, const float* ln_b, const float* et, int N, int K, int V, const int32_t* suppress,
                                     int n_suppress, int64_t* token, float* logprob, float* lse, float* logits, void* stream) {
    if (!x || !ln_g || !ln_b || !et || !token || !logprob || !lse) return set_error(LDS_EINVAL, "null argument");
    if (N < 1 || N > kWdMaxBatch || K < 32 || K > 8192 || V < 2 || V > kWdMaxVocab || n_suppress < 0 || (n_suppress > 0 && !suppress))
        return set_error(LDS_EINVAL, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int ntiles = (V + kWdCols - 1) / kWdCols;
    const size_t per = ((size_t)N * ntiles * sizeof(float) + 255) & ~(size_t)255, mbytes = ((size_t)V * sizeof(int) + 255) & ~(size_t)255;
    char* dev = nullptr;
    if (hipMalloc((void**)&dev, 3 * per + mbytes) != hipSuccess) return set_error(LDS_ENOMEM, "hipMalloc");
    int rc = LDS_OK;
    WdEpi ep{};
    ep.pmax = (float*)dev; ep.psum = (float*)(dev + per); ep.parg = (int*)(dev + 2 * per);
    int* mask = (int*)(dev + 3 * per);
    ep.mask = mask; ep.bits = 1; ep.logits = logits; ep.ldl = V; ep.ntiles = ntiles;
    hipLaunchKernelGGL(wd_mask_kernel, dim3((V + 255) / 256), dim3(256), 0, st, mask, V, (const int32_t*)nullptr, 0, 0);
    if (n_suppress > 0) hipLaunchKernelGGL(wd_mask_kernel, dim3((n_suppress + 255) / 256), dim3(256), 0, st, mask, V, suppress, n_suppress, 1);
    if (hipGetLastError() != hipSuccess || wd_linear<WD_HEAD>(x, K, ln_g, ln_b, et, nullptr, V, nullptr, nullptr, 0, N, ep, st) != hipSuccess) rc = set_error(LDS_EHIP, "launch");
    if (rc == LDS_OK) {
        hipLaunchKernelGGL(wd_choose_kernel, dim3(N), dim3(256), 0, st, (const float*)ep.pmax, (const int*)ep.parg, (const float*)ep.psum, ntiles, token, logprob, lse,
                           WdStep{}, 0);
        if (hipGetLastError() != hipSuccess) rc = set_error(LDS_EHIP, "launch");
    }
    if (hipStreamSynchronize(st) != hipSuccess) rc = set_error(LDS_EHIP, "sync");
    (void)hipFree(dev);
    return rc;
}
